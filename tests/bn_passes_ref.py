"""Float64 restatement of the BatchNorm / ReLU passes (csrc/bn_passes.hip) and
the seeded inputs of tests/test_gpu_bn_passes.py.  Plain numpy, no GPU, nothing from sonet_hip: tests/test_bn_passes_cpu.py pins this file
to float64 autograd of F.batch_norm, the GPU tests pin the kernels to this file.

Rounding model.  The kernels evaluate every element with f32 fmas: ``fma(x, sc, sh)`` for the forward, ``fma(a, g, fma(b, raw, c0))`` for the
backward apply.  An fma is the exact value rounded once.  Here the exact value is formed in float64 -- the product of two f32 values is exact
in float64, the sum then carries a relative error of at most 2^-53, i.e. at most 2^-29 of the gap between two adjacent f32 values -- and rounded
to f32.  The two agree unless the float64 value lies within that error of the midpoint of two adjacent f32 values.  ``tie_count`` counts the
elements within 2^-28 of the gap (twice the error) of such a midpoint; the CPU test asserts that it is zero for every seeded input, which is what
lets the GPU tests ask for bit equality.  (2^-28 of the VALUE would cover 1/11 of all f32 results: no input satisfies that reading.)
One kind of element is not counted: where the float64 sum was EXACT (its TwoSum residual is zero) the float64 value is the fma's own exact
value, and both sides round it to nearest even -- midpoint or not.  Such exact midpoints cannot be seeded away: a bf16 value times an f32
coefficient has 32 significant bits, so about one result in 2^8 sits exactly on an f32 midpoint.
bf16 storage: the f32 result is rounded to nearest-even bf16, as v_cvt_pk_bf16_f32 does; the same count is taken against bf16 midpoints."""
import math

import numpy as np

U24 = 2.0 ** -24
TIE_MARGIN = 2.0 ** -28                     # of the gap between the two neighbouring representable values
SCALAR_TOL = 1e-12                          # statistics, scalar kernels: every term carried in f64
EPS = 1e-5


def vector_tol(bf16):
    """Statistics, 16-byte kernels: the product is rounded to f32 once and the N = 4 (f32) / 8 (bf16) values of one access are summed
    pairwise in f32 (log2 N roundings) before they are carried in f64: (log2 N + 1) 2^-24 of the sum of the terms' magnitudes."""
    return (math.log2(8 if bf16 else 4) + 1) * U24


# ---------------------------------------------------------------------------------------------- number formats
def to_f32(v64):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v64, np.float64).astype(np.float32)


def bf16_bits(x32):
    """f32 -> bf16 bit patterns (uint16), round to nearest even; NaN -> a quiet NaN."""
    x32 = np.ascontiguousarray(x32, np.float32)
    u = x32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x32), np.uint16(0x7FC0), r)


def bf16_widen(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x32):
    """f32 -> the nearest-even bf16 value, held in f32."""
    return bf16_widen(bf16_bits(x32))


def holds_bf16(x32):
    return bool(((np.ascontiguousarray(x32, np.float32).view(np.uint32) & 0xFFFF) == 0).all())


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def ulp_bf16(x):
    """Gap between the bf16 values around |x| (x float64, normal range)."""
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)


def add64(p, z):
    """p + z in float64 -> (sum, inexact): TwoSum's residual tells whether the sum was rounded."""
    p, z = np.broadcast_arrays(np.asarray(p, np.float64), np.asarray(z, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + z
        bb = s - p
        err = (p - (s - bb)) + (z - bb)
    return s, err != 0


def tie_count(v64, bf16=False, inexact=None):
    """Number of finite elements of the float64 array within TIE_MARGIN * gap of the midpoint of two adjacent f32 (bf16) values;
    ``inexact`` (bool array): only those elements count (see the module's docstring)."""
    v = np.abs(np.asarray(v64, np.float64).ravel())
    keep = np.isfinite(v) if inexact is None else np.isfinite(v) & np.asarray(inexact, bool).ravel()
    v = v[keep]
    r = v.astype(np.float32)
    if bf16:
        t = r.view(np.uint32) & np.uint32(0xFFFF0000)
        lo, hi = t.view(np.float32).astype(np.float64), (t + np.uint32(0x10000)).view(np.float32).astype(np.float64)
    else:
        other = np.where(v >= r.astype(np.float64), np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
        lo, hi = np.minimum(r, other).astype(np.float64), np.maximum(r, other).astype(np.float64)
    gap = hi - lo
    ok = np.isfinite(gap)
    return int((np.abs(v - 0.5 * (lo + hi))[ok] <= TIE_MARGIN * gap[ok]).sum())


# ---------------------------------------------------------------------------------------------- element-wise passes
def _col(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1)


def pre64(x, sc, sh, want_inexact=False):
    """The forward's pre-activation x * sc[c] + sh[c] in float64 (the product of f32 values is exact)."""
    with np.errstate(invalid="ignore", over="ignore"):
        s, inexact = add64(np.asarray(x, np.float64) * _col(sc), _col(sh))
    return (s, inexact) if want_inexact else s


def affine_act(x, sc, sh, relu, bf16=False):
    """y = act(fma(x, sc[c], sh[c])), ``v < 0 ? 0 : v`` (keeps -0.0 and NaN), stored as f32 or as nearest-even bf16 (returned widened)."""
    v = to_f32(pre64(x, sc, sh))
    if relu:
        v = np.where(v < 0, np.float32(0), v)
    return round_bf16(v) if bf16 else v


def mask(raw, sc, sh, relu):
    if not relu:
        return np.ones(np.shape(raw), bool)
    with np.errstate(invalid="ignore"):
        return pre64(raw, sc, sh) > 0                      # NaN: False, as !(fma > 0) masks


def apply64(gy, raw, sc, sh, relu, a, b, c0, exact=False, want_inexact=False):
    """(inner, outer) float64 values in front of the two roundings of the backward apply (exact: the inner value is not rounded)."""
    g = np.where(mask(raw, sc, sh, relu), np.asarray(gy, np.float64), 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        inner, ix_i = add64(_col(b) * np.asarray(raw, np.float64), _col(c0))
        outer, ix_o = add64(_col(a) * g, inner if exact else to_f32(inner).astype(np.float64))
    return (inner, outer, ix_i, ix_o) if want_inexact else (inner, outer)


def bwd_apply(gy, raw, sc, sh, relu, a, b, c0, bf16=False):
    """g_raw = fma(a, gy * mask, fma(b, raw, c0)): two roundings to f32, one more to bf16 for bf16 storage."""
    v = to_f32(apply64(gy, raw, sc, sh, relu, a, b, c0)[1])
    return round_bf16(v) if bf16 else v


# ---------------------------------------------------------------------------------------------- statistics
def _fsum_rows(t):                                          # t [B][C][L] float64 -> [C] exactly rounded sums
    return np.array([math.fsum(t[:, c, :].ravel().tolist()) for c in range(t.shape[1])], np.float64)


def bwd_sums(gy, raw, sc, sh, relu):
    """-> s1 = sum gy*mask, s2 = sum gy*mask*raw (exact: every term is exact in float64, math.fsum rounds the sum once),
    sum |gy*mask|, sum |gy*mask*raw|, all [C]."""
    g = np.where(mask(raw, sc, sh, relu), np.asarray(gy, np.float64), 0.0)
    with np.errstate(invalid="ignore"):
        gr = g * np.asarray(raw, np.float64)
    return _fsum_rows(g), _fsum_rows(gr), _fsum_rows(np.abs(g)), _fsum_rows(np.abs(gr))


def channel_stats(y):
    """-> exact sum x, sum x^2 (= sum |x|^2, the magnitude the sum-of-squares bound scales with), sum |x|, all [C]."""
    y = np.asarray(y, np.float64)
    return _fsum_rows(y), _fsum_rows(y * y), _fsum_rows(np.abs(y))


def mean_var(s, s2, n):
    m = s / n
    return m, s2 / n - m * m


def stats_bounds(s, s2, sabs, n, tol):
    """Bounds of channel_stats' (mean, var) given the relative bound ``tol`` of its two sums.  mean = fl32(S / n): the sum's error over n
    plus one f32 rounding.  var = fl32(S2 / n - m^2): d(S2) / n + (2 |m| + d(S) / n) d(S) / n, the float64 evaluation (three operations on
    values of size S2 / n: 4 2^-53 S2 / n) and one f32 rounding."""
    m, v = mean_var(s, s2, n)
    d1, d2 = tol * sabs / n, tol * s2 / n
    bm = d1 + U24 * np.abs(m)
    dv = d2 + (2 * np.abs(m) + d1) * d1 + 4 * 2.0 ** -53 * (s2 / n)
    return bm, dv + U24 * (np.abs(v) + dv)


# ---------------------------------------------------------------------------------------------- per-channel coefficients
def fwd_coeffs(mean, var, gamma, beta, eps):
    """invstd = (var + eps)^-1/2, scale = gamma invstd, shift = beta - mean scale."""
    mean, var, gamma, beta = (np.asarray(t, np.float64) for t in (mean, var, gamma, beta))
    invstd = 1.0 / np.sqrt(var + float(eps))
    scale = gamma * invstd
    return invstd, scale, beta - mean * scale


def bwd_coeffs(s1, s2, mean, invstd, gamma, n):
    """sg = invstd (s2 - mean s1), a = gamma invstd, b = -a invstd sg / n, c0 = -a s1 / n - b mean -> (a, b, c0, g_gamma = sg, g_beta = s1)."""
    s1, s2, mean, invstd, gamma = (np.asarray(t, np.float64) for t in (s1, s2, mean, invstd, gamma))
    sg = invstd * (s2 - mean * s1)
    a = gamma * invstd
    b = -a * invstd * sg / n
    return a, b, -a * s1 / n - b * mean, sg, s1


def running_update(rmean, rvar, mean, var, momentum, unbias):
    """F.batch_norm's update: r (1 - m) + m stat, the variance entering unbiased."""
    rmean, rvar, mean, var = (np.asarray(t, np.float64) for t in (rmean, rvar, mean, var))
    return rmean * (1.0 - momentum) + momentum * mean, rvar * (1.0 - momentum) + momentum * (var * unbias)


def running_update_f32(rmean, rvar, mean, var, momentum, unbias, want64=False):
    """The kernel's f32 evaluation: fma(stat, m, fl(r fl(1 - m))) with stat = mean resp. fl(var unbias).  Products of two f32 values are exact
    in float64, so every step but the fma's sum is emulated exactly (the sum: see ``tie_count``)."""
    f = lambda t: np.asarray(t, np.float32).astype(np.float64)
    m = float(np.float32(momentum))
    omm = float(np.float32(1.0 - m))
    vu = to_f32(f(var) * float(np.float32(unbias))).astype(np.float64)
    pre_m = f(mean) * m + to_f32(f(rmean) * omm).astype(np.float64)
    pre_v = vu * m + to_f32(f(rvar) * omm).astype(np.float64)
    if want64:
        return add64(f(mean) * m, pre_m - f(mean) * m), add64(vu * m, pre_v - vu * m)
    return to_f32(pre_m), to_f32(pre_v)


# ---------------------------------------------------------------------------------------------- seeded inputs
class Case:
    """One input of the GPU tests.  ``k``: element offset of the operands in a larger flat buffer (0: the allocation itself)."""

    def __init__(self, dt, B, C, L, k, path, seed=0):
        self.dt, self.B, self.C, self.L, self.k, self.path, self.seed = dt, B, C, L, k, path, seed
        self.bf16 = dt == "bf16"
        self.id = "%s-B%d-C%d-L%d-k%d" % (dt, B, C, L, k)

    def rng(self, salt=0):
        # (the string hash of Python is salted per process: a fixed arithmetic key instead)
        return np.random.default_rng([self.seed, salt, self.bf16, self.B, self.C, self.L, self.k])


def _store(v, bf16):
    v = np.asarray(v, np.float32)
    return round_bf16(v) if bf16 else v


# Element-wise passes.  Dispatch (bn_passes.hip): 16 bytes per lane when L * elem_bytes % 16 == 0 and every pointer is 16-byte aligned
# (rowwise_vec_kernel; gridDim.y = ceil(Lv / 1024), Lv = L / 4 resp. L / 8); bf16 otherwise: dword pairs when L is even and the pointers
# 4-byte aligned (rowwise_kernel<., uint16_t, true>), else one element per lane (<., uint16_t, false>), gridDim.y = ceil(L / 2048); f32
# otherwise: rowwise_kernel<., float, false>, gridDim.y = ceil(L / 2048).  channel_affine_act_ (in place, f32) is always the flat
# channel_affine_act_kernel.  A grid row strides by 256 * gridDim.y lanes.
def _elementwise_cases():
    cs = []
    for B, C in ((3, 5), (1, 1)):
        cs += [Case("f32", B, C, 1, 0, "scalar"), Case("f32", B, C, 2, 0, "scalar"), Case("f32", B, C, 7, 0, "scalar"),
               Case("f32", B, C, 8, 0, "vec, Lv = 2"), Case("f32", B, C, 1023, 0, "scalar, 4 strides of 256"),
               Case("f32", B, C, 1030, 0, "scalar: 4120 bytes per row, not a multiple of 16"),
               Case("bf16", B, C, 1, 0, "scalar"), Case("bf16", B, C, 2, 0, "pair, Lv = 1"), Case("bf16", B, C, 7, 0, "scalar"),
               Case("bf16", B, C, 8, 0, "vec, Lv = 1"), Case("bf16", B, C, 1023, 0, "scalar, 4 strides"),
               Case("bf16", B, C, 1030, 0, "pair: 2060 bytes per row; Lv = 515, 3 strides")]
    cs += [Case("f32", 1, 5, 8, 0, "vec"), Case("f32", 3, 1, 7, 0, "scalar"), Case("bf16", 1, 5, 2, 0, "pair"), Case("bf16", 3, 1, 8, 0, "vec"),
           Case("f32", 3, 5, 1028, 0, "vec, Lv = 257: a second stride of one lane"),
           Case("bf16", 3, 5, 2056, 0, "vec, Lv = 257: a second stride of one lane"),
           Case("f32", 3, 5, 4100, 0, "vec, Lv = 1025 > 1024: gridDim.y = 2, the second y block holds one lane"),
           Case("f32", 1, 5, 2051, 0, "scalar, gridDim.y = 2 with a 3-element tail"),
           Case("bf16", 3, 5, 8200, 0, "vec, Lv = 1025 > 1024: gridDim.y = 2"),
           Case("bf16", 1, 5, 8202, 0, "pair, gridDim.y = 5, Lv = 4101: the fourth stride holds 5 lanes"),
           Case("bf16", 1, 5, 2049, 0, "scalar, gridDim.y = 2 with a one-element tail"),
           Case("f32", 3, 5, 8, 1, "scalar: 4-byte aligned view of a shape that is vec when aligned"),
           Case("f32", 1, 5, 4100, 1, "scalar, gridDim.y = 3: misaligned view"),
           Case("bf16", 3, 5, 8, 1, "scalar: 2-byte aligned view"),
           Case("bf16", 3, 5, 8, 2, "pair: 4-byte aligned view of a shape that is vec when aligned"),
           Case("bf16", 1, 5, 8200, 2, "pair, gridDim.y = 5: 4-byte aligned view"),
           Case("bf16", 1, 5, 1030, 1, "scalar: 2-byte aligned view of a pair shape")]
    return cs


ELEMENTWISE = _elementwise_cases()


def elementwise_inputs(case):
    """-> dict of f32 arrays (bf16 cases: holding bf16 values): raw, gy [B][C][L]; sc, sh, a, b, c0 [C]."""
    g = case.rng(1)
    B, C, L = case.B, case.C, case.L
    raw = _store(g.standard_normal((B, C, L)) * 1.5 + g.standard_normal((1, C, 1)), case.bf16)
    gy = _store(g.standard_normal((B, C, L)) * 1e-2, case.bf16)
    f = lambda v: np.asarray(v, np.float32)
    return dict(raw=raw, gy=gy, sc=f(g.random(C) + 0.5) * f(g.choice([-1.0, 1.0], C, p=[0.2, 0.8])), sh=f(g.standard_normal(C) * 0.4),
                a=f(g.random(C) + 0.5), b=f(g.standard_normal(C) * 1e-3), c0=f(g.standard_normal(C) * 1e-3))


# Mask edge.  Channel 0: sc = 1, sh = -raw[0][0][l0]: the pre-activation is exactly +0.  Channel 1: sc = 1, sh = -0.0 with raw = -0.0: -0.0.
# Channel 2: sc = 1, sh = -2^-149 with raw = 0: the nearest f32 below 0.  Channel 3: sc = 1, sh = +2^-149 with raw = 0: the nearest above 0.
# Channel 4: ordinary.  The first three must store a zero and mask the gradient, the fourth must do neither (bf16 storage rounds its forward
# value 2^-149 to zero: there only the mask tells).  One shape per kernel flavour.
MASK_EDGE = [Case("f32", 3, 5, 8, 0, "vec", 7), Case("f32", 3, 5, 7, 0, "scalar", 7), Case("bf16", 3, 5, 8, 0, "vec", 7),
             Case("bf16", 3, 5, 6, 0, "pair", 7), Case("bf16", 3, 5, 7, 0, "scalar", 7)]
TINY = float(np.float32(2.0 ** -149))


def mask_edge_inputs(case):
    d = elementwise_inputs(case)
    l0 = case.L - 1                                         # (the last column: also the tail of the row)
    d["sc"][:4] = 1.0
    d["sh"][0] = -d["raw"][0, 0, l0]
    d["sh"][1], d["raw"][1, 1, l0] = -0.0, -0.0
    d["sh"][2], d["raw"][2, 2, l0] = -TINY, 0.0
    d["sh"][3], d["raw"][0, 3, l0] = TINY, 0.0
    d["gy"][:, :, l0] = _store(np.float32(0.75), case.bf16)
    d["planted"] = [(0, 0, l0, True), (1, 1, l0, True), (2, 2, l0, True), (0, 3, l0, False)]      # (b, c, l, masked)
    return d


def nan_inputs(case):
    """``elementwise_inputs`` with one NaN in raw (cloud 1, channel 2, mid row)."""
    d = elementwise_inputs(case)
    d["at"] = (1, 2, case.L // 2)
    d["raw"][d["at"]] = np.nan
    return d


# Statistics.  pointwise_bwd_stats f32: stats_vec_kernel<false> when L % 4 == 0 and aligned, else stats_scalar_kernel<float, false, .> (chunks =
# ceil(B L / 16384) of a flat (b, l) index per channel).  bf16 (and channel_stats bf16): stats_vec_kernel<true> when L % 8 == 0 and aligned, else
# stats_scalar_kernel<uint16_t, true, .> (L even, 4-byte aligned; Lv = L / 2) or <uint16_t, false, .>.  channel_stats f32 is always the scalar kernel.
# stats_vec_kernel: seg = min(8, ceil(Lv / 1024)) segments per row; 8 clouds per workgroup once seg * C * ceil(B / 8) >= 2048.
def _stats_cases():
    cs = []
    for L in (1, 2, 7, 8, 1023, 1030):
        cs += [Case("f32", 3, 5, L, 0, "vec" if L % 4 == 0 else "scalar"),
               Case("bf16", 3, 5, L, 0, "vec" if L % 8 == 0 else "pair" if L % 2 == 0 else "scalar")]
    cs += [Case("f32", 1, 1, 7, 0, "scalar"), Case("bf16", 1, 1, 2, 0, "pair"),
           Case("f32", 3, 5, 8, 1, "scalar: 4-byte aligned view"), Case("bf16", 3, 5, 8, 1, "scalar: 2-byte aligned view"),
           Case("bf16", 3, 5, 8, 2, "pair: 4-byte aligned view"),
           Case("f32", 3, 5, 5463, 0, "scalar, B L = 16389: 2 chunks of 8195, the first ends inside cloud 1"),
           Case("bf16", 3, 5, 5463, 0, "scalar, 2 chunks of 8195"),
           Case("bf16", 3, 5, 5462, 2, "pair, Lv = 2731, B Lv = 8193: 2 chunks of 4097 dwords, the first ends inside cloud 1"),
           Case("f32", 9, 1024, 8, 0, "vec grouped: 1 * 1024 * ceil(9 / 8) = 2048, 2 groups, the last holds one cloud"),
           Case("bf16", 9, 1024, 8, 0, "vec grouped, 2 groups, the last holds one cloud"),
           Case("f32", 17, 1024, 8, 0, "vec grouped, 3 groups, the last holds one cloud"),
           Case("bf16", 17, 1024, 8, 0, "vec grouped, 3 groups, the last holds one cloud"),
           Case("f32", 3, 5, 4100, 0, "vec ungrouped, Lv = 1025: 2 segments, the second holds one lane per cloud"),
           Case("bf16", 3, 5, 8200, 0, "vec ungrouped, Lv = 1025: 2 segments")]
    return cs


STATS = _stats_cases()


def stats_tol(case, op):
    """Relative bound of a sum for ``op`` in ('bwd', 'channel').  channel_stats f32 has no vector kernel."""
    if case.path.startswith("vec") and not (op == "channel" and not case.bf16):
        return vector_tol(case.bf16)
    return SCALAR_TOL


def stats_inputs(case):
    """raw, gy, sc, sh as ``elementwise_inputs``; y for channel_stats: channel 0 has its mean at 1000 sigma (f32) / 8 sigma (bf16), the last
    channel (C > 1) is constant."""
    d = elementwise_inputs(case)
    g = case.rng(2)
    y = g.standard_normal((case.B, case.C, case.L)) * (g.random((1, case.C, 1)) + 0.5) + g.standard_normal((1, case.C, 1))
    y[:, 0, :] = g.standard_normal((case.B, case.L)) + (8.0 if case.bf16 else 1000.0)
    if case.C > 1:
        y[:, case.C - 1, :] = -3.25
    d["y"] = _store(y, case.bf16)
    return d


# A constant channel at a power-of-two count: n c and n c^2 are exact in f64 (and the f32 partial sums of the 16-byte kernel: 8 c = -26,
# 8 c^2 = 84.5), 1 / n is exact, so mean = c and E[x^2] - mean^2 = 0 exactly on every path.  (At other counts fl(1 / n) n != 1 leaves
# a residue of a few 2^-53 c^2 of either sign: there the clamp guarantees only var >= 0, which the general cases assert.)
CONSTANT = [Case("f32", 1, 2, 1, 0, "scalar"), Case("f32", 2, 2, 512, 0, "scalar"), Case("bf16", 1, 2, 8, 1, "scalar: 2-byte aligned view"),
            Case("bf16", 1, 2, 8, 2, "pair: 4-byte aligned view"), Case("bf16", 1, 2, 8, 0, "vec"), Case("bf16", 2, 2, 1024, 0, "vec")]


# The composed backward: one 16-byte and one fallback shape per dtype, gy ~2 % dense as below a max pool.
COMPOSED = [Case("f32", 3, 6, 1028, 0, "vec", 11), Case("f32", 3, 6, 1031, 0, "scalar", 11),
            Case("bf16", 3, 6, 1032, 0, "vec", 11), Case("bf16", 3, 6, 1030, 0, "pair", 11), Case("bf16", 3, 6, 1031, 0, "scalar", 11)]


def composed_inputs(case):
    g = case.rng(3)
    B, C, L = case.B, case.C, case.L
    raw = _store(g.standard_normal((B, C, L)) * (g.random((1, C, 1)) + 0.5) + 0.5 * g.standard_normal((1, C, 1)), case.bf16)
    gy = _store(g.standard_normal((B, C, L)) * (g.random((B, C, L)) < 0.02), case.bf16)
    f = lambda v: np.asarray(v, np.float32)
    return dict(raw=raw, gy=gy, gamma=f(g.random(C) + 0.5), beta=f(g.standard_normal(C) * 0.3))


def chain(raw, gy, gamma, beta, relu, bf16=False, eps=EPS):
    """The restatement chained as the training step chains the passes: statistics -> forward coefficients -> backward sums -> backward
    coefficients -> apply, the per-channel vectors rounded to f32 where the kernels store f32.  -> g_raw (f32 values), g_gamma, g_beta."""
    n = raw.shape[0] * raw.shape[2]
    s, s2, _ = channel_stats(raw)
    m, v = mean_var(s, s2, n)
    mean, var = to_f32(m), to_f32(np.maximum(v, 0.0))
    invstd, sc, sh = (to_f32(t) for t in fwd_coeffs(mean, var, gamma, beta, float(np.float32(eps))))
    s1, s2b, _, _ = bwd_sums(gy, raw, sc, sh, relu)
    a, b, c0, gg, gb = (to_f32(t) for t in bwd_coeffs(s1, s2b, mean, invstd, gamma, float(n)))
    return bwd_apply(gy, raw, sc, sh, relu, a, b, c0, bf16), gg, gb


# Coefficient kernels: C around the 256-thread block edge.
COEFF_C = (1, 255, 257)


def coeff_inputs(C, seed=5):
    """mean, var, gamma, beta (f32); channel 0 has var = 0, channel C - 1 a large variance, channel C // 2 a mean far above 1 / invstd."""
    g = np.random.default_rng([seed, C])
    f = lambda v: np.asarray(v, np.float32)
    mean, var = f(g.standard_normal(C)), f(g.random(C) * 2 + 0.05)
    var[0] = 0.0
    var[C - 1] = 3.0e7
    mean[C // 2] = 4096.0 if C > 1 else mean[0]
    d = dict(mean=mean, var=var, gamma=f(g.random(C) + 0.5), beta=f(g.standard_normal(C) * 0.3), n=3 * 1031.0)
    d["s1"], d["s2"] = g.standard_normal(C) * 5.0, g.standard_normal(C) * 40.0 + mean.astype(np.float64) * 3.0
    return d


def running_inputs(C, momentum, seed=6):
    """A batch x [2][C][4] of small dyadic values -- its mean and biased variance are exact in f32, n = 8 is small (unbias = 8 / 7) -- and
    running buffers of the mean's sign (no cancellation in r (1 - m) + m stat: an ulp of the result is an ulp of its terms)."""
    g = np.random.default_rng([seed, C, int(momentum * 1000)])
    x = g.integers(-8, 9, (2, C, 4)).astype(np.float64) / 4.0
    x[:, :, 0] += 0.25 * (x.std(axis=(0, 2), keepdims=True)[:, :, 0] == 0)          # (no constant channel: var > 0)
    mean, var = x.mean(axis=(0, 2)), x.var(axis=(0, 2))
    sign = np.where(mean < 0, -1.0, 1.0)
    f = lambda v: np.asarray(v, np.float32)
    assert (f(mean) == mean).all() and (f(var) == var).all()
    return dict(x=x, mean=f(mean), var=f(var), rmean=f(sign * (g.random(C) + 0.5)), rvar=f(g.random(C) + 0.5),
                momentum=float(np.float32(momentum)), unbias=8.0 / 7.0)
