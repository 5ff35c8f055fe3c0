"""Host restatement of the bf16-split ("x3") arithmetic, the operand families its tests walk, and the gates they apply.

The split, piece by piece as the kernels form it (csrc/pointmlp_x3.hip ``split3_pair`` / ``x3_pack_body``, csrc/wgrad_x3.hip
``wg_split3_pair``): h = bf16(v), m = bf16(v - h), l = bf16((v - h) - m), round-to-nearest-even at each level, residuals in float32; the
six kept products
      W.x ~= Wh.xh + Wh.xm + Wm.xh + Wh.xl + Wl.xh + Wm.xm
summed in float64: what comes out is the error of the ARITHMETIC alone, without the matrix cores' f32 accumulation.

Whether v_mfma_f32_32x32x16_bf16 keeps or flushes subnormal bf16 operands has not been measured: ``split3`` carries both cases (with
``flush`` every f32 / bf16 value below 2^-126 is a signed zero) and ``model_error`` reports the worse of the two.

``derived_interval`` finds, not states, the range of operand magnitudes over which the model stays within CAP = 0.5e-5 (the h3 envelope's
condition: half of the project's 1e-5 is left to the kernels' accumulation).  The families and the gates below are shared by
tests/test_x3_envelope_cpu.py (the model, and deliberately broken models, through the gates) and tests/test_gpu_x3_envelope.py (the kernels).
"""
import functools

import numpy as np

try:                                   # (many BLAS threads on matrices this small cost a hundred times the product itself)
    from threadpoolctl import ThreadpoolController
except ImportError:
    ThreadpoolController = None
_BLAS = []


def _mm(a, b):
    if ThreadpoolController is None:
        return a @ b
    if not _BLAS:
        _BLAS.append(ThreadpoolController())
    with _BLAS[0].limit(limits=1, user_api="blas"):
        return a @ b

CAP = 0.5e-5
COUT, L = 64, 2048                     # the CPU tests' shape: two 32-row output tiles, 2048 columns
KS = (6, 64, 387, 768)                 # a K tail inside one chunk, whole chunks, two panels (384 + 3), the widest shipped layer
TERMS = ("WhXh", "WhXm", "WmXh", "WhXl", "WlXh", "WmXm")
DROPPABLE = TERMS[1:]                  # the five products below the leading one
TINY = 2.0 ** -126                     # smallest normal f32 / bf16 magnitude
BF16_OVERFLOW_BITS = 0x7F7F8000        # smallest finite f32 whose bf16 rounding is inf (about 3.3895e38)


# ---- the split -----------------------------------------------------------------------------------------------------------------------
def _flush(v):
    v = np.array(v, dtype=np.float32)
    v[np.abs(v) < np.float32(TINY)] *= np.float32(0.0)          # (keeps the sign: a flushed value is a signed zero)
    return v


def bf16(v, flush=False):
    """float32 array -> its bf16 rounding (nearest, ties to even; overflow to inf; NaN stays NaN), returned as float32."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if flush:
        v = _flush(v)
    u = v.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(v), (v.view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), r).astype(np.uint32)
    out = r.view(np.float32).reshape(v.shape)
    return _flush(out) if flush else out


def split3(v, flush=False):
    """-> (h, m, l) float32 arrays, each a bf16 value: the three pieces of v as the kernels form them."""
    v = np.asarray(v, dtype=np.float32)
    if flush:
        v = _flush(v)
    with np.errstate(invalid="ignore"):
        h = bf16(v, flush)
        r = v - h
        if flush:
            r = _flush(r)
        m = bf16(r, flush)
        q = r - m
        if flush:
            q = _flush(q)
        l = bf16(q, flush)
    return h, m, l


def _sum_terms(Wp, xp, terms):
    """Sum of the named products of pieces in float64 (the x pieces that meet one W piece are added first: exact in float64)."""
    out = 0.0
    for wi, wn in enumerate("hml"):
        xs = [xp["hml".index(t[3])] for t in terms if t[1] == wn]
        if xs:
            out = out + _mm(Wp[wi].astype(np.float64), sum(p.astype(np.float64) for p in xs))
    return out


def model(W, x, flush=False, terms=TERMS):
    """The arithmetic's result for W [Cout][K] . x [K][N] (float32 operands) -> float64 [Cout][N]."""
    return _sum_terms(split3(W, flush), split3(x, flush), terms)


def model_without(term):
    """-> f(W, x): the model with one of the DROPPABLE products missing (what a kernel with a wrong or absent piece computes)."""
    assert term in DROPPABLE
    return lambda W, x, flush=False: model(W, x, flush, tuple(t for t in TERMS if t != term))


def _swap_pairs(a, axis):
    a = np.array(a)
    n = a.shape[axis] // 2 * 2
    idx = np.arange(a.shape[axis])
    idx[0:n:2], idx[1:n:2] = np.arange(1, n, 2), np.arange(0, n, 2)
    return np.take(a, idx, axis=axis)


def model_swapped_l(which="x"):
    """-> f(W, x): the model with the l pieces of each packed channel pair (2p, 2p + 1) exchanged in one operand -- the halves of the
    third ``v_cvt_pk_bf16_f32`` the wrong way round."""
    def f(W, x, flush=False):
        Wp, xp = list(split3(W, flush)), list(split3(x, flush))
        if which == "x":
            xp[2] = _swap_pairs(xp[2], 0)
        else:
            Wp[2] = _swap_pairs(Wp[2], 1)
        return _sum_terms(Wp, xp, TERMS)
    return f


def exact(W, x):
    return _mm(np.asarray(W, dtype=np.float64), np.asarray(x, dtype=np.float64))


# ---- metrics -------------------------------------------------------------------------------------------------------------------------
def rms_error(got, ref):
    """max |got - ref| / max(|ref|, rms(ref)): the figure conftest.assert_close_rms bounds."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    return float((np.abs(got - ref) / np.maximum(np.maximum(np.abs(ref), rms), 1e-300)).max())


def column_error(got, ref):
    """The same figure with every COLUMN judged against its own rms (rows = output channels).  Stricter than a 32-column tile's rms: a
    column is never judged against a larger neighbour."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = np.sqrt(np.mean(ref ** 2, axis=0, keepdims=True))
    return float((np.abs(got - ref) / np.maximum(np.maximum(np.abs(ref), rms), 1e-300)).max())


def error(got, ref, metric="all"):
    return column_error(got, ref) if metric == "column" else rms_error(got, ref)


def model_error(W, x, metric="all", f=model):
    """The worse of the subnormals-kept and subnormals-flushed model errors against float64."""
    ref = exact(W, x)
    return max(error(f(W, x, flush), ref, metric) for flush in (False, True))


def tight_gate(e_x3, e_f32, e_model):
    """The gate that sees a wrong low-order piece: the bf16 split may be 4 x as far from float64 as an f32 GEMM of the same operands (the
    factor tests/test_gpu_round2.py::test_wgrad_x3_vs_float64 grants) plus the arithmetic's own error."""
    return e_x3 <= 4.0 * e_f32 + e_model


# ---- seeded operands -----------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=64)
def _base(K, cout, n):
    """x ~ N(0, 1) [K][n], W ~ N(0, 2 / K) [cout][K]: one draw per shape, read-only."""
    rng = np.random.default_rng(_seed("x3", K, cout, n))
    x = rng.standard_normal((K, n)).astype(np.float32)
    W = (rng.standard_normal((cout, K)) * (2.0 / K) ** 0.5).astype(np.float32)
    x.setflags(write=False)
    W.setflags(write=False)
    return x, W


def _ldexp(a, e):
    return np.ldexp(a, np.asarray(e, dtype=np.int32)).astype(np.float32)


def uniform_scales(lo):
    return ((0, 0), (lo, 0), (0, lo), (100, 0), (0, 100), (60, 60), (-50, -50), (100, -100), (-20, 0))


def family_names(lo):
    return ["u(%d,%d)" % ab for ab in uniform_scales(lo)] + ["perchannel", "percolumn", "dgrad", "wgrad", "sparse"]


TIGHT_FAMILIES = ("u(0,0)", "perchannel", "dgrad", "wgrad")


def family(name, K, cout=COUT, n=L):
    """-> (W [cout][K], x [K][n], metric).  Every family keeps the float64 product well conditioned (random signs, or scalings that cancel
    in the product), so that a failure is the arithmetic's."""
    x, W = _base(K, cout, n)
    rng = np.random.default_rng(_seed(name, K, cout, n))
    metric = "all"
    if name.startswith("u("):
        a, b = (int(t) for t in name[2:-1].split(","))
        x, W = _ldexp(x, a), _ldexp(W, b)
    elif name == "perchannel":
        # input channel c times 2^e, its weight column times 2^-e: every channel contributes equally (BatchNorm-folded weights)
        e = rng.integers(-40, 41, size=K)
        x, W = _ldexp(x, e[:, None]), _ldexp(W, -e[None, :])
    elif name == "percolumn":
        x, metric = _ldexp(x, rng.integers(-40, 41, size=n)[None, :]), "column"
    elif name == "dgrad":
        # gradients from 1e-12 to 1e-7 per channel against weights ~1
        s = 10.0 ** rng.uniform(-12.0, -7.0, size=K)
        x = (x.astype(np.float64) * s[:, None]).astype(np.float32)
        W = rng.standard_normal((cout, K)).astype(np.float32)
    elif name == "wgrad":
        # the weight gradient's operands with K as the reduction axis: g ~ 1e-10 (1 + 10 u_o) in W's place, activations ~1e3
        W = (rng.standard_normal((cout, K)) * 1e-10 * (1.0 + 10.0 * rng.random((cout, 1)))).astype(np.float32)
        x = (x.astype(np.float64) * 1e3).astype(np.float32)
    elif name == "sparse":
        # post-ReLU: 90 % exact zeros, -0.0 among them, every seventh column all zero
        keep = rng.random((K, n)) < 0.1
        x = np.where(keep, np.abs(x), np.float32(0.0)).astype(np.float32)
        x[:, ::7] = 0.0
        x[(~keep) & (rng.random((K, n)) < 0.25)] = np.float32(-0.0)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(W), np.ascontiguousarray(x), metric


def zero_columns(x):
    return np.flatnonzero((x == 0).all(axis=0))


def wgrad_operands(kind, B, Cout, Cin, Lc):
    """-> (g [B][Cout][Lc], x [B][Cin][Lc]) for the weight-gradient kernels: "plain" (gradients ~1e-4, activations ~1: what the existing
    test feeds), "gradlike" (g ~ 1e-10 (1 + 10 u_o), x ~ 1e3), "relu" (one-signed activations, 60 % zeros), "balanced" ("plain" with column l
    of g times 2^e_l and of x times 2^-e_l, e_l in [-40, 40]: the per-channel family along THIS product's reduction axis)."""
    rng = np.random.default_rng(_seed("wg", kind, B, Cout, Cin, Lc))
    g = rng.standard_normal((B, Cout, Lc))
    x = rng.standard_normal((B, Cin, Lc))
    if kind in ("plain", "balanced"):
        g *= 1e-4 * (1.0 + 10.0 * rng.random((1, Cout, 1)))
        x *= 0.1 + rng.random((1, Cin, 1))
        if kind == "balanced":
            e = rng.integers(-40, 41, size=(B, 1, Lc))
            return _ldexp(g.astype(np.float32), e), _ldexp(x.astype(np.float32), -e)
    elif kind == "gradlike":
        g *= 1e-10 * (1.0 + 10.0 * rng.random((1, Cout, 1)))
        x *= 1e3
    elif kind == "relu":
        g = 1e-4 * (g + 0.3)
        x = np.maximum(x - 0.25, 0.0)
    else:
        raise ValueError(kind)
    return g.astype(np.float32), x.astype(np.float32)


# ---- piece identities ----------------------------------------------------------------------------------------------------------------
def bits22(a):
    """float32 array with the low two bits of every 24-bit significand cleared: h + m + l of such a value is exact in f32 in any order."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFFFFFC)).view(np.float32).reshape(a.shape)


def bits12(a):
    """float32 array cut to 12 significant bits: h (8 bits) + m, no l, and the product of two such values is exact in f32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32).reshape(a.shape)


INDEX_MAPS = ("fwd", "rev", "tail")


def index_map(kind, count, K):
    """Channel per output row / column i = 0 .. count - 1.  "fwd" walks the channels upwards from 0, "rev" downwards from the last one (the
    K tail, the second panel), "tail" gives EVERY 32-wide tile the last 32 channels.  32 consecutive channels hold every position of a
    16-channel chunk in both lane halves."""
    i = np.arange(count)
    if kind == "fwd":
        return i % K
    if kind == "rev":
        return (K - 1 - i) % K
    if kind == "tail":
        return (K - 1 - (i % 32)) % K
    raise ValueError(kind)


def identity_case(which, kind, K, cout, n):
    """-> (W [cout][K], x [K][n], expect [cout][n] float32), the output required BIT FOR BIT.
    which "x": W one-hot rows 2^a at channel c(o), x of 22-bit significands: y[o][j] = 2^a x[c(o)][j] -- the three x pieces against Wh.
    which "W": x one-hot columns 2^a at channel c(j), W of 22-bit significands: y[o][j] = 2^a W[o][c(j)] -- the three W pieces against xh.
    which "mm": W one-hot rows with a 12-bit value w at channel c(o), x of 12-bit significands: both have h and m pieces and no l, the four
    products Wh.xh + Wh.xm + Wm.xh + Wm.xm and every partial sum of them fit 24 bits: y[o][j] = w x[c(o)][j], exact -- Wm.xm among them."""
    rng = np.random.default_rng(_seed("id", which, kind, K, cout, n))
    if which == "mm":
        c = index_map(kind, cout, K)
        W = np.zeros((cout, K), dtype=np.float32)
        W[np.arange(cout), c] = bits12((rng.uniform(0.5, 2.0, size=cout) * np.where(rng.random(cout) < 0.5, -1.0, 1.0)).astype(np.float32))
        x = bits12(rng.standard_normal((K, n)).astype(np.float32) + np.float32(0.001))
        prod = W[np.arange(cout), c].astype(np.float64)[:, None] * x[c, :].astype(np.float64)
        expect = prod.astype(np.float32)
        assert (expect.astype(np.float64) == prod).all()
    elif which == "x":
        c = index_map(kind, cout, K)
        a = rng.integers(-3, 4, size=cout)
        W = np.zeros((cout, K), dtype=np.float32)
        W[np.arange(cout), c] = np.ldexp(np.float32(1.0), a)
        x = bits22(rng.standard_normal((K, n)).astype(np.float32) + np.float32(0.001))
        expect = _ldexp(x[c, :], a[:, None])
    else:
        c = index_map(kind, n, K)
        a = rng.integers(-3, 4, size=n)
        x = np.zeros((K, n), dtype=np.float32)
        x[c, np.arange(n)] = np.ldexp(np.float32(1.0), a)
        W = bits22((rng.standard_normal((cout, K)) * (2.0 / K) ** 0.5).astype(np.float32) + np.float32(0.001))
        expect = _ldexp(W[:, c], a[None, :])
    return W, x, expect


def identities(K, cout, n):
    for which in ("x", "W", "mm"):
        for kind in INDEX_MAPS:
            yield ("id-%s-%s" % (which, kind),) + identity_case(which, kind, K, cout, n)


# ---- the interval --------------------------------------------------------------------------------------------------------------------
def scale_fits(K, a, b, cout=COUT, n=L):
    """x . 2^a, W . 2^b: every element has a finite bf16 rounding and every partial sum fits f32 (sum |w||x| below 2^127)."""
    W, x, _ = family("u(%d,%d)" % (a, b), K, cout, n)
    with np.errstate(over="ignore"):
        big = float(_mm(np.abs(W).astype(np.float64), np.abs(x).astype(np.float64)).max())
    return bool(big < 2.0 ** 127 and np.isfinite(bf16(x)).all() and np.isfinite(bf16(W)).all())


def scale_ok(K, a, b, cout=COUT, n=L):
    """... and the model holds CAP there."""
    if not scale_fits(K, a, b, cout, n):
        return False
    W, x, _ = family("u(%d,%d)" % (a, b), K, cout, n)
    return model_error(W, x) <= CAP


def end_ok(e, test=scale_ok):
    return all(test(K, e, 0) and test(K, 0, e) for K in reversed(KS))


def _bisect(good, bad, ok):
    while abs(good - bad) > 2:
        mid = (good + bad) // 4 * 2
        good, bad = (mid, bad) if ok(mid) else (good, mid)
    return good


@functools.lru_cache(maxsize=1)
def derived_interval():
    """-> (lo, hi): the even exponents (powers of four) furthest from 0 at which an operand scaled by 2^e -- x or W, the other ~1 -- still
    meets CAP at every K of KS with subnormals kept and flushed.  Found by bisection between 2^+-60, where the model sits on its 4e-8 floor,
    and the ends of the f32 range.  Downwards the error grows monotonically once pieces begin to fall below 2^-126.  Upwards a scaling by a
    power of two changes nothing until something overflows: hi is where the operands and the partial sums still fit, and the model is
    evaluated there."""
    assert end_ok(-60)
    lo = _bisect(-60, -128, end_ok)
    hi = _bisect(60, 128, lambda e: end_ok(e, scale_fits))
    assert end_ok(hi)
    return lo, hi


def admitted(W, x, interval=None):
    """Are the operands inside the derived region?  The magnitude of each operand -- the rms of its non-zero elements, W's in the units of
    its He scaling sqrt(2 / K), which is how the interval was derived -- lies in [2^lo, 2^hi] and the largest sum |w||x| of an output in
    [2^lo, 2^127), to within half a binade (the derivation steps by two).  Elements below an operand's rms -- a normal draw's small values,
    exact zeros, the small channels of a per-channel scaling -- are admitted with it."""
    lo, hi = derived_interval() if interval is None else interval
    W, x = np.asarray(W, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if not (np.isfinite(W).all() and np.isfinite(x).all()):
        return False

    def rms_nz(a):
        nz = a[a != 0]
        return float(np.sqrt(np.mean(nz ** 2))) if nz.size else 1.0

    mags = [rms_nz(x), rms_nz(W) * (W.shape[1] / 2.0) ** 0.5]
    big = float(_mm(np.abs(W), np.abs(x)).max())
    return all(2.0 ** (lo - 0.5) <= m <= 2.0 ** (hi + 0.5) for m in mags) and 2.0 ** (lo - 0.5) <= big < 2.0 ** 127
