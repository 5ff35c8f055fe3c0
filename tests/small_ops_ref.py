"""Numpy restatements of the node-level gather, max, FC and Adam kernels (csrc/som.hip, csrc/node_train.hip, the node / FC kernels of
csrc/bn_passes.hip, csrc/fc_head.hip, csrc/optim.hip) and the seeded inputs of tests/test_gpu_small_ops.py.  Plain numpy, no torch, nothing from sonet_hip:
tests/test_small_ops_cpu.py pins this file to the reference's torch expressions on the CPU, the GPU tests pin the kernels to this file.

Every restatement follows the kernel's documented expression in the kernel's own operation order, in the dtype of its inputs (float32: the
kernel's numbers, bit for bit; float64: the same expression for the comparison with torch).  numpy's f32 add, subtract, multiply, divide and
sqrt are correctly rounded, and so are the kernels': the library is built with -ffp-contract=off -fno-fast-math and without
-fno-hip-fp32-correctly-rounded-divide-sqrt, so ``sum / (float)K`` is IEEE division.  The two kernels that use explicit fmas
(node_add_affine_act, node_gather_lead_affine_act) go through the float64 fma model of tests/bn_passes_ref.py; ``tie_count`` says for how many
elements that model could differ from a true fma (the CPU test asserts: none on the seeded inputs).

The functions take "breaks" as keyword parameters: the same restatement with one deliberate mistake, used by the CPU test to show that the seeded
inputs tell the mistake from the contract."""
import math

import numpy as np

from bn_passes_ref import U24, add64, bf16_bits, bf16_widen, round_bf16, tie_count, to_f32  # noqa: F401  (re-exported for the tests)

INT64_MIN = -2 ** 63
INT32_MIN = -2 ** 31


def same_bits(a, b):
    """Bit equality of two f32 arrays; a NaN equals a NaN (payloads are not part of any contract here)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def first_diff(a, b):
    """For assertion messages: count and first position of the elements that ``same_bits`` tells apart."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return "shapes %s vs %s" % (a.shape, b.shape)
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    if not bad.any():
        return "equal"
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    return "%d of %d differ, first at %s: %r vs %r" % (int(bad.sum()), bad.size, at, a[at], b[at])


# ---------------------------------------------------------------------------------------------- gathers
def in_range(I, M, trunc32=False):
    """The contract of every index-taking kernel here: an index outside [0, M) reads as 0 / belongs to nobody.  The int64 kernels compare
    the whole 64-bit pattern (as unsigned).  Break ``trunc32``: the comparison sees only the low 32 bits."""
    I = np.asarray(I).astype(np.int64)
    if trunc32:
        I = I.astype(np.int32).astype(np.int64)
    return I, (I >= 0) & (I < M)


def gather(x, I, trunc32=False):
    """x [B][C][M], I [B][...] (int64 or int32) -> [B][C][...]: x[b][c][I[b][...]], +0.0 where the index is out of range.
    knn_gather (I [B][M][K]), node_gather (I [B][kN]) and the feature rows of knn_group."""
    x = np.asarray(x)
    B, C, M = x.shape
    I, ok = in_range(I, M, trunc32)
    safe = np.where(ok, I, 0).reshape(B, 1, -1)
    out = np.take_along_axis(x, np.broadcast_to(safe, (B, C, safe.shape[2])), axis=2)
    out = np.where(ok.reshape(B, 1, -1), out, x.dtype.type(0))
    return out.reshape((B, C) + I.shape[1:])


def knn_center(coord, I, avg, count_in_range=False):
    """-> (neighbour coordinates [B][3][M][K], centre [B][3][M]).  'avg': a sequential sum in k order starting from +0, out-of-range
    neighbours entering as 0, then ONE division by K.  'center': the node itself.  Break ``count_in_range``: divides by the number of
    in-range neighbours (at least 1)."""
    coord = np.asarray(coord)
    B, _, M = coord.shape
    K = np.shape(I)[2]
    nb = gather(coord, I)
    if not avg:
        return nb, coord.copy()
    s = np.zeros((B, 3, M), coord.dtype)
    for k in range(K):
        s = s + nb[..., k]
    if count_in_range:
        div = np.maximum(in_range(I, M)[1].sum(-1), 1).astype(coord.dtype)[:, None, :]
    else:
        div = coord.dtype.type(K)
    return nb, s / div


def knn_group(coord, feat, I, avg, count_in_range=False):
    """-> (centre [B][3][M], out [B][3 + C][M][K]): rows 0-2 = neighbour coordinate - centre (one subtraction), rows 3.. = gathered features."""
    nb, ctr = knn_center(coord, I, avg, count_in_range)
    return ctr, np.concatenate([nb - ctr[..., None], gather(feat, I)], axis=1)


def knn_prepare(coord, I, avg):
    """-> (centre [B][3][M], dec [B][3][K * M] K-MAJOR, gidx [B][K * M] int32 = the index, or -1 out of range): knn_group's coordinate rows
    transposed, and the gather index the gathering layers consume."""
    nb, ctr = knn_center(coord, I, avg)
    B, _, M, K = nb.shape
    dec = (nb - ctr[..., None]).transpose(0, 1, 3, 2).reshape(B, 3, K * M)
    Iv, ok = in_range(I, M)
    gidx = np.where(ok, Iv, -1).astype(np.int32).transpose(0, 2, 1).reshape(B, K * M)
    return ctr, dec, gidx


def som_mask(ids, M):
    """ids [B][kN] -> one-hot [B][kN][M] int32; an id outside [0, M) gives a row of zeros."""
    return (np.asarray(ids)[..., None] == np.arange(M)).astype(np.int32)


# ---------------------------------------------------------------------------------------------- maxima
def lastdim_max(x, skip=None):
    """max over the last axis: a NaN wins, otherwise the maximum by value.  Break ``skip = (tpr, q)``: the share of lane q of tpr lanes
    (elements k = q mod tpr) never reaches the result."""
    x = np.asarray(x, np.float32)
    if skip is not None:
        tpr, q = skip
        x = np.where((np.arange(x.shape[-1]) % tpr) == q, np.float32(-np.inf), x)
    with np.errstate(invalid="ignore"):
        return np.max(x, axis=-1)                               # (np.max propagates NaN)


def planes_max(x, K):
    """x [B][C][K * M] k-major -> [B][C][M]: max over the K planes, a NaN wins."""
    x = np.asarray(x, np.float32)
    B, C, L = x.shape
    with np.errstate(invalid="ignore"):
        return np.max(x.reshape(B, C, K, L // K), axis=2)


def lastdim_argmax(x):
    """-> (value, index int32) of the FIRST maximum; the FIRST NaN wins.  x holds f32 or (widened) bf16 values: the value is one of them,
    so bf16 storage of it is exact."""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    idx = np.where(nan.any(-1), nan.argmax(-1), np.argmax(np.where(nan, np.float32(-np.inf), x), axis=-1))
    return np.take_along_axis(x, idx[..., None], axis=-1)[..., 0], idx.astype(np.int32)


def lastdim_max_bwd(g, idx, K):
    """gx[r][k] = g[r] where k == idx[r], +0.0 elsewhere."""
    g = np.asarray(g, np.float32)
    return np.where(np.arange(K) == np.asarray(idx)[..., None], g[..., None], np.float32(0))


# ---------------------------------------------------------------------------------------------- backward gathers
def _inverse_sum(gf, If, M, drop_last):
    """gf [B][C][E], If [B][E] -> [B][C][M]: for every node the sum of its entries in ASCENDING entry order, accumulated in gf's dtype from +0
    (an explicit loop over the entries: no library scatter whose order is its own business).  Entries outside [0, M) are dropped; a node
    without entries keeps +0.0.  Break ``drop_last``: every node's last entry is left out."""
    B, C, E = gf.shape
    gx = np.zeros((B, C, M), gf.dtype)
    for b in range(B):
        ids = If[b]
        last = {}
        if drop_last:
            for e in range(E):
                last[int(ids[e])] = e
        for e in range(E):
            i = int(ids[e])
            if 0 <= i < M and last.get(i) != e:
                gx[b, :, i] = gx[b, :, i] + gf[b, :, e]
    return gx


def knn_gather_bwd(g, I, M, drop_last=False):
    """g [B][C][M][K] (f32, or bf16 values widened: exact), I [B][M][K] int64 -> gx [B][C][M] f32 (float64 in, float64 out)."""
    g = np.asarray(g)
    B, C = g.shape[:2]
    return _inverse_sum(g.reshape(B, C, -1), np.asarray(I).astype(np.int64).reshape(B, -1), M, drop_last)


def node_gather_bwd(g, ids, M, drop_last=False):
    """g [B][C][L], ids [B][L] int32 -> gx [B][C][M] f32, every node's columns summed in ascending column order."""
    return _inverse_sum(np.asarray(g), np.asarray(ids).astype(np.int64), M, drop_last)


# ---------------------------------------------------------------------------------------------- the two fma kernels
def _fma(a, b, c, dtype=np.float32):
    """fma(a, b, c) on f32 arrays through float64 (a b is exact there) -> (f32 result, float64 value, inexact flags of the float64 sum).
    dtype float64: the plain float64 expression a b + c, for the comparison with torch."""
    with np.errstate(invalid="ignore", over="ignore"):
        s, ix = add64(np.asarray(a, np.float64) * np.asarray(b, np.float64), np.asarray(c, np.float64))
    return (s if dtype == np.float64 else to_f32(s)), s, ix


def _relu(v, relu):
    return np.where(v < 0, v.dtype.type(0), v) if relu else v      # v < 0 ? 0 : v keeps -0.0 and NaN


def node_add_affine_act(t, z, ids, sc, sh, relu, want_ties=False, dtype=np.float32):
    """act(fma(fl(t + z_or_0), sc[c], sh[c])): t [B][C][L], z [B][C][M], ids [B][L]; an id outside [0, M) adds +0.0."""
    u = np.asarray(t, dtype) + gather(np.asarray(z, dtype), ids)
    v, s, ix = _fma(u, np.asarray(sc, np.float32).reshape(1, -1, 1), np.asarray(sh, np.float32).reshape(1, -1, 1), dtype)
    out = _relu(v, relu)
    return (out, tie_count(s, inexact=ix)) if want_ties else out


def node_gather_lead(z, gidx, lead, wl, sc, sh, relu, bf16=False, want_ties=False, dtype=np.float32):
    """a = z_or_0[b][c][gidx[b][l]]; a = fma(wl[c][i], lead[b][i][l], a) for i = 0..3 in channel order (an absent channel is
    fma(0, 0, a) = a + 0: exact, -0.0 becomes +0.0); a = fma(a, sc[c], sh[c]); (relu && a < 0) ? 0 : a; stored as f32 or as nearest-even bf16
    (returned widened).  z [B][C][M] f32 (bf16: values widened), gidx [B][L] int32, lead [B][NL][L], wl [C][NL]."""
    a = gather(np.asarray(z, dtype), gidx)
    lead, wl = np.asarray(lead, np.float32), np.asarray(wl, np.float32)
    NL = lead.shape[1]
    ties = 0
    for i in range(4):
        if i < NL:
            a, s, ix = _fma(wl[:, i].reshape(1, -1, 1), lead[:, i:i + 1, :], a, dtype)
            ties += tie_count(s, inexact=ix)
        else:
            a = a + a.dtype.type(0)
    v, s, ix = _fma(a, np.asarray(sc, np.float32).reshape(1, -1, 1), np.asarray(sh, np.float32).reshape(1, -1, 1), dtype)
    ties += tie_count(s, inexact=ix)
    out = _relu(v, relu)
    if bf16:
        out = round_bf16(out)
    return (out, ties) if want_ties else out


# ---------------------------------------------------------------------------------------------- Adam
def adam_scalars(step, lr, b1, b2, eps):
    """The per-tensor and per-launch scalars as sonet_hip/optim.py forms them: in double, then ONE rounding to f32 on the way to the kernel."""
    f = np.float32
    return dict(ss=f(lr / (1.0 - b1 ** step)), bs=f(math.sqrt(1.0 - b2 ** step)), beta1=f(b1), beta2=f(b2), w1=f(1.0 - b1), w2=f(1.0 - b2),
                eps=f(eps))


def adam_step(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, dtype=np.float32, fma_v=False):
    """One step of adam_multi_kernel, line for line, every operation rounded to ``dtype`` (float32: the kernel's bits; float64: the same
    expression for the error count of the CPU test -- the SCALARS stay the f32 values the kernel receives).  -> (p, m, v).
    Break ``fma_v``: v = fma(fl(w2 g), g, fl(v beta2)) -- one rounding fewer."""
    c = {k: dtype(x) for k, x in adam_scalars(float(step), lr, b1, b2, eps).items()}
    p, g, m, v = (np.asarray(t, dtype) for t in (p, g, m, v))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        d = g - m
        m2 = m + c["w1"] * d if c["w1"] < 0.5 else g - d * (dtype(1) - c["w1"])
        if fma_v:
            v2 = to_f32(np.asarray(c["w2"] * g, np.float64) * np.asarray(g, np.float64) + np.asarray(v * c["beta2"], np.float64))
        else:
            v2 = v * c["beta2"] + (c["w2"] * g) * g
        denom = np.sqrt(v2) / c["bs"] + c["eps"]
        p2 = p + (-c["ss"]) * (m2 / denom)
    return p2, m2, v2


# ---------------------------------------------------------------------------------------------- linear_act
def linear_chain(Cin):
    """Longest fma chain of one lane of linear_act_kernel.  Lane ks of a row owns the float4 j * 16 + ks, j < ceil(Cin / 64), i.e. the columns
    64 j + 4 ks + e; lane 0 owns the most columns below Cin: 4 floor(Cin / 64) + min(4, Cin mod 64).  (Its padded columns are fma(0, 0, acc):
    exact.)  This is ceil(Cin / 16) when Cin mod 64 is 0 or above 48 and LARGER otherwise (Cin = 17: lane 0 adds 4 products, not 2)."""
    return 4 * (Cin // 64) + min(4, Cin % 64)


def linear_act(x, W, sc, sh, relu, drop_tail=False):
    """-> (y float64, bound): y = act((x W^T) scale + shift) in float64 and the per-element bound of the kernel's f32 evaluation.

    The kernel: a lane accumulates its columns with one fma each, n = linear_chain(Cin) roundings, |error| <= n u S_lane (u = 2^-24, S the
    sum of the |x_k w_k| it owns, first order); the row's 16 lane sums are then added in a fixed order starting from 0 (the first add is exact:
    15 roundings, each at most u times the sum of all |x_k w_k|, counted as 16); the epilogue is one fma, one rounding of a value of magnitude
    at most |scale| S + |shift|.  Carried through the multiplication by scale: (n + 16 + 1) u (|scale| S + |shift|).  The second-order terms
    are below (n + 17)^2 u^2 (...) < 2^-16 of the first-order bound for n <= 256; one more u covers them and the float64 reference's own
    2^-53-class error:  bound = (n + 16 + 2) 2^-24 (|scale| sum_k |x_k w_k| + |shift|).  ReLU is 1-Lipschitz: the bound passes through.
    Break ``drop_tail``: the last float4 of every row (columns >= Cin - 4) never enters the sum."""
    x64, W64 = np.asarray(x, np.float64), np.asarray(W, np.float64)
    sc, sh = np.asarray(sc, np.float64)[None, :], np.asarray(sh, np.float64)[None, :]
    Cin = x64.shape[1]
    with np.errstate(invalid="ignore"):
        S = np.abs(x64) @ np.abs(W64).T
        xs = x64[:, :max(Cin - 4, 0)] if drop_tail else x64
        y = (xs @ W64[:, :xs.shape[1]].T) * sc + sh
        if relu:
            y = np.where(y < 0, 0.0, y)
    return y, (linear_chain(Cin) + 16 + 2) * U24 * (np.abs(sc) * S + np.abs(sh))


# ---------------------------------------------------------------------------------------------- seeded inputs
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _f32(v):
    return np.ascontiguousarray(v, np.float32)


def oor_values(M):
    """Indices that must read as 0: below, at and far above the range, and two whose low 32 bits are a valid node (2^32 + 1 -> node 1,
    INT64_MIN -> node 0)."""
    return [-1, M, 2 ** 31, 2 ** 32 + 1, INT64_MIN]


# (B, C, M, K): M K = 1, 255, 256, 257 (the 256-thread block edge of knn_gather / knn_prepare), 1023, 1024, 1025 (the 1024-position grid edge
# of knn_group), K = 1, 3, 4, 5, 9 (quads of knn_group straddle two nodes unless K % 4 == 0), M K % 4 == 0 (float4 stores) and not
KNN_SHAPES = [(B, C, M, K) for (M, K) in ((1, 1), (85, 3), (64, 4), (257, 1), (341, 3), (256, 4), (205, 5), (7, 9), (29, 9))
              for (B, C) in ((1, 1), (3, 5))]


def knn_inputs(B, C, M, K, oor=True, seed=1):
    """coord [B][3][M], feat [B][C][M] (no zeros: a wrongly read 0 shows), I [B][M][K] int64 with ~1/8 of the entries out of range (all
    five kinds, wherever M K allows) and ALL K neighbours of node M // 2 of the last cloud out of range."""
    g = _rng(seed, B, C, M, K)
    coord, feat = _f32(g.standard_normal((B, 3, M))), _f32(g.standard_normal((B, C, M)) + 3.0)
    I = g.integers(0, M, (B, M, K)).astype(np.int64)
    if oor:
        vals = oor_values(M)
        flat = I.reshape(-1)
        pos = g.permutation(flat.size)[:max(min(len(vals), flat.size - 1), flat.size // 8)]
        for n, e in enumerate(pos):
            flat[e] = vals[n % len(vals)]
        I[B - 1, M // 2, :] = [vals[k % len(vals)] for k in range(K)]
    return coord, feat, I


def node_ids(g, B, L, M, oor=True):
    """[B][L] int32 node ids, ~1/8 of them -1, M or INT32_MIN."""
    ids = g.integers(0, M, (B, L)).astype(np.int32)
    if oor:
        vals = [-1, M, INT32_MIN]
        flat = ids.reshape(-1)
        for n, e in enumerate(g.permutation(flat.size)[:max(1, flat.size // 8)]):
            flat[e] = vals[n % 3]
    return ids


LASTDIM_K = (1, 5, 6, 7, 47, 48, 49, 64, 1000)          # 1 thread per row below 6, 4 below 48, 16 from 48
LASTDIM_ROWS = (1, 15, 16, 17, 63, 64, 65, 257)


def lastdim_inputs(rows, K, seed=2):
    """[rows][K] f32.  Row r (r % 3 != 1) carries one NaN at a position k = r mod 16 (every lane position in turn, walking through the
    row's groups of 16; row 0: k = 0) when that is below K; then, where the rows exist: row 1 all -inf, row 4 all equal, row 7 +inf and a
    NaN, row 10 a maximum in the LAST position."""
    g = _rng(seed, rows, K)
    x = _f32(g.standard_normal((rows, K)))
    for r in range(rows):
        pos = (r % 16) + 16 * ((r // 16) % max(1, K // 16))
        if r % 3 != 1 and pos < K:
            x[r, pos] = np.nan
    if rows > 1:
        x[1, :] = -np.inf
    if rows > 4:
        x[4, :] = np.float32(0.625)
    if rows > 7:
        x[7, :] = g.standard_normal(K)
        x[7, K // 2] = np.inf
        x[7, K - 1] = np.nan
    if rows > 10:
        x[10, :] = g.standard_normal(K)
        x[10, K - 1] = 100.0
    return x


def argmax_inputs(rows, K, bf16, seed=3):
    """[rows][K] (bf16: bf16 values in f32).  Ties from a coarse grid; row 0: two NaNs (K >= 3: at 1 and K - 1), row 1 all -inf, row 2 all
    equal, row 3 the maximum twice."""
    g = _rng(seed, rows, K, bf16)
    x = _f32(np.round(g.standard_normal((rows, K)) * 4) / 4)
    if K >= 3:
        x[0, 1] = x[0, K - 1] = np.nan
    if rows > 1:
        x[1, :] = -np.inf
    if rows > 2:
        x[2, :] = 1.5
    if rows > 3 and K >= 2:
        x[3, 0] = x[3, K - 1] = 50.0
    return round_bf16(x) if bf16 else x


def fma_case_inputs(B, C, L, M, NL, bf16, seed=4):
    """Inputs of the two fma kernels: t / lead [B][.][L], z [B][C][M], wl [C][NL], scale (both signs), shift, ids with out-of-range entries."""
    g = _rng(seed, B, C, L, M, NL, bf16)
    z = _f32(g.standard_normal((B, C, M)))
    if bf16:
        z = round_bf16(z)
    sign = np.where(g.random(C) < 0.25, -1.0, 1.0)
    return dict(t=_f32(g.standard_normal((B, C, L))), z=z, ids=node_ids(g, B, L, M), lead=_f32(g.standard_normal((B, NL, L)) * 0.5),
                wl=_f32(g.standard_normal((C, NL))), sc=_f32((g.random(C) + 0.5) * sign), sh=_f32(g.standard_normal(C) * 0.4))


def node_add_inputs(B, C, L, M):
    """``fma_case_inputs`` with two planted elements: (0, 0, 0) has the pre-activation -0.0 (t = z = -0.0 through an in-range id, a positive
    scale, shift = -0.0: fma(-0, sc, -0) = -0.0, and ``v < 0 ? 0 : v`` keeps it), the middle of the last row is NaN."""
    d = fma_case_inputs(B, C, L, M, 0, False)
    d["t"][0, 0, 0], d["z"][0, 0, 0], d["ids"][0, 0] = -0.0, -0.0, 0
    d["sc"][0], d["sh"][0] = abs(d["sc"][0]), -0.0
    d["nan_at"] = (B - 1, C - 1, L // 2)
    if d["nan_at"] != (0, 0, 0):
        d["t"][d["nan_at"]] = np.nan
    return d


# (B, C, L, M): M = 1, 257 (a second stride of the LDS fill), 8192 (the limit); L = 1, 2047, 2048, 2049 (gridDim.y = ceil(L / 2048))
NODE_ADD_SHAPES = [(3, 5, 1, 1), (1, 1, 2047, 257), (3, 5, 2048, 257), (2, 3, 2049, 8192), (1, 2, 300, 64)]
# (B, C, L, M, NL): every NL; C = 1, 8, 9 (8 channels per workgroup); L = 1, 3 (scalar), 4 (one quad), 129 / 516 (a second stride of 128 quads
# needs L > 512: 516 = 129 quads); M = 1, 1024 (the limit)
LEAD_SHAPES = [(1, 1, 1, 1, 0), (3, 8, 3, 1024, 1), (2, 9, 4, 1, 2), (1, 9, 129, 1024, 3), (3, 8, 516, 64, 4), (2, 9, 129, 64, 4),
               (1, 1, 4, 1024, 3), (2, 8, 1, 64, 4)]

LINEAR_CIN = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 1792, 1793, 4096)
LINEAR_B = (1, 15, 16, 17)
LINEAR_COUT = (1, 7, 8, 9)


def linear_inputs(B, Cin, Cout, seed=5):
    g = _rng(seed, B, Cin, Cout)
    sign = np.where(g.random(Cout) < 0.25, -1.0, 1.0)
    return dict(x=_f32(g.standard_normal((B, Cin))), W=_f32(g.standard_normal((Cout, Cin)) / math.sqrt(Cin)),
                sc=_f32((g.random(Cout) + 0.5) * sign), sh=_f32(g.standard_normal(Cout) * 0.4))


ADAM_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8193)
ADAM_STEPS = 5
ADAM_SKIPS = (2, 1)              # tensor 2 receives no gradient at step index 1: its step count falls behind
ADAM_ZERO_GRAD = 3               # tensor 3: every gradient is zero (denominator = eps)
ADAM_HUGE, ADAM_OVERFLOW, ADAM_NAN = (6, 4095), (6, 4096), (7, 8192)   # (tensor, element): g = 1e20, g = 1e30, g = NaN -- chunk tails / heads


def adam_inputs(seed=6):
    """-> (params, grads[step][tensor] or None).  Gradient scales 1e-2, 1e-1, 1 by tensor; the planted elements keep their value every step."""
    g = _rng(seed)
    params = [_f32(g.standard_normal(n)) for n in ADAM_SIZES]
    grads = []
    for s in range(ADAM_STEPS):
        row = []
        for t, n in enumerate(ADAM_SIZES):
            if (t, s) == ADAM_SKIPS:
                row.append(None)
                continue
            gr = _f32(g.standard_normal(n) * 10.0 ** ((t % 3) - 2))
            if t == ADAM_ZERO_GRAD:
                gr[:] = 0.0
            for (tt, e), val in ((ADAM_HUGE, 1e20), (ADAM_OVERFLOW, 1e30), (ADAM_NAN, np.nan)):
                if tt == t:
                    gr[e] = val
            row.append(gr)
        grads.append(row)
    return params, grads


def adam_run(params, grads, **kw):
    """The restatement over all steps -> list per step of [(p, m, v) per tensor]; a tensor without a gradient keeps state and step count."""
    st = [(p.copy(), np.zeros_like(p), np.zeros_like(p), 0) for p in params]
    out = []
    for row in grads:
        for t, gr in enumerate(row):
            if gr is None:
                continue
            p, m, v, n = st[t]
            st[t] = adam_step(p, gr, m, v, n + 1, **kw) + (n + 1,)
        out.append([(p.copy(), m.copy(), v.copy()) for p, m, v, _ in st])
    return out
