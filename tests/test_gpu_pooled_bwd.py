"""The pooled-layer backward (so-net_amd/csrc/pooled_bwd.hip) at its list and tile edges, against tests/pooled_bwd_ref.py: the sparse input
gradient and the weight gradient bit-equal to the numpy restatement of the order the kernels document, the large and wide launches and the
matrix-core kernel bit-equal to float64 on integer-exact operands, and continuous operands inside a bound derived per element:

    sparse dgrad    |got - want| <= n 2^-24 sum |term| (n the element's term count: one f32 rounding of at most 2^-24 of the running sum
                    per fma), n more for the head adds of the entry-balanced kernel; bf16 output between bf16_rne(want -+ d)
    matrix cores    d = (n + KC) 2^-23 sum |term|: one f32 ulp per addition (the rounding inside a 16-term block is not documented as
                    round-to-nearest), the n entries and the KC blocks; operands rounded to bf16 first
    wgrad, B = 64   d = (n + B + 1) 2^-24 sum |term|: the fmas, the add of the two halves, the sum over clouds

The worst observed / bound ratios are printed by the last test (docs/findings.md holds the figures of the run that added this file).
What each case reaches is asserted without a GPU in tests/test_pooled_bwd_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import pooled_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    """f32 tensors as they are, bf16 tensors as their bit patterns (uint16)"""
    if t is None:
        return None
    t = t.contiguous().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def run_dgrad(g, pos, W, C1, L, out="f32", wt_pack=None):
    from sonet_hip import ops
    gx = ops.pooled_dgrad(cu(g), cu(pos), cu(W), C1, W.shape[1] - C1, L, out_dtype=torch.float32 if out == "f32" else torch.bfloat16,
                          wt_pack=wt_pack)
    return [host(t) for t in gx]


def run_dgrad_c(g, pos, W, C1, L, out="f32"):
    """the C entry on a workspace and outputs first filled with 0xFF bytes"""
    from sonet_hip import _lib
    from sonet_hip.ops import ptr, stream_ptr
    lib = _lib.load()
    B, C, M = g.shape
    C2 = W.shape[1] - C1
    esz = 4 if out == "f32" else 2
    ws = torch.full((lib.sonet_pooled_dgrad_ws_size(B, C, M, L),), 0xFF, dtype=torch.uint8, device=DEV)
    o1 = torch.full((B * C1 * L * esz,), 0xFF, dtype=torch.uint8, device=DEV)
    o2 = torch.full((B * C2 * L * esz,), 0xFF, dtype=torch.uint8, device=DEV) if C2 else None
    dg, dp, dw = cu(g), cu(pos), cu(W)
    fn = lib.sonet_pooled_dgrad_f32 if out == "f32" else lib.sonet_pooled_dgrad_obf16
    rc = fn(ptr(dg), ptr(dp), ptr(dw), B, C, M, C1, C2, L, ptr(ws), ptr(o1), ptr(o2), stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    dt = np.float32 if out == "f32" else np.uint16
    return [o1.cpu().numpy().view(dt).reshape(B, C1, L), o2.cpu().numpy().view(dt).reshape(B, C2, L) if C2 else None]


def assert_bits(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), what
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
            if not R.same_bits(a, b):
                bad = np.argwhere(a.view("u%d" % a.dtype.itemsize) != b.view("u%d" % b.dtype.itemsize))
                pytest.fail("%s: output %d differs in %d of %d elements, first at %s" % (what, k, len(bad), a.size, bad[:4].tolist()))


def cat(gx):
    return np.concatenate([t for t in gx if t is not None], axis=1)


def note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), float(ratio))


def assert_within(got32, want, d, kind, what):
    """f32 results: |got - want| <= d per element"""
    err = np.abs(got32.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d > 0, err / d, np.where(err > 0, np.inf, 0.0))
    print("%s: worst |got - want| / bound = %.4f" % (what, ratio.max()))
    note(kind, ratio.max())
    assert bool((err <= d).all()), (what, float(ratio.max()))


def assert_bf16_between(got16, want, d, kind, what):
    """bf16 results: bf16_rne(want - d) <= got <= bf16_rne(want + d) per element"""
    lo, hi, mid = R.bf16_of_f64(want - d), R.bf16_of_f64(want + d), R.bf16_of_f64(want)
    got = R.widen(got16).astype(np.float64)
    span = np.maximum(hi - mid, mid - lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(span > 0, np.abs(got - mid) / span, np.where(got != mid, np.inf, 0.0))
    print("%s: worst bf16 distance / allowed = %.4f" % (what, ratio.max()))
    note(kind, ratio.max())
    assert bool(((got >= lo) & (got <= hi)).all()), (what, float(ratio.max()))


# ------------------------------------------------------------------------------------------------------------ sparse input gradient
@pytest.mark.parametrize("name", [s[0] for s in R.SHAPES] + list(R.LISTS))
def test_sparse_dgrad_is_bit_equal_to_the_restatement(name):
    g, pos, W, C1, L = R.dgrad_named(name)
    want32 = R.dgrad_bits(g, pos, W, C1, L, "f32")
    want16 = [None if t is None else R.bf16_rne(t) for t in want32]
    first = run_dgrad(g, pos, W, C1, L, "f32")
    assert_bits(first, want32, name + " f32")
    assert_bits(run_dgrad(g, pos, W, C1, L, "f32"), first, name + " f32, second run")
    assert_bits(run_dgrad(g, pos, W, C1, L, "bf16"), want16, name + " bf16")
    assert_bits(run_dgrad_c(g, pos, W, C1, L, "f32"), want32, name + " f32 over 0xFF")
    assert_bits(run_dgrad_c(g, pos, W, C1, L, "bf16"), want16, name + " bf16 over 0xFF")
    if name == "all_ignored":
        assert not cat(first).any()
    # the same run against float64, per element
    want, mag, n = R.dgrad64(g, pos, W, L)
    heads = 2 if W.shape[1] % 4 == 0 else 1
    d = heads * n * 2.0 ** -24 * mag
    assert_within(cat(first), want, d, "sparse dgrad f32", name)
    assert_bf16_between(cat(run_dgrad(g, pos, W, C1, L, "bf16")), want, d, "sparse dgrad bf16", name)


@pytest.mark.parametrize("name", ["shape_L161_Cin4_C11_B3_M64", "shape_L255_Cin27_C127_B1_M1"])
def test_sparse_dgrad_confines_a_nan(name):
    """a NaN in g and one in a row of W reach the columns that hold such an entry and no other"""
    g, pos, W, C1, L = R.dgrad_named(name)
    g, W = g.copy(), W.copy()
    B, C, M = g.shape
    live = np.argwhere((pos >= 0) & (pos < L))
    b0, c0, m0 = live[len(live) // 3]
    g[b0, c0, m0] = np.nan
    c1 = int(live[-1][1])
    W[c1, W.shape[1] // 2] = np.nan
    want = R.dgrad_bits(g, pos, W, C1, L, "f32")
    got = run_dgrad(g, pos, W, C1, L, "f32")
    assert_bits(got, want, name)
    hit = np.zeros((B, L), bool)
    hit[b0, pos[b0, c0, m0]] = True
    for b in range(B):
        p = pos[b, c1]
        hit[b, p[(p >= 0) & (p < L)]] = True
    nan = np.isnan(cat(got))
    assert nan.any() and not nan.any(axis=1)[~hit].any() and nan.any(axis=1)[hit].all()
    assert_bits(run_dgrad(g, pos, W, C1, L, "bf16"), [None if t is None else R.bf16_rne(t) for t in want], name + " bf16")


def test_wrapper_hands_the_entry_balanced_kernel_an_aligned_weight():
    """W as a contiguous view 4 bytes into a larger buffer passes every contiguity check; the entry-balanced kernel reads W with 16-byte
    loads, so the wrapper copies such a view (``_aligned16``) before the launch: the pointer the C entry gets is aligned, the bits are the
    restatement's"""
    from sonet_hip import _lib, ops
    g, pos, W, C1, L = R.dgrad_named("tile_385")
    buf = torch.zeros(W.size + 8, dtype=torch.float32, device=DEV)
    buf[1:1 + W.size] = cu(W).flatten()
    wv = buf[1:1 + W.size].view(W.shape)
    assert wv.is_contiguous() and wv.data_ptr() % 16 == 4 and W.shape[1] % 4 == 0
    seen = []
    real = ops.ptr

    def spy(t):
        p = real(t)
        if t is not None and tuple(t.shape) == tuple(W.shape) and t.dtype == torch.float32:
            assert t.data_ptr() % 16 == 0, "a misaligned W on its way to the C entry"          # (raised while the arguments are built: no launch)
            seen.append(t.data_ptr())
        return p
    ops.ptr = spy
    try:
        gx = ops.pooled_dgrad(cu(g), cu(pos), wv, C1, W.shape[1] - C1, L)
    finally:
        ops.ptr = real
    assert seen and all(p % 16 == 0 for p in seen)
    assert_bits([host(t) for t in gx], R.dgrad_bits(g, pos, W, C1, L), "W 4 bytes off its alignment")


def test_sparse_dgrad_replays_from_a_graph():
    from sonet_hip import ops
    g, pos, W, C1, L = R.dgrad_named("shape_L257_Cin84_C183_B3_M5")
    dg, dp, dw = cu(g), cu(pos), cu(W)
    a = ops.pooled_dgrad(dg, dp, dw, C1, W.shape[1] - C1, L)
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.pooled_dgrad(dg, dp, dw, C1, W.shape[1] - C1, L)           # (warm-up on the capture stream)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            out = ops.pooled_dgrad(dg, dp, dw, C1, W.shape[1] - C1, L)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[1])


@pytest.mark.parametrize("name", [c[0] for c in R.LARGE])
def test_large_and_wide_launches_are_exact(name):
    """integer-exact operands: no order can round, so the f32 result IS the float64 one (the serial and the parallel scan of the bucket
    kernel, the largest L, ids up to 2^20 - 2)"""
    g, pos, W, C1, L = R.large_case(name)
    want, mag, _ = R.dgrad64(g, pos, W, L)
    assert float(mag.max()) / R.INT_GRANULE < 2 ** 24
    got = cat(run_dgrad(g, pos, W, C1, L, "f32"))
    want32 = want.astype(np.float32)
    assert (want32.astype(np.float64) == want).all()
    if not R.same_bits(got, want32):
        bad = np.argwhere(got != want32)
        pytest.fail("%s: %d of %d elements differ, first at %s" % (name, len(bad), got.size, bad[:4].tolist()))
    assert_bits([R.bf16_rne(want32)], [cat(run_dgrad(g, pos, W, C1, L, "bf16"))], name + " bf16")


# ------------------------------------------------------------------------------------------------------------ matrix cores
def pack_of(W):
    from sonet_hip import ops
    C, Cin = W.shape
    wt = np.zeros(((Cin + 31) // 32 * 32, C), np.float32)
    wt[:Cin] = W.T
    return ops.pointmlp_pack(cu(wt), "bf16")


@pytest.mark.parametrize("name", [c[0] for c in R.MFMA])
def test_matrix_core_dgrad_exact_operands(name):
    from sonet_hip import ops
    g, pos, W, C1, L = R.mfma_case(name, exact=True)
    assert ops.pooled_dgrad_mfma_ok(g.shape[1], C1, W.shape[1] - C1, L)
    wp = pack_of(W)
    want, _, _ = R.dgrad64(g, pos, W, L)
    want16 = R.bf16_rne(want.astype(np.float32))
    got = cat(run_dgrad(g, pos, W, C1, L, "bf16", wp))
    assert_bits([got], [want16], name)
    assert_bits([cat(run_dgrad(g, pos, W, C1, L, "bf16", wp))], [got], name + ", second run")


@pytest.mark.parametrize("name", [c[0] for c in R.MFMA])
def test_matrix_core_dgrad_continuous_operands(name):
    g, pos, W, C1, L = R.mfma_case(name, exact=False)
    wp = pack_of(W)
    want, mag, n = R.dgrad64(R.to_bf16(g), pos, R.to_bf16(W), L)
    d = (n + g.shape[1] // 16) * 2.0 ** -23 * mag
    got = cat(run_dgrad(g, pos, W, C1, L, "bf16", wp))
    assert_bf16_between(got, want, d, "matrix-core dgrad", name)
    assert_bits([cat(run_dgrad(g, pos, W, C1, L, "bf16", wp))], [got], name + ", second run")


# ------------------------------------------------------------------------------------------------------------ weight gradient
def run_wgrad(g, pos, x, rows, triple, offset=False):
    from sonet_hip import ops
    if rows == "bf16":
        dx = cu(R.bf16_rne(x).view(np.int16)).view(torch.bfloat16)
    else:
        dx = cu(x)
    if offset:                                                            # a view one element into a larger buffer: the scalar copy
        buf = torch.zeros(dx.numel() + 8, dtype=dx.dtype, device=DEV)
        buf[1:1 + dx.numel()] = dx.flatten()
        dx = buf[1:1 + dx.numel()].view(dx.shape)
        assert dx.data_ptr() % 16 == dx.element_size() and dx.is_contiguous()
    xaff = None if triple is None else (cu(triple[0]), cu(triple[1]), bool(triple[2]))
    return host(ops.pooled_wgrad(cu(g), cu(pos), dx, xaff))


def wgrad_want(g, pos, x, sc, sh, rows, relu, parts=False):
    xin = R.bf16_rne(x) if rows == "bf16" else x
    return (R.wgrad_parts if parts else R.wgrad_bits)(g, pos, xin, rows, None if relu is None else (sc, sh, relu))


@pytest.mark.parametrize("name", [c[0] for c in R.WGRAD])
def test_wgrad_is_bit_equal_to_the_restatement(name):
    g, pos, x, sc, sh = R.wgrad_named(name)
    for rows, relu in R.WGRAD_RUNS:
        want = wgrad_want(g, pos, x, sc, sh, rows, relu)
        triple = None if relu is None else (sc, sh, relu)
        got = run_wgrad(g, pos, x, rows, triple)
        assert_bits([got], [want], "%s %s relu=%s" % (name, rows, relu))
        assert_bits([run_wgrad(g, pos, x, rows, triple, offset=True)], [want], "%s %s relu=%s, x off its alignment" % (name, rows, relu))


@pytest.mark.parametrize("rows", ["f32", "bf16"])
def test_wgrad_at_the_largest_rows_the_lds_holds(rows):
    L = R.wgrad_max_L(rows)
    g, pos, x, sc, sh = R.wgrad_named("wgrad_max_" + rows, (2, 40, 33, 3, L))
    pos[0, 0, 1], pos[0, 1, 1] = L - 1, 0
    for relu in (None, 1):
        assert_bits([run_wgrad(g, pos, x, rows, None if relu is None else (sc, sh, relu))], [wgrad_want(g, pos, x, sc, sh, rows, relu)],
                    "L=%d %s relu=%s" % (L, rows, relu))


@pytest.mark.parametrize("rows", ["f32", "bf16"])
def test_wgrad_partials_through_the_c_entry(rows):
    """per-cloud partials over an output first filled with 0xFF bytes"""
    from sonet_hip import _lib
    from sonet_hip.ops import ptr, stream_ptr
    lib = _lib.load()
    name, B, C, M, Ci, L = R.WGRAD[4]
    g, pos, x, sc, sh = R.wgrad_named(name)
    dx = cu(R.bf16_rne(x).view(np.int16)) if rows == "bf16" else cu(x)
    dg, dp, dsc, dsh = cu(g), cu(pos), cu(sc), cu(sh)
    plain, xaff = ((lib.sonet_pooled_wgrad_f32, lib.sonet_pooled_wgrad_xaff_f32) if rows == "f32" else
                   (lib.sonet_pooled_wgrad_xbf16, lib.sonet_pooled_wgrad_xaff_xbf16))
    for relu in (None, 0, 1):
        part = torch.full((B * C * Ci * 4,), 0xFF, dtype=torch.uint8, device=DEV)
        if relu is None:
            rc = plain(ptr(dg), ptr(dp), ptr(dx), B, C, M, Ci, L, ptr(part), stream_ptr())
        else:
            rc = xaff(ptr(dg), ptr(dp), ptr(dx), B, C, M, Ci, L, ptr(part), ptr(dsc), ptr(dsh), relu, stream_ptr())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        got = part.cpu().numpy().view(np.float32).reshape(B, C, Ci)
        assert_bits([got], [wgrad_want(g, pos, x, sc, sh, rows, relu, parts=True)], "%s relu=%s" % (rows, relu))


def test_wgrad_confines_a_nan():
    name, B, C, M, Ci, L = R.WGRAD[5]
    g, pos, x, sc, sh = R.wgrad_named(name)
    x[1, :, 2] = np.nan                                                  # a column of x
    g[0, 7, 5] = np.nan
    pos[0, 7, 5] = 1
    got = run_wgrad(g, pos, x, "f32", None)
    assert_bits([got], [wgrad_want(g, pos, x, sc, sh, "f32", None)], name)
    hit = (pos[1] == 2).any(axis=0)
    hit[5] = True
    assert np.isnan(got).all(axis=1)[hit].all() and not np.isnan(got)[~hit].any() and not hit.all()


def test_wgrad_sum_over_many_clouds():
    B, C, M, Ci, L = 64, 40, 33, 5, 50
    g, pos, x, sc, sh = R.wgrad_named("wgrad_b64", (B, C, M, Ci, L))
    got = run_wgrad(g, pos, x, "f32", None)
    assert_bits([run_wgrad(g, pos, x, "f32", None)], [got], "second run")
    want, mag, n = R.wgrad64(g, pos, x)
    assert_within(got, want, (n + B + 1) * 2.0 ** -24 * mag, "wgrad over 64 clouds", "B=64")


def test_zz_worst_ratios():
    """(runs last in the file: the worst observed / bound of the derived bounds)"""
    for kind in sorted(WORST):
        print("worst observed / bound, %s: %.4f" % (kind, WORST[kind]))
    assert all(v <= 1.0 for v in WORST.values())
