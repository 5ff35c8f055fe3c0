"""tests/pooled_bwd_ref.py, the reference of the pooled-layer backward's GPU tests, held to account without a GPU:

  * the restatement hashes to every recorded digest of the non-matrix-core cases of tests/golden/pooled_bits.json (a re-recording cannot
    bless a kernel that left the documented order), with the number of midpoint corrections of the fma emulation asserted;
  * dgrad64 / wgrad64 equal float64 autograd of the dense data flow (layer, gather at pos, dot with g);
  * every break of the restatement turns the case built for it red, and every order-sensitive layout ends on other bits under its break;
  * every layout reaches what its name says, computed from the constants restated next to the header's;
  * the integer-exact cases are exact by derivation;
  * the C entries refuse what they document before any launch (only calls that ARE refused: nothing here reaches a device)."""
import ctypes
import hashlib
import json

import numpy as np
import pytest
import torch

import pooled_bwd_ref as R

P = R.P


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------ the recording
def test_restatement_reproduces_every_recorded_digest():
    with open(P.FIXTURE) as f:
        rec = json.load(f)
    fixes, seen = R.FMA_FIXES[0], 0
    for name, shape, pile in P.DGRAD:
        B, C, M, C1, C2, L = shape
        g, pos, W = P.dgrad_inputs(name, shape, pile)
        for out in ("f32", "bf16"):
            got = [sha(t) for t in R.dgrad_bits(g, pos, W, C1, L, out) if t is not None]
            assert got == rec[name + "_" + out], (name, out)
            seen += len(got)
    for name, shape in P.WGRAD:
        g, pos, x, sc, sh = P.wgrad_inputs(name, shape)
        xb = R.bf16_rne(x)
        got = [sha(R.wgrad_bits(g, pos, x if rows == "f32" else xb, rows, None if relu is None else (sc, sh, relu))) for rows, relu in P.WGRAD_RUNS]
        assert got == rec[name], (name, [a == b for a, b in zip(got, rec[name])])
        seen += len(got)
    # every digest of the ten dgrad_* and eight wgrad_* cases: 18 output tensors of the sparse input gradient (one case has one panel), 48
    # weight gradients
    assert seen == sum(len(v) for k, v in rec.items() if not k.startswith("mfma")) == 66
    assert R.FMA_FIXES[0] - fixes == 0                          # the midpoint correction never fires on the recorded inputs


def test_fma32_rounds_once():
    """a * b + 2^29 around the midpoint 2^29 + 32 of two f32 numbers (their gap is 64 there, the float64 gap 2^-23)"""
    big, x = np.float32(2.0 ** 29), 2.0 ** -12
    a, b_up, b_dn = np.float32(1 + x), np.float32(32 * (1 - x + x * x)), np.float32(32 * (1 - x))
    assert float(a) * float(b_up) == 32 * (1 + x ** 3) and float(a) * float(b_dn) == 32 * (1 - x * x)          # exact in float64
    fixes = R.FMA_FIXES[0]
    assert float(R.fma32(np.float32(32), np.float32(1), big)) == big and R.FMA_FIXES[0] == fixes                  # ON the midpoint, exactly: to even
    assert float(R.fma32(a, b_dn, big)) == big and R.FMA_FIXES[0] == fixes                                        # below it, float64 holds the sum
    # 2^-31 above it: float64 rounds the sum ONTO the midpoint and a second rounding would go to even (down); the fma goes up
    assert float(big) + float(a) * float(b_up) == 2.0 ** 29 + 32
    assert float(R.fma32(a, b_up, big)) == np.float32(2.0 ** 29 + 64) and R.FMA_FIXES[0] == fixes + 1
    assert float(R.fma32(a, -b_up, -big)) == np.float32(-(2.0 ** 29 + 64)) and R.FMA_FIXES[0] == fixes + 2
    assert list(R.bf16_rne(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32))) == [0x3F80, 0x3F82, 0x3F81]
    assert R.bf16_of_f64(1 + 2.0 ** -8) == 1.0 and R.bf16_of_f64(1 + 2.0 ** -8 + 2.0 ** -40) == 1 + 2.0 ** -7


# ------------------------------------------------------------------------------------------------------------ the dense expression
def test_dense_float64_expressions_equal_autograd():
    name, B, C, M, Cin, L = "dense64", 3, 10, 6, 7, 21
    g, pos, W = R.dgrad_case(name, B, C, M, Cin, L, lambda p, *_: R.sprinkle(p, L))
    pos[:, 1, :3] = 4                                           # duplicates add
    x = P.unit(name, 7, (B, Cin, L))
    xt = torch.from_numpy(x).double().requires_grad_()
    Wt = torch.from_numpy(W).double().requires_grad_()
    y = torch.einsum("ci,bil->bcl", Wt, xt)                     # the layer
    pt = torch.from_numpy(pos).long()
    ok = (pt >= 0) & (pt < L)
    picked = torch.gather(y, 2, pt.clamp(0, L - 1)) * ok        # the gather at pos; out-of-range positions are ignored
    (picked * torch.from_numpy(g).double()).sum().backward()
    gx, mag, n = R.dgrad64(g, pos, W, L)
    assert np.abs(gx - xt.grad.numpy()).max() <= 1e-12 and (mag >= np.abs(gx) - 1e-15).all()
    assert n.sum() == ok.sum().item() and n.shape == (B, 1, L)
    gw, wmag, wn = R.wgrad64(np.ascontiguousarray(g.transpose(0, 2, 1)), np.ascontiguousarray(pos.transpose(0, 2, 1)), x)
    assert np.abs(gw - Wt.grad.numpy()).max() <= 1e-12 and (wmag >= np.abs(gw) - 1e-15).all()
    assert wn.sum() == ok.sum().item()
    # and the restatements compute the same gradients, inside the bound the GPU test derives
    got = np.concatenate([t for t in R.dgrad_bits(g, pos, W, 3, L) if t is not None], axis=1)
    assert (np.abs(got - gx) <= n * 2.0 ** -24 * mag).all()


# ------------------------------------------------------------------------------------------------------------ breaks
def differs(a, b):
    return not all(R.same_bits(x, y) for x, y in zip(a, b) if x is not None)


@pytest.mark.parametrize("name", list(R.LISTS))
def test_every_list_layout_is_red_under_its_breaks(name):
    g, pos, W, C1, L = R.dgrad_named(name)
    base = R.dgrad_bits(g, pos, W, C1, L)
    assert not differs(base, R.dgrad_bits(g, pos, W, C1, L))
    for br in R.LISTS[name][7]:
        assert differs(base, R.dgrad_bits(g, pos, W, C1, L, breaks=(br,))), (name, br)
    assert differs(R.dgrad_bits(g, pos, W, C1, L, "bf16"), R.dgrad_bits(g, pos, W, C1, L, "bf16", breaks=("bf16_trunc",))) or name == "all_ignored"


def test_every_break_is_red_somewhere():
    seen = set()
    for name in R.LISTS:
        seen |= set(R.LISTS[name][7])
    assert seen == {"sort_by_id", "rem_last", "head_reverse", "drop_last_bucket", "pos_eq_L"}
    # the weight gradient: two half chains, an entry on column L, the bf16 store of the normalised rows
    name = R.WGRAD[5][0]                                         # M = 64
    g, pos, x, sc, sh = R.wgrad_named(name)
    L = x.shape[2]
    assert (pos == L).any() and g.shape[1] == 64
    base = R.wgrad_bits(g, pos, x)
    assert not R.same_bits(base, R.wgrad_bits(g, pos, x, breaks=("one_chain",)))
    g2, pos2, x2, _, _ = R.wgrad_named(R.WGRAD[4][0])           # (rows beyond the first two: the element after a row's end is a drawn one)
    assert (pos2 == x2.shape[2]).any() and not R.same_bits(R.wgrad_bits(g2, pos2, x2), R.wgrad_bits(g2, pos2, x2, breaks=("pos_eq_L",)))
    xb = R.bf16_rne(x)
    assert not R.same_bits(R.wgrad_bits(g, pos, xb, "bf16", (sc, sh, 0)), R.wgrad_bits(g, pos, xb, "bf16", (sc, sh, 0), breaks=("bf16_trunc",)))
    assert set(R.BREAKS) == seen | {"one_chain", "bf16_trunc"}


@pytest.mark.parametrize("name", [c[0] for c in R.WGRAD if c[3] > 32])
def test_wgrad_layouts_show_the_two_half_chains(name):
    g, pos, x, sc, sh = R.wgrad_named(name)
    assert not R.same_bits(R.wgrad_bits(g, pos, x), R.wgrad_bits(g, pos, x, breaks=("one_chain",)))


# ------------------------------------------------------------------------------------------------------------ what the layouts reach
def test_shape_cases_cover_the_edges():
    Ls = [s[6] for s in R.SHAPES]
    assert Ls == [1, 2, 31, 32, 33, 127, 128, 129, 160, 161, 255, 257]
    assert {s[1] for s in R.SHAPES} == {1, 3} and {s[3] for s in R.SHAPES} >= {1, 64}
    cins = {(s[4], s[5]) for s in R.SHAPES}
    assert {c for c, _ in cins} == {1, 3, 27, 4, 8, 28, 40, 44, 84}
    assert (8, 3) in cins and (28, 10) in cins                  # a channel quad that straddles the panels: C1 % 4 != 0 with Cin % 4 == 0
    assert {c1 for c, c1 in cins} >= {1} and any(c1 == c - 1 for c, c1 in cins) and any(c1 == c for c, c1 in cins)
    assert any(-(-L // R.PD_SB) == 5 for L in Ls)               # five buckets: the fourth bucket workgroup has none
    assert any(s[4] > 2 * R.PD_CH for s in R.SHAPES)            # three channel slabs
    for name, B, C, M, Cin, C1, L in R.SHAPES:
        g, pos, W, _, _ = R.dgrad_named(name)
        assert C * M < 24 or all((pos == v).any() for v in R.ignored(L)), name


def test_list_layouts_reach_what_they_name():
    stats, sizes = {}, {}
    for name in R.LISTS:
        g, pos, W, C1, L = R.dgrad_named(name)
        stats[name] = R.balanced_stats(pos, L) if W.shape[1] % 4 == 0 else None
        sizes[name] = (R.tile_sizes(pos, L), R.bucket_sizes(pos, L), pos, L)
    assert all(t.sum() == 0 for t in sizes["all_ignored"][0]) and set(np.unique(sizes["all_ignored"][2])) == set(R.ignored(257))
    assert sizes["first_bucket"][1][0][0] == 13 * 64 and sizes["last_bucket"][1][0][-1] == 13 * 64
    assert (sizes["last_column"][2] == 256).all()
    for n in (1, 15, 16, 17, 383, 384, 385, 769):
        assert [int(t[0]) for t in sizes["tile_%d" % n][0]] == [n] and stats["tile_%d" % n]["rounds"] == -(-n // R.PD5_R)
    assert stats["tile_17"]["lengths"] == {1, 2} and stats["tile_383"]["lengths"] == {23, 24} and stats["tile_15"]["lengths"] == {0, 1}
    assert stats["tile_385"]["ns"] == {384, 1} and stats["tile_769"]["rounds"] == 3
    st = stats["three_whole_chunks"]
    assert st["span"] == 5 and st["ns"] == {384}                # the end of a chunk, three whole chunks, the start of the next
    st = stats["run_ends_on_chunk_edge"]
    assert st["run_ends_on_edge"] and st["span"] >= 2
    pos = sizes["round_edge"][2]
    ids, cols, _ = R.lists(pos, 257)[0]
    assert cols[383] == cols[384] and stats["round_edge"]["crosses_round"] and stats["round_edge"]["ns"] == {384, 7}
    for n in (2047, 2048, 2049):
        b = sizes["cap_%d" % n][1][0]
        assert b[0] == n and (n > R.PS_CAP) == (n == 2049) and len(np.unique(sizes["cap_%d" % n][2][sizes["cap_%d" % n][2] < 32])) > 8
    for n in (127, 128, 129):
        tiles, buckets, pos, L = sizes["group_%d" % n]
        assert all(b[0] == n for b in buckets) and (n > R.PD_SQ) == (n == 129)
    ids, cols, _ = R.lists(sizes["group_129"][2], 32)[0]
    assert cols[127] == cols[128]                               # the column resumed in the second round of the one-channel kernel
    assert (sizes["pos_is_L"][2] == 130).any()


def test_large_cases_reach_both_scans_and_the_limits():
    want = {"large_L131072": (4, 0), "large_L131073": (1, 3), "large_L262112": (0, 4)}
    for name, (par, ser) in want.items():
        g, pos, W, C1, L = R.large_case(name)
        edges, sizes = R.quarter_edges(L)
        assert sum(0 < s <= R.PB_SCAN for s in sizes) == par and sum(s > R.PB_SCAN for s in sizes) == ser, (name, sizes)
        assert set(edges) <= set(pos.reshape(-1)) and len(edges) == 16 and W.shape[1] == 4 and g.shape[0] == 1
    assert R.L_MAX == 262112 and (2 * -(-R.L_MAX // R.PD_SB) + 1) * 4 <= 64 * 1024 < (2 * -(-(R.L_MAX + 1) // R.PD_SB) + 1) * 4
    g, pos, W, C1, L = R.large_case("wide_ids")
    assert g.shape[1] * g.shape[2] == 16383 * 64 < R.PD_KEY_IDS
    g, pos, W, C1, L = R.large_case("most_ids")
    assert g.shape[1] * g.shape[2] == R.PD_KEY_IDS - 1


def test_large_cases_are_exact_by_derivation():
    for name in [c[0] for c in R.LARGE]:
        g, pos, W, C1, L = R.large_case(name)
        assert (g * 8 == np.rint(g * 8)).all() and (np.abs(g) <= 0.5).all() and (g != 0).all()
        assert (W * 16 == np.rint(W * 16)).all() and (np.abs(W) <= 0.5).all()
        want, mag, n = R.dgrad64(g, pos, W, L)
        assert mag.max() / R.INT_GRANULE < 2 ** 24 and (want.astype(np.float32).astype(np.float64) == want).all()
        assert (want / R.INT_GRANULE == np.rint(want / R.INT_GRANULE)).all()


def test_matrix_core_cases_reach_every_instance_and_are_exact():
    shapes = [R.mfma_shape(B, C, Cin, L) for _, B, C, M, Cin, C1, L in R.MFMA]
    assert {s[0] for s in shapes} == {1, 2, 3, 4, 5, 6} and {s[1] for s in shapes} == {1, 2, 3, 4, 5, 7, 24}
    assert {s[2] for s in shapes} == {1, 2} and {s[0] for s in shapes if s[2] == 2} >= {1, 2}
    assert {c[6] for c in R.MFMA} == {2, 6, 8, 62, 64, 66, 130, 136} and {c[4] for c in R.MFMA} == {40, 64, 100, 128, 192, 256, 320, 384}
    assert any(c[4] % 32 and c[5] == 10 for c in R.MFMA)        # rows beyond Cin in the last 32-row tile; two panels with C1 = 10
    for name, B, C, M, Cin, C1, L in R.MFMA:
        ct = -(-Cin // 32)
        assert L % 2 == 0 and C % 16 == 0 and C * 2 + 16 <= R.PM_PITCH and ct % 2 == 0 and ct <= 12 and M <= L
        if B * Cin * L > 2e6:
            continue                                            # (the big-B cases share the builder; the small ones are walked)
        g, pos, W, _, _ = R.mfma_case(name, exact=True)
        assert R.same_bits(R.to_bf16(g), g) and R.same_bits(R.to_bf16(W), W) and 4 * M < 256          # every sum of <= M entries is k / 8, |k| <= 4 M
        ok = (pos >= 0) & (pos < L)
        pairs = np.stack(np.nonzero(ok)[:2] + (pos[ok],), axis=1)
        counts = np.unique(pairs, axis=0, return_counts=True)[1]
        assert counts.max() >= 2 and counts.max() <= 4
        want, mag, n = R.dgrad64(g, pos, W, L)
        assert (want.astype(np.float32).astype(np.float64) == want).all() and mag.max() / R.INT_GRANULE < 2 ** 24
        g, pos, W, _, _ = R.mfma_case(name, exact=False)
        ok = (pos >= 0) & (pos < L)
        pairs = np.stack(np.nonzero(ok)[:2] + (pos[ok],), axis=1)
        assert np.unique(pairs, axis=0, return_counts=True)[1].max() == 1
        assert not ok[B - 1].any() and (L < 130 or set(R.MFMA_EDGE_COLS) <= set(pos[0].reshape(-1)))


def test_wgrad_cases_cover_the_edges():
    assert {c[3] for c in R.WGRAD} == {1, 31, 32, 33, 63, 64} and {c[2] for c in R.WGRAD} >= {1, 5, 383, 384}
    assert {c[4] for c in R.WGRAD} >= {1, 15, 16, 17, 33} and {c[5] for c in R.WGRAD} >= {1, 3, 4, 7, 8, 9}
    assert any(c[4] > 2 * R.PW_ROWS for c in R.WGRAD)           # a third workgroup
    for rows in ("f32", "bf16"):
        L = R.wgrad_max_L(rows)
        assert R.wgrad_lds(L, rows) <= R.PW_LDS < R.wgrad_lds(L + 1, rows)
    name = R.WGRAD[4][0]
    g, pos, x, sc, sh = R.wgrad_named(name)
    L = x.shape[2]
    assert all((pos == v).any() for v in (-1, L, R.INT32_MIN, R.INT32_MAX)) and (pos[:, :, 0] == L // 2).all() and (pos[:, 3, 1:] == 0).all()
    pre = R.fma32(x[0, :2, :8], sc[:2, None], sh[:2, None])
    assert pre[0, 0] == 0 and not np.signbit(pre[0, 0]) and np.signbit(pre[0, 1]) and pre[0, 2] == np.float32(2.0 ** -149) and pre[0, 3] == -pre[0, 2]
    ties = pre[1, 4:8].view(np.uint32) & 0xFFFF
    assert (ties == 0x8000).all()                               # halfway between two bf16 numbers


# ------------------------------------------------------------------------------------------------------------ refusals of the C entries
INV, UNS = 1, 2


@pytest.fixture(scope="module")
def lib():
    from sonet_hip import _lib
    return _lib.load()


def host_ptr():
    buf = (ctypes.c_float * 64)()
    host_ptr.keep = buf
    return ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)


def test_sparse_dgrad_entries_refuse_before_a_launch(lib):
    from sonet_hip import _lib
    p = host_ptr()
    for fn in (lib.sonet_pooled_dgrad_f32, lib.sonet_pooled_dgrad_obf16):
        def call(g=p, pos=p, W=p, ws=p, gx1=p, gx2=p, B=1, C=16, M=4, C1=3, C2=5, L=64):
            return fn(g, pos, W, B, C, M, C1, C2, L, ws, gx1, gx2, None)
        for name in ("g", "pos", "W", "ws", "gx1"):
            assert call(**{name: None}) == INV and "NULL" in _lib.last_error(), name
        assert call(gx2=None) == INV and "gx2" in _lib.last_error()
        assert call(C2=0) == INV and "gx2" in _lib.last_error()
        for kw in (dict(B=0), dict(C=0), dict(M=0), dict(C1=0), dict(C2=-1), dict(L=0)):
            assert call(**kw) == INV and "non-positive" in _lib.last_error(), kw
        assert call(C=16384, M=64) == UNS and "2^20" in _lib.last_error()          # C * M = 2^20 (2^20 - 1 runs: tests/test_gpu_pooled_bwd.py)
        assert call(C=1024, M=1024) == UNS
        assert call(B=65536) == UNS
        assert call(L=R.L_MAX + 1) == UNS and "too large" in _lib.last_error()
    assert lib.sonet_pooled_dgrad_ws_size(0, 16, 4, 64) == 0 and lib.sonet_pooled_dgrad_ws_size(1, 16, 4, 0) == 0
    assert lib.sonet_pooled_dgrad_ws_size(2, 16, 4, 70) == 2 * (64 * 12 + 4 * 4)


def test_matrix_core_entry_refuses_before_a_launch(lib):
    from sonet_hip import _lib
    p = host_ptr()

    def call(g=p, pos=p, wt=p, ws=p, gx1=p, gx2=p, B=1, C=16, M=4, C1=10, C2=30, L=64):
        return lib.sonet_pooled_dgrad_mfma_bf16(g, pos, wt, B, C, M, C1, C2, L, ws, gx1, gx2, None)
    for name in ("g", "pos", "wt", "ws", "gx1"):
        assert call(**{name: None}) == INV and "NULL" in _lib.last_error(), name
    assert call(gx2=None) == INV
    for kw in (dict(L=63), dict(C=24), dict(C1=10, C2=60), dict(C1=10, C2=430), dict(C=400), dict(gx1=ctypes.c_void_p(p.value + 2)),
               dict(gx2=ctypes.c_void_p(p.value + 2)), dict(C=16384, M=64), dict(L=R.L_MAX + 2)):
        assert call(**kw) == UNS and "not supported" in _lib.last_error(), kw          # L odd, C % 16, CT = 3, CT = 14, C = 400, outputs 2 bytes off


def test_wgrad_entries_refuse_before_a_launch(lib):
    from sonet_hip import _lib
    p = host_ptr()
    for rows, plain, xaff in (("f32", lib.sonet_pooled_wgrad_f32, lib.sonet_pooled_wgrad_xaff_f32),
                              ("bf16", lib.sonet_pooled_wgrad_xbf16, lib.sonet_pooled_wgrad_xaff_xbf16)):
        def call(g=p, pos=p, x=p, out=p, B=1, C=16, M=4, Ci=3, L=64):
            return plain(g, pos, x, B, C, M, Ci, L, out, None)

        def callx(g=p, pos=p, x=p, out=p, xs=p, xh=p, B=1, C=16, M=4, Ci=3, L=64):
            return xaff(g, pos, x, B, C, M, Ci, L, out, xs, xh, 1, None)
        for name in ("g", "pos", "x", "out"):
            assert call(**{name: None}) == INV and "NULL" in _lib.last_error(), name
        for name in ("g", "pos", "x", "out", "xs", "xh"):
            assert callx(**{name: None}) == INV and "NULL" in _lib.last_error(), name
        for c in (call, callx):
            for kw in (dict(B=0), dict(C=0), dict(M=0), dict(Ci=0), dict(L=0), dict(B=65536)):
                assert c(**kw) == INV and "bad size" in _lib.last_error(), kw
            assert c(M=R.PW_M + 1) == UNS and c(C=R.PW_CMAX + 1) == UNS
            assert c(L=R.wgrad_max_L(rows) + 1) == UNS and "LDS" in _lib.last_error()          # the first L past the LDS budget
