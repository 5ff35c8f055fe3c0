"""The host restatement of the weight packs (tests/pack_ref.py) held to itself, to the library's size functions and to its own deliberate
breaks -- no device.  tests/test_gpu_packs.py and tests/test_gpu_pack_registry.py hold the kernels to the restatement."""
import ctypes

import numpy as np
import pytest

import pack_ref as R

CINS = (1, 15, 16, 17, 127, 128, 129, 387, 768)
COUTS = (1, 31, 32, 33, 96)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


# ---- the restatement against itself --------------------------------------------------------------------------------------------------
def test_x3_pieces_sum_to_the_weight_exactly_below_the_resplit_threshold():
    """h + m + l == w in float64 for every finite w whose bf16 rounding is finite: ordinary weights, the finite edge values, and 2^e (1 + u)
    over the whole normal range.  (Three bf16 pieces hold 24 significant bits unless the low pieces fall below the subnormal spacing.)"""
    rng = np.random.default_rng(1)
    v = np.concatenate([R.weights("ordinary", 96, 129).reshape(-1), R._f(R.EDGE_FINITE_BITS),
                        np.ldexp(1.0 + rng.random(4096), rng.integers(-100, 127, 4096)).astype(np.float32) * rng.choice([-1.0, 1.0], 4096).astype(np.float32)])
    v = v[(_bits(v) & 0x7FFFFFFF) < R.BF16_OVERFLOW_BITS]
    h, m, l = (R.bf16_value(p).astype(np.float64) for p in R.split3_w(v))
    assert np.array_equal(h + m + l, v.astype(np.float64))


def test_x3_weight_side_fix_at_and_above_the_resplit_threshold():
    """From 0x7F7F8000 on the high piece is the largest finite bf16 of the sign and the pieces still sum to the weight; an infinity is the l
    piece alone; the value just below keeps the plain split."""
    v = R._f(R._both_signs([R.BF16_OVERFLOW_BITS, R.BF16_OVERFLOW_BITS + 1, R.FLT_MAX_BITS]))
    h, m, l = R.split3_w(v)
    assert ((h & 0x7FFF) == 0x7F7F).all() and ((h >> 15) == (_bits(v) >> 31)).all()
    assert np.array_equal(sum(R.bf16_value(p).astype(np.float64) for p in (h, m, l)), v.astype(np.float64))
    h, m, l = R.split3_w(R._f(R.INF_BITS))
    assert (h == 0).all() and (m == 0).all() and list(l) == [0x7F80, 0xFF80]
    h, m, l = R.split3_w(R._f([R.BF16_OVERFLOW_BITS - 1]))
    assert h[0] == 0x7F7F and R.bf16_value(h)[0].astype(np.float64) + R.bf16_value(m)[0] + R.bf16_value(l)[0] == float(R._f([R.BF16_OVERFLOW_BITS - 1])[0])


def test_h3_pieces_reproduce_the_clamped_weight_within_the_derived_bound():
    """h + res / 32 within 2^-22 relative of clamp(w, +-65504) (csrc/pointmlp_x3.hip: "dropped terms and the rounding of the scaled residuals
    <= 2^-22 relative"): |w - h| <= 2^-11 |w|, so |res| <= 2^-6 |w| and its fp16 rounding errs by 2^-11 relative, 2^-17 |w|, a 32nd of which is
    2^-22 |w| -- while res is an fp16 NORMAL.  A subnormal res errs by up to 2^-25 absolute instead, 2^-30 on w (ops.h3_weight_ok's "e"), which
    is below 2^-22 |w| from |w| = 2^-8 on: H3_COLUMN_MIN.  So: 2^-22 relative for |w| >= 2^-8, 2^-30 absolute below; the clamp at and beyond
    65504."""
    rng = np.random.default_rng(2)
    v = np.concatenate([R.weights("ordinary", 96, 129).reshape(-1),
                        np.ldexp(1.0 + rng.random(4096), rng.integers(-14, 16, 4096)).astype(np.float32) * rng.choice([-1.0, 1.0], 4096).astype(np.float32),
                        R._f(R._both_signs([R.B65504 - 1, R.B65504, R.B65504 + 1, 0x47C35000, 0x477FF000, R.FLT_MAX_BITS]))])
    v = v[np.abs(v) >= 2.0 ** -14]
    h, res = R.split_h3(v)
    got = R.f16_value(h).astype(np.float64) + R.f16_value(res).astype(np.float64) / 32.0
    want = np.clip(v.astype(np.float64), -65504.0, 65504.0)
    assert np.isfinite(got).all()
    big = np.abs(want) >= 2.0 ** -8
    assert big.sum() > 4000 and (~big).sum() > 1000
    assert (np.abs(got - want)[big] <= 2.0 ** -22 * np.abs(want)[big]).all()
    assert (np.abs(got - want)[~big] <= 2.0 ** -30).all()


@pytest.mark.parametrize("flavour", ["bf16", "x3", "h3", "h3p"])
@pytest.mark.parametrize("Cin,Cout", [(17, 33), (129, 31), (15, 96)])
def test_unpacking_returns_the_pieces_at_their_documented_position(flavour, Cin, Cout):
    W = R.weights("edge", Cout, Cin, 3)
    got = R.unpack16(R.PACKS[flavour](W), flavour, Cin, Cout)
    P, _ = R.padded(W, pad_rows=64 if flavour == "h3p" else 32)
    P = np.pad(P, ((0, 0), (0, got.shape[2] - P.shape[1])))
    want = {"bf16": lambda: (R._hi16(R.bf16(P)),), "x3": lambda: R.split3_w(P), "h3": lambda: R.split_h3(P), "h3p": lambda: R.split_h3p(P)}[flavour]()
    assert got.shape == (len(want),) + P.shape
    for s, piece in enumerate(want):
        assert np.array_equal(got[s], piece), (flavour, s)
    # rows and K chunks that do not exist are zero bytes
    assert not got[:, Cout:, :].any() and not got[:, :, Cin:].any()


def test_f32_pack_holds_every_element_once_and_zeros_elsewhere():
    W = R.weights("edge_nan", 33, 17, 4)
    p = R.pack_f32(W).view(np.uint32).reshape(2, 3, 64, 4)
    for o in (0, 31, 32):
        for c in (0, 1, 7, 8, 16):
            assert p[o // 32, c // 8, 32 * (c % 2) + o % 32, (c % 8) // 2] == _bits(W)[o, c]
    assert sorted(p[p != 0].tolist()) == sorted(_bits(W)[_bits(W) != 0].tolist())


def test_strided_matrix_is_the_pack_of_the_transposed_block():
    """The ``_strided`` description (rows, rs, cs, padded Cout) of a column block of W transposed equals the pack of the copy."""
    W = R.weights("edge", 40, 50, 5)
    lo, Ci, Cp = 7, 35, 64
    copy = np.zeros((Cp, 40), dtype=np.float32)
    copy[:Ci] = W[:, lo:lo + Ci].T
    for flavour in ("bf16", "x3", "h3"):
        got = R.PACKS[flavour](W.reshape(-1)[lo:], Cin=40, Cout=Cp, rows=Ci, rs=1, cs=50)
        assert np.array_equal(got, R.PACKS[flavour](copy)), flavour


def test_trailer_orders_nan_above_inf_above_finite_in_either_sign():
    for vals, want in (([0.5, -8.0, 3.0], 0x41000000), ([1.0, -np.inf], 0x7F800000), ([np.inf, -1.0], 0x7F800000), ([-0.0, 0.0], 0)):
        W = np.array([vals], dtype=np.float32)
        assert R.amax_bits(*R.padded(W)) == want
    for nan in (0x7FC01234, 0xFFC00001):
        W = R._f([[0x7F800000, nan, 0xFF800000]])
        assert (R.amax_bits(*R.padded(W)) & 0x7FFFFFFF) > 0x7F800000
    t = R.pack_x3(np.array([[0.5, -8.0]], dtype=np.float32))[-64:].view(np.uint32)
    assert t[0] == 0x41000000 and not t[1:].any()


# ---- sizes and table fields ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", CINS)
def test_sizes_and_chunk_counts_equal_the_library(Cin):
    from sonet_hip import _lib
    lib = _lib.load()
    for Cout in COUTS:
        assert lib.sonet_pointmlp_pack_size(Cin, Cout) * 4 == R.pack_size("f32", Cin, Cout)
        assert lib.sonet_pointmlp_bf16_pack_size(Cin, Cout) == R.pack_size("bf16", Cin, Cout)
        assert lib.sonet_pointmlp_x3_pack_size(Cin, Cout) == R.pack_size("x3", Cin, Cout) == R.pack_size("h3", Cin, Cout)
        assert lib.sonet_pointmlp_h3p_pack_size(Cin, Cout) == R.pack_size("h3p", Cin, Cout)
        W = R.weights("ordinary", Cout, Cin)
        for flavour in R.PACKS:
            assert R.PACKS[flavour](W).size == R.written_size(flavour, Cin, Cout) <= R.pack_size(flavour, Cin, Cout), (flavour, Cout)
    for fl, flavour in enumerate(R.FLAVOURS):
        assert lib.sonet_pack_multi_kc(fl, Cin) == R.chunks(flavour, Cin), flavour
    assert R.chunks("h3", 128) == 8 and R.chunks("h3", 129) == 16


def test_table_records():
    """Field by field against the struct documented in include/sonet_hip.h, read back with ctypes."""
    class Entry(ctypes.Structure):
        _fields_ = [("W", ctypes.c_void_p), ("Wp", ctypes.c_void_p), ("rs", ctypes.c_longlong), ("cs", ctypes.c_longlong), ("total", ctypes.c_longlong),
                    ("Cin", ctypes.c_int), ("rows", ctypes.c_int), ("KC", ctypes.c_int), ("flavour", ctypes.c_int), ("blk0", ctypes.c_int),
                    ("nblk", ctypes.c_int), ("pad", ctypes.c_longlong)]
    assert ctypes.sizeof(Entry) == 72
    entries = [dict(src=0x7F0000001000, dst=0x7F0000100000, rs=387, cs=1, Cin=387, rows=512, Cout=512, flavour="h3"),
               dict(src=0x7F0000002004, dst=0x7F0000200000, rs=1, cs=387, Cin=512, rows=3, Cout=32, flavour="x3"),
               dict(src=0x7F0000003000, dst=0x7F0000300000, rs=16, cs=1, Cin=16, rows=32, Cout=32, flavour="bf16")]
    tab, blocks = R.pack_table(entries)
    assert tab.dtype == np.uint8 and tab.size == 3 * 72
    got = (Entry * 3).from_buffer_copy(tab.tobytes())
    want = [(64 * 16 * 32, 32, 2, 0, 128), (64 * 1 * 32, 32, 1, 128, 8), (64, 1, 0, 136, 1)]
    for g, e, (total, kc, fl, blk0, nblk) in zip(got, entries, want):
        assert (g.W, g.Wp, g.rs, g.cs, g.Cin, g.rows) == (e["src"], e["dst"], e["rs"], e["cs"], e["Cin"], e["rows"])
        assert (g.total, g.KC, g.flavour, g.blk0, g.nblk, g.pad) == (total, kc, fl, blk0, nblk, 0)
    assert blocks == 137


# ---- breaks --------------------------------------------------------------------------------------------------------------------------
def _transposed_block():
    """A block as ``_pack_transposed`` asks for it: lo > 0, Ci < Cp, and larger weights next to the block than inside it."""
    W = R.weights("ordinary", 48, 40, 6)
    W[:, 30:] *= 16.0
    return dict(W=W.reshape(-1)[5:], Cin=48, Cout=32, rows=20, rs=1, cs=40)


BREAK_CASES = [("swap_halves", "f32"), ("swap_halves", "bf16"), ("swap_halves", "x3"), ("swap_halves", "h3"), ("swap_halves", "h3p"),
               ("term_order", "x3"), ("term_order", "h3"), ("term_order", "h3p"), ("kc_for_kcp", "h3"), ("kc_for_kcp", "h3p"),
               ("rows_is_cout", "bf16"), ("rows_is_cout", "x3"), ("rows_is_cout", "h3"), ("trailer_padded", "x3"), ("trailer_padded", "h3")]


@pytest.mark.parametrize("brk,flavour", BREAK_CASES)
def test_each_break_of_the_restatement_is_seen(brk, flavour):
    assert brk in R.BREAKS
    if brk in ("rows_is_cout", "trailer_padded"):
        a = _transposed_block()
    else:
        a = dict(W=R.weights("ordinary", 33, 17, 7))
    good, bad = R.PACKS[flavour](**a), R.PACKS[flavour](**a, **{brk: True})
    assert good.shape != bad.shape or not np.array_equal(good, bad)
    if brk == "trailer_padded":                                  # only the trailer's word 0 moves
        assert np.array_equal(good[:-64], bad[:-64]) and good[-64:].view(np.uint32)[0] < bad[-64:].view(np.uint32)[0]
    if brk == "kc_for_kcp":
        assert bad.size < good.size


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_pack_entries_refuse_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sonet_pack_multi(None, 1, 1, None) == 1 and "NULL" in _lib.last_error()
    assert lib.sonet_pack_multi(p, 0, 1, None) == 1 and "empty" in _lib.last_error()
    assert lib.sonet_pack_multi(p, -1, 1, None) == 1
    assert lib.sonet_pack_multi(p, 1, 0, None) == 1 and "empty" in _lib.last_error()
    assert lib.sonet_pack_multi(p, 1, -5, None) == 1
    for name in ("sonet_pointmlp_x3_pack_strided", "sonet_pointmlp_h3_pack_strided", "sonet_pointmlp_bf16_pack_strided"):
        fn = getattr(lib, name)
        assert fn(p, 4, 1, p, 4, 32, 0, None) == 1, name
        assert fn(p, 4, 1, p, 4, 32, -1, None) == 1, name
        assert fn(p, 4, 1, p, 4, 32, 33, None) == 1 and "rows" in _lib.last_error(), name
        assert fn(None, 4, 1, p, 4, 32, 4, None) == 1, name
