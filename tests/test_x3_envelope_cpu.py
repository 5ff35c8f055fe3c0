"""CPU pin of the bf16-split ("x3") arithmetic: a float64 model of the split (tests/x3_model.py) stays within 0.5e-5 of float64 on every
operand family over the interval of magnitudes ``derived_interval`` finds -- half of the project's 1e-5, the other half is left to the
kernels' f32 accumulation (tests/test_gpu_x3_envelope.py runs the kernels on the same families) -- and leaves it one power of four below.

The 1e-5 gate cannot see a wrong low-order piece (a dropped product is 1e-5 ... 3e-5 at the maximum over 131 k outputs, less on small
shapes).  The GPU file therefore carries two sharper gates, bit-exact piece identities and ``tight_gate``; here each of six deliberately
broken models is fed through them and must turn one red."""
import struct

import numpy as np
import pytest

import x3_model as X

N_SMALL = 256                           # columns of the reachability runs (the GPU shapes are this small)


def _f(bits):
    return np.float32(struct.unpack("<f", struct.pack("<I", bits))[0])


def test_bf16_rounding_overflows_from_0x7F7F8000_and_the_split_turns_it_into_nan():
    """Finding 3 of docs/findings.md "x3 envelope": h = bf16(v) is inf from 0x7F7F8000 on, v - h is inf - inf or finite - inf, and the
    lower pieces are NaN -- for +-inf and for the finite values above 3.3895e38 alike."""
    below, at = _f(X.BF16_OVERFLOW_BITS - 1), _f(X.BF16_OVERFLOW_BITS)
    assert np.isfinite(X.bf16(np.array([below, -below]))).all()
    assert np.isinf(X.bf16(np.array([at, -at]))).all() and np.isfinite(at)
    h, m, l = X.split3(np.array([below, -below], dtype=np.float32))
    assert np.isfinite(h).all() and np.isfinite(m).all() and np.isfinite(l).all()
    assert (h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64) == np.array([below, -below], dtype=np.float64)).all()
    bad = np.array([at, -at, np.finfo(np.float32).max, np.inf, -np.inf], dtype=np.float32)
    h, m, l = X.split3(bad)
    assert np.isinf(h).all() and (np.sign(h) == np.sign(bad)).all()
    assert np.isnan(m[3:]).all() and np.isnan(l[3:]).all()                # inf - inf
    assert np.isinf(m[:3]).all() and (np.sign(m[:3]) == -np.sign(bad[:3])).all() and np.isnan(l[:3]).all()     # finite - inf, then -inf + inf
    h, m, l = X.split3(np.array([np.nan], dtype=np.float32))
    assert np.isnan(h).all() and np.isnan(m).all() and np.isnan(l).all()


def test_pieces_of_22_bit_values_sum_exactly_in_every_order():
    """What the piece identities rest on: with the low two bits of the significand cleared, h + m + l is exact in f32 whichever way round
    the accumulator meets the three products, and most values do have a third piece."""
    import itertools
    rng = np.random.default_rng(11)
    v = X.bits22((rng.standard_normal(100000) * np.exp(rng.uniform(-3, 3, 100000))).astype(np.float32))
    p = X.split3(v)
    for order in itertools.permutations(range(3)):
        s = (p[order[0]] + p[order[1]]) + p[order[2]]                     # float32 adds
        assert s.dtype == np.float32 and (s == v).all(), order
    assert float((p[2] != 0).mean()) > 0.8
    # ... and with all 24 bits it is not: the reason for the 22
    w = (rng.standard_normal(600000)).astype(np.float32)
    q = X.split3(w)
    assert any((((q[o[0]] + q[o[1]]) + q[o[2]]) != w).any() for o in itertools.permutations(range(3)))


def test_interval_is_derived_and_the_model_leaves_the_cap_one_power_of_four_below_it():
    lo, hi = X.derived_interval()
    print("x3 envelope: derived interval [2^%d, 2^%d]" % (lo, hi))
    assert lo < -60 and hi > 60 and lo % 2 == 0 and hi % 2 == 0
    assert X.end_ok(lo) and X.end_ok(hi)
    assert not X.end_ok(lo - 2)
    assert not X.end_ok(hi + 2, X.scale_fits)
    for e in (lo, lo - 2, lo - 4):
        for K in X.KS:
            for tag, (a, b) in (("x", (e, 0)), ("W", (0, e))):
                W, x, _ = X.family("u(%d,%d)" % (a, b), K)
                ref = X.exact(W, x)
                print("x3 envelope: %s scaled by 2^%d, K=%d: kept %.3g  flushed %.3g" % (tag, e, K, X.rms_error(X.model(W, x), ref),
                                                                                       X.rms_error(X.model(W, x, True), ref)))


@pytest.mark.parametrize("K", X.KS)
def test_model_meets_half_the_bound_on_every_family(K):
    lo, _ = X.derived_interval()
    for name in X.family_names(lo):
        W, x, metric = X.family(name, K)
        assert X.admitted(W, x), name
        ref = X.exact(W, x)
        e = X.model_error(W, x, metric)
        print("x3 envelope K=%d %-14s %.3g" % (K, name, e))
        assert e <= X.CAP, (name, e)
        # nothing for the GPU gates to exclude: no output below the normal range, exact zeros only under the sparse family's zero columns
        assert np.isfinite(ref.astype(np.float32)).all(), name
        small = np.abs(ref) < X.TINY
        if name == "sparse":
            zc = X.zero_columns(x)
            assert zc.size > 0 and (ref[:, zc] == 0).all()
            small[:, zc] = False
        assert not small.any(), name


@pytest.mark.parametrize("K", X.KS)
def test_model_satisfies_the_piece_identities_bit_for_bit(K):
    for name, W, x, expect in X.identities(K, X.COUT, N_SMALL):
        for flush in (False, True):
            assert np.array_equal(X.model(W, x, flush), expect.astype(np.float64)), (name, flush)
        if name.startswith("id-mm"):
            assert float((X.split3(x)[1] != 0).mean()) > 0.8 and not X.split3(x)[2].any()
            assert float((X.split3(W[W != 0])[1] != 0).mean()) > 0.8 and not X.split3(W)[2].any()
        elif name.startswith("id-x"):
            assert float((X.split3(x)[2] != 0).mean()) > 0.8                # the third piece is there to be lost
        else:
            assert float((X.split3(W)[2] != 0).mean()) > 0.8


def _gates(f):
    """Feed f(W, x) -> float64 through the GPU file's two sharp gates -> the names of the gates it fails."""
    red = []
    for K in X.KS:
        for name, W, x, expect in X.identities(K, X.COUT, N_SMALL):
            if not np.array_equal(f(W, x), expect.astype(np.float64)):
                red.append("%s K=%d" % (name, K))
        for name in X.TIGHT_FAMILIES:
            W, x, metric = X.family(name, K, X.COUT, N_SMALL)
            ref = X.exact(W, x)
            e_f32 = X.error(X._mm(W, x), ref, metric)                        # an f32 GEMM of the same operands
            if not X.tight_gate(X.error(f(W, x), ref, metric), e_f32, X.model_error(W, x, metric)):
                red.append("tight %s K=%d" % (name, K))
    return red


def test_the_unbroken_model_passes_both_gates():
    assert _gates(X.model) == []


BREAKS = [(t, X.model_without(t)) for t in X.DROPPABLE] + [("l swapped in x", X.model_swapped_l("x")), ("l swapped in W", X.model_swapped_l("W"))]


@pytest.mark.parametrize("what,f", BREAKS, ids=[b[0].replace(" ", "_") for b in BREAKS])
def test_every_deliberate_break_turns_a_gate_red(what, f):
    red = _gates(f)
    print("x3 envelope: %-16s fails %d gates: %s" % (what, len(red), ", ".join(red[:6])))
    assert red, what
    # which gate pins which piece: identity "x" the three x pieces against Wh, identity "W" the three W pieces against xh, identity "mm" (and,
    # where K is small enough for 4 e_f32 to stay below the dropped product, the tight gate) Wm.xm
    want = {"WhXm": "id-x", "WhXl": "id-x", "WmXh": "id-W", "WlXh": "id-W", "WmXm": "id-mm", "l swapped in x": "id-x", "l swapped in W": "id-W"}[what]
    assert any(r.startswith(want) for r in red), (what, red)
    assert any(r.startswith("tight") for r in red), (what, red)
    # ... and how the same break looks to the 1e-5 gate on a shape of this size
    W, x, _ = X.family("u(0,0)", 64, X.COUT, N_SMALL)
    print("x3 envelope: %-16s on u(0,0), K=64, %d outputs: error %.3g against the 1e-5 gate" % (what, X.COUT * N_SMALL, X.rms_error(f(W, x), X.exact(W, x))))
