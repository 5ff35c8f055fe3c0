"""The fused Chamfer loss without a GPU: the numpy restatement (tests/chamfer_ref.py) against the fixtures of the live reference
(tests/golden/chamfer, tools/make_chamfer_golden.py) and against float64 autograd of the reference's expression; that the gradient
gate of tests/test_gpu_chamfer_loss.py is reachable by an f32-element kernel and sees two plausible mistakes; the reference's own f32
rounding; the C entries' argument checks; what the wrappers refuse before a device is needed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import chamfer_ref as R

CASES = R.GOLDEN_CASES
# worst |reference f32 gradient - float64 restatement| / (2^-24 sum|term|) that tools/make_chamfer_golden.py --check printed over the
# three fixtures (lattice_ties); the gate below is twice that.  The reference's own rounding, measured on the reference.
REFERENCE_GRAD_GAP = 3.375


def _fixture_inputs():
    out = [(c, golden("chamfer/" + c)) for c in CASES]
    return [(c, g["pred"], g["gt"], g["nn_pg"], g["nn_gp"]) for c, g in out]


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference_fixtures(case):
    g = golden("chamfer/" + case)
    pred, gt = g["pred"], g["gt"]
    assert pred.dtype == gt.dtype == np.float32 and g["nn_pg"].dtype == g["nn_gp"].dtype == np.int32
    t = R.terms(pred, gt)
    assert np.array_equal(t["nn_pg"], g["nn_pg"]) and np.array_equal(t["nn_gp"], g["nn_gp"])
    assert R.ulps(t["elem_fwd"], g["elem_fwd"]).max() <= 3 and R.ulps(t["elem_bwd"], g["elem_bwd"]).max() <= 3
    ls = R.losses(t)
    for k in ("forward_loss", "backward_loss"):
        assert abs(ls[k] - float(g[k])) <= 2e-6 * float(g[k]), (k, ls[k], float(g[k]))
    for k in ("forward_loss_array", "backward_loss_array", "loss_array"):
        np.testing.assert_allclose(ls[k], g[k], rtol=5e-6, err_msg=k)
    # the exactly rounded sums are what np.sum gives in float64 to n * 2^-53
    for d, e in enumerate((t["elem_fwd"], t["elem_bwd"])):
        s = e.astype(np.float64).sum(axis=1)
        assert (np.abs(s - t["sums"][:, d]) <= e.shape[1] * 2.0 ** -53 * t["sums"][:, d]).all()


def test_fixture_families_pin_what_they_are_named_for():
    g = golden("chamfer/continuous_b3_m257_n1000")
    assert g["pred"].shape == (3, 3, 257) and g["gt"].shape == (3, 3, 1000)
    g = golden("chamfer/lattice_ties")
    d = np.sort(R.E.dist_f32(g["pred"], g["gt"]), axis=2)
    assert (d[:, :, 0] == d[:, :, 1]).mean() > 0.3                               # exact ties for the nearest neighbour are common
    g = golden("chamfer/coincident_half")
    assert (g["elem_fwd"][:, ::2] == np.float32(1e-4)).all()                     # the floor of robust_norm
    assert np.isfinite(g["grad_predicted"]).all()                                # no NaN from 0 / 1e-4
    _, mag = R.grad(g["pred"], g["gt"], g["nn_pg"], g["nn_gp"], gb=0.0)
    assert (mag[:, :, ::2] == 0).all() and (mag[:, :, 1::2] > 0).any()           # forward terms of exactly zero
    for c in CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "chamfer", c + ".npz")) < 100 * 1024


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="reference checkout not mounted")
def test_fixtures_regenerate_from_the_live_reference():
    """tools/make_chamfer_golden.py --check in its own process (the reference's package names are the product's)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_chamfer_golden.py"), "--check"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "fixtures regenerate bit-identically" in out and out.count("reference gradient gap") == len(CASES)
    worst = max(float(line.split("gap ")[1].split(" x")[0]) for line in out.splitlines() if "reference gradient gap" in line)
    assert abs(worst - REFERENCE_GRAD_GAP) < 5e-4, worst                         # the figure the gate below is made from


def _seeded_cases():
    """(name, pred, gt, nn_pg, nn_gp) at every shape of the GPU gradient test: continuous data, lattice data at every other shape with
    N >= 256 (on a lattice gt of a few points every term can be exactly zero: nothing for a gate to see)."""
    out = []
    for k, (M, N) in enumerate(R.GRAD_SHAPES):
        for B in (1, 3):
            kind = "lattice" if (k + B) % 2 and N >= 256 else "continuous"
            pred, gt = R.make(kind, B, M, N)
            out.append(("%s B%d M%d N%d" % (kind, B, M, N), pred, gt) + R.indices(pred, gt))
    for M, N in ((300, 1025), (7, 1025)):
        pred, gt = R.one_owner(2, M, N, 77 + M)
        out.append(("one owner M%d N%d" % (M, N), pred, gt) + R.indices(pred, gt))
    return out


SEEDED = None


def seeded():
    global SEEDED
    if SEEDED is None:
        SEEDED = _seeded_cases()
    return SEEDED


def test_restatement_gradient_equals_float64_autograd_at_forced_indices():
    worst = 0.0
    for name, pred, gt, nn_pg, nn_gp in _fixture_inputs() + seeded()[::5]:
        for gf, gb in ((1.0, 1.0), (0.7, -1.3), (0.0, 2.0), (1.5, 0.0)):
            got, _ = R.grad(pred, gt, nn_pg, nn_gp, gf, gb)
            want = R.autograd64(pred, gt, nn_pg, nn_gp, gf, gb)
            worst = max(worst, R.rel_rms(got, want))
            assert R.rel_rms(got, want) <= 1e-12, (name, gf, gb, R.rel_rms(got, want))
    # forced indices that are NOT the nearest neighbours: the gradient is defined by the indices alone
    name, pred, gt, nn_pg, nn_gp = seeded()[8]
    r = np.random.default_rng(3)
    f_pg, f_gp = r.integers(0, gt.shape[2], nn_pg.shape).astype(np.int32), r.integers(0, pred.shape[2], nn_gp.shape).astype(np.int32)
    assert R.rel_rms(R.grad(pred, gt, f_pg, f_gp)[0], R.autograd64(pred, gt, f_pg, f_gp)) <= 1e-12
    print("restatement vs float64 autograd: worst relative rms %.3g" % worst)


def _gap(pred, gt, nn_pg, nn_gp, gf, gb, **mistake):
    """worst |f32(model gradient) - ref64| / sum|term| over the entries with a term; the model divides by the f32 elements."""
    ref64, mag = R.grad(pred, gt, nn_pg, nn_gp, gf, gb)
    model = R.grad(pred, gt, nn_pg, nn_gp, gf, gb, elems="f32", **mistake)[0].astype(np.float32).astype(np.float64)
    nz = mag > 0
    assert (model[~nz] == 0).all() or mistake
    return float((np.abs(model - ref64)[nz] / mag[nz]).max()) if nz.any() else 0.0


def test_f32_element_model_stays_inside_the_gate_and_the_gate_sees_mistakes():
    """The GPU gate |dpred - ref64| <= 6.4 x 2^-24 sum|term| (chamfer_ref.GATE, inside 2^-21): an f32-element, float64-accumulating, once-rounding kernel
    -- the restatement's model of it -- stays inside on every fixture and at every GPU test shape; dropping the backward-direction
    terms, or scaling them by gf instead of gb, leaves it on every seeded case that has a backward term."""
    worst = 0.0
    for name, pred, gt, nn_pg, nn_gp in _fixture_inputs() + seeded():
        for gf, gb in ((1.0, 1.0), (0.7, -1.3)):
            v = _gap(pred, gt, nn_pg, nn_gp, gf, gb)
            worst = max(worst, v)
            assert v <= R.GATE, (name, gf, gb, v / R.GATE)
    print("f32-element model: worst gap %.4f x 2^-24 sum|term| (gate %.1f)" % (worst / 2.0 ** -24, R.GATE / 2.0 ** -24))
    # the derived bound is 2^-22 = 4 x 2^-24; the model shows 3.173 x 2^-24 (docs/findings.md), and the gate is twice 3.2 x 2^-24
    assert worst <= 3.2 * 2.0 ** -24 and R.GATE == 6.4 * 2.0 ** -24
    seen = 0
    for name, pred, gt, nn_pg, nn_gp in seeded():
        if not (R.grad(pred, gt, nn_pg, nn_gp, 0.0, 1.0)[1] > 0).any():
            # every gt point coincides with its nearest predicted point (a dense lattice): the backward terms are exactly zero, and a
            # gradient without them is the right one.  Never a continuous cloud.
            assert name.startswith("lattice"), name
            continue
        seen += 1
        assert _gap(pred, gt, nn_pg, nn_gp, 0.7, -1.3, drop_backward=True) > R.GATE, name
        assert _gap(pred, gt, nn_pg, nn_gp, 0.7, -1.3, gb_is_gf=True) > R.GATE, name
    assert seen >= 0.9 * len(seeded()), (seen, len(seeded()))


@pytest.mark.parametrize("case", CASES)
def test_reference_f32_gradient_against_the_float64_restatement(case):
    """The reference's own rounding (f32 autograd on the CPU), measured on the reference: twice the worst value --check printed."""
    g = golden("chamfer/" + case)
    ref64, mag = R.grad(g["pred"], g["gt"], g["nn_pg"], g["nn_gp"])
    gap = np.abs(g["grad_predicted"].astype(np.float64) - ref64)
    nz = mag > 0
    assert (gap[~nz] == 0).all()
    worst = float((gap[nz] / (2.0 ** -24 * mag[nz])).max())
    print("%s: reference gradient gap %.3f x 2^-24 sum|term|" % (case, worst))
    assert worst <= 2 * REFERENCE_GRAD_GAP


def test_c_entries_reject_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def loss(B=1, M=2, N=4, **null):
        names = ("pred", "gt", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "sums", "ws")
        a = [None if null.get(k) else p for k in names]
        return lib.sonet_chamfer_loss_f32(*a, B, M, N, None)

    def grad(B=1, M=2, N=4, **null):
        names = ("pred", "gt", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "gscale", "dpred", "bad")
        a = [None if null.get(k) else p for k in names]
        return lib.sonet_chamfer_grad_f32(*a, B, M, N, None)

    for name in ("pred", "gt", "sums", "ws"):
        assert loss(**{name: True}) == 1 and "NULL" in _lib.last_error(), name
    for name in ("pred", "gt", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "gscale", "dpred", "bad"):
        assert grad(**{name: True}) == 1 and "NULL" in _lib.last_error(), name
    for fn in (loss, grad):
        for kw in (dict(B=0), dict(M=0), dict(N=0), dict(B=-1), dict(M=-3), dict(N=-5)):
            assert fn(**kw) == 1 and "non-positive" in _lib.last_error(), (fn.__name__, kw)
        assert fn(B=65536) == 2 and "B=65536" in _lib.last_error(), fn.__name__
    # the optional outputs of the loss entry are optional: with bad sizes the size check answers, not the NULL check
    assert loss(nn_pg=True, nn_gp=True, elem_fwd=True, elem_bwd=True, B=0) == 1 and "non-positive" in _lib.last_error()
    ws = lib.sonet_chamfer_loss_ws_size
    assert ws(0, 4, 4) == 0 and ws(2, 0, 8) == 0 and ws(2, 8, -1) == 0
    assert ws(1, 1, 1) == 2 * 8 and ws(3, 257, 256) == 3 * (2 + 1) * 8 and ws(2, 1280, 5000) == 2 * (5 + 20) * 8


def test_wrappers_refuse_before_a_device_is_needed():
    from models import losses as LS
    from sonet_hip import metrics, ops
    from sonet_hip._lib import SonetHipError
    pred, gt = torch.zeros(2, 3, 8), torch.zeros(2, 3, 16)
    for fn in (ops.chamfer_terms, ops.chamfer_loss, metrics.ChamferEvaluator().update):
        with pytest.raises(SonetHipError, match="CUDA"):
            fn(pred, gt)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.chamfer_grad(pred, gt, ops.ChamferTerms(), torch.zeros(2))
    with pytest.raises(SonetHipError, match="before any update"):
        metrics.ChamferEvaluator().result()
    assert {"nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "sums", "M", "N"} == set(ops.ChamferTerms.__slots__)
    # a CPU tensor takes the present path of ChamferLoss even with the option set: it ends in the search wrapper's refusal
    from argparse import Namespace
    with pytest.raises(SonetHipError, match="CUDA"):
        LS.ChamferLoss(Namespace(gpu_id=0, chamfer_fused=True))(pred, gt)
