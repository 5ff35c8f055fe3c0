"""The fused Chamfer loss on the MI355X (sonet_chamfer_loss_f32, sonet_chamfer_grad_f32, ops.chamfer_loss, ChamferLoss with
opt.chamfer_fused, sonet_hip.metrics.ChamferEvaluator): the forward against the restatement of tests/chamfer_ref.py at the workgroup,
pair-tail and tile edges, NaN and overflow, the gradient against float64 at the kernel's own indices, the fixtures of the live
reference, routing, the evaluator and every refusal.

Indices and elements are bit-equal to the restatement; the sums are held to n * 2^-53 * sum against the exactly rounded sum (the bound
for n - 1 float64 additions of non-negative terms in any order); the gradient to chamfer_ref.GATE * sum|term| per entry (derivation
there; the CPU suite shows an f32-element kernel can meet it and that it sees a dropped direction)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import assert_close_rms, golden
import chamfer_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
AE_CASES = ("autoencoder_b2_n1024", "autoencoder_b2_n5000")


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_f32(a, b):
    """Bit-equal, a NaN matching any NaN (the payload of a generated NaN is the processor's business)."""
    return bool(((_bits32(a) == _bits32(b)) | (np.isnan(a) & np.isnan(b))).all())


def _host(t):
    return {k: getattr(t, k).cpu().numpy() for k in ("nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "sums") if getattr(t, k) is not None}


def _check_forward(pred, gt, what, ref=None):
    """One shape: indices, elements, sums, two runs -> the device record and the restatement's terms."""
    from sonet_hip import ops
    ref = R.terms(pred, gt) if ref is None else ref
    dp, dg = _cu(pred), _cu(gt)
    t = ops.chamfer_terms(dp, dg)
    h = _host(t)
    assert (t.M, t.N) == (pred.shape[2], gt.shape[2])
    assert h["nn_pg"].dtype == h["nn_gp"].dtype == np.int32 and h["elem_fwd"].dtype == np.float32 and h["sums"].dtype == np.float64
    assert np.array_equal(h["nn_pg"], ref["nn_pg"]), "%s: nn_pg differs from the oracle" % what
    assert np.array_equal(h["nn_gp"], ref["nn_gp"]), "%s: nn_gp differs from the oracle" % what
    for k in ("elem_fwd", "elem_bwd"):
        assert _same_f32(h[k], ref[k]), "%s: %s not bit-equal" % (what, k)
    n = np.array([pred.shape[2], gt.shape[2]], np.float64)
    fin = np.isfinite(ref["sums"])
    err = np.abs(h["sums"] - ref["sums"])
    assert np.array_equal(np.isnan(h["sums"]), np.isnan(ref["sums"])), what
    assert np.array_equal(h["sums"][~fin & ~np.isnan(ref["sums"])], ref["sums"][~fin & ~np.isnan(ref["sums"])]), what
    assert (err[fin] <= (n[None, :] * 2.0 ** -53 * ref["sums"])[fin]).all(), "%s: sums off by %.3g x bound" % (
        what, float((err[fin] / np.maximum((n[None, :] * 2.0 ** -53 * ref["sums"])[fin], 1e-300)).max()))
    h2 = _host(ops.chamfer_terms(dp, dg))
    for k in h:
        assert h[k].tobytes() == h2[k].tobytes(), "%s: %s changes between two runs" % (what, k)
    return t, ref


def _raw_loss(dp, dg, mask):
    """sonet_chamfer_loss_f32 through ctypes with the outputs of ``mask`` (nn_pg, nn_gp, elem_fwd, elem_bwd) present, the others NULL."""
    from sonet_hip import _lib
    B, _, M = dp.shape
    N = dg.shape[2]
    lib = _lib.load()
    out = [torch.full((B, M), -7, dtype=torch.int32, device=DEV), torch.full((B, N), -7, dtype=torch.int32, device=DEV),
           torch.full((B, M), -7.0, device=DEV), torch.full((B, N), -7.0, device=DEV)]
    out = [o if m else None for o, m in zip(out, mask)]
    sums = torch.full((B, 2), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.empty((lib.sonet_chamfer_loss_ws_size(B, M, N) // 8,), dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.sonet_chamfer_loss_f32(_lib.ptr(dp), _lib.ptr(dg), *[_lib.ptr(o) for o in out], _lib.ptr(sums), _lib.ptr(ws),
                                              B, M, N, _lib.stream_ptr()), "sonet_chamfer_loss_f32")
    return out + [sums]


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("M", R.FWD_M)
def test_forward_against_the_restatement(M):
    """(M, N) over the workgroup (256), pair-tail and 1024-point tile edges, B of 1 and 3, lattice and continuous data; M = 256 and
    1024-free N = 256 are the sizes where the first direction's workgroups end exactly on a workgroup of points."""
    from sonet_hip import ops
    for N in R.FWD_N:
        for B in (1, 3):
            for kind in ("lattice", "continuous"):
                pred, gt = R.make(kind, B, M, N)
                _check_forward(pred, gt, "%s B%d M%d N%d" % (kind, B, M, N))
        # every combination of absent outputs leaves the present ones and the sums as they are (B = 3, continuous: the last made)
        dp, dg = _cu(pred), _cu(gt)
        full = _raw_loss(dp, dg, (1, 1, 1, 1))
        for bits in range(15):
            mask = tuple((bits >> k) & 1 for k in range(4))
            got = _raw_loss(dp, dg, mask)
            for k in range(5):
                if got[k] is not None:
                    assert torch.equal(got[k].view(torch.int32 if k < 4 else torch.int64), full[k].view(torch.int32 if k < 4 else torch.int64)), (
                        "M%d N%d outputs %s: output %d differs" % (M, N, mask, k))
        for want_nn in (False, True):
            for want_elems in (False, True):
                t = ops.chamfer_terms(dp, dg, want_nn=want_nn, want_elems=want_elems)
                assert (t.nn_pg is not None) == (t.nn_gp is not None) == want_nn
                assert (t.elem_fwd is not None) == (t.elem_bwd is not None) == want_elems
                assert torch.equal(t.sums.view(torch.int64), full[4].view(torch.int64))


def test_forward_at_the_autoencoder_size():
    pred, gt = R.make("continuous", 2, 1280, 5000)
    _check_forward(pred, gt, "B2 1280 x 5000")


def test_nan_coordinate_and_overflowing_coordinates():
    from sonet_hip import ops
    pred, gt = R.make("continuous", 3, 300, 1100)
    clean = R.terms(pred, gt)
    bad = pred.copy()
    bad[1, 1, 257] = np.nan
    t, ref = _check_forward(bad, gt, "NaN coordinate")                       # (bit-equal to the restatement, NaN patterns included)
    h = _host(t)
    assert np.isnan(h["elem_fwd"][1, 257]) and np.isnan(h["sums"][1, 0]) and h["nn_pg"][1, 257] == 0
    assert np.isnan(h["elem_fwd"]).sum() == 1 and not np.isnan(h["elem_bwd"]).any() and not np.isnan(h["sums"][1, 1])
    assert _same_f32(h["elem_bwd"][1], ref["elem_bwd"][1])
    for b in (0, 2):                                                         # the other clouds are unchanged
        for k in ("nn_pg", "nn_gp", "elem_fwd", "elem_bwd"):
            assert np.array_equal(h[k][b], clean[k][b]), (b, k)
        assert np.array_equal(_bits64(h["sums"][b]), _bits64(_host(ops.chamfer_terms(_cu(pred), _cu(gt)))["sums"][b]))
    # a NaN in a gt point: its own element and every predicted point's distance to it
    badg = gt.copy()
    badg[0, 2, 1024] = np.nan
    _check_forward(pred, badg, "NaN gt coordinate")
    # +-3e19: squared distances overflow to +inf, a point that far from everything keeps index 0 and an infinite element
    far_p, far_g = pred.copy(), gt.copy()
    far_p[0, 0, [0, 255, 256, 299]] = np.float32(3e19)
    far_p[2, 1, [1, 128]] = np.float32(-3e19)
    far_g[0, 0, [3, 1023, 1024]] = np.float32(3e19)                          # (dx = 0 against the far predicted points: finite)
    far_g[1, 2, [5, 1099]] = np.float32(-3e19)
    t, ref = _check_forward(far_p, far_g, "overflow")
    assert np.isinf(ref["elem_fwd"]).any() and np.isinf(ref["elem_bwd"]).any() and np.isinf(ref["sums"]).any()


# ------------------------------------------------------------------------------------------------------------ gradient
def _check_grad(pred, gt, what, scales=((1.0, 1.0),), terms=None):
    """The kernel's gradient at its own indices against the float64 restatement (== float64 autograd of the reference's expression:
    tests/test_chamfer_loss_cpu.py).  -> worst |error| / (GATE sum|term|)."""
    from sonet_hip import ops
    dp, dg = _cu(pred), _cu(gt)
    t = ops.chamfer_terms(dp, dg) if terms is None else terms
    nn_pg, nn_gp = t.nn_pg.cpu().numpy(), t.nn_gp.cpu().numpy()
    worst = 0.0
    for gf, gb in scales:
        gs = torch.tensor([gf, gb], dtype=torch.float32, device=DEV)
        gf32, gb32 = (float(v) for v in gs.cpu().numpy())
        dpred, bad = ops.chamfer_grad(dp, dg, t, gs)
        again, _ = ops.chamfer_grad(dp, dg, t, gs)
        assert int(bad) == 0 and dpred.dtype == torch.float32 and tuple(dpred.shape) == pred.shape
        assert torch.equal(dpred.view(torch.int32), again.view(torch.int32)), "%s: two runs differ" % what
        ref64, mag = R.grad(pred, gt, nn_pg, nn_gp, gf32, gb32)
        got = dpred.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), what
        err = np.abs(got - ref64)
        assert (err <= R.GATE * mag).all(), "%s gf=%g gb=%g: worst error %.3f x gate" % (
            what, gf, gb, float((err / np.maximum(R.GATE * mag, 1e-300)).max()))
        nz = mag > 0
        assert (got[~nz] == 0).all()
        if nz.any():
            worst = max(worst, float((err[nz] / (R.GATE * mag[nz])).max()))
    return worst


@pytest.mark.parametrize("M", R.FWD_M)
def test_gradient_against_float64(M):
    worst = 0.0
    for k, N in enumerate(n for n in R.FWD_N if n <= 1025):
        for B in (1, 3):
            for kind in ("lattice", "continuous"):
                pred, gt = R.make(kind, B, M, N)
                scales = ((1.0, 1.0), (0.7, -1.3)) if (k + B) % 2 else ((1.0, 1.0),)
                worst = max(worst, _check_grad(pred, gt, "%s B%d M%d N%d" % (kind, B, M, N), scales))
    print("M=%d: worst gradient error %.3f x gate" % (M, worst))


def test_gradient_lists_zero_terms_and_scales():
    from sonet_hip import ops
    # one predicted point owns all 1025 gt points (a list that crosses an LDS tile); every other predicted point owns none
    for M, owner in ((300, 150), (7, 6), (1, 0)):
        pred, gt = R.one_owner(2, M, 1025, 77 + M, owner=owner)
        t = ops.chamfer_terms(_cu(pred), _cu(gt))
        assert (t.nn_gp.cpu().numpy() == owner).all()
        _check_grad(pred, gt, "one owner M%d" % M, ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.25, 3.0)), terms=t)
    # a predicted point that no gt point chooses has its forward term alone
    pred, gt = R.make("continuous", 2, 257, 300)
    pred[:, :, 100] = np.array([5.0, 5.0, 5.0], np.float32)
    t = ops.chamfer_terms(_cu(pred), _cu(gt))
    assert not (t.nn_gp.cpu().numpy() == 100).any()
    _check_grad(pred, gt, "unchosen point", ((1.0, 1.0), (0.0, 1.0)), terms=t)
    gs = torch.tensor([0.0, 1.0], device=DEV)
    assert (ops.chamfer_grad(_cu(pred), _cu(gt), t, gs)[0][:, :, 100] == 0).all()
    # coincident points: elements at the 1e-4 floor, terms of exactly zero, no NaN from 0 / 1e-4
    g = golden("chamfer/coincident_half")
    _check_grad(g["pred"], g["gt"], "coincident fixture", ((1.0, 1.0), (0.7, -1.3), (0.0, 2.0), (1.5, 0.0)))
    gs = torch.tensor([1.0, 0.0], device=DEV)
    dp, dg = _cu(g["pred"]), _cu(g["gt"])
    d = ops.chamfer_grad(dp, dg, ops.chamfer_terms(dp, dg), gs)[0].cpu().numpy()
    assert (d[:, :, ::2] == 0).all() and (d[:, :, 1::2] != 0).any()
    # both scales zero: a gradient of zeros
    z = ops.chamfer_grad(dp, dg, ops.chamfer_terms(dp, dg), torch.zeros(2, device=DEV))[0]
    assert (z == 0).all()


def test_autograd_function_backward_twice_and_unused_outputs():
    from sonet_hip import ops
    pred, gt = R.make("continuous", 3, 257, 1025)
    dg = _cu(gt)
    p = _cu(pred).requires_grad_(True)
    fl, bl, fa, ba = ops.chamfer_loss(p, dg)
    assert fl.dtype == bl.dtype == fa.dtype == ba.dtype == torch.float32 and fl.dim() == bl.dim() == 0 and tuple(fa.shape) == (3,)
    assert fl.requires_grad and bl.requires_grad and not fa.requires_grad and not ba.requires_grad
    ref = R.terms(pred, gt)
    ls = R.losses(ref)
    # the scalars are the f32 rounding of the float64 quotient: within one rounding of the restatement's exactly summed value
    for got, want in ((fl, ls["forward_loss"]), (bl, ls["backward_loss"])):
        assert abs(float(got.detach()) - want) <= 2.0 ** -24 * want * 1.001
    np.testing.assert_allclose(fa.cpu().numpy(), ls["forward_loss_array"], rtol=2.0 ** -23)
    np.testing.assert_allclose(ba.cpu().numpy(), ls["backward_loss_array"], rtol=2.0 ** -23)
    with ops.kernel_timing() as rec:
        (0.7 * fl - 1.3 * bl).backward(retain_graph=True)
        torch.cuda.synchronize()
    assert rec.summary()["chamfer_grad"]["count"] == 1 and set(rec.summary()) == {"chamfer_grad"}     # one call, both scales stacked
    g1 = p.grad.clone()
    p.grad = None
    (0.7 * fl - 1.3 * bl).backward(retain_graph=True)
    assert torch.equal(g1.view(torch.int32), p.grad.view(torch.int32)), "second backward through the retained graph differs"
    ref64, mag = R.grad(pred, gt, ref["nn_pg"], ref["nn_gp"], float(np.float32(0.7)), float(np.float32(-1.3)))
    assert (np.abs(g1.cpu().numpy().astype(np.float64) - ref64) <= R.GATE * mag).all()
    # only one of the two losses used: the other scale is zero
    p.grad = None
    fl.backward(retain_graph=True)
    ref64, mag = R.grad(pred, gt, ref["nn_pg"], ref["nn_gp"], 1.0, 0.0)
    assert (np.abs(p.grad.cpu().numpy().astype(np.float64) - ref64) <= R.GATE * mag).all()


def test_forged_indices_are_counted_and_never_addresses():
    from sonet_hip import ops
    pred, gt = R.make("continuous", 2, 300, 1100)
    B, M, N = 2, 300, 1100
    dp, dg = _cu(pred), _cu(gt)
    t = ops.chamfer_terms(dp, dg)
    gs = torch.tensor([0.7, -1.3], device=DEV)
    clean, bad0 = ops.chamfer_grad(dp, dg, t, gs)
    assert int(bad0) == 0
    nn_pg, nn_gp = t.nn_pg.cpu().numpy().copy(), t.nn_gp.cpu().numpy().copy()
    forged_m = {(0, 0): -1, (0, 255): N, (1, 256): 2 ** 31 - 1, (1, 299): M + N}          # nn_pg entries outside [0, N)
    forged_n = {(0, 5): -1, (0, 1023): M, (0, 1024): N, (1, 1099): 2 ** 31 - 1}             # nn_gp entries outside [0, M)
    owners = set()
    for (b, n), v in forged_n.items():
        owners.add((b, int(nn_gp[b, n])))
        nn_gp[b, n] = v
    for (b, m), v in forged_m.items():
        nn_pg[b, m] = v
    f = ops.ChamferTerms()
    f.nn_pg, f.nn_gp, f.elem_fwd, f.elem_bwd, f.M, f.N = _cu(nn_pg), _cu(nn_gp), t.elem_fwd, t.elem_bwd, M, N
    got, bad = ops.chamfer_grad(dp, dg, f, gs)
    assert int(bad) == len(forged_m) + len(forged_n)
    touched = np.zeros((B, M), bool)
    for b, m in list(forged_m) + list(owners):
        touched[b, m] = True
    got, clean = got.cpu().numpy(), clean.cpu().numpy()
    assert np.array_equal(_bits32(got.transpose(0, 2, 1)[~touched]), _bits32(clean.transpose(0, 2, 1)[~touched]))
    assert np.isfinite(got).all()
    # a forged entry contributes nothing: a predicted point with a forged nn_pg (and no forged gt entry) keeps its backward terms alone
    only_bwd, mag = R.grad(pred, gt, t.nn_pg.cpu().numpy(), t.nn_gp.cpu().numpy(), 0.0, float(np.float32(-1.3)))
    for b, m in forged_m:
        if (b, m) not in owners:
            assert (np.abs(got[b, :, m] - only_bwd[b, :, m]) <= R.GATE * mag[b, :, m]).all(), (b, m)


# ------------------------------------------------------------------------------------------------------------ the reference
def _fixture(case):
    g = golden(case if case.startswith("autoencoder") else "chamfer/" + case)
    if case.startswith("autoencoder"):
        return g["predicted_pc"], g["pc"], g
    return g["pred"], g["gt"], g


@pytest.mark.parametrize("case", R.GOLDEN_CASES + AE_CASES)
def test_fused_and_default_loss_against_the_reference(case):
    from models import losses as LS
    pred, gt, g = _fixture(case)
    dg = _cu(gt)
    out = {}
    for name, opt in (("fused", Namespace(gpu_id=0, device=DEV, chamfer_fused=True)), ("default", Namespace(gpu_id=0, device=DEV)),
                      ("off", Namespace(gpu_id=0, device=DEV, chamfer_fused=False))):
        crit = LS.ChamferLoss(opt)
        p = _cu(pred).requires_grad_(True)
        loss = crit(p, dg)
        loss.backward()
        out[name] = dict(loss=loss.detach(), grad=p.grad, **{k: getattr(crit, k).detach() for k in (
            "forward_loss", "backward_loss", "forward_loss_array", "backward_loss_array", "loss_array")})
        assert loss.requires_grad and loss.dim() == 0
    for k, v in out["default"].items():                                        # same attributes, dtypes and shapes on both paths
        assert out["fused"][k].dtype == v.dtype == torch.float32 and out["fused"][k].shape == v.shape, k
        # the default path is the same with the option absent and with it false
        assert torch.equal(out["off"][k].view(torch.int32), v.view(torch.int32)) or k == "grad", k
    # (the default path's gradient ends in aten's atomic scatter-add: two runs of it differ by the reordering of an f32 sum, up to
    #  (k - 1) 2^-24 of sum|term| for a point that k gt points chose -- held to the project's f32 bar, the gradient tolerance below)
    assert_close_rms(out["off"]["grad"].cpu().numpy(), out["default"]["grad"].cpu().numpy(), 1e-5, "default path gradient, two runs")
    for name in ("fused", "default"):
        o = out[name]
        for k in ("forward_loss", "backward_loss"):
            assert abs(float(o[k]) - float(g[k])) <= 2e-6 * float(g[k]), (name, k, float(o[k]), float(g[k]))
        np.testing.assert_allclose(o["loss_array"].cpu().numpy(), g["loss_array"], rtol=5e-6, err_msg=name)
        assert_close_rms(o["grad"].cpu().numpy(), g["grad_predicted"], 1e-5, name + ": d loss / d predicted")
        assert abs(float(o["loss"]) - (float(g["forward_loss"]) + float(g["backward_loss"]))) <= 2e-6 * float(o["loss"])
    if not case.startswith("autoencoder"):
        from sonet_hip import ops
        t = ops.chamfer_terms(_cu(pred), dg)
        assert np.array_equal(t.nn_pg.cpu().numpy(), g["nn_pg"]) and np.array_equal(t.nn_gp.cpu().numpy(), g["nn_gp"])
        assert R.ulps(t.elem_fwd.cpu().numpy(), g["elem_fwd"]).max() <= 3 and R.ulps(t.elem_bwd.cpu().numpy(), g["elem_bwd"]).max() <= 3
        np.testing.assert_allclose(out["fused"]["forward_loss_array"].cpu().numpy(), g["forward_loss_array"], rtol=5e-6)
        np.testing.assert_allclose(out["fused"]["backward_loss_array"].cpu().numpy(), g["backward_loss_array"], rtol=5e-6)


def test_chamfer_loss_routing():
    from models import losses as LS
    from sonet_hip import ops
    pred, gt = R.make("continuous", 2, 257, 600)
    dp, dg = _cu(pred), _cu(gt)

    def kernels(opt, p, g):
        crit = LS.ChamferLoss(opt)
        with ops.kernel_timing() as rec:
            loss = crit(p, g)
            if loss.requires_grad:
                loss.backward()
            torch.cuda.synchronize()
        return {k: v["count"] for k, v in rec.summary().items()}, crit

    fused = Namespace(gpu_id=0, device=DEV, chamfer_fused=True)
    k, _ = kernels(fused, dp.clone().requires_grad_(True), dg)
    assert k == {"chamfer_loss": 1, "chamfer_grad": 1}
    k, _ = kernels(fused, dp, dg)
    assert k == {"chamfer_loss": 1}
    k, _ = kernels(fused, dp.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True), dg)      # a non-contiguous view
    assert k == {"chamfer_loss": 1, "chamfer_grad": 1}
    for opt in (Namespace(gpu_id=0, device=DEV), Namespace(gpu_id=0, device=DEV, chamfer_fused=False)):
        k, _ = kernels(opt, dp.clone().requires_grad_(True), dg)
        assert k == {"chamfer_nn": 2}
    # with the option set, these take the present path
    k, crit = kernels(fused, dp.bfloat16(), dg.bfloat16())
    assert k == {"chamfer_nn": 2}
    k, _ = kernels(fused, dp.clone().requires_grad_(True), dg.clone().requires_grad_(True))
    assert k == {"chamfer_nn": 2}
    from sonet_hip._lib import SonetHipError
    with ops.kernel_timing() as rec:
        with pytest.raises(SonetHipError, match="CUDA"):                       # the present path's own refusal of a CPU tensor
            LS.ChamferLoss(fused)(dp.cpu(), dg.cpu())
    assert not rec.records


# ------------------------------------------------------------------------------------------------------------ evaluator
def test_evaluator_over_the_fixtures():
    from sonet_hip._lib import SonetHipError
    from sonet_hip.metrics import ChamferEvaluator
    for case in R.GOLDEN_CASES + AE_CASES:
        pred, gt, g = _fixture(case)
        B = pred.shape[0]
        ev = ChamferEvaluator()
        la = ev.update(_cu(pred), _cu(gt))
        one = ev.result()
        assert sorted(one) == ["backward", "count", "forward", "test_loss"] and one["count"] == B
        assert la.dtype == torch.float32 and tuple(la.shape) == (B,)
        np.testing.assert_allclose(la.cpu().numpy(), g["loss_array"], rtol=5e-6)
        # uneven batches of the same clouds give what one call gives
        ev2 = ChamferEvaluator()
        for lo, hi in ((0, 1), (1, B)):
            ev2.update(_cu(pred[lo:hi]), _cu(gt[lo:hi]))
        two = ev2.result()
        for k in ("test_loss", "forward", "backward"):
            assert abs(one[k] - two[k]) <= 1e-14 * abs(one[k]), (case, k)
        # the reference's accumulation of its own batch values: sum of loss x B / count (autoencoder/train.py:94-96)
        want = (float(g["forward_loss"]) + float(g["backward_loss"])) * B / B
        assert abs(one["test_loss"] - want) <= 2e-6 * want, (case, one["test_loss"], want)
        assert abs(one["forward"] - float(g["forward_loss"])) <= 2e-6 * float(g["forward_loss"])
        assert abs(one["backward"] - float(g["backward_loss"])) <= 2e-6 * float(g["backward_loss"])
    # several fixtures of different sizes in one epoch: the per-cloud mean
    ev, tot, cnt = ChamferEvaluator(), 0.0, 0
    for case in R.GOLDEN_CASES:
        pred, gt, g = _fixture(case)
        ev.update(_cu(pred), _cu(gt))
        tot += (float(g["forward_loss"]) + float(g["backward_loss"])) * pred.shape[0]
        cnt += pred.shape[0]
    got = ev.result()
    assert got["count"] == cnt == 7 and abs(got["test_loss"] - tot / cnt) <= 2e-6 * tot / cnt
    ev.reset()
    with pytest.raises(SonetHipError, match="without any cloud"):
        ev.result()
    with pytest.raises(SonetHipError, match="before any update"):
        ChamferEvaluator().result()
    pred, gt, _ = _fixture(R.GOLDEN_CASES[0])
    bad = pred.copy()
    bad[2, 0, 17] = np.nan
    ev.update(_cu(pred), _cu(gt))
    ev.update(_cu(bad), _cu(gt))
    with pytest.raises(SonetHipError, match="1 cloud.* of 6 is NaN"):
        ev.result()


def test_evaluate_autoencoder_end_to_end():
    """41 clouds of 300 points, 256 sampled, 16 nodes, batches of 16 (the last one of 9): evaluate_autoencoder against a hand-run loop
    with the default ChamferLoss."""
    from models import losses as LS, networks as NW
    from sonet_hip import metrics, ops, synth
    from sonet_hip.batch import BatchAssembler, DeviceClouds
    S, n, N, M, BS = 41, 300, 256, 16, 16
    g = np.random.RandomState(41)
    pts = [g.uniform(-1, 1, size=(n, 3)).astype(np.float32) for _ in range(S)]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = np.stack([p[g.choice(n, M, replace=False)] for p in pts]).astype(np.float32)
    opt = Namespace(gpu_id=0, device=DEV, batch_size=BS, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                    normalization="batch", dropout=0.7, node_num=M, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                    bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40, output_fc_pc_num=256, output_conv_pc_num=1024)
    enc, dec = NW.Encoder(opt), NW.Decoder(opt)
    synth.fill_state_dict_(enc.state_dict(), 15)
    synth.fill_state_dict_(dec.state_dict(), 16)
    enc.to(DEV).train()
    dec.to(DEV).train()                                            # evaluate_autoencoder itself must switch to eval mode
    clouds = DeviceClouds(pts, nrm, np.zeros(S, np.int64), nodes=nodes, device=DEV)
    A = BatchAssembler(clouds, opt, "test", "modelnet", seed=4)
    with ops.kernel_timing() as rec:
        got = metrics.evaluate_autoencoder(enc, dec, A, BS)
        torch.cuda.synchronize()
    assert not enc.training and not dec.training
    assert rec.summary()["chamfer_loss"]["count"] == 3 and "chamfer_nn" not in rec.summary()
    crit = LS.ChamferLoss(opt)
    per_cloud, fwd, bwd, sizes = [], [], [], []
    with torch.no_grad():
        for pc, sn, label, node, knn in A.epoch(0, BS, shuffle=False):
            pred = dec(enc(pc, sn, node, knn, False, None))
            assert tuple(pred.shape) == (pc.shape[0], 3, 1280)
            crit(pred, pc)
            per_cloud.append(crit.loss_array.double().cpu().numpy())
            fwd.append(crit.forward_loss_array.double().cpu().numpy())
            bwd.append(crit.backward_loss_array.double().cpu().numpy())
            sizes.append(pc.shape[0])
    want = float(np.concatenate(per_cloud).mean())
    print("evaluate_autoencoder", got, "hand-run loop", want)
    assert sizes == [16, 16, 9] and got["count"] == S
    assert abs(got["test_loss"] - want) <= 2e-6 * want
    assert abs(got["forward"] - float(np.concatenate(fwd).mean())) <= 2e-6 * got["forward"]
    assert abs(got["backward"] - float(np.concatenate(bwd).mean())) <= 2e-6 * got["backward"]
    from sonet_hip._lib import SonetHipError
    with pytest.raises(SonetHipError, match="test-mode"):
        metrics.evaluate_autoencoder(enc, dec, BatchAssembler(clouds, opt, "train", "modelnet", seed=4), BS)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_wrappers_refuse_bad_arguments():
    from sonet_hip import _lib, ops
    from sonet_hip._lib import SonetHipError
    from sonet_hip.metrics import ChamferEvaluator
    pred, gt = torch.zeros(2, 3, 8, device=DEV), torch.zeros(2, 3, 16, device=DEV)
    t = ops.chamfer_terms(pred, gt)
    gs = torch.ones(2, device=DEV)
    calls = (lambda p, g: ops.chamfer_terms(p, g), lambda p, g: ops.chamfer_loss(p, g), lambda p, g: ops.chamfer_grad(p, g, t, gs),
             lambda p, g: ChamferEvaluator().update(p, g))
    for call in calls:
        with pytest.raises(SonetHipError, match="float32"):
            call(pred.double(), gt)
        with pytest.raises(SonetHipError, match="float32"):
            call(pred, gt.bfloat16())
        with pytest.raises(SonetHipError, match="contiguous"):
            call(torch.zeros(2, 8, 3, device=DEV).transpose(1, 2), gt)
        with pytest.raises(SonetHipError, match="contiguous"):
            call(pred, torch.zeros(2, 16, 3, device=DEV).transpose(1, 2))
        with pytest.raises(SonetHipError, match="CUDA"):
            call(pred, gt.cpu())
        with pytest.raises(SonetHipError, match="3 channels"):
            call(torch.zeros(2, 4, 8, device=DEV), gt)
        with pytest.raises(SonetHipError, match="3 channels"):
            call(pred, torch.zeros(2, 2, 16, device=DEV))
        with pytest.raises(SonetHipError, match="same number of clouds"):
            call(pred, gt[:1].contiguous())
        with pytest.raises(SonetHipError, match="gt must not require a gradient"):
            call(pred, gt.clone().requires_grad_(True))
        with pytest.raises(SonetHipError, match="3-D"):
            call(pred[0], gt)
    if torch.cuda.device_count() > 1:
        with pytest.raises(SonetHipError, match="different devices"):
            ops.chamfer_terms(pred, gt.to("cuda:1"))
    # the gradient wrapper's own operands
    with pytest.raises(SonetHipError, match="gscale"):
        ops.chamfer_grad(pred, gt, t, torch.ones(3, device=DEV))
    with pytest.raises(SonetHipError, match="gscale"):
        ops.chamfer_grad(pred, gt, t, torch.ones(2, device=DEV, dtype=torch.float64))
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.chamfer_grad(pred, gt, t, torch.ones(2))
    with pytest.raises(SonetHipError, match="indices and the elements"):
        ops.chamfer_grad(pred, gt, ops.chamfer_terms(pred, gt, want_nn=False), gs)
    other = ops.chamfer_terms(pred, torch.zeros(2, 3, 17, device=DEV))
    with pytest.raises(SonetHipError, match="nn_gp must have shape"):
        ops.chamfer_grad(pred, gt, other, gs)
    # B = 65536 is refused before a launch: by the wrapper, and by the C entries themselves (nothing is read: every pointer is one word)
    big_p, big_g = torch.zeros(65536, 3, 1, device=DEV), torch.zeros(65536, 3, 1, device=DEV)
    with ops.kernel_timing() as rec:
        with pytest.raises(SonetHipError, match="65535"):
            ops.chamfer_terms(big_p, big_g)
        with pytest.raises(SonetHipError, match="65535"):
            ops.chamfer_loss(big_p, big_g)
    assert not rec.records
    lib = _lib.load()
    word = torch.zeros(2, dtype=torch.float64, device=DEV)
    p = _lib.ptr(word)
    assert lib.sonet_chamfer_loss_f32(p, p, None, None, None, None, p, p, 65536, 1, 1, None) == 2 and "B=65536" in _lib.last_error()
    assert lib.sonet_chamfer_grad_f32(p, p, p, p, p, p, p, p, p, 65536, 1, 1, None) == 2 and "B=65536" in _lib.last_error()
    torch.cuda.synchronize()
    assert (word == 0).all()
