"""The Chamfer loss pyramid without a GPU: the restatement of the inverse-list gradient (tests/chamfer_pyramid_ref.py) against
tests/chamfer_ref.py bit for bit, two mistakes it must see, ``AutoencoderLoss`` on the autoencoder fixtures of the reference, the C
entries' argument checks, the exported extents and the routing of ``AutoencoderLoss`` when the option is absent."""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import golden
import chamfer_ref as R
import chamfer_pyramid_ref as P

AE_CASES = ("autoencoder_b2_n1024", "autoencoder_b2_n5000")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _list_cases():
    """(name, pred, gt): continuous and tie-heavy clouds, one predicted point owning every gt point (first, middle, last), a level
    of one predicted point, coincident points."""
    out = [("continuous", ) + R.make("continuous", 2, 257, 300), ("lattice", ) + R.make("lattice", 3, 255, 256),
           ("coincident", ) + R.make("coincident", 2, 64, 300), ("M = 1", ) + R.make("continuous", 3, 1, 130)]
    for owner in (0, 3, 6):
        out.append(("one_owner %d" % owner, ) + R.one_owner(2, 7, 300, 77 + owner, owner=owner))
    return out


def test_pyramid_restatement_is_chamfer_ref_per_level():
    gt = R.make("continuous", 2, 4, 130)[1]
    preds = [R.make("continuous", 2, M, 130, seed=k)[0] for k, M in enumerate((67, 1, 67))]
    ts = P.terms(preds, gt)
    gscale = np.array([[1.0, 1.0], [0.0, 2.0], [0.7, -1.3]])
    for l, (p, t) in enumerate(zip(preds, ts)):
        one = R.terms(p, gt)
        for k in one:
            assert np.array_equal(t[k], one[k]), (l, k)
        for k, v in R.losses(one).items():
            assert np.array_equal(P.losses(ts)[l][k], v), (l, k)
        want = R.grad(p, gt, one["nn_pg"], one["nn_gp"], gscale[l, 0], gscale[l, 1])[0]
        assert np.array_equal(_bits(P.grad(preds, gt, ts, gscale)[l][0]), _bits(want))


def test_inverse_lists_add_the_terms_in_the_order_of_chamfer_ref():
    for name, pred, gt in _list_cases():
        nn_pg, nn_gp = R.indices(pred, gt)
        M, N = pred.shape[2], gt.shape[2]
        if name.startswith("one_owner"):
            assert (nn_gp == int(name.split()[1])).all()                         # one list of length N, every other list empty
        for b in range(pred.shape[0]):
            order, start = P.inverse_lists(nn_gp[b], M)
            assert sorted(order.tolist()) == list(range(N)) and start[0] == 0 and start[M] == N and (np.diff(start) >= 0).all()
            for m in range(M):
                assert order[start[m]:start[m + 1]].tolist() == np.flatnonzero(nn_gp[b] == m).tolist(), (name, b, m)
        for gf, gb in ((1.0, 1.0), (0.7, -1.3), (0.0, 2.0)):
            for elems in ("f64", "f32"):
                want, wmag = R.grad(pred, gt, nn_pg, nn_gp, gf, gb, elems=elems)
                got, gmag = P.grad_lists(pred, gt, nn_pg, nn_gp, gf, gb, elems=elems)
                assert np.array_equal(_bits(got), _bits(want)), (name, gf, gb, elems)
                assert np.array_equal(_bits(gmag), _bits(wmag)), (name, gf, gb, elems)


def test_an_unstable_order_and_a_dropped_last_segment_are_seen():
    seen_order = seen_cut = 0
    for name, pred, gt in _list_cases():
        nn_pg, nn_gp = R.indices(pred, gt)
        want, mag = R.grad(pred, gt, nn_pg, nn_gp, 0.7, -1.3)
        # every list back to front: the same terms, another float64 sum wherever a list has a few entries
        rev = P.grad_lists(pred, gt, nn_pg, nn_gp, 0.7, -1.3, stable=False)[0]
        assert (np.abs(rev - want) <= 1e-12 * mag).all(), name                  # (the same value to float64 rounding ...)
        seen_order += int(not np.array_equal(_bits(rev), _bits(want)))          # (... and not the same bits)
        if name.startswith("one_owner"):
            assert not np.array_equal(_bits(rev), _bits(want)), name
        # the list of the largest owner never walked: off by whole terms, far outside the gradient gate
        # (wherever that list holds a term that is not exactly zero: on a lattice a gt point can coincide with its owner)
        bmag = R.grad(pred, gt, nn_pg, nn_gp, 0.0, 1.0)[1]
        if any((bmag[b, :, nn_gp[b].max()] > 0).any() for b in range(pred.shape[0])):
            seen_cut += 1
            cut = P.grad_lists(pred, gt, nn_pg, nn_gp, 0.7, -1.3, drop_last_segment=True)[0]
            assert (np.abs(cut - want) > R.GATE * mag).any(), name
    assert seen_order >= 5 and seen_cut >= 5


@pytest.mark.parametrize("case", AE_CASES)
def test_autoencoder_loss_on_the_reference_fixtures(case, monkeypatch):
    """``AutoencoderLoss`` on CPU tensors takes the ``ChamferLoss`` path; the search wrapper there is GPU-only, so the exact search of
    the CPU oracle stands in for it and the rest -- gathers, robust_norm, means, the sum of the terms -- is the module's own code."""
    from models import losses as LS
    from sonet_hip import ops
    monkeypatch.setattr(ops, "chamfer_nn", P.cpu_search)
    g = golden(case)
    dec = Namespace(conv_pc4=torch.from_numpy(g["conv_pc4"]), conv_pc5=None)
    for opt in (Namespace(gpu_id=-1, output_conv_pc_num=1024), Namespace(gpu_id=-1, output_conv_pc_num=1024, chamfer_pyramid=True)):
        crit = LS.AutoencoderLoss(opt)
        loss = crit(torch.from_numpy(g["predicted_pc"]), dec, torch.from_numpy(g["pc"]))
        assert loss is crit.loss and crit.loss_chamfer_conv5 is None
        for k in ("loss", "loss_chamfer", "loss_chamfer_conv4"):
            assert abs(float(getattr(crit, k)) - float(g[k])) <= 2e-6 * float(g[k]), (k, float(getattr(crit, k)), float(g[k]))
        assert abs(float(crit.forward_loss) - float(g["forward_loss"])) <= 2e-6 * float(g["forward_loss"])
        np.testing.assert_allclose(crit.loss_array.numpy(), g["loss_array"], rtol=5e-6)


class _Counting(torch.nn.Module):
    """Stands in for ``ChamferLoss``: counts its calls and returns a value that names the cloud."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, pred, gt):
        self.calls.append(pred.shape[2])
        self.forward_loss = self.backward_loss = torch.tensor(float(pred.shape[2]))
        self.forward_loss_array = self.backward_loss_array = self.loss_array = torch.zeros(pred.shape[0])
        return torch.tensor(float(pred.shape[2]))


def test_option_parsing_and_routing_without_the_option(monkeypatch):
    from models import losses as LS
    from sonet_hip import ops
    on = LS.AutoencoderLoss.pyramid_enabled
    assert not on(Namespace()) and not on(Namespace(chamfer_pyramid=False)) and not on(Namespace(chamfer_pyramid=None))
    assert not on(Namespace(chamfer_pyramid=0)) and on(Namespace(chamfer_pyramid=True)) and on(Namespace(chamfer_pyramid=1))

    def no_pyramid(*a, **k):
        raise AssertionError("the pyramid operator was called")

    monkeypatch.setattr(ops, "chamfer_pyramid_loss", no_pyramid)
    gt = torch.zeros(2, 3, 50)
    dec = Namespace(conv_pc4=torch.zeros(2, 3, 256), conv_pc5=torch.zeros(2, 3, 1024))
    for n, final, calls, loss in ((0, 256, [256], 256.0), (1024, 1280, [256, 1280], 1536.0), (4096, 4352, [1024, 256, 4352], 5632.0)):
        for extra in (dict(), dict(chamfer_pyramid=False), dict(chamfer_pyramid=True)):      # (on, but CPU tensors: the same path)
            crit = LS.AutoencoderLoss(Namespace(gpu_id=-1, output_conv_pc_num=n, **extra))
            assert isinstance(crit.chamfer_criteria, LS.ChamferLoss)
            crit.chamfer_criteria = count = _Counting()
            out = crit(torch.zeros(2, 3, final), dec, gt)
            assert count.calls == calls, (n, extra, count.calls)                 # once per term, in the reference's order
            assert float(out) == float(crit.loss) == loss
            assert float(crit.loss_chamfer) == final
            assert (crit.loss_chamfer_conv4 is None) == (n == 0) and (crit.loss_chamfer_conv5 is None) == (n != 4096)
    # what else keeps the present path with the option on: another dtype, a gt that asks for a gradient (checked on attributes alone)
    crit = LS.AutoencoderLoss(Namespace(gpu_id=-1, output_conv_pc_num=0, chamfer_pyramid=True))
    assert not crit._takes_pyramid([torch.zeros(2, 3, 8)], gt)
    assert not crit._takes_pyramid([torch.zeros(2, 3, 8, dtype=torch.float64)], gt.double())
    assert not crit._takes_pyramid([torch.zeros(2, 3, 8)], gt.clone().requires_grad_(True))


def test_exported_extents_match_the_wrapper():
    from sonet_hip import _lib, ops
    lib = _lib.load()
    assert lib.sonet_chamfer_pyramid_max_n() == ops.CHAMFER_PYRAMID_MAX_N
    assert lib.sonet_chamfer_pyramid_max_m() == ops.CHAMFER_PYRAMID_MAX_M
    assert ops.chamfer_pyramid_supported([ops.CHAMFER_PYRAMID_MAX_M, 1], ops.CHAMFER_PYRAMID_MAX_N)
    assert not ops.chamfer_pyramid_supported([ops.CHAMFER_PYRAMID_MAX_M + 1], 8)
    assert not ops.chamfer_pyramid_supported([8], ops.CHAMFER_PYRAMID_MAX_N + 1)
    assert not ops.chamfer_pyramid_supported([], 8) and not ops.chamfer_pyramid_supported([1, 2, 3, 4], 8)
    assert not ops.chamfer_pyramid_supported([0], 8) and not ops.chamfer_pyramid_supported([8], 0)
    # the workload's sizes are inside: the final cloud of either configuration against 5000 gt points
    assert ops.chamfer_pyramid_supported([4352, 1024, 256], 5000)


def test_c_entries_reject_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    max_n, max_m = lib.sonet_chamfer_pyramid_max_n(), lib.sonet_chamfer_pyramid_max_m()

    def arr(L, null_at=None):
        return (ctypes.c_void_p * 3)(*[None if l == null_at else p.value for l in range(3)])

    def loss(B=1, L=2, M=(2, 3, 4), N=4, null=(), null_at=None):
        names = ("pred", "gt", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "sums", "ws")
        a = [None if k in null else (arr(L, null_at if k == "pred" else None) if k in names[:1] + names[2:6] else p) for k in names]
        Ms = None if "M" in null else (ctypes.c_int * 3)(*M)
        return lib.sonet_chamfer_pyramid_loss_f32(*a, B, L, Ms, N, None)

    def grad(B=1, L=2, M=(2, 3, 4), N=4, null=(), null_at=None):
        names = ("pred", "gt", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "gscale", "dpred", "bad")
        arrays = ("pred", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "dpred")
        a = [None if k in null else (arr(L, null_at[1] if null_at and k == null_at[0] else None) if k in arrays else p) for k in names]
        Ms = None if "M" in null else (ctypes.c_int * 3)(*M)
        return lib.sonet_chamfer_pyramid_grad_f32(*a, B, L, Ms, N, None)

    for fn in (loss, grad):
        for L in (0, 4, -1):
            assert fn(L=L) == 1 and "outside 1..3" in _lib.last_error(), (fn.__name__, L)
        for kw in (dict(B=0), dict(N=0), dict(B=-1), dict(N=-5), dict(M=(2, 0, 4)), dict(M=(-3, 3, 4)), dict(L=3, M=(2, 3, 0))):
            assert fn(**kw) == 1 and "non-positive" in _lib.last_error(), (fn.__name__, kw)
        assert fn(null=("M",)) == 1 and "NULL" in _lib.last_error()
        assert fn(B=65536) == 2 and "B=65536" in _lib.last_error(), fn.__name__
        assert fn(N=max_n + 1) == 2 and "N=%d" % (max_n + 1) in _lib.last_error(), fn.__name__
        assert fn(M=(2, max_m + 1, 4)) == 2 and "M[1]=%d" % (max_m + 1) in _lib.last_error(), fn.__name__
    for name in ("pred", "gt", "sums", "ws"):
        assert loss(null=(name,)) == 1 and "NULL" in _lib.last_error(), name
    assert loss(null_at=1) == 1 and "pred[1]" in _lib.last_error()
    for name in ("pred", "gt", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "gscale", "dpred", "bad"):
        assert grad(null=(name,)) == 1 and "NULL" in _lib.last_error(), name
    for name in ("pred", "nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "dpred"):
        assert grad(null_at=(name, 1)) == 1 and "level 1" in _lib.last_error(), name
    # the optional outputs of the loss entry are optional: with bad sizes the size check answers, not the NULL check
    assert loss(null=("nn_pg", "nn_gp", "elem_fwd", "elem_bwd"), B=0) == 1 and "non-positive" in _lib.last_error()
    ws = lib.sonet_chamfer_pyramid_ws_size
    assert ws(0, 1, 4, 4, 4, 4) == 0 and ws(2, 2, 8, 0, 8, 8) == 0 and ws(2, 1, 8, 8, 8, -1) == 0 and ws(2, 0, 8, 8, 8, 8) == 0
    assert ws(2, 4, 8, 8, 8, 8) == 0 and ws(2, 3, 8, 8, -1, 8) == 0
    assert ws(1, 1, 1, 0, 0, 1) == 2 * 8 and ws(3, 2, 257, 256, 0, 256) == 3 * ((2 + 1) + (1 + 1)) * 8
    assert ws(2, 3, 4352, 1024, 256, 5000) == 2 * ((17 + 20) + (4 + 20) + (1 + 20)) * 8
    # per level the pyramid asks for what the single-level entry asks for
    one = lib.sonet_chamfer_loss_ws_size
    assert ws(2, 2, 1280, 256, 0, 5000) == one(2, 1280, 5000) + one(2, 256, 5000)


def test_wrappers_refuse_before_a_device_is_needed():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    pred, gt = torch.zeros(2, 3, 8), torch.zeros(2, 3, 16)
    for fn in (ops.chamfer_pyramid_terms, ops.chamfer_pyramid_loss):
        with pytest.raises(SonetHipError, match="CUDA"):
            fn([pred], gt)
        with pytest.raises(SonetHipError, match="1 to 3"):
            fn([], gt)
        with pytest.raises(SonetHipError, match="1 to 3"):
            fn([pred] * 4, gt)
        with pytest.raises(SonetHipError, match="1 to 3"):
            fn(pred, gt)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.chamfer_pyramid_grad([pred], gt, ops.ChamferPyramidTerms(), torch.zeros(1, 2))
    assert {"levels", "sums", "N"} == set(ops.ChamferPyramidTerms.__slots__)
