"""Cross-entropy without a GPU: the numpy restatement (tests/ce_ref.py) against torch's float64 cross_entropy and autograd, against the
fixtures of the live reference (tests/golden/ce, tools/make_ce_golden.py) and against the reference itself where it is mounted; the
exact family, derived; the five deliberate breaks of the restatement, each red in the check meant for it; the C entries' argument checks;
what the wrappers, the evaluator and the loss classes refuse or route before a device is needed."""
import ctypes
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, golden
import ce_ref as R

SEG_CASES = ("seg_4x50x64", "seg_2x6x257")
CLS_CASE = "cls_16_16_8"
TOL = 1e-12                    # the project's figure for a restatement against float64 autograd


def _torch64(score, target, reduction, **kw):
    s = torch.from_numpy(np.asarray(score, np.float64)).requires_grad_(True)
    loss = F.cross_entropy(s, torch.from_numpy(target), reduction=reduction, **kw)
    loss.backward()
    return loss.item(), s.grad.numpy()


def _check_against_torch(score, target, reduction, brk=None, **kw):
    want, gwant = _torch64(score, target, reduction, **kw)
    got, g = R.ce_loss(score, target, reduction, brk=brk), R.ce_grad(score, target, reduction, brk=brk)
    assert abs(got - want) <= TOL * max(abs(want), 1.0), (got, want)
    assert np.abs(g - gwant).max() <= TOL * max(np.abs(gwant).max(), 1e-300), np.abs(g - gwant).max()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("shape", [(7, 40, None), (1, 1, None), (3, 50, 33), (2, 2, 257), (64, 50, 5)])
def test_restatement_matches_torch_float64(shape, reduction):
    B, C, N = shape
    score, target = R.make_inputs(np.random.RandomState(B * 1000 + C), B, C, N)
    _check_against_torch(score, target, reduction)


def _check_seg_fixture(case, brk=None):
    g = golden("ce/" + case)
    score, target = g["score"], g["target"]
    assert score.dtype == np.float32 and target.dtype == np.int64 and g["loss_f32"].dtype == np.float32
    loss = R.ce_loss(score, target, brk=brk)
    assert abs(loss - float(g["loss_f64"])) <= TOL * abs(float(g["loss_f64"])), (loss, float(g["loss_f64"]))
    grad = R.ce_grad(score, target, brk=brk)
    assert np.abs(grad - g["grad_f64"]).max() <= TOL * np.abs(g["grad_f64"]).max()
    assert abs(loss - float(g["loss_f32"])) <= 1e-5 * abs(float(g["loss_f32"])), (loss, float(g["loss_f32"]))


@pytest.mark.parametrize("case", SEG_CASES)
def test_restatement_matches_the_segmentation_fixtures(case):
    _check_seg_fixture(case)


def _check_cls_fixture(brk=None):
    g = golden("ce/" + CLS_CASE)
    score, label, sizes = g["score"], g["label"], g["sizes"].tolist()
    assert sizes == [16, 16, 8] and score.shape == (40, 40) and g["test_loss"].dtype == g["test_accuracy"].dtype == np.float32
    off, scores, labels = 0, [], []
    for k, n in enumerate(sizes):
        s, l = score[off:off + n], label[off:off + n]
        off += n
        loss = R.ce_loss(s, l, brk=brk)
        assert abs(loss - g["loss_f64"][k]) <= TOL * g["loss_f64"][k], (k, loss, g["loss_f64"][k])
        grad = R.ce_grad(s, l, brk=brk)
        assert np.abs(grad - g["grad_f64"][off - n:off]).max() <= TOL * np.abs(g["grad_f64"]).max()
        scores.append(s)
        labels.append(l)
    ep = R.cls_epoch(scores, labels)
    assert abs(ep["test_loss"] - float(g["test_loss"])) <= 1e-5 * float(g["test_loss"])
    # within one float32 rounding of the exact ratio
    assert abs(ep["test_accuracy"] - float(g["test_accuracy"])) <= float(R.ulp_f32(ep["test_accuracy"]))
    assert ep["count"] == 40 and ep["confusion"].sum() == 40 and ep["confusion"].trace() == round(ep["test_accuracy"] * 40)
    assert 0.0 < ep["class_accuracy"] <= 1.0


def test_restatement_matches_the_classification_fixture():
    _check_cls_fixture()


@pytest.mark.parametrize("shape", [(4, 8, 64), (1, 1, 1), (2, 256, 128), (1, 2, 512), (256, 4, 1)])
def test_exact_family_is_exact(shape):
    """ce_ref.exact_family's docstring derives it; here the float64 restatement, rounded once to float32, gives those bits."""
    B, C, N = shape
    score, target, grad = R.exact_family(B, C, N, np.random.RandomState(C))
    assert (score == score[:, :1]).all()
    got = R.ce_grad(score, target).astype(np.float32)
    assert np.array_equal(got.view(np.int32), grad.view(np.int32))
    r = R.ce_terms(score, target)
    assert (r["pred"] == 0).all() and np.array_equal(r["pred"], torch.max(torch.from_numpy(score), dim=1)[1].numpy())
    assert np.abs(r["nll"] - np.log(C)).max() <= 16 * 2.0 ** -52                   # (m - x_t) = 0: nll is log(C) up to lse's rounding
    assert np.array_equal(r["correct"], (target == 0).sum(axis=1))


def _bad_target_case():
    score, target = R.make_inputs(np.random.RandomState(9), 3, 6, 40)
    target = target.copy()
    target[0, 3] = target[1, 7] = target[1, 8] = -1
    return score, target


def _check_bad_targets(brk=None):
    """torch's sum with ignore_index = -1 adds nothing for such a point and gives it a zero gradient: the contract's rule."""
    score, target = _bad_target_case()
    _check_against_torch(score, target, "sum", brk=brk, ignore_index=-1)
    r = R.ce_terms(score, target, brk)
    assert r["bad"].tolist() == [1, 2, 0] and r["confusion"].sum() == 3 * 40 - 3


def _check_large_scores(brk=None):
    score, target = R.make_inputs(np.random.RandomState(10), 2, 5, 9)
    _check_against_torch(score * np.float32(200.0), target, "mean", brk=brk)


BREAK_CHECKS = {
    "no_onehot": lambda brk: _check_seg_fixture(SEG_CASES[0], brk),
    "denominator_minus_one": lambda brk: _check_seg_fixture(SEG_CASES[1], brk),
    "skip_last_class": lambda brk: _check_cls_fixture(brk),
    "lse_without_max": _check_large_scores,
    "count_bad_target": _check_bad_targets,
}


@pytest.mark.parametrize("brk", R.BREAKS)
def test_each_break_turns_its_check_red(brk):
    assert set(BREAK_CHECKS) == set(R.BREAKS)
    BREAK_CHECKS[brk](None)                          # green as it stands
    with pytest.raises(AssertionError):
        BREAK_CHECKS[brk](brk)


def test_bound_helpers():
    assert R.ulp_f32(1.0) == 2.0 ** -23 and R.ulp_f32(1.5) == 2.0 ** -23 and R.ulp_f32(0.75) == 2.0 ** -24
    assert R.ulp_f32(0.0) == 2.0 ** -149 and R.ulp_f32(1e-40) == 2.0 ** -149
    assert R.grad_K(50, 20.0) == 2.0 * (250.0 + 2.0 * np.log(50.0) + 26.0)
    # the bound is the float32 rounding everywhere but where p - 1 cancels
    assert R.grad_bound(np.array([1e-3]), 50, 20.0, 1.0, 1.0 / 4096)[0] < 1.0001 * R.ulp_f32(1e-3)


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="reference checkout not mounted")
def test_fixtures_regenerate_and_restatement_equals_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_ce_golden.py"), "--check"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "fixtures regenerate bit-identically" in out and "restatement == live reference" in out


def test_fixtures_hold_data_only():
    for case in SEG_CASES + (CLS_CASE,):
        path = os.path.join(ROOT, "tests", "golden", "ce", case + ".npz")
        assert os.path.getsize(path) < 256 * 1024
        g = np.load(path, allow_pickle=False)
        assert all(g[k].dtype.kind in "fi" for k in g.files), case


# ------------------------------------------------------------------------------------------------------------ refusals, no device
def test_c_entries_reject_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    base = ctypes.addressof(buf)
    assert base % 8 == 0
    p, p4 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def loss(B=1, C=2, N=4, **over):
        names = ("score", "target", "lse", "nll_sum", "pred", "correct", "bad", "confusion", "ws")
        a = {k: over.get(k, p) for k in names}
        return lib.sonet_ce_loss_f32(*[a[k] for k in names], B, C, N, None)

    def grad(B=1, C=2, N=4, scale=1.0, **over):
        names = ("score", "target", "lse", "gout")
        a = {k: over.get(k, p) for k in names}
        return lib.sonet_ce_grad_f32(a["score"], a["target"], a["lse"], a["gout"], scale, over.get("grad", p), B, C, N, None)

    for name in ("score", "target", "nll_sum", "correct", "bad", "ws"):
        assert loss(**{name: None}) == 1 and "NULL" in _lib.last_error(), name
    for name in ("score", "target", "lse", "gout", "grad"):
        assert grad(**{name: None}) == 1 and "NULL" in _lib.last_error(), name
    for call in (loss, grad):
        for kw in (dict(B=0), dict(C=0), dict(N=0), dict(B=-1), dict(N=-5)):
            assert call(**kw) == 1 and "non-positive" in _lib.last_error(), kw
        cmax = lib.sonet_ce_max_c()
        assert call(C=cmax + 1) == 2 and "C=%d" % (cmax + 1) in _lib.last_error()
        assert call(B=65535, N=32769) == 2 and "2^31" in _lib.last_error()
        assert call(B=1 << 16, N=2) == 2 and "65535" in _lib.last_error()
        assert call(lse=p4) == 1 and "aligned" in _lib.last_error()
        assert call(target=p4) == 1 and "aligned" in _lib.last_error()
    assert loss(nll_sum=p4) == 1 and "aligned" in _lib.last_error()
    assert loss(confusion=p4) == 1 and "aligned" in _lib.last_error()
    size = lib.sonet_ce_loss_ws_size
    assert size(0, 50, 1024) == 0 and size(2, 0, 8) == 0 and size(2, 50, -1) == 0
    blk = lib.sonet_ce_block_points()
    assert size(3, 50, blk + 1) == 3 * 2 * 16 and size(1, 1, blk) == 16 and size(5, 40, 1) == 16


def test_torch_builds_no_misaligned_int64_or_float64_view():
    """Why the wrappers carry no copy for a target or lse at a 4-byte offset: torch refuses to build such a tensor, so the C entries'
    alignment refusals (above) are the only place the case can arise."""
    raw = torch.zeros(64, dtype=torch.uint8)
    for dtype in (torch.int64, torch.float64):
        with pytest.raises(RuntimeError):
            raw[4:36].view(dtype)
        assert raw[8:40].view(dtype).data_ptr() % 8 == 0


def test_exported_extents_equal_the_wrappers_constants():
    from sonet_hip import _lib, ops
    lib = _lib.load()
    assert lib.sonet_ce_max_c() == ops.CE_MAX_C and lib.sonet_ce_block_points() == ops.CE_BLOCK_POINTS
    assert ops.ce_supported(ops.CE_MAX_C) and not ops.ce_supported(ops.CE_MAX_C + 1) and not ops.ce_supported(0)
    assert not ops.ce_supported(4, 65536, 2) and ops.ce_supported(4, 65536, 1) and not ops.ce_supported(4, 1 << 31, 1)


def test_wrappers_refuse_before_a_device_is_needed():
    from sonet_hip import metrics, ops
    from sonet_hip._lib import SonetHipError
    score, target = torch.zeros(2, 50, 8), torch.zeros(2, 8, dtype=torch.int64)
    for call in (lambda: ops.ce_terms(score, target), lambda: ops.ce_loss(score, target),
                 lambda: ops.ce_loss(score[:, :, 0].contiguous(), target[:, 0].contiguous()),
                 lambda: ops.ce_grad(score, target, torch.zeros(16, dtype=torch.float64), torch.ones(()), 1.0),
                 lambda: metrics.ClsEvaluator(50).update(score[:, :, 0].contiguous(), target[:, 0].contiguous())):
        with pytest.raises(SonetHipError, match="CUDA"):
            call()
    with pytest.raises(SonetHipError, match="B x C x N or B x C"):
        ops.ce_terms(torch.zeros(2, 3, 4, 5), target)
    with pytest.raises(SonetHipError, match="reduction"):
        ops.ce_loss(score, target, reduction="none")
    with pytest.raises(SonetHipError, match="before any update"):
        metrics.ClsEvaluator(40).result()
    with pytest.raises(SonetHipError, match="classes must be"):
        metrics.ClsEvaluator(ops.CE_MAX_C + 1)
    with pytest.raises(SonetHipError, match="holds 40"):
        metrics.ClsEvaluator(40).update(torch.zeros(2, 41), torch.zeros(2, dtype=torch.int64))
    for recipe, mode in (("modelnet", "train"), ("shapenet", "test"), ("shrec", "train")):
        with pytest.raises(SonetHipError, match="test-mode modelnet or shrec"):
            metrics.evaluate_classification(None, None, Namespace(recipe=recipe, mode=mode), 16)


class _Fake:
    """What the routing rule asks of a tensor."""

    def __init__(self, shape, dtype, is_cuda=True):
        self.shape, self.dtype, self.is_cuda = tuple(shape), dtype, is_cuda

    def dim(self):
        return len(self.shape)


def test_routing_only_the_option_on_cuda_float32_reaches_the_operator(monkeypatch):
    from models import losses as LS
    calls = []

    def counting(score, target, reduction="mean", want_bad=False):
        calls.append(reduction)
        raise AssertionError("the operator was reached")

    monkeypatch.setattr(LS._ops, "ce_loss", counting)
    g = torch.Generator().manual_seed(1)
    s3, t3 = torch.randn(2, 5, 7, generator=g), torch.randint(0, 5, (2, 7), generator=g)
    s2, t2 = torch.randn(4, 5, generator=g), torch.randint(0, 5, (4,), generator=g)
    want3, want2 = F.cross_entropy(s3, t3), F.cross_entropy(s2, t2)
    for crit in (LS.CrossEntropyLossSeg(), LS.CrossEntropyLossSeg(fused=False), LS.CrossEntropyLossSeg(fused=True)):      # CPU tensors
        assert torch.allclose(crit(s3, t3), want3, rtol=1e-6) and crit.last_bad is None
    assert torch.allclose(LS.CrossEntropyLossSeg(fused=True)(s3.double(), t3), F.cross_entropy(s3.double(), t3), rtol=1e-12)
    w = torch.rand(5, generator=g) + 0.5
    assert torch.allclose(LS.CrossEntropyLossSeg(weight=w, fused=True)(s3, t3), F.cross_entropy(s3, t3, weight=w), rtol=1e-6)
    for crit in (LS.CrossEntropyLossCls(), LS.CrossEntropyLossCls(fused=True)):
        assert torch.equal(crit(s2, t2), want2) and crit.last_bad is None
    assert torch.equal(LS.CrossEntropyLossCls(fused=True)(s2.double(), t2), F.cross_entropy(s2.double(), t2))
    assert calls == []
    # the rule itself, on stand-ins for CUDA tensors: what reaches the operator and what does not
    f32, i64 = torch.float32, torch.int64
    rule = LS._takes_ce_operator
    assert rule(True, _Fake((2, 50, 8), f32), _Fake((2, 8), i64), None, 3) and rule(True, _Fake((4, 40), f32), _Fake((4,), i64), None, 2)
    assert not rule(False, _Fake((2, 50, 8), f32), _Fake((2, 8), i64), None, 3)
    assert not rule(True, _Fake((2, 50, 8), f32), _Fake((2, 8), i64), w, 3)
    assert not rule(True, _Fake((2, 50, 8), f32, False), _Fake((2, 8), i64), None, 3)
    assert not rule(True, _Fake((2, 50, 8), torch.float64), _Fake((2, 8), i64), None, 3)
    assert not rule(True, _Fake((2, 50, 8), torch.bfloat16), _Fake((2, 8), i64), None, 3)
    assert not rule(True, _Fake((2, 257, 8), f32), _Fake((2, 8), i64), None, 3)
    assert not rule(True, _Fake((2, 50, 8), f32), _Fake((2, 8), torch.int32), None, 3)
    assert not rule(True, _Fake((2, 50), f32), _Fake((2,), i64), None, 3)
