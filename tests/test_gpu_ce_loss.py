"""Cross-entropy on the MI355X (sonet_ce_loss_f32 / sonet_ce_grad_f32, ops.ce_terms / ce_loss, models.losses, sonet_hip.metrics): edge
shapes against the restatement of tests/ce_ref.py, the gradient against its derived bound, the exact family bit for bit, the arg-max
rule, non-finite scores, bad targets, buffers and determinism, routing, the option on against off, the reference's fixtures, and the
classification test loop end to end."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import golden
import ce_ref as R
import seg_metrics_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEG_CASES = ("seg_4x50x64", "seg_2x6x257")
CLS_CASE = "cls_16_16_8"
SEG_METRICS_CASES = ("part_sizes_2_3_4_6", "absent_part_and_stray_predictions", "ties_quantised", "one_cloud_all_wrong")
# B x C x N around the workgroup's 256 points, the class extent 256 and the 64 clouds of one finalize workgroup; N = None: the B x C form
SHAPES = [(1, 1, 1), (3, 2, 2), (65, 40, 255), (3, 50, 256), (1, 55, 257), (3, 256, 513), (65, 50, 2), (1, 40, 513), (3, 1, 257),
          (1, 40, None), (63, 40, None), (64, 55, None), (65, 256, None), (257, 40, None), (3, 1, None), (3, 2, None)]
_cache = {}


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(B, C, N):
    """Seeded inputs and their restatement, computed once and shared (never written to)."""
    key = (B, C, N)
    if key not in _cache:
        score, target = R.make_inputs(np.random.RandomState(B * 100003 + C * 1009 + (N or 0)), B, C, N)
        _cache[key] = (score, target, R.ce_terms(score, target))
    return _cache[key]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.maximum(np.abs(b), 1e-300)))


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_C%d_N%s" % s)
def test_forward_matches_the_restatement(shape):
    from sonet_hip import ops
    B, C, N = shape
    score, target, ref = _case(B, C, N)
    ds, dt = _cu(score), _cu(target)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    full = ops.ce_terms(ds, dt, want_pred=True, want_lse=True, confusion=conf)
    lean = ops.ce_terms(ds, dt)
    assert lean.pred is None and lean.lse is None and lean.confusion is None and full.N == (N or 1)
    assert np.array_equal(full.pred.cpu().numpy().astype(np.int64), ref["pred"])
    for t in (full, lean):
        assert np.array_equal(t.correct.cpu().numpy().astype(np.int64), ref["correct"])
        assert np.array_equal(t.bad.cpu().numpy().astype(np.int64), ref["bad"]) and not ref["bad"].any()
        assert torch.equal(t.nll_sum, full.nll_sum)
    assert np.array_equal(conf.cpu().numpy(), ref["confusion"])
    worst = _rel(full.nll_sum.cpu().numpy(), ref["nll_sum"])
    lse_err = float(np.abs(full.lse.cpu().numpy() - ref["lse"]).max())
    loss = ops.ce_loss(ds, dt).item()
    want = np.float32(R.ce_loss(score, target))
    print("forward %s: nll_sum worst relative error %.3g, lse worst error %.3g, loss %.8g against %.8g" % (shape, worst, lse_err, loss, want))
    assert worst <= 1e-12 and lse_err <= 1e-12 * max(1.0, float(np.abs(ref["lse"]).max()))
    assert R.f32_ulp_distance(loss, want) <= 1.0
    total = ops.ce_loss(ds, dt, reduction="sum").item()
    assert R.f32_ulp_distance(total, np.float32(R.ce_loss(score, target, "sum"))) <= 1.0
    conf2 = conf.clone()
    ops.ce_terms(ds, dt, confusion=conf2)                                                  # the table is added to, not overwritten
    assert torch.equal(conf2, 2 * conf)


# ------------------------------------------------------------------------------------------------------------ gradient
def _grad_ratio(g, score, target, reduction, gout, what):
    """worst |g - g64| / bound over the elements of points with finite scores."""
    B, C = score.shape[:2]
    n = 1 if score.ndim == 2 else score.shape[2]
    g64 = R.ce_grad(score, target, reduction, gout)
    scale = 1.0 / (B * n) if reduction == "mean" else 1.0
    bound = R.grad_bound(g64, C, float(np.abs(score).max()), gout, scale)
    ratio = float((np.abs(g.astype(np.float64) - g64) / bound).max())
    print("gradient %s: worst / bound = %.4f (K = %.0f)" % (what, ratio, R.grad_K(C, float(np.abs(score).max()))))
    return ratio


@pytest.mark.parametrize("shape", [(3, 50, 257), (64, 50, 33), (1, 256, 513), (65, 2, 255), (64, 40, None), (257, 55, None), (3, 1, 2)],
                         ids=lambda s: "B%d_C%d_N%s" % s)
def test_gradient_is_within_its_derived_bound(shape):
    from sonet_hip import ops
    B, C, N = shape
    score, target, _ = _case(B, C, N)
    dt = _cu(target)
    worst = 0.0
    for reduction, gout in (("mean", 1.0), ("mean", 3.0), ("sum", 1.0), ("sum", 3.0)):
        ds = _cu(score).requires_grad_(True)
        with ops.kernel_timing() as rec:
            loss = ops.ce_loss(ds, dt, reduction)
            (gout * loss).backward(retain_graph=True)
            first = ds.grad.clone()
            ds.grad = None
            (gout * loss).backward()                                                      # backward twice: the saved lse is read again
            torch.cuda.synchronize()
        assert torch.equal(ds.grad, first)
        assert rec.summary()["ce_loss"]["count"] == 1 and rec.summary()["ce_grad"]["count"] == 2
        assert ds.grad.shape == ds.shape and ds.grad.dtype == torch.float32
        worst = max(worst, _grad_ratio(ds.grad.cpu().numpy(), score, target, reduction, gout, "%s %s gout %g" % (shape, reduction, gout)))
    assert worst < 1.0


@pytest.mark.parametrize("shape", [(1, 8, 256), (4, 2, 64), (256, 4, None), (2, 2, 512), (1, 256, 1024), (4, 1, 64)],
                         ids=lambda s: "B%d_C%d_N%s" % s)
def test_exact_family_bit_for_bit(shape):
    """B N = 256 and two shapes across a workgroup seam (N = 512, 1024): ce_ref.exact_family derives why these bits are exact."""
    from sonet_hip import ops
    B, C, N = shape
    score, target, grad = R.exact_family(B, C, N or 1, np.random.RandomState(7 * C + B))
    if N is None:
        score, target, grad = score[:, :, 0], target[:, 0], grad[:, :, 0]
    ds, dt = _cu(score).requires_grad_(True), _cu(target)
    ops.ce_loss(ds, dt).backward()
    assert np.array_equal(ds.grad.cpu().numpy().view(np.int32), np.ascontiguousarray(grad).view(np.int32))
    t = ops.ce_terms(ds.detach(), dt, want_pred=True)
    assert (t.pred == 0).all() and torch.equal(t.correct.sum(), (dt == 0).sum())
    assert _rel(t.nll_sum.sum().item(), np.log(C) * B * (N or 1)) <= 1e-14 if C > 1 else t.nll_sum.abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------------------ rules
def test_argmax_rule_is_torch_max():
    from sonet_hip import ops
    for seed in range(3):
        s = SR.argmax_rule_inputs(np.random.RandomState(seed))                             # ties, +-0, +-inf columns, NaNs
        want = torch.max(torch.from_numpy(s), dim=1)[1].numpy()
        tgt = np.zeros((1, s.shape[2]), np.int64)
        got = ops.ce_terms(_cu(s), _cu(tgt), want_pred=True)
        assert np.array_equal(got.pred.cpu().numpy(), want), seed
        assert got.correct.item() == int((want == 0).sum())
        rows = np.ascontiguousarray(s[0].T)                                                # the B x C form: one cloud per point
        got = ops.ce_terms(_cu(rows), _cu(tgt[0]), want_pred=True)
        assert np.array_equal(got.pred.cpu().numpy()[:, 0], want[0]), seed


def test_non_finite_scores_stay_in_their_point():
    from sonet_hip import ops
    B, C, N = 3, 6, 300
    score, target, _ = _case(B, C, N)
    score = score.copy()
    score[1, 2, 17] = np.nan                                       # a NaN: its point's gradient and its cloud's sum, nothing else
    score[2, target[2, 290], 290] = -np.inf                        # -inf on the target beside finite scores: an infinite nll
    score[0, :, 5] = -np.inf                                       # nothing but -inf: NaN, as log_softmax
    ds, dt = _cu(score).requires_grad_(True), _cu(target)
    t = ops.ce_terms(ds.detach(), dt, want_lse=True)
    nll = t.nll_sum.cpu().numpy()
    assert np.isnan(nll[0]) and np.isnan(nll[1]) and nll[2] == np.inf and (t.bad == 0).all()
    ops.ce_loss(ds, dt, "sum").backward()
    g = ds.grad.cpu().numpy()
    nan_pts = np.isnan(g).any(axis=1)
    want = np.zeros((B, N), bool)
    want[1, 17] = want[0, 5] = True
    assert np.array_equal(nan_pts, want) and np.isnan(g[1, :, 17]).all() and np.isnan(g[0, :, 5]).all()
    assert g[2, target[2, 290], 290] == -1.0 and np.isfinite(g[2, :, 290]).all()
    clean = ~want
    clean[2, 290] = False
    ref = R.ce_grad(score, target, "sum")
    bound = R.grad_bound(ref, C, 40.0, 1.0, 1.0)
    assert (np.abs(g - ref) <= bound)[np.broadcast_to(clean[:, None, :], g.shape)].all()
    rows = np.ascontiguousarray(score[1].T)                                                # the B x C form
    t = ops.ce_terms(_cu(rows), _cu(target[1]))
    assert torch.isnan(t.nll_sum).nonzero().flatten().tolist() == [17]


@pytest.mark.parametrize("N", [300, None])
def test_bad_targets_add_nothing(N):
    from sonet_hip import ops
    B, C = 4, 7
    score, target, clean = _case(B, C, N)
    t2 = target.copy().reshape(B, -1)
    spots = [(0, 0, -1), (1, 0, C), (2, 0, -100), (3, 0, np.iinfo(np.int64).min)] + ([(1, 299, C + 5), (1, 256, 1 << 40)] if N else [])
    for b, n, v in spots:
        t2[b, n] = v
    t2 = t2.reshape(target.shape)
    ref = R.ce_terms(score, t2)
    ds, dt = _cu(score).requires_grad_(True), _cu(t2)
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    t = ops.ce_terms(ds.detach(), dt, want_pred=True, confusion=conf)
    assert t.bad.cpu().tolist() == ref["bad"].tolist() and sum(ref["bad"]) == len(spots)
    assert np.array_equal(t.correct.cpu().numpy(), ref["correct"]) and np.array_equal(conf.cpu().numpy(), ref["confusion"])
    assert conf.sum().item() == B * (N or 1) - len(spots)
    assert np.array_equal(t.pred.cpu().numpy().astype(np.int64), clean["pred"])          # the prediction does not depend on the target
    assert _rel(t.nll_sum.cpu().numpy(), ref["nll_sum"]) <= 1e-12
    loss, bad = ops.ce_loss(ds, dt, want_bad=True)
    assert R.f32_ulp_distance(loss.item(), np.float32(R.ce_loss(score, t2))) <= 1.0       # the denominator stays B N
    assert torch.equal(bad, t.bad) and not bad.requires_grad
    loss.backward()
    g = ds.grad.cpu().numpy().reshape(B, C, -1)
    for b, n, _ in spots:
        assert (g[b, :, n] == 0).all()
    assert _grad_ratio(ds.grad.cpu().numpy(), score, t2, "mean", 1.0, "bad targets N=%s" % N) < 1.0


# ------------------------------------------------------------------------------------------------------------ buffers, determinism
def _raw_forward(score, target, B, C, N):
    """The C entry on buffers of the test's own, every byte 0xFF beforehand: (lse, nll_sum, pred, correct, bad, ws)."""
    from sonet_hip import _lib, ops
    lib = _lib.load()
    ff = lambda n, dtype: torch.full((n,), -1, dtype=torch.int8, device=DEV).view(dtype)
    lse, nll, ws = ff(8 * B * N, torch.float64), ff(8 * B, torch.float64), ff(lib.sonet_ce_loss_ws_size(B, C, N), torch.float64)
    pred, correct, bad = ff(4 * B * N, torch.int32), ff(4 * B, torch.int32), ff(4 * B, torch.int32)
    ops._launch(DEV, None, lib.sonet_ce_loss_f32, ops.ptr(score), ops.ptr(target), ops.ptr(lse), ops.ptr(nll), ops.ptr(pred), ops.ptr(correct),
                ops.ptr(bad), None, ops.ptr(ws), B, C, N)
    return lse, nll, pred, correct, bad


@pytest.mark.parametrize("shape", [(3, 50, 513), (65, 40, 1)], ids=lambda s: "B%d_C%d_N%d" % s)
def test_outputs_do_not_depend_on_what_the_buffers_held(shape):
    from sonet_hip import _lib, ops
    B, C, N = shape
    score, target, ref = _case(B, C, N if N > 1 else None)
    ds, dt = _cu(score), _cu(target)
    t = ops.ce_terms(ds, dt, want_pred=True, want_lse=True)
    lse, nll, pred, correct, bad = _raw_forward(ds, dt, B, C, N)
    assert torch.equal(lse, t.lse.flatten()) and torch.equal(nll, t.nll_sum) and torch.equal(pred, t.pred.flatten())
    assert torch.equal(correct, t.correct) and torch.equal(bad, t.bad) and np.array_equal(correct.cpu().numpy(), ref["correct"])
    gout = torch.ones((), device=DEV)
    grad = torch.full((4 * B * C * N,), -1, dtype=torch.int8, device=DEV).view(torch.float32)
    ops._launch(DEV, None, _lib.load().sonet_ce_grad_f32, ops.ptr(ds), ops.ptr(dt), ops.ptr(lse), ops.ptr(gout), 1.0 / (B * N), ops.ptr(grad), B, C, N)
    assert torch.equal(grad.view(ds.shape), ops.ce_grad(ds, dt, t.lse, gout, 1.0 / (B * N)))
    # operands one float / one int64 off the start of their allocations, through the wrapper
    buf = torch.zeros(score.size + 1, device=DEV)
    buf[1:] = ds.flatten()
    view = buf[1:].view(ds.shape)
    tb = torch.zeros(target.size + 1, dtype=torch.int64, device=DEV)
    tb[1:] = dt.flatten()
    tview = tb[1:].view(dt.shape)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    o = ops.ce_terms(view, tview, want_pred=True, want_lse=True)
    assert torch.equal(o.lse, t.lse) and torch.equal(o.nll_sum, t.nll_sum) and torch.equal(o.pred, t.pred) and torch.equal(o.correct, t.correct)
    assert torch.equal(ops.ce_grad(view, tview, o.lse, gout, 1.0 / (B * N)), grad.view(ds.shape))


def test_two_runs_and_a_graph_replay_are_bit_identical():
    from sonet_hip import ops
    B, C, N = 3, 50, 513
    score, target, _ = _case(B, C, N)
    ds, dt, gout = _cu(score), _cu(target), torch.full((), 3.0, device=DEV)

    def run():
        t = ops.ce_terms(ds, dt, want_pred=True, want_lse=True)
        return t.nll_sum, t.lse, t.pred, t.correct, ops.ce_grad(ds, dt, t.lse, gout, 1.0 / (B * N))

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        run()                                                                              # (warm-up on the capture stream)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            c = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    ds.mul_(-0.5)                                                                          # the graph reads its operands in place
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(run(), c)) and not torch.equal(a[0], c[0])


# ------------------------------------------------------------------------------------------------------------ routing, on against off
def _parent_seg(inputs, targets):
    """The path of the commit before the option existed, written out."""
    logp = torch.nn.functional.log_softmax(inputs.unsqueeze(3), dim=1)
    return (-torch.gather(logp, 1, targets.unsqueeze(1).unsqueeze(3)).squeeze(1)).mean()


def _loss_and_grad(crit, score, target):
    ds = _cu(score).requires_grad_(True)
    loss = crit(ds, _cu(target))
    loss.backward()
    return loss.detach(), ds.grad


def test_routing_by_kernel_timing():
    from models import losses as LS
    from sonet_hip import ops
    score, target, _ = _case(3, 50, 257)
    rows, labels, _ = _case(64, 40, None)
    for crit, s, t in ((LS.CrossEntropyLossSeg(fused=True), score, target), (LS.CrossEntropyLossCls(fused=True), rows, labels)):
        with ops.kernel_timing() as rec:
            _loss_and_grad(crit, s, t)
            torch.cuda.synchronize()
        assert {k: v["count"] for k, v in rec.summary().items()} == {"ce_loss": 1, "ce_grad": 1}
        assert crit.last_bad.dtype == torch.int32 and crit.last_bad.shape == (s.shape[0],) and not crit.last_bad.any()
        with ops.kernel_timing() as rec:                                                   # no gradient asked for: no lse, no gradient launch
            loss = crit(_cu(s), _cu(t))
            torch.cuda.synchronize()
        assert {k: v["count"] for k, v in rec.summary().items()} == {"ce_loss": 1} and not loss.requires_grad
    seen = []
    real = ops._ce_forward
    try:
        ops._ce_forward = lambda *a: seen.append((a[6], a[7])) or real(*a)                # (want_pred, want_lse) of the launch
        ops.ce_loss(_cu(score), _cu(target))
        ops.ce_loss(_cu(score).requires_grad_(True), _cu(target))
    finally:
        ops._ce_forward = real
    assert seen == [(False, False), (False, True)]
    for crit, s, t, parent in ((LS.CrossEntropyLossSeg(), score, target, _parent_seg), (LS.CrossEntropyLossSeg(fused=False), score, target, _parent_seg),
                               (LS.CrossEntropyLossCls(), rows, labels, torch.nn.CrossEntropyLoss())):
        with ops.kernel_timing() as rec:
            a, b = _loss_and_grad(crit, s, t), _loss_and_grad(crit, s, t)
            torch.cuda.synchronize()
        assert rec.summary() == {} and crit.last_bad is None
        want = _loss_and_grad(parent, s, t)
        for x in (a, b):
            assert torch.equal(x[0], want[0]) and torch.equal(x[1], want[1])
    # what the option does not take goes the parent's way: float64 scores, a class weight, more classes than the extent
    with ops.kernel_timing() as rec:
        LS.CrossEntropyLossSeg(fused=True)(_cu(score).double(), _cu(target))
        LS.CrossEntropyLossSeg(weight=torch.ones(50, device=DEV), fused=True)(_cu(score), _cu(target))
        LS.CrossEntropyLossCls(fused=True)(torch.zeros(2, ops.CE_MAX_C + 1, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
    assert rec.summary() == {}


@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_option_on_against_off(kind):
    from models import losses as LS
    if kind == "seg":
        (score, target, _), on, off = _case(64, 50, 257), LS.CrossEntropyLossSeg(fused=True), LS.CrossEntropyLossSeg()
    else:
        (score, target, _), on, off = _case(64, 40, None), LS.CrossEntropyLossCls(fused=True), LS.CrossEntropyLossCls()
    (l_on, g_on), (l_off, g_off) = _loss_and_grad(on, score, target), _loss_and_grad(off, score, target)
    assert abs(l_on.item() - l_off.item()) <= 1e-6 * abs(l_off.item()), (l_on.item(), l_off.item())
    B, C = score.shape[:2]
    scale = 1.0 / (B * (1 if score.ndim == 2 else score.shape[2]))
    g64 = R.ce_grad(score, target)
    g_on, g_off = g_on.cpu().numpy().astype(np.float64), g_off.cpu().numpy().astype(np.float64)
    bound = R.grad_bound(g64, C, float(np.abs(score).max()), 1.0, scale)
    off_err = np.abs(g_off - g64)
    print("%s: the float32 path's gradient is up to %.1f float32 ulps from float64, the operator's %.3f" %
          (kind, (off_err / R.ulp_f32(g64)).max(), (np.abs(g_on - g64) / R.ulp_f32(g64)).max()))
    assert (np.abs(g_on - g_off) <= off_err + bound).all()


# ------------------------------------------------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("case", SEG_CASES)
def test_segmentation_fixtures_on_the_device(case):
    from models import losses as LS
    g = golden("ce/" + case)
    loss, grad = _loss_and_grad(LS.CrossEntropyLossSeg(fused=True), g["score"], g["target"])
    assert abs(loss.item() - float(g["loss_f32"])) <= 1e-5 * float(g["loss_f32"])
    assert R.f32_ulp_distance(loss.item(), np.float32(g["loss_f64"])) <= 1.0
    B, C, N = g["score"].shape
    bound = R.grad_bound(g["grad_f64"], C, float(np.abs(g["score"]).max()), 1.0, 1.0 / (B * N))
    assert (np.abs(grad.cpu().numpy() - g["grad_f64"]) <= bound).all()


@pytest.mark.parametrize("case", SEG_METRICS_CASES)
def test_segmentation_metrics_fixtures_loss(case):
    """The four fixtures of the segmentation metrics carry the reference's own CrossEntropyLossSeg value."""
    from models import losses as LS
    g = golden("seg_metrics/" + case)
    with torch.no_grad():
        loss = LS.CrossEntropyLossSeg(fused=True)(_cu(g["score"]), _cu(g["seg"]))
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * float(g["loss"]), (loss.item(), float(g["loss"]))


def _cls_batches():
    g = golden("ce/" + CLS_CASE)
    off, out = 0, []
    for n in g["sizes"].tolist():
        out.append((g["score"][off:off + n], g["label"][off:off + n]))
        off += n
    return g, out


def test_classification_fixture_on_the_device():
    from models import losses as LS
    g, batches = _cls_batches()
    off = 0
    for k, (s, l) in enumerate(batches):
        loss, grad = _loss_and_grad(LS.CrossEntropyLossCls(fused=True), s, l)
        assert R.f32_ulp_distance(loss.item(), np.float32(g["loss_f64"][k])) <= 1.0
        want = g["grad_f64"][off:off + len(l)]
        off += len(l)
        assert (np.abs(grad.cpu().numpy() - want) <= R.grad_bound(want, 40, float(np.abs(s).max()), 1.0, 1.0 / len(l))).all()


# ------------------------------------------------------------------------------------------------------------ the test loop
def test_cls_evaluator_against_the_fixture_and_the_restatement():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    from sonet_hip.metrics import ClsEvaluator
    g, batches = _cls_batches()
    ev = ClsEvaluator(40)
    with ops.kernel_timing() as rec:
        for s, l in batches:
            ev.update(_cu(s), _cu(l))
        torch.cuda.synchronize()
    assert rec.summary()["ce_loss"]["count"] == 3 and len(rec.summary()) == 1
    got = ev.result()
    assert abs(got["test_loss"] - float(g["test_loss"])) <= 1e-5 * float(g["test_loss"])
    assert abs(got["test_accuracy"] - float(g["test_accuracy"])) <= float(R.ulp_f32(got["test_accuracy"]))
    ref = R.cls_epoch([s for s, _ in batches], [l for _, l in batches])
    assert abs(got["test_loss"] - ref["test_loss"]) <= 1e-12 * ref["test_loss"] and got["test_accuracy"] == ref["test_accuracy"]
    assert abs(got["class_accuracy"] - ref["class_accuracy"]) <= 1e-12 and got["count"] == 40
    assert got["confusion"].dtype == np.int64 and np.array_equal(got["confusion"], ref["confusion"])
    # uneven batches equal one call; reset() starts over
    ev.reset()
    ev.update(_cu(g["score"]), _cu(g["label"]))
    one = ev.result()
    assert abs(one["test_loss"] - got["test_loss"]) <= 1e-14 * got["test_loss"] and np.array_equal(one["confusion"], got["confusion"])
    assert one["test_accuracy"] == got["test_accuracy"] and one["count"] == 40
    ev.reset()
    with pytest.raises(SonetHipError, match="without any cloud"):
        ev.result()
    bad = g["label"].copy()
    bad[3], bad[30] = 40, -1
    ev.update(_cu(g["score"]), _cu(bad))
    with pytest.raises(SonetHipError, match=r"2 label\(s\) of 40 clouds outside \[0, 40\)"):
        ev.result()
    ev.reset()
    s = g["score"].copy()
    s[5, 2] = np.nan
    ev.update(_cu(s), _cu(g["label"]))
    with pytest.raises(SonetHipError, match="NaN"):
        ev.result()


def test_evaluate_classification_end_to_end():
    """41 clouds of 300 points, 256 sampled, 16 nodes, batches of 16 (the last one of 9): evaluate_classification against a loop written
    by hand from the same forward and the restatement."""
    from models import networks as NW
    from sonet_hip import metrics, ops, synth
    from sonet_hip._lib import SonetHipError
    from sonet_hip.batch import BatchAssembler, DeviceClouds
    S, n, N, M, BS, C = 41, 300, 256, 16, 16, 40
    g = np.random.RandomState(43)
    pts = [g.uniform(-1, 1, size=(n, 3)).astype(np.float32) for _ in range(S)]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = np.stack([p[g.choice(n, M, replace=False)] for p in pts]).astype(np.float32)
    labels = g.randint(0, C, S).astype(np.int64)
    opt = Namespace(gpu_id=0, device=DEV, batch_size=BS, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                    normalization="batch", dropout=0.7, node_num=M, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                    bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=C)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), 17)
    synth.fill_state_dict_(cls.state_dict(), 18)
    enc.to(DEV).train()
    cls.to(DEV).train()                                            # evaluate_classification itself must switch to eval mode
    clouds = DeviceClouds(pts, nrm, labels, nodes=nodes, device=DEV)
    A = BatchAssembler(clouds, opt, "test", "modelnet", seed=4)
    with ops.kernel_timing() as rec:
        got = metrics.evaluate_classification(enc, cls, A, BS)
        torch.cuda.synchronize()
    assert not enc.training and not cls.training and rec.summary()["ce_loss"]["count"] == 3
    scores, labs = [], []
    with torch.no_grad():
        for pc, sn, label, node, knn in A.epoch(0, BS, shuffle=False):
            scores.append(cls(enc(pc, sn, node, knn, False, None)).float().cpu().numpy())
            labs.append(label.cpu().numpy())
    assert [len(l) for l in labs] == [16, 16, 9] and np.array_equal(np.concatenate(labs), labels)
    want = R.cls_epoch(scores, labs)
    print("evaluate_classification", {k: v for k, v in got.items() if k != "confusion"}, "hand-run loop", want["test_loss"], want["test_accuracy"])
    assert got["count"] == S and got["test_accuracy"] == want["test_accuracy"] and np.array_equal(got["confusion"], want["confusion"])
    assert abs(got["test_loss"] - want["test_loss"]) <= 1e-12 * want["test_loss"]
    assert abs(got["class_accuracy"] - want["class_accuracy"]) <= 1e-12
    with pytest.raises(SonetHipError, match="test-mode"):
        metrics.evaluate_classification(enc, cls, BatchAssembler(clouds, opt, "train", "modelnet", seed=4), BS)


def test_wrappers_refuse_bad_cuda_arguments():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    score, target = torch.zeros(2, 50, 8, device=DEV), torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    for bad_call, match in ((lambda: ops.ce_terms(score.double(), target), "float32"), (lambda: ops.ce_terms(score, target.int()), "int64"),
                            (lambda: ops.ce_terms(torch.zeros(2, 8, 50, device=DEV).transpose(1, 2), target), "contiguous"),
                            (lambda: ops.ce_terms(score, target[:, :7].contiguous()), "B x N"),
                            (lambda: ops.ce_terms(score, target.cpu()), "CUDA"),
                            (lambda: ops.ce_terms(torch.zeros(1, ops.CE_MAX_C + 1, 4, device=DEV), target[:1, :4].contiguous()), "C <="),
                            (lambda: ops.ce_terms(score, target, confusion=torch.zeros(50, 49, dtype=torch.int64, device=DEV)), "C x C"),
                            (lambda: ops.ce_terms(score, target, confusion=torch.zeros(50, 50, dtype=torch.int32, device=DEV)), "int64"),
                            (lambda: ops.ce_grad(score, target, torch.zeros(15, dtype=torch.float64, device=DEV), torch.ones((), device=DEV), 1.0),
                             "lse must hold"),
                            (lambda: ops.ce_loss(score[:, :, 0].contiguous(), target), "2-D|1-D")):
        with pytest.raises(SonetHipError, match=match):
            bad_call()
