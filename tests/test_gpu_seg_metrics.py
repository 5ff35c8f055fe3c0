"""Segmentation metrics on the MI355X (sonet_seg_metrics_f32, sonet_hip.metrics): the reference's fixtures, edge shapes against the
restatement of tests/seg_metrics_ref.py, the arg-max rule, bad inputs, determinism, and an evaluation epoch end to end.

Integers (pred, correct, the three count tables, bad) are exact and the IoU is bit-equal everywhere; the loss is held to 1e-5
relative, the project's f32 parity bar (the kernel's per-point NLL is float32, the restatement's float64)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import golden
import seg_metrics_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = ("part_sizes_2_3_4_6", "absent_part_and_stray_predictions", "ties_quantised", "one_cloud_all_wrong")
BLOCK = 256                                   # points per workgroup of seg_metrics_kernel (SM_THREADS)
LOSS_REL = 1e-5


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _compare(m, ref, N, what, pred=False, rows=None):
    """m: ops.SegMetrics, ref: the restatement's dict -> worst loss error / bound over the compared clouds."""
    rows = np.arange(len(ref["iou"])) if rows is None else np.asarray(rows)
    for k in ("correct", "inter", "pred_cnt", "gt_cnt", "bad"):
        got = getattr(m, k).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got[rows], ref[k][rows]), "%s: %s differs" % (what, k)
    if pred:
        assert m.pred.dtype == torch.int32 and np.array_equal(m.pred.cpu().numpy()[rows], ref["pred"][rows]), "%s: pred" % what
    else:
        assert m.pred is None
    iou, nll = m.iou.cpu().numpy(), m.nll_sum.cpu().numpy()
    assert iou.dtype == nll.dtype == np.float64
    assert np.array_equal(_bits(iou[rows]), _bits(ref["iou"][rows])), "%s: iou %s vs %s" % (what, iou[rows], ref["iou"][rows])
    got, want = nll[rows] / N, ref["nll_sum"][rows] / N
    err = np.abs(got - want)
    assert (err <= LOSS_REL * np.abs(want)).all(), "%s: loss off by up to %.3g x bound" % (
        what, float((err / np.maximum(LOSS_REL * np.abs(want), 1e-300)).max()))
    nz = want != 0
    return float((err[nz] / (LOSS_REL * np.abs(want[nz]))).max()) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", CASES)
def test_fixtures_of_the_live_reference(case):
    from sonet_hip import metrics, ops
    g = golden("seg_metrics/" + case)
    score, seg, label = g["score"], g["seg"], g["label"]
    N = score.shape[2]
    ref = R.seg_metrics(score, seg, label)
    m = ops.seg_metrics(_cu(score), _cu(seg), _cu(label), want_pred=True)
    worst = _compare(m, ref, N, case, pred=True)
    print("%s: worst loss error / bound = %.3g" % (case, worst))
    assert np.array_equal(_bits(m.iou.cpu().numpy()), _bits(g["iou_per_cloud"]))
    assert np.array_equal(m.union.cpu().numpy(), ref["pred_cnt"] + ref["gt_cnt"] - ref["inter"])
    assert np.array_equal(_bits(metrics.seg_iou(_cu(score), _cu(seg), _cu(label)).cpu().numpy()), _bits(g["iou_per_cloud"]))
    assert np.float32(int(m.correct.sum()) / (score.shape[0] * N)) == g["accuracy"]


def test_evaluator_over_the_fixtures_equals_the_reference_epoch():
    """Fed one fixture at a time, against the reference's accumulation of its own batch values (part-seg/train.py:87-104)."""
    from sonet_hip.metrics import SegEvaluator
    ev, acc = SegEvaluator(), R.Accumulator()
    for case in CASES:
        g = golden("seg_metrics/" + case)
        ev.update(_cu(g["score"]), _cu(g["seg"]), _cu(g["label"]))
        acc.add(float(g["loss"]), float(g["accuracy"]), float(g["iou_batch"]), len(g["label"]))
    got, want = ev.result(), acc.result()
    print("evaluator", got, "reference", want)
    assert sorted(got) == ["count", "test_acc_seg", "test_iou", "test_loss_seg"] and got["count"] == want["count"] == 12
    assert abs(got["test_iou"] - want["test_iou"]) <= 1e-12
    assert abs(got["test_acc_seg"] - want["test_acc_seg"]) <= 1e-12
    assert abs(got["test_loss_seg"] - want["test_loss_seg"]) <= LOSS_REL * abs(want["test_loss_seg"])
    ev.reset()
    g = golden("seg_metrics/" + CASES[0])
    ev.update(_cu(g["score"]), _cu(g["seg"]), _cu(g["label"]))
    one = ev.result()
    assert one["count"] == 4 and abs(one["test_iou"] - float(g["iou_batch"])) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ edge shapes
def _bump(C):
    """A bump that leaves 60-95 % of the points right against C - 1 unit-normal competitors."""
    return {1: 1.0, 2: 1.0}.get(C, 3.5 if C <= 64 else 4.2)


@pytest.mark.parametrize("C", [1, 2, 50, 64, 256])
def test_edge_shapes_against_the_restatement(C):
    """N around the workgroup's 256 points (one short, exact, one past = the first size with a second workgroup), four and five
    workgroups with a ragged last one, B of 1 and 3; with and without pred_out; score as a contiguous view 4 bytes into a buffer."""
    from sonet_hip import ops
    table = R.two_category_table(C)
    n_cat = len(table) - 1
    worst = 0.0
    for N in (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 1023, 1025):
        for B in (1, 3):
            g = np.random.RandomState(1000 * C + 10 * N + B)
            labels = [(b + N) % n_cat for b in range(B)]
            score, seg, label = R.make_inputs(g, labels, N, C=C, part_offsets=table, bump=_bump(C),
                                              stray=(1,) if (B > 1 and n_cat > 1) else ())
            ref = R.seg_metrics(score, seg, label, table)
            ds, dg, dl = _cu(score), _cu(seg), _cu(label)
            what = "C=%d N=%d B=%d" % (C, N, B)
            worst = max(worst, _compare(ops.seg_metrics(ds, dg, dl, table), ref, N, what))
            worst = max(worst, _compare(ops.seg_metrics(ds, dg, dl, table, want_pred=True), ref, N, what + " pred", pred=True))
            buf = torch.full((score.size + 3,), float("nan"), dtype=torch.float32, device=DEV)
            view = buf[1:1 + score.size].view(B, C, N)
            view.copy_(ds)
            assert view.is_contiguous() and view.data_ptr() % 8 == 4
            worst = max(worst, _compare(ops.seg_metrics(view, dg, dl, table, want_pred=True), ref, N, what + " offset view", pred=True))
    print("C=%d: worst loss error / bound = %.3g" % (C, worst))


def test_argmax_rule_on_the_device():
    from sonet_hip import ops
    for seed in range(4):
        s = R.argmax_rule_inputs(np.random.RandomState(seed))
        want = torch.max(torch.from_numpy(s), dim=1)[1].numpy()
        B, C, N = s.shape
        m = ops.seg_metrics(_cu(s), torch.zeros((B, N), dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV),
                            part_offsets=(0, C), want_pred=True)
        assert np.array_equal(m.pred.cpu().numpy(), want), seed
        assert np.array_equal(m.pred_cnt.cpu().numpy()[0], np.bincount(want[0], minlength=C))
    for case in CASES:
        g = golden("seg_metrics/" + case)
        m = ops.seg_metrics(_cu(g["score"]), _cu(g["seg"]), _cu(g["label"]), want_pred=True)
        assert np.array_equal(m.pred.cpu().numpy(), torch.max(torch.from_numpy(g["score"]), dim=1)[1].numpy())


# ------------------------------------------------------------------------------------------------------------ bad inputs
def test_bad_inputs_are_flagged_per_cloud_and_stop_the_evaluator():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    from sonet_hip.metrics import SegEvaluator
    N = 300
    score, seg, label = R.make_inputs(np.random.RandomState(9), [0, 1, 2, 3, 4], N, bump=3.5)
    seg2, label2 = seg.copy(), label.copy()
    seg2[0, 17], seg2[1, 299], label2[3] = -1, 50, 16            # one seg of -1, one seg of C, one label of n_cat
    ref = R.seg_metrics(score, seg2, label2)
    assert ref["bad"].tolist() == [1, 1, 0, 1, 0]
    m = ops.seg_metrics(_cu(score), _cu(seg2), _cu(label2), want_pred=True)
    assert m.bad.cpu().tolist() == [1, 1, 0, 1, 0]
    nll, iou = m.nll_sum.cpu().numpy(), m.iou.cpu().numpy()
    assert np.isnan(nll[[0, 1, 3]]).all() and np.isnan(iou[3]) and not np.isnan(iou[[0, 1, 2, 4]]).any()
    for k in ("correct", "inter", "pred_cnt", "gt_cnt"):            # the flagged clouds still count what is countable
        assert np.array_equal(getattr(m, k).cpu().numpy(), ref[k]), k
    assert np.array_equal(_bits(iou[[0, 1]]), _bits(ref["iou"][[0, 1]]))
    _compare(m, ref, N, "clean clouds beside bad ones", pred=True, rows=[2, 4])
    clean = R.seg_metrics(score, seg, label)
    assert np.array_equal(_bits(iou[[2, 4]]), _bits(clean["iou"][[2, 4]]))
    ev = SegEvaluator()
    ev.update(_cu(score), _cu(seg2), _cu(label2))
    with pytest.raises(SonetHipError, match="3 bad cloud"):
        ev.result()
    ev.reset()
    ev.update(_cu(score), _cu(seg), _cu(label))
    got = ev.result()
    loss, acc, miou, _ = R.batch_report(score, seg, label)
    assert got["count"] == 5 and abs(got["test_iou"] - miou) <= 1e-12 and abs(got["test_acc_seg"] - acc) <= 1e-12
    assert abs(got["test_loss_seg"] - loss) <= LOSS_REL * loss


def test_non_finite_scores_make_the_loss_nan_without_a_bad_flag():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    from sonet_hip.metrics import SegEvaluator
    score, seg, label = R.make_inputs(np.random.RandomState(10), [0, 1, 2], 70, bump=3.5)
    score[0, 5, 9], score[1, :, 3] = np.nan, -np.inf
    ref = R.seg_metrics(score, seg, label)
    m = ops.seg_metrics(_cu(score), _cu(seg), _cu(label), want_pred=True)
    assert m.bad.cpu().tolist() == [0, 0, 0]
    nll = m.nll_sum.cpu().numpy()
    assert np.isnan(nll[:2]).all() and np.isnan(ref["nll_sum"][:2]).all()
    _compare(m, ref, 70, "cloud beside non-finite ones", pred=True, rows=[2])
    assert np.array_equal(m.pred.cpu().numpy(), ref["pred"]) and np.array_equal(_bits(m.iou.cpu().numpy()), _bits(ref["iou"]))
    ev = SegEvaluator()
    ev.update(_cu(score), _cu(seg), _cu(label))
    with pytest.raises(SonetHipError, match="NaN"):
        ev.result()


def test_wrapper_refuses_wrong_dtypes_layouts_and_tables():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    score = torch.zeros(2, 50, 8, device=DEV)
    seg, label = torch.zeros(2, 8, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(SonetHipError, match="float32"):
        ops.seg_metrics(score.double(), seg, label)
    with pytest.raises(SonetHipError, match="int64"):
        ops.seg_metrics(score, seg.int(), label)
    with pytest.raises(SonetHipError, match="int64"):
        ops.seg_metrics(score, seg, label.int())
    with pytest.raises(SonetHipError, match="contiguous"):
        ops.seg_metrics(torch.zeros(2, 8, 50, device=DEV).transpose(1, 2), seg, label)
    with pytest.raises(SonetHipError, match="B x N"):
        ops.seg_metrics(score, seg[:, :7].contiguous(), label)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.seg_metrics(score, seg.cpu(), label)
    with pytest.raises(SonetHipError, match="C <= 256|<= 256"):
        ops.seg_metrics(torch.zeros(1, 257, 4, device=DEV), seg[:1, :4].contiguous(), label[:1], part_offsets=(0, 257))
    for bad in ((0, 4, 4, 50), (0, 6, 4, 50), (1, 4, 50), (0, 25, 51)):
        with pytest.raises(SonetHipError, match="part_offsets"):
            ops.seg_metrics(score, seg, label, part_offsets=bad)


# ------------------------------------------------------------------------------------------------------------ determinism
def test_two_runs_give_the_same_bits():
    from sonet_hip import ops
    score, seg, label = R.make_inputs(np.random.RandomState(21), [10, 0, 5], 1025, bump=3.5)
    ds, dg, dl = _cu(score), _cu(seg), _cu(label)
    a, b = ops.seg_metrics(ds, dg, dl), ops.seg_metrics(ds, dg, dl)
    torch.cuda.synchronize()
    assert torch.equal(a.nll_sum.view(torch.int64), b.nll_sum.view(torch.int64))
    assert torch.equal(a.iou.view(torch.int64), b.iou.view(torch.int64))
    assert torch.equal(a.inter, b.inter) and torch.equal(a.correct, b.correct)
    assert torch.isfinite(a.nll_sum).all() and a.nll_sum.data_ptr() != b.nll_sum.data_ptr()


# ------------------------------------------------------------------------------------------------------------ end to end
def test_evaluation_epoch_end_to_end():
    """5 clouds of 300 points, 256 sampled, 16 nodes, batches of 2 (the last one short): evaluate_segmentation against the restatement
    applied per batch to the same forwards' scores on the host, accumulated as the reference's test loop does."""
    from models import networks as NW
    from sonet_hip import metrics, ops, synth
    from sonet_hip.batch import BatchAssembler, DeviceClouds
    S, n, N, M, BS = 5, 300, 256, 16, 2
    g = np.random.RandomState(31)
    off = R.SHAPENET_PART_OFFSETS
    labels = np.array([0, 10, 5, 1, 15])
    pts = [g.normal(size=(n, 3)).astype(np.float32) for _ in range(S)]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = np.stack([p[g.choice(n, M, replace=False)] for p in pts]).astype(np.float32)
    opt = Namespace(gpu_id=0, device=DEV, batch_size=BS, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                    normalization="batch", dropout=0.6, node_num=M, k=3, som_k=9, som_k_type="center", bn_momentum=0.1,
                    bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=50)
    enc, seg = NW.Encoder(opt), NW.Segmenter(opt)
    synth.fill_state_dict_(enc.state_dict(), 5)
    synth.fill_state_dict_(seg.state_dict(), 6)
    enc.to(DEV).eval()
    seg.to(DEV).eval()
    # Seeded weights predict what they like: the ground truth is made FROM a first pass, so that the epoch has something to count.  With
    # the global point index as "part label" the assembler hands out which source point every sampled point is (the draws depend on
    # seed, step and slot only); 70 % of the sampled points then get the predicted part as their label, the others (and the points never
    # sampled) a part of the cloud's category.
    index_clouds = DeviceClouds(pts, nrm, labels, nodes=nodes, seg=[np.arange(i * n, (i + 1) * n) for i in range(S)], device=DEV)
    truth = np.concatenate([g.randint(off[c], off[c + 1], n) for c in labels])
    with torch.no_grad():
        for pc, sn, label, chosen, node, knn in BatchAssembler(index_clouds, opt, "test", "shapenet", seed=4).epoch(0, BS, shuffle=False):
            pred = NW.segmentation_forward(enc, seg, pc, sn, label, node, knn).float().argmax(dim=1).cpu().numpy().reshape(-1)
            chosen = chosen.cpu().numpy().reshape(-1)
            keep = g.uniform(size=chosen.shape) < 0.7
            truth[chosen[keep]] = pred[keep]
    clouds = DeviceClouds(pts, nrm, labels, nodes=nodes, seg=[truth[i * n:(i + 1) * n] for i in range(S)], device=DEV)
    A = BatchAssembler(clouds, opt, "test", "shapenet", seed=4)
    enc.train()
    seg.train()                                                    # evaluate_segmentation itself must switch to eval mode
    with ops.kernel_timing() as rec:
        got = metrics.evaluate_segmentation(enc, seg, A, BS)
        torch.cuda.synchronize()
    assert not enc.training and not seg.training
    assert rec.summary()["seg_metrics"]["count"] == 3
    acc, sizes = R.Accumulator(), []
    with torch.no_grad():
        for pc, sn, label, sg, node, knn in A.epoch(0, BS, shuffle=False):
            score = NW.segmentation_forward(enc, seg, pc, sn, label, node, knn).float()
            assert tuple(score.shape) == (pc.shape[0], 50, N)
            loss, a, miou, _ = R.batch_report(score.cpu().numpy(), sg.cpu().numpy(), label.cpu().numpy())
            acc.add(loss, a, miou, pc.shape[0])
            sizes.append(pc.shape[0])
    want = acc.result()
    print("evaluate_segmentation", got, "restatement", want)
    assert sizes == [2, 2, 1] and got["count"] == want["count"] == S
    assert 0.5 < want["test_acc_seg"] < 0.95                       # (the epoch counts something: see above)
    assert abs(got["test_acc_seg"] - want["test_acc_seg"]) <= 1e-12
    assert abs(got["test_iou"] - want["test_iou"]) <= 1e-12
    assert abs(got["test_loss_seg"] - want["test_loss_seg"]) <= LOSS_REL * abs(want["test_loss_seg"])
