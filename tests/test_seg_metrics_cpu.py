"""Segmentation metrics without a GPU: the numpy restatement (tests/seg_metrics_ref.py) against the fixtures of the live reference
(tests/golden/seg_metrics, tools/make_seg_metrics_golden.py) and against the reference itself where it is mounted; the arg-max rule
against torch.max on CPU tensors; the C entry's argument checks; what the wrapper refuses before a device is needed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import seg_metrics_ref as R

CASES = ("part_sizes_2_3_4_6", "absent_part_and_stray_predictions", "ties_quantised", "one_cloud_all_wrong")


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference_fixtures(case):
    g = golden("seg_metrics/" + case)
    score, seg, label = g["score"], g["seg"], g["label"]
    B, C, N = score.shape
    assert C == 50 and score.dtype == np.float32 and seg.dtype == label.dtype == np.int64
    r = R.seg_metrics(score, seg, label)
    loss, acc, iou, _ = R.batch_report(score, seg, label)
    assert np.array_equal(_bits(r["iou"]), _bits(g["iou_per_cloud"]))
    assert _bits(iou) == _bits(g["iou_batch"])
    assert g["accuracy"].dtype == np.float32 and np.float32(acc) == g["accuracy"]
    assert abs(loss - float(g["loss"])) <= 1e-6 * abs(float(g["loss"])), (loss, float(g["loss"]))
    assert (r["bad"] == 0).all()
    # the counts are consistent with each other
    assert (r["pred_cnt"].sum(1) == N).all() and (r["gt_cnt"].sum(1) == N).all() and (r["inter"].sum(1) == r["correct"]).all()


def test_fixture_families_pin_what_they_are_named_for():
    off = R.SHAPENET_PART_OFFSETS
    g = golden("seg_metrics/part_sizes_2_3_4_6")
    assert [off[c + 1] - off[c] for c in g["label"]] == [2, 3, 4, 6]
    assert ((g["iou_per_cloud"] > 0) & (g["iou_per_cloud"] < 1)).all()
    g = golden("seg_metrics/absent_part_and_stray_predictions")
    r = R.seg_metrics(g["score"], g["seg"], g["label"])
    last = off[g["label"][0] + 1] - 1
    assert r["pred_cnt"][0, last] == 0 and r["gt_cnt"][0, last] == 0            # union 0: that part gives 1.0
    lo, hi = off[g["label"][1]], off[g["label"][1] + 1]
    outside = r["pred_cnt"][1].sum() - r["pred_cnt"][1, lo:hi].sum()
    assert outside > g["score"].shape[2] // 5                                    # many predictions outside the category
    g = golden("seg_metrics/ties_quantised")
    s = g["score"]
    assert ((s == s.max(1, keepdims=True)).sum(1) > 1).mean() > 0.05             # equal maxima are common
    g = golden("seg_metrics/one_cloud_all_wrong")
    r = R.seg_metrics(g["score"], g["seg"], g["label"])
    assert r["correct"][0] == 0 and g["iou_per_cloud"][0] == 0.0 and r["correct"][1] > 0


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="reference checkout not mounted")
def test_fixtures_regenerate_and_restatement_equals_the_live_reference():
    """tools/make_seg_metrics_golden.py --check in its own process (the reference's package names are the product's): the fixtures
    regenerate bit for bit, and on fresh seeded inputs of odd sizes the restatement equals the reference's own functions."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_seg_metrics_golden.py"), "--check"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "fixtures regenerate bit-identically" in out and "restatement == live reference" in out


def test_argmax_rule_is_torch_max_on_cpu():
    for seed in range(4):
        s = R.argmax_rule_inputs(np.random.RandomState(seed))
        want = torch.max(torch.from_numpy(s), dim=1)[1].numpy()
        assert np.array_equal(R.argmax_rule(s), want), seed
    s = R.argmax_rule_inputs(np.random.RandomState(0))
    assert np.isnan(s).any() and np.isinf(s).any() and (np.signbit(s) & (s == 0)).any()
    for case in CASES:
        s = golden("seg_metrics/" + case)["score"]
        assert np.array_equal(R.argmax_rule(s), torch.max(torch.from_numpy(s), dim=1)[1].numpy())


def test_restatement_flags_bad_inputs():
    score, seg, label = R.make_inputs(np.random.RandomState(5), [0, 1, 2, 3], 40, bump=3.5)
    clean = R.seg_metrics(score, seg, label)
    seg2, label2 = seg.copy(), label.copy()
    seg2[0, 3], seg2[1, 7], label2[2] = -1, 50, 16
    r = R.seg_metrics(score, seg2, label2)
    assert r["bad"].tolist() == [1, 1, 1, 0]
    assert np.isnan(r["nll_sum"][:3]).all() and np.isnan(r["iou"][2]) and not np.isnan(r["iou"][:2]).any()
    assert r["nll_sum"][3] == clean["nll_sum"][3] and r["iou"][3] == clean["iou"][3]
    assert r["gt_cnt"][0].sum() == 39 and np.array_equal(r["pred_cnt"], clean["pred_cnt"])


def test_c_entry_rejects_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, C=2, N=4, n_cat=1, **null):
        names = ("score", "seg", "label", "part_offsets", "pred_out", "correct", "nll_sum", "inter", "pred_cnt", "gt_cnt", "iou", "bad", "ws")
        a = {k: (None if null.get(k) else p) for k in names}
        return lib.sonet_seg_metrics_f32(a["score"], a["seg"], a["label"], a["part_offsets"], n_cat, a["pred_out"], a["correct"],
                                         a["nll_sum"], a["inter"], a["pred_cnt"], a["gt_cnt"], a["iou"], a["bad"], a["ws"], B, C, N, None)

    for name in ("score", "seg", "label", "part_offsets", "correct", "nll_sum", "inter", "pred_cnt", "gt_cnt", "iou", "bad", "ws"):
        assert call(**{name: True}) == 1 and "NULL" in _lib.last_error(), name
    for kw in (dict(B=0), dict(C=0), dict(N=0), dict(B=-1), dict(N=-5)):
        assert call(**kw) == 1 and "non-positive" in _lib.last_error(), kw
    assert call(n_cat=0) == 1 and "n_cat=0" in _lib.last_error()
    assert call(C=257) == 2 and "C=257" in _lib.last_error()
    assert call(B=65536) == 2 and "B=65536" in _lib.last_error()
    assert lib.sonet_seg_metrics_ws_size(0, 50, 1024) == 0 and lib.sonet_seg_metrics_ws_size(2, 0, 8) == 0
    assert lib.sonet_seg_metrics_ws_size(2, 50, -1) == 0
    assert lib.sonet_seg_metrics_ws_size(3, 50, 257) == 3 * 2 * 8 and lib.sonet_seg_metrics_ws_size(1, 1, 256) == 8


def test_wrapper_refuses_before_a_device_is_needed():
    """CPU tensors are refused, and so is a bad part table -- host data, checked first.  (Wrong dtypes and non-contiguous scores on CUDA
    tensors: tests/test_gpu_seg_metrics.py.)"""
    from sonet_hip import metrics, ops
    from sonet_hip._lib import SonetHipError
    score, seg, label = torch.zeros(2, 50, 8), torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.seg_metrics(score, seg, label)
    with pytest.raises(SonetHipError, match="CUDA"):
        metrics.seg_iou(score, seg, label)
    with pytest.raises(SonetHipError, match="CUDA"):
        metrics.SegEvaluator().update(score, seg, label)
    for bad in ((0, 4, 4, 50), (0, 6, 4, 50), (1, 4, 50), (0, 25, 51), (0,), ()):
        with pytest.raises(SonetHipError, match="part_offsets"):
            ops.seg_metrics(score, seg, label, part_offsets=bad)
    with pytest.raises(SonetHipError, match="part_offsets"):
        ops.seg_metrics(torch.zeros(2, 49, 8), seg, label)                         # the default table ends at 50 > C
    with pytest.raises(SonetHipError, match="B x C x N"):
        ops.seg_metrics(torch.zeros(2, 50), seg, label)
    with pytest.raises(SonetHipError, match="before any update"):
        metrics.SegEvaluator().result()
    assert ops.SHAPENET_PART_OFFSETS == R.SHAPENET_PART_OFFSETS
