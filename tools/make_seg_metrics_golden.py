"""tools/make_seg_metrics_golden.py -- fixtures of the segmentation metrics (sonet_seg_metrics_f32) from the LIVE reference.

Run where the reference checkout is mounted, in its own process:   python tools/make_seg_metrics_golden.py [out_dir] [--check]
(default out_dir: tests/golden/seg_metrics).

For every case the reference's OWN models.losses.compute_iou_np_array, compute_iou and CrossEntropyLossSeg, and the accuracy
expression of part-seg/train.py:89-91, run on seeded CPU inputs (tests/seg_metrics_ref.py: make_inputs -- labels inside the cloud's
category, scores a bump on the true part plus noise).  The three arguments compute_iou never reads without its debug flag
(visualizer, opt, input_pc) are None.  Written per case (data only):
  score [B][50][N] f32, seg [B][N] i64, label [B] i64                         the inputs;
  iou_per_cloud [B] f64, iou_batch f64, loss f32, accuracy f32                the reference's outputs.

The reference's accuracy is a float32 mean: it is the exact ratio only when B * N is a power of two.  Every case has such a size, so
that an epoch accumulated from these values is the exact one (tests/test_gpu_seg_metrics.py holds SegEvaluator to 1e-12 against it);
odd sizes, sizes around the workgroup's 256 points and other class counts are the business of the edge-shape tests against the
restatement, which these fixtures pin.
--check regenerates into a temporary directory and compares with out_dir array by array, then holds the restatement of
tests/seg_metrics_ref.py to the live reference on fresh seeded inputs of odd sizes (FRESH).
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seg_metrics_ref as R  # noqa: E402

from oracle import ref_harness  # noqa: E402

# name: seed, categories of the clouds, N, keyword arguments of seg_metrics_ref.make_inputs
# (categories 1, 5, 0, 10 have 2, 3, 4 and 6 parts)
CASES = {
    "part_sizes_2_3_4_6": (11, [1, 5, 0, 10], 256, dict()),
    "absent_part_and_stray_predictions": (12, [3, 12], 512, dict(absent_part=(0,), stray=(1,))),
    "ties_quantised": (13, [8, 2, 14, 10], 256, dict(quantum=0.25, bump=3.0)),
    "one_cloud_all_wrong": (14, [7, 15], 256, dict(all_wrong=(0,))),
}
BUMP = 3.5


def make_case(ref, name, seed, labels, N, kw):
    import torch
    g = np.random.RandomState(seed)
    kw = dict(dict(bump=BUMP), **kw)
    score, seg, label = R.make_inputs(g, labels, N, **kw)
    ts, tg, tl = torch.from_numpy(score), torch.from_numpy(seg), torch.from_numpy(label)
    L = ref.losses
    iou_per_cloud = np.asarray(L.compute_iou_np_array(ts, tg, tl, None, None, None), dtype=np.float64)
    iou_batch = np.float64(L.compute_iou(ts, tg, tl, None, None, None))
    loss = L.CrossEntropyLossSeg()(ts, tg)
    _, predicted_seg = torch.max(ts, dim=1, keepdim=False)                           # part-seg/train.py:89-91
    correct_mask = torch.eq(predicted_seg, tg).float()
    accuracy = torch.mean(correct_mask)
    assert loss.dtype == torch.float32 and accuracy.dtype == torch.float32
    # the fixtures must pin something: IoUs neither all 0 nor all 1, ordinary clouds 60-95 % right
    special = set(kw.get("all_wrong", ())) | set(kw.get("stray", ()))
    per_cloud = correct_mask.mean(dim=1).numpy()
    for b in range(len(labels)):
        if b in kw.get("all_wrong", ()):
            assert per_cloud[b] == 0.0, (name, b, per_cloud[b])
        elif b not in special:
            assert 0.6 <= per_cloud[b] <= 0.95, (name, b, per_cloud[b])
            assert 0.0 < iou_per_cloud[b] < 1.0
    n = len(labels) * N
    assert n & (n - 1) == 0, "B * N must be a power of two (see the module docstring)"
    return dict(score=score, seg=seg, label=label, iou_per_cloud=iou_per_cloud, iou_batch=iou_batch,
                loss=np.float32(loss.item()), accuracy=np.float32(accuracy.item()))


def reference_report(ref, score, seg, label):
    """(per-cloud IoU f64, batch IoU f64, loss f32, accuracy f32) from the reference's own code."""
    import torch
    ts, tg, tl = torch.from_numpy(score), torch.from_numpy(seg), torch.from_numpy(label)
    L = ref.losses
    _, predicted_seg = torch.max(ts, dim=1, keepdim=False)
    return (np.asarray(L.compute_iou_np_array(ts, tg, tl, None, None, None), dtype=np.float64),
            np.float64(L.compute_iou(ts, tg, tl, None, None, None)), np.float32(L.CrossEntropyLossSeg()(ts, tg).item()),
            np.float32(torch.mean(torch.eq(predicted_seg, tg).float()).item()), predicted_seg.numpy())


FRESH = [   # seed, categories, N, make_inputs keywords
    (101, [0, 1, 5, 10, 15], 257, dict()),
    (102, [4, 9, 13], 100, dict(quantum=0.25, bump=3.0, absent_part=(1,))),
    (103, list(range(16)), 33, dict(stray=(2, 7), all_wrong=(11,))),
    (104, [6], 1, dict()),
]


def check_restatement(ref):
    for seed, labels, N, kw in FRESH:
        score, seg, label = R.make_inputs(np.random.RandomState(seed), labels, N, **dict(dict(bump=BUMP), **kw))
        iou_pc, iou_b, loss, acc, pred = reference_report(ref, score, seg, label)
        r = R.seg_metrics(score, seg, label)
        mloss, macc, miou, _ = R.batch_report(score, seg, label)
        assert np.array_equal(r["pred"], pred), seed
        assert np.array_equal(r["iou"].view(np.int64), iou_pc.view(np.int64)), seed
        assert np.float64(miou).view(np.int64) == iou_b.view(np.int64), seed
        assert np.float32(macc) == acc, (seed, macc, acc)
        assert abs(mloss - float(loss)) <= 1e-6 * abs(float(loss)), (seed, mloss, loss)
    print("restatement == live reference on %d fresh inputs" % len(FRESH))


def generate(out_dir):
    ref = ref_harness.import_reference()
    assert ref.losses.__file__.startswith(ref_harness.REF_ROOT)
    os.makedirs(out_dir, exist_ok=True)
    for name, (seed, labels, N, kw) in CASES.items():
        d = make_case(ref, name, seed, labels, N, kw)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **d)
        print("%-40s %7.1f KB  accuracy %.4f  iou %.4f  loss %.4f" % (name + ".npz", os.path.getsize(path) / 1024, d["accuracy"],
                                                                      d["iou_batch"], d["loss"]))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "seg_metrics")
    if "--check" not in sys.argv:
        generate(out_dir)
        return
    with tempfile.TemporaryDirectory() as tmp:
        generate(tmp)
        for name in CASES:
            a, b = np.load(os.path.join(tmp, name + ".npz")), np.load(os.path.join(out_dir, name + ".npz"))
            assert sorted(a.files) == sorted(b.files), name
            for k in a.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: %s differs" % (name, k)
    print("fixtures regenerate bit-identically")
    check_restatement(ref_harness.import_reference())


if __name__ == "__main__":
    main()
