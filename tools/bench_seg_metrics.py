"""tools/bench_seg_metrics.py -- the segmentation metrics on the device (csrc/seg_metrics.hip, sonet_hip.metrics) against the host
step of the reference's test loop they replace.  No time is a gate: the numbers go to docs/findings.md.

At 64 x 50 x 1024 (BASELINE configs[2]) and 16 x 50 x 5000, in one process, after a spin-up (1 s of untimed calls, GC frozen: what
bench.py does before a timed region):
  device   ops.seg_metrics alone, and one SegEvaluator.update (the launches plus the few small torch reductions into the epoch's
           totals): one HIP event pair per call on the current stream, median of --reps calls.
  host     what part-seg/train.py:95 does per batch: the device-to-host copy of score, seg and label (score is the 13 MB one), then
           the IoU double loop over clouds and parts -- the numpy restatement of tests/seg_metrics_ref.py (arg-max, counts, IoU and
           the float64 loss; the reference's own loop makes four tensor ops and two .item() calls per part instead).  Wall clock
           around copy + metrics with the device idle before it, median of --host-reps.

  python tools/bench_seg_metrics.py [--reps 50] [--host-reps 7]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import seg_metrics_ref as R  # noqa: E402
from sonet_hip import host, ops  # noqa: E402
from sonet_hip.metrics import SegEvaluator  # noqa: E402

DEV = torch.device("cuda:0")


def spin_up(fn, seconds=1.0, chunk=16):
    host.freeze_gc()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(chunk):
            fn()
        torch.cuda.synchronize()


def median_event_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=7)
    args = ap.parse_args()
    torch.set_num_threads(1)
    print("%-16s | %21s | %21s | %10s %10s %10s | %s" % ("B x C x N", "seg_metrics ms (min..max)", "evaluator.update ms", "D2H ms",
                                                         "host ms", "host total", "host total / update"))
    for B, N in ((64, 1024), (16, 5000)):
        g = np.random.RandomState(B)
        labels = g.randint(0, 16, B).tolist()
        score, seg, label = R.make_inputs(g, labels, N, bump=3.5)
        ds, dg, dl = (torch.from_numpy(a).to(DEV) for a in (score, seg, label))
        ev = SegEvaluator()
        spin_up(lambda: ops.seg_metrics(ds, dg, dl))
        t_op = median_event_ms(lambda: ops.seg_metrics(ds, dg, dl), args.reps)
        spin_up(lambda: ev.update(ds, dg, dl), 0.3)
        t_up = median_event_ms(lambda: ev.update(ds, dg, dl), args.reps)
        res = ev.result()
        want = R.batch_report(score, seg, label)
        assert abs(res["test_iou"] - want[2]) <= 1e-12 and abs(res["test_acc_seg"] - want[1]) <= 1e-12, (res, want)
        copies, totals = [], []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs, hg, hl = ds.cpu(), dg.cpu(), dl.cpu()
            t1 = time.perf_counter()
            R.batch_report(hs.numpy(), hg.numpy(), hl.numpy())
            t2 = time.perf_counter()
            copies.append((t1 - t0) * 1e3)
            totals.append((t2 - t0) * 1e3)
        c, t = statistics.median(copies), statistics.median(totals)
        print("%-16s | %7.4f (%6.4f..%6.4f) | %7.4f (%6.4f..%6.4f) | %10.3f %10.3f %10.3f | %.0fx"
              % ("%d x 50 x %d" % (B, N), t_op[0], t_op[1], t_op[2], t_up[0], t_up[1], t_up[2], c, t - c, t, t / t_up[0]), flush=True)
        print("  %.1f MB of scores: %.0f GB/s through seg_metrics; epoch values of the timed batch: loss %.6f acc %.6f iou %.6f"
              % (score.nbytes / 1e6, score.nbytes / (t_op[0] * 1e-3) / 1e9, res["test_loss_seg"], res["test_acc_seg"], res["test_iou"]),
              flush=True)


if __name__ == "__main__":
    main()
