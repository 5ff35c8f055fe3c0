"""tools/bench_retrieval.py -- the retrieval lists on the device (csrc/retrieval.hip, ops.retrieval_lists) against the reference's loop
structure in torch on the same device tensors.  No time is a gate: the numbers go to docs/findings.md, "Retrieval lists".

Shape: N = 10 265 shapes (the SHREC16 test split) x 55 class scores, then x 1024 (the width of ``encoder.feature``); a skewed class
histogram over 55 classes whose largest class holds about 20 % of the shapes; random normal features, labels given; top = 1000.
In one process, after a spin-up (1 s of untimed calls):
  device   ops.retrieval_lists: one HIP event pair per call on the current stream, median of --reps calls; its lists are checked
           against the numpy restatement on a sample of queries before anything is timed.
  loop     shrec16/test.py:69-86 restated on the same device tensors -- per shape torch.eq, torch.nonzero, the gathered rows,
           torch.norm, torch.sort, the gather of the ids and the two device-to-host copies; no file is written.  Host clock around
           the loop, the device idle before it and synchronised after it, --loop-reps runs.
  --sweep  with the variants library loaded (SONET_HIP_LIB=so-net_amd/lib/libsonet_hip_variants.so): the device time for every LDS
           chunk size 2048 .. 8192 (SONET_RETRIEVAL_CHUNK) and 256 / 512 / 1024 threads per query (SONET_RETRIEVAL_THREADS), alternating,
           to choose the constants of the product library.

  python tools/bench_retrieval.py [--reps 30] [--loop-reps 2] [--sweep]"""
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

import retrieval_ref as R  # noqa: E402
from sonet_hip import _lib, host, ops  # noqa: E402

DEV = torch.device("cuda:0")
N_SHAPES, N_CLASSES, TOP = 10265, 55, 1000


def skewed_labels(g, N, C):
    """Class shares ~ 1 / (rank + 4): the largest of 55 classes holds about 20 %."""
    w = 1.0 / (np.arange(C) + 4.0)
    w[0] = 0.2 * w[1:].sum() / 0.8
    return R.class_labels(g, N, w / w.sum())


def spin_up(fn, seconds=1.0, chunk=4):
    host.freeze_gc()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(chunk):
            fn()
        torch.cuda.synchronize()


def event_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def torch_loop(feature_map, predicted_labels, model_name_ids, top):
    """The reference's neighbour stage without its file writing: per shape the same tensor operations and host copies."""
    rows = 0
    for i in range(feature_map.shape[0]):
        mask = torch.eq(predicted_labels, predicted_labels[i])
        same = torch.nonzero(mask).squeeze(1)
        distance = torch.norm(feature_map[i].unsqueeze(0) - feature_map[same], p=2, dim=1)
        srt, indices = torch.sort(distance)
        nn_id = model_name_ids[same][indices].cpu().numpy()
        nn_dist = srt.cpu().numpy()
        rows += min(len(nn_id), top) + 0 * len(nn_dist)
    torch.cuda.synchronize()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    lib = _lib.load()
    print("library %s, chunk %d keys" % (os.path.basename(_lib.LIB_PATH), lib.sonet_retrieval_chunk_keys()), flush=True)
    for D in (55, 1024):
        g = np.random.RandomState(D)
        labels = skewed_labels(g, N_SHAPES, N_CLASSES)
        feat = (g.normal(size=(N_SHAPES, D)) * 3).astype(np.float32)
        ids = g.choice(100000, N_SHAPES, replace=False).astype(np.int64)
        sizes = np.bincount(labels, minlength=N_CLASSES)
        df, dl, di = (torch.from_numpy(a).to(DEV) for a in (feat, labels, ids))
        call = lambda: ops.retrieval_lists(df, dl, di, None, TOP, N_CLASSES)          # noqa: E731
        r = call()
        sample = g.choice(N_SHAPES, 12, replace=False)
        want = R.retrieval_lists(feat, labels, ids, sample, TOP, N_CLASSES)
        assert np.array_equal(r.nn_id.cpu().numpy()[sample], want["nn_id"]), "lists differ from the restatement"
        assert np.array_equal(r.nn_dist.cpu().numpy()[sample].view(np.uint32), want["nn_dist"].view(np.uint32))
        pairs = float((sizes.astype(np.float64) ** 2).sum())
        print("N %d x D %d, %d classes, largest %d (%.1f %%), %.3g query-member pairs, %.2f GFLOP of distances"
              % (N_SHAPES, D, N_CLASSES, sizes.max(), 100 * sizes.max() / N_SHAPES, pairs, 3 * pairs * D / 1e9), flush=True)
        if args.sweep:
            for rnd in range(2):                                               # alternating: two rounds over the settings
                for threads in (256, 512, 1024):
                    for ck in (2048, 4096, 8192):
                        os.environ["SONET_RETRIEVAL_CHUNK"], os.environ["SONET_RETRIEVAL_THREADS"] = str(ck), str(threads)
                        if lib.sonet_retrieval_chunk_keys() != ck:
                            raise SystemExit("--sweep needs the variants library (SONET_HIP_LIB)")
                        x = call()
                        assert torch.equal(x.nn_id, r.nn_id) and torch.equal(x.nn_dist.view(torch.int32), r.nn_dist.view(torch.int32))
                        spin_up(call, 0.2)
                        t = event_ms(call, args.reps)
                        print("  %4d threads, chunk %5d keys (%3d KiB of LDS): %8.3f ms (%.3f..%.3f)"
                              % (threads, ck, (ck * 8 + D * 4) // 1024, t[0], t[1], t[2]), flush=True)
            os.environ.pop("SONET_RETRIEVAL_THREADS")
            os.environ.pop("SONET_RETRIEVAL_CHUNK")
            continue
        spin_up(call)
        t = event_ms(call, args.reps)
        loops = []
        for _ in range(args.loop_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = torch_loop(df, dl, di, TOP)
            loops.append((time.perf_counter() - t0) * 1e3)
        assert rows == int(r.count.sum().cpu())
        lp = statistics.median(loops)
        print("  ops.retrieval_lists %8.3f ms (%.3f..%.3f) | torch loop %9.1f ms (%s) | %.0fx | %d list rows"
              % (t[0], t[1], t[2], lp, ", ".join("%.1f" % v for v in loops), lp / t[0], rows), flush=True)


if __name__ == "__main__":
    main()
