"""tools/bench_som_train.py -- BatchSOM.optimize as ONE som_train launch (csrc/som_train.hip) against the batch_update loop on the same
schedule (8 x 8 nodes, max_iteration 60 -> T = 80 iterations), for B in {64, 256, 1024} and N in {1024, 5000, 10000}.

Each side: spin-up calls, GC frozen, one HIP event pair per call on the current stream, median of --reps calls (>= 20).  The loop
side is node_init + 80 batch_update calls enqueued from Python (its time includes the host enqueue, which is what a caller pays).
Work model of the one launch: B * T * N * M * ~10 lane-ops (distance 8, compare/select 2); the VALU roof is 256 CUs x 64 lane-ops
per clock (128 when every operation is packed) at 2.4 GHz.

  python tools/bench_som_train.py [--reps 20] [--quick] [--shapes B:N,...] [--json out.json]"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))

import torch  # noqa: E402

from util import som  # noqa: E402

DEV = "cuda:0"
CUS, CLK = 256, 2.4e9


def median_ms(fn, reps, spin=3):
    for _ in range(spin):
        fn()
    torch.cuda.synchronize()
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="B = 256, N = 5000 only (the profiler run)")
    ap.add_argument("--shapes", default=None, help="B:N,B:N,... instead of the default grid")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    reps = max(20, args.reps)
    shapes = [(256, 5000)] if args.quick else [(B, N) for B in (64, 256, 1024) for N in (1024, 5000, 10000)]
    if args.shapes:
        shapes = [tuple(int(v) for v in sh.split(":")) for sh in args.shapes.split(",")]
    rows = []
    gc.collect()
    gc.freeze()
    gc.disable()
    print("%5s %6s %3s | %10s %10s %8s | %10s %10s | %7s | %9s %9s" % ("B", "N", "T", "launch ms", "min..max", "clouds/s", "loop ms",
                                                                    "clouds/s", "speedup", "roof64", "roof128"))
    for B, N in shapes:
        g = torch.Generator().manual_seed(B * 7 + N)
        x = (torch.rand(B, 3, N, generator=g) * 2 - 1).to(DEV)
        s = som.BatchSOM(8, 8, 3, 0, B)
        T = len(s.train_schedule()[0])
        s.train_tables(DEV)

        def one():
            s.optimize(x)

        def loop():
            s.node_init(B)
            for lr, sigma in zip(*s.train_schedule()):
                s.batch_update(x, lr, sigma)

        t1, lo1, hi1 = median_ms(one, reps)
        t2, lo2, hi2 = median_ms(loop, reps)
        work = float(B) * T * N * 64 * 10
        r64, r128 = work / (t1 * 1e-3) / (CUS * 64 * CLK), work / (t1 * 1e-3) / (CUS * 128 * CLK)
        rows.append(dict(B=B, N=N, T=T, launch_ms=t1, launch_min=lo1, launch_max=hi1, loop_ms=t2, loop_min=lo2, loop_max=hi2,
                         clouds_per_s_launch=B / (t1 * 1e-3), clouds_per_s_loop=B / (t2 * 1e-3), speedup=t2 / t1,
                         valu_roof64=r64, valu_roof128=r128))
        print("%5d %6d %3d | %10.3f %4.2f..%-5.2f %8.0f | %10.3f %10.0f | %6.1fx | %9.3f %9.3f"
              % (B, N, T, t1, lo1, hi1, B / (t1 * 1e-3), t2, B / (t2 * 1e-3), t2 / t1, r64, r128), flush=True)
        del s, x
        torch.cuda.empty_cache()
    gc.enable()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
