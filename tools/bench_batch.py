"""tools/bench_batch.py -- the batch assembler (csrc/batch.hip, sonet_hip.batch) against the host loader it replaces.

Three parts, each printed as it finishes (--json writes them all):
  launch   ops.assemble_batch (the assembly launch + the node kNN launch) for B in {64, 256}, N = 5000 of n_s = 10 000, M = 64,
           K = 9, modelnet recipe with every flag; and the shapenet recipe at N = 2048 from ragged clouds of 1500..3000 points.
           The kNN launch alone (ops.knn_self on the same nodes) and the assembly alone (K = 1: no kNN launch) are timed too.
           Spin-up calls, GC frozen, one HIP event pair per call on the current stream, median of --reps (>= 20) calls.
  host     the numpy restatement of the reference's __getitem__ (choice, two rotations, jitter, scale, shift, astype; the faiss
           self-kNN as an argsort of the 64 x 64 distances) for 64 clouds + collate (torch.stack) + the host-to-device copy,
           single process, data already in memory (no disk I/O): what each DataLoader worker does per batch.
  loop     --loop-steps (50) training steps (Encoder + Classifier, cross entropy, backward, FusedAdam; no gradient all-reduce) at
           B = 64, N = 5000, in the bf16 and the f32-class arithmetic, fed once by BatchAssembler.epoch over a device-resident split
           and once by one fixed batch.  Median of --windows windows, HIP events around each window.

  python tools/bench_batch.py [--reps 20] [--quick] [--no-loop] [--json out.json]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sonet_hip import ops  # noqa: E402
from sonet_hip.batch import BatchAssembler, DeviceClouds  # noqa: E402

DEV = torch.device("cuda:0")


def median_ms(fn, reps, spin=5):
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


def synthetic(S, sizes, M=64, seed=0):
    g = np.random.RandomState(seed)
    pts = [g.normal(size=(int(n), 3)).astype(np.float32) for n in sizes]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    return DeviceClouds(pts, nrm, g.randint(0, 40, S), nodes=g.normal(size=(S, M, 3)).astype(np.float32), device=DEV,
                        seg=[g.randint(0, 50, int(n)) for n in sizes])


def opt_of(N, som_k=9, flags=True, B=64):
    return Namespace(gpu_id=0, device=DEV, batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                     normalization="batch", dropout=0.7, node_num=64, k=3, som_k=som_k, som_k_type="avg", bn_momentum=0.1,
                     bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40, rot_horizontal=flags, rot_perturbation=flags,
                     translation_perturbation=flags)


def part_launch(reps, quick):
    rows = []
    S = 512
    full = synthetic(S, [10000] * S, seed=1)
    g = np.random.RandomState(2)
    shp = synthetic(S, g.randint(1500, 3001, S), seed=3)
    cases = [("modelnet", full, 64, 5000), ("modelnet", full, 256, 5000), ("shapenet", shp, 64, 2048), ("shapenet", shp, 256, 2048)]
    if quick:
        cases = cases[:1]
    print("%-9s %4s %5s | %9s %13s | %9s | %9s | %s" % ("recipe", "B", "N", "total ms", "min..max", "knn ms", "K=1 ms", "clouds/s"))
    for recipe, c, B, N in cases:
        A = BatchAssembler(c, opt_of(N), "train", recipe, seed=5)
        A1 = BatchAssembler(c, opt_of(N, som_k=1), "train", recipe, seed=5)
        idx = torch.from_numpy(np.random.RandomState(B).permutation(S)[:B]).to(DEV)
        st = [0]

        def run(a=A):
            st[0] += 1
            a._run(idx, st[0], False)

        node = A.batch(idx, 0)[-2]
        t, lo, hi = median_ms(run, reps)
        tk = median_ms(lambda: ops.knn_self(node, 9), reps)[0]
        t1 = median_ms(lambda: run(A1), reps)[0]
        # bytes: source points read (6 f32 of every chosen point; the selection passes read no point data), pc / sn written,
        # chosen written, nodes read + written
        nbytes = B * (N * (24 + 24 + 8) + 64 * 3 * 8)
        rows.append(dict(recipe=recipe, B=B, N=N, total_ms=t, min_ms=lo, max_ms=hi, knn_ms=tk, assemble_k1_ms=t1,
                         clouds_per_s=B / (t * 1e-3), bytes=nbytes, gbps=nbytes / (t1 * 1e-3) / 1e9))
        print("%-9s %4d %5d | %9.4f %6.4f..%-6.4f | %9.4f | %9.4f | %.0f  (%.1f MB, %.0f GB/s at K=1)"
              % (recipe, B, N, t, lo, hi, tk, t1, B / (t * 1e-3), nbytes / 1e6, nbytes / (t1 * 1e-3) / 1e9), flush=True)
    return rows


def host_item(data, som, N, rng):
    """The reference's __getitem__ (modelnet, all flags) restated in numpy, argsort for faiss."""
    d = data[rng.choice(data.shape[0], N, replace=False), :]
    pc, sn, node = d[:, 0:3], d[:, 3:6], som
    a = rng.uniform() * 2 * np.pi
    c, s = np.cos(a), np.sin(a)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    pc, sn, node = np.dot(pc, R), np.dot(sn, R), np.dot(node, R)
    ang = np.clip(0.06 * rng.randn(3), -0.18, 0.18)
    Rx = np.array([[1, 0, 0], [0, np.cos(ang[0]), -np.sin(ang[0])], [0, np.sin(ang[0]), np.cos(ang[0])]])
    Ry = np.array([[np.cos(ang[1]), 0, np.sin(ang[1])], [0, 1, 0], [-np.sin(ang[1]), 0, np.cos(ang[1])]])
    Rz = np.array([[np.cos(ang[2]), -np.sin(ang[2]), 0], [np.sin(ang[2]), np.cos(ang[2]), 0], [0, 0, 1]])
    R = np.dot(Rz, np.dot(Ry, Rx))
    pc, sn, node = np.dot(pc, R), np.dot(sn, R), np.dot(node, R)
    pc = np.clip(0.01 * rng.randn(*pc.shape), -0.05, 0.05) + pc
    sn = np.clip(0.01 * rng.randn(*sn.shape), -0.05, 0.05) + sn
    node = np.clip(0.04 * rng.randn(*node.shape), -0.1, 0.1) + node
    sc = rng.uniform(0.8, 1.2)
    pc, node, sn = pc * sc, node * sc, sn * sc
    shift = rng.uniform(-0.1, 0.1, (1, 3))
    pc += shift
    node += shift
    node32 = np.ascontiguousarray(node, dtype=np.float32)
    dist = ((node32[:, None, :] - node32[None, :, :]) ** 2).sum(-1)
    knn = np.argsort(dist, axis=1, kind="stable")[:, :9]
    return (torch.from_numpy(pc.T.astype(np.float32)), torch.from_numpy(sn.T.astype(np.float32)), 0,
            torch.from_numpy(node.T.astype(np.float32)), torch.from_numpy(knn.astype(np.int64)))


def part_host(reps):
    rng = np.random.RandomState(0)
    data = [rng.normal(size=(10000, 6)).astype(np.float32) for _ in range(64)]
    som = [rng.normal(size=(64, 3)).astype(np.float32) for _ in range(64)]
    torch.set_num_threads(1)

    def batch():
        items = [host_item(data[i], som[i], 5000, rng) for i in range(64)]
        pc, sn, lab, node, knn = zip(*items)
        out = [torch.stack(pc), torch.stack(sn), torch.tensor(lab), torch.stack(node), torch.stack(knn)]
        out = [t.to(DEV) for t in out]
        torch.cuda.synchronize()
        return out

    batch()
    ts, items = [], []
    for _ in range(max(5, reps // 4)):
        t0 = time.perf_counter()
        batch()
        ts.append((time.perf_counter() - t0) * 1e3)
    t_item = []
    for _ in range(200):
        t0 = time.perf_counter()
        host_item(data[0], som[0], 5000, rng)
        t_item.append((time.perf_counter() - t0) * 1e3)
    r = dict(batch_ms=statistics.median(ts), batch_min_ms=min(ts), item_ms=statistics.median(t_item), threads=1,
             host_cpus_visible=len(os.sched_getaffinity(0)))
    print("host loader (numpy restatement, 1 thread): %.1f ms per 64-cloud batch (min %.1f), %.3f ms per item"
          % (r["batch_ms"], r["batch_min_ms"], r["item_ms"]), flush=True)
    return r


def part_loop(steps, windows):
    from models import networks as NW
    from sonet_hip import synth
    from sonet_hip.optim import FusedAdam
    B, N, S = 64, 5000, 1024
    clouds = synthetic(S, [10000] * S, seed=7)
    res = {}
    for precision in ("bf16", ops.POINTMLP_PRECISION):
        with ops.precision(precision):
            opt = opt_of(N, B=B)
            enc, cls = NW.Encoder(opt), NW.Classifier(opt)
            enc.want_first_pn_out = False
            synth.fill_state_dict_(enc.state_dict(), 0)
            synth.fill_state_dict_(cls.state_dict(), 1)
            enc.to(DEV).train()
            cls.to(DEV).train()
            oe, oc = FusedAdam(enc.parameters(), lr=1e-3), FusedAdam(cls.parameters(), lr=1e-3)
            A = BatchAssembler(clouds, opt, "train", "modelnet", seed=3)
            fixed = A.batch(list(range(B)), 0)

            def step(batch):
                pc, sn, label, node, knn = batch
                feat = enc(pc, sn, node, knn, True, 0)
                score = cls(feat, 0)
                enc.zero_grad(set_to_none=True)
                cls.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(score, label)
                loss.backward()
                oe.step()
                oc.step()
                return loss

            def feed_fixed(n):
                for _ in range(n):
                    yield fixed

            ep = [0]

            def feed_epoch(n):
                got = 0
                while got < n:
                    for batch in A.epoch(ep[0], B):
                        if batch[0].shape[0] != B:
                            continue                       # (the short last batch of an epoch: keep the shape)
                        yield batch
                        got += 1
                        if got == n:
                            return
                    ep[0] += 1

            def window(feed):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                for batch in feed(steps):
                    loss = step(batch)
                b.record()
                b.synchronize()
                assert torch.isfinite(loss)
                return a.elapsed_time(b) / steps, (time.perf_counter() - t0) * 1e3 / steps

            for feed in (feed_fixed, feed_epoch):
                window(feed)                                  # warm-up window of each feed
            tf, te = [], []
            for _ in range(windows):
                tf.append(window(feed_fixed))
                te.append(window(feed_epoch))
            mf, me = statistics.median(t[0] for t in tf), statistics.median(t[0] for t in te)
            res[precision] = dict(fixed_ms=mf, epoch_ms=me, delta_ms=me - mf, fixed_all=[t[0] for t in tf], epoch_all=[t[0] for t in te],
                                  fixed_wall_ms=statistics.median(t[1] for t in tf), epoch_wall_ms=statistics.median(t[1] for t in te))
            print("loop %-4s: fixed batch %.3f ms/step, BatchAssembler.epoch %.3f ms/step, delta %+.3f ms  (windows %s | %s)"
                  % (precision, mf, me, me - mf, " ".join("%.3f" % t[0] for t in tf), " ".join("%.3f" % t[0] for t in te)), flush=True)
            del enc, cls, oe, oc, A, fixed
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the B = 64 modelnet launch only (the profiler run)")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--loop-steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    reps = max(20, args.reps)
    gc.collect()
    gc.freeze()
    gc.disable()
    out = dict(launch=part_launch(reps, args.quick))
    if not args.quick and not args.no_host:
        out["host"] = part_host(reps)
    if not args.quick and not args.no_loop:
        out["loop"] = part_loop(args.loop_steps, args.windows)
    gc.enable()
    if "host" in out and "loop" in out:
        for p, r in out["loop"].items():
            print("workers needed to feed the %s step (%.2f ms) at the measured single-process rate: %.1f (worker scaling not measured)"
                  % (p, r["fixed_ms"], out["host"]["batch_ms"] / r["fixed_ms"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
