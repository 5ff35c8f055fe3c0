"""tools/bench_ce_loss.py -- the cross-entropy operator (csrc/ce_loss.hip, ops.ce_loss, models.losses, sonet_hip.metrics) against the
paths it replaces, in ONE process on one MI355X.

    python tools/bench_ce_loss.py [--rounds 9] [--iters 20] [--spin-up 1.0] [--clouds 2468] [--points 5000] [--epoch-rounds 3]

After the clock spin-up bench.py uses (untimed calls for --spin-up seconds: an idle MI355X sits at its lowest clock) the variants of
each section are timed INTERLEAVED, --rounds rounds of --iters calls each, and the median over the rounds is reported:
  (a) segmenter loss, B 64 x C 50 x N 1024: loss + backward, CrossEntropyLossSeg(fused=True) against fused=False -- device time by HIP
      events around a group, host enqueue time by perf_counter around the same calls (before the synchronize);
  (b) classifier loss, B 64 x C 40: CrossEntropyLossCls(fused=True) against torch.nn.CrossEntropyLoss, the same two figures;
  (c) one test epoch, --clouds synthetic clouds of --points points at B 64: metrics.evaluate_classification against a loop of the
      reference's structure (modelnet/train.py:70-90: the criterion, an arg-max, a mean and a .cpu() per batch) on the same models -- wall time
      per epoch including the final synchronize;
  (d) what float64 costs: the forward launch of (a)'s shape against the same kernel with float32 expf / logf (sonet_ce_loss_f32_sp, an
      entry of the variants library only), both from the variants library.
Prints a table and one JSON line (last line)."""
import argparse
import ctypes
import json
import os
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "so-net_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fns, rounds, iters):
    """fns: name -> callable.  Interleaved rounds of `iters` calls per variant -> name -> ([device ms per call], [host enqueue ms per call])."""
    out = {k: ([], []) for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            h1 = time.perf_counter()
            e1.synchronize()
            out[k][0].append(e0.elapsed_time(e1) / iters)
            out[k][1].append((h1 - h0) * 1e3 / iters)
    return out


def spin_up(fns, seconds):
    t0 = time.time()
    while time.time() - t0 < seconds:
        for fn in fns:
            fn()
        torch.cuda.synchronize()


def report(tag, t, res):
    res[tag] = {k: dict(device_ms=round(median(v[0]), 5), host_ms=round(median(v[1]), 5), device_ms_rounds=[round(x, 5) for x in v[0]])
                for k, v in t.items()}
    for k, v in res[tag].items():
        print("    %-28s device %8.4f ms   host enqueue %8.4f ms   (device min %.4f max %.4f)" % (
            k, v["device_ms"], v["host_ms"], min(v["device_ms_rounds"]), max(v["device_ms_rounds"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--spin-up", type=float, default=1.0)
    ap.add_argument("--clouds", type=int, default=2468)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--epoch-rounds", type=int, default=3)
    args = ap.parse_args()
    from models import losses as LS, networks as NW
    from sonet_hip import _lib, metrics, ops, synth
    from sonet_hip.batch import BatchAssembler, DeviceClouds
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    res = {"config": dict(rounds=args.rounds, iters=args.iters, clouds=args.clouds, points=args.points)}

    def loss_step(crit, score, target):
        score.grad = None
        crit(score, target).backward()

    # ---- (a) segmenter loss
    B, C, N = 64, 50, 1024
    score = (4.0 * torch.randn(B, C, N, generator=gen)).to(dev).requires_grad_(True)
    target = torch.randint(0, C, (B, N), generator=gen).to(dev)
    on, off = LS.CrossEntropyLossSeg(fused=True), LS.CrossEntropyLossSeg(fused=False)
    fns = {"fused=False": lambda: loss_step(off, score, target), "fused=True": lambda: loss_step(on, score, target)}
    spin_up(fns.values(), args.spin_up)
    print("(a) segmenter loss + backward, B %d x C %d x N %d (%.1f MB of scores); loss off %.7f on %.7f" % (
        B, C, N, score.numel() * 4 / 1e6, off(score, target).item(), on(score, target).item()))
    report("seg_loss", timed(fns, args.rounds, args.iters), res)

    # ---- (b) classifier loss
    Bc, Cc = 64, 40
    rows = (2.0 * torch.randn(Bc, Cc, generator=gen)).to(dev).requires_grad_(True)
    labels = torch.randint(0, Cc, (Bc,), generator=gen).to(dev)
    con, coff = LS.CrossEntropyLossCls(fused=True), torch.nn.CrossEntropyLoss()
    fns = {"nn.CrossEntropyLoss": lambda: loss_step(coff, rows, labels), "CrossEntropyLossCls(fused)": lambda: loss_step(con, rows, labels)}
    spin_up(fns.values(), 0.3)
    print("(b) classifier loss + backward, B %d x C %d; loss off %.7f on %.7f" % (Bc, Cc, coff(rows, labels).item(), con(rows, labels).item()))
    report("cls_loss", timed(fns, args.rounds, args.iters), res)

    # ---- (d) float64 against float32 arithmetic in the forward launch (variants library)
    if os.path.exists(_lib.VARIANTS_PATH):
        var = ctypes.CDLL(_lib.VARIANTS_PATH)
        for name in ("sonet_ce_loss_f32", "sonet_ce_loss_f32_sp"):
            getattr(var, name).argtypes = _lib.SIGNATURES["sonet_ce_loss_f32"]
            getattr(var, name).restype = ctypes.c_int
        s, lib = score.detach(), _lib.load()
        f64 = torch.empty(B + B * N + lib.sonet_ce_loss_ws_size(B, C, N) // 8, dtype=torch.float64, device=dev)
        ints = torch.empty(2 * B, dtype=torch.int32, device=dev)

        def forward(fn, keep_lse):
            _lib.check(fn(ops.ptr(s), ops.ptr(target), ops.ptr(f64[B:]) if keep_lse else None, ops.ptr(f64), None, ops.ptr(ints), ops.ptr(ints[B:]),
                          None, ops.ptr(f64[B + B * N:]), B, C, N, _lib.stream_ptr()), "ce_loss")

        fns = {"float64": lambda: forward(var.sonet_ce_loss_f32, False), "float32 expf/logf": lambda: forward(var.sonet_ce_loss_f32_sp, False),
               "float64 + lse": lambda: forward(var.sonet_ce_loss_f32, True), "float32 + lse": lambda: forward(var.sonet_ce_loss_f32_sp, True)}
        spin_up(fns.values(), 0.3)
        forward(var.sonet_ce_loss_f32, False)
        a = f64[:B].clone()
        forward(var.sonet_ce_loss_f32_sp, False)
        print("(d) forward launches alone, B %d x C %d x N %d (%.2f M exponentials): float32 sums differ from float64 by up to %.3g relative" % (
            B, C, N, B * C * N / 1e6, ((f64[:B] - a).abs() / a.abs()).max().item()))
        report("forward_f64_vs_f32", timed(fns, args.rounds, args.iters), res)
        gb = s.numel() * 4 / 1e9
        print("    %.1f MB of scores once: float64 %.0f GB/s, float32 %.0f GB/s" % (
            gb * 1e3, gb / res["forward_f64_vs_f32"]["float64"]["device_ms"] * 1e3, gb / res["forward_f64_vs_f32"]["float32 expf/logf"]["device_ms"] * 1e3))
    else:
        print("(d) skipped: the variants library is not built")

    # ---- (c) one test epoch
    S, n, M, BS, classes = args.clouds, args.points, 64, 64, 40
    g = np.random.RandomState(3)
    pts = [g.uniform(-1, 1, size=(n, 3)).astype(np.float32) for _ in range(S)]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = np.stack([p[g.choice(n, M, replace=False)] for p in pts]).astype(np.float32)
    opt = Namespace(gpu_id=0, device=dev, batch_size=BS, input_pc_num=n, surface_normal=True, feature_num=1024, activation="relu",
                    normalization="batch", dropout=0.7, node_num=M, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                    bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=classes)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), 7)
    synth.fill_state_dict_(cls.state_dict(), 8)
    enc.to(dev).eval()
    cls.to(dev).eval()
    clouds = DeviceClouds(pts, nrm, g.randint(0, classes, S).astype(np.int64), nodes=nodes, device=dev)
    A = BatchAssembler(clouds, opt, "test", "modelnet", seed=4)
    crit = torch.nn.CrossEntropyLoss()

    def reference_loop():
        """A loop of the reference's structure: per batch the criterion, an arg-max, the mean of the hits -- and that mean brought to
        the host, which is the loop's one sync per batch."""
        loss_sum, hit_share_sum, seen = torch.zeros((), device=dev), 0.0, 0
        with torch.no_grad():
            for pc, sn, label, node, knn in A.epoch(0, BS, shuffle=False):
                sc = cls(enc(pc, sn, node, knn, False, None))
                n = label.shape[0]
                loss_sum += n * crit(sc, label)
                hit_share_sum += n * (sc.argmax(dim=1) == label).float().mean().cpu()             # the per-batch sync
                seen += n
        return (loss_sum / seen).item(), float(hit_share_sum / seen)

    ev = metrics.ClsEvaluator(classes)
    device_loop = lambda: metrics.evaluate_classification(enc, cls, A, BS, ev)
    r0, r1 = reference_loop(), device_loop()
    print("(c) one test epoch, %d clouds x %d points at B %d (%d batches): reference loop loss %.6f acc %.6f; device loop loss %.6f acc %.6f" % (
        S, n, BS, -(-S // BS), r0[0], r0[1], r1["test_loss"], r1["test_accuracy"]))
    wall = {"reference loop (.cpu() per batch)": [], "evaluate_classification": []}
    for _ in range(args.epoch_rounds):
        for k, fn in (("reference loop (.cpu() per batch)", reference_loop), ("evaluate_classification", device_loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    res["test_epoch_ms"] = {k: round(median(v), 3) for k, v in wall.items()}
    res["test_epoch_ms_rounds"] = {k: [round(x, 3) for x in v] for k, v in wall.items()}
    for k, v in wall.items():
        print("    %-36s %9.2f ms per epoch   rounds %s" % (k, median(v), [round(x, 2) for x in v]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
