"""tools/bench_chamfer_loss.py -- the fused Chamfer loss (csrc/chamfer.hip: sonet_chamfer_loss_f32 + sonet_chamfer_grad_f32, behind
opt.chamfer_fused) against the present ChamferLoss path (two sonet_chamfer_nn_f32 launches, then aten gathers, reductions and their
backward), and ChamferEvaluator.update against the reference's test-loop structure in torch on device tensors.  No time is a gate: the
numbers go to docs/findings.md.

At B = 64: 1280 predicted against 5000 gt points (BASELINE configs[3]) and the two pyramid sizes, 256 and 1024 predicted points.  One
process; after a spin-up (1 s of untimed calls of both variants, GC frozen) the two variants ALTERNATE, --rounds rounds of --reps calls
each; a call is loss + backward, timed with one HIP event pair around the --reps calls of a round on the current stream (so the host's
launch time is inside it, as it is in a training step); the figure is the median over rounds of time / reps, with the range.
  evaluator   ChamferEvaluator.update (one fused forward without index or element outputs + a few small reductions into the epoch's
              float64 totals) against what autoencoder/train.py:89-94 does per batch with the present loss: the loss forward, then
              ``test_loss += loss.detach() * B`` on the device.

  python tools/bench_chamfer_loss.py [--reps 20] [--rounds 9]"""
import argparse
import os
import statistics
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))

import torch  # noqa: E402

from models import losses as LS  # noqa: E402
from sonet_hip import host  # noqa: E402
from sonet_hip.metrics import ChamferEvaluator  # noqa: E402

DEV = torch.device("cuda:0")


def spin_up(fns, seconds=1.0, chunk=8):
    host.freeze_gc()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for fn in fns:
            for _ in range(chunk):
                fn()
        torch.cuda.synchronize()


def alternate(fns, reps, rounds):
    """-> per variant (median, min, max) of ms per call over ``rounds`` rounds, the variants taking turns."""
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / reps)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    B, N = 64, 5000
    gen = torch.Generator().manual_seed(7)
    gt = (torch.rand(B, 3, N, generator=gen) * 2 - 1).to(DEV)
    fused = LS.ChamferLoss(Namespace(gpu_id=0, device=DEV, chamfer_fused=True))
    present = LS.ChamferLoss(Namespace(gpu_id=0, device=DEV))
    print("%-18s | %-30s | %-30s | %s" % ("B x M x N", "fused loss+backward ms", "present loss+backward ms", "present / fused"))
    for M in (1280, 256, 1024):
        pred = (torch.rand(B, 3, M, generator=gen) * 2 - 1).to(DEV).requires_grad_(True)

        def step(crit):
            pred.grad = None
            crit(pred, gt).backward()

        f, p = (lambda: step(fused)), (lambda: step(present))
        # same loss, same gradient (to the present path's own f32 rounding) at the size timed
        f()
        gf, lf = pred.grad.clone(), float((fused.forward_loss + fused.backward_loss).detach())
        p()
        gp, lp = pred.grad.clone(), float((present.forward_loss + present.backward_loss).detach())
        assert abs(lf - lp) <= 2e-6 * lp, (lf, lp)
        assert float((gf - gp).abs().max()) <= 1e-5 * float(gp.abs().max()), float((gf - gp).abs().max())
        spin_up([f, p])
        tf, tp = alternate([f, p], args.reps, args.rounds)
        print("%-18s | %8.4f (%7.4f..%7.4f) | %8.4f (%7.4f..%7.4f) | %.2fx" % ("%d x %d x %d" % (B, M, N), tf[0], tf[1], tf[2], tp[0],
                                                                                tp[1], tp[2], tp[0] / tf[0]), flush=True)
    # evaluation: per batch of the test loop
    pred = (torch.rand(B, 3, 1280, generator=gen) * 2 - 1).to(DEV)
    ev = ChamferEvaluator()
    test_loss = torch.zeros(1, device=DEV)

    def ref_loop():
        with torch.no_grad():
            loss = present(pred, gt)
            test_loss.add_(loss.detach() * B)

    def dev_loop():
        ev.update(pred, gt)

    spin_up([dev_loop, ref_loop])
    ev.reset()
    test_loss.zero_()
    te, tr = alternate([dev_loop, ref_loop], args.reps, args.rounds)
    n = args.reps * args.rounds * B
    got, want = ev.result(), float(test_loss) / n
    assert got["count"] == n and abs(got["test_loss"] - want) <= 1e-4 * want, (got, want)     # (the loop on the right keeps an f32 running sum)
    print("%-18s | %8.4f (%7.4f..%7.4f) | %8.4f (%7.4f..%7.4f) | %.2fx    (ChamferEvaluator.update | present loss forward + "
          "accumulate)" % ("%d x 1280 x %d" % (B, N), te[0], te[1], te[2], tr[0], tr[1], tr[2], tr[0] / te[0]), flush=True)


if __name__ == "__main__":
    main()
