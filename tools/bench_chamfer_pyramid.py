"""tools/bench_chamfer_pyramid.py -- the loss of a whole autoencoder step through ``models.losses.AutoencoderLoss``: the pyramid operator
(csrc/chamfer.hip: sonet_chamfer_pyramid_loss_f32 + sonet_chamfer_pyramid_grad_f32, behind opt.chamfer_pyramid) against the option-off
path of the same tree (``ChamferLoss`` per term: two sonet_chamfer_nn_f32 launches, aten gathers, reductions and their backward) and
against ``opt.chamfer_fused`` per term (sonet_chamfer_loss_f32 + sonet_chamfer_grad_f32).  No time is a gate: the numbers go to the
README and docs/findings.md.

At B = 64, N = 5000: the levels (1280, 256) of output_conv_pc_num = 1024 and (4352, 1024, 256) of 4096.  One process; after a spin-up
(1 s of untimed calls of every variant, GC frozen) the variants ALTERNATE, --rounds rounds of --reps calls each; a call is loss +
backward, timed with one HIP event pair around the --reps calls of a round on the current stream (so the host's launch time is inside
it, as it is in a training step); the figure is the median over rounds of time / reps, with the range.  The last rows time the
gradient launch alone at 1280 x 5000: ops.chamfer_pyramid_grad on one level against ops.chamfer_grad at the same indices.

  python tools/bench_chamfer_pyramid.py [--reps 20] [--rounds 9]"""
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
from sonet_hip import host, ops  # noqa: E402

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


def cell(t):
    return "%8.4f (%7.4f..%7.4f)" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    B, N = 64, 5000
    gen = torch.Generator().manual_seed(7)
    gt = (torch.rand(B, 3, N, generator=gen) * 2 - 1).to(DEV)
    print("%-28s | %-28s | %-28s | %-28s | %s" % ("B x levels x N (loss+backward)", "pyramid ms", "option off ms", "chamfer_fused per term ms",
                                                 "off / pyramid, fused / pyramid"))
    for conv, Ms in ((1024, (1280, 256)), (4096, (4352, 1024, 256))):
        clouds = [(torch.rand(B, 3, M, generator=gen) * 2 - 1).to(DEV).requires_grad_(True) for M in Ms]
        dec = Namespace(conv_pc4=clouds[-1], conv_pc5=clouds[1] if len(clouds) > 2 else None)
        crits = [LS.AutoencoderLoss(Namespace(gpu_id=0, device=DEV, output_conv_pc_num=conv, **kw))
                 for kw in (dict(chamfer_pyramid=True), dict(), dict(chamfer_fused=True))]

        def step(crit):
            for c in clouds:
                c.grad = None
            crit(clouds[0], dec, gt).backward()

        fns = [(lambda c=c: step(c)) for c in crits]
        # same loss, same gradients (to the option-off path's own f32 rounding) at the size timed
        seen = []
        for fn, crit in zip(fns, crits):
            fn()
            seen.append((float(crit.loss.detach()), [c.grad.clone() for c in clouds]))
        for loss, grads in seen[:1] + seen[2:]:
            assert abs(loss - seen[1][0]) <= 2e-6 * seen[1][0], (loss, seen[1][0])
            for g, r in zip(grads, seen[1][1]):
                assert float((g - r).abs().max()) <= 1e-5 * float(r.abs().max()), float((g - r).abs().max())
        spin_up(fns)
        tp, to, tf = alternate(fns, args.reps, args.rounds)
        print("%-28s | %s | %s | %s | %.2fx, %.2fx" % ("%d x %s x %d" % (B, Ms, N), cell(tp), cell(to), cell(tf), to[0] / tp[0], tf[0] / tp[0]),
              flush=True)
    # the gradient launch alone, 1280 x 5000, at the same indices and elements
    pred = (torch.rand(B, 3, 1280, generator=gen) * 2 - 1).to(DEV)
    t = ops.chamfer_pyramid_terms([pred], gt)
    gs = torch.tensor([[0.7, -1.3]], device=DEV)
    new = lambda: ops.chamfer_pyramid_grad([pred], gt, t, gs)                  # noqa: E731
    old = lambda: ops.chamfer_grad(pred, gt, t.levels[0], gs[0])               # noqa: E731
    assert torch.equal(new()[0][0].view(torch.int32), old()[0].view(torch.int32))
    spin_up([new, old])
    tn, tg = alternate([new, old], args.reps, args.rounds)
    print("%-28s | %s | %s | %.2fx    (chamfer_pyramid_grad, one level | chamfer_grad)" % ("gradient launch 64 x 1280 x 5000", cell(tn), cell(tg),
                                                                                           tg[0] / tn[0]), flush=True)
    # the forward launch alone: one pyramid launch against one chamfer_loss launch per level
    for Ms in ((1280, 256), (4352, 1024, 256)):
        ps = [(torch.rand(B, 3, M, generator=gen) * 2 - 1).to(DEV) for M in Ms]
        new = lambda: ops.chamfer_pyramid_terms(ps, gt)                        # noqa: E731
        old = lambda: [ops.chamfer_terms(p, gt) for p in ps]                   # noqa: E731
        spin_up([new, old])
        tn, tg = alternate([new, old], args.reps, args.rounds)
        print("%-28s | %s | %s | %.2fx    (chamfer_pyramid_terms | chamfer_terms per level)" % ("forward 64 x %s x 5000" % (Ms,), cell(tn), cell(tg),
                                                                                                 tg[0] / tn[0]), flush=True)


if __name__ == "__main__":
    main()
