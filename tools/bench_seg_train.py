"""tools/bench_seg_train.py -- the part-segmentation TRAINING step with segmenter layer 1 dense (the default) against node-wise
(``opt.seg_nodewise_train``), in ONE process on one MI355X, at BASELINE configs[2]: B = 64 clouds, N = 1024 points, k = 3, h3.

    python tools/bench_seg_train.py [--batch 64] [--points 1024] [--rounds 7] [--iters 5] [--spin-up 1.0]

After the clock spin-up bench.py uses (untimed steps for --spin-up seconds: an idle MI355X sits at its lowest clock) the variants are
timed INTERLEAVED -- off, on, off, on, ... --rounds rounds of --iters calls each, every group bracketed by HIP events on the launch
stream -- and the median over the rounds is reported:
  (a) the step: segmentation_forward + CrossEntropyLossSeg + backward (no optimizer step), option off and on, two models with the same
      weights on the same batch; and the peak allocated memory of one step of each;
  (b) layer 1 per launch on both sides: every launch of one step whose name belongs to layer 1 (``ops.kernel_timing``: one event pair
      per launch, so the sum is an upper bound of the launches' share of the step, which overlaps two streams);
  (c) the backward's apply-and-sum launch (``ops.pointwise_bwd_apply_nodesum``) against the two launches it replaces
      (``ops.pointwise_bwd_apply`` + ``ops.node_gather_bwd``) on the same B x 1024 x kN tensors.
Prints a table and one JSON line (last line)."""
import argparse
import json
import os
import re
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "so-net_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

# launches of one step that belong to segmenter layer 1 (dense: the three gathers and their backward, the 3356-channel layer, its
# BatchNorm passes are shared names and counted by shape below; node-wise: the split's launches)
DENSE = r"node_gather(_bwd)?|pointmlp\w*_3356x1024_L\d+|pointmlp\w*_1024x3456_L\d+|wgradx3_1024x3356_L\d+"
SPLIT = (r"pointmlph3_1923x1024_L\d+|pointmlph3_nodeadd_stats_393x1024_L\d+|pointwise_bwd_apply_nodesum|pointmlpx3_1024x384_L\d+|"
         r"pointmlpx3_1024x1920_L\d+|wgradx3_1024x393_L\d+|wgradx3_1024x1923_L\d+")


def timed_pairs(fns, rounds, iters):
    """fns: name -> callable.  Interleaved rounds of `iters` calls per variant between two events -> name -> [ms per call per round]."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters)
    return out


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--spin-up", type=float, default=1.0)
    args = ap.parse_args()
    from models import networks as NW
    from models.losses import CrossEntropyLossSeg
    from sonet_hip import ops, synth
    dev = torch.device("cuda:0")
    B, N, k, M = args.batch, args.points, 3, 64
    assert ops.POINTMLP_PRECISION == "h3", "the node-wise training path is the h3 arithmetic's"

    def models(option):
        opt = Namespace(gpu_id=0, device=dev, batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                        normalization="batch", dropout=0.0, node_num=M, k=k, som_k=9, som_k_type="center", bn_momentum=0.1,
                        bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=50)
        if option:
            opt.seg_nodewise_train = True
        enc, seg = NW.Encoder(opt), NW.Segmenter(opt)
        synth.fill_state_dict_(enc.state_dict(), 11)
        synth.fill_state_dict_(seg.state_dict(), 12)
        return enc.to(dev).train(), seg.to(dev).train()

    inp = synth.make_inputs(B, N, M=M, som_k=9, seed=61, node_kind="som", device=dev)
    gen = torch.Generator().manual_seed(61)
    label = torch.randint(0, 16, (B,), generator=gen).to(dev)
    target = torch.randint(0, 50, (B, N), generator=gen).to(dev)
    crit = CrossEntropyLossSeg()
    pair = {"off": models(False), "on": models(True)}

    def step(which):
        enc, seg = pair[which]
        score = NW.segmentation_forward(enc, seg, inp["pc"], inp["sn"], label, inp["node"], inp["node_knn_I"], is_train=True, epoch=0)
        for m in (enc, seg):
            m.zero_grad(set_to_none=True)
        loss = crit(score, target)
        loss.backward()
        return loss

    # ---- spin-up, and what one step of each side is
    t0 = time.time()
    while time.time() - t0 < args.spin_up:
        for w in pair:
            step(w)
        torch.cuda.synchronize()
    res = {"config": dict(B=B, N=N, k=k, M=M, precision="h3", rounds=args.rounds, iters=args.iters)}
    losses = {w: float(step(w).detach()) for w in pair}
    print("configs[2] segmentation training step, B = %d, N = %d, k = %d, h3; loss off %.6f on %.6f" % (B, N, k, losses["off"], losses["on"]))
    launches = {}
    for w in pair:
        with ops.kernel_timing() as rec:
            step(w)
        torch.cuda.synchronize()
        launches[w] = rec.summary()
    assert "pointwise_bwd_apply_nodesum" in launches["on"] and "node_gather" not in launches["on"], sorted(launches["on"])
    assert "pointwise_bwd_apply_nodesum" not in launches["off"] and "node_gather" in launches["off"], sorted(launches["off"])

    # ---- (a) the step, interleaved; peak memory of one step
    t = timed_pairs({w: (lambda w=w: step(w)) for w in pair}, args.rounds, args.iters)
    res["step_ms"] = {w: median(v) for w, v in t.items()}
    res["step_ms_rounds"] = {w: [round(x, 3) for x in v] for w, v in t.items()}
    peak = {}
    for w in pair:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step(w)
        torch.cuda.synchronize()
        peak[w] = (torch.cuda.max_memory_allocated(dev), base)
    res["peak_allocated_MB"] = {w: round(p[0] / 2 ** 20, 1) for w, p in peak.items()}
    res["allocated_before_step_MB"] = {w: round(p[1] / 2 ** 20, 1) for w, p in peak.items()}
    print("(a) step, median of %d rounds x %d:  off %.3f ms   on %.3f ms   (on / off %.3f)" % (
        args.rounds, args.iters, res["step_ms"]["off"], res["step_ms"]["on"], res["step_ms"]["on"] / res["step_ms"]["off"]))
    print("    rounds off %s" % res["step_ms_rounds"]["off"])
    print("    rounds on  %s" % res["step_ms_rounds"]["on"])
    print("    peak allocated in one step: off %.1f MB   on %.1f MB" % (res["peak_allocated_MB"]["off"], res["peak_allocated_MB"]["on"]))

    # ---- (b) layer 1 per launch (kernel_timing of ONE step per side, after the interleaved runs)
    res["layer1_launches_ms"] = {}
    for w, rx in (("off", DENSE), ("on", SPLIT)):
        with ops.kernel_timing() as rec:
            step(w)
        torch.cuda.synchronize()
        rows = {n: v for n, v in rec.summary().items() if re.fullmatch(rx, n)}
        res["layer1_launches_ms"][w] = {n: round(v["total_ms"], 4) for n, v in rows.items()}
        print("(b) layer 1, option %s: %d launch names, %.3f ms in all (event pairs per launch)" % (w, len(rows), sum(v["total_ms"] for v in rows.values())))
        for n, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"]):
            print("      %-46s x%d  %.3f ms" % (n, v["count"], v["total_ms"]))

    # ---- (c) the apply-and-sum launch against the two launches it replaces, same tensors
    L, C = k * N, 1024
    g = torch.Generator().manual_seed(3)
    gy, raw = torch.randn(B, C, L, generator=g).to(dev), torch.randn(B, C, L, generator=g).to(dev)
    vec = lambda lo, hi: (torch.rand(C, generator=g) * (hi - lo) + lo).to(dev)
    sc, sh, a, b, c0 = vec(0.5, 1.5), vec(-0.5, 0.5), vec(0.5, 2.0), vec(-0.1, 0.1), vec(-0.01, 0.01)
    ids = pair["on"][0]._lazy["a"].min_idx_i32.contiguous()
    assert tuple(ids.shape) == (B, L)

    def two():
        g_raw = ops.pointwise_bwd_apply(gy, raw, sc, sh, True, a, b, c0)
        return g_raw, ops.node_gather_bwd(g_raw, ids, M)

    def fused():
        return ops.pointwise_bwd_apply_nodesum(gy, raw, sc, sh, True, a, b, c0, ids, M)
    (g1, z1), (g2, z2) = two(), fused()
    assert torch.equal(g1, g2) and torch.equal(z1, z2), "the fused launch does not give the bits of the two launches"
    t = timed_pairs({"apply+node_gather_bwd": two, "apply_nodesum": fused, "apply_only": lambda: ops.pointwise_bwd_apply(gy, raw, sc, sh, True, a, b, c0)},
                    args.rounds, 10)
    res["apply_nodesum_ms"] = {n: median(v) for n, v in t.items()}
    gb = 3 * B * C * L * 4 / 1e9
    print("(c) B x 1024 x %d (%.2f GB through memory once): apply + node_gather_bwd %.3f ms   apply_nodesum %.3f ms (%.2f TB/s)   apply alone %.3f ms" % (
        L, gb, res["apply_nodesum_ms"]["apply+node_gather_bwd"], res["apply_nodesum_ms"]["apply_nodesum"],
        gb / res["apply_nodesum_ms"]["apply_nodesum"], res["apply_nodesum_ms"]["apply_only"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
