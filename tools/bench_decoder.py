"""tools/bench_decoder.py -- the decoder's up-convolutions: the aten path (upsample + MIOpen conv + BatchNorm + ReLU) against the fused
launch (ops.upconv3x3, opt.decoder_fused), in ONE process on one MI355X.

    python tools/bench_decoder.py [--batch 64] [--rounds 5] [--iters 20] [--points 5000] [--spin-up 1.0] [--skip-forward]
    python tools/bench_decoder.py --train [--batch 64] [--rounds 5] [--iters 10] [--spin-up 1.0]

After the clock spin-up bench.py uses (untimed calls for --spin-up seconds: an idle MI355X sits at its lowest clock), every pair of
variants is timed INTERLEAVED -- aten, fused, aten, fused, ... --rounds rounds of --iters calls each, every group bracketed by HIP
events on the launch stream -- and the median over the rounds is reported:
  (a)/(b) each of the six layers of DecoderConv at feature_num 1024, eval mode, on the activations the layer sees in the decoder;
          with the algorithmic floor of the fused launch: deconv1 / deconv2 -- the packed weight bytes the launch reads (the (parity, tap)
          pairs that are live) over the time = achieved weight bandwidth; deconv5 / deconv6 -- 3 MFMA products x 2 x 4 Cin Cout per
          output-parity pixel over the time, against the sustained rate of a pure v_mfma_f32_32x32x16_f16 loop on this chip
          (ops.mfma_f16_sustained_rate) = fraction of the three-term matrix ceiling;
  (-)     the whole Decoder.forward (FC decoder + conv pyramid + point heads), eager, option off and on;
  (c)     configs[3] of bench.py: encoder + decoder + two-resolution Chamfer loss, HIP-graph replay on one stream, option off and on.
--train: the TRAINING step of the same six layers at feature_num 1024, option off (the two aten lines per layer) against
opt.decoder_fused_train (layers._UpConvTrainFn), interleaved in the same way.  Per layer: the forward (autograd on), forward + backward
and their difference, and for the fused backward its parts timed on their own -- the folded input gradient (ops.upconv3x3_dgrad), the
weight gradient (upsample + aten's convolution backward, weight only) and the BatchNorm / ReLU / bias passes; then one training step of
the whole DecoderConv (forward + backward on fixed cotangents), option off, on, and on for layers (4, 5, 6).  A third variant,
opt.decoder_fused_train plus opt.decoder_fused_wgrad, is interleaved with the two: per layer the folded weight-gradient launch
(ops.upconv3x3_wgrad, column "wgrad hip") beside the aten weight gradient it replaces (column "wgrad") and the layer's step with it, and
the DecoderConv step with it on all six layers and on (4, 5, 6).
Prints a table and one JSON line (last line).
"""
import argparse
import json
import os
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "so-net_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


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


def live_pairs(H, W):
    """(parity, tap) pairs whose shifted operand is inside the map for at least one pixel: 4 at 1 x 1 ... 16 from 2 x 2 on (per axis: the
    shifts -1 and +1 need a second row / column)."""
    ny = 2 if H == 1 else 4
    nx = 2 if W == 1 else 4
    return ny * nx


def train_bench(args):
    import bench
    from models import networks as NW
    from sonet_hip import ops, synth
    dev = torch.device("cuda", 0)
    B, F_ = args.batch, 1024

    def make(train_opt, wgrad_opt=False):
        opt = Namespace(gpu_id=0, device=dev, feature_num=F_, activation="relu", normalization="batch", output_fc_pc_num=0,
                        output_conv_pc_num=4096, decoder_fused_train=train_opt, decoder_fused_wgrad=wgrad_opt)
        d = NW.Decoder(opt)
        synth.fill_state_dict_(d.state_dict(), 2)
        return d.to(dev).train()

    decs = {"aten": make(False), "fused": make(True), "fused456": make((4, 5, 6)), "wgrad": make(True, True),
            "wgrad456": make((4, 5, 6), (4, 5, 6))}
    feat = torch.randn(B, F_, generator=torch.Generator().manual_seed(5)).abs().to(dev)
    gen = torch.Generator().manual_seed(6)
    cots = {i: (torch.randn(B, 3, n, generator=gen) * 1e-3).to(dev) for i, n in ((4, 256), (5, 1024), (6, 4096))}
    result = {"batch": B, "rounds": args.rounds, "iters": args.iters, "train_layers": {}}

    def step(dec):
        feat.grad = None
        for p in dec.parameters():
            p.grad = None
        dec(feat)
        sum((getattr(dec, "conv_pc%d" % i) * cots[i]).sum() for i in (4, 5, 6)).backward()

    with torch.no_grad():
        xs, x = [], feat.view(-1, F_, 1, 1)
        for i in range(1, 7):
            xs.append(x)
            x = getattr(decs["aten"].conv_decoder, "deconv%d" % i)(x)
    feat = feat.clone().requires_grad_(True)                     # (in training the feature is the encoder's: it needs its gradient)
    for _ in range(3):
        for d in decs.values():
            step(d)
    torch.cuda.synchronize()
    bench._spin_up(lambda: [step(d) for d in decs.values()], args.spin_up)
    print("%-8s %-16s | %9s %9s | %9s %9s %9s | %8s %8s %9s %8s | %7s %7s" % (
        "layer", "Cin->Cout @ HxW", "aten fwd", "aten bwd", "fused fwd", "fused bwd", "+wgrad bwd", "dgrad", "wgrad", "wgrad hip", "passes",
        "step x", "+wgrad x"))
    for i in range(1, 7):
        ma, mf, mw = (getattr(decs[k].conv_decoder, "deconv%d" % i) for k in ("aten", "fused", "wgrad"))
        xi = xs[i - 1].clone().requires_grad_(True)
        Cin, Cout, H, W = xi.shape[1], ma.conv.conv.out_channels, xi.shape[2], xi.shape[3]
        gy = torch.randn(B, Cout, 2 * H, 2 * W, generator=torch.Generator().manual_seed(i)).to(dev) * 1e-3

        def fb(m):
            xi.grad = None
            for p in m.parameters():
                p.grad = None
            m(xi).backward(gy)

        # the parts of the fused backward on their own operands
        wpt = ops.upconv3x3_dgrad_pack(mf.conv.conv.weight.detach().contiguous())
        ones, zeros = ops.const_vec(Cout, 1.0, dev), ops.const_vec(Cout, 0.0, dev)
        with torch.no_grad():
            raw = ops.upconv3x3(xi.detach(), mf._packed_upconv(), ones, mf.conv.conv.bias.detach(), False, Cout)
            raw3, gy3 = raw.view(B, Cout, -1), gy.view(B, Cout, -1)
            mean, var = ops.channel_stats(raw3)
            invstd, sc, sh = ops.bn_fwd_coeffs(mean, var, mf.conv.norm.weight, mf.conv.norm.bias, 1e-5)
            wgt = mf.conv.conv.weight.detach()

        def passes():
            sums = ops.pointwise_bwd_stats(gy3, raw3, sc, sh, True, want_sums=True)
            a, b, c0, _gg, _gb = ops.bn_bwd_coeffs(sums, mean, invstd, mf.conv.norm.weight, float(B * 4 * H * W))
            g_raw3 = ops.pointwise_bwd_apply(gy3, raw3, sc, sh, True, a, b, c0)
            ops.pointwise_bwd_stats(g_raw3, g_raw3, ones, zeros, False)

        def wgrad():
            up = torch.nn.functional.interpolate(xi.detach(), scale_factor=2)
            torch.ops.aten.convolution_backward(gy, up, wgt, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))

        xd = xi.detach()
        fns = {"aten_fwd": lambda: ma(xi), "aten_fb": lambda: fb(ma), "fused_fwd": lambda: mf(xi), "fused_fb": lambda: fb(mf),
               "wgrad_fb": lambda: fb(mw), "dgrad": lambda: ops.upconv3x3_dgrad(gy, wpt, Cin), "wgrad": wgrad,
               "wgrad_hip": lambda: ops.upconv3x3_wgrad(gy, xd), "passes": passes}
        for fn in fns.values():
            for _ in range(3):
                fn()
        t = {k: median(v) for k, v in timed_pairs(fns, args.rounds, args.iters).items()}
        e = {"shape": "%d->%d @ %dx%d" % (Cin, Cout, H, W)}
        e.update({k + "_ms": round(v, 4) for k, v in t.items()})
        e["aten_bwd_ms"], e["fused_bwd_ms"] = round(t["aten_fb"] - t["aten_fwd"], 4), round(t["fused_fb"] - t["fused_fwd"], 4)
        e["wgrad_bwd_ms"] = round(t["wgrad_fb"] - t["fused_fwd"], 4)
        e["step_speedup"], e["wgrad_step_speedup"] = round(t["aten_fb"] / t["fused_fb"], 3), round(t["aten_fb"] / t["wgrad_fb"], 3)
        print("deconv%d  %-16s | %9.4f %9.4f | %9.4f %9.4f %9.4f | %8.4f %8.4f %9.4f %8.4f | %6.2fx %6.2fx" % (
            i, e["shape"], t["aten_fwd"], e["aten_bwd_ms"], t["fused_fwd"], e["fused_bwd_ms"], e["wgrad_bwd_ms"], t["dgrad"], t["wgrad"],
            t["wgrad_hip"], t["passes"], e["step_speedup"], e["wgrad_step_speedup"]))
        result["train_layers"]["deconv%d" % i] = e
    t = {k: median(v) for k, v in timed_pairs({k: (lambda d=d: step(d)) for k, d in decs.items()}, args.rounds, args.iters).items()}
    print("DecoderConv training step (forward + backward, eager): option off %.4f ms, on %.4f ms (%.2fx), on for layers 4-6 %.4f ms (%.2fx)"
          % (t["aten"], t["fused"], t["aten"] / t["fused"], t["fused456"], t["aten"] / t["fused456"]))
    print("... with decoder_fused_wgrad as well: on %.4f ms (%.2fx), both on for layers 4-6 %.4f ms (%.2fx)"
          % (t["wgrad"], t["aten"] / t["wgrad"], t["wgrad456"], t["aten"] / t["wgrad456"]))
    result["decoder_train_step"] = {k + "_ms": round(v, 4) for k, v in t.items()}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--spin-up", type=float, default=1.0)
    ap.add_argument("--skip-forward", action="store_true", help="layers and Decoder.forward only (no encoder / Chamfer graph)")
    ap.add_argument("--train", action="store_true", help="the training step: option off against opt.decoder_fused_train")
    args = ap.parse_args()
    if args.train:
        return train_bench(args)
    import bench
    from models import losses as LS, networks as NW
    from sonet_hip import ops, synth
    from sonet_hip.graph import GraphedForward
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.points

    def make_opt(fused):
        return Namespace(gpu_id=0, device=dev, batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                         normalization="batch", dropout=0.6, node_num=64, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                         bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40, output_fc_pc_num=256, output_conv_pc_num=1024,
                         decoder_fused=fused)

    decs = {}
    for fused in (False, True):
        d = NW.Decoder(make_opt(fused))
        synth.fill_state_dict_(d.state_dict(), 2)
        decs[fused] = d.to(dev).eval()
    feat = torch.randn(B, 1024, generator=torch.Generator().manual_seed(5)).abs().to(dev)
    result = {"batch": B, "rounds": args.rounds, "iters": args.iters, "layers": {}}

    with torch.no_grad():
        # the activations each layer sees (from the aten decoder)
        xs, x = [], feat.view(-1, 1024, 1, 1)
        for i in range(1, 7):
            xs.append(x)
            x = getattr(decs[False].conv_decoder, "deconv%d" % i)(x)
        torch.cuda.synchronize()
        both = lambda: (decs[False](feat), decs[True](feat))          # noqa: E731
        for _ in range(3):
            both()
        bench._spin_up(both, args.spin_up)
        tf, ghz = ops.mfma_f16_sustained_rate(random_operands=True)
        result["mfma_f16_sustained_tflops"], result["mfma_clock_ghz"] = round(tf, 1), round(ghz, 3)
        print("sustained v_mfma_f32_32x32x16_f16 rate (random operands): %.1f TFLOP/s at %.2f GHz" % (tf, ghz))
        print("%-8s %-16s %10s %10s %8s  %s" % ("layer", "Cin->Cout @ HxW", "aten ms", "fused ms", "speedup", "fused launch against its floor"))
        for i in range(1, 7):
            ma, mf = (getattr(decs[k].conv_decoder, "deconv%d" % i) for k in (False, True))
            xi = xs[i - 1]
            Cin, Cout, H, W = xi.shape[1], ma.conv.conv.out_channels, xi.shape[2], xi.shape[3]
            fns = {"aten": lambda: ma(xi), "fused": lambda: mf(xi)}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            t = timed_pairs(fns, args.rounds, args.iters)
            a, f = median(t["aten"]), median(t["fused"])
            e = {"shape": "%d->%d @ %dx%d" % (Cin, Cout, H, W), "aten_ms": round(a, 4), "fused_ms": round(f, 4),
                 "aten_ms_rounds": [round(v, 4) for v in t["aten"]], "fused_ms_rounds": [round(v, 4) for v in t["fused"]]}
            wbytes = live_pairs(H, W) * Cout * (-(-Cin // ops.UPCONV_K_CHUNK) * ops.UPCONV_K_CHUNK) * 4          # two fp16 pieces per folded weight
            flop3 = 3 * 2.0 * 4 * Cin * Cout * 4 * B * H * W                                                        # three MFMA products per multiply
            e["weight_GBps"] = round(wbytes / (f * 1e-3) / 1e9, 1)
            e["mfma_tflops_equiv"] = round(flop3 / (f * 1e-3) / 1e12, 1)
            e["fraction_of_matrix_ceiling"] = round(flop3 / (f * 1e-3) / 1e12 / tf, 3)
            note = ("%.0f GB/s of packed weights (%.1f MB)" % (e["weight_GBps"], wbytes / 1e6)) if i <= 2 else \
                   ("%.1f TF-equivalent = %.1f %% of the matrix ceiling" % (e["mfma_tflops_equiv"], 100 * e["fraction_of_matrix_ceiling"]))
            print("deconv%d  %-16s %10.4f %10.4f %7.2fx  %s" % (i, e["shape"], a, f, a / f, note))
            result["layers"]["deconv%d" % i] = e
        fns = {"aten": lambda: decs[False](feat), "fused": lambda: decs[True](feat)}
        t = timed_pairs(fns, args.rounds, args.iters)
        a, f = median(t["aten"]), median(t["fused"])
        print("Decoder.forward (eager, FC + conv pyramid + heads): aten %.4f ms, fused %.4f ms (%.2fx)" % (a, f, a / f))
        result["decoder_forward"] = {"aten_ms": round(a, 4), "fused_ms": round(f, 4), "aten_ms_rounds": [round(v, 4) for v in t["aten"]],
                                     "fused_ms_rounds": [round(v, 4) for v in t["fused"]]}
        if not args.skip_forward:
            inp = synth.make_inputs(B, N, seed=3, device=dev)
            graphs = {}
            for fused in (False, True):
                opt = make_opt(fused)
                enc, crit = NW.Encoder(opt), LS.ChamferLoss(opt)
                synth.fill_state_dict_(enc.state_dict(), 1)
                enc.to(dev).eval()
                dec = decs[fused]

                def fwd(pc, sn, node, knn, enc=enc, dec=dec, crit=crit):
                    pred = dec(enc(pc, sn, node, knn, False, None))
                    return crit(pred, pc) + crit(dec.conv_pc4, pc)
                graphs[fused] = GraphedForward(fwd, (inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"]), warmup=3)
            fns = {"aten": lambda: graphs[False](inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"]),
                   "fused": lambda: graphs[True](inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"])}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            t = timed_pairs(fns, args.rounds, args.iters)
            a, f = median(t["aten"]), median(t["fused"])
            la, lf = float(graphs[False].static_output), float(graphs[True].static_output)
            bad = graphs[True].range_violations()
            print("configs[3] autoencoder forward (graph replay, %d x %d): option off %.4f ms (%.0f clouds/s), on %.4f ms (%.0f clouds/s), %.2fx; "
                  "loss off %.6f on %.6f; range-guard violations %d" % (B, N, a, B / a * 1e3, f, B / f * 1e3, a / f, la, lf, len(bad)))
            result["autoencoder_forward"] = {"off_ms": round(a, 4), "on_ms": round(f, 4), "off_ms_rounds": [round(v, 4) for v in t["aten"]],
                                             "on_ms_rounds": [round(v, 4) for v in t["fused"]], "loss_off": la, "loss_on": lf,
                                             "range_guard_violations": len(bad)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
