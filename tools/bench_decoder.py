"""tools/bench_decoder.py -- the decoder's up-convolutions: the aten path (upsample + MIOpen conv + BatchNorm + ReLU) against the fused
launch (ops.upconv3x3, opt.decoder_fused), in ONE process on one MI355X.

    python tools/bench_decoder.py [--batch 64] [--rounds 5] [--iters 20] [--points 5000] [--spin-up 1.0] [--skip-forward]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--spin-up", type=float, default=1.0)
    ap.add_argument("--skip-forward", action="store_true", help="layers and Decoder.forward only (no encoder / Chamfer graph)")
    args = ap.parse_args()
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
