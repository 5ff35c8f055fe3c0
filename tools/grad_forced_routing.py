#!/usr/bin/env python3
"""Per-parameter deviation of the training step's gradients from a float64 run of the same step with the SAME arg-max routing
(tests/f64_classifier.py, the restatement pinned to the reference's float64 run), for each arithmetic and both training fixtures --
the table behind tests/test_gpu_parity.py::test_training_gradients_with_forced_routing.

    python tools/grad_forced_routing.py [--modes h3,x3,f32] [--fixtures train_step_b16_n512,train_step_b8_n5000] [--env KEY=VAL ...]

``--modes bf16``: the bf16 step against the twin with ``rounding="bf16"`` and the run's rounding decisions forced (and, for scale, against
the plain float64 twin with the routing forced), for every bf16
switch setting of ``--fusions`` (default: every fusion on; off: tests/test_gpu_bf16_forced_routing.py FUSIONS) -- the table behind
tests/test_gpu_bf16_forced_routing.py::test_bf16_training_gradients_with_forced_routing (``synthetic_b36_n5000`` is its third case).

``--head segmenter``: the part-segmentation step (``networks.segmentation_forward``) against tests/f64_segmenter.py with its routing and
ten ReLU patterns forced, every gradient listed -- the table behind tests/test_gpu_seg_training.py::test_seg_training_gradients_with_forced_routing
(fixtures default to ``seg_train_step_b8_n512,synthetic_b16_n1024``).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="h3,x3,f32")
ap.add_argument("--fixtures", default=None, help="default: train_step_b16_n512,train_step_b8_n5000 (segmenter: seg_train_step_b8_n512,"
                                                  "synthetic_b16_n1024)")
ap.add_argument("--head", default="classifier", choices=("classifier", "segmenter"))
ap.add_argument("--fusions", default="default,off", help="bf16 mode: the switch settings")
ap.add_argument("--set", nargs="*", default=[], help="ops switches, e.g. DEFER_WGRAD_JOIN=0 BNB_ON_LOAD=0")
args = ap.parse_args()
if args.fixtures is None:
    args.fixtures = "train_step_b16_n512,train_step_b8_n5000" if args.head == "classifier" else "seg_train_step_b8_n512,synthetic_b16_n1024"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import test_gpu_parity as T  # noqa: E402
from argparse import Namespace  # noqa: E402
from models import networks as NW  # noqa: E402
from sonet_hip import ops, synth  # noqa: E402

for kv in args.set:
    k, v = kv.split("=")
    setattr(ops, k, v not in ("0", "False", "false"))
    print("ops.%s = %s" % (k, getattr(ops, k)))
DEV = T.DEV


def bf16_case(fixture, fusions):
    """The bf16 step against the bf16 twin (and the plain float64 twin): the per-parameter table, loss, feature and running statistics."""
    import test_gpu_bf16_forced_routing as BF
    res = BF.run_bf16_forced(fixture, fusions)
    r, cap = res["r"], res["cap"]
    rel = BF.grad_residuals(res)
    plain = BF.grad_residuals(dict(res, r=T._f64_step(res["enc"], res["cls"], res["g"], cap, forced=True)))
    print("\n== %s  bf16 %s  carry=%s  loss %.9f (bf16 twin %.9f, rel %.2e)  masks %d layers" % (
        fixture, "default" if fusions else "fusions_off", res["carry"], float(res["loss"]), float(r["loss"]),
        abs(float(res["loss"]) - float(r["loss"])) / abs(float(r["loss"])), len(cap["masks"])))
    print("   kernels:", " ".join(sorted(res["names"])))
    print("   stored bf16 tensors vs the twin's exact values: worst ulps of max(|value|, rms) / rel-rms / relative scale error")
    for k, v in sorted(r["snap"].items()):
        print("     %-32s %6.3f  %.3e  %+.2e" % (k, v["ulps"], v["rel"], v["scale"]))
    for what, f_got, f_ref in (("pool1", res["stages"]["pool1"], r["sites"]["pool1"]), ("pool2", res["stages"]["pool2"], r["sites"]["pool2"]),
                               ("feature", res["feature"], r["feature"])):
        f_got = f_got.double()
        d = (f_got - f_ref).abs()
        print("   %-8s rel-rms %.3e  worst |d| / max(|ref|, rms) %.3e  elements that differ %d / %d" % (
            what, float((f_got - f_ref).norm() / f_ref.norm()), float((d / torch.maximum(f_ref.abs(), f_ref.pow(2).mean().sqrt())).max()),
            int((d > 0).sum()), d.numel()))
    worst_run = ("", 0.0)
    for k, (want, got) in BF.expected_running(res).items():
        want, got = want.double(), got.double()
        e = float(((got - want).abs() / torch.maximum(want.abs(), want.pow(2).mean().sqrt())).max())
        worst_run = max(worst_run, (k, e), key=lambda kv: kv[1])
    print("   running statistics: worst err / max(|ref|, rms) %.3e (%s)" % (worst_run[1], worst_run[0]))
    print("   %-45s %-11s %s" % ("parameter (rel-rms vs)", "bf16 twin", "plain f64 twin"))
    for k, v in sorted(rel.items(), key=lambda kv: -kv[1]):
        print("   %-45s %.3e   %.3e" % (k, v, plain.get(k, float("nan"))))
    print("   worst %.3e over %d parameters (plain f64 twin: %.3e)" % (max(rel.values()), len(rel), max(plain.values())))


def seg_case(case, mode):
    """The segmentation step against the forced float64 segmenter twin: loss, scores, running statistics, every gradient."""
    import test_gpu_seg_training as S
    g = S._inputs(case)
    res = S.run_seg_step(g, mode)
    r = S.f64_seg_step(res, g, forced=True)
    free = S.f64_seg_step(res, g, forced=False)
    cap = res["cap"]
    fl = [int((free["route"][p] != cap[p]).sum()) for p in ("pool1", "pool2", "pool3")]
    rel = S.grad_residuals(res, r)
    sc, sr = res["score"].double(), r["score"]
    print("\n== %s  %s  dense=%s  loss %.9f (f64 forced %.9f, rel %.2e)  score rel-rms %.2e  flips vs free f64 run: pool1 %d pool2 %d "
          "pool3 %d  masks %d layers" % (case, mode, cap["need_dense"], float(res["loss"]), float(r["loss"]),
                                        abs(float(res["loss"]) - float(r["loss"])) / abs(float(r["loss"])),
                                        float((sc - sr).norm() / sr.norm()), fl[0], fl[1], fl[2], len(cap["masks"])))
    worst_run = ("", 0.0)
    for k, (want, got) in S.expected_running(res, r).items():
        want, got = want.double(), got.double()
        e = float(((got - want).abs() / torch.maximum(want.abs(), want.pow(2).mean().sqrt())).max())
        worst_run = max(worst_run, (k, e), key=lambda kv: kv[1])
    print("   running statistics: worst err / max(|ref|, rms) %.3e (%s)" % (worst_run[1], worst_run[0]))
    print("   kernels:", " ".join(sorted(res["names"])))
    for k, v in sorted(rel.items(), key=lambda kv: -kv[1]):
        print("   %-45s %.3e" % (k, v))
    print("   worst %.3e over %d parameters" % (max(rel.values()), len(rel)))


for fixture in args.fixtures.split(","):
    for mode in args.modes.split(","):
        if args.head == "segmenter":
            seg_case(fixture, mode)
            torch.cuda.empty_cache()
            continue
        if mode == "bf16":
            for fu in args.fusions.split(","):
                bf16_case(fixture, fu == "default")
                torch.cuda.empty_cache()
            continue
        g = T.golden(fixture)
        B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
        opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                        activation="relu", normalization="batch", dropout=0.0, node_num=64, k=3, som_k=9, som_k_type="avg",
                        bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)
        enc, cls = NW.Encoder(opt), NW.Classifier(opt)
        synth.fill_state_dict_(enc.state_dict(), seed)
        synth.fill_state_dict_(cls.state_dict(), seed + 1)
        enc.to(DEV).train()
        cls.to(DEV).train()
        enc.want_first_pn_out = False
        with ops.precision(mode):
            cap = T._capture_stage(enc)
            feat = enc(T.cu(g["pc"]), T.cu(g["sn"]), T.cu(g["node"]), T.cu(g["node_knn_I"]), is_train=True, epoch=0)
            score = cls(feat, 0)
            cap.update(T._routing_of(enc, feat))
            loss = torch.nn.functional.cross_entropy(score, T.cu(g["label"]))
            cap["masks"] = T._relu_masks_of(loss, enc, cls)
            print("masks:", {k: tuple(v.shape) for k, v in cap["masks"].items()})
            loss.backward()
        torch.cuda.synchronize()
        r = T._f64_step(enc, cls, g, cap, forced=True)
        free = T._f64_step(enc, cls, g, cap, forced=False)
        fl = [int((free["route"][p] != cap[p]).sum()) for p in ("pool1", "pool2", "pool3")]
        mine = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
        mine.update({"cls." + k: p.grad for k, p in cls.named_parameters() if p.grad is not None})
        print("\n== %s  %s  sorted=%s  loss %.9f (f64 forced %.9f)  flips vs free f64 run: pool1 %d pool2 %d pool3 %d"
              % (fixture, mode, cap["pos0"] is not None, float(loss), float(r["loss"]), fl[0], fl[1], fl[2]))
        rows = []
        for k, ref in r["grads"].items():
            rn = float(ref.norm()) / max(1.0, float(ref.numel()) ** 0.5)
            if rn < 1e-7 or k not in mine:
                continue
            rows.append((float((mine[k].double() - ref).norm() / ref.norm()), k))
        for rel, k in sorted(rows, reverse=True)[:12]:
            print("   %-45s %.3e" % (k, rel))
