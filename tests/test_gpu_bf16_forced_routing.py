"""The bf16 training step's gradients against float64 with the run's routing forced (BASELINE configs[1], ``bench.py --precision bf16
--mode train``).

tests/test_gpu_parity.py::test_training_gradients_with_forced_routing is the gate of the f32-class arithmetics: the run's discrete decisions
(the positions its three arg-max pools took, the ReLU patterns of its eight BatchNorm + ReLU layers) forced on tests/f64_classifier.py, the
float64 restatement pinned to the reference's own float64 run.  Here the same in bf16: the twin runs with ``rounding="bf16"`` and rounds
exactly where the bf16 step stores bf16 (the site list is in the twin's docstring).  In bf16 the roundings are discrete decisions too: a
value a hair from a rounding midpoint goes either way with the f32 summation order, and each such flip perturbs every output of the next
layer in its column -- left free, the flips multiply ~100x per layer and the end-to-end gradients differ by 4e-3 .. 8e-3 rel-rms (measured),
which would hide a bug of that size.  So the run's stored bf16 tensors (raw outputs, pooled values, the input gradients the dgrad launches
store) are forced on the twin as well.  A forced tensor is taken out of every gradient comparison downstream, so each is checked on its own
against the twin's exact value: worst element, rel-rms and scale error within bf16 rounding (BF16_SNAP_*) -- that is what pins the dgrad
launches and the layer outputs.  Every parameter gradient must agree to T = BF16_FORCED_TOL rel-rms, which pins the weight gradients and
the BatchNorm backward.  Measured: profiles/bf16_grad_forced_routing.log.  A 1 % error in any input-gradient launch or layer output, a
weight gradient 2^-7 too large or a BatchNorm-backward term dropped on one layer fails here, while the cosine gate of
tests/test_gpu_bf16.py::test_classifier_training_step_bf16 passes on all but the layer-output error (docs/findings.md, sensitivity)."""
from argparse import Namespace

import pytest
import torch

from conftest import assert_close_rms, golden
from test_gpu_parity import DEV, _capture_stage, _f64_step, _relu_masks_of, _routing_of, cu

pytestmark = pytest.mark.gpu

# worst gradient measured over the six cases 1.1e-4 (synthetic_b36_n5000; 3.6e-5 .. 7.6e-5 on the fixtures): profiles/bf16_grad_forced_routing.log
BF16_FORCED_TOL = 3e-4
# A forced site hides from every gradient downstream whatever error the run's stored tensor carries: these bounds on the distance of each
# stored tensor from the twin's exact value (f64_classifier._snap_stats) are what checks the launch that produced it.  Measured over the six
# cases (profiles/bf16_grad_forced_routing.log); a 1 % error in any input-gradient launch or layer output: ulps 3.5-4.0, rel 1.0e-2, scale 9.7e-3.
#   worst element, in bf16 ulps of max(|value|, rms): 0.5 = correctly rounded, more where a neighbour's rounding decision one layer up went the
#   other way (the twin rounds the activations and g_raw itself); measured <= 2.5.  Catches a local error.
BF16_SNAP_ULPS = 3.0
#   rel-rms distance: bf16 rounding noise, measured 1.65e-3 .. 1.72e-3 on every gradient and layer output.  Catches a global error.
BF16_SNAP_REL = 2.2e-3
#   relative scale error <stored - exact, exact> / <exact, exact>: the noise averages out over the tensor, measured <= 2.4e-5
BF16_SNAP_SCALE = 1e-4

# every bf16 fusion on (default) / off: the store + index_max pool, the apply pass + dgrad backward, the non-matrix-core pooled dgrad
FUSIONS = ("BF16_NORM_ON_LOAD", "BF16_BNB_ON_LOAD", "POOLED_TRAIN_EPILOGUE", "POOLED_DGRAD_MFMA")
LAYERS = ["cls.fc1", "cls.fc2", "final_pointnet.layers.0", "first_pointnet.layers.0", "first_pointnet.layers.1", "first_pointnet.layers.2",
          "knnlayer.layers.0", "knnlayer.layers.1"]


def _inputs(case):
    """A golden fixture, or "synthetic_b36_n5000": the smallest batch of 5000-point clouds whose hidden first-PointNet layers take the
    normalise-on-load (xaff) kernels (B * ceil(3N / 64) >= 8192 column groups: ops.bf16_xaff_ok) -- neither fixture reaches them."""
    if case.startswith("synthetic"):
        from sonet_hip import synth
        B, N = (int(v[1:]) for v in case.split("_")[1:])
        inp = synth.make_inputs(B, N, seed=21)
        return dict(B=B, N=N, seed=5, pc=inp["pc"].numpy(), sn=inp["sn"].numpy(), node=inp["node"].numpy(),
                    node_knn_I=inp["node_knn_I"].numpy(), label=inp["label"].numpy(),
                    # (the parameters without a gradient are the encoder's dead Transformer: a property of the architecture, not of the
                    #  data -- the fixture's count holds for any input)
                    dead_grad_count=int(golden("train_step_b8_n5000")["dead_grad_count"]))
    g = golden(case)
    return {k: g[k] for k in ("B", "N", "seed", "pc", "sn", "node", "node_knn_I", "label", "dead_grad_count")}


def _stored_raws(loss, enc):
    """The stored raw output of every BatchNorm + ReLU layer of the encoder (what its _PointwiseFn node saved for the backward; call BEFORE
    backward): {layer prefix: bf16 tensor}."""
    by_ptr = {p.data_ptr(): k.rsplit(".", 2)[0] for k, p in enc.named_parameters() if k.endswith("conv.weight")}
    out, seen, stack = {}, set(), [loss.grad_fn]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        stack.extend(fn for fn, _ in node.next_functions)
        if type(node).__name__ == "_PointwiseFnBackward" and len(node.saved_tensors) == 10:        # 'batch' mode (see _relu_masks_of)
            layer = by_ptr.get(node.saved_tensors[2].data_ptr())
            if layer is not None:
                out[layer] = node.saved_tensors[5].detach()
    return out


def _hook_stored_grads(loss, enc, feat, grads):
    """Register hooks on the step's autograd nodes (call BEFORE backward) that copy into ``grads`` the bf16 gradients the backward stores at
    the twin's backward sites: the incoming gradient of every BatchNorm layer's output (its consumer's input gradient; for the first layer
    the sum of its two consumers'), the input gradients of the layers whose input is not such an output, and the feature's gradient."""
    from test_gpu_parity import _lastdim_max_node
    by_ptr = {p.data_ptr(): k.rsplit(".", 2)[0] for k, p in enc.named_parameters() if k.endswith("conv.weight")}
    into = {"first_pointnet.layers.0": "first_pointnet.skip.g", "first_pointnet.layers.1": "first_pointnet.layers.2.g_in",
            "first_pointnet.layers.2": None, "knnlayer.layers.0": "knnlayer.layers.1.g_in", "knnlayer.layers.1": None,
            "final_pointnet.layers.0": "final_pointnet.layers.1.g_in"}
    own_in = {"first_pointnet.layers.1": "first_pointnet.layers.1.g_in", "knnlayer.layers.0": "knnlayer.layers.0.g_in",
              "final_pointnet.layers.0": "final_pointnet.layers.0.g_in"}

    def keep(name, t):
        if name is not None and t is not None:
            grads[name] = t.detach().clone()           # (the engine may add a second gradient into this buffer in place)
    seen, stack = set(), [loss.grad_fn]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        stack.extend(fn for fn, _ in node.next_functions)
        kind = type(node).__name__
        if kind not in ("_PointwiseFnBackward", "_PooledLastLayerFnBackward"):
            continue
        layer = by_ptr.get(node.saved_tensors[2].data_ptr())
        if kind == "_PooledLastLayerFnBackward":
            # both panels' input gradients (with the gradient carry the first one is deposited in the carry instead of returned: the node
            # is its own autograd context, and the second layer takes the deposit only after this hook has run)
            def pooled(gi, go, node=node):
                g1 = gi[0] if gi[0] is not None else (node.carry.g if node.carry is not None else None)
                keep("first_pointnet.layers.3.g_in", torch.cat((g1, gi[1]), dim=1) if g1 is not None else None)
            node.register_hook(pooled)
        elif layer in into:
            node.register_hook(lambda gi, go, a=into[layer], b=own_in.get(layer): (keep(a, go[0]), keep(b, gi[0])) and None)
    node = _lastdim_max_node(feat)
    node.register_hook(lambda gi, go: keep("feature.g", go[0]))


def run_bf16_forced(case, fusions, rounding="bf16", probe=None):
    """One bf16 training step of the classifier (``fusions`` False: the switches of FUSIONS off) and the float64 twin with its routing and
    ReLU patterns forced -> dict(loss, feature, mine {param: grad}, r (the twin's result), cap, names (kernels that ran), running {key:
    (before, after)}, g (inputs), carry, enc, cls, stages {pool1, pool2: the pooled values}, probe: what ``probe(loss, enc, cls)`` returned
    before the backward)."""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = _inputs(case)
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.0, node_num=64, k=3, som_k=9, som_k_type="avg",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), seed)
    synth.fill_state_dict_(cls.state_dict(), seed + 1)
    enc.to(DEV).train()
    cls.to(DEV).train()
    enc.want_first_pn_out = False                  # (said explicitly: a live Segmenter of another test would keep the dense tensor)
    before = {("" if m is enc else "cls.") + k: v.detach().clone() for m in (enc, cls) for k, v in m.state_dict().items() if "running" in k}
    old = {k: getattr(ops, k) for k in FUSIONS}
    try:
        if not fusions:
            for k in FUSIONS:
                setattr(ops, k, False)
        with ops.precision("bf16"), ops.kernel_timing() as rec:
            cap = _capture_stage(enc)
            feat = enc(cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), is_train=True, epoch=0)
            score = cls(feat, 0)
            cap.update(_routing_of(enc, feat))
            loss = torch.nn.functional.cross_entropy(score, cu(g["label"]))
            cap["masks"] = _relu_masks_of(loss, enc, cls)
            stored = {k + ".raw": v for k, v in _stored_raws(loss, enc).items()}
            stored.update({"pool1": enc.first_pn_out_masked_max.detach(), "pool2": enc.knn_feature_1.detach(),
                           "final_pointnet.layers.1.raw": enc.final_pn_out.detach()})
            probed = probe(loss, enc, cls) if probe is not None else None
            grads = {}
            _hook_stored_grads(loss, enc, feat, grads)
            loss.backward()
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
    names = set(n for n, _, _ in rec.records)
    # the first layer's two input gradients summed by the store of the second layer's input-gradient launch (the gradient carry)
    carry = any(n.startswith(("pointmlpbf16_bnba", "pointmlpbf16_acc")) for n in names)
    # (the pooled first-PointNet values come back as f32 holding bf16 values)
    assert len(stored) == 9 and all(torch.equal(v, v.to(torch.bfloat16).to(v.dtype)) for v in stored.values()), sorted(stored)
    mfma = "pooled_dgrad_mfma" in names
    assert mfma or "pooled_dgrad" in names, names
    if carry:
        # (its store adds the carried gradient: the second layer's own rounded input gradient is never a tensor -- the twin rounds it)
        grads.pop("first_pointnet.layers.1.g_in", None)
    r = _f64_step(enc, cls, g, cap, forced=True, rounding=rounding, stored=stored if rounding == "bf16" else None,
                  stored_grads=grads if rounding == "bf16" else None, pooled_dgrad="mfma" if mfma else "f32")
    mine = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
    mine.update({"cls." + k: p.grad for k, p in cls.named_parameters() if p.grad is not None})
    after = {("" if m is enc else "cls.") + k: v for m in (enc, cls) for k, v in m.state_dict().items() if "running" in k}
    stages = dict(pool1=enc.first_pn_out_masked_max.detach(), pool2=enc.knn_feature_1.detach())
    return dict(loss=loss.detach(), feature=feat.detach(), mine=mine, r=r, cap=cap, names=names, carry=carry, g=g, enc=enc, cls=cls, stages=stages, probe=probed,
                running={k: (before[k], after[k]) for k in before}, dead=sum(1 for p in enc.parameters() if p.grad is None))


def grad_residuals(res):
    """{param: rel-rms of the run's gradient against the twin's} over the parameters with a true gradient (rms >= 1e-7)."""
    out = {}
    for k, ref in res["r"]["grads"].items():
        if float(ref.norm()) / max(1.0, float(ref.numel()) ** 0.5) < 1e-7:        # biases in front of a BatchNorm: the true gradient is 0
            continue
        out[k] = float((res["mine"][k].double() - ref).norm() / ref.norm()) if k in res["mine"] else float("inf")
    return out


def expected_running(res):
    """The running statistics the step must leave: F.batch_norm's momentum update (momentum 0.1, unbiased variance) of the twin's batch
    statistics.  -> {state-dict key: (expected, got)}."""
    out = {}
    for prefix, (mean, var, n) in res["r"]["bn"].items():
        key = ("cls." + prefix if not prefix.startswith(("first", "knn", "final")) else prefix) + ".norm."
        for stat, batch in (("running_mean", mean), ("running_var", var * n / (n - 1))):
            before, after = res["running"][key + stat]
            out[key + stat] = (0.9 * before.double() + 0.1 * batch, after)
    return out


@pytest.mark.parametrize("fusions", [True, False], ids=["default", "fusions_off"])
@pytest.mark.parametrize("case", ["train_step_b16_n512", "train_step_b8_n5000", "synthetic_b36_n5000"])
def test_bf16_training_gradients_with_forced_routing(case, fusions):
    """Every gradient of the bf16 training step against the float64 twin with the SAME routing and ReLU patterns and bf16 rounding at the
    step's own rounding sites: loss and feature agree, every encoder and head gradient (whole tensors) within BF16_FORCED_TOL rel-rms,
    the running statistics are the twin's batch statistics through the momentum update."""
    res = run_bf16_forced(case, fusions)
    names, cap, r = res["names"], res["cap"], res["r"]
    N, B = int(res["g"]["N"]), int(res["g"]["B"])
    # the case exercises what it claims
    assert any(n.startswith("pointmlpbf16") for n in names) and not any(n.startswith(("pointmlph3", "pointmlpx3")) for n in names), names
    assert {"pointwise_bwd_stats_bf16", "pooled_wgrad", "knn_gather_bwd", "lastdim_max_bwd"} <= names or \
        {"pointwise_bwd_stats_bf16", "pooled_wgrad_xaff", "knn_gather_bwd", "lastdim_max_bwd"} <= names, names
    bnb = B * 3 * N >= 65536                       # B * L: the bf16 BatchNorm backward on the dgrad's operand load (pointmlp_bf16_bnb)
    xaff = B * ((3 * N + 63) // 64) >= 8192        # the normalise-on-load hidden layers (bf16_xaff_ok)
    assert any(n.startswith("pointmlpbf16_bnb") for n in names) == (fusions and bnb), names
    assert ("pooled_dgrad_mfma" in names) == fusions and ("pooled_dgrad" in names) == (not fusions), names
    assert any(n.startswith("pointmlpbf16_pool") for n in names) == fusions and ("index_max_gather_bf16" in names) == (not fusions), names
    assert any(n.endswith("_xaff") or "_xaff_" in n for n in names) == (fusions and xaff), names
    assert res["carry"] == (fusions and xaff), names
    # the helpers saw the bf16 graph: all eight ReLU patterns, the three pools' positions, every stored tensor the twin takes its rounding
    # decisions from -- and each of those is the twin's exact value rounded (to within a neighbour's decision)
    assert len(r["snap"]) == 9 + (8 if res["carry"] else 9), sorted(r["snap"])     # (with the carry the second layer's g_in is not stored)
    for what, bound in (("ulps", BF16_SNAP_ULPS), ("rel", BF16_SNAP_REL), ("scale", BF16_SNAP_SCALE)):
        worst = max(r["snap"].items(), key=lambda kv: abs(kv[1][what]))
        assert abs(worst[1][what]) <= bound, (what, worst)
    # no empty node in these cases: the column-0 mat-vec of the sparse dgrad (models/layers.py:625, :644-646: f32 weights, a second bf16
    # rounding of column 0) does not run, and the twin does not model it
    assert int((cap["row_max"] == 0).sum()) == 0
    assert sorted(cap["masks"]) == LAYERS, sorted(cap["masks"])
    assert cap["pos0"] is None and cap["pool1"].shape == (B, 384, 64) and cap["pool2"].shape == (B, 512, 64) and cap["pool3"].shape == (B, 1024)
    # the feature is the run's stored final-layer output gathered at the run's positions (both forced): it equals the twin's by
    # construction, and what checks it is the snap of "final_pointnet.layers.1.raw" above.  Given that feature, the loss checks the heads'
    # f32 forward against float64.
    assert torch.equal(res["feature"].double(), r["feature"])
    assert abs(float(res["loss"]) - float(r["loss"])) <= 1e-5 * abs(float(r["loss"])), (float(res["loss"]), float(r["loss"]))
    # every parameter gradient
    rel = grad_residuals(res)
    worst = max(rel.items(), key=lambda kv: kv[1])
    print("bf16 forced routing %s %s: worst gradient %s %.3e (T %.0e)" % (case, "default" if fusions else "fusions_off", worst[0], worst[1],
                                                                          BF16_FORCED_TOL))
    assert len(rel) >= 25, len(rel)
    assert worst[1] <= BF16_FORCED_TOL, sorted(rel.items(), key=lambda kv: -kv[1])[:6]
    assert res["dead"] == int(res["g"]["dead_grad_count"])
    # running statistics
    run = expected_running(res)
    assert len(run) == 2 * 8, sorted(run)
    for k, (want, got) in run.items():
        assert_close_rms(got.cpu().numpy(), want.cpu().numpy(), 1e-5, "running stat " + k)       # (measured <= 7.5e-7)
