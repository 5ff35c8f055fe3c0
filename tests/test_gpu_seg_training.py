"""The part-segmentation training step on the MI355X (``networks.segmentation_forward(..., is_train=True)`` + the reference's
CrossEntropyLossSeg + backward) against float64.

The classifier's step is gated by tests/test_gpu_parity.py; the segmentation step takes paths the classifier never takes: the encoder's
dense ``first_pn_out`` (the last first-PointNet layer's gradient is the sum of a dense branch -- segmenter layer 1 -- and the sparse pool
branch), three node-level maps with two consumers each (the encoder's next stage and the segmenter's back-broadcast gather), and the
head's layers in training mode (layer 1: 3356 -> 1024 over k x N columns, the k-copy mean between layers 3 and 4, layer 5: 128 -> 50).

(a) forced routing: the float64 twin (tests/f64_segmenter.py, pinned on the CPU to the reference's float64 run by
    tests/test_f64_segmenter_cpu.py) is fed the run's SOM stage, pool positions and all ten ReLU patterns; every gradient must then
    agree to SEG_FORCED_TOL rel-rms -- no flipped decision can explain a difference;
(b) free routing against the reference fixture (tests/golden/seg_train_step_b8_n512.npz), as the classifier's golden step test;
(c) which kernels ran (a silent fallback would make (a) vacuous);
(d) the reference Model's own data flow (models/segmenter.py:79-109 restated: mask argmax, three torch.gather calls, segmenter(...))
    gives the segmentation_forward step bit for bit (both under torch's deterministic algorithms: the reference's torch.gather has an
    atomic backward otherwise);
(e) two identical segmentation_forward steps give bit-identical loss, scores, gradients and running statistics.
"""
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import assert_close_rms, golden
from train_step_helpers import DEV, _capture_stage, _relu_masks_of, _routing_of, cu

pytestmark = pytest.mark.gpu

FIXTURE = "seg_train_step_b8_n512"
SEG_FORCED_TOL = 1e-4          # every gradient, whole tensors, rel-rms against the forced float64 twin (the classifier's bound)
ENC_LAYERS = ["final_pointnet.layers.0", "first_pointnet.layers.0", "first_pointnet.layers.1", "first_pointnet.layers.2",
              "knnlayer.layers.0", "knnlayer.layers.1"]
SEG_LAYERS = ["seg.layer1", "seg.layer2", "seg.layer3", "seg.layer4"]
# (Cin, Cout) of the segmenter's five layers at the part-seg defaults (surface normals, som_k 9, feature 1024, 50 part classes)
SEG_SHAPES = [(3356, 1024), (1024, 512), (512, 256), (256, 128), (128, 50)]


def _inputs(case):
    """The fixture, or "synthetic_b16_n1024": configs[2]'s point count at 16 clouds (no fixture: the forced twin is the reference)."""
    if case.startswith("synthetic"):
        from sonet_hip import synth
        B, N = (int(v[1:]) for v in case.split("_")[1:])
        inp = synth.make_inputs(B, N, M=64, som_k=9, seed=61, node_kind="som")
        gen = torch.Generator().manual_seed(61)
        return dict(B=B, N=N, seed=601, pc=inp["pc"].numpy(), sn=inp["sn"].numpy(), node=inp["node"].numpy(),
                    node_knn_I=inp["node_knn_I"].numpy(), label=torch.randint(0, 16, (B,), generator=gen).numpy(),
                    seg=torch.randint(0, 50, (B, N), generator=gen).numpy(),
                    # (the parameters without a gradient are the encoder's dead Transformer: a property of the architecture)
                    dead_grad_count=int(golden(FIXTURE)["dead_grad_count"]))
    return golden(case)


def _models(g):
    from models import networks as NW
    from sonet_hip import synth
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.0, node_num=64, k=3, som_k=9, som_k_type="center",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=50)
    enc, seg = NW.Encoder(opt), NW.Segmenter(opt)
    synth.fill_state_dict_(enc.state_dict(), seed)
    synth.fill_state_dict_(seg.state_dict(), seed + 1)
    enc.to(DEV).train()
    seg.to(DEV).train()
    return enc, seg


def _running(enc, seg):
    return {("seg." if m is seg else "") + k: v.detach().clone() for m in (enc, seg) for k, v in m.state_dict().items() if "running" in k}


def run_seg_step(g, mode, data_flow="segmentation_forward"):
    """One segmentation training step in arithmetic ``mode`` on fresh models: forward, loss, backward (no optimizer step).
    ``data_flow`` "segmentation_forward" (the project's entry) or "reference_model" (models/segmenter.py:79-109 restated: nobody tells
    the encoder that first_pn_out is read, the mask argmax and three torch.gather calls, the Segmenter called directly).
    -> dict(loss, score, mine {param: grad; head "seg." + key}, cap (stage, routing, ReLU patterns), names (kernels that ran), bmm
    (shapes of the torch.bmm calls: the library GEMM, which ``kernel_timing`` does not see), running {key: (before, after)}, enc, seg,
    dead)."""
    from models import networks as NW
    from models.losses import CrossEntropyLossSeg
    from sonet_hip import ops
    enc, seg = _models(g)
    before = _running(enc, seg)
    pc, sn, node, knn_I, label = cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), cu(g["label"])
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = mode
    bmm, orig_bmm = [], torch.bmm

    def recording_bmm(a, b, *args, **kw):
        bmm.append((tuple(a.shape), tuple(b.shape)))
        return orig_bmm(a, b, *args, **kw)
    try:
        torch.bmm = recording_bmm
        with ops.kernel_timing() as rec:
            cap = _capture_stage(enc)
            if data_flow == "segmentation_forward":
                score = NW.segmentation_forward(enc, seg, pc, sn, label, node, knn_I, is_train=True, epoch=0)
            elif data_flow == "reference_model":
                assert "want_first_pn_out" not in enc.__dict__
                feature = enc(pc, sn, node, knn_I, True, 0)
                B, F_, N, k = feature.size()[0], feature.size()[1], pc.size()[2], 3
                _, mask_max_idx = torch.max(enc.mask, dim=2, keepdim=False)
                mask_max_idx = mask_max_idx.unsqueeze(1)
                g1 = torch.gather(enc.first_pn_out_masked_max, dim=2, index=mask_max_idx.expand(B, 384, k * N).detach())
                g2 = torch.gather(enc.knn_feature_1, dim=2, index=mask_max_idx.expand(B, 512, k * N).detach())
                g3 = torch.gather(enc.final_pn_out, dim=2, index=mask_max_idx.expand(B, F_, k * N).detach())
                score = seg(enc.x_decentered, pc, enc.centers, sn, label, enc.first_pn_out, g1, g2, g3, feature)
            else:
                raise ValueError(data_flow)
            cap.update(_routing_of(enc, enc.feature))
            cap.update(x_decentered=enc.x_decentered.detach().clone(), centers=enc.centers.detach().clone())
            enc.zero_grad()
            seg.zero_grad()
            loss = CrossEntropyLossSeg()(score, cu(g["seg"]))
            cap["masks"] = _relu_masks_of(loss, enc, seg=seg)
            loss.backward()
        torch.cuda.synchronize()
    finally:
        torch.bmm = orig_bmm
        ops.POINTMLP_PRECISION = old
    mine = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
    mine.update({"seg." + k: p.grad for k, p in seg.named_parameters() if p.grad is not None})
    after = _running(enc, seg)
    dead = sum(1 for m in (enc, seg) for p in m.parameters() if p.grad is None)
    return dict(loss=loss.detach(), score=score.detach(), mine=mine, cap=cap, names=set(n for n, _, _ in rec.records), bmm=bmm, enc=enc,
                seg=seg, running={k: (before[k], after[k]) for k in before}, dead=dead)


def f64_seg_step(res, g, forced):
    """tests/f64_segmenter.py on the GPU in float64, fed the run's SOM stage (original column order); ``forced``: its pool positions and
    ReLU patterns too."""
    import f64_classifier as F64
    import f64_segmenter as S64
    cap = res["cap"]
    assert "x_aug" in cap, "the training forward did not go through first_pointnet.forward_pooled"
    stage = dict(x_aug=cap["x_aug"], min_idx=cap["min_idx"], row_max=cap["row_max"], som_node=cap["som_node"], pos0=cap["pos0"])
    route = dict(pool1=cap["pool1"], pool2=cap["pool2"], pool3=cap["pool3"]) if forced else None
    return S64.train_step(F64.leaf_params(res["enc"].state_dict(), DEV), F64.leaf_params(res["seg"].state_dict(), DEV), cu(g["label"]),
                          cu(g["seg"]), cu(g["node_knn_I"]), cu(g["pc"]).double(), cu(g["sn"]).double(), stage=stage, route=route,
                          masks=cap["masks"] if forced else None)


def grad_residuals(res, r):
    """{param: rel-rms of the run's gradient against the twin's} over the parameters with a true gradient."""
    out = {}
    for k, ref in r["grads"].items():
        if float(ref.norm()) / max(1.0, float(ref.numel()) ** 0.5) < 1e-7:        # biases in front of a BatchNorm: the true gradient is 0
            continue
        out[k] = float((res["mine"][k].double() - ref).norm() / ref.norm()) if k in res["mine"] else float("inf")
    return out


def expected_running(res, r):
    """F.batch_norm's momentum update (0.1, unbiased variance) of the twin's batch statistics -> {state-dict key: (expected, got)}."""
    out = {}
    for prefix, (mean, var, n) in r["bn"].items():
        for stat, batch in (("running_mean", mean), ("running_var", var * n / (n - 1))):
            before, after = res["running"][prefix + ".norm." + stat]
            out[prefix + ".norm." + stat] = (0.9 * before.double() + 0.1 * batch, after)
    return out


# ------------------------------------------------------------------------------------------------------------------ (a) forced routing
@pytest.mark.parametrize("case,mode", [(FIXTURE, "h3"), (FIXTURE, "x3"), (FIXTURE, "f32"), ("synthetic_b16_n1024", "h3")])
def test_seg_training_gradients_with_forced_routing(case, mode):
    """Every encoder and segmenter gradient of the segmentation step against the float64 twin with the run's SOM stage, pool positions and
    ten ReLU patterns (six encoder layers, segmenter layers 1-4) forced: loss to 1e-5, scores to 1e-4, every gradient (whole tensors) to
    SEG_FORCED_TOL rel-rms, the running statistics the twin's batch statistics through the momentum update to 1e-5."""
    g = _inputs(case)
    res = run_seg_step(g, mode)
    cap = res["cap"]
    B, N = int(g["B"]), int(g["N"])
    assert sorted(cap["masks"]) == sorted(ENC_LAYERS + SEG_LAYERS), sorted(cap["masks"])
    assert cap["pos0"] is None and cap["need_dense"] is True
    assert cap["pool1"].shape == (B, 384, 64) and cap["pool2"].shape == (B, 512, 64) and cap["pool3"].shape == (B, 1024)
    r = f64_seg_step(res, g, forced=True)
    # the per-point attributes the head read are the stage's (x_decentered) and the node coordinates at every copy's node (centers)
    assert torch.equal(res["cap"]["x_decentered"], cap["x_aug"][:, :3])
    assert torch.equal(res["cap"]["centers"], cap["som_node"].gather(2, cap["min_idx"].long().unsqueeze(1).expand(B, 3, -1)))
    assert abs(float(res["loss"]) - float(r["loss"])) <= 1e-5 * abs(float(r["loss"])), (float(res["loss"]), float(r["loss"]))
    assert_close_rms(res["score"].cpu().numpy(), r["score"].cpu().numpy(), 1e-4, "score, same routing")
    rel = grad_residuals(res, r)
    worst = max(rel.items(), key=lambda kv: kv[1])
    print("seg forced routing %s %s: worst gradient %s %.3e (T %.0e)" % (case, mode, worst[0], worst[1], SEG_FORCED_TOL))
    # (20 encoder tensors, 14 head tensors; the biases in front of a BatchNorm -- and the biases of first_pointnet.layers.3 and
    #  final_pointnet.layers.1, whose consumers all end in a BatchNorm -- have no true gradient)
    assert len(rel) == 34 and {"seg.layer%d.conv.weight" % i for i in range(1, 6)} <= set(rel), sorted(rel)
    assert worst[1] <= SEG_FORCED_TOL, sorted(rel.items(), key=lambda kv: -kv[1])[:6]
    assert res["dead"] == int(g["dead_grad_count"])
    run = expected_running(res, r)
    assert len(run) == 2 * 10, sorted(run)
    for k, (want, got) in run.items():
        assert_close_rms(got.cpu().numpy(), want.cpu().numpy(), 1e-5, "running stat " + k)


# ------------------------------------------------------------------------------------------------------------------ (b) free routing
@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_seg_training_step_golden(mode):
    """The segmentation step (train-mode BatchNorm, backward, the two Adam steps) against the reference's Model.optimize (fixture), with
    the routing free: loss to 1e-4, the run's decisions against a float64 run on the same stage (pool flips <= 8, ReLU disagreement <=
    1e-4 per layer), sampled gradients to 2e-2 of the reference's float64 gradients, running statistics to 1e-4, the Adam update."""
    g = golden(FIXTURE)
    res = run_seg_step(g, mode)
    cap, enc, seg = res["cap"], res["enc"], res["seg"]
    assert abs(float(res["loss"]) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    free = f64_seg_step(res, g, forced=False)
    flips1 = int((free["route"]["pool1"] != cap["pool1"]).sum())
    flips2 = int((free["route"]["pool2"] != cap["pool2"]).sum())
    assert flips1 <= 8 and flips2 <= 8, (flips1, flips2)
    assert sorted(cap["masks"]) == sorted(free["masks"])
    for layer, m in cap["masks"].items():
        diff = float((free["masks"][layer].reshape(m.shape) != m).float().mean())
        assert diff <= 1e-4, (layer, diff)
    n = int(g["sub_n"])

    def sub(t):
        f = t.detach().flatten()
        return f[::max(1, f.numel() // n)].cpu().numpy().astype(np.float64)

    def rel_rms(a, r):
        return float(np.sqrt(np.mean((a - r) ** 2)) / np.sqrt(np.mean(r ** 2)))
    params = {k: p for k, p in enc.named_parameters()}
    params.update({"seg." + k: p for k, p in seg.named_parameters()})
    checked = 0
    for k in [k[7:] for k in g.files if k.startswith("grad64/")]:
        truth = g["grad64/" + k].astype(np.float64)
        if np.sqrt(np.mean(truth ** 2)) < 1e-5:        # biases in front of a BatchNorm: true gradient is 0
            continue
        mine = rel_rms(sub(params[k].grad), truth)
        assert mine <= 2e-2, (k, mine, float(g["ref32_dev/" + k]), flips1, flips2)
        checked += 1
    assert checked >= 20, checked
    assert res["dead"] == int(g["dead_grad_count"])
    sd = {k: v for k, v in enc.state_dict().items()}
    sd.update({"seg." + k: v for k, v in seg.state_dict().items()})
    for k in [k[3:] for k in g.files if k.startswith("bn/")]:
        assert_close_rms(sd[k].cpu().numpy(), g["bn/" + k], 1e-4, "running stat " + k)
    torch.optim.Adam(enc.parameters(), lr=0.001, betas=(0.9, 0.999), weight_decay=0).step()
    torch.optim.Adam(seg.parameters(), lr=0.001, betas=(0.9, 0.999), weight_decay=0).step()
    # first Adam step = -lr * sign(grad) per element: 95 % of the well-conditioned conv weights' elements match the reference update
    adam = 0
    for k in [k[6:] for k in g.files if k.startswith("after/")]:
        if np.sqrt(np.mean(g["grad64/" + k].astype(np.float64) ** 2)) < 1e-5 or not k.endswith("conv.weight"):
            continue
        got, ref = sub(params[k]), g["after/" + k].astype(np.float64)
        assert np.mean(np.abs(got - ref) <= 1e-4 * np.maximum(np.abs(ref), 1e-2)) >= 0.95, k
        adam += 1
    assert adam >= 10, adam


# ------------------------------------------------------------------------------------------------------------------ (c) kernels
def _ceil_pad(ci):
    """models/layers.py _pack_transposed: the split-operand dgrad pads its output rows to 32 (and an odd tile count >= 256 rows to 128)."""
    if ci % 32 == 0 or ci <= 32:
        return ci
    cp = (ci + 31) // 32 * 32
    return (ci + 127) // 128 * 128 if (cp // 32) % 2 == 1 and cp >= 256 else cp


@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_seg_training_step_runs_the_project_kernels(mode):
    """Segmenter layers 1-4 run forward, input gradient and weight gradient on the project's point-wise kernels; the encoder takes the
    dense first_pn_out branch (original column order, index_max on the stored tensor, dense input gradient of the last layer; no
    node-sorted pool, no sparse pooled dgrad); layer 5 (Cout = 50: no 32-row tiles, ``x3_supported`` fails) runs its forward on the
    exact-f32 point-wise kernel, its input gradient on the split-operand kernel in the f32-class modes (the transposed problem, 128
    output rows, has the tiles) and on the exact-f32 one in f32 mode, its 50 x 128 weight gradient on one batched library GEMM
    (``torch.bmm``: hipBLASLt, which ``kernel_timing`` does not see -- the test records the call itself).  In f32 mode the weight
    gradients of layers 1-4 are that GEMM too (models/layers.py ``_wgrad``: the split-operand kernel serves the f32-class modes)."""
    g = golden(FIXTURE)
    res = run_seg_step(g, mode)
    names, cap = res["names"], res["cap"]
    B, N = int(g["B"]), int(g["N"])
    fam = {"h3": "(h3|x3)", "x3": "x3", "f32": ""}[mode]        # (h3: the range guard may send a layer to x3)
    dfam = {"h3": "x3", "x3": "x3", "f32": ""}[mode]            # input gradients: bf16 pieces in both f32-class modes

    def ran(pattern):
        rx = re.compile(pattern)
        return any(rx.fullmatch(n) for n in names)
    for i, (cin, cout) in enumerate(SEG_SHAPES[:4]):
        L = 3 * N if i < 3 else N
        assert ran(r"pointmlp%s(_stats)?_%dx%d_L%d" % (fam, cin, cout, L)), ("forward", i + 1, sorted(names))
        cp = _ceil_pad(cin) if mode != "f32" else cin
        if mode == "f32" and cin > 1024:               # (the exact-f32 input gradient: one launch per 1024 output rows, models/layers.py)
            assert ran(r"pointmlp_%dx1024_L%d" % (cout, L)) and ran(r"pointmlp_%dx%d_L%d" % (cout, cin % 1024, L)), sorted(names)
        else:
            assert ran(r"pointmlp%s(_bnba?s?)?_%dx%d_L%d" % (dfam, cout, cp, L)), ("input gradient", i + 1, sorted(names))
        if mode != "f32":
            assert ran(r"wgradx3_%dx%d_L%d" % (cout, cin, L)), ("weight gradient", i + 1, sorted(names))
        else:
            assert ((B, cout, L), (B, L, cin)) in res["bmm"], ("weight gradient", i + 1, res["bmm"])
    # layer 5
    assert ran(r"pointmlp_128x50_L%d" % N) and not ran(r"pointmlp(h3|x3)\w*_128x50_L%d" % N), sorted(names)
    assert ran(r"pointmlp%s_50x128_L%d" % (dfam, N)), sorted(names)
    assert not ran(r"wgradx3_50x128_L\d+") and ((B, 50, N), (B, N, 128)) in res["bmm"], res["bmm"]
    # the three back-broadcast gathers: the project's gather and its fixed-order backward
    assert {"node_gather", "node_gather_bwd"} <= names, sorted(names)
    # the encoder's dense branch
    assert cap["need_dense"] is True and cap["pos0"] is None
    assert "index_max_gather" in names and not any(n.startswith(("pooled_dgrad", "pooled_wgrad", "som_sort_group", "pointmlph3_segpool"))
                                                   for n in names), sorted(names)
    assert ran(r"pointmlp%s_384x(64|256)_L%d" % (dfam, 3 * N)), sorted(names)      # the last first-PointNet layer's dense input gradient


# ------------------------------------------------------------------------------------------------------------------ (d), (e)
def _same_step(a, b, what):
    assert torch.equal(a["score"], b["score"]), what
    assert torch.equal(a["loss"], b["loss"]), (what, float(a["loss"]), float(b["loss"]))
    for k in a["running"]:
        assert torch.equal(a["running"][k][1], b["running"][k][1]), (what, k)
    assert sorted(a["mine"]) == sorted(b["mine"]), what
    for k in a["mine"]:
        assert torch.equal(a["mine"][k], b["mine"][k]), (what, k, float((a["mine"][k] - b["mine"][k]).abs().max()))


@pytest.mark.parametrize("mode", ["h3", "f32"])
def test_seg_training_reference_model_data_flow_is_bit_identical(mode):
    """models/segmenter.py's Model "trains unchanged" (INTEGRATION.md): its forward -- want_first_pn_out left unset with a Segmenter
    alive, the mask argmax, three torch.gather calls, segmenter(...) called directly -- gives the loss, the scores, the running statistics
    and every gradient of the segmentation_forward step bit for bit.  Both run under ``torch.use_deterministic_algorithms``: torch.gather's
    backward is an atomic scatter-add otherwise (its sum of a node's copies changes from run to run); the deterministic one sums them in
    ascending column order, as ``ops.node_gather_bwd`` does."""
    g = golden(FIXTURE)
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        a = run_seg_step(g, mode)
        b = run_seg_step(g, mode, data_flow="reference_model")
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert a["cap"]["need_dense"] is True and b["cap"]["need_dense"] is True
    _same_step(a, b, "reference data flow")


@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_seg_training_step_is_bit_reproducible(mode):
    """Two identical segmentation steps from the same state: bit-identical loss, scores, gradients and running statistics (DESIGN.md:
    training is bit-reproducible)."""
    g = golden(FIXTURE)
    _same_step(run_seg_step(g, mode), run_seg_step(g, mode), "second run")


def test_node_gather_backward_vs_float64_and_reproducible():
    """ops.node_gather_autograd: the forward is torch.gather's, the backward is every node's copies summed in ascending column order --
    f32 to 1e-6 of float64, bit-identical on a second call; nodes without a copy get 0."""
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(3)
    for B, C, M, L in [(3, 384, 64, 3072), (2, 5, 7, 13), (1, 1024, 64, 15000), (2, 16, 1024, 9000)]:
        feat = torch.randn(B, C, M, generator=gen)
        ids = torch.randint(0, M - 1, (B, L), generator=gen, dtype=torch.int32)             # node M-1 stays empty
        gy = torch.randn(B, C, L, generator=gen)
        f = feat.to(DEV).requires_grad_(True)
        out = ops.node_gather_autograd(f, ids.to(DEV))
        assert torch.equal(out.detach().cpu(), torch.gather(feat, 2, ids.long().unsqueeze(1).expand(B, C, L)))
        g1 = torch.autograd.grad(out, f, gy.to(DEV))[0]
        g2 = torch.autograd.grad(ops.node_gather_autograd(f, ids.to(DEV)), f, gy.to(DEV))[0]
        assert torch.equal(g1, g2)
        ref = torch.zeros(B, C, M, dtype=torch.float64).scatter_add_(2, ids.long().unsqueeze(1).expand(B, C, L), gy.double())
        assert float((g1.cpu().double() - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))
        assert float(g1[:, :, M - 1].abs().max()) == 0.0
