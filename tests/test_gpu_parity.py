"""GPU parity tests: the HIP path (through the C ABI, via the python mirror of the reference API)
against the golden fixtures of the live reference and against the CPU oracle on seeded inputs.

Integer / index outputs: bit-exact.  Float outputs: |got-ref| <= 1e-5 * max(|ref|, rms(ref))
(BASELINE.json north_star tolerance, metric of SURVEY.md section 7 hard part 4)."""
import glob
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_close_rms, golden
from train_step_helpers import _capture_stage, _f64_step, _lastdim_max_node, _relu_masks_of, _routing_of  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def test_library_loaded_and_device_is_gfx950():
    from sonet_hip import _lib
    lib = _lib.load()
    assert lib.sonet_abi_version() == 1
    assert lib.sonet_build_arch() == b"gfx950"
    _lib.require_device(torch.device(DEV))
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


# ------------------------------------------------------------------------------------------ index_max
INDEX_MAX_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "index_max_*.npz")))


@pytest.mark.parametrize("case", INDEX_MAX_CASES)
def test_index_max_golden(case):
    import index_max
    g = golden(case)
    K = int(g["K"])
    data, index = cu(g["data"]), cu(g["index"])
    out = index_max.forward_cuda(data, index, K)
    assert out.dtype == torch.int32 and out.device == data.device and tuple(out.shape) == g["out"].shape
    np.testing.assert_array_equal(out.cpu().numpy(), g["out"])
    np.testing.assert_array_equal(index_max.forward_cuda_shared_mem(data, index, K).cpu().numpy(), g["out"])
    # CPU-tensor entry points keep the reference signature (staged through the GPU)
    np.testing.assert_array_equal(index_max.forward_cpu(torch.from_numpy(g["data"]), torch.from_numpy(g["index"]), K).numpy(),
                                  g["out"])
    np.testing.assert_array_equal(index_max.forward_multi_thread_cpu(torch.from_numpy(g["data"]),
                                                                     torch.from_numpy(g["index"]), K, 4).numpy(), g["out"])


@pytest.mark.parametrize("shape", [(8, 384, 15000, 64), (4, 384, 3072, 64), (3, 30, 1023, 64), (2, 7, 4097, 100),
                                   (1, 64, 20000, 1024)])
def test_index_max_vs_oracle_random(shape):
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    B, C, N, K = shape
    g = torch.Generator().manual_seed(B * 1000 + C)
    data = torch.randn(B, C, N, generator=g)
    index = torch.randint(0, K, (B, N), generator=g, dtype=torch.int32)
    ref = O.index_max(data.numpy(), index.numpy(), K)
    out = ops.index_max(data.to(DEV), index.to(DEV), K)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    # gather variant: positions identical, values = data at (position * row_max)
    row_max = (torch.bincount(index[0].long(), minlength=K) > 0)
    row_max = torch.stack([(torch.bincount(index[b].long(), minlength=K) > 0) for b in range(B)]).to(torch.int32)
    idx, val = ops.index_max_gather(data.to(DEV), index.to(DEV), K, row_max.to(DEV))
    np.testing.assert_array_equal(idx.cpu().numpy(), ref)
    exp = torch.gather(data, 2, torch.from_numpy(ref).long() * row_max.unsqueeze(1).long())
    np.testing.assert_array_equal(val.cpu().numpy(), exp.numpy())


def test_index_max_bf16_ties():
    """bf16 features make exact ties common: the tie rule (smallest n) is load-bearing."""
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    g = torch.Generator().manual_seed(5)
    data = torch.randn(4, 48, 6000, generator=g).to(torch.bfloat16)
    index = torch.randint(0, 64, (4, 6000), generator=g, dtype=torch.int32)
    ref = O.index_max(data.float().numpy(), index.numpy(), 64)
    out = ops.index_max(data.to(DEV), index.to(DEV), 64)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)


def test_index_max_error_behaviour():
    import index_max
    data = torch.randn(2, 4, 64)
    index = torch.zeros(2, 64, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        index_max.forward_cuda(data, index.to(DEV), 8)                       # CHECK_CUDA
    with pytest.raises(RuntimeError, match="contiguous"):
        index_max.forward_cuda(data.to(DEV).transpose(1, 2), index.to(DEV), 8)   # CHECK_CONTIGUOUS
    with pytest.raises(RuntimeError):
        index_max.forward_cuda(data.to(DEV), index.to(DEV).long(), 8)


# ------------------------------------------------------------------------------------------ SOM assignment
@pytest.mark.parametrize("case", ["query_topk_a", "query_topk_b", "query_topk_c"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_query_topk_golden(case, k):
    from util import som
    g = golden(case)
    x, node = cu(g["x"]), cu(g["node"])
    B, _, N = x.shape
    M = node.shape[2]
    rows = int(round(M ** 0.5))
    bs = som.BatchSOM(rows, rows, 3, 0, B)
    bs.node.resize_(node.size()).copy_(node)                                  # as models/networks.py:124 does
    mask, mask_row_max, min_idx = bs.query_topk(x, k)
    assert mask.dtype == torch.int32 and mask_row_max.dtype == torch.int32 and min_idx.dtype == torch.int64
    assert tuple(mask.shape) == (B, k * N, M) and tuple(min_idx.shape) == (B, k * N)
    np.testing.assert_array_equal(min_idx.cpu().numpy(), g["min_idx_sorted_k%d" % k])        # canonical order: exact
    ref_u = np.sort(g["min_idx_unsorted_k%d" % k].reshape(B, k, N), axis=1)                   # reference as-is: same sets
    np.testing.assert_array_equal(np.sort(min_idx.cpu().numpy().reshape(B, k, N), axis=1), ref_u)
    np.testing.assert_array_equal(mask_row_max.cpu().numpy(), g["mask_row_max_k%d" % k])
    np.testing.assert_array_equal(mask.sum(1).cpu().numpy(), g["mask_row_sum_k%d" % k])
    np.testing.assert_array_equal(mask.argmax(dim=2).cpu().numpy(), g["min_idx_sorted_k%d" % k])
    if k == 1:
        fmask, frow = bs.query(x)
        assert fmask.dtype == torch.float32
        np.testing.assert_array_equal(fmask.argmax(dim=2).cpu().numpy(), g["min_idx_sorted_k1"])


@pytest.mark.parametrize("B,N,M,k", [(64, 5000, 64, 3), (3, 777, 16, 2), (2, 1, 64, 1), (1, 300, 256, 4)])
def test_som_assign_and_group_vs_oracle(B, N, M, k):
    from oracle import cpu_oracle as O
    from sonet_hip import ops, synth
    inp = synth.make_inputs(B, N, M=M, som_k=min(9, M), seed=N + M, node_kind="uniform" if N < M else "som")
    a = ops.som_assign(inp["pc"].to(DEV), inp["node"].to(DEV), k, want_i64=True)
    ref_idx, ref_cnt, ref_rm = O.som_query_topk(inp["pc"].numpy(), inp["node"].numpy(), k)
    np.testing.assert_array_equal(a.min_idx_i64.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(a.min_idx_i32.cpu().numpy(), ref_idx.astype(np.int32))
    np.testing.assert_array_equal(a.count.cpu().numpy(), ref_cnt)
    g = ops.som_group(inp["pc"].to(DEV), inp["sn"].to(DEV), a, want_centers=True, want_decentered=True, want_augmented=True)
    node_ref, ctr_ref, xd_ref = O.som_group(inp["pc"].numpy(), ref_idx, M, k)
    np.testing.assert_array_equal(g["row_max"].cpu().numpy(), ref_rm)
    assert_close_rms(g["som_node"].cpu().numpy(), node_ref, 1e-6, "som_node")
    assert_close_rms(g["centers"].cpu().numpy(), ctr_ref, 1e-6, "centers")
    assert_close_rms(g["x_decentered"].cpu().numpy(), xd_ref, 1e-6, "x_decentered")
    aug = g["x_augmented"].cpu()
    np.testing.assert_array_equal(aug[:, :3].numpy(), g["x_decentered"].cpu().numpy())
    np.testing.assert_array_equal(aug[:, 3:].numpy(), torch.cat([inp["sn"]] * k, dim=2).numpy())
    # run-to-run reproducibility of the f64-accumulated means
    a2 = ops.som_assign(inp["pc"].to(DEV), inp["node"].to(DEV), k)
    g2 = ops.som_group(inp["pc"].to(DEV), None, a2)
    np.testing.assert_array_equal(g2["som_node"].cpu().numpy(), g["som_node"].cpu().numpy())


def test_knn_gather_vs_oracle():
    from models import operations
    from oracle import cpu_oracle as O
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 387, 64, generator=g)
    I = torch.randint(0, 64, (5, 64, 9), generator=g)
    out = operations.knn_gather_by_indexing(x.to(DEV), I.to(DEV))
    np.testing.assert_array_equal(out.cpu().numpy(), O.knn_gather(x.numpy(), I.numpy()))
    out3 = operations.knn_gather_wrapper(x[:, :3].contiguous().to(DEV), I.to(DEV))
    np.testing.assert_array_equal(out3.cpu().numpy(), O.knn_gather(x[:, :3].numpy(), I.numpy()))


def test_chamfer_nn_vs_oracle():
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    g = torch.Generator().manual_seed(4)
    q = torch.rand(3, 3, 1280, generator=g) * 2 - 1
    db = torch.rand(3, 3, 5000, generator=g) * 2 - 1
    np.testing.assert_array_equal(ops.chamfer_nn(q.to(DEV), db.to(DEV)).cpu().numpy(), O.chamfer_nn(q.numpy(), db.numpy()))
    np.testing.assert_array_equal(ops.chamfer_nn(db.to(DEV), q.to(DEV)).cpu().numpy(), O.chamfer_nn(db.numpy(), q.numpy()))


# ------------------------------------------------------------------------------------------ pointmlp
@pytest.mark.parametrize("B,C1,C2,Cout,L,bn,relu", [
    (2, 6, 0, 64, 300, True, True), (2, 64, 0, 128, 768, True, True), (1, 64, 256, 384, 1000, False, False),
    (3, 387, 0, 512, 576, True, True), (4, 515, 0, 768, 64, True, True), (2, 768, 0, 1024, 64, False, False),
    (2, 128, 0, 50, 77, False, False), (1, 3, 0, 32, 1, True, True)])
def test_pointmlp_vs_oracle(B, C1, C2, Cout, L, bn, relu):
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    g = torch.Generator().manual_seed(C1 + Cout + L)
    Cin = C1 + C2
    x = torch.randn(B, Cin, L, generator=g)
    W = torch.randn(Cout, Cin, generator=g) * (2.0 / Cin) ** 0.5
    bias = torch.rand(Cout, generator=g) * 0.2 - 0.1
    if bn:
        gamma, beta = 0.5 + torch.rand(Cout, generator=g), torch.rand(Cout, generator=g) * 0.4 - 0.2
        mean, var = 0.2 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g)
        scale = gamma / torch.sqrt(var + 1e-5)
        shift = (bias - mean) * scale + beta
        ref = O.pointwise_layer(x.numpy(), W.numpy(), bias.numpy(), bn=(gamma.numpy(), beta.numpy(), mean.numpy(), var.numpy()),
                                relu=relu)
    else:
        scale, shift = torch.ones(Cout), bias
        ref = O.pointwise_layer(x.numpy(), W.numpy(), bias.numpy(), bn=None, relu=relu)
    wp = ops.pointmlp_pack(W.to(DEV))
    x1 = x[:, :C1].contiguous().to(DEV)
    x2 = x[:, C1:].contiguous().to(DEV) if C2 else None
    y = ops.pointmlp(x1, wp, scale.to(DEV), shift.to(DEV), relu, Cout, x2=x2)
    assert_close_rms(y.cpu().numpy(), ref, 1e-5, "pointmlp")


def test_channel_stats_and_affine():
    from sonet_hip import ops
    g = torch.Generator().manual_seed(9)
    y = torch.randn(3, 70, 1234, generator=g) * 3 + 1
    mean, var = ops.channel_stats(y.to(DEV))
    y64 = y.double()
    assert_close_rms(mean.cpu().numpy(), y64.mean(dim=(0, 2)).numpy(), 1e-6, "mean")
    assert_close_rms(var.cpu().numpy(), y64.var(dim=(0, 2), unbiased=False).numpy(), 1e-6, "var")
    sc, sh = torch.rand(70, generator=g), torch.randn(70, generator=g)
    out = ops.channel_affine_act_(y.to(DEV).clone(), sc.to(DEV), sh.to(DEV), True)
    assert_close_rms(out.cpu().numpy(), torch.relu(y * sc.view(1, -1, 1) + sh.view(1, -1, 1)).numpy(), 1e-6, "affine")


# ------------------------------------------------------------------------------------------ layers (golden)
def test_equivariant_layer_eval_and_train_golden():
    from models import layers as L
    from sonet_hip import synth
    g = golden("layers")
    x = cu(g["eq_x"])
    layer = L.EquivariantLayer(6, 64, "relu", "batch", 0.1, None, 1)
    synth.fill_state_dict_(layer.state_dict(), seed=5)
    layer.to(DEV).eval()
    with torch.no_grad():
        assert_close_rms(layer(x).cpu().numpy(), g["eq_eval_y"], 1e-5, "eval y")
    layer.train()
    y = layer(x, epoch=None)
    assert_close_rms(y.detach().cpu().numpy(), g["eq_train_y"], 1e-5, "train y")
    assert_close_rms(layer.norm.running_mean.cpu().numpy(), g["eq_train_running_mean"], 1e-5, "running_mean")
    assert_close_rms(layer.norm.running_var.cpu().numpy(), g["eq_train_running_var"], 1e-5, "running_var")
    assert int(layer.norm.num_batches_tracked) == int(g["eq_train_num_batches_tracked"])
    # backward (fresh statistics, same weights)
    layer2 = L.EquivariantLayer(6, 64, "relu", "batch", 0.1, None, 1)
    synth.fill_state_dict_(layer2.state_dict(), seed=5)
    layer2.to(DEV).train()
    xg = x.clone().requires_grad_(True)
    layer2(xg).backward(cu(g["eq_gy"]))
    assert_close_rms(xg.grad.cpu().numpy(), g["eq_train_gx"], 1e-4, "gx")
    assert_close_rms(layer2.conv.weight.grad.cpu().numpy(), g["eq_train_gw"], 1e-4, "gw")
    assert_close_rms(layer2.norm.weight.grad.cpu().numpy(), g["eq_train_ggamma"], 1e-4, "ggamma")
    assert_close_rms(layer2.norm.bias.grad.cpu().numpy(), g["eq_train_gbeta"], 1e-4, "gbeta")
    # momentum decay rule (models/layers.py:60-65)
    layer3 = L.EquivariantLayer(6, 64, "relu", "batch", 0.5, 2, 0.6)
    synth.fill_state_dict_(layer3.state_dict(), seed=6)
    layer3.to(DEV).train()
    layer3(x, epoch=5)
    assert abs(layer3.norm.momentum - float(g["eq_decay_momentum"])) < 1e-12
    assert_close_rms(layer3.norm.running_mean.cpu().numpy(), g["eq_decay_running_mean"], 1e-5, "decayed running_mean")


def test_point_resnet_eval_golden():
    from models import layers as L
    from sonet_hip import synth
    g = golden("layers")
    pr = L.PointResNet(6, [64, 128, 256, 384], "relu", "batch", 0.1, None, 1)
    synth.fill_state_dict_(pr.state_dict(), seed=7)
    pr.to(DEV).eval()
    with torch.no_grad():
        y = pr(cu(g["eq_x"]))
    assert_close_rms(y[:, ::8].cpu().numpy(), g["prn_eval_y"], 1e-5, "PointResNet eval")


# ------------------------------------------------------------------------------------------ encoder + classifier (golden)
def make_opt(g, B, N):
    return Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True,
                     feature_num=1024, activation="relu", normalization="batch", dropout=0.7, node_num=64,
                     k=int(g["k"]), som_k=int(g["som_k"]), som_k_type=str(g["som_k_type"]), bn_momentum=0.1,
                     bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)


@pytest.mark.parametrize("case", ["classifier_b2_n256", "classifier_b8_n1024", "classifier_b2_n5000",
                                  "classifier_b2_n300_k1_center"])
def test_encoder_classifier_forward_golden(case):
    from models import networks as NW
    from sonet_hip import synth
    g = golden(case)
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = make_opt(g, B, N)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), seed)
    synth.fill_state_dict_(cls.state_dict(), seed + 1)
    enc.to(DEV).eval()
    cls.to(DEV).eval()
    with torch.no_grad():
        feat = enc(cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), is_train=False)
        score = cls(feat)
    # integer outputs: bit exact
    np.testing.assert_array_equal(enc.min_idx.cpu().numpy(), g["min_idx"])
    np.testing.assert_array_equal(enc.mask.argmax(dim=2).cpu().numpy(), g["min_idx"])       # models/segmenter.py:90
    np.testing.assert_array_equal(enc.mask.sum(1).cpu().numpy(), g["mask_row_sum"])
    # float outputs
    tol = 1e-5
    assert_close_rms(enc.som_node.cpu().numpy(), g["som_node"], tol, "som_node")
    assert_close_rms(enc.som_builder.node.cpu().numpy(), g["som_node"], tol, "som_builder.node")
    assert_close_rms(enc.centers[:, :, ::7].cpu().numpy(), g["centers"], tol, "centers")
    assert_close_rms(enc.x_decentered[:, :, ::7].cpu().numpy(), g["x_decentered"], tol, "x_decentered")
    assert_close_rms(enc.first_pn_out[:, ::16, ::5].cpu().numpy(), g["first_pn_out_sub"], tol, "first_pn_out")
    assert_close_rms(enc.first_pn_out_masked_max.cpu().numpy(), g["first_pn_out_masked_max"], tol, "masked_max")
    assert_close_rms(enc.knn_center_1.cpu().numpy(), g["knn_center_1"], tol, "knn_center_1")
    assert_close_rms(enc.knn_feature_1[:, ::4].cpu().numpy(), g["knn_feature_1"], tol, "knn_feature_1")
    assert_close_rms(enc.final_pn_out[:, ::4].cpu().numpy(), g["final_pn_out"], tol, "final_pn_out")
    assert_close_rms(feat.cpu().numpy(), g["feature"], tol, "feature")
    assert_close_rms(score.cpu().numpy(), g["score"], tol, "score")


def test_graphed_forward_equals_eager():
    """HIP-graph replay of the classifier forward is bit-identical to the eager launch sequence."""
    from models import networks as NW
    from sonet_hip import synth
    from sonet_hip.graph import GraphedForward
    g = golden("classifier_b8_n1024")
    opt = make_opt(g, 8, 1024)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), 3)
    synth.fill_state_dict_(cls.state_dict(), 4)
    enc.to(DEV).eval()
    cls.to(DEV).eval()
    args = (cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]))
    with torch.no_grad():
        eager = cls(enc(*args)).clone()
    fwd = GraphedForward(lambda pc, sn, node, knn: cls(enc(pc, sn, node, knn)), args)
    out1 = fwd(*args).clone()
    # new data through the same graph
    args2 = (args[0].flip(0).contiguous(), args[1].flip(0).contiguous(), args[2].flip(0).contiguous(), args[3].flip(0).contiguous())
    out2 = fwd(*args2).clone()
    with torch.no_grad():
        eager2 = cls(enc(*args2))
    assert torch.equal(out1, eager)
    assert torch.equal(out2, eager2)
    assert torch.equal(out2.flip(0), eager)


# ------------------------------------------------------------------------------------------ 3 x bf16 split path
@pytest.fixture
def x3_mode():
    from sonet_hip import ops
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = "x3"
    yield
    ops.POINTMLP_PRECISION = old


@pytest.mark.parametrize("B,C1,C2,Cout,L,bn,relu", [
    (2, 6, 0, 64, 300, True, True), (2, 64, 0, 128, 768, True, True), (1, 64, 256, 384, 1000, False, False),
    (3, 387, 0, 512, 576, True, True), (4, 515, 0, 768, 64, True, True), (2, 768, 0, 1024, 64, False, False),
    (2, 100, 0, 96, 77, False, True), (1, 3, 0, 32, 1, True, True), (2, 16, 16, 64, 40, False, False)])
@pytest.mark.parametrize("split", ["x3", "h3"])
def test_pointmlp_x3_vs_oracle(B, C1, C2, Cout, L, bn, relu, split):
    """Split-operand MFMA paths (six bf16 terms / three fp16 terms): f32-class accuracy, the exact-f32 path's 1e-5 tolerance."""
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    g = torch.Generator().manual_seed(C1 + Cout + L)
    Cin = C1 + C2
    x = torch.randn(B, Cin, L, generator=g)
    W = torch.randn(Cout, Cin, generator=g) * (2.0 / Cin) ** 0.5
    bias = torch.rand(Cout, generator=g) * 0.2 - 0.1
    if bn:
        gamma, beta = 0.5 + torch.rand(Cout, generator=g), torch.rand(Cout, generator=g) * 0.4 - 0.2
        mean, var = 0.2 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g)
        scale = gamma / torch.sqrt(var + 1e-5)
        shift = (bias - mean) * scale + beta
        ref = O.pointwise_layer(x.numpy(), W.numpy(), bias.numpy(), bn=(gamma.numpy(), beta.numpy(), mean.numpy(), var.numpy()),
                                relu=relu)
    else:
        scale, shift = torch.ones(Cout), bias
        ref = O.pointwise_layer(x.numpy(), W.numpy(), bias.numpy(), bn=None, relu=relu)
    wp = ops.pointmlp_pack(W.to(DEV), split)
    assert wp.dtype == (torch.uint8 if split == "x3" else torch.int8)
    x1 = x[:, :C1].contiguous().to(DEV)
    x2 = x[:, C1:].contiguous().to(DEV) if C2 else None
    y = ops.pointmlp(x1, wp, scale.to(DEV), shift.to(DEV), relu, Cout, x2=x2)
    assert_close_rms(y.cpu().numpy(), ref, 1e-5, "pointmlp " + split)


@pytest.fixture
def f32_mode():
    from sonet_hip import ops
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = "f32"
    yield
    ops.POINTMLP_PRECISION = old


@pytest.mark.parametrize("case", ["classifier_b2_n256", "classifier_b8_n1024", "classifier_b2_n5000",
                                  "classifier_b2_n300_k1_center"])
def test_encoder_classifier_forward_golden_x3(case, x3_mode):
    test_encoder_classifier_forward_golden(case)


@pytest.mark.parametrize("case", ["classifier_b2_n256", "classifier_b8_n1024", "classifier_b2_n5000",
                                  "classifier_b2_n300_k1_center"])
def test_encoder_classifier_forward_golden_exact_f32(case, f32_mode):
    test_encoder_classifier_forward_golden(case)


def test_point_resnet_eval_golden_x3(x3_mode):
    test_point_resnet_eval_golden()


def test_point_resnet_and_layer_golden_exact_f32(f32_mode):
    test_point_resnet_eval_golden()
    test_equivariant_layer_eval_and_train_golden()


def test_pointresnet_fused_vs_layerwise_and_golden():
    """One-kernel first PointNet (register-chained layers) == the four-launch path == the reference fixture."""
    from models import layers as L
    from sonet_hip import ops, synth
    g = golden("layers")
    pr = L.PointResNet(6, [64, 128, 256, 384], "relu", "batch", 0.1, None, 1)
    synth.fill_state_dict_(pr.state_dict(), seed=7)
    pr.to(DEV).eval()
    old = (ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET)
    try:
        ops.POINTMLP_PRECISION = "h3"                  # the fused kernel's arithmetic (x3 never takes the fused kernel)
        for shape in [(2, 6, 300), (3, 6, 15000), (1, 6, 1), (2, 3, 129)]:
            gen = torch.Generator().manual_seed(shape[2])
            x = torch.randn(shape, generator=gen).to(DEV)
            prn = pr if shape[1] == 6 else L.PointResNet(3, [64, 128, 256, 384], "relu", "batch", 0.1, None, 1).to(DEV).eval()
            with torch.no_grad():
                ops.FUSE_POINTRESNET = True
                with ops.kernel_timing() as rec:
                    y_fused = prn(x)
                assert any(n.startswith("pointresnet_fused") for n, _, _ in rec.records), "fused kernel did not run"
                ops.FUSE_POINTRESNET = False
                y_layer = prn(x)
            assert_close_rms(y_fused.cpu().numpy(), y_layer.cpu().numpy(), 1e-5, "fused vs layerwise %s" % (shape,))
        with torch.no_grad():
            ops.FUSE_POINTRESNET = True
            y = pr(cu(g["eq_x"]))
        assert_close_rms(y[:, ::8].cpu().numpy(), g["prn_eval_y"], 1e-5, "fused PointResNet vs reference")
    finally:
        ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET = old


# ------------------------------------------------------------------------------------------ segmenter (config 3)
@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_segmenter_forward_golden(mode, case="segmenter_b2_n256"):
    """Part-segmentation forward (level-2 encoder + back-broadcast gathers + Segmenter head) vs the reference."""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden(case)
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.6, node_num=64, k=3, som_k=9, som_k_type="center",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=50)
    enc, seg = NW.Encoder(opt), NW.Segmenter(opt)
    assert sorted(seg.state_dict().keys()) == [str(k) for k in g["segmenter_keys"]]
    synth.fill_state_dict_(enc.state_dict(), seed)
    synth.fill_state_dict_(seg.state_dict(), seed + 1)
    enc.to(DEV).eval()
    seg.to(DEV).eval()
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = mode
    try:
        with torch.no_grad():
            seg.nodewise = False                      # the reference's data flow: gather to the copies, dense 3356-channel layer
            score_dense = NW.segmentation_forward(enc, seg, cu(g["pc"]), cu(g["sn"]), cu(g["label"]), cu(g["node"]), cu(g["node_knn_I"]))
            seg.nodewise = True                       # per-node / per-cloud blocks of layer 1 computed once per node
            score = NW.segmentation_forward(enc, seg, cu(g["pc"]), cu(g["sn"]), cu(g["label"]), cu(g["node"]), cu(g["node_knn_I"]))
            bb = ops.node_gather(enc.first_pn_out_masked_max.contiguous(), enc._lazy["a"].min_idx_i32)
    finally:
        ops.POINTMLP_PRECISION = old
    assert_close_rms(score_dense.cpu().numpy(), g["score_segmenter"], 1e-5, "score_segmenter (dense layer 1)")
    np.testing.assert_array_equal(enc.min_idx.cpu().numpy(), g["min_idx"])
    assert_close_rms(bb[:, ::8].cpu().numpy(), g["feature_max_first_pn_out"], 1e-5, "back-broadcast")
    assert tuple(score.shape) == (B, 50, N)
    assert_close_rms(score.cpu().numpy(), g["score_segmenter"], 1e-5, "score_segmenter")


# ------------------------------------------------------------------------------------------ autoencoder (config 4)
@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_autoencoder_forward_and_chamfer_golden(mode, case="autoencoder_b2_n1024"):
    """Encoder -> FC + conv decoder -> multi-resolution Chamfer loss (models/autoencoder.py:62-125) vs the reference
    run with an exact flat-L2 search in place of faiss; gradient of the loss w.r.t. the predicted cloud."""
    from models import networks as NW, losses as LS
    from sonet_hip import ops, synth
    g = golden(case)
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40,
                    output_fc_pc_num=256, output_conv_pc_num=1024)
    enc, dec, crit = NW.Encoder(opt), NW.Decoder(opt), LS.ChamferLoss(opt)
    assert sorted(dec.state_dict().keys()) == [str(k) for k in g["decoder_keys"]]
    synth.fill_state_dict_(enc.state_dict(), seed)
    synth.fill_state_dict_(dec.state_dict(), seed + 1)
    enc.to(DEV).eval()
    dec.to(DEV).eval()
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = mode
    try:
        with torch.no_grad():
            feature = enc(cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), False, None)
            pred = dec(feature)
            loss = crit(pred, cu(g["pc"])) + crit(dec.conv_pc4, cu(g["pc"]))      # autoencoder.py:118-122 at 1024 conv points
    finally:
        ops.POINTMLP_PRECISION = old
    assert_close_rms(feature.cpu().numpy(), g["feature"], 1e-5, "feature")
    assert_close_rms(pred.cpu().numpy(), g["predicted_pc"], 1e-5, "predicted_pc")
    assert_close_rms(dec.conv_pc4.cpu().numpy(), g["conv_pc4"], 1e-5, "conv_pc4")
    assert abs(float(loss) - float(g["loss"])) <= 2e-5 * float(g["loss"])
    # the loss itself, on the reference's predicted cloud: values and gradient
    p = cu(g["predicted_pc"]).requires_grad_(True)
    l2 = crit(p, cu(g["pc"]))
    l2.backward()
    assert abs(float(crit.forward_loss.detach()) - float(g["forward_loss"])) <= 2e-6 * float(g["forward_loss"])
    assert abs(float(crit.backward_loss.detach()) - float(g["backward_loss"])) <= 2e-6 * float(g["backward_loss"])
    np.testing.assert_allclose(crit.loss_array.detach().cpu().numpy(), g["loss_array"], rtol=5e-6)
    assert_close_rms(p.grad.cpu().numpy(), g["grad_predicted"], 1e-5, "d loss / d predicted_pc")


def test_chamfer_loss_full_size_properties():
    """Config 4 size (B=8, 1280 predicted vs 5000 gt points): size-independent properties of the loss."""
    from models import losses as LS
    gen = torch.Generator().manual_seed(5)
    gt = (torch.rand(8, 3, 5000, generator=gen) * 2 - 1).to(DEV)
    crit = LS.ChamferLoss(Namespace(gpu_id=0, device=torch.device(DEV)))
    sub = gt[:, :, :1280].clone()
    crit(sub, gt)                                                  # a subset: every predicted point has distance 0
    assert abs(float(crit.forward_loss) - 1e-4) < 1e-7             # sqrt(0 + 1e-8)
    perm = torch.randperm(5000, generator=gen).to(DEV)
    a = float(crit(sub, gt))
    b = float(crit(sub, gt[:, :, perm]))                            # permuting the database changes nothing
    assert abs(a - b) <= 1e-6 * abs(a)
    pred = (torch.rand(8, 3, 1280, generator=gen) * 2 - 1).to(DEV)
    l1 = float(crit(pred, gt))
    d = torch.cdist(pred.transpose(1, 2).double(), gt.transpose(1, 2).double())     # brute force, float64
    ref = (d.min(2).values.pow(2) + 1e-8).sqrt().mean() + (d.min(1).values.pow(2) + 1e-8).sqrt().mean()
    assert abs(l1 - float(ref)) <= 1e-5 * float(ref)


def test_pooled_last_layer_node_dense_and_sparse_branches():
    """The joint (last layer + arg-max pool) autograd node vs the plain data flow (layer, index_max, torch gather):
    gradients when only the pooled output is used (sparse dgrad) and when first_pn_out is used too (dense branch with the
    pooled gradient scatter-added, as the segmenter needs)."""
    from models import networks as NW
    from sonet_hip import synth
    B, N = 4, 600
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)
    inp = synth.make_inputs(B, N, seed=21, device=DEV)
    w_dense = torch.randn(B, 384, 3 * N, generator=torch.Generator().manual_seed(1)).to(DEV)
    grads = {}
    for use_dense in (False, True):
        for joint in (True, False):
            enc = NW.Encoder(opt)
            synth.fill_state_dict_(enc.state_dict(), 5)
            enc.to(DEV).train()
            enc.pooled_backward = joint
            enc.want_first_pn_out = use_dense                         # (a head that reads first_pn_out per point copy says so: the segmenter does)
            feat = enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], True, 0)
            loss = feat.square().mean()
            if use_dense:
                loss = loss + 1e-3 * (enc.first_pn_out * w_dense).mean()
            loss.backward()
            grads[(use_dense, joint)] = {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None}
    for use_dense in (False, True):
        a, b = grads[(use_dense, True)], grads[(use_dense, False)]
        assert a.keys() == b.keys()
        for k in a:
            # (conv biases sit in front of a training-mode BatchNorm -- directly or through the pool -- so their true gradient
            #  is zero and both sides hold rounding noise of ~1e-8)
            if k.startswith("first_pointnet") and not k.endswith("conv.bias"):
                assert_close_rms(a[k].cpu().numpy(), b[k].cpu().numpy(), 2e-5, "%s (dense=%s)" % (k, use_dense))


def test_pooled_dgrad_vs_dense():
    """Sparse W^T.g of the pooled last layer vs scatter_add + dense matmul (float64), incl. duplicate and empty-node positions."""
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(11)
    for B, C, M, C1, C2, L in [(2, 384, 64, 64, 256, 3072), (1, 32, 5, 16, 0, 100), (3, 96, 8, 16, 48, 130), (2, 40, 6, 10, 17, 70), (2, 48, 7, 44, 0, 257)]:
        g = torch.randn(B, C, M, generator=gen)
        pos = torch.randint(0, L, (B, C, M), generator=gen, dtype=torch.int32)
        pos[:, : C // 4, 0] = 0
        pos[:, : C // 8, 1] = 0                                            # duplicates on one column
        pos[:, 0, 2] = -1                                                  # ignored entry
        W = torch.randn(C, C1 + C2, generator=gen) * 0.1
        G = torch.zeros(B, C, L + 1, dtype=torch.float64).scatter_add_(2, torch.where(pos < 0, L, pos).long(), g.double())[:, :, :L]
        ref = torch.matmul(W.double().t().unsqueeze(0), G)
        gx1, gx2 = ops.pooled_dgrad(g.to(DEV), pos.to(DEV), W.to(DEV), C1, C2, L)
        got = torch.cat([gx1.cpu()] + ([gx2.cpu()] if C2 else []), dim=1).double()
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        gx1b, _ = ops.pooled_dgrad(g.to(DEV), pos.to(DEV), W.to(DEV), C1, C2, L)
        assert torch.equal(gx1b, gx1)                                      # deterministic


@pytest.mark.parametrize("B,C,N,k", [(2, 256, 1024, 3), (3, 7, 333, 3), (2, 16, 130, 2), (1, 5, 8, 1), (64, 256, 1024, 3)])
def test_chunk_mean_is_the_reference_expression_bit_for_bit(B, C, N, k):
    """sonet_chunk_mean_f32 == (1/3) * (h0 + h1 + h2) / 0.5 * (h0 + h1) of models/networks.py:331-336 as aten evaluates it."""
    from sonet_hip import ops
    g = torch.Generator().manual_seed(B + C + N + k)
    h = torch.randn(B, C, k * N, generator=g).to(DEV)
    got = ops.chunk_mean(h, k)
    parts = torch.split(h, N, dim=2)
    ref = parts[0] if k == 1 else 0.5 * (parts[0] + parts[1]) if k == 2 else (1.0 / 3.0) * (parts[0] + parts[1] + parts[2])
    assert tuple(got.shape) == (B, C, N) and torch.equal(got, ref)


@pytest.mark.parametrize("B,C,M,C1,C2,L", [(3, 384, 64, 64, 256, 3000), (2, 96, 8, 16, 48, 130), (2, 64, 16, 64, 0, 514), (64, 384, 64, 64, 256, 15000)])
def test_pooled_dgrad_on_the_matrix_cores(B, C, M, C1, C2, L):
    """sonet_pooled_dgrad_mfma_bf16 (the tile of the never-built gradient assembled in LDS, times W^T on bf16 MFMAs) against scatter_add +
    dense matmul in float64 on the bf16-rounded operands: within bf16 output rounding; bit-identical run to run when the positions of a
    (cloud, channel) row are distinct (the arg-max positions of different nodes are); a repeated (channel, column) pair adds up."""
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(B + C + L)
    g = torch.randn(B, C, M, generator=gen)
    pos = (torch.arange(M).view(1, 1, M) * (L // M) + torch.randint(0, L // M, (B, C, M), generator=gen)).to(torch.int32)
    pos[:, 0, 2] = -1                                                  # ignored entry
    W = torch.randn(C, C1 + C2, generator=gen) * 0.1
    wt = W.t().contiguous()
    if wt.shape[0] % 32:
        wt = torch.cat((wt, wt.new_zeros(32 - wt.shape[0] % 32, C)), dim=0)
    wtp = ops.pointmlp_pack(wt.to(DEV), "bf16")
    assert ops.pooled_dgrad_mfma_ok(C, C1, C2, L)

    def run(p):
        gx1, gx2 = ops.pooled_dgrad(g.to(DEV), p.to(DEV), W.to(DEV), C1, C2, L, out_dtype=torch.bfloat16, wt_pack=wtp)
        return torch.cat([gx1] + ([gx2] if C2 else []), dim=1)

    def ref(p):
        dev = DEV if B * C * L > 5e7 else "cpu"
        gb, Wb = g.to(torch.bfloat16).double().to(dev), W.to(torch.bfloat16).double().to(dev)
        out = []
        for b0 in range(0, B, 8):                                       # float64 on the GPU in slices (the benchmark shape)
            pp = p[b0:b0 + 8].to(dev)
            G = torch.zeros(pp.shape[0], C, L + 1, dtype=torch.float64, device=dev).scatter_add_(2, torch.where(pp < 0, L, pp).long(), gb[b0:b0 + 8])[:, :, :L]
            out.append(torch.matmul(Wb.t().unsqueeze(0), G).cpu())
        return torch.cat(out, dim=0)

    got, want = run(pos), ref(pos)
    err = (got.cpu().double() - want).abs()
    assert bool((err <= want.abs() * 2.0 ** -8 + 1e-6 * float(want.abs().max())).all()), float(err.max())
    assert torch.equal(run(pos), got)
    if B <= 3:
        dup = pos.clone()
        dup[:, : C // 4, 1] = dup[:, : C // 4, 0]                        # the same (channel, column) twice: the two gradients add (bf16 sum)
        got, want = run(dup), ref(dup)
        assert float((got.cpu().double() - want).abs().max()) <= 2.0 ** -6 * float(want.abs().max())


@pytest.mark.parametrize("node_num,sn,k,N", [(16, True, 3, 700), (64, False, 3, 900), (36, True, 2, 333), (16, False, 1, 257)])
def test_encoder_other_configs_fast_path_vs_exact_path(node_num, sn, k, N):
    """Configurations the reference fixtures do not cover (other SOM sizes, no surface normals, other k): the default
    path (fused kernel / fp16-split arithmetic / pooled epilogue) against the exact-f32 layer-wise path of the same
    encoder -- two independent implementations of the same forward."""
    from models import networks as NW
    from sonet_hip import ops, synth
    B = 3
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=sn, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.7, node_num=node_num, k=k, som_k=5, som_k_type="avg",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)
    enc = NW.Encoder(opt)
    synth.fill_state_dict_(enc.state_dict(), 31)
    enc.to(DEV).eval()
    inp = synth.make_inputs(B, N, M=node_num, som_k=5, seed=32, device=DEV)
    old = (ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET, ops.FUSE_POOL)
    out = {}
    try:
        for name, cfg in (("fast", ("h3", True, True)), ("exact", ("f32", False, False))):
            ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET, ops.FUSE_POOL = cfg
            with torch.no_grad():
                f = enc(inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], False, None)
                out[name] = (f.cpu().numpy(), enc.first_pn_out_masked_max.cpu().numpy(), enc.som_node.cpu().numpy())
    finally:
        ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET, ops.FUSE_POOL = old
    np.testing.assert_array_equal(out["fast"][2], out["exact"][2])
    assert_close_rms(out["fast"][1], out["exact"][1], 1e-5, "first_pn_out_masked_max")
    assert_close_rms(out["fast"][0], out["exact"][0], 1e-5, "feature")


def test_linear_act_vs_torch():
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(13)
    for B, Cin, Cout, relu in [(64, 1024, 512, True), (8, 512, 256, True), (3, 256, 40, False), (70, 33, 5, True), (5, 2500, 48, True),
                               (2, 4096, 8, False), (17, 1026, 9, True)]:
        x, W = torch.randn(B, Cin, generator=gen), torch.randn(Cout, Cin, generator=gen) * 0.05
        sc, sh = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout, generator=gen)
        ref = (x.double() @ W.double().t()) * sc.double() + sh.double()
        ref = torch.relu(ref) if relu else ref
        got = ops.linear_act(x.to(DEV), W.to(DEV), sc.to(DEV), sh.to(DEV), relu).cpu().double()
        assert float((got - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))


def test_knn_self_vs_topk():
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(9)
    for B, M, K in [(4, 64, 9), (2, 100, 16), (3, 5, 5)]:
        node = torch.rand(B, 3, M, generator=gen) * 2 - 1
        d = ((node.unsqueeze(3) - node.unsqueeze(2)) ** 2).sum(dim=1)        # (dx^2 + dy^2) + dz^2, as layers.py:333-337
        ref = torch.topk(d, k=K, dim=2, largest=False, sorted=True)[1]
        got = ops.knn_self(node.to(DEV), K).cpu()
        assert torch.equal(got[:, :, 0], torch.arange(M).expand(B, M))       # itself first
        assert torch.equal(got, ref)
    dup = torch.zeros(1, 3, 8)                                                # all nodes coincide: ties -> ascending index
    assert torch.equal(ops.knn_self(dup.to(DEV), 4).cpu()[0, 5], torch.tensor([0, 1, 2, 3]))


def test_batch_som_update_golden():
    """BatchSOM.batch_update (SOM training iterations, util/som.py:295-366) on the assignment / grouping kernels."""
    from util import som
    g = golden("som_update_b2_n3000")
    x = cu(g["x"])
    s = som.BatchSOM(8, 8, 3, 0, x.shape[0])
    np.testing.assert_allclose(s.get_weighting_matrix(0.3).cpu().numpy(), g["weighting"], rtol=1e-6, atol=1e-12)
    s.node = cu(g["node0"]).clone()
    s.batch_update(x, s.learning_rate, s.sigma)
    assert_close_rms(s.node.cpu().numpy(), g["node1"], 1e-5, "nodes after one update")
    for it in range(5):
        decay = 1 + 2 * it / 5
        s.batch_update(x, s.learning_rate / decay, s.sigma / decay)
    assert_close_rms(s.node.cpu().numpy(), g["node6"], 1e-4, "nodes after six updates")


def test_knn_group_and_lastdim_max_vs_torch():
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(4)
    for B, C, M, K, avg in [(3, 384, 64, 9, True), (2, 5, 16, 4, False), (1, 1, 7, 7, True)]:
        coord, feat = torch.randn(B, 3, M, generator=gen), torch.randn(B, C, M, generator=gen)
        I = torch.stack([torch.stack([torch.randperm(M, generator=gen)[:K] for _ in range(M)]) for _ in range(B)])
        idx = I.reshape(B, 1, M * K)
        nb = torch.gather(coord, 2, idx.expand(B, 3, M * K)).reshape(B, 3, M, K)
        center = nb.mean(dim=3, keepdim=True) if avg else coord.unsqueeze(3)
        ref = torch.cat((nb - center, torch.gather(feat, 2, idx.expand(B, C, M * K)).reshape(B, C, M, K)), dim=1)
        c, out = ops.knn_group(coord.to(DEV), feat.to(DEV), I.to(DEV), avg)
        assert torch.allclose(c.cpu(), center.squeeze(3), rtol=1e-6, atol=1e-6)
        assert torch.allclose(out.cpu(), ref, rtol=1e-6, atol=1e-6)
        assert torch.equal(out[:, 3:].cpu(), ref[:, 3:])
    x = torch.randn(5, 17, 64, 9, generator=gen)
    x[0, 0, 0, 3] = float("nan")
    got = ops.lastdim_max(x.to(DEV)).cpu()
    ref = torch.amax(x, dim=3)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~torch.isnan(ref)], ref[~torch.isnan(ref)])
    y = torch.randn(4, 1024, 64, generator=gen)
    assert torch.equal(ops.lastdim_max(y.to(DEV)).cpu(), torch.amax(y, dim=2))


def test_node_add_affine_act_vs_torch():
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(2)
    for B, C, M, L, relu in [(2, 1024, 64, 3072, True), (3, 7, 5, 33, False), (1, 64, 64, 15000, True)]:
        t = torch.randn(B, C, L, generator=gen)
        z = torch.randn(B, C, M, generator=gen)
        idx = torch.randint(0, M, (B, L), generator=gen, dtype=torch.int32)
        sc, sh = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
        ref = (t + torch.gather(z, 2, idx.long().unsqueeze(1).expand(B, C, L))) * sc.view(1, -1, 1) + sh.view(1, -1, 1)
        ref = torch.relu(ref) if relu else ref
        out = ops.node_add_affine_act_(t.to(DEV), z.to(DEV), idx.to(DEV), sc.to(DEV), sh.to(DEV), relu)
        assert torch.allclose(out.cpu(), ref, rtol=1e-6, atol=1e-6)


def test_node_gather_vs_torch():
    from sonet_hip import ops
    gen = torch.Generator().manual_seed(1)
    for B, C, M, kN in [(3, 384, 64, 3072), (2, 5, 7, 13), (1, 1024, 64, 15000)]:
        feat = torch.randn(B, C, M, generator=gen)
        idx = torch.randint(0, M, (B, kN), generator=gen, dtype=torch.int32)
        ref = torch.gather(feat, 2, idx.long().unsqueeze(1).expand(B, C, kN))
        out = ops.node_gather(feat.to(DEV), idx.to(DEV))
        assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------ training step (configs 2 / 5)


@pytest.mark.parametrize("fixture", ["train_step_b16_n512", "train_step_b8_n5000"])       # the second: configs[1] / configs[4] point count
@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_classifier_training_step_golden(mode, fixture):
    """One training step (train-mode BN, backward, two Adam steps) vs the reference's Model.optimize."""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden(fixture)
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.0, node_num=64, k=3, som_k=9, som_k_type="avg",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), seed)
    synth.fill_state_dict_(cls.state_dict(), seed + 1)
    enc.to(DEV).train()
    cls.to(DEV).train()
    opt_e = torch.optim.Adam(enc.parameters(), lr=0.001, betas=(0.9, 0.999), weight_decay=0)
    opt_c = torch.optim.Adam(cls.parameters(), lr=0.001, betas=(0.9, 0.999), weight_decay=0)
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = mode
    try:
        captured = _capture_stage(enc)
        feat = enc(cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), is_train=True, epoch=0)
        score = cls(feat, 0)
        captured.update(_routing_of(enc, feat))
        enc.zero_grad()
        cls.zero_grad()
        loss = torch.nn.functional.cross_entropy(score, cu(g["label"]))
        captured["masks"] = _relu_masks_of(loss, enc, cls)
        loss.backward()
    finally:
        ops.POINTMLP_PRECISION = old
    assert_close_rms(feat.detach().cpu().numpy(), g["feature"], 1e-4, "train feature")
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))

    def sub(t):
        f = t.detach().flatten()
        return f[::max(1, f.numel() // 16384)].cpu().numpy().astype(np.float64)

    def rel_rms(a, r):
        return float(np.sqrt(np.mean((a - r) ** 2)) / np.sqrt(np.mean(r ** 2)))

    # End-to-end gradients pass three arg-max pools and eight ReLU patterns: DISCRETE decisions.  ANY change of rounding flips a few of them
    # (the reference's own float32 run: 1 winner of the first pool, 0 .. 1 of the second; route32/ vs route64/), one flipped winner moves a
    # first-PointNet weight gradient by ~3e-3 rel-rms, one flipped ReLU element that happens to carry gradient by up to 1e-3 -- which ones
    # flip is a lottery of the particular rounding, so a per-parameter bound against grad64/ can only be loose.  What is asserted instead:
    #   1. (test_training_gradients_with_forced_routing, below) with THIS run's decisions forced on the float64 restatement of the
    #      reference step (pinned to grad64/ and route64/ on the CPU), every gradient agrees to 1e-4 (measured: <= 2.2e-5, every arithmetic,
    #      both fixtures: profiles/r06b_grad_forced_routing.log) -- no flip can hide a bug, a 3e-3 error in one layer fails;
    #   2. (here) the decisions themselves: against a float64 run on the same columns this run flips no more winners than a handful and
    #      no more than 1e-4 of any layer's ReLU elements;
    #   3. (here) the gross check against the reference's own float64 gradients: 2e-2 rel-rms on the sampled elements.
    params = dict(enc.named_parameters())
    free = _f64_step(enc, cls, g, captured, forced=False)
    flips1 = int((free["route"]["pool1"] != captured["pool1"]).sum())
    flips2 = int((free["route"]["pool2"] != captured["pool2"]).sum())
    assert flips1 <= 8 and flips2 <= 8, (flips1, flips2)
    for layer, m in captured["masks"].items():
        diff = float((free["masks"][layer].reshape(m.shape) != m).float().mean())
        assert diff <= 1e-4, (layer, diff)
    for k in [k[7:] for k in g.files if k.startswith("grad64/") and not k.startswith("grad64/cls.")]:
        truth = g["grad64/" + k].astype(np.float64)
        if np.sqrt(np.mean(truth ** 2)) < 1e-5:        # biases in front of a BatchNorm: true gradient is 0
            continue
        mine = rel_rms(sub(params[k].grad), truth)
        assert mine <= 2e-2, (k, mine, float(g["ref32_dev/" + k]), flips1, flips2)
    assert rel_rms(sub(dict(cls.named_parameters())["fc1.linear.weight"].grad), g["grad64/cls.fc1.linear.weight"].astype(np.float64)) <= 5e-4
    assert sum(1 for p in enc.parameters() if p.grad is None) == int(g["dead_grad_count"])     # the dead Transformer
    sd = enc.state_dict()
    for k in [k[3:] for k in g.files if k.startswith("bn/")]:
        assert_close_rms(sd[k].cpu().numpy(), g["bn/" + k], 1e-4, "running stat " + k)
    opt_e.step()
    opt_c.step()
    # first Adam step = -lr * sign(grad) per element: elements whose true gradient is ~0 move by noise in ANY
    # implementation, so require 95 % of the well-conditioned tensors' elements to match the reference update
    for k in [k[6:] for k in g.files if k.startswith("after/")]:
        if np.sqrt(np.mean(g["grad64/" + k].astype(np.float64) ** 2)) < 1e-5 or not k.endswith("conv.weight"):
            continue                                    # BN affine terms of dead (all-negative) channels have ~0 gradient too
        got, ref = sub(params[k]), g["after/" + k].astype(np.float64)
        assert np.mean(np.abs(got - ref) <= 1e-4 * np.maximum(np.abs(ref), 1e-2)) >= 0.95, k


@pytest.mark.parametrize("fixture", ["train_step_b16_n512", "train_step_b8_n5000"])
@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
def test_training_gradients_with_forced_routing(mode, fixture):
    """Every gradient of the training step against float64 -- with the arg-max ROUTING taken out of the comparison.

    The float64 side is tests/f64_classifier.py (pinned on the CPU to the unmodified reference's float64 run: same positions at all three
    pools, gradients to 1e-12).  It is fed the SOM stage of the run under test (bit-exact on its own: test_som_*), in the column order the
    run used, and the run's DISCRETE decisions are forced on it: the positions its three pools took (gathers instead of arg-max) and the
    ReLU pattern of its eight BatchNorm + ReLU layers (read from what the run's autograd nodes saved; a mask instead of the sign test).
    Neither a flipped winner nor a flipped ReLU element can then explain a difference: the loss must agree to 1e-5 and EVERY parameter
    gradient (whole tensors, not samples) to 1e-4 rel-rms (measured <= 2.2e-5).  This is the gate that replaced the flat 5e-3 floor of
    round 5: a real 3e-3 gradient error in any layer fails here.  (With the pools forced but the ReLU patterns free the same comparison
    sits at 3e-4 .. 5e-3 -- and so does plain float32 torch autograd of the same step: tools/grad_forced_routing.py.)"""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden(fixture)
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
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION = mode
    try:
        cap = _capture_stage(enc)
        feat = enc(cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), is_train=True, epoch=0)
        score = cls(feat, 0)
        cap.update(_routing_of(enc, feat))
        loss = torch.nn.functional.cross_entropy(score, cu(g["label"]))
        cap["masks"] = _relu_masks_of(loss, enc, cls)
        loss.backward()
    finally:
        ops.POINTMLP_PRECISION = old
    assert sorted(cap["masks"]) == ["cls.fc1", "cls.fc2", "final_pointnet.layers.0", "first_pointnet.layers.0", "first_pointnet.layers.1",
                                    "first_pointnet.layers.2", "knnlayer.layers.0", "knnlayer.layers.1"], sorted(cap["masks"])
    if mode == "h3" and N >= 5000:
        assert cap["pos0"] is not None, "the f32-class training forward was expected to run on node-sorted columns"
    r = _f64_step(enc, cls, g, cap, forced=True)
    assert abs(float(loss.detach()) - float(r["loss"])) <= 1e-5 * abs(float(r["loss"]))
    assert_close_rms(feat.detach().cpu().numpy(), r["feature"].cpu().numpy(), 1e-4, "feature, same routing")   # (training-mode BatchNorm: the bound of the golden test)
    mine = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
    mine.update({"cls." + k: p.grad for k, p in cls.named_parameters() if p.grad is not None})
    worst, checked = ("", 0.0), 0
    for k, ref in r["grads"].items():
        rn = float(ref.norm()) / max(1.0, float(ref.numel()) ** 0.5)
        if rn < 1e-7:                                  # biases in front of a BatchNorm: the true gradient is 0
            continue
        assert k in mine, k
        rel = float((mine[k].double() - ref).norm() / ref.norm())
        checked += 1
        if rel > worst[1]:
            worst = (k, rel)
    assert checked >= 25, checked
    assert worst[1] <= 1e-4, worst
    # the parameters autograd left without a gradient are the reference's dead ones (the Transformer) and nothing else
    assert sum(1 for p in enc.parameters() if p.grad is None) == int(g["dead_grad_count"])


def test_backward_components_vs_float64():
    """Backward of the fused layers (train-mode BN + ReLU, no-norm, Conv2d 1x1 + max over K', PointResNet with the
    fused skip concat, knn gather) against float64 autograd of the same math -- no arg-max routing in between."""
    import torch.nn.functional as F
    from models import layers as L, operations
    from sonet_hip import ops
    torch.manual_seed(0)

    def rel(a, b):
        return ((a.double() - b.double()).norm() / b.double().norm()).item()

    def ref_layer(l, t, w=None):
        w = l.conv.weight.detach().double() if w is None else w
        conv = F.conv2d if t.dim() == 4 else F.conv1d
        r = conv(t, w, l.conv.bias.detach().double())
        if l.normalization == "batch":
            r = F.batch_norm(r, None, None, l.norm.weight.detach().double(), l.norm.bias.detach().double(), True, 0.1, 1e-5)
        return F.relu(r) if l.activation == "relu" else r

    for mode in ("h3", "x3", "f32"):
        old = ops.POINTMLP_PRECISION
        ops.POINTMLP_PRECISION = mode
        try:
            for mk, shape, sparse in [(lambda: L.EquivariantLayer(515, 768, "relu", "batch"), (16, 515, 64), True),
                                      (lambda: L.EquivariantLayer(320, 384, None, None), (4, 320, 300), False),
                                      (lambda: L.MyConv2d(387, 512, 1, activation="relu", normalization="batch"), (8, 387, 64, 9), True)]:
                layer = mk().to(DEV).train()
                with torch.no_grad():
                    layer.conv.bias.uniform_(-0.1, 0.1)
                x = torch.randn(*shape, device=DEV, requires_grad=True)
                y = layer(x)
                gy = torch.randn_like(y)
                if sparse:
                    gy = gy * (torch.rand_like(gy) < 0.02)
                y.backward(gy)
                x64 = x.detach().double().requires_grad_(True)
                w64 = layer.conv.weight.detach().double().requires_grad_(True)
                r = ref_layer(layer, x64, w64)
                r.backward(gy.double())
                assert rel(y.detach(), r.detach()) < 1e-5
                assert rel(x.grad, x64.grad) < 1e-5 and rel(layer.conv.weight.grad, w64.grad) < 1e-5, (mode, shape)
            pr = L.PointResNet(6, [64, 128, 256, 384], "relu", "batch").to(DEV).train()
            x = torch.randn(4, 6, 500, device=DEV, requires_grad=True)
            y = pr(x)
            gy = torch.randn_like(y)
            y.backward(gy)
            x64 = x.detach().double().requires_grad_(True)
            ws = [l.conv.weight.detach().double().requires_grad_(True) for l in pr.layers]
            l0 = ref_layer(pr.layers[0], x64, ws[0])
            t = ref_layer(pr.layers[2], ref_layer(pr.layers[1], l0, ws[1]), ws[2])
            r = ref_layer(pr.layers[3], torch.cat((l0, t), 1), ws[3])
            r.backward(gy.double())
            assert rel(x.grad, x64.grad) < 1e-5
            for l, w in zip(pr.layers, ws):
                assert rel(l.conv.weight.grad, w.grad) < 1e-5
        finally:
            ops.POINTMLP_PRECISION = old
    xk = torch.randn(3, 20, 64, device=DEV, requires_grad=True)
    I = torch.randint(0, 64, (3, 64, 9), device=DEV)
    o = operations.knn_gather_by_indexing(xk, I)
    go = torch.randn_like(o)
    o.backward(go)
    xk2 = xk.detach().clone().requires_grad_(True)
    torch.gather(xk2, 2, I.reshape(3, 1, 576).expand(3, 20, 576)).view(3, 20, 64, 9).backward(go)
    assert rel(xk.grad, xk2.grad) < 1e-6


def test_sort_group_and_fused_pool():
    """Node-sorted grouping + (first PointNet & per-node max-pool in one kernel) == layerwise path + index_max_gather."""
    from models import layers as L
    from sonet_hip import ops, synth
    pr = L.PointResNet(6, [64, 128, 256, 384], "relu", "batch", 0.1, None, 1)
    synth.fill_state_dict_(pr.state_dict(), seed=7)
    pr.to(DEV).eval()
    old = (ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET)
    ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET = "h3", True
    try:
        # (sizes around the kernel's tiling: 256 points per workgroup tile, 64 per wave, 32 per column tile; more than 16 nodes in one
        # tile -- the straight-to-memory atomics --, nodes spanning many tiles, a single point)
        for B, N, M, k, kind in [(3, 5000, 64, 3, "som"), (2, 333, 64, 3, "uniform"), (2, 40, 64, 1, "uniform"), (1, 1, 64, 3, "uniform"),
                                 (2, 86, 9, 3, "uniform"), (1, 64, 4, 1, "uniform"), (2, 171, 64, 3, "uniform"), (1, 2000, 4, 3, "uniform"),
                                 (3, 97, 64, 2, "uniform")]:
            inp = synth.make_inputs(B, N, M=M, som_k=min(9, M), seed=N + k, node_kind=kind)
            x, sn = inp["pc"].to(DEV), inp["sn"].to(DEV)
            a = ops.som_assign(x, inp["node"].to(DEV), k)
            g = ops.som_group(x, sn, a, want_augmented=True)
            s = ops.som_sort_group(x, sn, a)
            # sorted grouping: same per-node means / occupancy, ids non-decreasing, same multiset of rows per node
            assert torch.equal(s["som_node"], g["som_node"]) and torch.equal(s["row_max"], g["row_max"])
            ids = s["ids_sorted"]
            assert bool((ids[:, 1:] >= ids[:, :-1]).all())
            assert torch.equal(torch.sort(a.min_idx_i32, dim=1)[0], ids)
            xa, xs = g["x_augmented"].cpu(), s["x_aug_sorted"].cpu()
            for b in range(B):
                p0 = int(s["pos0"][b])
                assert torch.equal(xs[b, :, p0], xa[b, :, 0])                          # original copy 0
                order = torch.sort(a.min_idx_i32[b].cpu().long(), stable=True)[1]
                ref_rows = xa[b][:, order].t()                                          # grouped by node, some order inside
                got_rows = xs[b].t()
                idsb = ids[b].cpu()
                for m in torch.unique(idsb).tolist():
                    sel = idsb == m
                    assert torch.equal(torch.sort(ref_rows[sel], dim=0)[0], torch.sort(got_rows[sel], dim=0)[0])
            with torch.no_grad():
                first = pr(g["x_augmented"])                                            # fused, stores
                _, ref = ops.index_max_gather(first, a.min_idx_i32, M, g["row_max"])
                wstream, affine = pr._fused_state()
                got = ops.pointresnet_fused_pool(s, wstream, affine, M)
            assert tuple(got.shape) == (B, 384, M)
            assert_close_rms(got.cpu().numpy(), ref.cpu().numpy(), 1e-6, "fused pool B=%d N=%d" % (B, N))
    finally:
        ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET = old


def test_encoder_fast_path_lazily_materialises_first_pn_out():
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden("classifier_b2_n256")
    opt = make_opt(g, 2, 256)
    enc = NW.Encoder(opt)
    synth.fill_state_dict_(enc.state_dict(), int(g["seed"]))
    enc.to(DEV).eval()
    args = (cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]))
    # the fast path is what this test is about: pin the switches that select it, whatever the
    # environment defaults (SONET_POINTMLP_PRECISION / SONET_FUSE_*) say
    old = ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET, ops.FUSE_POOL
    ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET, ops.FUSE_POOL = "h3", True, True
    try:
        with torch.no_grad(), ops.kernel_timing() as rec:
            enc(*args)
        names = [n for n, _, _ in rec.records]
        assert any(n.startswith("pointresnet_fused_pool") for n in names) and not any(n.startswith("index_max") for n in names)
        assert enc._first_pn_out is None
        assert_close_rms(enc.first_pn_out[:, ::16, ::5].cpu().numpy(), g["first_pn_out_sub"], 1e-5, "lazy first_pn_out")
    finally:
        ops.POINTMLP_PRECISION, ops.FUSE_POINTRESNET, ops.FUSE_POOL = old


def test_mfma_sustained_rate_probe():
    """The roofline measuring stick (sonet_diag_mfma_f16_rate): constant operands run near the nominal matrix rate,
    random mantissas cannot be faster, and both report a plausible shader clock."""
    from sonet_hip import ops
    tf_c, ghz_c = ops.mfma_f16_sustained_rate(random_operands=False, iters=2000)
    tf_r, ghz_r = ops.mfma_f16_sustained_rate(random_operands=True, iters=2000)
    assert 500.0 < tf_r <= tf_c * 1.05 and tf_c < 2700.0, (tf_c, tf_r)
    assert 0.8 < ghz_r < 2.6 and 0.8 < ghz_c < 2.6, (ghz_c, ghz_r)


@pytest.mark.parametrize("M,K,C", [(64, 9, 384), (36, 5, 48), (100, 3, 16)])
def test_pointmlp_gather_and_planes_max(M, K, C):
    """knn_prepare + a gather index in the layer's operand load + planes_max reproduce knn_group -> layer -> max over K
    bit for bit (same MFMA sequence; only the gathered tensor is never written)."""
    from sonet_hip import ops
    B, Cout = 3, 64
    g = torch.Generator(device="cpu").manual_seed(M * 10 + K)
    feat = torch.randn(B, C, M, generator=g).to(DEV)
    coord = torch.randn(B, 3, M, generator=g).to(DEV)
    knn_I = torch.randint(0, M, (B, M, K), generator=g).to(DEV)
    knn_I[0, 1, 0] = M + 5                                           # out of range: reads as zeros
    center, dec, gidx = ops.knn_prepare(coord, knn_I, True)
    c_ref, grouped = ops.knn_group(coord, feat, knn_I, True)         # B x (3 + C) x M x K
    assert torch.equal(center, c_ref)
    kmaj = grouped.permute(0, 1, 3, 2).reshape(B, 3 + C, K * M).contiguous()      # k-major columns
    assert torch.equal(dec, kmaj[:, :3].contiguous())
    W = (torch.randn(Cout, 3 + C, generator=g) * 0.1).to(DEV)
    sc, sh = (torch.rand(Cout, generator=g) + 0.5).to(DEV), torch.randn(Cout, generator=g).to(DEV)
    w_rot = ops.pointmlp_pack(torch.cat((W[:, 3:], W[:, :3]), dim=1).contiguous(), "h3")
    x_rot = torch.cat((kmaj[:, 3:], kmaj[:, :3]), dim=1).contiguous()
    ref = ops.pointmlp(x_rot, w_rot, sc, sh, True, Cout)             # B x Cout x (K*M)
    got = ops.pointmlp(feat, w_rot, sc, sh, True, Cout, x2=dec, gidx=gidx)
    assert torch.equal(got, ref)
    assert torch.equal(ops.planes_max(got, K), ref.reshape(B, Cout, K, M).amax(dim=2))
    bad = got.clone()
    bad[1, 5, 2 * M + 3] = float("nan")                              # plane 2, node 3
    out = ops.planes_max(bad, K)
    assert bool(torch.isnan(out[1, 5, 3])) and int(torch.isnan(out).sum()) == 1


def test_encoder_node_stage_gather_matches_materialised_path():
    """SONET_GATHER_NODE_STAGE on/off: same features within the split arithmetic's own noise (the 3 coordinate channels
    move to the end of the summation order, nothing else changes)."""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden("classifier_b2_n256")
    opt = make_opt(g, 2, 256)
    enc = NW.Encoder(opt)
    synth.fill_state_dict_(enc.state_dict(), int(g["seed"]))
    enc.to(DEV).eval()
    args = (cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]))
    old = ops.GATHER_NODE_STAGE, ops.POINTMLP_PRECISION
    old_flat = ops.NODE_STAGE_P16
    try:
        ops.POINTMLP_PRECISION = "h3"
        ops.NODE_STAGE_P16 = False               # (the flat stage of round 5 has its own comparison: tests/test_gpu_node_stage.py)
        outs = {}
        for flag in (True, False):
            ops.GATHER_NODE_STAGE = flag
            with torch.no_grad(), ops.kernel_timing() as rec:
                f = enc(*args).clone()
            names = [n for n, _, _ in rec.records]
            assert ("knn_prepare" in names) == flag and ("knn_group" in names) == (not flag)
            outs[flag] = (f, enc.knn_feature_1.clone(), enc.final_pn_out.clone(), enc.knn_center_1.clone())
        for a, b in zip(outs[True], outs[False]):
            assert_close_rms(a.cpu().numpy(), b.cpu().numpy(), 5e-6, "gathering node stage vs materialised")   # the split itself: ~3e-6
    finally:
        ops.GATHER_NODE_STAGE, ops.POINTMLP_PRECISION = old
        ops.NODE_STAGE_P16 = old_flat


def test_pooled_wgrad_matches_dense_scatter_gemm():
    """sonet_pooled_wgrad_f32 == (scatter g into zeros at pos) @ x^T summed over the batch (float64 reference), including
    duplicate positions, position 0 pile-ups (empty nodes) and out-of-range entries."""
    from sonet_hip import ops
    B, C, M, Ci, L = 3, 40, 16, 10, 500
    g = torch.Generator(device="cpu").manual_seed(5)
    gp = torch.randn(B, C, M, generator=g).to(DEV)
    pos = torch.randint(0, L, (B, C, M), generator=g, dtype=torch.int32).to(DEV)
    pos[:, :, 3] = 0                                                  # an "empty node": every channel gathers position 0
    pos[1, 5, 7] = pos[1, 5, 8]                                       # duplicate
    pos[2, 0, 0] = -1                                                 # ignored
    x = torch.randn(B, Ci, L, generator=g).to(DEV)
    got = ops.pooled_wgrad(gp.transpose(1, 2).contiguous(), pos.transpose(1, 2).contiguous(), x)
    G = torch.zeros(B, C, L, dtype=torch.float64, device=DEV)
    ok = pos >= 0
    G.scatter_add_(2, pos.clamp_min(0).long(), (gp.double() * ok))
    ref = torch.bmm(G, x.double().transpose(1, 2)).sum(0)
    assert_close_rms(got.cpu().numpy(), ref.cpu().numpy(), 1e-5, "pooled wgrad")


@pytest.mark.parametrize("B,N,M,k,kind", [(64, 5000, 64, 3, "som"), (3, 1024, 64, 3, "som"), (2, 333, 64, 3, "uniform"), (2, 40, 64, 1, "uniform"),
                                          (1, 1, 64, 3, "uniform"), (2, 2500, 100, 2, "som"), (2, 1025, 16, 4, "uniform"), (1, 3000, 9, 3, "uniform")])
def test_som_assign_sort_equals_the_separate_launches(B, N, M, k, kind):
    """The two-launch SOM stage (sonet_som_assign_sort_f32) against som_assign + som_sort_group: node ids, counts, node means,
    offsets bit-identical; the sorted copies are the same MULTISET per node (order inside a node is free); and the oracle's ids."""
    from oracle import cpu_oracle as O
    from sonet_hip import ops, synth
    inp = synth.make_inputs(B, N, M=M, seed=31, node_kind=kind)
    x, sn, node = inp["pc"].to(DEV), inp["sn"].to(DEV), inp["node"].to(DEV)
    a0 = ops.som_assign(x, node, k)
    g0 = ops.som_sort_group(x, sn, a0)
    a1, g1 = ops.som_assign_sort(x, sn, node, k, want_i64=True)
    assert torch.equal(a1.min_idx_i32, a0.min_idx_i32) and torch.equal(a1.min_idx_i64, a0.min_idx_i32.long())
    assert torch.equal(a1.count, a0.count) and torch.equal(g1["row_max"], g0["row_max"]) and torch.equal(g1["node_off"], g0["node_off"])
    np.testing.assert_allclose(a1.sum_ws.cpu().numpy(), a0.sum_ws.cpu().numpy(), rtol=1e-12, atol=1e-12)   # double sums, other order
    assert torch.equal(g1["som_node"], g0["som_node"])
    if B * N <= 64 * 1024:
        np.testing.assert_array_equal(a1.min_idx_i32.cpu().numpy(), O.som_query_topk(inp["pc"], inp["node"], k)[0])
    ids0, ids1 = g0["ids_sorted"].cpu().numpy(), g1["ids_sorted"].cpu().numpy()
    np.testing.assert_array_equal(ids0, ids1)                        # (sorted by node: the id sequence itself is the same)
    assert (np.diff(ids1, axis=1) >= 0).all()
    xa0, xa1 = g0["x_aug_sorted"].cpu().numpy(), g1["x_aug_sorted"].cpu().numpy()
    kN = k * N
    for b in range(min(B, 3)):                                       # same multiset of 6-vectors inside every node
        o0 = np.lexsort(tuple(xa0[b, c] for c in range(5, -1, -1)) + (ids0[b],))
        o1 = np.lexsort(tuple(xa1[b, c] for c in range(5, -1, -1)) + (ids1[b],))
        np.testing.assert_array_equal(xa0[b][:, o0], xa1[b][:, o1])
    # pos0 = the sorted position of original copy 0: its six values and its node
    p1 = g1["pos0"].cpu().numpy()
    for b in range(B):
        assert ids1[b, p1[b]] == int(a1.min_idx_i32[b, 0])
        np.testing.assert_array_equal(xa1[b, 3:, p1[b]], inp["sn"][b, :, 0].numpy())
    assert kN == ids1.shape[1]
