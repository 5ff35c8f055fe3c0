"""Batch assembler on the MI355X (sonet_assemble_batch_f32, sonet_hip.batch): replay parity with the reference loaders' fixtures,
the random mode's exactness (determinism, slot independence, the documented generator, replay of its own draws), its statistics,
edge cases, checks before the launch, and the training / test loop fed by BatchAssembler."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = ("modelnet_train_all_flags", "modelnet_train_no_flags", "modelnet_test", "shrec_train_4x4_k1", "shapenet_train_ragged",
         "modelnet_train_bench_shape")


def _opt(N, M=64, som_k=9, **kw):
    return Namespace(input_pc_num=N, node_num=M, som_k=som_k, rot_horizontal=kw.get("rot_horizontal", False),
                     rot_perturbation=kw.get("rot_perturbation", False),
                     translation_perturbation=kw.get("translation_perturbation", False))


def _clouds_from(g):
    from sonet_hip.batch import DeviceClouds
    off, src = g["offsets"], g["src"]
    pts = [src[:3, off[s]:off[s + 1]].T for s in range(len(off) - 1)]
    nrm = [src[3:, off[s]:off[s + 1]].T for s in range(len(off) - 1)]
    seg = [g["seg"][off[s]:off[s + 1]] for s in range(len(off) - 1)] if "seg" in g.files else None
    return DeviceClouds(pts, nrm, g["labels"], nodes=g["nodes_src"], seg=seg, device=DEV)


def _synthetic(sizes, M=64, seed=0, seg=False):
    from sonet_hip.batch import DeviceClouds
    g = np.random.RandomState(seed)
    pts = [g.normal(size=(n, 3)).astype(np.float32) for n in sizes]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = g.normal(size=(len(sizes), M, 3)).astype(np.float32)
    sg = [g.randint(0, 50, n) for n in sizes] if seg else None
    return DeviceClouds(pts, nrm, g.randint(0, 40, len(sizes)), nodes=nodes, seg=sg, device=DEV)


def _within_one_ulp(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert np.isfinite(got).all() and (err <= ulp).all(), "%s: %d values off by more than 1 ulp, worst %.3g ulp" % (
        what, int((err > ulp).sum()), float((err / ulp).max()))
    return float((err > 0).mean())


# ------------------------------------------------------------------------------------------------------------ replay parity
@pytest.mark.parametrize("case", CASES)
def test_replay_matches_reference_loader(case):
    from sonet_hip.batch import BatchAssembler
    g = golden("batch/" + case)
    fl = int(g["flags"])
    recipe, mode = str(g["recipe"]), str(g["mode"])
    opt = _opt(int(g["N"]), int(g["M"]), int(g["K"]), rot_horizontal=bool(fl & 4), rot_perturbation=bool(fl & 8),
               translation_perturbation=bool(fl & 16))
    A = BatchAssembler(_clouds_from(g), opt, mode, recipe, seed=123)
    assert A.flags == fl
    rep_i = torch.from_numpy(g["replay_idx"]).to(DEV)
    rep_d = torch.from_numpy(g["replay_draws"]).to(DEV) if mode == "train" else None
    out, raw = A.batch_with_draws(g["idx"], 5, replay_idx=rep_i, replay_draws=rep_d)
    torch.cuda.synchronize()
    if recipe == "shapenet":
        pc, sn, label, seg, node, knn = out
        assert seg.dtype == torch.int64 and np.array_equal(seg.cpu().numpy(), g["seg_out"])
    else:
        pc, sn, label, node, knn = out[:5]
        if recipe == "shrec":
            assert np.array_equal(out[5].cpu().numpy(), g["idx"])
    assert pc.dtype == sn.dtype == node.dtype == torch.float32 and label.dtype == knn.dtype == torch.int64
    assert np.array_equal(label.cpu().numpy(), g["label"])
    assert np.array_equal(knn.cpu().numpy(), g["knn_I"])
    assert np.array_equal(raw["chosen"].cpu().numpy(), g["offsets"][g["idx"]][:, None] + g["replay_idx"])
    assert (raw["bad"].cpu().numpy() == 0).all()
    if mode == "train":
        for got, what in ((pc, "pc"), (sn, "sn"), (node, "node")):
            frac = _within_one_ulp(got.cpu().numpy(), g[what], "%s %s" % (case, what))
            print("%s %s: %.2f%% of values 1 ulp off" % (case, what, 100 * frac))
        assert np.array_equal(raw["draws"].cpu().numpy(), g["replay_draws"])        # draws_out echoes the replayed draws
    else:
        for got, what in ((pc, "pc"), (sn, "sn"), (node, "node")):
            assert np.array_equal(got.cpu().numpy().view(np.int32), g[what].view(np.int32)), what


# ------------------------------------------------------------------------------------------------------------ random mode, exact
def _assembler(sizes=(300, 260, 400, 333), N=200, mode="train", recipe="modelnet", seed=7, M=64, som_k=9, flags=True):
    from sonet_hip.batch import BatchAssembler
    c = _synthetic(sizes, M=M, seg=recipe == "shapenet")
    kw = dict(rot_horizontal=True, rot_perturbation=True, translation_perturbation=True) if flags and recipe != "shapenet" else {}
    return BatchAssembler(c, _opt(N, M, som_k, **kw), mode, recipe, seed=seed)


def _np(t):
    return [x.cpu().numpy() for x in t]


def test_random_mode_is_deterministic_and_keyed_by_seed_and_step():
    A = _assembler()
    a, b = _np(A.batch([0, 1, 2, 3], 11)), _np(A.batch([0, 1, 2, 3], 11))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = _np(A.batch([0, 1, 2, 3], 12))
    d = _np(_assembler(seed=8).batch([0, 1, 2, 3], 11))
    for other in (c, d):
        assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[3], other[3])


def test_slot_depends_only_on_seed_step_and_slot():
    A = _assembler()
    full = _np(A.batch([2, 0, 3, 1], 4))
    short = _np(A.batch([2, 0], 4))
    other = _np(A.batch([2, 0, 1, 1, 3, 2, 0], 4))
    for k in (0, 1, 3, 4):
        assert np.array_equal(full[k][:2], short[k]) and np.array_equal(full[k][:2], other[k][:2])


@pytest.mark.parametrize("recipe", ["modelnet", "shapenet"])
def test_draws_equal_numpy_generator_and_replay_is_bit_exact(recipe):
    from sonet_hip import batch as BA
    sizes = (300, 200, 150, 257) if recipe == "shapenet" else (300, 260, 400, 333)
    A = _assembler(sizes=sizes, N=200 if recipe == "modelnet" else 257, recipe=recipe)
    idx, step = [3, 1, 0, 2, 3], 2 ** 33 + 5
    out, raw = A.batch_with_draws(idx, step)
    chosen, draws = raw["chosen"].cpu().numpy(), raw["draws"].cpu().numpy()
    off = A.clouds.offsets_host
    local = chosen - off[np.asarray(idx)][:, None]
    for b, s in enumerate(idx):
        c, d = BA.slot_draws(A.seed, step, b, int(A.clouds.sizes[s]), A.N, A.M, recipe)
        assert np.array_equal(local[b], c), "slot %d: chosen indices differ from the numpy generator" % b
        exact = [0, 4, 5, 6, 7]                         # uniforms: the same f64 arithmetic
        assert np.array_equal(draws[b, exact], d[exact])
        # normals: log / cos / sin of the device libm against numpy's, within 2^-44 absolute (|z| < 6.7)
        assert np.abs(draws[b] - d).max() <= 2.0 ** -44
    # the exported draws, fed back in, give the same batch bit for bit (one downstream path)
    rep, raw2 = A.batch_with_draws(idx, step, replay_idx=torch.from_numpy(local).to(DEV), replay_draws=raw["draws"])
    for x, y in zip(_np(out), _np(rep)):
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    from sonet_hip import ops
    node, knn = out[-2], out[-1]
    assert torch.equal(knn, ops.knn_self(node, A.K))


def test_random_mode_matches_restated_augmentation():
    """The kernel's augmentation against the float64 restatement fed with its own draws: within 1 ulp."""
    from sonet_hip import batch as BA
    A = _assembler()
    idx = [1, 3, 0]
    out, raw = A.batch_with_draws(idx, 9)
    pc, sn, label, node, knn = _np(out)
    off, draws, chosen = A.clouds.offsets_host, raw["draws"].cpu().numpy(), raw["chosen"].cpu().numpy()
    src, nodes = A.clouds.src.cpu().numpy(), A.clouds.nodes.cpu().numpy()
    for b, s in enumerate(idx):
        data = src[:, off[s]:off[s + 1]].T
        want = BA.augment_np(data, nodes[s], chosen[b] - off[s], draws[b], True, "modelnet", rot_horizontal=True, rot_perturbation=True,
                             translation_perturbation=True)
        for got, w, what in zip((pc[b], sn[b], node[b]), want, ("pc", "sn", "node")):
            _within_one_ulp(got, w, what)


# ------------------------------------------------------------------------------------------------------------ statistics
def test_selection_statistics():
    """20 000 draws of 16 of 64 (one launch): no duplicates, all in range, per-index inclusion frequency passes chi^2."""
    A = _assembler(sizes=(64,), N=16, mode="test", M=4, som_k=2)
    B = 20000
    _, raw = A.batch_with_draws(np.zeros(B, np.int64), 3)
    ch = raw["chosen"].cpu().numpy()
    assert ch.min() >= 0 and ch.max() < 64
    srt = np.sort(ch, 1)
    assert (np.diff(srt, axis=1) > 0).all(), "duplicate index within a slot"
    assert (np.diff(ch, axis=1) > 0).all(), "random mode emits ascending source order"
    counts = np.bincount(ch.reshape(-1), minlength=64)
    E = B * 16 / 64
    chi2 = float(((counts - E) ** 2 / E).sum())
    # without replacement the statistic is (1 - 16/64) x chi^2(63): mean ~47; 63 + 5 sqrt(126) = 119 is far out in the tail
    assert chi2 < 119, chi2


def test_augmentation_statistics():
    A = _assembler(sizes=(1000,) * 4, N=500)
    _, raw = A.batch_with_draws(np.arange(400) % 4, 1)
    d = raw["draws"].cpu().numpy()
    N, M = 500, 64
    u, pert, scale, shift = d[:, 0], d[:, 1:4], d[:, 4], d[:, 5:8]
    assert (u >= 0).all() and (u < 1).all() and ((u * 2 * math.pi) < 2 * math.pi).all()
    ang = np.clip(0.06 * pert, -0.18, 0.18)
    assert (np.abs(ang) <= 0.18).all()
    assert (scale >= 0.8).all() and (scale < 1.2).all()
    assert (shift >= -0.1).all() and (shift < 0.1).all()
    for lo, hi in ((0.8, 1.2), (-0.1, 0.1)):
        v = scale if lo == 0.8 else shift.reshape(-1)
        assert abs(v.mean() - (lo + hi) / 2) < 0.05 * (hi - lo)
    z = d[:, 8:].reshape(-1)
    assert z.size == 400 * (6 * N + 3 * M)
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    assert abs(np.mean(z ** 3)) < 2e-2 and abs(np.mean(z ** 4) - 3) < 5e-2
    # the applied jitter stays inside its clip: modelnet without flags, pc = (p + j) * scale
    B2 = _assembler(sizes=(1000,) * 4, N=500, flags=False)
    out, raw2 = B2.batch_with_draws(np.arange(8) % 4, 2)
    pc, sn, node = out[0].cpu().numpy().astype(np.float64), out[1].cpu().numpy().astype(np.float64), out[3].cpu().numpy().astype(np.float64)
    sc = raw2["draws"].cpu().numpy()[:, 4][:, None, None]
    src = B2.clouds.src.cpu().numpy().astype(np.float64)
    ch = raw2["chosen"].cpu().numpy()
    jp = pc / sc - np.stack([src[:3, c] for c in ch])
    jn = sn / sc - np.stack([src[3:, c] for c in ch])
    jm = node / sc - B2.clouds.nodes.cpu().numpy()[np.arange(8) % 4].transpose(0, 2, 1)
    assert np.abs(jp).max() <= 0.05 + 1e-5 and np.abs(jn).max() <= 0.05 + 1e-5 and np.abs(jm).max() <= 0.1 + 1e-5
    assert np.abs(jp).max() > 0.04


# ------------------------------------------------------------------------------------------------------------ edges
def test_shapenet_ragged_below_equal_above():
    N = 256
    A = _assembler(sizes=(300, 256, 200), N=N, recipe="shapenet")
    (pc, sn, label, seg, node, knn), raw = A.batch_with_draws([0, 1, 2], 0)
    ch = raw["chosen"].cpu().numpy() - A.clouds.offsets_host[[0, 1, 2]][:, None]
    assert len(set(ch[0])) == N and ch[0].max() < 300                       # n_s > N: without replacement
    assert np.array_equal(ch[1], np.arange(256))                              # n_s == N: every point, in order, no extra draw
    assert np.array_equal(ch[2][:200], np.arange(200)) and ch[2][200:].max() < 200 and ch[2][200:].min() >= 0   # n_s < N
    assert np.array_equal(seg.cpu().numpy(), A.clouds.seg.cpu().numpy()[raw["chosen"].cpu().numpy()])
    assert tuple(pc.shape) == (3, 3, N) and tuple(knn.shape) == (3, 64, 9)


def test_small_node_grid_k1_k16_b1_and_repeated_index():
    A = _assembler(M=16, som_k=1)
    pc, sn, label, node, knn = A.batch([2], 0)
    assert tuple(knn.shape) == (1, 16, 1) and np.array_equal(knn.cpu().numpy()[0, :, 0], np.arange(16))
    assert tuple(node.shape) == (1, 3, 16)
    A16 = _assembler(som_k=16)
    pc, sn, label, node, knn = A16.batch([1, 1, 1], 3)
    assert tuple(knn.shape) == (3, 64, 16)
    from sonet_hip import ops
    assert torch.equal(knn, ops.knn_self(node, 16))
    assert not torch.equal(pc[0], pc[1])                                     # the same cloud twice: different draws per slot
    T = _assembler(mode="test")
    a = _np(T.batch([1, 1], 3))
    c = T.clouds
    _, raw = T.batch_with_draws([1, 1], 3)
    ch = raw["chosen"].cpu().numpy()
    assert np.array_equal(a[0][0], c.src[:3].cpu().numpy()[:, ch[0]])         # test mode: bit-exact gathers
    assert np.array_equal(a[3][0], c.nodes[1].cpu().numpy().T)


def test_errors_before_launch():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    from sonet_hip.batch import BatchAssembler
    A = _assembler()
    with pytest.raises(SonetHipError, match="out of range"):
        A.batch([0, 4], 0)
    with pytest.raises(SonetHipError, match="out of range"):
        A.batch([-1], 0)
    c = _synthetic((300, 150))
    with pytest.raises(SonetHipError, match="input_pc_num"):
        BatchAssembler(c, _opt(200), "train", "modelnet")
    with pytest.raises(SonetHipError, match="K"):
        BatchAssembler(_synthetic((300,)), _opt(200, som_k=17), "train", "modelnet").batch([0], 0)
    with pytest.raises(SonetHipError, match="node_num"):
        BatchAssembler(_synthetic((300,)), _opt(200, M=16), "train", "modelnet")
    with pytest.raises(SonetHipError, match="seg"):
        BatchAssembler(_synthetic((300,)), _opt(200), "train", "shapenet")
    with pytest.raises(SonetHipError, match="N=200 > n_s=150"):
        ops.assemble_batch(c.src, c.offsets, c.nodes, torch.tensor([0, 1], device=DEV), 200, 9, ops.BATCH_TRAIN, 0, 0, sizes=c.sizes)
    with pytest.raises(SonetHipError, match="replay_idx"):
        ops.assemble_batch(c.src, c.offsets, c.nodes, torch.tensor([0], device=DEV), 100, 9, 0, 0, 0,
                           replay_idx=torch.zeros(1, 99, dtype=torch.int64, device=DEV))
    # device data the host did not check: the kernel marks the slot bad instead of reading outside the dataset
    r = ops.assemble_batch(c.src, c.offsets, c.nodes, torch.tensor([0, 1, 7], device=DEV), 200, 9, ops.BATCH_TRAIN, 0, 0)
    assert r["bad"].cpu().tolist() == [0, 1, 1]
    assert torch.isnan(r["pc"][1:]).all() and (r["chosen"][1:] == -1).all() and torch.isfinite(r["pc"][0]).all()
    bad_rep = torch.zeros(1, 100, dtype=torch.int64, device=DEV)
    bad_rep[0, 7] = 150
    r = ops.assemble_batch(c.src, c.offsets, c.nodes, torch.tensor([1], device=DEV), 100, 9, 0, 0, 0, replay_idx=bad_rep)
    assert r["bad"].item() == 1 and r["chosen"][0, 7].item() == -1 and r["chosen"][0, 6].item() == 300


# ------------------------------------------------------------------------------------------------------------ end to end
class _SetInput:
    """The staging of the reference's Model.set_input (models/classifier.py:65-73): resize_ + copy_ into the model's own tensors."""

    def __init__(self, dev):
        self.input_pc, self.input_sn = torch.FloatTensor(1, 3, 1).to(dev), torch.FloatTensor(1, 3, 1).to(dev)
        self.input_label, self.input_node = torch.LongTensor(1).to(dev), torch.FloatTensor(1, 3, 1).to(dev)
        self.input_node_knn_I = torch.LongTensor(1, 1).to(dev)

    def set_input(self, input_pc, input_sn, input_label, input_node, input_node_knn_I):
        self.input_pc.resize_(input_pc.size()).copy_(input_pc)
        self.input_sn.resize_(input_sn.size()).copy_(input_sn)
        self.input_label.resize_(input_label.size()).copy_(input_label)
        self.input_node.resize_(input_node.size()).copy_(input_node)
        self.input_node_knn_I.resize_(input_node_knn_I.size()).copy_(input_node_knn_I)
        self.pc, self.sn, self.label = self.input_pc.detach(), self.input_sn.detach(), self.input_label.detach()


def _model_opt(B, N):
    return Namespace(gpu_id=0, device=DEV, batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                     normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                     bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40, rot_horizontal=True, rot_perturbation=True,
                     translation_perturbation=True)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_epoch_feeds_training_steps(precision):
    from models import networks as NW
    from sonet_hip import ops, synth
    from sonet_hip.batch import BatchAssembler
    from sonet_hip.optim import FusedAdam
    B, N = 4, 1024
    opt = _model_opt(B, N)
    A = BatchAssembler(_synthetic((1200,) * 10, seed=3), opt, "train", "modelnet", seed=1)
    ctx = ops.precision("bf16") if precision == "bf16" else ops.precision(ops.POINTMLP_PRECISION)
    with ctx:
        enc, cls = NW.Encoder(opt), NW.Classifier(opt)
        synth.fill_state_dict_(enc.state_dict(), 0)
        synth.fill_state_dict_(cls.state_dict(), 1)
        enc.to(DEV).train()
        cls.to(DEV).train()
        oe, oc = FusedAdam(enc.parameters(), lr=1e-3), FusedAdam(cls.parameters(), lr=1e-3)
        m = _SetInput(DEV)
        losses = []
        for i, batch in enumerate(A.epoch(0, B)):
            if i == 3:
                break
            m.set_input(*batch)
            feat = enc(m.pc, m.sn, m.input_node, m.input_node_knn_I, True, 0)
            score = cls(feat, 0)
            enc.zero_grad(set_to_none=True)
            cls.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(score, m.label)
            loss.backward()
            oe.step()
            oc.step()
            losses.append(loss.detach())
        torch.cuda.synchronize()
    assert len(losses) == 3 and all(torch.isfinite(v).item() for v in losses)
    # an epoch visits every cloud once; another epoch is another permutation
    sizes = [b[0].shape[0] for b in A.epoch(1, 3)]
    assert sizes == [3, 3, 3, 1] and A.batches_per_epoch(3) == 4


def test_test_mode_forward_equals_forward_on_gathered_points():
    from models import networks as NW
    from sonet_hip import synth
    from sonet_hip.batch import BatchAssembler
    B, N = 3, 512
    opt = _model_opt(B, N)
    A = BatchAssembler(_synthetic((700, 600, 900), seed=4), opt, "test", "modelnet", seed=2)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), 0)
    synth.fill_state_dict_(cls.state_dict(), 1)
    enc.to(DEV).eval()
    cls.to(DEV).eval()
    (pc, sn, label, node, knn), raw = A.batch_with_draws([2, 0, 1], 6)
    ch = raw["chosen"]
    c = A.clouds
    pc2 = c.src[:3][:, ch].permute(1, 0, 2).contiguous()
    sn2 = c.src[3:][:, ch].permute(1, 0, 2).contiguous()
    node2 = c.nodes[torch.tensor([2, 0, 1], device=DEV)].transpose(1, 2).contiguous()
    from sonet_hip import ops
    knn2 = ops.knn_self(node2, 9)
    with torch.no_grad():
        s1 = cls(enc(pc, sn, node, knn, False))
        s2 = cls(enc(pc2, sn2, node2, knn2, False))
    torch.cuda.synchronize()
    assert torch.equal(pc, pc2) and torch.equal(node, node2) and torch.equal(knn, knn2)
    torch.testing.assert_close(s1, s2, rtol=1e-5, atol=1e-6)
