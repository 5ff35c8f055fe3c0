"""The distance-search kernels (som_assign_keys, som_assign_rank + som_sort_fill2, knn_self, chamfer_nn) on the edge inputs of
tests/edge_clouds.py: lattices full of exact ties, near ties below the bits the packed keys keep, degenerate occupancy and sizes,
distances that overflow, Chamfer sizes around the tile / pair / workgroup edges.  The reference is always the CPU oracle or the numpy
restatement of the search (tests/test_search_edges_cpu.py shows that the two agree and that the inputs have the properties they are
built for), never another HIP kernel.  Index outputs are exact; float outputs use the bounds of the tests they extend.
(The insertion-list kernel som_assign_kernel is only dispatched by the variants build: tests/variants/variants_gpu.py runs it on the same
inputs.)"""
from argparse import Namespace

import numpy as np
import pytest
import torch

import edge_clouds as E
from conftest import assert_close_rms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).contiguous()


def _finite_som_cases():
    out = [("lattice_B%d_N%d_M%d_k%d_q%d" % c,) + E.lattice_case(c) for c in E.LATTICE_CASES]
    out += [("near_ties_B%d_M%d_k%d_s%d" % c,) + E.near_tie_case(c)[:3] for c in E.NEAR_TIE_CASES]
    return out + E.occupancy_cases() + E.overflow_cases()


SOM_CASES = _finite_som_cases()
NAN_CASES = E.nan_cases()


def _lexsorted_columns(cols, ids):
    """cols 6 x L, ids L -> cols with every node's run sorted by its six values (a canonical form of the per-node multiset)."""
    o = np.lexsort(tuple(cols[c] for c in range(5, -1, -1)) + (ids,))
    return cols[:, o]


def _check_assign(a, ref_idx, ref_cnt, i64=True):
    np.testing.assert_array_equal(a.min_idx_i32.cpu().numpy(), ref_idx.astype(np.int32))
    if i64:
        np.testing.assert_array_equal(a.min_idx_i64.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(a.count.cpu().numpy(), ref_cnt)


def _check_sorted_stage(a, g, x, sn, k, ref_idx, ref_cnt, ref_rm, node_ref, floats=True):
    B, _, N = x.shape
    kN = k * N
    _check_assign(a, ref_idx, ref_cnt)
    np.testing.assert_array_equal(g["row_max"].cpu().numpy(), ref_rm)
    np.testing.assert_array_equal(g["node_off"].cpu().numpy(), np.cumsum(ref_cnt, axis=1) - ref_cnt)
    ids = g["ids_sorted"].cpu().numpy()
    assert ids.shape == (B, kN) and (np.diff(ids, axis=1) >= 0).all()
    np.testing.assert_array_equal(ids, np.sort(ref_idx, axis=1).astype(np.int32))
    som_node = g["som_node"].cpu().numpy()
    if not floats:
        return
    assert_close_rms(som_node, node_ref, 1e-6, "som_node")
    xa = g["x_aug_sorted"].cpu().numpy()
    p0 = g["pos0"].cpu().numpy()
    for b in range(B):
        # the sorted copy, built on the host from the ORACLE's ids: column j = (x[n] - mean[id_j], sn[n]), one float32 subtraction.
        # The means are the RUN's own som_node (held to the oracle's within 1e-6 just above): the comparison has to be exact.
        host = np.concatenate([np.concatenate([x[b]] * k, axis=1) - som_node[b][:, ref_idx[b]], np.concatenate([sn[b]] * k, axis=1)], axis=0)
        np.testing.assert_array_equal(_lexsorted_columns(xa[b], ids[b]), _lexsorted_columns(host, ref_idx[b]))
        assert ids[b, p0[b]] == ref_idx[b, 0]                           # pos0 = the sorted position of original copy 0
        np.testing.assert_array_equal(xa[b, 3:, p0[b]], sn[b, :, 0])


def _knn_reference(node_mean, I, K):
    """KNNModule's neighbourhood centres ("avg": sequential float32 sum / K) from the means."""
    B, _, M = node_mean.shape
    nb = np.take_along_axis(node_mean[:, :, None, :].repeat(M, 2), I[:, None, :, :K].repeat(3, 1), axis=3)    # B x 3 x M x K
    s = np.zeros((B, 3, M), np.float32)
    for q in range(K):
        s = s + nb[..., q]
    return s / np.float32(K)


@pytest.mark.parametrize("i", range(len(SOM_CASES)), ids=[c[0] for c in SOM_CASES])
def test_som_assignment_on_edge_clouds(i):
    """ops.som_assign (+ som_group) and ops.som_assign_sort -- plain, deterministic, with the kNN rider -- against the oracle: node ids
    (both widths), counts, row_max and node offsets exact; means, centres and de-centred points within 1e-6; the sorted copy is sorted,
    holds per node exactly the columns the oracle's ids put there (de-centred with the run's own means), and pos0 points at copy 0; the deterministic sort repeats bit for
    bit; the rider's records are those of ops.knn_stage_prepare on the oracle's means."""
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    name, x, node, k = SOM_CASES[i]
    B, _, N = x.shape
    M = node.shape[2]
    sn = E.normals(B, N, 99 + N)
    ref_idx, ref_cnt, ref_rm = O.som_query_topk(x, node, k)
    node_ref, ctr_ref, xd_ref = O.som_group(x, ref_idx, M, k)
    xg, sng, nodeg = cu(x), cu(sn), cu(node)
    a = ops.som_assign(xg, nodeg, k, want_i64=True)
    _check_assign(a, ref_idx, ref_cnt)
    g = ops.som_group(xg, sng, a, want_centers=True, want_decentered=True)
    # (On the overflow cases the rel-rms bounds below are set by the 2e19 entries and say little about the ordinary nodes: the exact
    #  ids, counts, row_max, node offsets and the exact sorted copy carry those cases.)
    np.testing.assert_array_equal(g["row_max"].cpu().numpy(), ref_rm)
    assert_close_rms(g["som_node"].cpu().numpy(), node_ref, 1e-6, "som_node")
    assert_close_rms(g["centers"].cpu().numpy(), ctr_ref, 1e-6, "centers")
    assert_close_rms(g["x_decentered"].cpu().numpy(), xd_ref, 1e-6, "x_decentered")
    # the stage the forward runs
    a1, g1 = ops.som_assign_sort(xg, sng, nodeg, k, want_i64=True)
    _check_sorted_stage(a1, g1, x, sn, k, ref_idx, ref_cnt, ref_rm, node_ref)
    a2, g2 = ops.som_assign_sort(xg, sng, nodeg, k, want_i64=True, deterministic=True)
    _check_sorted_stage(a2, g2, x, sn, k, ref_idx, ref_cnt, ref_rm, node_ref)
    a3, g3 = ops.som_assign_sort(xg, sng, nodeg, k, want_i64=True, deterministic=True)
    for key in ("x_aug_sorted", "ids_sorted", "pos0", "som_node", "node_off"):
        assert torch.equal(g2[key], g3[key]), key
    assert torch.equal(a2.min_idx_i32, a3.min_idx_i32)
    K = min(9, M)
    I = E.knn_self_topk(node, K)
    a4, g4 = ops.som_assign_sort(xg, sng, nodeg, k, want_i64=True, knn=(cu(I), K, True))
    _check_sorted_stage(a4, g4, x, sn, k, ref_idx, ref_cnt, ref_rm, node_ref)
    got, ref = g4["knn_prep"], ops.knn_stage_prepare(cu(node_ref), cu(I), K, True)
    assert got["G"] == ref["G"] and got["Lp"] == ref["Lp"]
    np.testing.assert_array_equal(got["rec"][:, 0].cpu().numpy(), ref["rec"][:, 0].cpu().numpy())       # source columns / padding marks
    # The coordinates: the run's means and the oracle's come from float64 sums taken in different orders and rounded to float32, so
    # they may differ by one float32 step (1.2e-7 |mean|); a centre (mean of K means) inherits at most that plus its own rounding, a
    # de-centred coordinate (mean - centre) twice that: 4e-7 max|mean| bounds all three.
    tol = 4e-7 * float(np.abs(node_ref).max())
    assert float((got["center"] - ref["center"]).abs().max()) <= tol
    assert float((got["rec"][:, 1:].contiguous().view(torch.float32) - ref["rec"][:, 1:].contiguous().view(torch.float32)).abs().max()) <= tol
    np.testing.assert_allclose(ref["center"].cpu().numpy(), _knn_reference(node_ref, I, K), rtol=0, atol=tol)


@pytest.mark.parametrize("i", range(len(NAN_CASES)), ids=[c[0] for c in NAN_CASES])
def test_som_assignment_with_nan_coordinates(i):
    """A NaN distance orders as +inf: ids, counts, row_max and node offsets equal the oracle's (the float outputs of the touched nodes
    are NaN on both sides and are not compared)."""
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    name, x, node, k = NAN_CASES[i]
    B, _, N = x.shape
    sn = E.normals(B, N, 98)
    ref_idx, ref_cnt, ref_rm = O.som_query_topk(x, node, k)
    np.testing.assert_array_equal(ref_idx, E.som_topk(x, node, k)[0])
    xg, sng, nodeg = cu(x), cu(sn), cu(node)
    _check_assign(ops.som_assign(xg, nodeg, k, want_i64=True), ref_idx, ref_cnt)
    for det in (False, True):
        a, g = ops.som_assign_sort(xg, sng, nodeg, k, want_i64=True, deterministic=det)
        _check_sorted_stage(a, g, x, sn, k, ref_idx, ref_cnt, ref_rm, None, floats=False)


@pytest.mark.parametrize("N,M,k", E.REJECTED_SHAPES)
def test_unsupported_shapes_are_rejected_before_a_launch(N, M, k):
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    x, sn, node = cu(E.uniform(1, N, 1)), cu(E.normals(1, N, 2)), cu(E.uniform(1, M, 3))
    with pytest.raises(SonetHipError):
        ops.som_assign_sort(x, sn, node, k)
    with pytest.raises(SonetHipError):
        ops.som_assign(x, node, k)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ knn_self
def _knn_self_cases():
    dup = E.uniform(2, 64, 41)
    dup[:, :, 32:] = dup[:, :, :32]
    same = np.zeros((1, 3, 16), np.float32)
    return [("lattice_M64_K9", E.lattice(3, 1, 64, 2, 42)[1], 9, False), ("lattice_M100_K16", E.lattice(2, 1, 100, 4, 43)[1], 16, False),
            ("dup_nodes_M64_K9", dup, 9, False), ("K_eq_M_5", E.uniform(3, 5, 44), 5, True), ("K_eq_M_16_lattice", E.lattice(2, 1, 16, 1, 45)[1], 16, False),
            ("M1", E.uniform(4, 1, 46), 1, True), ("all_equal_M16_K16", same, 16, False), ("uniform_M257_K16", E.uniform(1, 257, 47), 16, True)]


KNN_CASES = _knn_self_cases()


@pytest.mark.parametrize("i", range(len(KNN_CASES)), ids=[c[0] for c in KNN_CASES])
def test_knn_self_is_the_stable_topk_on_tied_nodes(i):
    from sonet_hip import ops
    name, node, K, distinct = KNN_CASES[i]
    got = ops.knn_self(cu(node), K).cpu().numpy()
    np.testing.assert_array_equal(got, E.knn_self_topk(node, K))
    if distinct:                                                        # "itself first" holds only where no node has a twin
        B, _, M = node.shape
        np.testing.assert_array_equal(got[:, :, 0], np.arange(M)[None].repeat(B, 0))


# ------------------------------------------------------------------------------------------ chamfer_nn
@pytest.mark.parametrize("Nq,Nd", E.chamfer_cases())
def test_chamfer_nn_edges(Nq, Nd):
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    q, db = E.chamfer_case(Nq, Nd)
    np.testing.assert_array_equal(ops.chamfer_nn(cu(q), cu(db)).cpu().numpy(), O.chamfer_nn(q, db))
    np.testing.assert_array_equal(ops.chamfer_nn(cu(db), cu(q)).cpu().numpy(), O.chamfer_nn(db, q))


@pytest.mark.parametrize("Nq,Nd", E.chamfer_cases())
def test_chamfer_loss_edges(Nq, Nd):
    """LS.ChamferLoss on the same clouds: the loss within 1e-5 of the float64 brute-force expression, the gradient with respect to the
    predicted cloud equal to float64 autograd with the ORACLE's nearest-neighbour indices forced (1e-5 rel-rms)."""
    from models import losses as LS
    from oracle import cpu_oracle as O
    pred, gt = E.chamfer_case(Nq, Nd)
    crit = LS.ChamferLoss(Namespace(gpu_id=0, device=torch.device(DEV)))
    p = cu(pred).requires_grad_(True)
    loss = crit(p, cu(gt))
    loss.backward()
    p64, g64 = torch.from_numpy(pred).double().requires_grad_(True), torch.from_numpy(gt).double()
    d = torch.cdist(p64.detach().transpose(1, 2), g64.transpose(1, 2))
    ref = (d.min(2).values.pow(2) + 1e-8).sqrt().mean() + (d.min(1).values.pow(2) + 1e-8).sqrt().mean()
    print("chamfer loss (%d, %d): %.9g vs float64 %.9g" % (Nq, Nd, float(loss.detach()), float(ref)))
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref)
    nn_gt = torch.from_numpy(O.chamfer_nn(pred, gt)).long()              # predicted -> nearest gt
    nn_pr = torch.from_numpy(O.chamfer_nn(gt, pred)).long()              # gt -> nearest predicted
    sel_gt = torch.gather(g64, 2, nn_gt.unsqueeze(1).expand(-1, 3, -1))
    sel_pr = torch.gather(p64, 2, nn_pr.unsqueeze(1).expand(-1, 3, -1))
    forced = ((sel_gt - p64).pow(2).sum(1) + 1e-8).sqrt().mean() + ((sel_pr - g64).pow(2).sum(1) + 1e-8).sqrt().mean()
    assert abs(float(forced) - float(ref)) <= 1e-12 * float(ref)
    forced.backward()
    assert_close_rms(p.grad.cpu().numpy(), p64.grad.numpy(), 1e-5, "d loss / d predicted")


# ------------------------------------------------------------------------------------------ downstream: the eval forward
def _opt(B, N, k=3, dropout=0.7):
    return Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                     activation="relu", normalization="batch", dropout=dropout, node_num=64, k=k, som_k=9, som_k_type="avg",
                     bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)


def _one_node_cloud(B, N, seed):
    """All points around node 37, the other 63 nodes far away."""
    node = (E.uniform(B, 64, seed) * np.float32(0.5) + np.float32(5.0)).astype(np.float32)
    node[:, :, 37] = np.array([0.1, 0.2, -0.3], np.float32)
    x = (node[:, :, 37:38] + np.float32(0.05) * E.uniform(B, N, seed + 1)).astype(np.float32)
    return x, node


def _forward_clouds():
    xl, nl = E.lattice(2, 1024, 64, 4, 61)
    xo, no = _one_node_cloud(2, 1200, 62)
    h = E.uniform(2, 513, 63)
    return [("lattice", xl, nl, 3), ("one_node_k1", xo, no, 1), ("one_node_k3", xo, no, 3),
            ("dup_points_N1025", np.concatenate([h, h[:, :, :512]], axis=2), E.uniform(2, 64, 64), 3)]


FWD_CLOUDS = _forward_clouds()


@pytest.mark.parametrize("mode", ["h3", "x3", "f32"])
@pytest.mark.parametrize("i", range(len(FWD_CLOUDS)), ids=[c[0] for c in FWD_CLOUDS])
def test_eval_forward_on_degenerate_clouds(i, mode):
    """The eval Encoder on a lattice cloud, a cloud whose points all fall into one node (k = 1: 63 empty nodes, one segment of N
    columns; k = 3: three segments of N) and a cloud of duplicated points at N = 1025: min_idx exact, the feature within 1e-5 of
    O.encoder_forward."""
    from models import networks as NW
    from oracle import cpu_oracle as O
    from sonet_hip import ops, synth
    name, x, node, k = FWD_CLOUDS[i]
    B, _, N = x.shape
    sn = E.normals(B, N, 65)
    I = E.knn_self_topk(node, 9)
    enc = NW.Encoder(_opt(B, N, k))
    sd = synth.fill_state_dict_(enc.state_dict(), 7)
    cpu_sd = {key: v.clone() for key, v in sd.items()}
    enc.to(DEV).eval()
    with ops.precision(mode), torch.no_grad():
        feat = enc(cu(x), cu(sn), cu(node), cu(I))
    ref = O.encoder_forward(cpu_sd, torch.from_numpy(x), torch.from_numpy(sn), torch.from_numpy(node), torch.from_numpy(I), k=k)
    np.testing.assert_array_equal(enc.min_idx.cpu().numpy(), ref["min_idx"])
    if name == "one_node_k1":
        assert (ref["row_max"].sum(1) == 1).all()
    assert_close_rms(feat.cpu().numpy(), ref["feature"].numpy(), 1e-5, "feature (%s, %s)" % (name, mode))


def test_training_step_on_a_one_node_cloud_is_bit_reproducible():
    """One f32-class training forward + backward on the one-node cloud (every point copy in three segments of N columns), twice: the
    loss and every gradient repeat bit for bit."""
    from models import networks as NW
    from sonet_hip import ops, synth
    B, N = 4, 1025
    x, node = _one_node_cloud(B, N, 71)
    sn = E.normals(B, N, 72)
    I = E.knn_self_topk(node, 9)
    label = torch.tensor([3, 17, 0, 39], device=DEV)
    outs = []
    with ops.precision("h3"):
        for _ in range(2):
            opt = _opt(B, N, dropout=0.0)
            enc, cls = NW.Encoder(opt), NW.Classifier(opt)
            enc.want_first_pn_out = False
            synth.fill_state_dict_(enc.state_dict(), 3)
            synth.fill_state_dict_(cls.state_dict(), 4)
            enc.to(DEV).train()
            cls.to(DEV).train()
            feat = enc(cu(x), cu(sn), cu(node), cu(I), is_train=True, epoch=0)
            loss = torch.nn.functional.cross_entropy(cls(feat, 0), label)
            loss.backward()
            assert np.array_equal(enc.min_idx.cpu().numpy(), E.som_topk(x, node, 3)[0])
            grads = {key: p.grad.clone() for key, p in list(enc.named_parameters()) + list(cls.named_parameters()) if p.grad is not None}
            assert grads and all(bool(torch.isfinite(v).all()) for v in grads.values()) and bool(torch.isfinite(loss))
            outs.append((loss.detach().clone(), grads))
    assert torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1].keys() == outs[1][1].keys()
    for key in outs[0][1]:
        assert torch.equal(outs[0][1][key], outs[1][1][key]), key
