"""SOM trainer on the GPU: sonet_som_train_f32 (csrc/som_train.hip) through ops.som_train, BatchSOM.optimize, build_nodes and the
raw-cloud Encoder.forward -- against the reference's fixtures, a float64 numpy restatement of the iteration, the batch_update loop
and the CPU oracle.  Measured deviations are printed (pytest -s)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import assert_close_rms, golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN_SOM = ("som/som_optimize_8x8_n5000", "som/som_optimize_4x4_n1024", "som/som_optimize_8x8_n40")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).contiguous()


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))


def np_train(x, node0, w, lr):
    """float64 restatement of T iterations (util/som.py:295-352).  The assignment takes the kernel's f32 distance,
    (dx*dx + dy*dy) + dz*dz on the f32-rounded nodes, first minimum; counts, sums, means and the Jacobi update are float64."""
    x = np.asarray(x, np.float32)
    B, _, N = x.shape
    node = np.array(np.broadcast_to(np.asarray(node0, np.float64), (B, 3, np.shape(node0)[-1])))
    M = node.shape[2]
    w = np.asarray(w, np.float64).reshape(len(lr), M, M)
    for t in range(len(lr)):
        for b in range(B):
            nf = node[b].astype(np.float32)
            dx, dy, dz = (x[b, c][:, None] - nf[c][None, :] for c in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            idx = np.argmin(d, axis=1)
            cnt = np.bincount(idx, minlength=M).astype(np.float64)
            s = np.stack([np.bincount(idx, weights=x[b, c].astype(np.float64), minlength=M) for c in range(3)])
            mean = s / (cnt + 1e-5)
            r = (cnt > 0).astype(np.float64)
            # delta_j = sum_i (mean_i - node_j) r_i w_ij lr
            wr = w[t] * r[:, None] * float(np.float32(lr[t]))
            node[b] = node[b] + (mean @ wr - node[b] * wr.sum(0)[None, :])
    return node


def run(x, node0, w, lr):
    from sonet_hip import ops
    lr_t = torch.as_tensor(np.asarray(lr, np.float32)).to(DEV)
    return ops.som_train(cu(np.asarray(x, np.float32)), cu(np.asarray(node0, np.float32)),
                         cu(np.asarray(w, np.float32).reshape(len(lr), *np.shape(w)[1:])), lr_t.contiguous())


# ------------------------------------------------------------------------------------------ the existing batch_update fixture
def test_one_and_six_iterations_from_update_fixture():
    """The schedule of test_batch_som_update_golden (one update at (lr, sigma), five at decayed values) as single launches."""
    from util import som
    g = golden("som_update_b2_n3000")
    s = som.BatchSOM(8, 8, 3, 0, 2)
    sched = [(s.learning_rate, s.sigma)] + [(s.learning_rate / (1 + 2 * it / 5), s.sigma / (1 + 2 * it / 5)) for it in range(5)]
    w = torch.stack([s.get_weighting_matrix(sg).reshape(64, 64) for _, sg in sched]).to(DEV).contiguous()
    lr = torch.tensor([l for l, _ in sched], dtype=torch.float32, device=DEV)
    from sonet_hip import ops
    x, node0 = cu(g["x"]), cu(g["node0"])
    node1 = ops.som_train(x, node0, w[:1].contiguous(), lr[:1].contiguous()).cpu().numpy()
    node6 = ops.som_train(x, node0, w, lr).cpu().numpy()
    print("\nsom_train vs reference fixture: node1 rel-rms %.2e, node6 rel-rms %.2e" % (rel_rms(node1, g["node1"]), rel_rms(node6, g["node6"])))
    assert_close_rms(node1, g["node1"], 1e-5, "nodes after one iteration")
    assert_close_rms(node6, g["node6"], 1e-4, "nodes after six iterations")


# ------------------------------------------------------------------------------------------ BatchSOM.optimize vs the reference
def _nn_dist(x, node):
    d = ((x[:, :, :, None].astype(np.float64) - node[:, :, None, :]) ** 2).sum(1)
    return np.sqrt(d.min(2)).mean(1)


@pytest.mark.parametrize("case", GOLDEN_SOM)
def test_optimize_against_reference_goldens(case):
    from util import som
    g = golden(case)
    x = g["x"]
    s = som.BatchSOM(int(g["rows"]), int(g["cols"]), 3, 0, 1)
    s.max_iteration = int(g["max_iteration"])
    np.testing.assert_array_equal(s.node_init_value.numpy(), g["node_init"])
    s.optimize(cu(x))
    assert s.node.dtype == torch.float32 and s.node.is_contiguous() and tuple(s.node.shape) == g["ref64"].shape
    assert s.batch_size == x.shape[0]
    got = s.node.cpu().numpy()
    ref64 = g["ref64"]
    d_got, d_ref, d_32 = _nn_dist(x, got), _nn_dist(x, ref64), _nn_dist(x, g["ref32"].astype(np.float64))
    for b in range(x.shape[0]):
        err = float(np.sqrt(np.mean((got[b].astype(np.float64) - ref64[b]) ** 2)))
        gate = max(1.5 * float(g["ref32_dev"][b]), 1e-5 * float(np.sqrt(np.mean(ref64[b] ** 2))))
        dist_rel = abs(d_got[b] - d_ref[b]) / d_ref[b]
        # (12 distinct points: nodes settle on them, the mean distance is ~1e-4 and the reference's own float32 run is 4.6e-4
        #  off in it -- there the gate is 1.5 x that measured spread, as for the nodes)
        dist_gate = max(1e-4, 1.5 * abs(d_32[b] - d_ref[b]) / d_ref[b])
        print("\n%s cloud %d: rms(got-ref64) %.2e = %.2f x gate (ref32_dev %.2e), mean nn distance rel %.2e (gate %.1e)"
              % (case, b, err, err / gate, g["ref32_dev"][b], dist_rel, dist_gate))
        assert err <= gate, (case, b, err, gate)
        assert dist_rel <= dist_gate, (case, b, dist_rel, dist_gate)


def test_node_init_and_optimize_run_here():
    """No reference checkout on this machine: the initialiser is the repository's own."""
    from util import som
    g = golden("som/som_optimize_8x8_n5000")
    s = som.BatchSOM(8, 8, 3, 0, 3)
    s.node_init(3)
    np.testing.assert_array_equal(s.node.cpu().numpy(), np.broadcast_to(g["node_init"], (3, 3, 64)))
    s.optimize(cu(g["x"][:3]))
    assert tuple(s.node.shape) == (3, 3, 64) and torch.isfinite(s.node).all()


# ------------------------------------------------------------------------------------------ determinism
def test_bit_identical_runs_and_independent_of_batch():
    from util import som
    g = golden("som/som_optimize_8x8_n5000")
    x = g["x"]
    s = som.BatchSOM(8, 8, 3, 0, 1)
    lr, w, node0 = s.train_tables(DEV)
    from sonet_hip import ops
    a = ops.som_train(cu(x), node0, w, lr)
    b = ops.som_train(cu(x), node0, w, lr)
    assert torch.equal(a, b)
    rng = np.random.RandomState(3)
    big = rng.uniform(-1, 1, (300, 3, 5000)).astype(np.float32)
    pos = [0, 137, 255, 299]                                    # > 256 clouds: several per CU, and the grid's last ones
    for p, c in zip(pos, range(4)):
        big[p] = x[c]
    out = ops.som_train(cu(big), node0, w, lr)
    for p, c in zip(pos, range(4)):
        alone = ops.som_train(cu(x[c:c + 1]), node0, w, lr)
        assert torch.equal(out[p], alone[0]), (p, c)
        assert torch.equal(out[p], a[c])


# ------------------------------------------------------------------------------------------ edge cases vs the float64 restatement
def _tables(rows, cols, max_iteration):
    from util import som
    s = som.BatchSOM(rows, cols, 3, 0, 1)
    s.max_iteration = max_iteration
    lr, w, _ = s.train_tables("cpu")
    return w.numpy(), lr.numpy()


EDGE = ["n1", "n_lt_m", "identical", "m16", "m121", "rows_ne_cols", "n2p17"]


@pytest.mark.parametrize("case", EDGE)
def test_edge_cases_vs_float64_restatement(case):
    rng = np.random.RandomState(EDGE.index(case) + 40)
    rows, cols, N, B, mi = 8, 8, 1000, 2, 6
    if case == "n1":
        N = 1
    elif case == "n_lt_m":
        N = 37
    elif case == "m16":
        rows, cols = 4, 4
    elif case == "m121":
        rows, cols, N = 11, 11, 3000
    elif case == "rows_ne_cols":
        rows, cols, N = 4, 6, 2000
    elif case == "n2p17":
        N, B, mi = 1 << 17, 1, 3
    M = rows * cols
    w, lr = _tables(rows, cols, mi)
    x = rng.uniform(-1, 1, (B, 3, N)).astype(np.float32)
    if case == "identical":
        x[:] = x[:, :, :1]
    node0 = rng.uniform(-0.9, 0.9, (B, 3, M)).astype(np.float32)
    got = run(x, node0, w, lr).cpu().numpy()
    ref = np_train(x, node0, w, lr)
    err = rel_rms(got, ref)
    print("\n%s (B=%d N=%d M=%d T=%d): rel-rms vs float64 %.2e" % (case, B, N, M, len(lr), err))
    assert err <= 1e-5, (case, err)


def test_ties_go_to_the_lowest_node_id():
    """Points exactly on nodes, duplicated nodes and a point equidistant from two nodes."""
    M = 16
    node0 = np.zeros((1, 3, M), np.float32)
    node0[0, 0] = np.arange(M, dtype=np.float32) * 0.25 - 2.0
    node0[0, :, 5] = node0[0, :, 4]                     # a duplicated node: its points belong to node 4
    node0[0, :, 9] = node0[0, :, 8]
    pts = [node0[0, :, m] for m in range(M)] + [np.array([-1.875, 0, 0], np.float32)]   # the last: exactly between nodes 0 and 1
    x = np.stack(pts, axis=1)[None].astype(np.float32)
    w = np.eye(M, dtype=np.float32)[None]               # no neighbourhood: node j moves to its own cluster mean
    lr = np.array([1.0], np.float32)
    got = run(x, node0, w, lr).cpu().numpy()
    ref = np_train(x, node0, w, lr)
    assert rel_rms(got, ref) <= 1e-6
    for empty in (5, 9):                                # the higher id of a duplicate pair got no point and did not move
        assert np.array_equal(got[0, :, empty], node0[0, :, empty])
    # node 0 took the equidistant point: its mean is ((-2) + (-1.875)) / 2, node 1 kept its own point only
    assert abs(got[0, 0, 0] - (-1.9375)) < 2e-5 and abs(got[0, 0, 1] - (-1.75)) < 1e-4


def test_shared_node0_and_zero_iterations():
    from sonet_hip import ops
    rng = np.random.RandomState(9)
    x = cu(rng.uniform(-1, 1, (5, 3, 700)).astype(np.float32))
    w, lr = _tables(8, 8, 6)
    node_s = rng.uniform(-1, 1, (3, 64)).astype(np.float32)
    a = ops.som_train(x, cu(node_s), cu(w), cu(lr))
    b = ops.som_train(x, cu(np.broadcast_to(node_s, (5, 3, 64))), cu(w), cu(lr))
    assert torch.equal(a, b)
    node_b = rng.uniform(-1, 1, (5, 3, 64)).astype(np.float32)
    empty_w, empty_lr = torch.empty((0, 64, 64), device=DEV), torch.empty((0,), device=DEV)
    assert torch.equal(ops.som_train(x, cu(node_b), empty_w, empty_lr).cpu(), torch.from_numpy(node_b))
    assert torch.equal(ops.som_train(x, cu(node_s), empty_w, empty_lr).cpu(), torch.from_numpy(np.broadcast_to(node_s, (5, 3, 64)).copy()))


# ------------------------------------------------------------------------------------------ the batch_update loop (fallback path)
def test_optimize_agrees_with_batch_update_loop():
    from util import som
    g = golden("som/som_optimize_8x8_n5000")
    x = cu(g["x"])
    s = som.BatchSOM(8, 8, 3, 0, 4)
    s.optimize(x)
    one = s.node.clone()
    s.node_init(4)
    for lr, sigma in zip(*s.train_schedule()):
        s.batch_update(x, lr, sigma)
    err = rel_rms(one.cpu().numpy(), s.node.cpu().numpy())
    print("\noptimize (one launch) vs batch_update loop: rel-rms %.2e" % err)
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------ raw-cloud Encoder.forward
def _opt(B, N):
    return Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                     activation="relu", normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg",
                     bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)


def test_encoder_forward_builds_nodes_from_raw_clouds():
    from models import networks as NW
    from oracle import cpu_oracle as O
    from sonet_hip import ops, synth
    from util import som
    B, N = 2, 1024
    opt = _opt(B, N)
    enc = NW.Encoder(opt)
    sd = synth.fill_state_dict_(enc.state_dict(), 7)
    sd_cpu = {k: v.clone() for k, v in sd.items()}
    enc.to(DEV)
    inp = synth.make_inputs(B, N, seed=5)
    pc, sn = inp["pc"].to(DEV), inp["sn"].to(DEV)
    node = som.build_nodes(pc)
    knn = ops.knn_self(node, opt.som_k)
    # eval / inference
    enc.eval()
    with torch.no_grad():
        a = enc(pc, sn, None, None).clone()
        ia = enc.min_idx.clone()
        b = enc(pc, sn, node, knn).clone()
    assert torch.equal(a, b) and torch.equal(ia, enc.min_idx)
    ref = O.encoder_forward(sd_cpu, pc.cpu(), sn.cpu(), node.cpu(), knn.cpu())
    assert np.array_equal(enc.min_idx.cpu().numpy(), ref["min_idx"])
    got, exp = a.cpu().double().numpy(), ref["feature"].double().numpy()
    bound = 1e-5 * np.maximum(np.abs(exp), np.sqrt(np.mean(exp ** 2)))
    print("\nraw-cloud encoder vs CPU oracle: feature error %.2f x bound" % (np.abs(got - exp) / bound).max())
    assert (np.abs(got - exp) <= bound).all()
    # a training forward (BatchNorm batch statistics; same starting state for both calls)
    enc.train()
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    ta = enc(pc, sn, None, None, is_train=True).detach().clone()
    enc.load_state_dict(state)
    tb = enc(pc, sn, node, knn, is_train=True).detach().clone()
    assert torch.equal(ta, tb)
