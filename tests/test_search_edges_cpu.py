"""The edge inputs of tests/edge_clouds.py, checked without a GPU: the C oracle (oracle/sonet_oracle.c) equals the numpy restatement of
the searches on every family, the families have the properties they are built for (conditions on the INPUTS: a generator that misses
one is wrong), and the contract for distances that are not finite is pinned on the oracle.  tests/test_gpu_search_edges.py then holds
the HIP kernels to the same references."""
import numpy as np
import pytest

import edge_clouds as E
from oracle import cpu_oracle as O


def _check_som(x, node, k):
    ref_idx, ref_cnt, ref_rm = E.som_topk(x, node, k)
    idx, cnt, rm = O.som_query_topk(x, node, k)
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(cnt, ref_cnt)
    np.testing.assert_array_equal(rm, ref_rm)
    return idx


def _check_group(x, idx, M, k):
    """O.som_group against float64 numpy: cluster mean = sum / (count + 1e-5) (count + 1e-5 and the division in float32)."""
    B, _, N = x.shape
    som_node, centers, xd = O.som_group(x, idx, M, k)
    xs = np.concatenate([x] * k, axis=2).astype(np.float64)
    for b in range(B):
        cnt = np.bincount(idx[b], minlength=M)
        s = np.stack([np.bincount(idx[b], weights=xs[b, c], minlength=M) for c in range(3)])
        mean = (s.astype(np.float32) / (cnt.astype(np.float32) + np.float32(1e-5))).astype(np.float32)
        np.testing.assert_allclose(som_node[b], mean, rtol=2e-7, atol=0)
        np.testing.assert_array_equal(centers[b], som_node[b][:, idx[b]])
        np.testing.assert_array_equal(xd[b], np.concatenate([x[b]] * k, axis=1) - centers[b])


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("case", E.LATTICE_CASES, ids=lambda c: "B%d_N%d_M%d_k%d_q%d" % c)
def test_lattice_clouds_tie_and_the_oracle_orders_them_by_id(case):
    x, node, k = E.lattice_case(case)
    share = E.tie_share(E.dist_f32(x, node), k)
    print("lattice %s: tie share %.3f" % (case, share))
    assert share >= 0.5
    idx = _check_som(x, node, k)
    _check_group(x, idx, node.shape[2], k)


# ------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("case", E.NEAR_TIE_CASES, ids=lambda c: "B%d_M%d_k%d_s%d" % c)
def test_near_tie_clouds_reach_both_paths_of_the_packed_key_selection(case):
    """At the id width the dispatcher picks for M: the exact redo is needed for >= 20 % of the points and not needed for >= 20 %; among
    the former the keys alone WOULD pick other ids than the exact order, both inside the list and through its guard entry (so a selection
    that dropped either check would emit other ids on these inputs); groups placed behind slot k do not ask for a redo."""
    x, node, k, kinds = E.near_tie_case(case)
    M = node.shape[2]
    IB = E.key_bits(M)
    d = E.dist_f32(x, node)
    redo = E.needs_exact_redo(d, k, IB)
    print("near ties %s: IB %d, redo share %.3f" % (case, IB, redo.mean()))
    assert redo.mean() >= 0.2 and (~redo).mean() >= 0.2
    assert not redo[kinds == 3].any() and redo[kinds == 2].all() and redo[kinds == 1].all()
    idx = _check_som(x, node, k)
    B, _, N = x.shape
    exact = idx.reshape(B, k, N).transpose(0, 2, 1)
    by_keys = E.key_order_topk(d, k, IB)
    wrong = (by_keys != exact).any(axis=2)
    assert not wrong[~redo].any()                                     # the fast path is right wherever the kernel takes it
    # the keys alone misorder some points of the "across the last slot" kind: only the guard entry t[k] sees those ...
    hi = E._smallest_keys(d, k, IB) & ~np.uint32((1 << IB) - 1)
    inner = (hi[..., :k - 1] == hi[..., 1:k]).any(axis=-1) if k > 1 else np.zeros_like(redo)
    assert (wrong & ~inner).sum() >= 3
    if k > 1:                                                          # ... and some inside the list
        assert (wrong & inner).sum() >= 3
    _check_group(x, idx, M, k)


# ------------------------------------------------------------------------------------------ C
_OCC = E.occupancy_cases()


@pytest.mark.parametrize("i", range(len(_OCC)), ids=[c[0] for c in _OCC])
def test_occupancy_and_size_edges_on_the_oracle(i):
    name, x, node, k = _OCC[i]
    idx = _check_som(x, node, k)
    M = node.shape[2]
    cnt = np.stack([np.bincount(r, minlength=M) for r in idx])
    if name.startswith("one_node") and k == 1:
        assert ((cnt > 0).sum(1) == 1).all()                          # M - 1 empty nodes
    if name.startswith("coincide"):
        assert ((cnt > 0).sum(1) == k).all() and cnt.max() == x.shape[2]
    _check_group(x, idx, M, k)


def test_case_lists_cover_the_sizes_they_promise():
    shapes = [(x.shape[0], x.shape[2], node.shape[2], k) for _, x, node, k in _OCC]
    assert {1, 2, 511, 512, 513, 1023, 1025} <= {s[1] for s in shapes}
    assert {1, 4, 9, 36, 63, 65, 100, 1024} <= {s[2] for s in shapes}
    assert {1, 2, 3, 4} <= {s[3] for s in shapes} and any(s[2] == s[3] for s in shapes)
    assert any(s[0] == 1 for s in shapes) and any(s[0] > 1 and s[0] % 2 for s in shapes)
    assert any(s[2] % 8 and s[2] > 8 for s in shapes)


# ------------------------------------------------------------------------------------------ D
def _check_nonfinite_contract(x, node, k, idx, cnt, rm):
    d = E.dist_f32(x, node)
    B, N, M = d.shape
    slots = idx.reshape(B, k, N).transpose(0, 2, 1)                    # B x N x k
    fin = np.isfinite(d)
    short = 0
    for b in range(B):
        for n in range(N):
            ids = slots[b, n]
            assert len(set(ids.tolist())) == k                         # k DISTINCT nodes
            f = np.flatnonzero(fin[b, n])
            nf = min(k, len(f))
            order = f[np.lexsort((f, d[b, n, f]))][:nf]                 # finite distances first, ascending (d, id)
            np.testing.assert_array_equal(ids[:nf], order)
            rest = np.flatnonzero(~fin[b, n])[:k - nf]                  # then the lowest ids among the others
            np.testing.assert_array_equal(ids[nf:], rest)
            short += nf < k
    np.testing.assert_array_equal(cnt, np.stack([np.bincount(r, minlength=M) for r in idx]))
    np.testing.assert_array_equal(rm, (cnt > 0).astype(np.int32))
    return short


_OVF = E.overflow_cases()
_NAN = E.nan_cases()


@pytest.mark.parametrize("i", range(len(_OVF)), ids=[c[0] for c in _OVF])
def test_overflowing_distances_contract_on_the_oracle(i):
    """Fewer than k finite distances: finite ones first in ascending (d, id) order, then DISTINCT ids of the nodes at a non-finite
    distance, lowest first (what torch.topk gives the reference); count is the histogram of the emitted ids."""
    name, x, node, k = _OVF[i]
    idx, cnt, rm = O.som_query_topk(x, node, k)
    assert np.isfinite(x).all() and np.isfinite(node).all()
    short = _check_nonfinite_contract(x, node, k, idx, cnt, rm)
    assert short >= 9                                                  # the far points of at least one cloud
    _check_som(x, node, k)


@pytest.mark.parametrize("i", range(len(_NAN)), ids=[c[0] for c in _NAN])
def test_nan_distances_order_as_infinity_on_the_oracle(i):
    name, x, node, k = _NAN[i]
    idx, cnt, rm = O.som_query_topk(x, node, k)
    assert _check_nonfinite_contract(x, node, k, idx, cnt, rm) >= 10
    _check_som(x, node, k)


def test_a_nan_entry_does_not_block_the_finite_candidates_behind_it():
    x = np.zeros((1, 3, 1), np.float32)
    node = np.array([[[np.nan, 5.0, 1.0, 2.0], [0, 0, 0, 0], [0, 0, 0, 0]]], np.float32)
    idx, cnt, _ = O.som_query_topk(x, node, 3)
    assert idx.tolist() == [[2, 3, 1]] and cnt.tolist() == [[0, 1, 1, 1]]
    assert O.som_query_topk(x, node, 4)[0].tolist() == [[2, 3, 1, 0]]


# ------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("Nq,Nd", E.chamfer_cases())
def test_chamfer_oracle_equals_argmin_on_lattice_clouds(Nq, Nd):
    q, db = E.chamfer_case(Nq, Nd)
    d = E.dist_f32(q, db)
    if Nd > 1 and Nq > 1:
        assert ((d == d.min(axis=2, keepdims=True)).sum(axis=2) > 1).mean() >= 0.25      # tied minima
    np.testing.assert_array_equal(O.chamfer_nn(q, db), E.chamfer_argmin(q, db))
    np.testing.assert_array_equal(O.chamfer_nn(db, q), E.chamfer_argmin(db, q))


def test_knn_self_restatement_on_duplicated_nodes():
    node = E.uniform(1, 8, 3)
    node[:, :, 4:] = node[:, :, :4]
    I = E.knn_self_topk(node, 3)
    assert I[0, 5, 0] == 1 and I[0, 5, 1] == 5                          # a duplicate's first neighbour is its lower-id twin, not itself
    assert (I[0, :4, 0] == np.arange(4)).all()
