"""Retrieval lists on the GPU (sonet_retrieval_lists_f32, ops.retrieval_lists, sonet_hip.retrieval): every output bit for bit against the
numpy restatement of the contract (tests/retrieval_ref.py) -- on the fixtures of the live reference (also held to the stored reference
lists by the rules of that module), on class sizes around the wave, the workgroup, the `top` cut and the LDS chunk, on every feature
width class, on special values and bad inputs; ShapeRetrieval and retrieve_shrec end to end.  Every case is small."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import golden
import retrieval_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = {"continuous_3_classes": True, "truncated_class": True, "ties_quantised": False}


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def run(feat, labels=None, ids=None, query=None, top=1000, n_label=None):
    from sonet_hip import ops
    return ops.retrieval_lists(dev(feat), dev(labels), dev(ids), dev(query, np.int32), top, n_label, want_pos=True)


def assert_bits(r, want, what=""):
    """nn_id, nn_pos, the bits of nn_dist, count, labels and bad: all equal."""
    assert np.array_equal(r.count.cpu().numpy(), want["count"]), what
    assert np.array_equal(r.labels.cpu().numpy(), want["labels"]), what
    assert int(r.bad.cpu()[0]) == want["bad"], (what, int(r.bad.cpu()[0]), want["bad"])
    assert np.array_equal(r.nn_pos.cpu().numpy(), want["nn_pos"]), what
    assert np.array_equal(r.nn_id.cpu().numpy(), want["nn_id"]), what
    got = r.nn_dist.cpu().numpy().view(np.uint32)
    ref = want["nn_dist"].view(np.uint32)
    assert np.array_equal(got, ref), "%s: %d distances differ in their bits" % (what, int((got != ref).sum()))


def both(feat, labels=None, ids=None, query=None, top=1000, n_label=None, what=""):
    r = run(feat, labels, ids, query, top, n_label)
    want = R.retrieval_lists(feat, labels, ids, query, top, n_label)
    assert_bits(r, want, what)
    return r, want


def chunk_keys():
    from sonet_hip import _lib
    return _lib.load().sonet_retrieval_chunk_keys()


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", sorted(CASES))
def test_fixtures_bit_for_bit_and_against_the_reference_lists(case):
    g = golden("retrieval/" + case)
    n_label = int(g["labels"].max()) + 1
    r, want = both(g["feat"], g["labels"], g["model_ids"], g["query"], 1000, n_label, case)
    positions, excused, worst = R.check_fixture(g, r.nn_id.cpu().numpy(), r.nn_dist.cpu().numpy(), r.count.cpu().numpy(), CASES[case], case)
    print("%s: %d positions, %d excused, worst distance error %.3f of its allowance" % (case, positions, excused, worst))
    both(g["feat"], g["labels"], g["model_ids"], None, 1000, n_label, case + " every query")


# ------------------------------------------------------------------------------------------------------------ class sizes
def _sizes():
    return [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001, 1023, 1024, 1025, "CK-1", "CK", "CK+1", "2CK-top+1"]


@pytest.mark.parametrize("K", _sizes())
def test_class_sizes_around_the_wave_the_cut_and_the_chunk(K):
    CK, top = chunk_keys(), 1000
    K = {"CK-1": CK - 1, "CK": CK, "CK+1": CK + 1, "2CK-top+1": 2 * CK - top + 1}.get(K, K)
    g = np.random.RandomState(K)
    feat, lab, query = R.sized_class(g, K, 37, 3)
    assert len(query) <= 4 and (lab == 0).sum() == K
    r, want = both(feat, lab, None, query, top, 2, "K=%d" % K)
    assert (want["count"] == min(K, top)).all()
    feat, lab, query = R.sized_class(g, K, 5, 2, quantum=1.0)          # exact ties across the cut and the chunk borders
    both(feat, lab, None, query, top, 2, "K=%d quantised" % K)


# ------------------------------------------------------------------------------------------------------------ other parameters
@pytest.mark.parametrize("D", [1, 3, 55, 64, 65, 1024])
def test_feature_widths_with_given_and_derived_labels(D):
    g = np.random.RandomState(D)
    feat, lab, ids = R.make_inputs(g, 150, D, (0.6, 0.3, 0.1))
    both(feat, lab, ids, None, 1000, 3, "D=%d given" % D)
    r, want = both(feat, None, ids, None, 1000, None, "D=%d derived" % D)
    assert np.array_equal(want["labels"], torch.max(torch.from_numpy(feat), dim=1)[1].numpy())
    if D > 1:
        assert len(set(want["labels"].tolist())) > 1


@pytest.mark.parametrize("top", [1, 7, 1000, 1024])
def test_list_lengths(top):
    g = np.random.RandomState(top)
    feat, lab, query = R.sized_class(g, 1100, 40, 4)
    query = np.concatenate([query, np.nonzero(lab == 1)[0][:2].astype(np.int32)])
    r, want = both(feat, lab, None, query, top, 2, "top=%d" % top)
    assert want["count"].tolist() == [min(1100, top)] * 3 + [min(40, top)] * 2
    assert (r.nn_id.cpu().numpy()[3:, 40:] == -1).all()


@pytest.mark.parametrize("n_label", [1, 55, 65535])
def test_label_ranges_with_empty_classes(n_label):
    g = np.random.RandomState(n_label)
    feat = (g.normal(size=(200, 5)) * 3).astype(np.float32)
    used = np.unique(g.randint(0, n_label, 6))
    used[-1] = n_label - 1                                             # the last class is in use; most of the others are empty
    lab = used[g.randint(0, len(used), 200)].astype(np.int64)
    both(feat, lab, None, None, 1000, n_label, "n_label=%d" % n_label)


# ------------------------------------------------------------------------------------------------------------ special inputs
def test_identical_shapes_and_duplicates_of_the_query():
    g = np.random.RandomState(1)
    feat = np.tile((g.normal(size=(1, 6)) * 3).astype(np.float32), (300, 1))
    lab = (np.arange(300) % 3 == 0).astype(np.int64)
    r, want = both(feat, lab, None, None, 1000, 2, "identical")
    d = r.nn_dist.cpu().numpy()
    assert (d[want["nn_pos"] >= 0].view(np.uint32) == 0).all()          # every distance is +0 ...
    assert (np.diff(want["nn_id"][0, :want["count"][0]]) > 0).all()     # ... and the order is the gallery index
    feat, lab, ids = R.make_inputs(g, 120, 7, (0.5, 0.5))
    feat[5::11] = feat[5]                                                # duplicates of shape 5, in both classes
    both(feat, lab, ids, [5, 16, 0], 1000, 2, "duplicates")


def test_special_values_sort_as_the_contract_says():
    g = np.random.RandomState(2)
    feat = R.special_values(g, 130, 5)
    r, want = both(feat, np.zeros(130, np.int64), None, None, 130, 1, "special")
    assert np.isnan(want["nn_dist"]).any() and np.isposinf(want["nn_dist"]).any()
    both(feat, None, None, None, 1000, None, "special, labels derived")
    both(R.argmax_rule_inputs(g), None, None, None, 16, None, "arg-max rule rows")


def test_queries_none_subset_repeated_and_offset_views():
    from sonet_hip import ops
    g = np.random.RandomState(4)
    feat, lab, ids = R.make_inputs(g, 90, 9, (0.5, 0.3, 0.2))
    both(feat, lab, None, None, 50, 3, "ids None, query None")
    both(feat, lab, ids, [88, 3, 3, 41, 3], 50, 3, "repeated")
    # 4-byte-offset views of larger buffers (the int64 operands cannot be: their elements are 8 bytes)
    fbuf = torch.zeros(90 * 9 + 3, dtype=torch.float32, device=DEV)
    qbuf = torch.zeros(8, dtype=torch.int32, device=DEV)
    fbuf[1:1 + 90 * 9] = dev(feat).reshape(-1)
    qbuf[1:6] = dev([7, 0, 89, 7, 30], np.int32)
    fv, qv = fbuf[1:1 + 90 * 9].view(90, 9), qbuf[1:6]
    assert fv.data_ptr() % 8 == 4 and qv.data_ptr() % 8 == 4
    r = ops.retrieval_lists(fv, dev(lab), dev(ids), qv, 50, 3, want_pos=True)
    assert_bits(r, R.retrieval_lists(feat, lab, ids, [7, 0, 89, 7, 30], 50, 3), "offset views")
    r = ops.retrieval_lists(fv, dev(lab), dev(ids), [7, 0, 89], 50, 3)             # a host query; no nn_pos asked for
    assert r.nn_pos is None and np.array_equal(r.nn_id.cpu().numpy(), R.retrieval_lists(feat, lab, ids, [7, 0, 89], 50, 3)["nn_id"])


def test_bad_labels_and_bad_queries_are_counted_and_touch_nothing_else():
    g = np.random.RandomState(5)
    feat, lab, ids = R.make_inputs(g, 140, 4, (0.5, 0.3, 0.2))
    clean = R.retrieval_lists(feat, lab, ids, None, 1000, 3)
    lab2 = lab.copy()
    victims = np.nonzero(lab == 0)[0][[0, 3, 9]]
    lab2[victims] = [-1, 3, 2 ** 40]
    r, want = both(feat, lab2, ids, None, 1000, 3, "bad labels")
    assert want["bad"] == 3 and (want["count"][victims] == 0).all() and not np.isin(ids[victims], want["nn_id"]).any()
    untouched = np.nonzero(lab != 0)[0]
    assert np.array_equal(want["nn_id"][untouched], clean["nn_id"][untouched])
    assert np.array_equal(r.nn_dist.cpu().numpy()[untouched].view(np.uint32), clean["nn_dist"][untouched].view(np.uint32))
    # a device query is not read back: the kernel counts the indices outside [0, N) and leaves their rows empty
    q = np.array([0, 140, -1, 139, 2 ** 31 - 1, int(victims[0])], dtype=np.int32)
    r, want = both(feat, lab2, ids, q, 9, 3, "bad queries")
    assert want["bad"] == 6 and want["count"].tolist()[1:3] == [0, 0] and want["count"][4] == want["count"][5] == 0


def test_two_runs_give_identical_bits():
    g = golden("retrieval/ties_quantised")
    a = run(g["feat"], None, g["model_ids"], None, 1000, None)
    b = run(g["feat"], None, g["model_ids"], None, 1000, None)
    torch.cuda.synchronize()
    for name in ("nn_id", "nn_pos", "count", "labels", "bad"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.nn_dist.view(torch.int32), b.nn_dist.view(torch.int32)) and a.nn_id.data_ptr() != b.nn_id.data_ptr()


def test_wrapper_refuses_cuda_tensors_it_cannot_take():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    feat, lab = torch.zeros(6, 4, device=DEV), torch.zeros(6, dtype=torch.int64, device=DEV)
    with pytest.raises(SonetHipError, match="contiguous"):
        ops.retrieval_lists(torch.zeros(4, 6, device=DEV).t(), lab, None, None, 5, 3)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.retrieval_lists(feat, lab.cpu(), None, None, 5, 3)
    with pytest.raises(SonetHipError, match="int32"):
        ops.retrieval_lists(feat, lab, None, torch.zeros(2, dtype=torch.int64, device=DEV), 5, 3)
    with pytest.raises(SonetHipError, match="outside"):
        ops.retrieval_lists(feat, lab, None, [6], 5, 3)


# ------------------------------------------------------------------------------------------------------------ ShapeRetrieval
def test_shape_retrieval_accumulates_and_writes_the_reference_files(tmp_path):
    from sonet_hip import ops
    from sonet_hip.retrieval import ShapeRetrieval
    g = golden("retrieval/truncated_class")
    feat, ids = dev(g["feat"]), dev(g["model_ids"])
    N, D = g["feat"].shape
    acc = ShapeRetrieval(N + 10, D)
    at = 0
    for b in (1, 7, 500, 64, N):                                          # uneven batches
        b = min(b, N - at)
        acc.update(feat[at:at + b], ids[at:at + b])
        at += b
    assert acc.filled == N
    n_label = int(g["labels"].max()) + 1
    got = acc.lists(labels=dev(g["labels"]), n_label=n_label, want_pos=True)
    one = ops.retrieval_lists(feat, dev(g["labels"]), ids, None, 1000, n_label, want_pos=True)
    for name in ("nn_id", "nn_pos", "count", "labels", "bad"):
        assert torch.equal(getattr(got, name), getattr(one, name)), name
    assert torch.equal(got.nn_dist.view(torch.int32), one.nn_dist.view(torch.int32))
    assert acc.write(str(tmp_path)) == N
    qids = g["model_ids"][g["query"]]
    rid, rd, cnt = R.parse_folder(str(tmp_path), qids)
    R.check_fixture(g, rid, rd, cnt, True, "files")
    # derived labels on the continuous fixture's scores: the same as handing the arg-max in
    g = golden("retrieval/continuous_3_classes")
    acc = ShapeRetrieval(len(g["feat"]), 55, top=7)
    acc.update(dev(g["feat"]), dev(g["model_ids"]))
    assert_bits(acc.lists(want_pos=True), R.retrieval_lists(g["feat"], None, g["model_ids"], None, 7, None), "derived")


# ------------------------------------------------------------------------------------------------------------ end to end
def test_retrieve_shrec_end_to_end():
    """41 clouds of 300 points, 256 sampled, 4 x 4 nodes, batches of 8 (the last one short): retrieve_shrec against
    ops.retrieval_lists on the scores and indices of hand-run per-batch forwards; labels against torch.max on the CPU."""
    from models import networks as NW
    from sonet_hip import ops, retrieval, synth
    from sonet_hip._lib import SonetHipError
    from sonet_hip.batch import BatchAssembler, DeviceClouds
    S, n, N, M, BS = 41, 300, 256, 16, 8
    g = np.random.RandomState(41)
    pts = [g.normal(size=(n, 3)).astype(np.float32) for _ in range(S)]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = np.stack([p[g.choice(n, M, replace=False)] for p in pts]).astype(np.float32)
    opt = Namespace(gpu_id=0, device=DEV, batch_size=BS, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                    normalization="batch", dropout=0.7, node_num=M, k=3, som_k=9, som_k_type="center", bn_momentum=0.1,
                    bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=55, rot_horizontal=False, rot_perturbation=False,
                    translation_perturbation=False, pretrain=None, pretrain_lr_ratio=1)
    enc, cls = NW.Encoder(opt), NW.Classifier(opt)
    synth.fill_state_dict_(enc.state_dict(), 5)
    synth.fill_state_dict_(cls.state_dict(), 6)
    enc.to(DEV).train()
    cls.to(DEV).train()                                                   # retrieve_shrec itself must switch to eval mode
    clouds = DeviceClouds(pts, nrm, g.randint(0, 55, S), nodes=nodes, device=DEV)
    A = BatchAssembler(clouds, opt, "test", "shrec", seed=3)
    with ops.kernel_timing() as rec:
        acc = retrieval.retrieve_shrec(enc, cls, A, BS, top=1000)
        torch.cuda.synchronize()
    assert not enc.training and not cls.training and acc.filled == S
    assert rec.summary()["retrieval_lists"]["count"] == 1
    scores, index, sizes = [], [], []
    with torch.no_grad():
        for pc, sn, label, node, knn, idx in A.epoch(0, BS, shuffle=False):
            scores.append(cls(enc(pc, sn, node, knn)).float())
            index.append(idx)
            sizes.append(pc.shape[0])
    assert sizes == [8, 8, 8, 8, 8, 1]
    score, index = torch.cat(scores).contiguous(), torch.cat(index).contiguous()
    assert tuple(score.shape) == (S, 55) and index.tolist() == list(range(S))
    want = ops.retrieval_lists(score, None, index, None, 1000, None)
    got = acc.lists()
    for name in ("nn_id", "count", "labels", "bad"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert torch.equal(got.nn_dist.view(torch.int32), want.nn_dist.view(torch.int32))
    assert np.array_equal(got.labels.cpu().numpy(), torch.max(score.cpu(), dim=1)[1].numpy())
    assert int(got.bad.cpu()[0]) == 0 and int(got.count.sum().cpu()) >= S
    assert_bits(ops.retrieval_lists(score, None, index, None, 1000, None, want_pos=True),
                R.retrieval_lists(score.cpu().numpy(), None, index.cpu().numpy(), None, 1000, None), "end to end")
    for recipe, mode in (("modelnet", "test"), ("shrec", "train")):
        with pytest.raises(SonetHipError, match="test-mode shrec"):
            retrieval.retrieve_shrec(enc, cls, BatchAssembler(clouds, opt, mode, recipe, seed=3), BS)
