"""Retrieval lists without a GPU: the numpy restatement (tests/retrieval_ref.py) against the fixtures of the live reference
(tests/golden/retrieval, tools/make_retrieval_golden.py) and against the reference itself where it is mounted; the arg-max rule against
torch.max on CPU tensors; the C entry's argument checks; what the wrapper refuses before a device is needed; the file writer."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import retrieval_ref as R
from oracle import ref_harness

CASES = {"continuous_3_classes": True, "truncated_class": True, "ties_quantised": False}      # name: continuous rules?
_restated = {}


def restated(case):
    """The restatement's lists for a fixture's queries (computed once per session, never modified)."""
    if case not in _restated:
        g = golden("retrieval/" + case)
        _restated[case] = R.retrieval_lists(g["feat"], g["labels"], g["model_ids"], g["query"], 1000, int(g["labels"].max()) + 1)
    return _restated[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_matches_the_reference_fixtures(case):
    g = golden("retrieval/" + case)
    assert g["feat"].dtype == np.float32 and g["labels"].dtype == g["model_ids"].dtype == np.int64 and g["query"].dtype == np.int32
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "retrieval", case + ".npz")) < 256 * 1000
    r = restated(case)
    positions, excused, worst = R.check_fixture(g, r["nn_id"], r["nn_dist"], r["count"], CASES[case], case)
    print("%s: %d positions, %d excused, worst distance error %.3f of its allowance" % (case, positions, excused, worst))
    assert positions == g["list_count"].sum() and r["bad"] == 0
    if not CASES[case]:                                            # the restatement's own order inside a run: ascending gallery index
        for q in range(len(g["query"])):
            k = r["count"][q]
            d, p = r["nn_dist"][q, :k], r["nn_pos"][q, :k]
            assert ((np.diff(d) > 0) | (np.diff(p) > 0)).all(), q
            assert (np.diff(d) == 0).any(), "no exact tie in list %d" % q


def test_fixture_families_pin_what_they_are_named_for():
    g = golden("retrieval/continuous_3_classes")
    N, D = g["feat"].shape
    assert 590 <= N <= 610 and D == 55 and len(g["query"]) == 24
    share = np.bincount(g["labels"]) / N
    assert np.allclose(share, [0.70, 0.25, 0.05], atol=0.01)
    for c in range(3):
        mem = np.nonzero(g["labels"] == c)[0]
        assert mem[0] in g["query"] and mem[-1] in g["query"]
    assert len(set(g["model_ids"].tolist())) == N and 0 <= g["model_ids"].min() and g["model_ids"].max() < 100000
    g = golden("retrieval/truncated_class")
    assert g["feat"].shape[1] == 8 and len(g["query"]) == 16 and np.bincount(g["labels"]).max() >= 1100
    assert g["list_count"].max() == 1000 and (g["list_count"] == 1000).sum() >= 8          # the files stop at 1000 rows
    g = golden("retrieval/ties_quantised")
    assert g["feat"].shape == (400, 8) and len(g["query"]) == 32 and (g["feat"] == np.round(g["feat"])).all()
    _, rid, rd = R.load_lists(g)
    assert all((np.diff(d) == 0).any() for d in rd)                                          # every stored list has exact ties


@pytest.mark.skipif(not ref_harness.available(), reason="reference checkout not mounted")
def test_fixtures_regenerate_and_restatement_equals_the_live_reference():
    """tools/make_retrieval_golden.py --check in its own process: the fixtures regenerate bit for bit, and on fresh seeded inputs of odd
    sizes the restatement is held to the reference's own neighbour stage by the rules of retrieval_ref."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_retrieval_golden.py"), "--check"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "fixtures regenerate bit-identically" in out and "restatement == live reference" in out


def test_argmax_rule_is_torch_max_on_cpu():
    for seed in range(4):
        s = R.argmax_rule_inputs(np.random.RandomState(seed))
        want = torch.max(torch.from_numpy(s), dim=1)[1].numpy()
        assert np.array_equal(R.argmax_rule(s), want), seed
    s = R.argmax_rule_inputs(np.random.RandomState(0))
    assert np.isnan(s).any() and np.isinf(s).any() and (np.signbit(s) & (s == 0)).any()
    r = R.retrieval_lists(s, top=5)                                 # labels derived: the rule feeds the lists
    assert np.array_equal(r["labels"], torch.max(torch.from_numpy(s), dim=1)[1].numpy())


def test_restatement_on_bad_labels_and_special_values():
    g = np.random.RandomState(3)
    feat, labels, ids = R.make_inputs(g, 50, 4, (0.5, 0.5))
    clean = R.retrieval_lists(feat, labels, ids, None, 7, 2)
    lab2 = labels.copy()
    lab2[[3, 17]] = [-1, 2]
    r = R.retrieval_lists(feat, lab2, ids, np.array([3, 17, 0, 49, 50, -1]), 7, 2)
    assert r["bad"] == 4 and r["count"][[0, 1, 4, 5]].tolist() == [0, 0, 0, 0] and r["labels"][[3, 17]].tolist() == [-1, -1]
    assert (r["nn_id"][0] == -1).all() and np.isposinf(r["nn_dist"][0]).all() and (r["nn_pos"][0] == -1).all()
    assert not np.isin(ids[[3, 17]], r["nn_id"]).any()
    other = 1 - labels[3]
    q = int(np.nonzero((labels == other) & (labels != labels[17]))[0][0]) if labels[3] != labels[17] else None
    if q is not None:                                               # a class that lost nobody keeps its list
        a = R.retrieval_lists(feat, lab2, ids, [q], 7, 2)
        assert np.array_equal(a["nn_id"][0], clean["nn_id"][q])
    s = R.special_values(g, 40, 5)
    r = R.retrieval_lists(s, np.zeros(40, np.int64), None, None, 40, 1)
    bits = r["nn_dist"].view(np.uint32)
    assert (r["count"] == 40).all() and np.isnan(r["nn_dist"]).any()
    assert (bits[np.isnan(r["nn_dist"])] == R.NAN_BITS).all()
    assert np.isposinf(r["nn_dist"]).any() and (r["nn_dist"] == 0).sum() > 40
    for q in range(40):                                             # the bits ascend: numbers, +inf, then NaN; ties by position
        b, p = bits[q].astype(np.int64), r["nn_pos"][q].astype(np.int64)
        assert ((np.diff(b) > 0) | ((np.diff(b) == 0) & (np.diff(p) > 0))).all() and len(set(p.tolist())) == 40


def test_c_entry_rejects_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    names = ("feat", "label", "ids", "query", "nn_id", "nn_dist", "nn_pos", "count", "label_out", "bad", "ws")

    def call(N=4, D=2, Q=4, n_label=2, top=3, **null):
        a = {k: (None if null.get(k) else p) for k in names}
        return lib.sonet_retrieval_lists_f32(a["feat"], a["label"], a["ids"], a["query"], n_label, top, a["nn_id"], a["nn_dist"],
                                             a["nn_pos"], a["count"], a["label_out"], a["bad"], a["ws"], N, D, Q, None)

    for name in ("feat", "nn_id", "nn_dist", "count", "bad", "ws"):
        assert call(**{name: True}) == 1 and "NULL" in _lib.last_error(), name
    for kw in (dict(N=0), dict(D=0), dict(Q=0), dict(N=-1), dict(Q=-5)):
        assert call(**kw) == 1 and "non-positive" in _lib.last_error(), kw
    for top in (0, -1, 1025):
        assert call(top=top) == 1 and "top=%d" % top in _lib.last_error()
    for n_label in (0, -3, 65536):
        assert call(n_label=n_label) == 1 and "n_label=%d" % n_label in _lib.last_error()
    assert call(label=True, n_label=3) == 1 and "n_label == D" in _lib.last_error()             # derived labels: n_label must be D
    assert call(query=True, Q=3) == 1 and "Q must be N" in _lib.last_error()
    assert call(N=1 << 24, Q=1) == 2 and "2^24" in _lib.last_error()
    assert call(D=1025, n_label=1025) == 2 and "D=1025" in _lib.last_error()
    ws = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    assert lib.sonet_retrieval_lists_f32(p, p, p, p, 2, 3, p, p, p, p, p, p, ws, 4, 2, 4, None) == 1 and "aligned" in _lib.last_error()
    for args in ((0, 55, 10, 1000), (10, 0, 10, 1000), (10, 55, 0, 1000), (10, 55, 10, 0), (-1, 55, 10, 1000), (10, 55, 10, -2)):
        assert lib.sonet_retrieval_ws_size(*args) == 0, args
    assert lib.sonet_retrieval_ws_size(100, 55, 100, 1000) >= 100 * 55 * 4 + 2 * 100 * 4
    ck = lib.sonet_retrieval_chunk_keys()
    assert ck >= 2 * 1024 and ck & (ck - 1) == 0


def test_wrapper_refuses_before_a_device_is_needed():
    """Shapes, dtypes, top, n_label and a host query are host data, checked first; CPU tensors are refused after them.  (Wrong devices and
    non-contiguous CUDA tensors: tests/test_gpu_retrieval.py.)"""
    from sonet_hip import ops, retrieval
    from sonet_hip._lib import SonetHipError
    feat, lab, ids = torch.zeros(6, 4), torch.zeros(6, dtype=torch.int64), torch.arange(6)
    for bad, match in ((dict(feat=torch.zeros(6)), "N x D"), (dict(feat=torch.zeros(6, 4, 1)), "N x D"), (dict(feat=feat.double()), "float32"),
                       (dict(feat=feat.numpy()), "N x D"), (dict(labels=lab.int()), "int64"), (dict(labels=lab[:5]), "N = 6"),
                       (dict(ids=ids.float()), "int64"), (dict(ids=torch.zeros(6, 1, dtype=torch.int64)), "N = 6"),
                       (dict(top=0), "top"), (dict(top=1025), "top"), (dict(top=7.0), "top"), (dict(top=True), "top"),
                       (dict(n_label=0), "n_label"), (dict(n_label=65536), "n_label"), (dict(n_label=None), "n_label is needed"),
                       (dict(labels=None, n_label=5), "arg-max over D = 4"),
                       (dict(query=[0, 6]), "outside"), (dict(query=[-1]), "outside"), (dict(query=torch.tensor([2, 7])), "outside"),
                       (dict(query=[]), "non-empty"), (dict(query=[0.5]), "integers"), (dict(query=[[0, 1]]), "1-D"),
                       (dict(feat=torch.zeros(6, 1025)), "D <= 1024"), (dict(feat=torch.zeros(0, 4), labels=lab[:0], ids=None), "1 <= N")):
        kw = dict(dict(feat=feat, labels=lab, ids=ids, query=None, top=5, n_label=3), **bad)
        with pytest.raises(SonetHipError, match=match):
            ops.retrieval_lists(**kw)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.retrieval_lists(feat, lab, ids, [0, 5], 5, 3)
    acc = retrieval.ShapeRetrieval(10, 4, top=5)
    with pytest.raises(SonetHipError, match="CUDA"):
        acc.update(feat, ids)
    with pytest.raises(SonetHipError, match="before any update"):
        acc.lists()
    for kw in (dict(capacity=0, channels=4), dict(capacity=10, channels=1025), dict(capacity=10, channels=4, top=0),
               dict(capacity=1 << 24, channels=4)):
        with pytest.raises(SonetHipError):
            retrieval.ShapeRetrieval(**kw)

    class Fake:
        recipe, mode = "modelnet", "test"
    with pytest.raises(SonetHipError, match="test-mode shrec"):
        retrieval.retrieve_shrec(None, None, Fake(), 4)
    Fake.recipe, Fake.mode = "shrec", "train"
    with pytest.raises(SonetHipError, match="test-mode shrec"):
        retrieval.retrieve_shrec(None, None, Fake(), 4)


def test_writer_files_are_the_reference_files(tmp_path):
    """write_lists on the restatement's lists: names, row format, row counts -- and the parsed files meet the stored reference lists."""
    from sonet_hip import retrieval
    row = re.compile(r"^\d{6} \d+\.\d{6}$")
    for case in ("truncated_class", "ties_quantised"):
        g = golden("retrieval/" + case)
        r = restated(case)
        folder = tmp_path / case
        qids = g["model_ids"][g["query"]]
        assert retrieval.write_lists(str(folder), qids, r["nn_id"], r["nn_dist"], r["count"]) == len(qids)
        assert sorted(os.listdir(folder)) == sorted("%06d" % m for m in qids)
        rid, rd, cnt = R.parse_folder(str(folder), qids)
        assert cnt == r["count"].tolist() and max(cnt) <= 1000
        R.check_fixture(g, rid, rd, cnt, CASES[case], case + " files")
        lines = open(folder / ("%06d" % qids[0])).read().splitlines()
        assert all(row.match(ln) for ln in lines) and lines[0] == "%06d 0.000000" % qids[0]      # the query itself comes first
    # a class of one: one row; top = 7: at most 7 rows
    feat, labels, ids = R.make_inputs(np.random.RandomState(8), 30, 3, (0.9, 0.1))
    labels[:] = 0
    labels[11] = 1
    r = R.retrieval_lists(feat, labels, ids, None, 7, 2)
    folder = tmp_path / "small"
    retrieval.write_lists(str(folder), ids, r["nn_id"], r["nn_dist"], r["count"])
    rid, rd, cnt = R.parse_folder(str(folder), ids)
    assert cnt[11] == 1 and rid[11].tolist() == [ids[11]] and rd[11].tolist() == [0.0]
    assert all(c == 7 for n, c in enumerate(cnt) if n != 11)
