"""tools/make_retrieval_golden.py -- fixtures of the retrieval lists (sonet_retrieval_lists_f32) from the LIVE reference.

Run where the reference checkout is mounted:   python tools/make_retrieval_golden.py [out_dir] [--check]
(default out_dir: tests/golden/retrieval).

The neighbour stage of the reference is not a function: it is the tail of the script shrec16/test.py, from its '# calculate
neighbors' comment to the end.  This tool reads that file from the reference checkout at run time, compiles that part and executes
it in a namespace holding what the script's first half would have left: CPU tensors feature_map, predicted_labels, model_name_ids, a
sized testset and a temporary output_folder.  (That part has no .cuda() call: it runs on CPU tensors as it is.)  The files it writes
are parsed.  Nothing of the reference is stored: the fixtures hold data only --
  feat [N][D] f32, labels [N] i64, model_ids [N] i64                          the inputs;
  query [nq] i32                                                              the gallery indices whose files are kept;
  list_count [nq] i64, list_ids [sum] i64, list_dist_micro [sum] i64          their rows: ids and printed distances * 10^6.
While writing, the reference's own lists are held against the float64 order by the rules of tests/retrieval_ref.py (positions that
differ must be near ties, at most 1 % of the positions on the continuous cases).
--check regenerates into a temporary directory and compares with out_dir array by array, then holds the restatement of
tests/retrieval_ref.py to the live reference on fresh seeded inputs of odd sizes (FRESH) by the same rules.
"""
import os
import sys
import tempfile
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import retrieval_ref as R  # noqa: E402

from oracle import ref_harness  # noqa: E402

MARK = "# calculate neighbors"
MAX_BYTES = 256 * 1000

# name: seed, N, D, class shares, make_inputs keywords, queries per class beyond the first and last member, continuous?
CASES = {
    "continuous_3_classes": (21, 600, 55, (0.70, 0.25, 0.05), dict(scale=3.0), (6, 6, 6), True),
    "truncated_class": (22, 1300, 8, (0.846, 0.077, 0.077), dict(scale=3.0), (8, 1, 1), True),
    "ties_quantised": (23, 400, 8, (0.6, 0.4), dict(scale=3.0, quantum=1.0), (14, 14), False),
}
FRESH = [   # seed, N, D, shares, make_inputs keywords, continuous?
    (201, 257, 55, (0.5, 0.3, 0.2), dict(), True),
    (202, 1111, 3, (0.95, 0.05), dict(), True),
    (203, 333, 7, (0.6, 0.4), dict(quantum=1.0), False),
    (204, 65, 1024, (0.9, 0.1), dict(), True),
    (205, 1, 5, (1.0,), dict(), True),
]


def reference_neighbour_stage():
    """The code object of the reference's neighbour stage, compiled from its file."""
    path = os.path.join(ref_harness.REF_ROOT, "shrec16", "test.py")
    src = open(path).read()
    assert src.count(MARK) == 1, "the neighbour stage of %s is not where it was" % path
    return compile(textwrap.dedent(src[src.rindex("\n", 0, src.index(MARK)) + 1:]), path, "exec")


def reference_lists(code, feat, labels, ids):
    """Run the stage on CPU tensors; parse every file: {model id: (ids i64, printed distances * 10^6 i64)}."""
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        ns = dict(torch=torch, np=np, os=os, feature_map=torch.from_numpy(feat), predicted_labels=torch.from_numpy(labels),
                  model_name_ids=torch.from_numpy(ids), testset=range(feat.shape[0]), output_folder=tmp)
        exec(code, ns)
        out = {}
        for name in os.listdir(tmp):
            rows = [ln.split() for ln in open(os.path.join(tmp, name)).read().splitlines()]
            assert all(len(r) == 2 and len(r[1].split(".")[1]) == 6 for r in rows), name
            out[int(name)] = (np.array([int(r[0]) for r in rows], dtype=np.int64),
                              np.array([int(r[1].replace(".", "")) for r in rows], dtype=np.int64))
    assert len(out) == feat.shape[0]
    return out


def float64_lists(feat, labels, ids, query, top=1000):
    """The lists in float64 order (ties by gallery index): what the reference's own lists are held against while the fixtures are written."""
    got_ids, got_dist, got_count = [], [], []
    for i in query:
        mem = np.nonzero(labels == labels[i])[0]
        dd = R.d64(feat, i, mem)
        o = np.argsort(dd, kind="stable")[:top]
        got_ids.append(ids[mem[o]])
        got_dist.append(dd[o])
        got_count.append(len(o))
    return got_ids, got_dist, got_count


def hold(feat, labels, ids, query, lists, got_ids, got_dist, got_count, continuous, what):
    rid = [lists[int(ids[i])][0] for i in query]
    rd = [lists[int(ids[i])][1] / 1e6 for i in query]
    if not continuous:
        R.check_ties_against_reference(rid, rd, got_ids, got_dist, got_count, 1000, what)
        return 0.0, 0.0
    positions, excused, worst = R.check_against_reference(feat, labels, ids, query, rid, rd, got_ids, got_dist, got_count, what)
    assert excused <= 0.01 * positions, "%s: %d of %d positions excused" % (what, excused, positions)
    return excused / max(positions, 1), worst


def choose_queries(g, labels, extra):
    q = []
    for c, n in enumerate(extra):
        mem = np.nonzero(labels == c)[0]
        q += [mem[0], mem[-1]]
        rest = mem[1:-1]
        q += g.choice(rest, min(n, len(rest)), replace=False).tolist()
    return np.unique(np.asarray(q)).astype(np.int32)


def make_case(code, name, seed, N, D, shares, kw, extra, continuous):
    g = np.random.RandomState(seed)
    feat, labels, ids = R.make_inputs(g, N, D, shares, **kw)
    query = choose_queries(g, labels, extra)
    lists = reference_lists(code, feat, labels, ids)
    got_ids, got_dist, got_count = float64_lists(feat, labels, ids, query)
    if not continuous:                       # exact d2: the reference's f32 root is the float64 one rounded once more
        got_dist = [d.astype(np.float32) for d in got_dist]
    share, worst = hold(feat, labels, ids, query, lists, got_ids, got_dist, got_count, continuous, name + " (reference vs float64)")
    count = np.array([len(lists[int(ids[i])][0]) for i in query], dtype=np.int64)
    d = dict(feat=feat, labels=labels, model_ids=ids, query=query, list_count=count,
             list_ids=np.concatenate([lists[int(ids[i])][0] for i in query]),
             list_dist_micro=np.concatenate([lists[int(ids[i])][1] for i in query]))
    return d, share, worst


def check_restatement(code):
    worst_all = 0.0
    for seed, N, D, shares, kw, continuous in FRESH:
        feat, labels, ids = R.make_inputs(np.random.RandomState(seed), N, D, shares, **kw)
        lists = reference_lists(code, feat, labels, ids)
        r = R.retrieval_lists(feat, labels, ids, None, 1000, len(shares))
        query = np.arange(N)
        share, worst = hold(feat, labels, ids, query, lists, r["nn_id"], r["nn_dist"], r["count"], continuous, "fresh %d" % seed)
        worst_all = max(worst_all, worst)
        if not continuous:                                       # inside a run of equal distance: ascending gallery index
            for q in range(N):
                k = r["count"][q]
                d, p = r["nn_dist"][q, :k], r["nn_pos"][q, :k]
                assert ((np.diff(d) > 0) | (np.diff(p) > 0)).all(), (seed, q)
        print("fresh %d: N %d D %d, %.4f %% of the positions excused, worst distance error %.3f of its allowance"
              % (seed, N, D, 100 * share, worst))
    print("restatement == live reference on %d fresh inputs (worst distance error %.3f of its allowance)" % (len(FRESH), worst_all))


def generate(out_dir):
    assert ref_harness.available(), "the reference checkout is not mounted"
    code = reference_neighbour_stage()
    os.makedirs(out_dir, exist_ok=True)
    for name, case in CASES.items():
        d, share, worst = make_case(code, name, *case)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (name, size)
        print("%-24s %6.1f KB  %d queries, %d rows (longest %d); reference vs float64: %.4f %% excused, worst distance %.3f of its allowance"
              % (name + ".npz", size / 1024, len(d["query"]), d["list_count"].sum(), d["list_count"].max(), 100 * share, worst))
    return code


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "retrieval")
    if "--check" not in sys.argv:
        generate(out_dir)
        return
    with tempfile.TemporaryDirectory() as tmp:
        code = generate(tmp)
        for name in CASES:
            a, b = np.load(os.path.join(tmp, name + ".npz")), np.load(os.path.join(out_dir, name + ".npz"))
            assert sorted(a.files) == sorted(b.files), name
            for k in a.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: %s differs" % (name, k)
    print("fixtures regenerate bit-identically")
    check_restatement(code)


if __name__ == "__main__":
    main()
