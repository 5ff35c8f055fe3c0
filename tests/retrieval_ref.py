"""numpy restatement of the retrieval-lists contract (include/sonet_hip.h: sonet_retrieval_lists_f32), written from that contract:
the checker of tests/test_retrieval_cpu.py, tests/test_gpu_retrieval.py, tools/make_retrieval_golden.py and tools/bench_retrieval.py.

Also the seeded input makers the fixtures and the tests share, and the rules by which a list is held to the reference's own files
(``check_against_reference``), whose f32 norm sums in another order than the contract's sequential one:

  d64 is the float64 distance of the f32 rows.  Any f32 evaluation of norm(a - b), in any summation order, is within
  bound = (D + 4) * 2^-24 * d64 of it (to first order: the subtraction 1 u, the square 1 u, the sum D - 1 u on d^2 -- halved by the
  root -- plus the root's 1 u).  Two members are a NEAR TIE when their d64 differ by less than twice that bound.  Per stored list:
  the count is equal; every distance is within 0.5e-6 (the print rounding of '%f') + bound of the printed one; the id at a position
  is equal unless that position's member is in a near tie with the member of a neighbouring position (such a position is EXCUSED)."""
import numpy as np

NAN_BITS = 0x7FC00000
U = 2.0 ** -24
PRINT = 0.5e-6


def argmax_rule(feat):
    """feat N x D -> N int64: the first of equal maxima wins, a NaN beats every number, the first NaN wins (torch.max on CPU)."""
    feat = np.asarray(feat)
    best = feat[:, 0].copy()
    idx = np.zeros(best.shape, dtype=np.int64)
    for c in range(1, feat.shape[1]):
        x = feat[:, c]
        with np.errstate(invalid="ignore"):
            take = (x > best) | (np.isnan(x) & ~np.isnan(best))
        best = np.where(take, x, best)
        idx = np.where(take, c, idx)
    return idx


def d2_f32(q, rows):
    """Sequential f32 sum of squared differences, c ascending, accumulator from +0, every operation rounded to f32: K float32."""
    q, rows = np.asarray(q, dtype=np.float32), np.asarray(rows, dtype=np.float32)
    acc = np.zeros(rows.shape[0], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(rows.shape[1]):
            t = q[c] - rows[:, c]
            acc = acc + t * t
    return acc


def retrieval_lists(feat, labels=None, ids=None, query=None, top=1000, n_label=None):
    """Everything the entry point returns: dict of nn_id [Q][top] i64, nn_dist [Q][top] f32, nn_pos [Q][top] i32, count [Q] i32,
    labels [N] i32, bad int."""
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    N, D = feat.shape
    if labels is None:
        lab64, n_label = argmax_rule(feat), D
    else:
        lab64 = np.asarray(labels, dtype=np.int64)
    good = (lab64 >= 0) & (lab64 < n_label)
    lab = np.where(good, lab64, -1).astype(np.int32)
    ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    query = np.arange(N, dtype=np.int64) if query is None else np.asarray(query, dtype=np.int64)
    Q = query.shape[0]
    out = dict(nn_id=np.full((Q, top), -1, np.int64), nn_dist=np.full((Q, top), np.inf, np.float32),
               nn_pos=np.full((Q, top), -1, np.int32), count=np.zeros(Q, np.int32), labels=lab, bad=int((~good).sum()))
    members = {}
    for qi, i in enumerate(query):
        if not 0 <= i < N:
            out["bad"] += 1
            continue
        if lab[i] < 0:
            continue
        if lab[i] not in members:
            members[lab[i]] = np.nonzero(lab == lab[i])[0]
        mem = members[lab[i]]
        bits = d2_f32(feat[i], feat[mem]).view(np.uint32).astype(np.uint64)
        bits[(bits & 0x7FFFFFFF) > 0x7F800000] = NAN_BITS
        key = (bits << np.uint64(32)) | np.arange(mem.shape[0], dtype=np.uint64)
        order = np.argsort(key, kind="stable")[:top]
        k = order.shape[0]
        d2 = (key[order] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(d2)
        dist.view(np.uint32)[np.isnan(d2)] = NAN_BITS
        out["count"][qi] = k
        out["nn_pos"][qi, :k] = order
        out["nn_id"][qi, :k] = ids[mem[order]]
        out["nn_dist"][qi, :k] = dist
    return out


# ---------------------------------------------------------------------------------------------------- seeded inputs
def class_labels(g, N, shares):
    """N labels with about the given class shares, shuffled; every class at least one member."""
    sizes = np.maximum(1, np.round(np.asarray(shares, dtype=np.float64) * N).astype(np.int64))
    sizes[0] += N - sizes.sum()
    assert sizes.min() >= 1
    lab = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    g.shuffle(lab)
    return lab


def make_inputs(g, N, D, shares, scale=3.0, quantum=None, id_range=100000):
    """(feat N x D f32, labels N i64, model ids N i64): normal * scale features (rounded to multiples of ``quantum`` when given: exact
    ties and duplicate rows), labels with the class shares, ids a random subset of [0, id_range)."""
    feat = (g.normal(size=(N, D)) * scale).astype(np.float32)
    if quantum:
        feat = (np.round(feat / quantum) * quantum).astype(np.float32)
    return feat, class_labels(g, N, shares), g.choice(id_range, N, replace=False).astype(np.int64)


def sized_class(g, K, others, D, scale=3.0, quantum=None):
    """One class 0 of exactly K members scattered among ``others`` shapes of class 1: (feat, labels, queries at the first, middle and
    last member of class 0)."""
    lab = np.concatenate([np.zeros(K, np.int64), np.ones(others, np.int64)])
    g.shuffle(lab)
    feat = (g.normal(size=(K + others, D)) * scale).astype(np.float32)
    if quantum:
        feat = (np.round(feat / quantum) * quantum).astype(np.float32)
    mem = np.nonzero(lab == 0)[0]
    return feat, lab, np.unique(mem[[0, K // 2, K - 1]]).astype(np.int32)


def special_values(g, N, D):
    """Rows holding +-0, +-inf, NaN and huge values beside ordinary ones, and duplicates of row 0."""
    feat = g.normal(size=(N, D)).astype(np.float32)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 1e-45], dtype=np.float32)
    hit = g.uniform(size=(N, D)) < 0.08
    feat[hit] = pool[g.randint(0, len(pool), int(hit.sum()))]
    feat[1::7] = feat[0]
    return feat


def argmax_rule_inputs(g, N=64, D=9):
    """Rows with equal maxima, +-0, +-inf and one / several / only NaNs."""
    s = np.round(g.normal(size=(N, D)) * 2).astype(np.float32)
    s[0] = 0.0
    s[1] = [0.0, -0.0] * (D // 2) + [-0.0]
    s[2, 3], s[2, 6] = np.inf, np.inf
    s[3] = -np.inf
    s[4, 5] = np.nan
    s[5, 2], s[5, 7] = np.nan, np.nan
    s[6] = np.nan
    s[7, 0], s[7, 4] = np.inf, np.nan
    s[8, 8] = np.nan
    return s


# ---------------------------------------------------------------------------------------------------- rules against reference lists
def d64(feat, i, members):
    f = np.asarray(feat, dtype=np.float64)
    return np.sqrt(((f[i] - f[members]) ** 2).sum(axis=1))


def check_against_reference(feat, labels, ids, query, ref_ids, ref_dist, got_ids, got_dist, got_count, what=""):
    """The continuous rules (module docstring).  ref_ids / ref_dist: per query the parsed file (ids, printed distances); got_*: rows
    of the lists under test for the same queries.  Asserts the rules; returns (positions, excused positions, worst |got - printed| as
    a fraction of its allowance)."""
    feat = np.asarray(feat, dtype=np.float32)
    N, D = feat.shape
    ids = np.asarray(ids, dtype=np.int64)
    where = {int(v): j for j, v in enumerate(ids)}
    assert len(where) == N, "model ids must be unique"
    positions = excused = 0
    worst = 0.0
    for n, i in enumerate(query):
        rid, rd = np.asarray(ref_ids[n], dtype=np.int64), np.asarray(ref_dist[n], dtype=np.float64)
        k = rid.shape[0]
        assert int(got_count[n]) == k, "%s query %d: count %d != %d" % (what, i, got_count[n], k)
        members = np.array([where[int(v)] for v in rid])
        assert (np.asarray(labels)[members] == np.asarray(labels)[i]).all(), "%s query %d: a member of another class" % (what, i)
        dd = d64(feat, i, members)
        bound = (D + 4) * U * dd
        err = np.abs(np.asarray(got_dist[n][:k], dtype=np.float64) - rd)
        assert (err <= PRINT + bound).all(), "%s query %d: distance off by %.3g (allowed %.3g)" % (
            what, i, err.max(), (PRINT + bound)[err.argmax()])
        worst = max(worst, float((err / (PRINT + bound)).max()))
        near = np.zeros(k, dtype=bool)
        if k > 1:
            gap = np.abs(np.diff(dd))
            near[:-1] |= gap < 2 * np.maximum(bound[:-1], bound[1:])
            near[1:] |= gap < 2 * np.maximum(bound[:-1], bound[1:])
        differ = np.asarray(got_ids[n][:k], dtype=np.int64) != rid
        assert not (differ & ~near).any(), "%s query %d: %d ids differ outside a near tie" % (what, i, int((differ & ~near).sum()))
        positions += k
        excused += int(differ.sum())
    return positions, excused, worst


def check_ties_against_reference(ref_ids, ref_dist, got_ids, got_dist, got_count, cut, what=""):
    """The quantised rules: distance sequences equal within print rounding; ids equal as multisets within every run of equal printed
    distance that the cut (a list of ``cut`` rows) does not split; the ids under test ascend inside a run only by gallery index, which
    the caller checks on positions."""
    for n in range(len(ref_ids)):
        rid, rd = np.asarray(ref_ids[n], dtype=np.int64), np.asarray(ref_dist[n], dtype=np.float64)
        k = rid.shape[0]
        assert int(got_count[n]) == k, (what, n)
        gd = np.asarray(got_dist[n][:k], dtype=np.float64)
        assert (np.abs(gd - rd) <= PRINT).all(), (what, n, np.abs(gd - rd).max())
        start = 0
        for end in list(np.nonzero(np.diff(rd) != 0)[0] + 1) + [k]:
            if not (end == k and k == cut):                      # (the last run of a cut list may be split by the cut)
                assert sorted(rid[start:end].tolist()) == sorted(np.asarray(got_ids[n][start:end]).tolist()), (what, n, start, end)
            start = end


def load_lists(g):
    """A fixture's stored lists: (query, [ids per query], [printed distances per query])."""
    start = np.concatenate([[0], np.cumsum(g["list_count"])])
    rid = [g["list_ids"][start[n]:start[n + 1]] for n in range(len(g["query"]))]
    rd = [g["list_dist_micro"][start[n]:start[n + 1]] / 1e6 for n in range(len(g["query"]))]
    return g["query"], rid, rd


def parse_folder(folder, model_ids):
    """The files of a folder for the shapes named ``model_ids``: ([ids per file], [printed distances per file], [rows per file])."""
    import os
    import re
    row = re.compile(r"^\d{6} \d+\.\d{6}$")
    rid, rd, cnt = [], [], []
    for m in model_ids:
        lines = open(os.path.join(folder, "%06d" % m)).read().splitlines()
        assert all(row.match(ln) for ln in lines), (m, [ln for ln in lines if not row.match(ln)][:3])
        rid.append(np.array([int(ln.split()[0]) for ln in lines], dtype=np.int64))
        rd.append(np.array([int(ln.split()[1].replace(".", "")) for ln in lines], dtype=np.int64) / 1e6)
        cnt.append(len(lines))
    return rid, rd, cnt


def check_fixture(g, got_ids, got_dist, got_count, continuous, what=""):
    """Lists under test (rows for the fixture's queries, in their order) against the fixture's stored reference lists.  Returns
    (positions, excused, worst) of the continuous rules."""
    query, rid, rd = load_lists(g)
    if continuous:
        positions, excused, worst = check_against_reference(g["feat"], g["labels"], g["model_ids"], query, rid, rd, got_ids, got_dist,
                                                            got_count, what)
        assert excused <= 0.01 * positions, "%s: %d of %d positions excused" % (what, excused, positions)
        return positions, excused, worst
    check_ties_against_reference(rid, rd, got_ids, got_dist, got_count, 1000, what)
    return int(np.sum(g["list_count"])), 0, 0.0
