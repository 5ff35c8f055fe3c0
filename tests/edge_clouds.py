"""Edge inputs of the distance-search kernels (SOM assignment, node self-kNN, Chamfer 1-NN) and float32 numpy restatements of
the three searches.  Plain module: seeded numpy generators, no fixtures, no torch, no GPU.

The searches are specified bit-exactly: d = (dx*dx + dy*dy) + dz*dz in float32 (separate multiplies and adds), ties to the lowest
id, a distance that is not finite orders as +inf.  Continuous random clouds never exercise that contract; these families do:

A  lattice      coordinates rounded to multiples of 1/q: exact ties everywhere
B  near ties    node pairs / triples mirrored about a point, one coordinate stepped by 1 .. 2^IB ulps: distances that agree in the
                bits the packed keys keep and differ below them, placed inside the selected list, across its last slot and behind it
C  occupancy    coinciding points, one node taking everything, duplicated points / nodes, a point on a node, size edges
D  overflow     finite coordinates whose squared distance is +inf (and, separately, NaN coordinates)
E  Chamfer      database / query sizes around the 1024-point tile, the pair tail and the 256-thread workgroup, on lattice data

Arrays are laid out as the kernels take them: x B x 3 x N, node B x 3 x M, float32.
"""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------ the searches, restated
def dist_f32(x, node):
    """B x N x M float32: (dx*dx + dy*dy) + dz*dz, every operation rounded to float32 (numpy never fuses)."""
    x = np.asarray(x, F32)
    node = np.asarray(node, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = x[:, 0, :, None] - node[:, 0, None, :]
        dy = x[:, 1, :, None] - node[:, 1, None, :]
        dz = x[:, 2, :, None] - node[:, 2, None, :]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F32
    return d


def order_key(d):
    """What the searches order by: the distance, NaN counted as +inf."""
    return np.where(np.isnan(d), F32(np.inf), d)


def som_topk(x, node, k):
    """Stable argsort of the distance matrix, first k -> (min_idx B x kN int64 k-major, count B x M int32, row_max B x M int32)."""
    d = order_key(dist_f32(x, node))
    B, N, M = d.shape
    idx = np.argsort(d, axis=2, kind="stable")[:, :, :k]                 # B x N x k, ascending (d, id)
    min_idx = np.ascontiguousarray(idx.transpose(0, 2, 1)).reshape(B, k * N).astype(np.int64)
    count = np.stack([np.bincount(min_idx[b], minlength=M) for b in range(B)]).astype(np.int32)
    return min_idx, count, (count > 0).astype(np.int32)


def chamfer_argmin(q, db):
    """B x Nq int32: first arg-min of the distance row (finite data only)."""
    return np.argmin(dist_f32(q, db), axis=2).astype(np.int32)


def knn_self_topk(node, K):
    """B x M x K int64: stable (d, id) top-K of the nodes' own distance matrix."""
    d = order_key(dist_f32(node, node))
    return np.argsort(d, axis=2, kind="stable")[:, :, :K].astype(np.int64)


# ------------------------------------------------------------------------------------------ kernel-side predicates
def key_bits(M):
    """Id bits of the packed keys the dispatcher picks for M nodes."""
    return 6 if M <= 64 else 10


def packed_keys(d, IB):
    """(bits(d) & ~mask) | id, uint32, for a ... x M matrix of non-negative distances."""
    d = np.ascontiguousarray(d, F32)
    mask = np.uint32((1 << IB) - 1)
    ids = np.arange(d.shape[-1], dtype=np.uint32)
    return (d.view(np.uint32) & ~mask) | ids


def _smallest_keys(d, k, IB):
    keys = np.sort(packed_keys(d, IB), axis=-1)
    pad = k + 1 - keys.shape[-1]
    if pad > 0:
        keys = np.concatenate([keys, np.full(keys.shape[:-1] + (pad,), 0xFFFFFFFF, np.uint32)], axis=-1)
    return keys[..., :k + 1]


def needs_exact_redo(d, k, IB):
    """The kernels' condition for leaving the packed-key fast path, on the k + 1 smallest keys t[0..k] of every point: the list reaches
    +inf / NaN (t[k-1] >= 0x7F800000) or two neighbours t[s], t[s+1] (s < k) have equal high parts.  -> bool, one per point."""
    t = _smallest_keys(d, k, IB)
    hi = t & ~np.uint32((1 << IB) - 1)
    return (t[..., k - 1] >= np.uint32(0x7F800000)) | (hi[..., :k] == hi[..., 1:k + 1]).any(axis=-1)


def key_order_topk(d, k, IB):
    """The ids the packed keys alone would select (no exact redo): ... x k."""
    return (_smallest_keys(d, k, IB)[..., :k] & np.uint32((1 << IB) - 1)).astype(np.int64)


def tie_share(d, k):
    """Share of points with an exact tie among their k + 1 smallest distances."""
    s = np.sort(order_key(d), axis=-1)[..., :k + 1]
    return float((s[..., 1:] == s[..., :-1]).any(axis=-1).mean())


# ------------------------------------------------------------------------------------------ helpers
def normals(B, N, seed):
    r = np.random.default_rng(seed)
    sn = r.standard_normal((B, 3, N)).astype(F32)
    return (sn / np.maximum(np.sqrt((sn * sn).sum(1, keepdims=True)), F32(1e-12))).astype(F32)


def uniform(B, N, seed):
    return (np.random.default_rng(seed).random((B, 3, N)) * 2 - 1).astype(F32)


def step_ulps(v, u, away_from_zero):
    """v float32 array moved by u (int array) float32 steps, away from or towards zero (|v| stays normal and non-zero here)."""
    b = np.ascontiguousarray(v, F32).view(np.int32).copy()
    b += np.where(away_from_zero, u, -u).astype(np.int32)
    return b.view(F32)


# ------------------------------------------------------------------------------------------ A. lattice
def lattice(B, N, M, q, seed):
    """Points and nodes on the lattice of multiples of 1/q inside [-1, 1]^3."""
    r = np.random.default_rng(seed)
    x = (np.rint(r.uniform(-1, 1, (B, 3, N)) * q) / q).astype(F32)
    node = (np.rint(r.uniform(-1, 1, (B, 3, M)) * q) / q).astype(F32)
    return x, node


LATTICE_CASES = [  # (B, N, M, k, q)
    (2, 3000, 64, 3, 4), (2, 3000, 100, 4, 2), (2, 3000, 16, 3, 1), (3, 1025, 63, 2, 2), (1, 700, 256, 4, 4)]


def lattice_case(case):
    B, N, M, k, q = case
    return lattice(B, N, M, q, seed=1000 + N + M + q) + (k,)


# ------------------------------------------------------------------------------------------ B. near ties
def near_ties(B, M, k, seed, generic_per_centre=1.0):
    """Clouds whose nodes come in groups around "centre" points of the cloud.  A group is j filler nodes at distinct, clearly smaller
    radii, then a PAIR (or triple) of nodes at mirrored offsets +v, -v (and (-vx, vy, vz)) from the centre: equal distances, exactly.
    The z coordinate of all but the first of them is then stepped by 1 .. 2^IB float32 steps away from the centre; vz is 2^-12, so one
    step moves the distance by about a quarter of its ulp: the distances agree in the bits the packed keys keep and differ -- or tie
    exactly -- below them.  j puts the pair inside the selected list (j <= k - 2), across its last slot (j = k - 1) or behind it
    (j = k: must not matter).  Node ids are a random permutation, and a coin decides whether the stepped (farther) node of a pair is the
    one with the lower id.  The cloud is its centres plus ``generic_per_centre`` times as many continuous random points.
    -> x B x 3 x N, node B x 3 x M, kinds B x N (0 generic, 1 inside, 2 across, 3 behind)."""
    r = np.random.default_rng(seed)
    IB = key_bits(M)
    cells = np.array([(a, b, c) for a in range(4) for b in range(4) for c in range(4)], np.float64) * 0.5 - 0.75   # 64 centres, 0.5 apart
    G = k + 3                                                              # nodes per group at most: k fillers + a triple
    C = min(64, M // G)
    assert C >= 3, "too few nodes for three kinds of group"
    n_gen = int(round(generic_per_centre * C))
    N = C + n_gen
    x = np.empty((B, 3, N), F32)
    node = np.empty((B, 3, M), F32)
    kinds = np.zeros((B, N), np.int32)
    for b in range(B):
        centres = cells[r.permutation(64)[:C]] + np.rint(r.uniform(-8, 8, (C, 3))) / 1024.0          # on the 2^-10 grid
        ids = r.permutation(M)
        nodes_b = np.empty((M, 3), F32)
        used = 0
        for ci in range(C):
            c = centres[ci]
            kind = 1 + ci % 3
            if kind == 1 and k < 2:
                kind = 2
            j = int(r.integers(0, k - 1)) if kind == 1 else (k - 1 if kind == 2 else k)
            triple = bool(r.integers(0, 2)) and not (kind == 1 and j + 3 > k)
            kinds[b, ci] = kind
            grp = []
            for f in range(j):                                            # fillers: radii 1/256 .. j/256 along x (pair radius ~ 0.04)
                grp.append(c + np.array([(f + 1) / 256.0, 0.0, 0.0]))
            v = np.array([r.integers(24, 40) / 1024.0 * r.choice([-1, 1]), r.integers(8, 24) / 1024.0 * r.choice([-1, 1]),
                          r.choice([-1, 1]) / 4096.0])
            members = [c + v, c - v] + ([c + v * np.array([-1.0, 1.0, 1.0])] if triple else [])
            sign_z = [np.sign(v[2]), -np.sign(v[2])] + ([np.sign(v[2])] if triple else [])
            n_f, n_m = len(grp), len(members)
            slot = ids[used:used + n_f + n_m]
            used += n_f + n_m
            for f in range(n_f):
                nodes_b[slot[f]] = grp[f].astype(F32)
            mid = np.sort(slot[n_f:])                                      # the members' ids, ascending
            if r.integers(0, 2):
                mid = mid[::-1]                                            # coin: the un-stepped (nearest) member has the HIGHEST id
            for t in range(n_m):
                p = members[t].astype(F32)
                assert (p.astype(np.float64) == members[t]).all()         # the grid is exact in float32
                if t > 0:
                    u = int(np.rint(2.0 ** r.uniform(0, IB)))              # 1 .. 2^IB steps, log-uniform
                    # away from the centre in z: up when the member sits above the centre
                    up = sign_z[t] > 0
                    p[2:3] = step_ulps(p[2:3], np.array([u]), away_from_zero=(p[2] > 0) == up)
                nodes_b[mid[t]] = p
        far = M - used                                                     # left-over nodes: far away, distinct
        for t in range(far):
            nodes_b[ids[used + t]] = np.array([3.0 + t / 64.0, 3.0, 3.0], F32)
        node[b] = nodes_b.T
        x[b, :, :C] = centres.T.astype(F32)
        x[b, :, C:] = r.uniform(-1, 1, (3, n_gen)).astype(F32)
        perm = r.permutation(N)
        x[b] = x[b][:, perm]
        kinds[b] = kinds[b][perm]
    return x, node, kinds


NEAR_TIE_CASES = [  # (B, M, k, seed)
    (6, 64, 3, 11), (6, 64, 1, 12), (5, 64, 4, 13), (3, 100, 2, 14), (2, 256, 3, 15), (2, 256, 4, 16)]


def near_tie_case(case):
    B, M, k, seed = case
    x, node, kinds = near_ties(B, M, k, seed)
    return x, node, k, kinds


# ------------------------------------------------------------------------------------------ C. occupancy and size edges
def occupancy_cases():
    """-> list of (name, x, node, k)."""
    out = []
    r = np.random.default_rng(77)

    def add(name, x, node, k):
        out.append((name, np.ascontiguousarray(x, F32), np.ascontiguousarray(node, F32), k))

    # all points coincide (every workgroup's copies go to the same k nodes)
    for N, M, k in [(1025, 64, 4), (512, 9, 1)]:
        x = np.repeat(np.array([0.3, -0.2, 0.1], F32)[None, :, None], N, axis=2).repeat(2, axis=0)
        add("coincide_N%d_M%d_k%d" % (N, M, k), x, uniform(2, M, 5 + M), k)
    # all points nearest to one node, the others far away (k = 1: M - 1 empty nodes)
    for N, M, k, j0 in [(1025, 64, 1, 37), (2048, 64, 4, 0), (513, 63, 3, 62), (1300, 100, 1, 99)]:
        node = (uniform(1, M, 6 + M) * F32(0.5) + F32(5.0)).astype(F32)
        node[:, :, j0] = np.array([0.1, 0.2, -0.3], F32)
        x = (node[:, :, j0:j0 + 1] + F32(0.05) * uniform(1, N, 7 + N)).astype(F32)
        add("one_node_N%d_M%d_k%d" % (N, M, k), x, node, k)
    # every point duplicated (what the shapenet loader does when it has fewer samples than N)
    for N, M, k in [(1025, 64, 3), (512, 36, 2)]:
        h = (N + 1) // 2
        x0 = uniform(3, h, 8 + N)
        add("dup_points_N%d_M%d_k%d" % (N, M, k), np.concatenate([x0, x0[:, :, :N - h]], axis=2), uniform(3, M, 9 + M), k)
    # duplicated nodes: the lower id wins every slot it ties for
    for N, M, k in [(700, 64, 3), (511, 65, 4), (300, 4, 2)]:
        node = uniform(2, M, 10 + M)
        node[:, :, M // 2:2 * (M // 2)] = node[:, :, :M // 2]
        add("dup_nodes_N%d_M%d_k%d" % (N, M, k), uniform(2, N, 11 + N), node, k)
    # points that sit on nodes (distance 0)
    for N, M, k in [(513, 64, 3), (100, 100, 1)]:
        x, node = uniform(2, N, 12 + N), uniform(2, M, 13 + M)
        pick = r.permutation(N)[:min(N, M) // 2]
        node[:, :, :len(pick)] = x[:, :, pick]
        add("point_on_node_N%d_M%d_k%d" % (N, M, k), x, node, k)
    # sizes: N around the 512-point workgroup, M with and without a tail of the 8-wide visit loop, every k up to k == M, B = 1 and odd B
    sizes = [(1, 1, 1, 1), (1, 2, 4, 4), (3, 511, 9, 1), (1, 512, 36, 2), (5, 513, 63, 3), (1, 1023, 65, 4), (3, 1025, 100, 3),
             (1, 1025, 1024, 4), (1, 2, 1, 1), (3, 1, 4, 3), (1, 511, 4, 4), (3, 512, 1, 1), (1, 513, 9, 4), (1, 1023, 1024, 1),
             (3, 2, 63, 2), (1, 1, 65, 4), (1, 3, 3, 3), (5, 1025, 2, 2)]
    for B, N, M, k in sizes:
        x, node = lattice(B, N, M, 4, seed=14 + N + M) if (N + M) % 2 else (uniform(B, N, 15 + N), uniform(B, M, 16 + M))
        add("size_B%d_N%d_M%d_k%d" % (B, N, M, k), x, node, k)
    return out


REJECTED_SHAPES = [(64, 1025, 3), (3, 3, 4), (64, 64, 5), (600, 2, 3)]      # (N, M, k): refused before a launch


# ------------------------------------------------------------------------------------------ D. overflow and NaN
BIG = F32(2e19)         # finite, its square is not: (2e19)^2 = 4e38 > FLT_MAX = 3.4e38; sums of thousands of them stay finite in f64 and f32


def overflow_cases():
    """-> list of (name, x, node, k).  Ordinary clouds with a few far points at (+-BIG, y, z): their squared distance to every ordinary
    node is +inf.  ``n_fin`` nodes share the far x coordinate (dx = 0: finite distance) -- none, one, or k - 1 --, placed at the lowest
    ids (node 0 finite) or at the highest (node 0 not finite)."""
    out = []
    for M, k, n_fin, low in [(64, 3, 0, True), (64, 3, 1, True), (64, 3, 1, False), (64, 3, 2, True), (64, 3, 2, False),
                             (64, 1, 0, True), (64, 4, 3, False), (64, 4, 1, True), (100, 4, 3, True), (100, 2, 0, False),
                             (100, 2, 1, False), (9, 4, 3, False), (4, 4, 3, True), (1, 1, 0, True)]:
        B, N = 2, 1100
        x, node = uniform(B, N, 20 + M + k), uniform(B, M, 21 + M + n_fin)
        far = np.array([0, 1, 255, 256, 511, 512, 513, 1024, 1099])
        x[:, 0, far] = BIG
        x[1, 0, far[::2]] = -BIG
        for b in range(B):
            ids = np.arange(n_fin) if low else M - 1 - np.arange(n_fin)
            node[b, 0, ids] = BIG if b == 0 else -BIG                      # (cloud 1: finite only for its -BIG points)
        out.append(("overflow_M%d_k%d_fin%d_%s" % (M, k, n_fin, "low" if low else "high"), x, node, k))
    return out


def nan_cases():
    """-> list of (name, x, node, k): a few points with a NaN coordinate (every distance NaN), a node with one (NaN for every point)."""
    out = []
    for M, k, nan_node in [(64, 3, None), (64, 3, 0), (64, 3, 63), (100, 4, 1), (4, 4, 2)]:
        x, node = uniform(2, 600, 30 + M), uniform(2, M, 31 + M)
        x[:, 1, [0, 300, 511, 512, 599]] = np.nan
        if nan_node is not None:
            node[:, 2, nan_node] = np.nan
        out.append(("nan_M%d_k%d_node%s" % (M, k, nan_node), x, node, k))
    return out


# ------------------------------------------------------------------------------------------ E. Chamfer sizes
CHAMFER_ND = [1, 2, 3, 1023, 1024, 1025, 2047, 2049]
CHAMFER_NQ = [1, 255, 256, 257]


def chamfer_case(Nq, Nd, B=2, q=4):
    """Lattice clouds: the second half of the database repeats the first (ties between far-apart indices), every other query is a
    database point (distance 0).  -> q B x 3 x Nq, db B x 3 x Nd."""
    r = np.random.default_rng(5000 + 7 * Nq + Nd)
    db = (np.rint(r.uniform(-1, 1, (B, 3, Nd)) * q) / q).astype(F32)
    h = Nd // 2
    if h:
        db[:, :, Nd - h:] = db[:, :, :h][:, :, r.permutation(h)]
    qs = (np.rint(r.uniform(-1, 1, (B, 3, Nq)) * 2 * q) / (2 * q)).astype(F32)      # a finer lattice: ties between distinct points too
    take = r.integers(0, Nd, Nq)
    qs[:, :, ::2] = db[:, :, take[::2]]
    return qs, db


def chamfer_cases():
    return [(Nq, Nd) for Nd in CHAMFER_ND for Nq in CHAMFER_NQ]
