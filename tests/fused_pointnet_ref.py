"""Host restatement of the fused first PointNet (so-net_amd/csrc/pointresnet_fused.hip), the seeded networks its tests run, and the
node layouts of its pool variant.

``forward64`` is PointResNet.forward (models/layers.py: 6 -> 64 -> 128 -> 256 -> [64 + 256] -> 384, eval BatchNorm folded to ``affine``) in
float64; ``pool64`` is the per-node max-pool of models/networks.py:175-185 (running maximum started at -1000, gather index 0 where nothing
beat it).  ``split_forward`` restates the kernel's ARITHMETIC -- the fp16 pieces of every operand, tests/h3_model.py flavour "h3p", chained
through the four layers -- with every product and sum in float64.

Exact networks: weights, inputs, scales and shifts chosen so that every fp16 piece, every partial sum, every affine result and every output
is representable where the kernel keeps it.  The kernel's result is then THE float64 result, bit for bit, whatever the order of its
accumulation: a permuted channel, a stale register, a missed flush or a tail error changes bits.  tests/test_fused_pointnet_cpu.py derives
the exactness from the pieces; nothing here is fitted to what the kernel returns.

Deliberate breaks are parameters of the restatements (``brk=``), never of the library.
"""
import functools

import numpy as np
import torch

import h3_model as H

C1, C2, C3, C4 = 64, 128, 256, 384
LB = (0, C1, C1 + C2, C1 + C2 + C3)                # first row of each layer in ``affine``
CH_TOTAL = C1 + C2 + C3 + C4                       # 832
CIN0S = (1, 3, 6, 8, 9, 16)
TPTS, CTILE, SEG_SLOTS = 256, 32, 16               # points per workgroup tile / per column tile; nodes of a tile pre-reduced in LDS
BREAKS_FORWARD = ("swap", "panels")
BREAKS_POOL = ("ge", "boundary", "slot16")


def same_bits(a, b):
    """float32 arrays equal bit for bit (the sign of a zero aside: the pool's keys count -0 as +0, as torch.max does)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32, (a.dtype, b.dtype)
    return a.shape == b.shape and np.array_equal((a + np.float32(0)).view(np.uint32), (b + np.float32(0)).view(np.uint32))


def rms_ratio(got, ref):
    """The figure conftest.assert_close_rms bounds: the worst |got - ref| / max(|ref|, rms(ref))."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), np.sqrt(np.mean(ref ** 2)))).max())


def f32_exact(v64):
    """float64 array -> float32, refusing a value that float32 does not hold."""
    v32 = np.asarray(v64, np.float64).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v64), "not representable in float32"
    return v32


# ---------------------------------------------------------------------------------------------- restatements
def forward64(x, W1, W2, W3, W4, affine, brk=None, hidden=False):
    """x [B][Cin0][L] -> y [B][384][L] float64.  affine [832][2] = (scale, shift) per channel, layer after layer.
    brk: "swap" = layer 2 reads channels 5 and 6 of layer 1's output exchanged (a packing-order mistake inside a 16-channel chunk);
    "panels" = layer 4 reads [a3; a1] where it should read [a1; a3]."""
    assert brk in (None,) + BREAKS_FORWARD
    x, aff = np.asarray(x, np.float64), np.asarray(affine, np.float64)
    Ws = [np.asarray(W, np.float64) for W in (W1, W2, W3, W4)]
    assert aff.shape == (CH_TOTAL, 2) and x.ndim == 3 and Ws[3].shape == (C4, C1 + C3)

    def layer(i, inp, relu):
        n = Ws[i].shape[0]
        s, b = aff[LB[i]:LB[i] + n, 0].reshape(1, n, 1), aff[LB[i]:LB[i] + n, 1].reshape(1, n, 1)
        v = s * np.einsum("oc,bcl->bol", Ws[i], inp) + b
        return np.maximum(v, 0.0) if relu else v

    a1 = layer(0, x, True)
    a1_in = a1
    if brk == "swap":
        a1_in = a1.copy()
        a1_in[:, [5, 6]] = a1[:, [6, 5]]
    a2 = layer(1, a1_in, True)
    a3 = layer(2, a2, True)
    cat = np.concatenate((a3, a1) if brk == "panels" else (a1, a3), axis=1)          # skip channels first
    y = layer(3, cat, False)
    return (y, (a1, a2, a3)) if hidden else y


def pool64(y, ids, pos0, M, brk=None):
    """y [B][C][L], ids [B][L] non-decreasing, pos0 [B] -> [B][C][M], dtype of y.  Per node and channel: the maximum over the node's
    columns where it is strictly greater than -1000, else y[:, pos0] (empty nodes too); a NaN never wins.
    brk: "ge" = '>=' at -1000; "boundary" = in a full 32-column tile holding exactly two nodes the first column of the second node counts
    for the first; "slot16" = the columns of node (first node of a 256-column tile) + 16 inside that tile are dropped."""
    assert brk in (None,) + BREAKS_POOL
    y, ids = np.asarray(y), np.array(ids, dtype=np.int64)
    B, C, L = y.shape
    keep = np.ones((B, L), bool)
    if brk == "boundary":
        for b in range(B):
            for t in range(0, L - CTILE + 1, CTILE):
                seg = ids[b, t:t + CTILE]
                if seg[0] != seg[-1] and len(np.unique(seg)) == 2:
                    ids[b, t + int((seg == seg[0]).sum())] = seg[0]
    if brk == "slot16":
        for b in range(B):
            for t in range(0, L, TPTS):
                seg = ids[b, t:t + TPTS]
                keep[b, t:t + TPTS] &= seg != seg[0] + SEG_SLOTS
    out = np.empty((B, C, M), y.dtype)
    for b in range(B):
        fall = y[b][:, int(pos0[b])]
        out[b] = fall[:, None]
        for m in np.unique(ids[b][keep[b]]):
            cols = y[b][:, (ids[b] == m) & keep[b]]
            with np.errstate(invalid="ignore"):
                mx = np.fmax.reduce(cols, axis=1)                                   # fmax: a NaN operand is ignored
                win = (mx >= -1000.0) if brk == "ge" else (mx > -1000.0)            # (an all-NaN node compares false)
            out[b][:, int(m)] = np.where(win, mx, fall)
    return out + y.dtype.type(0)                                                    # -0 -> +0


def sort_group(x, ids, pos0, M):
    """The dict ops.som_sort_group returns, built by hand from per-column node ids: x [B][Cin0][L] float32 and ids [B][L] in the SAME column
    order, pos0 [B] = column of original copy 0 in that order.  Columns are sorted by node (stable), node_off is the exclusive prefix of
    the node counts -- what som_sort_group_kernel writes.  CPU tensors; the caller moves them."""
    x, ids = np.asarray(x, np.float32), np.asarray(ids, np.int64)
    B, _, L = x.shape
    assert ids.shape == (B, L) and ids.min() >= 0 and ids.max() < M, "node ids must lie in [0, M)"
    xs, ids_s, p0 = np.empty_like(x), np.empty((B, L), np.int32), np.empty((B,), np.int32)
    count = np.zeros((B, M), np.int32)
    for b in range(B):
        order = np.argsort(ids[b], kind="stable")
        xs[b], ids_s[b] = x[b][:, order], ids[b][order]
        p0[b] = int(np.nonzero(order == int(pos0[b]))[0][0])
        count[b] = np.bincount(ids[b], minlength=M)
    node_off = (np.cumsum(count, axis=1) - count).astype(np.int32)
    assert (ids_s[:, 1:] >= ids_s[:, :-1]).all()
    return dict(x_aug_sorted=torch.from_numpy(xs), ids_sorted=torch.from_numpy(ids_s), pos0=torch.from_numpy(p0),
                node_off=torch.from_numpy(node_off), count=torch.from_numpy(count))


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic, in float64
def split_w(W):
    """-> (Wh, Wr) = fp16(32 w), fp16(32 w - Wh): the two slices of the weight stream (pointresnet_pack_kernel)."""
    W32 = np.clip(np.float32(32.0) * np.asarray(W, np.float32), np.float32(-65504.0), np.float32(65504.0))
    Wh = H.f16(W32)
    return Wh, H.f16(W32 - Wh)


def split_forward(x, W1, W2, W3, W4, affine):
    """The fused kernel's arithmetic with every product and sum in float64 -> (y float64 [B][384][L], per-layer records).  Each record holds
    the pieces (Xh, Xm of 32 x; Wh, Wr of 32 w), the operands they stand for (x, w), the float64 accumulator (1024 W.x), sum_abs = the sum
    of |term| over the three product sets, and pre = the affine's float64 result before it is rounded to float32 (32 x for layers 1-3, y
    for layer 4)."""
    aff = np.asarray(affine, np.float32)
    Ws = [np.asarray(W, np.float32) for W in (W1, W2, W3, W4)]
    recs = []

    def layer(i, xin, last):
        Xh, Xm = H.split_x(xin)                                                     # clamp to +-2047, 32 x, two fp16 roundings
        Wh, Wr = split_w(Ws[i])
        Xh64, Xm64, Wh64, Wr64 = (a.astype(np.float64) for a in (Xh, Xm, Wh, Wr))
        ein = lambda w, v: np.einsum("oc,bcl->bol", w, v)
        acc = ein(Wr64, Xh64) + ein(Wh64, Xm64) + ein(Wh64, Xh64)
        sum_abs = ein(np.abs(Wr64), np.abs(Xh64)) + ein(np.abs(Wh64), np.abs(Xm64)) + ein(np.abs(Wh64), np.abs(Xh64))
        n = Ws[i].shape[0]
        s, b = aff[LB[i]:LB[i] + n, 0], aff[LB[i]:LB[i] + n, 1]
        if last:                                                                    # y = fma(acc, scale / 1024, shift)
            k, c = (s * np.float32(2.0 ** -10)).astype(np.float64), b.astype(np.float64)
        else:                                                                       # 32 x = fma(acc, scale / 32, 32 shift)
            k, c = (s * np.float32(2.0 ** -5)).astype(np.float64), (np.float32(32.0) * b).astype(np.float64)
        pre = acc * k.reshape(1, n, 1) + c.reshape(1, n, 1)
        recs.append(dict(x=np.asarray(xin, np.float32), w=Ws[i], Xh=Xh, Xm=Xm, Wh=Wh, Wr=Wr, acc=acc, sum_abs=sum_abs, pre=pre))
        out = pre.astype(np.float32)
        if last:
            return out
        return np.clip(out, np.float32(0), np.float32(65504.0)) * np.float32(2.0 ** -5)    # ReLU and the fp16 range clamp on 32 x

    a1 = layer(0, np.asarray(x, np.float32), False)
    a2 = layer(1, a1, False)
    a3 = layer(2, a2, False)
    y = layer(3, np.concatenate((a1, a3), axis=1), True)
    return recs[3]["pre"], recs


def p16_planes(y):
    """float32 [B][C][L] -> the P16 planes of include/sonet_hip.h as uint16 [B][ceil(C/16)][piece][half][L][8]: fp16(32 y) and
    fp16(32 y - that) of the value clamped to +-2047; channel 16 kc + 4 half + (e & 3) + 8 (e >> 2)."""
    y = np.asarray(y, np.float32)
    B, C, L = y.shape
    KC = (C + 15) // 16
    pad = np.zeros((B, KC * 16, L), np.float32)
    pad[:, :C] = y
    X = np.float32(32.0) * np.clip(pad, np.float32(-2047.0), np.float32(2047.0))
    hi = X.astype(np.float16)
    lo = (X - hi.astype(np.float32)).astype(np.float16)
    out = np.empty((B, KC, 2, 2, L, 8), np.uint16)
    for h in range(2):
        for e in range(8):
            ch = 4 * h + (e & 3) + 8 * (e >> 2)
            out[:, :, 0, h, :, e] = hi[:, ch::16].view(np.uint16)
            out[:, :, 1, h, :, e] = lo[:, ch::16].view(np.uint16)
    return out


def p16_planes_flat(out, Lm):
    """The pooled map [B][384][M] on the flat column axis of the node-level stage (column b M + m of Lm) -> planes [24][2][2][B M][8]."""
    B, C, M = out.shape
    flat = np.ascontiguousarray(np.transpose(out, (1, 0, 2)).reshape(1, C, B * M))
    assert B * M <= Lm
    return p16_planes(flat)[0]


# ---------------------------------------------------------------------------------------------- seeded networks
class Net:
    """Weights [Cout][Cin] float32, affine [832][2] float32 and a seeded input maker."""

    def __init__(self, name, Ws, affine, make_x, pool=None):
        self.name, self.Ws, self.affine, self.make_x = name, tuple(np.ascontiguousarray(W, dtype=np.float32) for W in Ws), affine, make_x
        self.pool = pool                                   # exact networks: [Cin0][POOL], every column make_x can return
        self.cin0 = self.Ws[0].shape[1]
        self._pool_ref = None

    def x_and_ref(self, B, L, seed=0):
        """Exact networks: (make_x(B, L, seed), its float32 reference).  A column's result depends on that column alone, so forward64 runs
        ONCE, over the pool's 2048 columns, and every case gathers from it (tests/test_fused_pointnet_cpu.py checks it against ref())."""
        x, idx = self.make_x(B, L, seed, with_index=True)
        if self._pool_ref is None:
            self._pool_ref = f32_exact(self.ref(self.pool[None]))[0]
        return x, np.ascontiguousarray(np.transpose(self._pool_ref[:, idx], (1, 0, 2)))

    def ref(self, x, brk=None, hidden=False):
        return forward64(x, *self.Ws, self.affine, brk=brk, hidden=hidden)

    def with_affine(self, affine):
        return Net(self.name, self.Ws, np.ascontiguousarray(affine, dtype=np.float32), self.make_x, self.pool)


def _sparse_rows(rng, cout, cin, nnz, values, tails, probe=None, scale=1.0):
    """cout rows of nnz non-zeros drawn from ``values`` (fewer where the row is shorter), each with a shift drawn from ``tails``
    -> (W, shifts).  No two (row, shift) pairs are equal.  probe [cin][n] (hidden layers): the row's activation relu(scale row . probe +
    shift) must be active on 10 % to 90 % of the probe columns and differ from every earlier row's -- a dead channel, or two channels
    that agree, could hide a permutation."""
    W, kept, seen, acts, deck = np.zeros((cout, cin), np.float64), [], set(), set(), []
    while len(kept) < cout:
        row = np.zeros(cin)
        # the columns come off a deck of shuffled permutations: every input channel is used equally often (no all-zero weight column)
        cols = []
        while len(cols) < min(nnz, cin):
            if not deck:
                deck = list(rng.permutation(cin))
            c = deck.pop()
            if c not in cols:
                cols.append(c)
        row[cols] = rng.choice(values, size=len(cols))
        t = float(rng.choice(tails))
        if (tuple(row), t) in seen:
            continue
        if probe is not None:
            act = np.maximum(scale * (row @ probe) + t, 0.0)
            if not 0.1 <= (act > 0).mean() <= 0.9 or act.tobytes() in acts:
                continue
            acts.add(act.tobytes())
        seen.add((tuple(row), t))
        W[len(kept)] = row
        kept.append(t)
    if cin > 1 and len(np.unique(W.T, axis=0)) != cin:                              # two input channels with the same weights: draw again
        return _sparse_rows(rng, cout, cin, nnz, values, tails, probe, scale)
    return W, np.array(kept)


SCALES = (1.0, 2.0 ** -2, 2.0 ** -3)               # hidden layers; powers of two: the affine moves no bit
NNZ = {"A": (4, 6, 6, 8), "B": (4, 3, 3, 4)}       # non-zeros per weight row (B: see the bit budget below)
XMAX = {"A": 8, "B": 2}
POOL, PROBE = 2048, 512                            # seeded input columns of an exact network; those its rows are drawn against
SPECIAL = 3                                        # layer-4 channels 0..2 carry the -1000 cases of the pool


@functools.lru_cache(maxsize=None)
def exact_network(cin0, flavour, l4="unit"):
    """Flavour A: weights in {0, +-1, +-2} (weight residual slice 0), integer inputs in [-8, 8].  The hidden scales 1, 2^-2, 2^-3 move no bit,
    so the significant bits of an activation come from its magnitude and from the granule of its shift: layer 1's shifts are multiples of
    2^-7 in [-4, 4], which gives a1 14 bits, a2 (granule 2^-9) 15 and a3 (granule 2^-12) 18 -- beyond fp16's 11, so the activation
    residual pieces of layers 2, 3 and 4 are in use; the other shifts are integers in [-4, 4].
    Flavour B: W1 = k + j 2^-12 (32 w1 does not fit fp16: the weight residual slice of layer 1 is j 2^-7), inputs of two bits (activation
    residual 0 where the weight residual is not).  Bit budget of B: a1 has granule 2^-12, a2 2^-14, a3 2^-17 and y 2^-17 times the layer-4
    scale; float32 holds 24 bits and a sum is exact only while sum |terms| / granule < 2^24, which leaves the later layers of B three and
    four non-zeros per row, inputs in [-2, 2] and quarter-integer shifts in layer 1 (4 weights x 33 shifts: 64 live rows over ONE input
    channel can still all differ).
    l4: layer-4 scales "unit" (all 1: the pool takes its bias after the maximum), "half" (all 2^-1) or "mixed" (a third of the channels at
    -1, 2, -2^-1, ... : the pool's general branch).
    Layer-4 channels 0, 1, 2 are the pool's -1000 cases: y0 = -a1[0] - 1000 (a node's maximum is exactly -1000 where a1[0] has a zero in it),
    y1 = -a1[1] - 1001 (never beats -1000), y2 = -1000 (constant)."""
    assert flavour in ("A", "B") and l4 in ("unit", "half", "mixed")
    rng = np.random.default_rng([2024, cin0, ord(flavour)])
    vals = np.array([-2.0, -1.0, 1.0, 2.0])
    n1, n2, n3, n4 = NNZ[flavour]
    xmax = XMAX[flavour]
    # every input column comes from one pool of 2048 seeded columns: what the CPU test derives for the pool holds for every input drawn
    pool = np.random.default_rng([77, cin0, ord(flavour)]).integers(-xmax, xmax + 1, size=(cin0, POOL)).astype(np.float32)
    ints = np.arange(-4.0, 5.0)
    relu = lambda v: np.maximum(v, 0.0)
    p0 = pool[:, :PROBE].astype(np.float64)
    W1, b1 = _sparse_rows(rng, C1, cin0, n1, vals, np.arange(-512, 513) / 128.0 if flavour == "A" else np.arange(-16, 17) / 4.0, p0, SCALES[0])
    if flavour == "B":
        j = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=W1.shape)
        W1 = W1 + (W1 != 0) * j * 2.0 ** -12
    p1 = relu(SCALES[0] * (W1 @ p0) + b1[:, None])
    W2, b2 = _sparse_rows(rng, C2, C1, n2, vals, ints, p1, SCALES[1])
    p2 = relu(SCALES[1] * (W2 @ p1) + b2[:, None])
    W3, b3 = _sparse_rows(rng, C3, C2, n3, vals, ints, p2, SCALES[2])
    W4, b4 = _sparse_rows(rng, C4, C1 + C3, n4, vals, ints)
    aff = np.zeros((CH_TOTAL, 2))
    aff[LB[0]:LB[1], 0], aff[LB[1]:LB[2], 0], aff[LB[2]:LB[3], 0] = SCALES
    aff[:, 1] = np.concatenate((b1, b2, b3, b4))
    aff[LB[3]:, 0] = 1.0 if l4 != "half" else 0.5
    if l4 == "mixed":
        third = np.arange(SPECIAL, C4)[rng.permutation(C4 - SPECIAL)[:C4 // 3]]
        aff[LB[3] + third, 0] = rng.choice(np.array([-1.0, 2.0, -0.5, 0.5, -2.0]), size=len(third))
    W4[:SPECIAL] = 0.0
    W4[0, 0], W4[1, 1] = -1.0, -1.0
    aff[LB[3]:LB[3] + SPECIAL, 0] = 1.0
    aff[LB[3]:LB[3] + SPECIAL, 1] = (-1000.0, -1001.0, -1000.0)

    def make_x(B, L, seed=0, with_index=False):
        idx = np.random.default_rng([78, cin0, B, L, seed]).integers(0, POOL, size=(B, L))
        x = np.ascontiguousarray(np.transpose(pool[:, idx], (1, 0, 2)))
        return (x, idx) if with_index else x
    return Net("exact%s_cin%d_%s" % (flavour, cin0, l4), (W1, W2, W3, W4), f32_exact(aff), make_x, pool=pool)


_CONT = {}


def continuous_network(cin0=6):
    """The seeded network of the parity tests: synth.fill_state_dict_(PointResNet(cin0, ...), seed=7), BatchNorm folded in float64 and
    rounded to the float32 ``affine`` the kernel reads -> (Net, the torch module in float64 on the CPU)."""
    if cin0 not in _CONT:
        from models import layers as ML
        from sonet_hip import synth
        pr = ML.PointResNet(cin0, [C1, C2, C3, C4], "relu", "batch", 0.1, None, 1)
        synth.fill_state_dict_(pr.state_dict(), seed=7)
        pr = pr.double().eval()
        Ws, sc, sh = [], [], []
        for lay in pr.layers:
            w = lay.conv.weight.detach()
            Ws.append(w.reshape(w.shape[0], w.shape[1]).numpy())
            b = lay.conv.bias.detach() if lay.conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
            if lay.normalization == "batch":
                s = lay.norm.weight.detach() / torch.sqrt(lay.norm.running_var + lay.norm.eps)
                h = (b - lay.norm.running_mean) * s + lay.norm.bias.detach()
            else:
                s, h = torch.ones_like(b), b
            sc.append(s.numpy())
            sh.append(h.numpy())
        aff = np.stack((np.concatenate(sc), np.concatenate(sh)), axis=1).astype(np.float32)

        def make_x(B, L, seed=0):
            inp = synth.make_inputs(B, L, M=1, som_k=1, seed=seed)                  # coordinates in [-1, 1], unit normals
            return np.ascontiguousarray(torch.cat((inp["pc"], inp["sn"]), dim=1).numpy()[:, :cin0])
        _CONT[cin0] = (Net("continuous_cin%d" % cin0, Ws, aff, make_x), pr)
    return _CONT[cin0]


# ---------------------------------------------------------------------------------------------- node layouts of the pool variant
def _runs(*pairs):
    return np.concatenate([np.full(n, m, np.int64) for m, n in pairs])


def _spread(L, ids):
    """L columns over the given node ids, evenly, in order."""
    ids = np.asarray(ids, np.int64)
    return ids[(np.arange(L) * len(ids)) // L]


def layouts(cus):
    """name -> (ids [B][L] non-decreasing, pos0 [B], M): the layouts of the pool epilogue's code paths (two-node sweep, general loop, LDS
    bins, straight-to-memory atomics) and of the decode kernel's stitching, reached on purpose."""
    out = {}
    # 1. two nodes in a full 32-column tile, the boundary at every e = 1..31 (one cloud per e)
    out["two_nodes_every_boundary"] = (np.stack([_runs((0, e), (1, 32 - e)) for e in range(1, 32)]), np.arange(31) % 32, 2)
    # 2. three nodes in a column tile; 32 one-point nodes (slots 16..31 go straight to memory)
    out["three_nodes_and_one_point_nodes"] = (np.stack([_runs((0, 10), (1, 10), (2, 12)), np.arange(32)]), np.array([11, 20]), 32)
    # 3. a ragged last column tile (7 of 32 columns) holding one node, and holding two
    out["ragged_last_tile"] = (np.stack([_runs((0, 32), (1, 7)), _runs((0, 32), (1, 3), (2, 4))]), np.array([38, 33]), 3)
    # 4. a 256-point tile with 17, 18 and 64 distinct ids
    out["tile_17_18_64_ids"] = (np.stack([_spread(256, np.arange(n)) for n in (17, 18, 64)]), np.array([0, 100, 255]), 64)
    # 5. tile 0 begins with node 1, so node 19 begins at slot 19 - 1 = 18 of tile 0 (straight to memory) and continues as slot 0 of
    #    tile 1 (LDS bins); 8. node 0 and node M - 1 empty
    out["slot18_continues_as_slot0"] = (np.stack([np.concatenate((_spread(240, np.arange(1, 19)), _runs((19, 60)), _spread(212, np.arange(20, 31))))]),
                                        np.array([250]), 33)
    # 6. a tile holding only ids n and n + 20: the slot comes from the id difference, not from a count of nodes
    out["ids_n_and_n_plus_20"] = (np.stack([_runs((3, 100), (23, 156)), _runs((0, 255), (20, 1))]), np.array([99, 255]), 33)
    # 7. a node spanning four tiles (columns 100..899), L = 1024
    out["node_spans_four_tiles"] = (np.stack([_runs((0, 100), (1, 800), (2, 124))]), np.array([512]), 4)
    # 8. empty nodes 0, M - 1 and 4
    out["empty_nodes"] = (np.stack([_spread(300, [1, 2, 3, 5, 6, 7]), _spread(300, [2, 3, 5, 7])]), np.array([0, 299]), 9)
    # 10. pos0 at the tile edges, different per cloud
    ids3 = np.stack([_spread(300, np.arange(5))] * 3)
    out["pos0_0_31_32"] = (ids3, np.array([0, 31, 32]), 5)
    out["pos0_255_256_last"] = (ids3, np.array([255, 256, 299]), 5)
    # 11. M = 1, 33, 64, 65 (the decode kernel's 32-node blocks: one partial block, two whole ones, a third of one node)
    for M in (1, 33, 64, 65):
        out["M%d" % M] = (np.stack([_spread(300, np.arange(M)), _spread(300, np.arange(M)[::-1][:max(1, M // 2)][::-1])]), np.array([7, 290]), M)
    # 12. more clouds than compute units, a 40-point tile each: every workgroup flushes a tile's bins during its next tile, and its last
    #     tile's at the end
    B = cus + 3
    rows = []
    for b in range(B):
        n_nodes = 1 + b % 4                                 # 1..4 nodes, the first n_nodes ids ...
        first = 1 if (b % 3 == 0 and n_nodes < 4) else 0    # ... moved up by one in every third cloud where that stays below M = 4
        rows.append(_spread(40, first + np.arange(n_nodes)))
    out["persistent_small_clouds"] = (np.stack(rows), np.arange(B) % 40, 4)
    return out
