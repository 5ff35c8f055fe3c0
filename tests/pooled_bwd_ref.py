"""The pooled-layer backward (so-net_amd/csrc/pooled_bwd.hip) restated in numpy: the order of every fma chain and every add the kernels
document, so that a GPU result can be asked to be bit-equal; and the dense float64 expressions of the same two gradients.

  fma32                 the f32 fma through float64: the product of two f32 numbers is exact in float64, the sum is taken with TwoSum, and
                        where the float64 sum sits exactly on the midpoint of two f32 numbers while its error term is not zero the sum is
                        stepped one float64 towards the error's sign before it is rounded (tests/bn_passes_ref.py treats the same double
                        rounding by counting near-ties; here they are corrected, and counted in ``FMA_FIXES``)
  lists                 what pooled_bucket_kernel + pooled_sort_kernel leave behind: per cloud the valid entries by (column, entry id),
                        entry id = c * M + m, and the offsets of the 32-column buckets
  dgrad_plain           pooled_dgrad_kernel (C1 + C2 no multiple of 4) and its column-owned twin: one chain per (column, channel)
  dgrad_balanced        pooled_dgrad5_kernel: rounds of 384 entries of a 128-column tile in sixteen chunks of equal length
  wgrad_bits            pooled_wgrad_kernel: per cloud, two half chains per (channel, row), one add
  dgrad64 / wgrad64     scatter-add, then a matmul, in float64; with sum |term| and the number of terms per output element

Every ``breaks`` argument names mistakes a kernel could make (``BREAKS``); tests/test_pooled_bwd_cpu.py asserts that each layout built
here ends on other bits under the break it was built for.  The constants below are restated from pooled_bwd.hip once."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import pooled_bits as P  # noqa: E402  (the splitmix64 inputs: imported, not copied)

# pooled_bwd.hip
PD_TL, PD_CH, PD_SB, PD_SQ = 128, 40, 32, 128
PD_KEY_IDS = 1 << 20
PB_Q, PB_SCAN = 4, 1024                      # workgroups per cloud in the bucket kernel; buckets of a quarter the parallel scan takes
PS_CAP = 2048
PD5_R, PD5_G = 384, 16
PM_TL, PM_PITCH, PM_BIG = 64, 784, 2048      # matrix cores: columns per 64-column workgroup, G^T pitch, B * ceil(L / 128) for 128 columns
PW_ROWS, PW_M, PW_T, PW_CMAX, PW_LDS = 16, 64, 768, 384, 152 * 1024
L_MAX = ((64 * 1024 // 4 - 1) // 2) * PD_SB  # (2 * nbucket + 1) * 4 <= 64 KiB: nbucket <= 8191

INT_GRANULE = 2.0 ** -7
BREAKS = ("sort_by_id", "rem_last", "head_reverse", "drop_last_bucket", "pos_eq_L", "one_chain", "bf16_trunc")

FMA_FIXES = [0]                              # midpoint corrections fma32 has made (the CPU test asserts the count)


# ------------------------------------------------------------------------------------------------------------ number formats
def fma32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, as v_fma_f32 / __fmaf_rn; a, b, c float32 (broadcast)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                              # exact: 48 significant bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                        # TwoSum: p + c = s + err exactly
        s = np.array(s, np.float64, ndmin=1)
        fix = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (np.broadcast_to(err, s.shape) != 0) & np.isfinite(s)
        if fix.any():
            FMA_FIXES[0] += int(fix.sum())
            e = np.broadcast_to(err, s.shape)[fix]
            s[fix] = np.nextafter(s[fix], np.where(e > 0, np.inf, -np.inf))
        return s.astype(np.float32).reshape(np.broadcast(a, b, c).shape)


def bf16_rne(x32, trunc=False):
    """f32 -> bf16 bit patterns (uint16), round to nearest even: (u + 0x7FFF + ((u >> 16) & 1)) >> 16.  (NaN inputs: compare NaN-aware.)"""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    if trunc:
        return (u >> np.uint64(16)).astype(np.uint16)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def widen(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def to_bf16(x32):
    """the nearest-even bf16 value, held in f32"""
    return widen(bf16_rne(x32))


def bf16_of_f64(v64):
    """the nearest-even bf16 number of a float64 value, in ONE rounding (normal range), as float64"""
    m, e = np.frexp(np.asarray(v64, np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)                  # (rint: halfway cases to the even neighbour)


def same_bits(a, b):
    """bit equality that lets any NaN equal any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.uint16:
        fa, fb = widen(a), widen(b)
    else:
        fa, fb = a, b
    nan = np.isnan(fa) & np.isnan(fb)
    ua, ub = a.view("u%d" % a.dtype.itemsize), b.view("u%d" % b.dtype.itemsize)
    return bool(((ua == ub) | nan).all())


# ------------------------------------------------------------------------------------------------------------ the lists
def lists(pos, L, breaks=()):
    """pos [B][C][M] -> per cloud (ids, cols, tile_off): the valid entries (0 <= pos < L) sorted by (column, id), id = c * M + m, and
    tile_off[nbucket + 1], the offsets of the 32-column buckets in that list"""
    B = pos.shape[0]
    nbucket = -(-L // PD_SB)
    out = []
    for b in range(B):
        p = pos[b].reshape(-1).astype(np.int64)
        ok = (p >= 0) & ((p <= L) if "pos_eq_L" in breaks else (p < L))
        ids = np.nonzero(ok)[0]
        cols = p[ids]
        if "drop_last_bucket" in breaks:
            keep = cols // PD_SB < nbucket - 1
            ids, cols = ids[keep], cols[keep]
        key = cols // PD_SB if "sort_by_id" in breaks else cols
        order = np.argsort(key, kind="stable")                 # (ids ascend already: a stable sort by column is the sort by (column, id))
        ids, cols = ids[order], cols[order]
        tile_off = np.searchsorted(cols // PD_SB, np.arange(nbucket + 1), side="left")
        out.append((ids, cols, tile_off.astype(np.int64)))
    return out


def bucket_sizes(pos, L):
    return [np.diff(t) for _, _, t in lists(pos, L)]


def tile_sizes(pos, L):
    """entries per 128-column tile, per cloud"""
    ntile = -(-L // PD_TL)
    return [np.bincount(c // PD_TL, minlength=ntile) for _, c, _ in lists(pos, L)]


def chunks(n, breaks=()):
    """the sixteen (start, length) of a round of n entries"""
    per, rem = divmod(n, PD5_G)
    if "rem_last" in breaks:
        return [(g * per + max(0, g - (PD5_G - rem)), per + (1 if g >= PD5_G - rem else 0)) for g in range(PD5_G)]
    return [(g * per + min(g, rem), per + (1 if g < rem else 0)) for g in range(PD5_G)]


# ------------------------------------------------------------------------------------------------------------ sparse dgrad
def _split(gx, C1, out, breaks):
    """[B][Cin][L] f32 -> (gx1, gx2 or None) in the output type"""
    if out == "bf16":
        gx = bf16_rne(gx, trunc="bf16_trunc" in breaks)
    return np.ascontiguousarray(gx[:, :C1]), (np.ascontiguousarray(gx[:, C1:]) if gx.shape[1] > C1 else None)


def dgrad_plain(g, pos, W, C1, L, out="f32", breaks=()):
    """per (cloud, column, input channel) ONE chain from 0 over the column's entries in id order: sum = fma32(g[id], W[id // M][ch], sum)"""
    B, C, M = g.shape
    Cin = W.shape[1]
    gx = np.zeros((B, Cin, L), np.float32)
    for b, (ids, cols, _) in enumerate(lists(pos, L, breaks)):
        gb = g[b].reshape(-1)
        acc = np.zeros((L + 1, Cin), np.float32)
        for e, col in zip(ids, cols):
            acc[col] = fma32(gb[e], W[e // M], acc[col])
        gx[b] = acc[:L].T
    return _split(gx, C1, out, breaks)


def dgrad_balanced(g, pos, W, C1, L, out="f32", breaks=()):
    """pooled_dgrad5_kernel: per (cloud, 128-column tile) the entries in (column, id) order, rounds of 384, sixteen chunks per round; a chunk
    that continues the column of the entry before it starts that column from 0 into head[g]; after the chunks the first chunk of a run on
    one column adds the run's heads to the accumulator in chunk order, with plain f32 adds"""
    B, C, M = g.shape
    Cin = W.shape[1]
    gx = np.zeros((B, Cin, L), np.float32)
    ntile = -(-L // PD_TL)
    for b, (ids, cols, tile_off) in enumerate(lists(pos, L, breaks)):
        gb = g[b].reshape(-1)
        acc = np.zeros((ntile * PD_TL + 1, Cin), np.float32)
        nbucket = len(tile_off) - 1
        for tile in range(ntile):
            beg, end = tile_off[min(tile * 4, nbucket)], tile_off[min(tile * 4 + 4, nbucket)]
            for base in range(beg, end, PD5_R):
                n = min(PD5_R, end - base)
                rid, rcol = ids[base:base + n], cols[base:base + n]
                head = np.zeros((PD5_G, Cin), np.float32)
                headcol = [-1] * PD5_G
                for grp, (lo, cnt) in enumerate(chunks(n, breaks)):
                    if cnt == 0:
                        continue
                    in_head = lo > 0 and rcol[lo - 1] == rcol[lo]
                    cur = rcol[lo]
                    if in_head:
                        headcol[grp] = cur
                    s = np.zeros(Cin, np.float32) if in_head else acc[cur].copy()
                    for e, col in zip(rid[lo:lo + cnt], rcol[lo:lo + cnt]):
                        if col != cur:
                            if in_head:
                                head[grp] = s
                            else:
                                acc[cur] = s
                            in_head, cur, s = False, col, acc[col].copy()
                        s = fma32(gb[e], W[e // M], s)
                    if in_head:
                        head[grp] = s
                    else:
                        acc[cur] = s
                for grp in range(1, PD5_G):
                    hc = headcol[grp]
                    if hc >= 0 and headcol[grp - 1] != hc:
                        run = [k for k in range(grp, PD5_G) if all(headcol[j] == hc for j in range(grp, k + 1))]
                        s = acc[hc].copy()
                        for k in (run[::-1] if "head_reverse" in breaks else run):
                            s = s + head[k]
                        acc[hc] = s
        gx[b] = acc[:L].T
    return _split(gx, C1, out, breaks)


def dgrad_bits(g, pos, W, C1, L, out="f32", breaks=()):
    """what ops.pooled_dgrad without a pack computes: the entry-balanced kernel when C1 + C2 is a multiple of 4, else the one-channel one"""
    return (dgrad_balanced if W.shape[1] % 4 == 0 else dgrad_plain)(g, pos, W, C1, L, out, breaks)


def balanced_stats(pos, L):
    """what a layout reaches in the entry-balanced kernel: ``ns`` the entries per round seen, ``rounds`` the most rounds of a tile,
    ``lengths`` the chunk lengths seen, ``span`` the most chunks one column of a round lies in, ``run_ends_on_edge`` a cut column whose last
    entry is the last of a chunk, ``crosses_round`` a column whose entries lie in two rounds"""
    st = dict(rounds=0, span=0, run_ends_on_edge=False, crosses_round=False, lengths=set(), ns=set())
    ntile = -(-L // PD_TL)
    for ids, cols, tile_off in lists(pos, L):
        nbucket = len(tile_off) - 1
        for tile in range(ntile):
            beg, end = tile_off[min(tile * 4, nbucket)], tile_off[min(tile * 4 + 4, nbucket)]
            st["rounds"] = max(st["rounds"], -(-(end - beg) // PD5_R))
            for base in range(beg, end, PD5_R):
                n = min(PD5_R, end - base)
                st["ns"].add(int(n))
                rcol = cols[base:base + n]
                if base > beg and cols[base - 1] == cols[base]:
                    st["crosses_round"] = True
                owner = np.zeros(n, np.int64)                  # the chunk of every entry of the round
                for k, (lo, cnt) in enumerate(chunks(n)):
                    st["lengths"].add(cnt)
                    owner[lo:lo + cnt] = k
                for col in np.unique(rcol):
                    ks = np.unique(owner[rcol == col])
                    st["span"] = max(st["span"], len(ks))
                    if len(ks) > 1:
                        last = np.nonzero(rcol == col)[0][-1]
                        lo, cnt = chunks(n)[owner[last]]
                        if last == lo + cnt - 1:
                            st["run_ends_on_edge"] = True
    return st


# ------------------------------------------------------------------------------------------------------------ sparse wgrad
def wgrad_rows(x, rows, triple=None, breaks=()):
    """the rows as the kernel holds them in LDS, in f32: x [B][Ci][L] f32 (``rows`` = "f32") or bf16 bits (uint16, "bf16"); with the triple
    (scale, shift, relu) f32 rows become act(fma32(raw, sc, sh)) with v < 0 -> 0, bf16 rows bf16_rne of the same"""
    xr = widen(x) if rows == "bf16" else np.asarray(x, np.float32)
    if triple is not None:
        sc, sh, relu = triple
        v = fma32(xr, np.asarray(sc, np.float32).reshape(1, -1, 1), np.asarray(sh, np.float32).reshape(1, -1, 1))
        if relu:
            v = np.where(v < 0, np.float32(0), v)
        xr = widen(bf16_rne(v, trunc="bf16_trunc" in breaks)) if rows == "bf16" else v
    return xr


def wgrad_parts(g_t, pos_t, x, rows="f32", triple=None, breaks=()):
    """per-cloud partials [B][C][Ci]: the chain over m = 0 .. 31 from 0 plus the chain over m = 32 .. 63 from 0; ignored entries skipped"""
    B, M, C = g_t.shape
    Ci, L = x.shape[1], x.shape[2]
    xr = wgrad_rows(x, rows, triple, breaks)
    half = PW_M if "one_chain" in breaks else PW_M // 2
    part = np.zeros((B, C, Ci), np.float32)
    for b in range(B):
        flat = xr[b].reshape(-1)
        acc = np.zeros((2, C, Ci), np.float32)
        for m in range(M):
            p = pos_t[b, m].astype(np.int64)
            ok = (p >= 0) & ((p <= L) if "pos_eq_L" in breaks else (p < L))
            if not ok.any():
                continue
            cs = np.nonzero(ok)[0]
            idx = np.arange(Ci)[None, :] * L + p[cs][:, None]                  # (pos == L under its break: the next row's first element)
            xv = np.where(idx < flat.size, flat[np.minimum(idx, flat.size - 1)], np.float32(0))
            h = m // half
            acc[h, cs] = fma32(g_t[b, m, cs][:, None], xv, acc[h, cs])
        part[b] = acc[0] + acc[1]
    return part


def wgrad_bits(g_t, pos_t, x, rows="f32", triple=None, breaks=()):
    """what ops.pooled_wgrad returns at B <= 3: the sequential f32 sum of the per-cloud partials"""
    part = wgrad_parts(g_t, pos_t, x, rows, triple, breaks)
    s = part[0].copy()
    for b in range(1, part.shape[0]):
        s = s + part[b]
    return s


# ------------------------------------------------------------------------------------------------------------ float64
def _scatter_rows(idx, rows, n):
    """out[n][K] with out[idx[k]] += rows[k] (float64; sorted by index, summed per run)"""
    out = np.zeros((n, rows.shape[1]))
    if len(idx):
        order = np.argsort(idx, kind="stable")
        si = idx[order]
        first = np.nonzero(np.r_[True, si[1:] != si[:-1]])[0]
        out[si[first]] = np.add.reduceat(rows[order], first, axis=0) + 0.0       # (added INTO zeros: a sum of -0.0 terms is +0, as every
                                                                                 # accumulator that starts at +0 has it)
    return out


def dgrad64(g, pos, W, L):
    """-> (gx [B][Cin][L], sum |term| [B][Cin][L], terms [B][1][L]) of gx[b][:, l] = sum over entries (c, m) -> l of g * W[c]: the dense
    data flow (scatter-add of the entries into the never-built gradient, then W^T times it) with the two steps merged per entry"""
    B, C, M = g.shape
    Cin = W.shape[1]
    g64, W64 = np.asarray(g, np.float64), np.asarray(W, np.float64)
    bb, cc, mm = np.nonzero((pos >= 0) & (pos < L))
    idx = bb.astype(np.int64) * L + pos[bb, cc, mm]
    terms = g64[bb, cc, mm][:, None] * W64[cc]
    shape = lambda a: np.ascontiguousarray(a.reshape(B, L, -1).transpose(0, 2, 1))
    return (shape(_scatter_rows(idx, terms, B * L)), shape(_scatter_rows(idx, np.abs(terms), B * L)),
            shape(_scatter_rows(idx, np.ones((len(idx), 1)), B * L)))


def wgrad64(g_t, pos_t, x64):
    """-> (gW [C][Ci], sum |term|, terms [C][1]) of gW[c][ci] = sum over (b, m) of g * x[b][ci][pos]"""
    B, M, C = g_t.shape
    L = x64.shape[2]
    g64, x64 = np.asarray(g_t, np.float64), np.asarray(x64, np.float64)
    G, A, N = np.zeros((B, C, L)), np.zeros((B, C, L)), np.zeros((C, 1))
    bb, mm, cc = np.nonzero((pos_t >= 0) & (pos_t < L))
    ll = pos_t[bb, mm, cc]
    np.add.at(G, (bb, cc, ll), g64[bb, mm, cc])
    np.add.at(A, (bb, cc, ll), np.abs(g64[bb, mm, cc]))
    np.add.at(N, (cc, 0), 1.0)
    return np.einsum("bcl,bil->ci", G, x64), np.einsum("bcl,bil->ci", A, np.abs(x64)), N


# ------------------------------------------------------------------------------------------------------------ seeded inputs, layouts
def dgrad_case(name, B, C, M, Cin, L, layout):
    """g [B][C][M], pos, W [C][Cin] from the splitmix64 stream of tools/pooled_bits.py under ``name``; ``layout(pos, B, C, M, L)``
    edits the uniformly drawn positions in place (or returns new ones)"""
    g = P.unit(name, 0, (B, C, M))
    W = P.unit(name, 1, (C, Cin)) * np.float32(0.1)
    pos = P.below(name, 2, (B, C, M), L)
    if layout is not None:
        r = layout(pos, B, C, M, L)
        pos = pos if r is None else r
    return g, np.ascontiguousarray(pos, np.int32), W


def tile_count(n, col_of=None):
    """a layout that leaves exactly n entries per cloud in the first tile, the others ignored; entry k (in id order) goes to col_of(k)"""
    def layout(pos, B, C, M, L):
        flat = np.full((B, C * M), -1, np.int32)
        k = np.arange(n)
        flat[:, :n] = (k * 7 % min(L, PD_TL)) if col_of is None else col_of(k)
        return flat.reshape(B, C, M)
    return layout


def int_case(name, B, C, M, Cin, L, pos):
    """integer-exact operands: g in {-4 .. 4} / 8 (never 0), W in {-8 .. 8} / 16: every product is a multiple of 2^-7 (the granule ``INT_GRANULE``) of at most 1/4, so a
    sum is exact in f32, in any order, while sum |term| / 2^-7 < 2^24 (asserted per case through sum |term| by the CPU test)"""
    gi = P.below(name, 10, (B, C, M), 8).astype(np.float32) - 4
    gi[gi >= 0] += 1
    W = (P.below(name, 11, (C, Cin), 17).astype(np.float32) - 8) / np.float32(16)
    return (gi / np.float32(8)).astype(np.float32), np.ascontiguousarray(pos, np.int32), W


def wgrad_case(name, B, C, M, Ci, L):
    return P.wgrad_inputs(name, (B, C, M, Ci, L))


def wgrad_lds(L, rows):
    """the launcher's LDS formula -> bytes"""
    r, sz = (1, 4) if rows == "f32" else (2, 2)
    return ((r * L * sz + 15) & ~15) + (PW_T // 2) * r * 4


def wgrad_max_L(rows):
    L = PW_LDS // 4
    while wgrad_lds(L, rows) > PW_LDS:
        L -= 1
    while wgrad_lds(L + 1, rows) <= PW_LDS:
        L += 1
    return L


# ------------------------------------------------------------------------------------------------------------ the case tables
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def ignored(L):
    return (-1, L, L + 7, INT32_MIN)


def sprinkle(pos, L):
    """a few ignored entries among drawn positions (where the tensor is large enough to spare them)"""
    flat = pos.reshape(pos.shape[0], -1)
    if flat.shape[1] >= 24:
        for k, v in enumerate(ignored(L)):
            flat[:, 3 + 5 * k] = v
    return pos


# the bucket, tile and quarter-range edges: (name, B, C, M, Cin, C1, L); drawn positions, a few of them ignored.  Five buckets (L = 129 .. 160)
# leave the fourth bucket workgroup without a bucket; odd L takes the scalar bf16 store, even L the packed one
SHAPES = [("shape_L%d_Cin%d_C1%d_B%d_M%d" % (L, Cin, C1, B, M), B, C, M, Cin, C1, L) for L, (Cin, C1), B, (C, M) in zip(
    (1, 2, 31, 32, 33, 127, 128, 129, 160, 161, 255, 257),
    ((1, 1), (3, 1), (27, 26), (4, 4), (8, 3), (28, 10), (40, 39), (44, 44), (84, 1), (4, 1), (27, 27), (84, 83)),
    (1, 3) * 6,
    ((6, 64), (150, 1), (40, 5)) * 4)]


def _monotone(span=None):
    """col_of for tile_count, non-decreasing in k, so that the sorted order is the id order: seven entries per column, (k + 3) // 7; with
    ``span`` = (first, last + 1, column) those entries sit on that column, the ones before on the columns below it, the ones after above"""
    def col_of(k):
        if span is None:
            return (k + 3) // 7
        a, b, c = span
        return np.where(k < a, k * (c - 1) // a, np.where(k < b, c, c + 1 + (k - b) // 7))
    return col_of


def _piled(n):
    return lambda k: (k * 7) % max(1, min(50, n // 3 + 1))         # (seven or eight entries per column: chunks of 24 cut them)


def _only(cols_of_draw):
    def layout(pos, B, C, M, L):
        return cols_of_draw(pos, L).astype(np.int32)
    return layout


def _bucket0(n, others):
    """the first n entries (id order) in bucket 0 over several columns, the rest on ``others(k)``"""
    def layout(pos, B, C, M, L):
        k = np.arange(C * M)
        flat = np.where(k < n, (k * 5) % PD_SB, others(k, L)).astype(np.int32)
        return np.broadcast_to(flat, (B, C * M)).reshape(B, C, M).copy()
    return layout


# the lists: name -> (B, C, M, Cin, C1, L, layout, the breaks that turn the case red).  Cin = 8 with C1 = 3: a channel quad that straddles
# the two panels; Cin = 3: the one-channel kernel, whose chains do not depend on where a list is cut -- its cases name the breaks that
# change WHICH entries a column gets
LISTS = {
    "all_ignored": (2, 13, 64, 8, 3, 257, _only(lambda p, L: np.array(ignored(L), np.int64)[p % 4]), ()),
    "first_bucket": (1, 13, 64, 8, 3, 255, _only(lambda p, L: p % 32), ("sort_by_id",)),
    "last_bucket": (1, 13, 64, 8, 3, 255, _only(lambda p, L: 224 + p % 31), ("sort_by_id", "drop_last_bucket")),
    "last_column": (1, 13, 64, 8, 3, 257, _only(lambda p, L: p * 0 + L - 1), ("head_reverse", "drop_last_bucket")),
    "tile_1": (1, 13, 64, 8, 3, 257, tile_count(1, _piled(1)), ()),
    "tile_15": (1, 13, 64, 8, 3, 257, tile_count(15, _piled(15)), ("head_reverse",)),
    "tile_16": (1, 13, 64, 8, 3, 257, tile_count(16, _piled(16)), ("head_reverse",)),
    "tile_17": (1, 13, 64, 8, 3, 257, tile_count(17, _piled(17)), ("rem_last",)),
    "tile_383": (1, 13, 64, 8, 3, 257, tile_count(383, _piled(383)), ("rem_last", "sort_by_id")),
    "tile_384": (1, 13, 64, 8, 3, 257, tile_count(384, _piled(384)), ("sort_by_id",)),
    "tile_385": (1, 13, 64, 8, 3, 257, tile_count(385, _piled(385)), ("sort_by_id",)),
    "tile_769": (1, 13, 64, 8, 3, 257, tile_count(769, _piled(769)), ("sort_by_id",)),
    # 384 entries, chunks of 24: column 20 holds entries 10 .. 109 -- the end of chunk 0, chunks 1, 2, 3 whole, the start of chunk 4
    "three_whole_chunks": (1, 13, 64, 8, 3, 257, tile_count(384, _monotone((10, 110, 20))), ("head_reverse",)),
    # 383 entries: fifteen chunks of 24, one of 23.  Column 40 holds entries 130 .. 167: it begins inside chunk 5 and ends with the last
    # entry of chunk 6
    "run_ends_on_chunk_edge": (1, 13, 64, 8, 3, 257, tile_count(383, _monotone((130, 168, 40))), ("rem_last",)),
    # entries 384 and 385 of the tile (indices 383, 384) share a column: it crosses the round edge; the third round's seven chunks of one
    # entry continue one column
    "round_edge": (1, 13, 64, 8, 3, 257, tile_count(775, _monotone()), ("head_reverse",)),
    "cap_2047": (1, 33, 64, 4, 1, 70, _bucket0(2047, lambda k, L: 40 + k % 20), ("sort_by_id",)),
    "cap_2048": (1, 33, 64, 4, 1, 70, _bucket0(2048, lambda k, L: 40 + k % 20), ("sort_by_id",)),
    "cap_2049": (1, 33, 64, 4, 1, 70, _bucket0(2049, lambda k, L: 40 + k % 20), ("sort_by_id",)),
    # the one-channel kernel: a group (bucket) of 127 / 128 / 129 entries; entries 128 and 129 share a column, resumed in the second round
    "group_127": (2, 13, 64, 3, 1, 32, tile_count(127, _monotone()), ("drop_last_bucket",)),
    "group_128": (2, 13, 64, 3, 1, 32, tile_count(128, _monotone()), ("drop_last_bucket",)),
    "group_129": (2, 13, 64, 3, 2, 32, tile_count(129, _monotone()), ("drop_last_bucket",)),
    # entries ON column L, which a kernel that accepts pos == L would count: the last tile's rounds are cut elsewhere
    "pos_is_L": (1, 13, 64, 8, 3, 130, _only(lambda p, L: np.where(p % 3 == 0, L, 128 + p % 2)), ("pos_eq_L",)),
}


def dgrad_named(name):
    """-> (g, pos, W, C1, L) of a case of SHAPES or LISTS"""
    for n, B, C, M, Cin, C1, L in SHAPES:
        if n == name:
            g, pos, W = dgrad_case(name, B, C, M, Cin, L, lambda p, *_: sprinkle(p, L))
            return g, pos, W, C1, L
    B, C, M, Cin, C1, L, layout, _ = LISTS[name]
    g, pos, W = dgrad_case(name, B, C, M, Cin, L, layout)
    return g, pos, W, C1, L


def quarter_edges(L):
    """the first and the last column of the first and the last bucket of every quarter of the bucket kernel's range, and the quarter sizes"""
    nbucket = -(-L // PD_SB)
    nbq = -(-nbucket // PB_Q)
    cols, sizes = [], []
    for q in range(PB_Q):
        t0, t1 = q * nbq, min(nbucket, (q + 1) * nbq)
        sizes.append(max(0, t1 - t0))
        for t in (t0, t1 - 1):
            if t0 < t1:
                cols += [t * PD_SB, min(L, (t + 1) * PD_SB) - 1]
    return np.array(cols, np.int64), sizes


# large and wide, integer-exact: (name, C, M, L)
LARGE = [("large_L131072", 16, 8, 131072), ("large_L131073", 16, 8, 131073), ("large_L262112", 16, 8, L_MAX), ("wide_ids", 16383, 64, 4096),
         ("most_ids", 1023, 1025, 4096)]                       # C * M = 2^20 - 1, the most the launchers admit: ids up to 2^20 - 2


def large_case(name):
    """-> (g, pos, W, C1, L): B = 1, Cin = 4 (the entry-balanced kernel).  The three large L: 128 entries, on the first and last columns of the
    first and last bucket of every quarter, twice over (two entries per such column), the others drawn.  wide_ids, most_ids: every id up to C * M - 1
    in use, 256 entries per column -- the channel of an entry is id / M"""
    C, M, L = [c for c in LARGE if c[0] == name][0][1:]
    pos = P.below(name, 2, (1, C, M), L)
    if name.startswith("large"):
        edges, _ = quarter_edges(L)
        flat = pos.reshape(-1)
        flat[: 2 * len(edges)] = np.r_[edges, edges]
    g, pos, W = int_case(name, 1, C, M, 4, L, pos)
    return g, pos, W, 3, L


# the matrix cores: (name, B, C, M, Cin, C1, L).  Cin -> NMT = ceil(Cin / 32) / 2 = 1 .. 6 (40, 100: rows beyond Cin in the last 32-row tile),
# C -> KC = C / 16 = 1, 2, 3, 4, 5, 7, 24; L: the 16-byte store (L % 8 == 0), the dword tail, a last piece partly past L.  B = 2: 64-column
# workgroups; B * ceil(L / 128) >= 2048: 128-column workgroups
MFMA = [("mfma_Cin%d_C%d_L%d_B%d" % (Cin, C, L, B), B, C, M, Cin, C1, L) for B, C, M, Cin, C1, L in (
    (2, 16, 2, 40, 10, 2), (2, 32, 3, 64, 64, 6), (2, 48, 4, 100, 10, 8), (2, 64, 4, 128, 64, 62), (2, 80, 4, 192, 191, 64),
    (2, 112, 4, 256, 1, 66), (2, 384, 4, 320, 64, 130), (2, 16, 4, 384, 10, 136),
    (2048, 16, 2, 40, 10, 6), (2048, 16, 2, 64, 64, 8), (1024, 80, 2, 40, 10, 130), (1024, 32, 2, 100, 100, 136))]
MFMA_EDGE_COLS = (31, 32, 63, 64, 127, 128)


def mfma_shape(B, C, Cin, L):
    """-> (NMT, KC, CH) the launcher picks"""
    return -(-Cin // 32) // 2, C // 16, 2 if B * -(-L // (2 * PM_TL)) >= PM_BIG else 1


def mfma_case(name, exact):
    """-> (g, pos, W, C1, L).  exact: g = k / 8, W = j / 16 (bf16 numbers), positions drawn, (channel, column) pairs two to four times over
    where M allows -- every sum in the G image is k / 8 with |k| <= 4 M < 256, a bf16 number, so the order of the adds does not show.
    Continuous: the positions of a (cloud, channel) row are distinct columns (M <= L), operands rounded to bf16 by the kernel."""
    B, C, M, Cin, C1, L = [c for c in MFMA if c[0] == name][0][1:]
    if exact:
        pos = P.below(name, 2, (B, C, M), L)
        pos[:, ::2, 1:] = pos[:, ::2, :1]                       # every other channel: all its entries on one column (M of them)
        if M >= 3:
            pos[:, 1::4, 1] = pos[:, 1::4, 0]                   # ... and a pair twice
        g, pos, W = int_case(name, B, C, M, Cin, L, pos)
    else:
        g = P.unit(name, 0, (B, C, M))
        W = P.unit(name, 1, (C, Cin)) * np.float32(0.1)
        step = L // M
        pos = (np.arange(M, dtype=np.int32).reshape(1, 1, M) * step + P.below(name, 2, (B, C, M), step)).astype(np.int32)
    if L >= 130:
        edge = np.array(MFMA_EDGE_COLS, np.int32)
        if not exact:
            pos[0, :6, 1:] = -1                                 # (their other entries leave: the pairs stay distinct)
        pos[0, :6, 0] = edge
    pos[0, 6, 0] = -1
    pos[0, 7, 1] = L + 3
    pos[B - 1] = -1                                             # a cloud with no entry
    return g, np.ascontiguousarray(pos, np.int32), W, C1, L


# the weight gradient: (name, B, C, M, Ci, L)
WGRAD = [("wgrad_M%d_C%d_Ci%d_L%d" % (M, C, Ci, L), B, C, M, Ci, L) for B, C, M, Ci, L in (
    (1, 1, 1, 1, 1), (3, 5, 31, 15, 3), (3, 383, 32, 16, 4), (1, 384, 33, 17, 7), (3, 5, 63, 33, 8), (3, 40, 64, 2, 9), (2, 384, 64, 33, 8))]
WGRAD_RUNS = [("f32", None), ("bf16", None), ("f32", 0), ("f32", 1), ("bf16", 0), ("bf16", 1)]


def wgrad_named(name, shape=None):
    """-> (g_t [B][M][C], pos_t, x [B][Ci][L] f32, scale, shift): all M entries of channel 0 on one column, row m = 3 piled on column 0,
    ignored entries -1 / L / INT32_MIN / INT32_MAX; the first two coefficient pairs are (1, -0.0) and (1 + 2^-8, -0.0) and the first columns of
    rows 0 and 1 hold +0, -0.0, +-2^-149 and 1, 2, -1, -0.5: pre-activations at the ReLU's edge and, in row 1, bf16 results on a rounding tie
    (v (1 + 2^-8) for a power of two v lies halfway between two bf16 numbers)"""
    B, C, M, Ci, L = shape or [c for c in WGRAD if c[0] == name][0][1:]
    g = P.unit(name, 0, (B, M, C))
    x = P.unit(name, 1, (B, Ci, L))
    pos = P.below(name, 2, (B, M, C), L)
    if M > 3 and C > 1:
        pos[:, 3, :] = 0
    pos[:, :, 0] = L // 2
    if M * C >= 16 and C > 1:
        for k, v in enumerate((-1, L, INT32_MIN, INT32_MAX)):
            pos[k % B, (5 * k + 1) % M, 1 + (3 * k) % (C - 1)] = v
    scale = np.float32(1.0) + np.float32(0.5) * P.unit(name, 4, (Ci,))
    shift = np.float32(0.3) * P.unit(name, 5, (Ci,))
    edge = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1.0, 2.0, -1.0, -0.5], np.float32)
    for r in range(min(Ci, 2)):
        scale[r], shift[r] = (1.0, -0.0) if r == 0 else (1.0 + 2.0 ** -8, -0.0)      # (a shift of +0 would turn a product of -0.0 into +0)
        x[:, r, : min(L, 8)] = edge[: min(L, 8)]
    return g, np.ascontiguousarray(pos, np.int32), x, scale, shift
