"""Numpy restatement of the weight packs (csrc/pointmlp.hip, pointmlp_bf16.hip, pointmlp_x3.hip, pointmlp_h3p.hip) and of the table
``sonet_pack_multi`` reads (include/sonet_hip.h).  Plain numpy, no torch, nothing from sonet_hip: tests/test_pack_cpu.py holds this file to
itself and to the library's size functions, tests/test_gpu_packs.py and tests/test_gpu_pack_registry.py hold the kernels to this file, byte
for byte.

Every layout is written from the comment in front of its kernel, as a reshape / transpose of the zero-padded matrix:

  f32   Wp[ct][g][lane][s]          (f32)        = W[32 ct + (lane & 31)][8 g + 2 s + (lane >> 5)]
  bf16  Wp[ct][kc][lane][t]         (8 bf16)     = W[32 ct + (lane & 31)][16 kc + 8 (lane >> 5) + t]
  x3    Wp[ct][kc][term][lane][t]   (8 bf16)       the same element; term = h, m, l of the three-way bf16 split
  h3    Wp[ct][kcp][term][lane][t]  (8 fp16)       the same element; term 0 = fp16(w), term 1 = fp16(32 (w - term 0)); kcp runs to KC rounded
                                                   up to a multiple of 8 with zero chunks
  h3p   Wp[ct][kcp][form][lane][e]  (8 fp16)     = W[32 ct + (lane & 31)][16 kcp + 4 (lane >> 5) + (e & 3) + 8 (e >> 2)]; form 0 = fp16(32 w),
                                                   form 1 = fp16(32 w - form 0); an even number of 32-row tiles
and x3 / h3 / h3p end in a 64-byte trailer: word 0 = the bits of max |w| over the elements that exist, ordered as unsigned integers (a NaN of
either sign above inf above every finite value), words 1..15 zero.

A matrix is given either as a 2-D array (rows = Cout = shape[0]) or, as the ``_strided`` entry points take it, as a flat buffer with
``rows``, ``rs``, ``cs`` and the padded ``Cout``: element (o, c) = buf[o rs + c cs] for o < rows, c < Cin, zero elsewhere.

Every function returns the bytes the kernel WRITES: data and trailer.  A buffer of ``pack_size`` bytes can be longer (the x3 / h3 size is the
larger of the two flavours'); what lies behind the trailer is nobody's.

f32 subnormals: ``flush=False`` keeps them through every conversion and subtraction, ``flush=True`` reads every f32 / bf16 value below 2^-126
as a zero of its sign (tests/x3_model.py carries the same pair).  The f32 pack copies bits and the trailer is an integer maximum of bits:
neither depends on the model.

"Breaks" are keyword parameters: the same restatement with one deliberate mistake, used by the CPU test to show that the seeded weights tell
the mistake from the contract."""
import numpy as np

from x3_model import BF16_OVERFLOW_BITS, _flush, bf16, split3

H3_KPAD = 8
FLAVOURS = ("bf16", "x3", "h3")                                  # the table's flavour numbers 0, 1, 2
BREAKS = ("swap_halves", "term_order", "kc_for_kcp", "rows_is_cout", "trailer_padded")


def _cdiv(a, b):
    return -(-a // b)


def chunks(flavour, Cin):
    """K chunks of 16 channels in a pack: the fp16 flavours pad to a multiple of 8 chunks."""
    kc = _cdiv(Cin, 16)
    return _cdiv(kc, H3_KPAD) * H3_KPAD if flavour in ("h3", "h3p") else kc


def tiles(flavour, Cout):
    return _cdiv(Cout, 64) * 2 if flavour == "h3p" else _cdiv(Cout, 32)


def written_size(flavour, Cin, Cout):
    """Bytes a pack kernel writes (data + trailer)."""
    if flavour == "f32":
        return tiles(flavour, Cout) * _cdiv(Cin, 8) * 256 * 4
    per_chunk = {"bf16": 1024, "x3": 3072, "h3": 2048, "h3p": 2048}[flavour]
    return tiles(flavour, Cout) * chunks(flavour, Cin) * per_chunk + (0 if flavour == "bf16" else 64)


def pack_size(flavour, Cin, Cout):
    """Bytes of the buffer a caller allocates: x3 and h3 share one size, the larger of the two."""
    if flavour in ("x3", "h3"):
        return max(written_size("x3", Cin, Cout), written_size("h3", Cin, Cout))
    return written_size(flavour, Cin, Cout)


# ---- the matrix a pack sees ----------------------------------------------------------------------------------------------------------
def _as_spec(W, Cin, Cout, rows, rs, cs):
    W = np.ascontiguousarray(W, dtype=np.float32)
    if W.ndim == 2 and rs is None:
        n_rows, Cin_ = W.shape
        return W.reshape(-1), Cin_, (n_rows if Cout is None else Cout), n_rows, Cin_, 1
    assert None not in (Cin, Cout, rows, rs, cs), "a strided matrix needs Cin, Cout, rows, rs and cs"
    return W.reshape(-1), int(Cin), int(Cout), int(rows), int(rs), int(cs)


def padded(W, Cin=None, Cout=None, rows=None, rs=None, cs=None, pad_rows=32, pad_cols=16, rows_is_cout=False):
    """-> (P [pad_rows-multiple][pad_cols-multiple] f32, exists bool of the same shape): the matrix with +0.0 wherever no element exists.
    Break ``rows_is_cout``: every row up to the padded Cout is read from the buffer."""
    buf, Cin, Cout, rows, rs, cs = _as_spec(W, Cin, Cout, rows, rs, cs)
    assert 0 < rows <= Cout and Cin > 0
    R, C = _cdiv(Cout, pad_rows) * pad_rows, _cdiv(Cin, pad_cols) * pad_cols
    take = Cout if rows_is_cout else rows
    P = np.zeros((R, C), dtype=np.float32)
    exists = np.zeros((R, C), dtype=bool)
    o, c = np.meshgrid(np.arange(take), np.arange(Cin), indexing="ij")
    at = o * rs + c * cs
    P[:take, :Cin] = buf[at % buf.size] if rows_is_cout else buf[at]
    exists[:take, :Cin] = True
    return P, exists


def amax_bits(P, exists):
    """The bits of max |w| over the elements that exist: NaN above inf above finite, in either sign; 0 for an empty or all-zero set."""
    mag = P.view(np.uint32)[exists] & np.uint32(0x7FFFFFFF)
    return int(mag.max()) if mag.size else 0


def trailer(P, exists):
    t = np.zeros(16, dtype="<u4")
    t[0] = amax_bits(P, exists)
    return t.view(np.uint8)


# ---- the conversions -----------------------------------------------------------------------------------------------------------------
def _hi16(v):
    """bf16 values held as f32 -> their 16 bits."""
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) >> 16).astype("<u2")


def split3_w(v, flush=False):
    """The WEIGHT side of the three-way bf16 split -> (h, m, l) as uint16 bf16 bits.  tests/x3_model.py::split3, then the weight-side fix: a
    value whose high piece rounds to infinity is split again from the largest finite bf16 of its sign (0x7F7F), whose residual fits m and l
    exactly; a true infinity goes to the l piece alone, h = m = +0."""
    v = np.array(v, dtype=np.float32)
    if flush:
        v = _flush(v)
    h, m, l = (_hi16(p) for p in split3(v, flush))
    over = (h & 0x7FFF) == 0x7F80
    inf = over & np.isinf(v)
    fin = over & ~inf
    l = np.where(inf, h, l)
    m = np.where(inf, 0, m)
    h = np.where(inf, 0, h)
    if fin.any():
        h = np.where(fin, h - 1, h).astype("<u2")
        hf = (h.astype(np.uint32) << 16).view(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            r = (v - hf).astype(np.float32)
            mf = bf16(np.where(fin, r, 0), flush)
            lf = bf16(np.where(fin, r - mf, 0), flush)
        m = np.where(fin, _hi16(mf), m)
        l = np.where(fin, _hi16(lf), l)
    return h.astype("<u2"), m.astype("<u2"), l.astype("<u2")


def _f16_bits(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, dtype=np.float32).astype(np.float16).view(np.uint16).astype("<u2")   # (numpy rounds to nearest even)


def _clamp(v, lim):
    """Clamp to +-lim; a NaN stays a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(v > lim, np.float32(lim), np.where(v < -lim, np.float32(-lim), v)).astype(np.float32)


def split_h3(v, flush=False):
    """-> (fp16(clamp(w, +-65504)), fp16(32 (w_clamped - h))) as uint16 fp16 bits; the residual is formed in f32."""
    v = np.array(v, dtype=np.float32)
    if flush:
        v = _flush(v)
    w = _clamp(v, 65504.0)
    h = _f16_bits(w)
    with np.errstate(invalid="ignore"):
        res = (np.float32(32.0) * (w - h.view(np.float16).astype(np.float32))).astype(np.float32)
    return h, _f16_bits(res)


def split_h3p(v, flush=False):
    """-> (fp16(32 clamp(w, +-2047)), fp16(32 w_clamped - form 0))."""
    v = np.array(v, dtype=np.float32)
    if flush:
        v = _flush(v)
    w = (np.float32(32.0) * _clamp(v, 2047.0)).astype(np.float32)
    h = _f16_bits(w)
    with np.errstate(invalid="ignore"):
        res = (w - h.view(np.float16).astype(np.float32)).astype(np.float32)
    return h, _f16_bits(res)


# ---- the layouts ---------------------------------------------------------------------------------------------------------------------
def _lanes16(piece, swap_halves=False):
    """[32 CT][16 KC] 16-bit pieces -> [CT][KC][lane][8]: lane = 32 (which half of the chunk's 16 channels) + (row inside the tile)."""
    R, C = piece.shape
    a = piece.reshape(R // 32, 32, C // 16, 2, 8).transpose(0, 2, 3, 1, 4)             # tile, chunk, half, row, element
    if swap_halves:
        a = a[:, :, ::-1]
    return a.reshape(R // 32, C // 16, 64, 8)


def _lanes16_p16(piece, swap_halves=False):
    """The same with the chunk's channels in P16 order: element e of half h is channel 4 h + (e & 3) + 8 (e >> 2)."""
    R, C = piece.shape
    a = piece.reshape(R // 32, 32, C // 16, 2, 2, 4).transpose(0, 2, 4, 1, 3, 5)       # tile, chunk, half, row, e >> 2, e & 3
    if swap_halves:
        a = a[:, :, ::-1]
    return a.reshape(R // 32, C // 16, 64, 8)


def _terms(pieces, lanes, swap_halves, term_order):
    """pieces: T arrays [32 CT][16 KC] -> bytes of [CT][KC][term][lane][8]."""
    t = [lanes(p, swap_halves) for p in pieces]
    if term_order:
        t = t[::-1]
    return np.ascontiguousarray(np.stack(t, axis=2)).astype("<u2").reshape(-1).view(np.uint8)


def pack_f32(W, Cin=None, Cout=None, rows=None, rs=None, cs=None, swap_halves=False, rows_is_cout=False, **_):
    P, _e = padded(W, Cin, Cout, rows, rs, cs, 32, 8, rows_is_cout)
    R, C = P.shape
    a = P.reshape(R // 32, 32, C // 8, 4, 2).transpose(0, 2, 4, 1, 3)                  # tile, group, half (k parity), row, s
    if swap_halves:
        a = a[:, :, ::-1]
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def pack_bf16(W, Cin=None, Cout=None, rows=None, rs=None, cs=None, flush=False, swap_halves=False, rows_is_cout=False, **_):
    P, _e = padded(W, Cin, Cout, rows, rs, cs, 32, 16, rows_is_cout)
    return _terms([_hi16(bf16(P, flush))], _lanes16, swap_halves, False)


def pack_x3(W, Cin=None, Cout=None, rows=None, rs=None, cs=None, flush=False, swap_halves=False, term_order=False, rows_is_cout=False,
            trailer_padded=False, **_):
    P, ex = padded(W, Cin, Cout, rows, rs, cs, 32, 16, rows_is_cout)
    if trailer_padded:
        ex = padded(W, Cin, Cout, rows, rs, cs, 32, 16, True)
        return np.concatenate([_terms(split3_w(P, flush), _lanes16, swap_halves, term_order), trailer(*ex)])
    return np.concatenate([_terms(split3_w(P, flush), _lanes16, swap_halves, term_order), trailer(P, ex)])


def _pad_chunks(P, ex, kc_for_kcp):
    kcp = P.shape[1] // 16 if kc_for_kcp else _cdiv(P.shape[1] // 16, H3_KPAD) * H3_KPAD
    add = kcp * 16 - P.shape[1]
    return np.pad(P, ((0, 0), (0, add))), np.pad(ex, ((0, 0), (0, add)))


def pack_h3(W, Cin=None, Cout=None, rows=None, rs=None, cs=None, flush=False, swap_halves=False, term_order=False, kc_for_kcp=False,
            rows_is_cout=False, trailer_padded=False, **_):
    P, ex = padded(W, Cin, Cout, rows, rs, cs, 32, 16, rows_is_cout)
    tr = trailer(*padded(W, Cin, Cout, rows, rs, cs, 32, 16, True)) if trailer_padded else trailer(P, ex)
    P, ex = _pad_chunks(P, ex, kc_for_kcp)
    return np.concatenate([_terms(split_h3(P, flush), _lanes16, swap_halves, term_order), tr])


def pack_h3p(W, Cin=None, Cout=None, rows=None, rs=None, cs=None, flush=False, swap_halves=False, term_order=False, kc_for_kcp=False,
             rows_is_cout=False, **_):
    P, ex = padded(W, Cin, Cout, rows, rs, cs, 64, 16, rows_is_cout)
    tr = trailer(P, ex)
    P, ex = _pad_chunks(P, ex, kc_for_kcp)
    return np.concatenate([_terms(split_h3p(P, flush), _lanes16_p16, swap_halves, term_order), tr])


PACKS = {"f32": pack_f32, "bf16": pack_bf16, "x3": pack_x3, "h3": pack_h3, "h3p": pack_h3p}


# ---- the inverse, written on its own: one 16-bit piece at a time from its documented position ------------------------------------------
def unpack16(data, flavour, Cin, Cout):
    """bytes of a bf16 / x3 / h3 / h3p pack -> uint16 [terms][32 CT][16 KC(P)]: the piece of row o, channel c, term s is read from position
    (tile, chunk, term, lane, element) of the documented layout."""
    T = {"bf16": 1, "x3": 3, "h3": 2, "h3p": 2}[flavour]
    CT, KC = tiles(flavour, Cout), chunks(flavour, Cin)
    u = np.frombuffer(np.ascontiguousarray(data, dtype=np.uint8)[:CT * KC * T * 1024].tobytes(), dtype="<u2")
    out = np.zeros((T, CT * 32, KC * 16), dtype=np.uint16)
    for o in range(CT * 32):
        for c in range(KC * 16):
            ct, kc, k = o // 32, c // 16, c % 16
            if flavour == "h3p":
                half, e = (k >> 2) & 1, (k & 3) + 4 * (k >> 3)
            else:
                half, e = k >> 3, k & 7
            lane = 32 * half + o % 32
            for s in range(T):
                out[s, o, c] = u[((((ct * KC + kc) * T + s) * 64) + lane) * 8 + e]
    return out


def bf16_value(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def f16_value(bits):
    return np.asarray(bits).astype(np.uint16).view(np.float16).astype(np.float32)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
ENTRY = np.dtype([("W", "<u8"), ("Wp", "<u8"), ("rs", "<i8"), ("cs", "<i8"), ("total", "<i8"), ("Cin", "<i4"), ("rows", "<i4"), ("KC", "<i4"),
                  ("flavour", "<i4"), ("blk0", "<i4"), ("nblk", "<i4"), ("pad", "<i8")])
assert ENTRY.itemsize == 72


def pack_table(entries):
    """entries: dicts with src, dst (addresses), rs, cs, Cin, rows, Cout, flavour (a name of FLAVOURS) -> (the 72-byte records as uint8,
    total_blocks): total = 64 work items per (tile, chunk), 256 per workgroup, workgroup ranges back to back in the order given."""
    rec = np.zeros(len(entries), dtype=ENTRY)
    blk = 0
    for i, e in enumerate(entries):
        kc = chunks(e["flavour"], e["Cin"])
        total = 64 * tiles(e["flavour"], e["Cout"]) * kc
        nblk = _cdiv(total, 256)
        rec[i] = (e["src"], e["dst"], e["rs"], e["cs"], total, e["Cin"], e["rows"], kc, FLAVOURS.index(e["flavour"]), blk, nblk, 0)
        blk += nblk
    return rec.view(np.uint8).reshape(-1).copy(), blk


# ---- seeded weights ------------------------------------------------------------------------------------------------------------------
def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _both_signs(bits):
    return [b for x in bits for b in (x, x | 0x80000000)]


FLT_MAX_BITS, FLT_MIN_BITS = 0x7F7FFFFF, 0x00800000
B65504 = 0x477FE000
EDGE_FINITE_BITS = _both_signs([
    0x00000000,                                                  # +-0
    FLT_MAX_BITS, FLT_MIN_BITS,                                  # largest and smallest normal
    0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001,              # bf16 ties (to even: down, up) and their neighbours
    0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001,              # fp16 ties and their neighbours
    0x3F808080, 0x3F818180,                                      # a tie in the second bf16 piece
    BF16_OVERFLOW_BITS - 1, BF16_OVERFLOW_BITS, BF16_OVERFLOW_BITS + 1,
    B65504 - 1, B65504, B65504 + 1, 0x47C35000,                  # 65504, its neighbours, 1e5
    0x44FFE000 - 1, 0x44FFE000, 0x44FFE000 + 1, 0x45000000,      # 2047 (the h3p clamp), its neighbours, 2048
    0x477FF000, 0x477FEFFF,                                      # 65520: the fp16 tie between 65504 and infinity, and the value below
])
INF_BITS = [0x7F800000, 0xFF800000]
NAN_BITS = [0x7FC01234]
SUBNORMAL_BITS = _both_signs([0x00000001, 0x00000100, 0x00008000, 0x00010000, 0x00400000, 0x007F8000, 0x007FFFFF, 0x00012345])
WEIGHT_SETS = ("ordinary", "edge", "edge_inf", "edge_nan", "subnormal")


def weights(kind, Cout, Cin, seed=0):
    """Seeded [Cout][Cin] f32 weights.  "ordinary": N(0, 2 / Cin).  The other sets put their special values (each at least once when the
    matrix has room, in seeded places; cyclically otherwise) into an ordinary matrix: "edge" the finite edge values, "edge_inf" those and
    +-inf, "edge_nan" those and one NaN, "subnormal" f32 subnormals of both signs."""
    rng = np.random.default_rng([seed, Cout, Cin, WEIGHT_SETS.index(kind)])
    W = (rng.standard_normal((Cout, Cin)) * (2.0 / Cin) ** 0.5).astype(np.float32)
    if kind == "ordinary":
        return W
    special = {"edge": EDGE_FINITE_BITS, "edge_inf": EDGE_FINITE_BITS + INF_BITS, "edge_nan": EDGE_FINITE_BITS,
               "subnormal": SUBNORMAL_BITS}[kind]
    flat = W.reshape(-1)
    places = rng.permutation(flat.size)[:min(flat.size, 2 * len(special))]
    start = int(rng.integers(len(special)))
    flat[places] = _f([special[(start + i) % len(special)] for i in range(places.size)])
    if kind == "edge_nan":
        flat[int(rng.integers(flat.size))] = _f(NAN_BITS[0])
    return W


def nan_lane_mask(flavour, W, Cin=None, Cout=None, rows=None, rs=None, cs=None):
    """Bytes of the written pack that hold a piece of a NaN weight, or the trailer's word 0 when a NaN exists: a NaN's payload is nobody's
    contract, so these bytes leave the byte comparison (the caller checks that they decode to NaN)."""
    P, ex = padded(W, Cin, Cout, rows, rs, cs, 64 if flavour == "h3p" else 32, 8 if flavour == "f32" else 16)
    nan = np.isnan(P)
    if flavour == "f32":
        return np.zeros(P.size * 4, dtype=bool)                  # (a copy keeps the payload)
    if flavour in ("h3", "h3p"):
        nan, _ = _pad_chunks(nan, ex, False)
    lanes = _lanes16_p16 if flavour == "h3p" else _lanes16
    T = {"bf16": 1, "x3": 3, "h3": 2, "h3p": 2}[flavour]
    m = np.repeat(np.stack([lanes(nan)] * T, axis=2).reshape(-1), 2)
    if flavour != "bf16":
        tr = np.zeros(64, dtype=bool)
        tr[:4] = nan.any()
        m = np.concatenate([m, tr])
    return m
