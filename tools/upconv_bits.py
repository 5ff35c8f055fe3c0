#!/usr/bin/env python
"""tools/upconv_bits.py [--out FILE] | --check -- the bits of the decoder's up-convolution kernels (so-net_amd/csrc/upconv.hip,
upconv_bwd.hip, upconv_wgrad.hip) on fixed inputs that round.

Every case of ``CASES`` runs through ``sonet_hip.ops`` (``upconv3x3_pack`` + ``upconv3x3`` with ReLU on and off under a mixed-sign scale;
``upconv3x3_dgrad_pack`` + ``upconv3x3_dgrad``; ``upconv3x3_wgrad``) and every output tensor's bytes -- the packs count as outputs, the
forward's trailer included -- are hashed with sha256.  Run on an MI355X this writes case name -> list of digests (default
tests/golden/upconv_bits.json); tests/test_gpu_upconv_bits.py walks the same table and holds the tree to that file.  The file is a recording
of the kernels' outputs: it is regenerated only when a change is MEANT to change the family's arithmetic, from the parent of that change.

Inputs are the continuous splitmix values of tools/pooled_bits.py (its ``u64`` / ``unit`` / ``below``; weights times 0.1), so that
products and sums round: the integer cases of tests/test_gpu_upconv*.py are exact by construction and a reordered chain passes them.

``--check`` (no GPU; tests/test_upconv_bits_cpu.py) holds the table to what it says: the names are unique, every case reaches what its row
claims (``REACHES``: computed from the extents ``sonet_hip.ops`` exports and ``tests/upconv_wgrad_ref.plan``), and the inputs are
order-sensitive -- the f32 sum of a case's per-chunk partial products in the kernel's order differs from the sum in reversed order in at
least one output element (every case has three chunks or more for that: two f32 numbers add to the same bits either way round); the
same figure product by product is printed beside it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "so-net_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from pooled_bits import DEV, below, digest, unit  # noqa: E402,F401  (u64 through unit / below: one copy of the inputs' arithmetic)

FIXTURE = os.path.join(ROOT, "tests", "golden", "upconv_bits.json")

# ---------------------------------------------------------------------------------------------------------------- the case table
# (name, (B, Cin, Cout, H, W)): the smallest shapes at which each kernel can still go wrong AND its chain has three chunks or more (two f32
# partial sums add to the same bits in either order, so a shorter chain cannot show a reordering); what a case reaches is in REACHES below.
# forward: each case gives the pack, y with ReLU on and y with ReLU off, both under a scale of mixed sign
FWD = [
    ("fwd_1x1", (3, 33, 32, 1, 1)),             # twelve of sixteen pairs skipped; a K tail of one channel
    ("fwd_seams", (3, 40, 64, 3, 5)),           # cloud seams inside one tile; three chunks with a tail; two row blocks
    ("fwd_two_tiles", (3, 48, 32, 8, 8)),       # 192 columns: a full tile and one with two idle waves
    ("fwd_w64", (2, 40, 32, 2, 64)),            # the widest halo: every staged slot, all three staging items per thread
    ("fwd_flush", (1, 272, 32, 2, 2)),          # 17 chunks: one chain flush inside the loop and one at the end
]
# input gradient: the pack and dx
DGRAD = [
    ("dg_1x1", (3, 33, 64, 1, 1)),              # the second row block holds one row
    ("dg_seams", (3, 20, 96, 3, 5)),            # six chunks: crosses the flush length
    ("dg_two_tiles", (3, 40, 64, 8, 8)),        # a full tile and a partial one
    ("dg_w64", (2, 17, 64, 2, 64)),             # the widest halo
]
# weight gradient: dw.  (name, shape, name the inputs are drawn under, byte offset of g and x into a larger buffer)
WGRAD = [
    ("wg_1x1", (35, 17, 32, 1, 1), "wg_1x1", 0),                # four live pairs; 35 columns = 3 steps
    ("wg_scalar", (3, 33, 64, 3, 5), "wg_scalar", 0),           # element-wise loads; two Cin blocks; 45 columns = 3 steps, the last short
    ("wg_vec", (3, 16, 32, 4, 4), "wg_vec", 0),                 # the 16-byte loads
    ("wg_vec_offset", (3, 16, 32, 4, 4), "wg_vec", 8),          # wg_vec's operands 8 bytes into a buffer: W % 4 == 0 but element-wise
    ("wg_two_slices", (9, 16, 32, 8, 8), "wg_two_slices", 0),   # 576 columns: 2 slices of 18 steps, each crossing one 16-step flush
]
CASES = ([(n, ("fwd", n, s)) for n, s in FWD] + [(n, ("dgrad", n, s)) for n, s in DGRAD] + [(n, ("wgrad", n, s, src, off)) for n, s, src, off in WGRAD])
NAMES = [n for n, _ in CASES]
SAME_BITS = [("wg_vec_offset", "wg_vec")]       # pairs of cases whose digests must be equal

# what each case's row claims, as the figures ``reached`` computes from the shape
REACHES = {
    "fwd_1x1": dict(tiles=1, live_pairs=4, chunks=3, k_tail=1),
    "fwd_seams": dict(tiles=1, clouds_in_first_tile=3, chunks=3, k_tail=8, row_blocks=2),
    "fwd_two_tiles": dict(tiles=2, columns=192, idle_waves_last_tile=2),
    "fwd_w64": dict(staged_slots_of_max=(258, 258), staging_items=3),
    "fwd_flush": dict(chunks=17, flushes_inside=1, flushes=2),
    "dg_1x1": dict(row_blocks=2, rows_last_block=1, live_pairs=4),
    "dg_seams": dict(chunks=6, flushes_inside=1, flushes=2, clouds_in_first_tile=3),
    "dg_two_tiles": dict(tiles=2, idle_waves_last_tile=2, row_blocks=2),
    "dg_w64": dict(staged_slots_of_max=(258, 258), staging_items=3),
    "wg_1x1": dict(live_pairs=4, steps=3),
    "wg_scalar": dict(vec=False, row_blocks=2, steps=3, columns_last_step=13),
    "wg_vec": dict(vec=True, steps=3),
    "wg_vec_offset": dict(vec=False, w_mod_4=0),
    "wg_two_slices": dict(columns=576, slices=2, steps_per_slice=18, flushes_inside_slice=1),
}


# ---------------------------------------------------------------------------------------------------------------- the inputs
def weights(name, Cin, Cout):
    return unit(name, 1, (Cout, Cin, 3, 3)) * np.float32(0.1)


def fwd_inputs(name, shape):
    B, Cin, Cout, H, W = shape
    sign = np.where(below(name, 4, (Cout,), 4) == 0, np.float32(-1.0), np.float32(1.0))
    scale = (np.float32(1.0) + np.float32(0.5) * unit(name, 2, (Cout,))) * sign
    assert (scale < 0).any() and (scale > 0).any(), name
    return unit(name, 0, (B, Cin, H, W)), weights(name, Cin, Cout), scale.astype(np.float32), np.float32(0.3) * unit(name, 3, (Cout,))


def dgrad_inputs(name, shape):
    B, Cin, Cout, H, W = shape
    return unit(name, 0, (B, Cout, 2 * H, 2 * W)), weights(name, Cin, Cout)


def wgrad_inputs(name, shape):
    B, Cin, Cout, H, W = shape
    return unit(name, 0, (B, Cout, 2 * H, 2 * W)), unit(name, 1, (B, Cin, H, W))


# ---------------------------------------------------------------------------------------------------------------- running a case
def run_case(name):
    """the sha256 of every output tensor of case ``name``, in order"""
    import torch
    from sonet_hip import ops

    def dev(a, off=0):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not off:
            return t.to(DEV)
        buf = torch.empty(t.numel() + off // 4, dtype=t.dtype, device=DEV)      # (a fresh allocation is 16-byte aligned and more)
        view = buf[off // 4:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == off, name
        return view

    spec = dict(CASES)[name]
    if spec[0] == "fwd":
        B, Cin, Cout, H, W = spec[2]
        x, w, scale, shift = fwd_inputs(name, spec[2])
        wp, dx, dsc, dsh = ops.upconv3x3_pack(dev(w)), dev(x), dev(scale), dev(shift)
        return [digest(wp)] + [digest(ops.upconv3x3(dx, wp, dsc, dsh, relu, Cout)) for relu in (True, False)]
    if spec[0] == "dgrad":
        B, Cin, Cout, H, W = spec[2]
        g, w = dgrad_inputs(name, spec[2])
        wpt = ops.upconv3x3_dgrad_pack(dev(w))
        return [digest(wpt), digest(ops.upconv3x3_dgrad(dev(g), wpt, Cin))]
    _, _, shape, src, off = spec
    g, x = wgrad_inputs(src, shape)
    return [digest(ops.upconv3x3_wgrad(dev(g, off), dev(x, off)))]


# ---------------------------------------------------------------------------------------------------------------- --check (no GPU)
def live_pairs(H, W):
    """(parity, tap) pairs whose shift (py + dy - 1, px + dx - 1) stays inside an H x W map for some pixel"""
    return sum(1 for pt in range(16) if (H > 1 or (pt >> 3) + ((pt >> 1) & 1) == 1) and (W > 1 or ((pt >> 2) & 1) + (pt & 1) == 1))


def reached(name):
    """the figures of case ``name`` that REACHES quotes, from the extents of sonet_hip.ops and the weight gradient's plan"""
    from sonet_hip import ops
    import upconv_wgrad_ref as G
    TP, KC, CB, MAXHW = ops.UPCONV_TILE_PIXELS, ops.UPCONV_K_CHUNK, ops.UPCONV_COUT_BLOCK, ops.UPCONV_MAX_HW
    spec = dict(CASES)[name]
    kind, (B, Cin, Cout, H, W) = spec[0], spec[2]
    assert ops.upconv3x3_supported(Cin, Cout, H, W), name
    ncols = B * H * W
    out = dict(columns=ncols, live_pairs=live_pairs(H, W), w_mod_4=W % 4)
    if kind in ("fwd", "dgrad"):
        red, rows = (Cin, Cout) if kind == "fwd" else (Cout, Cin)              # reduction channels, output rows
        flush = 1024 // (KC * (4 if kind == "fwd" else 16))                    # chunks per chain of 1024 products: 16 forward, 4 input gradient
        chunks, tiles = -(-red // KC), -(-ncols // TP)
        ends = [kc for kc in range(chunks) if kc % flush == flush - 1 or kc == chunks - 1]
        slots = TP + 2 * W + 2
        out.update(tiles=tiles, chunks=chunks, k_tail=red % KC, row_blocks=-(-rows // CB), rows_last_block=rows - (-(-rows // CB) - 1) * CB,
                   flushes=len(ends), flushes_inside=sum(1 for kc in ends if kc < chunks - 1),
                   clouds_in_first_tile=-(-min(ncols, TP) // (H * W)), idle_waves_last_tile=(tiles * TP - ncols) // 32,
                   staged_slots_of_max=(slots, TP + 2 * MAXHW + 2), staging_items=-(-2 * slots // 256))
    else:
        off = spec[4]
        nslice, cols, _ = G.plan(B, Cin, Cout, H, W)
        steps = -(-ncols // G.K_STEP)
        out.update(vec=W % 4 == 0 and off % 16 == 0, row_blocks=-(-Cin // ops.UPWGRAD_CIN_BLOCK), steps=steps,
                   columns_last_step=ncols - (steps - 1) * G.K_STEP, slices=nslice, steps_per_slice=cols // G.K_STEP,
                   flushes_inside_slice=(min(cols, ncols) - 1) // ops.UPWGRAD_FLUSH_COLS)
        assert G.K_STEP == ops.UPWGRAD_K_STEP and G.FLUSH_COLS == ops.UPWGRAD_FLUSH_COLS
    return out


def order_terms(name):
    """-> (A [rows][R] f32, Bm [R][cols] f32, chunk length): one GEMM of the case with its reduction axis in the kernel's order, chunk
    after chunk.  forward: the parity (0, 0), R = (chunk, tap, channel); input gradient: R = (chunk, pair, channel); weight gradient: the
    pair of the shift (0, 0) of the parity (0, 0), R = the flat column axis in steps."""
    import upconv_ref as R
    import upconv_train_ref as T
    import upconv_wgrad_ref as G
    spec = dict(CASES)[name]
    kind, (B, Cin, Cout, H, W) = spec[0], spec[2]

    def chunked(A, Bm, groups, C, kc):                                         # (group, channel) -> (chunk, group, channel), channels padded
        Cp = -(-C // kc) * kc
        A2, B2 = np.zeros((A.shape[0], groups, Cp), np.float32), np.zeros((groups, Cp, Bm.shape[1]), np.float32)
        A2[:, :, :C], B2[:, :C] = A.reshape(A.shape[0], groups, C), Bm.reshape(groups, C, -1)
        A2 = A2.reshape(A.shape[0], groups, Cp // kc, kc).transpose(0, 2, 1, 3).reshape(A.shape[0], -1)
        B2 = B2.reshape(groups, Cp // kc, kc, -1).transpose(1, 0, 2, 3).reshape(groups * Cp, -1)
        return A2, B2, groups * kc

    if kind == "fwd":
        x, w, _, _ = fwd_inputs(name, spec[2])
        Wg, Xg = R.parity_gemm(x, w, 0, 0)
        return chunked(Wg, Xg, 4, Cin, 16)
    if kind == "dgrad":
        g, w = dgrad_inputs(name, spec[2])
        Wg, Gg = T.dgrad_gemm(g, w)
        return chunked(Wg, Gg, 16, Cout, 16)
    g, x = wgrad_inputs(spec[3], spec[2])
    return G._flat(g[:, :, 0::2, 0::2]), np.ascontiguousarray(G._flat(x).T), G.K_STEP


def order_sensitive(name):
    """-> (chunks, output elements whose f32 sum of the chunks' partial products differs run backwards, the same product by product)"""
    A, Bm, clen = order_terms(name)
    Rn = A.shape[1]
    prod = A.astype(np.float64).T[:, :, None] * Bm.astype(np.float64)[:, None, :]          # [R][rows][cols], exact in float64
    bounds = list(range(0, Rn, clen)) + [Rn]
    parts = np.stack([prod[a:b].sum(axis=0) for a, b in zip(bounds[:-1], bounds[1:])]).astype(np.float32)

    def differs(terms):
        fwd, bwd = np.zeros(terms.shape[1:], np.float32), np.zeros(terms.shape[1:], np.float32)
        for t in range(len(terms)):
            fwd, bwd = fwd + terms[t], bwd + terms[len(terms) - 1 - t]
        return int((fwd != bwd).sum())

    return len(parts), differs(parts), differs(prod.astype(np.float32))


def check():
    """prints the figures and returns the list of what does not hold (empty: the table is what it says)"""
    bad = []
    if len(set(NAMES)) != len(NAMES):
        bad.append("case names are not unique")
    if sorted(REACHES) != sorted(NAMES):
        bad.append("REACHES does not hold exactly the case table")
    for name in NAMES:
        got = reached(name)
        for key, want in REACHES.get(name, {}).items():
            if got[key] != want:
                bad.append("%s: %s is %r, its row claims %r" % (name, key, got[key], want))
        chunks, by_chunk, by_product = order_sensitive(name)
        print("%-16s %2d chunks; reversed order ends on other bits in %d (chunk by chunk), %d (product by product) output elements"
              % (name, chunks, by_chunk, by_product))
        if by_chunk == 0:
            bad.append("%s: its inputs are not order-sensitive (%d chunks)" % (name, chunks))
    return bad


def main(argv):
    if "--check" in argv:
        bad = check()
        print("\n".join(bad) if bad else "ok")
        return 1 if bad else 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else FIXTURE
    rec = {name: run_case(name) for name in NAMES}
    for a, b in SAME_BITS:
        assert rec[a] == rec[b], "%s and %s differ" % (a, b)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d digests -> %s" % (len(rec), sum(len(v) for v in rec.values()), out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
