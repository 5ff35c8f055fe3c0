#!/usr/bin/env python
"""tools/pooled_bits.py [--out FILE] | --check -- the bits of the pooled-layer backward (so-net_amd/csrc/pooled_bwd.hip) on fixed inputs.

Every case of ``CASES`` runs through ``sonet_hip.ops`` (``pooled_dgrad`` with f32 output, bf16 output and ``wt_pack``; ``pooled_wgrad``
with f32 / bf16 rows, with and without the ``(scale, shift, relu)`` triple) and every output tensor's bytes are hashed with sha256.  Run on
an MI355X this writes case name -> list of digests (default tests/golden/pooled_bits.json); tests/test_gpu_pooled_bits.py walks the same
table and holds the tree to that file.  The file is a recording of the kernels' outputs: it is regenerated only when a change is MEANT to
change the family's arithmetic, from the parent of that change.

Inputs are integer arithmetic written here: splitmix64 of (case name, tensor number, index) in uint64, the top 24 bits to a float in
[-1, 1) (k / 2^23 - 1, exact in f32), weights times 0.1 in f32.  No library's random stream is involved.  ``--check`` (no GPU) is how
the inputs were checked to make the fmas round, so that a changed order of a sum shows.  It prints, per case, the share of the products
an entry contributes that are not f32 numbers (float64 holds them exactly): 99.9 % or more of g * W in every dgrad case, 99.97 % or
more of g * x with f32 rows, 88 - 89 % with bf16 rows (8-bit factors); and on the first dgrad case the share of the (column, channel)
fma chains of three or more entries that end on other bits when run backwards: 58 % (most chains there have three or four entries)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pooled_bits.json")
DEV = "cuda:0"

# ---------------------------------------------------------------------------------------------------------------- the case table
# dgrad: (B, C, M, C1, C2, L), what is piled on one column; each runs with f32 and with bf16 output.  A few positions are -1 and a few
# >= L (ignored entries) and the first entry of a quarter of the channels sits on column 3 (several entries per column) in every case.
#   balanced   Cin = 64: the entry-balanced kernel; two tiles, the last with 2 columns; channel slabs 40 + 24, the first mixes the panels
#   ragged1    Cin = 27, no multiple of 4: the one-channel kernel; one ragged tile; L even: the packed bf16 store
#   onepanel   no second panel; L odd: the scalar bf16 store; the last tile holds one column
#   rankpile   half of the entries on column 5, a quarter on column L - 1: a bucket above PS_CAP = 2048 (the sort kernel's global rank
#              path), tens of rounds of 384 with a cut column in every chunk and chunks that are one column end to end
#   resume1    400 entries on one column in the one-channel kernel: more than PD_SQ = 128 per group, a column resumed from the stored value
DGRAD = [
    ("dgrad_balanced", (2, 96, 8, 16, 48, 130), None),
    ("dgrad_ragged1", (2, 40, 6, 10, 17, 70), None),
    ("dgrad_onepanel", (2, 48, 7, 44, 0, 257), None),
    ("dgrad_rankpile", (1, 384, 64, 64, 256, 512), "half_quarter"),
    ("dgrad_resume1", (2, 96, 8, 10, 17, 130), "400"),
]
# matrix cores (wt_pack given, bf16 output).  The positions of a (cloud, channel) row are DISTINCT columns: the kernel adds the entries of a
# (channel, column) pair with a compare-and-swap in arrival order, which is order-free -- and so reproducible to the bit -- only when no
# pair occurs twice.  64-column workgroups with L even and no multiple of 8; B * ceil(L / 128) >= 2048 selects the 128-column workgroups,
# L = 16384 with the 16-byte store, L = 16386 with the dword tail.
MFMA = [
    ("mfma_64col_two_panels", (2, 96, 8, 16, 48, 130)),
    ("mfma_64col_one_panel", (2, 64, 16, 64, 0, 514)),
    ("mfma_128col_vector_store", (16, 16, 4, 64, 0, 16384)),
    ("mfma_128col_dword_tail", (16, 16, 4, 64, 0, 16386)),
]
# wgrad: (B, C, M, Ci, L); each runs the four entry points, the two with the triple with relu off and on (six outputs).
#   Ci = 11: the last bf16 row pair has one row; L = 500: f32 rows take the vector copy, bf16 rows the scalar one; L = 501: rows neither
#   16-byte sized nor aligned, the scalar copy; L = 504: the vector copy for both; M = 64 / 33: the second half of the entries full / holds
#   one; C = 384 / 5: every thread / a handful of threads own a channel
WGRAD = [
    ("wgrad_base", (3, 40, 16, 10, 500)),
    ("wgrad_ci11", (3, 40, 16, 11, 500)),
    ("wgrad_l501", (3, 40, 16, 10, 501)),
    ("wgrad_l504", (3, 40, 16, 10, 504)),
    ("wgrad_m64", (3, 40, 64, 10, 500)),
    ("wgrad_m33", (3, 40, 33, 10, 500)),
    ("wgrad_c384", (3, 384, 16, 10, 500)),
    ("wgrad_c5", (3, 5, 16, 10, 500)),
]
WGRAD_RUNS = [("f32", None), ("bf16", None), ("f32", 0), ("f32", 1), ("bf16", 0), ("bf16", 1)]      # (rows, relu of the triple or None)

CASES = ([(n + "_" + o, ("dgrad", n, s, p, o)) for n, s, p in DGRAD for o in ("f32", "bf16")] + [(n, ("mfma", n, s)) for n, s in MFMA] +
         [(n, ("wgrad", n, s)) for n, s in WGRAD])
NAMES = [n for n, _ in CASES]


# ---------------------------------------------------------------------------------------------------------------- the inputs
def u64(case, tensor, n):
    """splitmix64 of (case name, tensor number, index 0 .. n - 1)"""
    seed = 0xCBF29CE484222325
    for ch in case.encode():
        seed = ((seed ^ ch) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF                         # FNV-1a of the name
    seed ^= (tensor * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def unit(case, tensor, shape):
    """floats in [-1, 1): the top 24 bits k of the hash as k / 2^23 - 1"""
    k = (u64(case, tensor, int(np.prod(shape))) >> np.uint64(40)).astype(np.float64)
    return (k / 2.0 ** 23 - 1.0).astype(np.float32).reshape(shape)


def below(case, tensor, shape, n):
    return (u64(case, tensor, int(np.prod(shape))) % np.uint64(n)).astype(np.int32).reshape(shape)


def dgrad_inputs(name, shape, pile):
    B, C, M, C1, C2, L = shape
    g = unit(name, 0, (B, C, M))
    W = unit(name, 1, (C, C1 + C2)) * np.float32(0.1)
    pos = below(name, 2, (B, C, M), L)
    if pile == "half_quarter":
        sel = below(name, 3, (B, C, M), 4)
        pos = np.where(sel < 2, 5, np.where(sel == 2, L - 1, pos)).astype(np.int32)
    elif pile == "400":
        pos.reshape(B, C * M)[:, :400] = 77
    pos[:, : C // 4, 0] = 3
    pos[:, 0, 2] = -1
    pos[:, 1, 1] = -1
    pos[:, 2, 0] = L
    pos[:, 3, 1] = L + 7
    return g, pos, W


def mfma_inputs(name, shape):
    B, C, M, C1, C2, L = shape
    g = unit(name, 0, (B, C, M))
    W = unit(name, 1, (C, C1 + C2)) * np.float32(0.1)
    step = L // M
    pos = (np.arange(M, dtype=np.int32).reshape(1, 1, M) * step + below(name, 2, (B, C, M), step)).astype(np.int32)
    pos[:, 0, 2] = -1
    pos[:, 1, 1] = L + 3
    return g, pos, W


def wgrad_inputs(name, shape):
    B, C, M, Ci, L = shape
    g = unit(name, 0, (B, M, C))                                   # (the entries come transposed: B x M x C)
    x = unit(name, 1, (B, Ci, L))
    pos = below(name, 2, (B, M, C), L)
    pos[:, 3, :] = 0                                               # an "empty node": every channel gathers position 0
    pos[1, 8, 0] = pos[1, 7, 0]                                    # a column twice in one channel
    pos[2, 0, 0] = -1
    pos[0, 1, C - 1] = L + 5
    scale = np.float32(1.0) + np.float32(0.5) * unit(name, 4, (Ci,))
    shift = np.float32(0.3) * unit(name, 5, (Ci,))
    return g, pos, x, scale, shift


# ---------------------------------------------------------------------------------------------------------------- running a case
def digest(t):
    import torch
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(name):
    """the sha256 of every output tensor of case ``name``, in order"""
    import torch
    from sonet_hip import ops

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    spec = dict(CASES)[name]
    if spec[0] == "dgrad":
        _, base, shape, pile, out = spec
        B, C, M, C1, C2, L = shape
        g, pos, W = dgrad_inputs(base, shape, pile)
        outs = ops.pooled_dgrad(dev(g), dev(pos), dev(W), C1, C2, L, out_dtype=torch.float32 if out == "f32" else torch.bfloat16)
        return [digest(t) for t in outs if t is not None]
    if spec[0] == "mfma":
        _, base, shape = spec
        B, C, M, C1, C2, L = shape
        g, pos, W = mfma_inputs(base, shape)
        assert ops.pooled_dgrad_mfma_ok(C, C1, C2, L), name
        wt = np.zeros(((C1 + C2 + 31) // 32 * 32, C), np.float32)
        wt[: C1 + C2] = W.T
        outs = ops.pooled_dgrad(dev(g), dev(pos), dev(W), C1, C2, L, out_dtype=torch.bfloat16, wt_pack=ops.pointmlp_pack(dev(wt), "bf16"))
        return [digest(t) for t in outs if t is not None]
    _, base, shape = spec
    g, pos, x, scale, shift = wgrad_inputs(base, shape)
    dg, dp, dx, dsc, dsh = dev(g), dev(pos), dev(x), dev(scale), dev(shift)
    dxb = dx.to(torch.bfloat16)                                    # (round to nearest even, as every bf16 store of the project)
    return [digest(ops.pooled_wgrad(dg, dp, dx if rows == "f32" else dxb, None if relu is None else (dsc, dsh, bool(relu))))
            for rows, relu in WGRAD_RUNS]


# ---------------------------------------------------------------------------------------------------------------- --check (no GPU)
def inexact(a, b):
    """share of the products a * b (float32 operands, broadcast) that are not float32 numbers; float64 holds them exactly"""
    p = a.astype(np.float64) * b.astype(np.float64)
    return float((p.astype(np.float32).astype(np.float64) != p).mean())


# what --check holds the inputs to (the figures it printed when the table was written are in the module's docstring): the share of the
# products that are no f32 numbers, over the dgrad cases, the wgrad cases with f32 and with bf16 rows (an 8-bit factor: the product is
# exact when the two factors' trailing zero bits add up to 8 or more), and the share of the reversed chains that end on other bits
CHECK_FLOORS = {"dgrad": 0.99, "wgrad_f32": 0.99, "wgrad_bf16": 0.85, "chains": 0.5}


def check():
    """prints the figures and returns the worst share per kind (the keys of CHECK_FLOORS)"""
    worst = {k: 1.0 for k in CHECK_FLOORS}
    for name, shape, pile in DGRAD:
        B, C, M, C1, C2, L = shape
        g, pos, W = dgrad_inputs(name, shape, pile)
        live = (pos >= 0) & (pos < L)
        share = inexact(g[live][:2048, None], W[np.nonzero(live)[1][:2048]])        # (the first 2048 entries, every input channel)
        worst["dgrad"] = min(worst["dgrad"], share)
        print("%-16s g * W not f32: %.4f of %d products" % (name, share, min(2048, int(live.sum())) * (C1 + C2)))
    for name, shape in WGRAD:
        g, pos, x, _, _ = wgrad_inputs(name, shape)
        B, M, C = g.shape
        live = (pos >= 0) & (pos < shape[4])
        bb, mm, cc = np.nonzero(live)
        xg = x[bb, :, pos[live]]                                  # [entries][Ci]
        xb = (((xg.view(np.uint32) + np.uint32(0x7FFF) + ((xg.view(np.uint32) >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16))
              << np.uint32(16)).view(np.float32)
        s32, s16 = inexact(g[live][:, None], xg), inexact(g[live][:, None], xb)
        worst["wgrad_f32"], worst["wgrad_bf16"] = min(worst["wgrad_f32"], s32), min(worst["wgrad_bf16"], s16)
        print("%-16s g * x not f32: %.4f (f32 rows) %.4f (bf16 rows)" % (name, s32, s16))
    name, shape, pile = DGRAD[0]
    B, C, M, C1, C2, L = shape
    g, pos, W = dgrad_inputs(name, shape, pile)
    diff = total = 0
    for b in range(B):
        for col in range(L):
            ids = np.nonzero(pos[b].reshape(-1) == col)[0]
            if len(ids) < 3:
                continue
            fwd, bwd = np.zeros(C1 + C2, np.float64), np.zeros(C1 + C2, np.float64)
            for order, acc in ((ids, fwd), (ids[::-1], bwd)):
                for e in order:                                   # fma: the exact product plus the sum, one rounding to f32
                    acc[:] = (g[b].reshape(-1)[e].astype(np.float64) * W[e // M].astype(np.float64) + acc).astype(np.float32)
            diff += int((fwd != bwd).sum())
            total += C1 + C2
    print("%-16s chains of >= 3 entries that end on other bits run backwards: %.4f of %d" % (name, diff / total, total))
    worst["chains"] = diff / total
    return worst


def main(argv):
    if "--check" in argv:
        worst = check()
        bad = [k for k, floor in CHECK_FLOORS.items() if worst[k] < floor]
        print("worst shares %s: %s" % (worst, "below the floor: " + ", ".join(bad) if bad else "ok"))
        return 1 if bad else 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else FIXTURE
    sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))
    rec = {name: run_case(name) for name in NAMES}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d digests -> %s" % (len(rec), sum(len(v) for v in rec.values()), out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
