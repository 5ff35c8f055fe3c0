"""Numpy restatement of the fused Chamfer loss (sonet_chamfer_loss_f32 / sonet_chamfer_grad_f32) and seeded input makers.
Plain module: no fixtures, no GPU.

* indices: the exact search of oracle.cpu_oracle.chamfer_nn, both directions;
* elements: float32, d = sel - q per coordinate, sqrt(((dx*dx + dy*dy) + dz*dz) + 1e-8f), every operation rounded to float32 (numpy
  never fuses; its float32 square root is correctly rounded) -- what the kernel is held to bit for bit;
* sums, losses and the gradient: float64, from GIVEN indices.

The gradient has two element models: ``elems="f64"`` recomputes the elements in float64 (the reference's expression in double precision:
what ``autograd64`` differentiates), ``elems="f32"`` divides by the float32 elements widened to float64 (what the kernel does).  Every
gradient function also returns sum|term| per entry, the scale of the gates.
"""
import math

import numpy as np

import edge_clouds as E

F32 = np.float32
EPS = 1e-8


# ------------------------------------------------------------------------------------------ forward
def indices(pred, gt):
    """(nn_pg B x M i32, nn_gp B x N i32)."""
    from oracle import cpu_oracle as O
    return O.chamfer_nn(pred, gt), O.chamfer_nn(gt, pred)


def _select(src, idx):
    """src B x 3 x Ns, idx B x Nq -> B x 3 x Nq."""
    return np.take_along_axis(src, np.broadcast_to(idx[:, None, :].astype(np.int64), (src.shape[0], 3, idx.shape[1])), axis=2)


def elements(q, db, nn):
    """B x Nq float32: robust_norm of (db[nn] - q) in float32, the kernel's order of operations."""
    q, db = np.asarray(q, F32), np.asarray(db, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = _select(db, nn) - q
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        e = np.sqrt(((dx * dx + dy * dy) + dz * dz) + F32(EPS))
    assert e.dtype == F32
    return e


def elements64(q, db, nn):
    d = _select(np.asarray(db, np.float64), nn) - np.asarray(q, np.float64)
    return np.sqrt((d * d).sum(axis=1) + EPS)


def fsum_rows(e):
    """B float64: the exactly rounded sum of every row (math.fsum); NaN / inf rows by numpy."""
    out = np.empty(e.shape[0], np.float64)
    for b in range(e.shape[0]):
        row = e[b].astype(np.float64)
        out[b] = math.fsum(row.tolist()) if np.isfinite(row).all() else row.sum()
    return out


def terms(pred, gt, nn_pg=None, nn_gp=None):
    """dict: nn_pg, nn_gp, elem_fwd, elem_bwd (f32), sums B x 2 f64 (exactly rounded sums of the elements)."""
    if nn_pg is None:
        nn_pg, nn_gp = indices(pred, gt)
    ef, eb = elements(pred, gt, nn_pg), elements(gt, pred, nn_gp)
    return dict(nn_pg=nn_pg, nn_gp=nn_gp, elem_fwd=ef, elem_bwd=eb, sums=np.stack([fsum_rows(ef), fsum_rows(eb)], axis=1))


def losses(t):
    """The five attributes of ChamferLoss from ``terms`` (float64): forward_loss, backward_loss, forward_loss_array,
    backward_loss_array, loss_array."""
    B, M, N = t["elem_fwd"].shape[0], t["elem_fwd"].shape[1], t["elem_bwd"].shape[1]
    fa, ba = t["sums"][:, 0] / M, t["sums"][:, 1] / N
    return dict(forward_loss=t["sums"][:, 0].sum() / (B * M), backward_loss=t["sums"][:, 1].sum() / (B * N), forward_loss_array=fa,
                backward_loss_array=ba, loss_array=fa + ba)


# ------------------------------------------------------------------------------------------ gradient
def grad(pred, gt, nn_pg, nn_gp, gf=1.0, gb=1.0, elems="f64", drop_backward=False, gb_is_gf=False):
    """(d(gf * forward_loss + gb * backward_loss) / d pred B x 3 x M float64, sum|term| B x 3 x M float64) at the given indices.
    Forward term first, then the backward terms in ascending n.  ``drop_backward`` / ``gb_is_gf``: two deliberate mistakes, for the
    tests that show the gate sees them."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    B, _, M = p.shape
    N = g.shape[2]
    if elems == "f32":
        ef, eb = elements(pred, gt, nn_pg).astype(np.float64), elements(gt, pred, nn_gp).astype(np.float64)
    else:
        ef, eb = elements64(pred, gt, nn_pg), elements64(gt, pred, nn_gp)
    if gb_is_gf:
        gb = gf
    cf, cb = float(gf) / (B * M), float(gb) / (B * N)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = cf * (p - _select(g, nn_pg)) / ef[:, None, :]
        mag = np.abs(out)
        if not drop_backward:
            tb = cb * (_select(p, nn_gp) - g) / eb[:, None, :]                 # B x 3 x N: the term of gt point n, owed to nn_gp[n]
            for b in range(B):
                for c in range(3):
                    np.add.at(out[b, c], nn_gp[b], tb[b, c])                   # (unbuffered, in index order: ascending n)
                    np.add.at(mag[b, c], nn_gp[b], np.abs(tb[b, c]))
    return out, mag


def autograd64(pred, gt, nn_pg, nn_gp, gf=1.0, gb=1.0):
    """float64 autograd of the reference's expression (models/losses.py:269-290) with gathers by the given indices -> B x 3 x M."""
    import torch
    p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    g = torch.from_numpy(np.asarray(gt, np.float64))
    B = p.shape[0]
    ipg = torch.from_numpy(nn_pg.astype(np.int64)).unsqueeze(1).expand(B, 3, nn_pg.shape[1])
    igp = torch.from_numpy(nn_gp.astype(np.int64)).unsqueeze(1).expand(B, 3, nn_gp.shape[1])
    sel_gt = torch.gather(g, 2, ipg).unsqueeze(1)
    sel_pr = torch.gather(p, 2, igp).unsqueeze(1)
    robust_norm = lambda v: ((v ** 2).sum(dim=2) + EPS).sqrt()                   # noqa: E731  (models/losses.py:17-27)
    fwd = robust_norm(sel_gt - p.unsqueeze(1)).mean()
    bwd = robust_norm(sel_pr - g.unsqueeze(1)).mean()
    (gf * fwd + gb * bwd).backward()
    return p.grad.numpy()


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-300))


def ulps(a, b):
    """|a - b| in units of the float32 spacing at b (finite, positive b)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


# |dpred - ref64| <= GATE * sum|term| per entry.  The only f32 quantity in a term is the element: relative error at most 3 * 2^-24 (the
# rounded squares, three additions of non-negative terms halved by the root, the root's own rounding); the final rounding adds 2^-24:
# 2^-22 together, and twice that, 2^-21, is the bound an implementation must meet.  The f32-element model of this file stays within
# 3.173 x 2^-24 on every fixture and test shape (tests/test_chamfer_loss_cpu.py), so the gate is tightened to twice 3.2 x 2^-24.
GATE = 6.4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------ inputs
def continuous(B, M, N, seed):
    """pred B x 3 x M, gt B x 3 x N: uniform in [-1, 1]^3."""
    r = np.random.default_rng(seed)
    return (r.random((B, 3, M)) * 2 - 1).astype(F32), (r.random((B, 3, N)) * 2 - 1).astype(F32)


def lattice(B, M, N):
    """The tie-heavy lattice clouds of edge_clouds.chamfer_case: pred = its queries, gt = its database."""
    return E.chamfer_case(M, N, B=B)


def coincident(B, M, N, seed):
    """Continuous clouds where every other predicted point IS a gt point (distinct ones while M / 2 <= N): elements at the 1e-4 floor
    of robust_norm, gradient terms of exactly zero."""
    pred, gt = continuous(B, M, N, seed)
    r = np.random.default_rng(seed + 1)
    h = (M + 1) // 2
    for b in range(B):
        take = r.permutation(N)[:h] if h <= N else r.integers(0, N, h)
        pred[b, :, ::2] = gt[b][:, take]
    return pred, gt


def one_owner(B, M, N, seed, owner=None):
    """Every gt point is nearest to ONE predicted point (the others sit far away): a list of N backward terms for that point, none for
    the rest."""
    r = np.random.default_rng(seed)
    gt = (r.random((B, 3, N)) * F32(0.2) - F32(0.1)).astype(F32)
    pred = (r.random((B, 3, M)) + F32(4.0)).astype(F32)
    owner = M // 2 if owner is None else owner
    pred[:, :, owner] = np.array([0.01, -0.02, 0.03], F32)
    return pred, gt


def make(kind, B, M, N, seed=0):
    if kind == "continuous":
        return continuous(B, M, N, 9000 + 31 * M + N + B + seed)
    if kind == "lattice":
        return lattice(B, M, N)
    if kind == "coincident":
        return coincident(B, M, N, 9500 + 31 * M + N + B + seed)
    raise ValueError(kind)


FWD_M = (1, 2, 255, 256, 257, 1023, 1025)
FWD_N = (1, 3, 256, 257, 1024, 1025, 2049)
GRAD_SHAPES = [(M, N) for M in FWD_M for N in FWD_N if N <= 1025]
GOLDEN_CASES = ("continuous_b3_m257_n1000", "lattice_ties", "coincident_half")
