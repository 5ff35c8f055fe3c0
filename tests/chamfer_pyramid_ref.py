"""Numpy restatement of the Chamfer loss pyramid (sonet_chamfer_pyramid_loss_f32 / sonet_chamfer_pyramid_grad_f32): up to three
predicted clouds against one gt cloud.  Plain module: no fixtures, no GPU.

The pyramid is tests/chamfer_ref.py per level -- ``terms``, ``losses`` and ``grad`` below are that and nothing else.  What is new in the
kernel is HOW the gradient finds the backward terms of a predicted point: through stable inverse lists (the gt points n sorted by
their owner nn_gp[n], ties by ascending n) instead of a compare of every predicted point with every gt point.  ``inverse_lists`` and
``grad_lists`` restate that route; it adds the float64 terms in the order ``chamfer_ref.grad`` adds them, so the two agree bit for bit.
``grad_lists`` also carries two deliberate mistakes (an order that is not stable, a dropped last segment) for the tests that show
they are seen."""
import numpy as np

import chamfer_ref as R


def terms(preds, gt):
    return [R.terms(p, gt) for p in preds]


def losses(ts):
    return [R.losses(t) for t in ts]


def grad(preds, gt, ts, gscale, elems="f64"):
    """Per level (gradient B x 3 x M_l float64, sum|term|) at the indices of ``ts``; gscale L x 2 (gf_l, gb_l)."""
    return [R.grad(p, gt, t["nn_pg"], t["nn_gp"], float(gs[0]), float(gs[1]), elems=elems) for p, t, gs in zip(preds, ts, gscale)]


def inverse_lists(nn_gp_row, M, stable=True):
    """One cloud: (order N, start M + 1) -- order lists the gt points by ascending owner, inside an owner by ascending n; the list of
    predicted point m is order[start[m]:start[m + 1]].  The starts come from the boundaries of the sorted owners, as in the kernel.
    ``stable=False``: the same segments with every list reversed (what a sort that does not keep equal owners in order may give)."""
    owner = np.asarray(nn_gp_row, np.int64)
    N = owner.shape[0]
    if stable:
        order = np.argsort(owner, kind="stable")
    else:
        order = np.lexsort((-np.arange(N), owner))
    so = owner[order]
    start = np.full(M + 1, -1, np.int64)
    start[M] = N
    first = np.flatnonzero(np.concatenate([[True], so[1:] != so[:-1]]))          # positions where a new owner begins
    start[so[first]] = first
    for m in range(M - 1, -1, -1):                                               # an owner without a list: an empty segment
        if start[m] < 0:
            start[m] = start[m + 1]
    return order, start


def grad_lists(pred, gt, nn_pg, nn_gp, gf=1.0, gb=1.0, elems="f64", stable=True, drop_last_segment=False):
    """``chamfer_ref.grad`` by way of the inverse lists: the forward term first, then the list of m front to back -> (B x 3 x M
    float64, sum|term|).  ``drop_last_segment``: the list of the largest owner is never walked (a boundary scan that forgets the end)."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    B, _, M = p.shape
    N = g.shape[2]
    if elems == "f32":
        ef, eb = R.elements(pred, gt, nn_pg).astype(np.float64), R.elements(gt, pred, nn_gp).astype(np.float64)
    else:
        ef, eb = R.elements64(pred, gt, nn_pg), R.elements64(gt, pred, nn_gp)
    cf, cb = float(gf) / (B * M), float(gb) / (B * N)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = cf * (p - R._select(g, nn_pg)) / ef[:, None, :]
        mag = np.abs(out)
        tb = cb * (R._select(p, nn_gp) - g) / eb[:, None, :]
        for b in range(B):
            order, start = inverse_lists(nn_gp[b], M, stable=stable)
            owners = np.unique(nn_gp[b])
            for m in owners:
                if drop_last_segment and m == owners[-1]:
                    continue
                for n in order[start[m]:start[m + 1]]:
                    out[b, :, m] += tb[b, :, n]
                    mag[b, :, m] += np.abs(tb[b, :, n])
    return out, mag


def cpu_search(q, db):
    """A stand-in for ops.chamfer_nn on CPU tensors (the exact search of oracle.cpu_oracle): lets ChamferLoss's torch arithmetic run
    where there is no GPU."""
    import torch
    from oracle import cpu_oracle as O
    return torch.from_numpy(O.chamfer_nn(q.detach().numpy(), db.detach().numpy()).astype(np.int32))


# (M_l per level, N): the workgroup (256), pair-tail and 1024-point tile edges of the search, two equal levels, a level of one point
FWD_SHAPES = [((1,), 1), ((2,), 3), ((255, 2), 1023), ((256, 256), 1024), ((257, 1, 255), 1025), ((1025, 257, 2), 2049), ((1025, 256), 3),
              ((2, 1025, 1), 1024)]
GRAD_SHAPES = [((1,), 1), ((2, 1), 3), ((255, 257), 256), ((256, 256, 1), 257), ((1025, 2, 255), 1024), ((257, 1023), 1025), ((1, 256), 1025)]
