"""Segmenter layer 1 in its node-wise (split) form, restated for the tests -- forward AND backward, in float64, without autograd.

The layer's input concatenates, in the order of ``Segmenter._layer1_blocks()``,

    x_dec | x | centers | sn | onehot | first | fm_first | fm_knn | fm_final | feature

of which x_dec, x, sn, first vary per column (point copy), centers and the three fm_* maps are node features broadcast back to the
columns through ``ids`` and onehot, feature are per cloud.  With W's columns split the same way,

    raw = W_p . x_p + (W_n . x_n + W_g . x_g)[node of the column] + bias,     y = relu(batch_norm(raw))

and every gradient of the per-node / per-cloud blocks is a function of gz[b][c][m] = the sum of g_raw[b][c][l] over the columns of
node m.  ``dense_step`` is float64 autograd of relu(batch_norm(conv1x1(cat(...)))): the expression the split must reproduce.
``node_sum_f32`` restates the device's per-node sum: one f32 chain per (b, c, m) in ascending column order."""
import numpy as np
import torch

ORDER = ("x_dec", "x", "centers", "sn", "onehot", "first", "fm_first", "fm_knn", "fm_final", "feature")
PER_COLUMN, PER_NODE, PER_CLOUD = ("x_dec", "x", "sn", "first"), ("centers", "fm_first", "fm_knn", "fm_final"), ("onehot", "feature")
WITH_GRAD = ("first", "fm_first", "fm_knn", "fm_final", "feature")            # the reference detaches the others
# narrowed blocks for the CPU tests, the same order (the model: 3 3 3 3 16 384 384 512 1024 1024)
SMALL_WIDTHS = dict(x_dec=3, x=3, centers=3, sn=3, onehot=4, first=6, fm_first=6, fm_knn=5, fm_final=7, feature=7)
BREAKS = ("drop_glob_grad", "swap_blocks", "miss_last_copy", "centers_grad", "drop_sum_m")


def blocks(widths):
    out, pos = {}, 0
    for name in ORDER:
        out[name] = (pos, pos + widths[name])
        pos += widths[name]
    return out


def make_case(seed=0, B=2, N=40, k=3, M=4, Cout=8, widths=SMALL_WIDTHS, empty_node=2):
    """float64 inputs, parameters and an output gradient; ``empty_node`` owns no column."""
    g = torch.Generator().manual_seed(seed)
    L = k * N
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ids = torch.randint(0, M - 1, (B, L), generator=g)
    ids = ids + (ids >= empty_node).long()                                    # skips empty_node, reaches M - 1
    x = {}
    for name in ORDER:
        w = widths[name]
        x[name] = rnd(B, w, L) if name in PER_COLUMN else (rnd(B, w, M) if name in PER_NODE else rnd(B, w))
    Cin = sum(widths.values())
    return dict(B=B, L=L, M=M, Cout=Cout, widths=dict(widths), ids=ids, x=x, W=rnd(Cout, Cin) / Cin ** 0.5, bias=rnd(Cout),
                gamma=1.0 + 0.1 * rnd(Cout), beta=0.1 * rnd(Cout), gy=rnd(B, Cout, L), eps=1e-5)


def dense_step(c, relu=True):
    """float64 autograd of the dense expression -> (y, {name: gradient}) over the inputs with a gradient, 'W', 'gamma', 'beta'."""
    B, L, ids = c["B"], c["L"], c["ids"]
    leaf = {n: c["x"][n].clone().requires_grad_(n in WITH_GRAD) for n in ORDER}
    W, gamma, beta = (c[n].clone().requires_grad_(True) for n in ("W", "gamma", "beta"))
    parts = []
    for n in ORDER:
        t = leaf[n]
        if n in PER_NODE:
            t = torch.gather(t, 2, ids.unsqueeze(1).expand(B, t.shape[1], L))
        elif n in PER_CLOUD:
            t = t.unsqueeze(2).expand(B, t.shape[1], L)
        parts.append(t)
    raw = torch.nn.functional.conv1d(torch.cat(parts, dim=1), W.unsqueeze(2), c["bias"])
    y = torch.nn.functional.batch_norm(raw, None, None, gamma, beta, True, 0.1, c["eps"])
    if relu:
        y = torch.relu(y)
    y.backward(c["gy"])
    grads = {n: leaf[n].grad for n in WITH_GRAD}
    grads.update(W=W.grad, gamma=gamma.grad, beta=beta.grad)
    return y.detach(), grads


def split_step(c, relu=True, brk=None):
    """The split layer step by hand in float64 -> (y, {name: gradient}).  ``brk``: one of BREAKS, a deliberately wrong step."""
    B, L, M, ids, x, W = c["B"], c["L"], c["M"], c["ids"], c["x"], c["W"]
    blk = blocks(c["widths"])
    cols = lambda names: torch.cat([W[:, blk[n][0]:blk[n][1]] for n in names], dim=1)
    x_p, x_n, x_g = (torch.cat([x[n] for n in names], dim=1) for names in (PER_COLUMN, PER_NODE, PER_CLOUD))
    W_p, W_n, W_g = cols(PER_COLUMN), cols(PER_NODE), cols(PER_CLOUD)
    # forward
    z = torch.einsum("oc,bcm->bom", W_n, x_n) + (x_g @ W_g.t()).unsqueeze(2)
    idx = ids.unsqueeze(1).expand(B, c["Cout"], L)
    raw = torch.einsum("oc,bcl->bol", W_p, x_p) + torch.gather(z, 2, idx) + c["bias"].view(1, -1, 1)
    n = B * L
    mean = raw.mean(dim=(0, 2))
    var = ((raw - mean.view(1, -1, 1)) ** 2).mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(var + c["eps"])
    sc, sh = c["gamma"] * invstd, c["beta"] - mean * c["gamma"] * invstd
    pre = raw * sc.view(1, -1, 1) + sh.view(1, -1, 1)
    y = torch.relu(pre) if relu else pre
    # backward: the two sums, the coefficients, the apply pass, the per-node sums
    g = c["gy"] * (pre > 0) if relu else c["gy"]
    s1, s2 = g.sum(dim=(0, 2)), (g * raw).sum(dim=(0, 2))
    sg = invstd * (s2 - mean * s1)
    a = c["gamma"] * invstd
    b = -a * invstd * sg / n
    c0 = -a * s1 / n - b * mean
    g_raw = a.view(1, -1, 1) * g + b.view(1, -1, 1) * raw + c0.view(1, -1, 1)
    src = g_raw
    if brk == "miss_last_copy":                                               # every node's last column is left out of its sum
        src = g_raw.clone()
        for bb in range(B):
            for m in range(M):
                own = (ids[bb] == m).nonzero().flatten()
                if own.numel():
                    src[bb, :, own[-1]] = 0
    gz = torch.zeros(B, c["Cout"], M, dtype=torch.float64).scatter_add_(2, idx, src)
    gsum = gz[:, :, 0] if brk == "drop_sum_m" else gz.sum(dim=2)
    d_p = torch.einsum("oc,bol->bcl", W_p, g_raw)
    d_n = torch.einsum("oc,bom->bcm", W_n, gz)
    d_g = gsum @ W_g
    dW_p = torch.einsum("bol,bcl->oc", g_raw, x_p)
    dW_n = torch.einsum("bom,bcm->oc", gz, x_n)
    dW_g = gz.sum(dim=2).t() @ x_g
    if brk == "drop_glob_grad":
        dW_g = torch.zeros_like(dW_g)
    # every block back to its place: inputs by name, the weight gradient into W's column blocks
    grads, dW = {}, torch.zeros_like(W)
    where = {n: n for n in ORDER}
    if brk == "swap_blocks":
        where["fm_first"], where["first"] = "first", "fm_first"              # (equal widths: the scatter still fits)
    for names, dx, dw in ((PER_COLUMN, d_p, dW_p), (PER_NODE, d_n, dW_n), (PER_CLOUD, d_g, dW_g)):
        at = 0
        for nme in names:
            w = c["widths"][nme]
            lo, hi = blk[where[nme]]
            dW[:, lo:hi] = dw[:, at:at + w]
            if nme in WITH_GRAD or (brk == "centers_grad" and nme == "centers"):
                grads[nme] = dx[:, at:at + w]
            at += w
    grads.update(W=dW, gamma=sg, beta=s1)
    return y, grads


def worst_difference(got, want):
    """Largest |got - want| / max(1, max |want|) over the gradients; inf when the two do not name the same tensors."""
    if sorted(got) != sorted(want):
        return float("inf")
    return max(float((got[k] - want[k]).abs().max()) / max(1.0, float(want[k].abs().max())) for k in want)


def same_bits(a, b):
    """Two float32 arrays hold the same bit patterns (a NaN equals the same NaN, +0 differs from -0)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def node_sum_f32(g_raw, ids, M):
    """gz[b][c][m] = g_raw[b][c][l] summed over the columns with ids[b][l] == m in ascending l, ONE float32 chain from 0 (ids outside
    [0, M): nowhere) -- numpy float32 arrays in, float32 out."""
    g_raw = np.ascontiguousarray(g_raw, dtype=np.float32)
    B, C, L = g_raw.shape
    gz = np.zeros((B, C, M), dtype=np.float32)
    for b in range(B):
        for l in range(L):
            m = int(ids[b, l])
            if 0 <= m < M:
                gz[b, :, m] = gz[b, :, m] + g_raw[b, :, l]                    # (float32 + float32: one rounding per addend)
    return gz
