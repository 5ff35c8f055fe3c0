"""Float64 restatements of the decoder's up-convolution layer in TRAINING (UpConv, models/layers.py:214-240 of the reference; the six
``UpConv`` + three ``ConvToPC`` of DecoderConv, models/networks.py:372-431):

    pre = BatchNorm_train(conv3x3_pad1(upsample2_nearest(x), w) + b),   y = relu(pre)

``dgrad_folded`` is the input gradient in the folded form the kernel computes (sonet_upconv3x3_dgrad_f32): with the sixteen (parity, tap)
matrices Wf of ``upconv_ref.fold_weights`` and its zero-padded shift,

    dx = sum over py, px, dy, dx' of  Wf[py][px][dy][dx']^T . shifted(g[:, :, py::2, px::2], 1 - py - dy, 1 - px - dx')

``layer_train64`` is the whole layer step written out (forward, BatchNorm statistics, every gradient) with an optional FORCED ReLU mask;
``decoder_train64`` the DecoderConv chain by float64 autograd with per-layer forced masks.  The BREAKS are the mistakes a kernel of this
form can make; the CPU tests show that each one is seen.
"""
import numpy as np
import torch
import torch.nn.functional as F

import upconv_ref as R

BREAKS = ("shift_sign", "parity_dropped", "taps_transposed", "seam")
FOLD_T = tuple(tuple(R.FOLD[tap][par] for tap in range(2)) for par in range(2))        # the tap table with parity and tap exchanged


def _rolled(x, sy, sx):
    """The shift on the FLAT column axis without the zero slot: rows, maps and clouds run into one another."""
    B, C, H, W = x.shape
    flat = x.transpose(1, 0, 2, 3).reshape(C, B * H * W)
    return np.roll(flat, -(sy * W + sx), axis=1).reshape(C, B, H, W).transpose(1, 0, 2, 3)


def dgrad_folded(g, w, brk=None):
    """g [B][Cout][2H][2W], w [Cout][Cin][3][3] -> dx [B][Cin][H][W] float64, the folded form (``brk``: one of BREAKS)."""
    assert brk is None or brk in BREAKS
    g = np.asarray(g, np.float64)
    wf = R.fold_weights(w, FOLD_T if brk == "taps_transposed" else R.FOLD)
    B, Cout, H2, W2 = g.shape
    dx = np.zeros((B, wf.shape[5], H2 // 2, W2 // 2))
    for py in range(2):
        for px in range(2):
            if brk == "parity_dropped" and (py, px) == (1, 1):
                continue
            plane = g[:, :, py::2, px::2]
            for dy in range(2):
                for dx_ in range(2):
                    sy, sx = 1 - py - dy, 1 - px - dx_
                    if brk == "shift_sign":
                        sx = -sx
                    src = _rolled(plane, sy, sx) if brk == "seam" else R.shifted(plane, sy, sx)
                    dx += np.einsum("oc,bohw->bchw", wf[py, px, dy, dx_], src)
    return dx


def make_g(B, Cout, H, W, seed, scale=1.0):
    """Seeded cotangent at gradient scale: a Chamfer gradient through the point heads is of order 1e-3 per element and sparse in sign."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, Cout, 2 * H, 2 * W)) * 1e-3 * scale).astype(np.float32)


def make_w(Cin, Cout, seed):
    """Weights as ``UpConv.weight_init``: standard deviation sqrt(2 / (9 Cout))."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cout))).astype(np.float32)


def make_layer_case(B, Cin, Cout, H, W, seed):
    """Seeded operands of one layer step: x of order 1, weights as ``UpConv.weight_init``, a non-trivial bias / BatchNorm affine and running
    statistics, a cotangent at gradient scale."""
    x, w, _, _ = R.make_case(B, Cin, Cout, H, W, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return dict(x=x, w=w, b=(0.1 * rng.standard_normal(Cout)).astype(np.float32), gamma=rng.uniform(0.5, 1.5, Cout).astype(np.float32),
                beta=(0.3 * rng.standard_normal(Cout)).astype(np.float32), g=make_g(B, Cout, H, W, seed + 2),
                running=((0.1 * rng.standard_normal(Cout)).astype(np.float32), rng.uniform(0.5, 1.5, Cout).astype(np.float32)))


# (B, Cin, Cout, H, W) of the GPU tests' exact case; the last one puts a tile seam (128 columns) inside a row of its one cloud
# tests/golden/upconv_train (tools/make_upconv_train_golden.py): name -> (Cin, Cout, activation, normalization, B, H, W)
FIXTURES = {"upconv_16x32_3x5": (16, 32, "relu", "batch", 3, 3, 5), "upconv_40x32_1x1": (40, 32, None, None, 5, 1, 1)}

INT_SHAPES = ((2, 33, 32, 1, 1), (3, 16, 64, 2, 2), (3, 20, 32, 3, 5), (3, 40, 32, 8, 8), (1, 17, 32, 5, 30))


def int_case(shape):
    B, Cin, Cout, H, W = shape
    rng = np.random.default_rng(13 * Cin + H)
    return rng.integers(-2, 3, (B, Cout, 2 * H, 2 * W)).astype(np.float32), rng.integers(-3, 4, (Cout, Cin, 3, 3)).astype(np.float32)


def dgrad_gemm(g, w):
    """-> (Wg [Cin][16 Cout] f32: the transposed folded weights rounded to f32 as the pack does, Gg [16 Cout][B H W] f32: the shifted parity
    planes): the ONE GEMM of the input gradient, for the arithmetic model (tests/x3_model.py)."""
    g = np.asarray(g, np.float32)
    wf = R.fold_weights(w)
    B, Cout, H2, W2 = g.shape
    Ws, Gs = [], []
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx_ in range(2):
                    Ws.append(wf[py, px, dy, dx_].T)
                    Gs.append(R.shifted(g[:, :, py::2, px::2], 1 - py - dy, 1 - px - dx_).transpose(1, 0, 2, 3).reshape(Cout, -1))
    return np.concatenate(Ws, axis=1).astype(np.float32), np.ascontiguousarray(np.concatenate(Gs, axis=0))


def wgrad64(g_raw, x):
    """dW [Cout][Cin][3][3] of conv3x3_pad1 on the upsampled x, float64."""
    x = np.asarray(x, np.float64)
    up = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
    dW = np.zeros((g_raw.shape[1], x.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = np.einsum("bohw,bchw->oc", g_raw, R.shifted(up, ky - 1, kx - 1))
    return dW


def layer_train64(x, w, b, gamma, beta, eps, relu, mask=None, g=None, running=None, momentum=0.1):
    """One training step of the layer in float64.  gamma None: no normalization.  mask (0 / 1, the shape of y) replaces the layer's own
    ``pre > 0``.  running = (mean, var) before the step.  -> dict: y, pre, mask, raw and -- given the cotangent g -- g_raw, dx, dW, db,
    dgamma, dbeta; with BatchNorm also mean, var, running_mean, running_var."""
    x = np.asarray(x, np.float64)
    bc = lambda v: np.asarray(v, np.float64)[None, :, None, None]
    raw = R.conv_folded(x, w) + bc(b)
    out = dict(raw=raw)
    n = raw.shape[0] * raw.shape[2] * raw.shape[3]
    if gamma is not None:
        mean, var = raw.mean(axis=(0, 2, 3)), raw.var(axis=(0, 2, 3))
        invstd = 1.0 / np.sqrt(var + eps)
        xhat = (raw - bc(mean)) * bc(invstd)
        pre = xhat * bc(gamma) + bc(beta)
        out.update(mean=mean, var=var)
        if running is not None:
            out["running_mean"] = (1 - momentum) * np.asarray(running[0], np.float64) + momentum * mean
            out["running_var"] = (1 - momentum) * np.asarray(running[1], np.float64) + momentum * var * n / max(n - 1, 1)
    else:
        pre = raw
    if relu:
        mask = (pre > 0).astype(np.float64) if mask is None else np.asarray(mask, np.float64)
        y = pre * mask
    else:
        mask, y = np.ones_like(pre), pre
    out.update(y=y, pre=pre, mask=mask)
    if g is None:
        return out
    gp = np.asarray(g, np.float64) * mask
    if gamma is not None:
        dbeta, dgamma = gp.sum(axis=(0, 2, 3)), (gp * xhat).sum(axis=(0, 2, 3))
        g_raw = bc(np.asarray(gamma, np.float64) * invstd) * (gp - bc(dbeta) / n - xhat * bc(dgamma) / n)
        out.update(dgamma=dgamma, dbeta=dbeta)
    else:
        g_raw = gp
    out.update(g_raw=g_raw, dx=dgrad_folded(g_raw, w), dW=wgrad64(g_raw, x), db=g_raw.sum(axis=(0, 2, 3)))
    return out


def autograd64(x, w, b, gamma, beta, eps, relu, g, running=None, momentum=0.1):
    """The same step by float64 autograd of the reference's expression, relu(F.batch_norm(conv2d(interpolate(x)) ...)) -> dict."""
    t = lambda v: None if v is None else torch.tensor(np.asarray(v, np.float64), requires_grad=True)
    xt, wt, bt, gt, bet = t(x), t(w), t(b), t(gamma), t(beta)
    pre = F.conv2d(F.interpolate(xt, scale_factor=2), wt, bt, padding=1)
    out = {}
    if gamma is not None:
        rm = rv = None
        if running is not None:
            rm, rv = (torch.tensor(np.asarray(r, np.float64)) for r in running)
        pre = F.batch_norm(pre, rm, rv, gt, bet, True, momentum, eps)
        if running is not None:
            out.update(running_mean=rm.numpy(), running_var=rv.numpy())
    y = torch.relu(pre) if relu else pre
    y.backward(torch.tensor(np.asarray(g, np.float64)))
    out.update(y=y.detach().numpy(), pre=pre.detach().numpy(), dx=xt.grad.numpy(), dW=wt.grad.numpy(), db=bt.grad.numpy())
    if gamma is not None:
        out.update(dgamma=gt.grad.numpy(), dbeta=bet.grad.numpy())
    return out


# ---- the DecoderConv chain ------------------------------------------------------------------------------------------------------------
DECONVS = tuple("deconv%d" % i for i in range(1, 7))
HEADS = (4, 5, 6)
MASKED = DECONVS + tuple("conv2pc%d.conv1" % i for i in HEADS)        # the BatchNorm + ReLU layers, in forward order per branch


def decoder_train64(sd, feature, cots, masks=None, eps=1e-5):
    """DecoderConv ('relu', 'batch', training mode) in float64 autograd.  sd: state_dict-style mapping name -> array; feature [B][F];
    cots = {4: g_pc4, 5: g_pc5, 6: g_pc6}; masks = {layer name of MASKED: 0 / 1 array} forced in place of ``pre > 0`` (missing: the
    layer's own).  -> dict(pc={4, 5, 6}, pre={name: pre-activation}, mask={name: mask used}, grads={parameter name: gradient},
    dfeature, graw_abs={name: per-channel sum |gradient of the convolution's output|}: the unit of a bias gradient that is analytically zero
    behind its BatchNorm)."""
    P = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items()
         if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))}
    f = torch.tensor(np.asarray(feature, np.float64), requires_grad=True)
    pres, used, pcs, raws = {}, {}, {}, {}

    def bn_relu(pre, layer):                                   # layer: "deconv3" or "conv2pc4.conv1"
        pre.retain_grad()
        raws[layer] = pre
        pre = F.batch_norm(pre, None, None, P[layer + ".norm.weight" if layer.startswith("conv2pc") else layer + ".conv.norm.weight"],
                           P[layer + ".norm.bias" if layer.startswith("conv2pc") else layer + ".conv.norm.bias"], True, 0.1, eps)
        pres[layer] = pre.detach().numpy()
        m = (pre.detach() > 0).double() if masks is None or layer not in masks else torch.tensor(np.asarray(masks[layer], np.float64))
        used[layer] = m.numpy()
        return pre * m

    x = f.view(f.shape[0], -1, 1, 1)
    for i in range(1, 7):
        name = "deconv%d" % i
        x = bn_relu(F.conv2d(F.interpolate(x, scale_factor=2), P[name + ".conv.conv.weight"], P[name + ".conv.conv.bias"], padding=1), name)
        if i in HEADS:
            head = "conv2pc%d" % i
            h = bn_relu(F.conv2d(x, P[head + ".conv1.conv.weight"], P[head + ".conv1.conv.bias"]), head + ".conv1")
            pcs[i] = F.conv2d(h, P[head + ".conv2.conv.weight"], P[head + ".conv2.conv.bias"])
    loss = sum((pcs[i] * torch.tensor(np.asarray(cots[i], np.float64))).sum() for i in HEADS)
    loss.backward()
    return dict(pc={i: pcs[i].detach().numpy() for i in HEADS}, pre=pres, mask=used,
                grads={k: (v.grad.numpy() if v.grad is not None else None) for k, v in P.items()}, dfeature=f.grad.numpy(),
                graw_abs={k: v.grad.abs().sum(dim=(0, 2, 3)).numpy() for k, v in raws.items()})


def rel_rms(got, ref):
    """rms(got - ref) / rms(ref): the forced-routing gate of tests/test_gpu_parity.py."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-300))
