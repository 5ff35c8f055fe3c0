"""Float64 restatements of the decoder's up-convolution layer (UpConv, models/layers.py:214-240 of the reference):

    y = act(conv3x3_pad1(upsample2_nearest(x), w) * scale + shift)

``reference`` is the expression as the reference writes it (F.interpolate + F.conv2d, in float64); ``folded`` is the four-parity form the
kernel computes: output pixel (2i + py, 2j + px) reads the LOW-resolution pixels (i - 1 + py + dy, j - 1 + px + dx), dy, dx in {0, 1},
zeros outside the map, with the weights of FOLD below.  ``fold_weights`` returns those sixteen (parity, tap) matrices; ``parity_gemm``
lays the folded form out as the four GEMMs (Cout x 4 Cin) . (4 Cin x B H W) the arithmetic model is applied to.
"""
import numpy as np
import torch
import torch.nn.functional as F

# FOLD[parity][tap] = the ky (kx) indices whose weights the tap sums
FOLD = (((0,), (1, 2)), ((0, 1), (2,)))
SHAPES = ((1, 1), (1, 2), (2, 2), (3, 5), (8, 8), (32, 32))


def make_case(B, Cin, Cout, H, W, seed, affine=True):
    """Seeded decoder-scaled operands: activations of order 1, weights of standard deviation sqrt(2 / (9 Cout)) (UpConv.weight_init),
    a non-trivial per-channel affine (scale in [0.5, 1.5] with both signs, shift of order 0.3)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cout))).astype(np.float32)
    if affine:
        scale = (rng.uniform(0.5, 1.5, Cout) * np.where(rng.random(Cout) < 0.25, -1.0, 1.0)).astype(np.float32)
        shift = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    else:
        scale, shift = np.ones(Cout, np.float32), np.zeros(Cout, np.float32)
    return x, w, scale, shift


def _finish(y, scale, shift, relu):
    y = y * np.asarray(scale, np.float64)[None, :, None, None] + np.asarray(shift, np.float64)[None, :, None, None]
    return np.maximum(y, 0.0) if relu else y


def reference(x, w, scale, shift, relu):
    """The reference's expression in float64 -> [B][Cout][2H][2W]."""
    xt = torch.from_numpy(np.asarray(x, np.float64))
    wt = torch.from_numpy(np.asarray(w, np.float64))
    up = F.interpolate(xt, scale_factor=2)                     # nn.Upsample's default mode: nearest
    return _finish(F.conv2d(up, wt, padding=1).numpy(), scale, shift, relu)


def fold_weights(w, fold=FOLD):
    """w [Cout][Cin][3][3] -> wf [py][px][dy][dx][Cout][Cin] float64."""
    w = np.asarray(w, np.float64)
    wf = np.zeros((2, 2, 2, 2) + w.shape[:2])
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    for ky in fold[py][dy]:
                        for kx in fold[px][dx]:
                            wf[py, px, dy, dx] += w[:, :, ky, kx]
    return wf


def shifted(x, sy, sx):
    """x [B][C][H][W] -> the map read at (i + sy, j + sx), zeros outside."""
    B, C, H, W = x.shape
    p = np.zeros((B, C, H + 2, W + 2), x.dtype)
    p[:, :, 1:H + 1, 1:W + 1] = x
    return p[:, :, 1 + sy:1 + sy + H, 1 + sx:1 + sx + W]


def conv_folded(x, w, fold=FOLD):
    """The four-parity form without the affine -> [B][Cout][2H][2W] float64."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    wf = fold_weights(w, fold)
    y = np.zeros((B, wf.shape[4], 2 * H, 2 * W))
    for py in range(2):
        for px in range(2):
            acc = 0.0
            for dy in range(2):
                for dx in range(2):
                    acc = acc + np.einsum("oc,bchw->bohw", wf[py, px, dy, dx], shifted(x, py + dy - 1, px + dx - 1))
            y[:, :, py::2, px::2] = acc
    return y


def folded(x, w, scale, shift, relu, fold=FOLD):
    return _finish(conv_folded(x, w, fold), scale, shift, relu)


def parity_gemm(x, w, py, px):
    """-> (Wg [Cout][4 Cin] f32: the folded weights rounded to f32 as the pack does, Xg [4 Cin][B H W] f32) of one output parity."""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    wf = fold_weights(w)
    Wg = np.concatenate([wf[py, px, dy, dx] for dy in range(2) for dx in range(2)], axis=1).astype(np.float32)
    Xg = np.concatenate([shifted(x, py + dy - 1, px + dx - 1).transpose(1, 0, 2, 3).reshape(C, -1) for dy in range(2) for dx in range(2)], axis=0)
    return Wg, np.ascontiguousarray(Xg)


def eval_affine(g, Cout):
    """(scale, shift) in float64 of a tests/golden/upconv UpConv fixture: the conv bias and, when the fixture has them, the eval-mode
    BatchNorm buffers (eps 1e-5) folded as the layer folds them."""
    b = g["conv__conv__bias"].astype(np.float64)
    if "conv__norm__weight" not in g.files:
        return np.ones(Cout), b
    scale = g["conv__norm__weight"].astype(np.float64) / np.sqrt(g["conv__norm__running_var"].astype(np.float64) + 1e-5)
    return scale, (b - g["conv__norm__running_mean"].astype(np.float64)) * scale + g["conv__norm__bias"].astype(np.float64)


def rms_error(got, ref):
    """max |got - ref| / max(|ref|, rms(ref)): the figure conftest.assert_close_rms bounds."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    return float((np.abs(got - ref) / np.maximum(np.maximum(np.abs(ref), rms), 1e-300)).max())
