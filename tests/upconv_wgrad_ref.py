"""Float64 restatements of the up-convolution's weight gradient in the folded form the kernel computes (sonet_upconv3x3_wgrad_f32):

    dWf[py][px][dy][dx'][o][c] = sum over b, i, j of  g[b][o][2i + py][2j + px] * shifted(x, py + dy - 1, px + dx' - 1)[b][c][i][j]
    dW[o][c][ky][kx]           = sum of dWf[py][px][dy][dx'] over the (py, dy) with ky in FOLD[py][dy] and the (px, dx') with kx in FOLD[px][dx']

``wgrad_folded`` is that form (with the BREAKS a kernel of this form can make), ``plan`` the kernel's column slices (a function of the
shape alone), ``wgrad_gemm`` the one GEMM the sixteen products and the unfold amount to, ``wgrad_model`` the bf16-split arithmetic
(tests/x3_model.py) chained as the kernel chains it, ``int_case`` operands on which the kernel must equal float64 bit for bit.
"""
import numpy as np

import upconv_ref as R
import upconv_train_ref as T
import x3_model

BREAKS = ("shift_sign", "parity_dropped", "unfold_transposed", "seam", "last_slice_dropped")

# include/sonet_hip.h SONET_UPWGRAD_*
K_STEP, CIN_BLOCK, FLUSH_COLS, SLICE_COLS, MAX_SLICES, WS_CAP = 16, 32, 256, 512, 128, 64 << 20


def plan(B, Cin, Cout, H, W):
    """-> (number of slices, columns per slice, workspace bytes) as uw_plan of csrc/upconv_wgrad.hip."""
    ncols = B * H * W
    nstep = -(-ncols // K_STEP)
    per = 16 * Cout * (-(-Cin // CIN_BLOCK) * CIN_BLOCK) * 4
    want = max(1, min(-(-ncols // SLICE_COLS), MAX_SLICES, WS_CAP // per))
    sps = -(-nstep // want)
    nslice = -(-nstep // sps)
    return nslice, sps * K_STEP, nslice * per


def _flat(a):
    """[B][C][H][W] -> [C][B H W], the kernel's flat column axis."""
    return np.ascontiguousarray(a.transpose(1, 0, 2, 3).reshape(a.shape[1], -1))


def pairs():
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    yield py, px, dy, dx


def unfold(dwf, fold=R.FOLD):
    """dWf [py][px][dy][dx][Cout][Cin] -> dW [Cout][Cin][3][3]: the transpose of ``upconv_ref.fold_weights``."""
    dW = np.zeros(dwf.shape[4:] + (3, 3), dwf.dtype)
    for py, px, dy, dx in pairs():
        for ky in fold[py][dy]:
            for kx in fold[px][dx]:
                dW[:, :, ky, kx] += dwf[py, px, dy, dx]
    return dW


def wgrad_folded(g, x, brk=None):
    """g [B][Cout][2H][2W], x [B][Cin][H][W] -> dW [Cout][Cin][3][3] float64, the folded form (``brk``: one of BREAKS)."""
    assert brk is None or brk in BREAKS
    g, x = np.asarray(g, np.float64), np.asarray(x, np.float64)
    B, Cout, H2, W2 = g.shape
    Cin, H, W = x.shape[1], H2 // 2, W2 // 2
    keep = B * H * W
    if brk == "last_slice_dropped":
        nslice, cols, _ = plan(B, Cin, Cout, H, W)
        keep = (nslice - 1) * cols
    dwf = np.zeros((2, 2, 2, 2, Cout, Cin))
    for py, px, dy, dx in pairs():
        if brk == "parity_dropped" and (py, px) == (1, 1):
            continue
        sy, sx = py + dy - 1, px + dx - 1
        if brk == "shift_sign":
            sx = -sx
        src = T._rolled(x, sy, sx) if brk == "seam" else R.shifted(x, sy, sx)
        dwf[py, px, dy, dx] = _flat(g[:, :, py::2, px::2])[:, :keep] @ _flat(src)[:, :keep].T
    return unfold(dwf, T.FOLD_T if brk == "unfold_transposed" else R.FOLD)


def wgrad_gemm(g, x):
    """-> (Gg [Cout][16 K] f32, Xg [16 K][9 Cin] f32), K = B H W: the ONE GEMM dW[o][(c, ky, kx)] = Gg . Xg -- the sixteen parity planes of g
    side by side against the sixteen shifted copies of x, each placed in the (ky, kx) columns its pair unfolds into."""
    g, x = np.asarray(g, np.float32), np.asarray(x, np.float32)
    Cin = x.shape[1]
    Gs, Xs = [], []
    for py, px, dy, dx in pairs():
        Gs.append(_flat(g[:, :, py::2, px::2]))
        xs = _flat(R.shifted(x, py + dy - 1, px + dx - 1)).T                   # [K][Cin]
        blk = np.zeros((xs.shape[0], Cin, 3, 3), np.float32)
        for ky in R.FOLD[py][dy]:
            for kx in R.FOLD[px][dx]:
                blk[:, :, ky, kx] = xs
        Xs.append(blk.reshape(xs.shape[0], Cin * 9))
    return np.concatenate(Gs, axis=1), np.concatenate(Xs, axis=0)


def wgrad_model(g, x, flush=False):
    """The bf16-split arithmetic chained as the kernel chains it: per (parity, tap) pair and slice, chains of FLUSH_COLS products (the six
    piece products in float64, rounded to f32 once per chain), the chains of a slice added in f32, the slices and the four-term unfold in
    float64, one rounding -> dW as float64."""
    g, x = np.asarray(g, np.float32), np.asarray(x, np.float32)
    B, Cout, H2, W2 = g.shape
    Cin, H, W = x.shape[1], H2 // 2, W2 // 2
    K = B * H * W
    nslice, cols, _ = plan(B, Cin, Cout, H, W)
    dwf = np.zeros((2, 2, 2, 2, Cout, Cin))
    for py, px, dy, dx in pairs():
        Gp = x3_model.split3(_flat(g[:, :, py::2, px::2]), flush)
        Xp = x3_model.split3(_flat(R.shifted(x, py + dy - 1, px + dx - 1)).T, flush)
        for s in range(nslice):
            tot = np.zeros((Cout, Cin), np.float32)
            for k0 in range(s * cols, min(K, (s + 1) * cols), FLUSH_COLS):
                k1 = min(k0 + FLUSH_COLS, K, (s + 1) * cols)
                acc = x3_model._sum_terms([p[:, k0:k1] for p in Gp], [p[k0:k1] for p in Xp], x3_model.TERMS)
                tot = tot + acc.astype(np.float32)
            dwf[py, px, dy, dx] += tot.astype(np.float64)
    return unfold(dwf).astype(np.float32).astype(np.float64)


def make_case(B, Cin, Cout, H, W, seed, scale=1.0):
    """Seeded operands: x of order 1 (``upconv_ref.make_case``), g at gradient scale (``upconv_train_ref.make_g``) times ``scale``."""
    x = R.make_case(B, Cin, Cout, H, W, seed=seed)[0]
    return T.make_g(B, Cout, H, W, seed + 1, scale), x


def int_case(shape):
    """(B, Cin, Cout, H, W) -> integer g in [-2, 2] and x in [-3, 3].  Each value is a bf16 number: its h piece is the value, m and l are
    zero, so of the six products five are zero and one is the integer g x.  Every partial sum of an accumulator -- in any order -- is an
    integer of magnitude at most sum |g| |x| < 2^24: exact in f32.  The slices are then added in float64 and the four folded gradients of
    a tap as well: integers below 2^24 again, so the one rounding to f32 changes nothing.  The kernel's dW must EQUAL the float64 one."""
    B, Cin, Cout, H, W = shape
    rng = np.random.default_rng(17 * Cin + 3 * H + B)
    g = rng.integers(-2, 3, (B, Cout, 2 * H, 2 * W)).astype(np.float32)
    x = rng.integers(-3, 4, (B, Cin, H, W)).astype(np.float32)
    for v in (g, x):
        h, m, l = x3_model.split3(v)
        assert np.array_equal(h, v) and not m.any() and not l.any()
    assert float(wgrad_folded(np.abs(g), np.abs(x)).max()) < 2 ** 24           # sum |terms| of the worst tap
    return g, x
