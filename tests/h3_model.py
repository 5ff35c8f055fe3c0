"""Host restatement of the fp16-split ("h3") arithmetic and of its operand-range guard, and the corner families of the admitted region.

The split, piece by piece as the kernels form it (float32 where they use float32, fp16 round-to-nearest-even incl. subnormals where they
convert), with every product and sum in float64: what comes out is the error of the ARITHMETIC alone, without the noise of the matrix
cores' f32 accumulation.

  second generation (csrc/pointmlp_x3.hip, split16_pair / split16_w; ops.pointmlp with an "h3" pack, the segment-pool epilogue):
      a = fp16(32 x), b = fp16(32 x - a), xh = fp16(a 2^-5), wh = fp16(w), wm = fp16(32 (w - wh));   W.x ~= (wh.a + wh.b + wm.xh) / 32
  third generation and the fused first PointNet (csrc/pointmlp_h3p.hip, csrc/pointresnet_fused.hip; X arrives as P16 planes):
      Xh = fp16(32 x), Xm = fp16(32 x - Xh), Wh = fp16(32 w), Wr = fp16(32 w - Wh);                  W.x ~= (Wr.Xh + Wh.Xm + Wh.Xh) / 1024

``admitted`` restates the guard (ops.range_scope.violations on the launch side, ops.h3_weight_ok on the weight side) from the constants of
sonet_hip/ops.py -- imported, not copied: a change of the guard moves the region these tests walk.
"""
import struct

import numpy as np

from sonet_hip import ops

FLAVOURS = ("h3", "h3p")
COUT, L = 64, 2048                     # two 32-row output tiles; 2048 columns (enough for the metric's maximum over elements to settle)
KS = (6, 64, 387, 768)                 # a K tail inside one chunk, whole chunks, two panels (3 + 384), the widest shipped layer


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


X_HIGH, X_LOW = _f(ops._B_2047), _f(ops._B_XLOW)
W_LOW = _f(ops._B_WLOW)
assert _f(ops._B_WLOW32) == 32.0 * W_LOW          # the fused kernel logs 32 |w|: the same limit as the third generation's


def w_high(flavour):
    """Largest |w| the launch guard admits: fp16(w) must be finite (second generation), fp16(32 w) must be (third generation, fused)."""
    return _f(ops._B_65504) if flavour == "h3" else _f(ops._B_65504) / 32.0


assert w_high("h3p") == X_HIGH                     # ... which violations() writes as _B_2047


def f16(v):
    """float32 array -> its fp16 rounding, returned as float32 (exact)."""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)


def split_x(x):
    """-> (Xh, Xm) = fp16(32 x), fp16(32 x - Xh) of the clamped x: the P16 planes, and the second generation's a, b."""
    X = np.float32(32.0) * np.clip(np.asarray(x, dtype=np.float32), np.float32(-2047.0), np.float32(2047.0))
    hi = f16(X)
    return hi, f16(X - hi)


def model(x, W, flavour):
    """The arithmetic's result for W [Cout][K] . x [K][L] (float32 operands) -> float64 [Cout][L]."""
    W = np.asarray(W, dtype=np.float32)
    hi, mid = split_x(x)
    if flavour == "h3":
        xh = (hi.astype(np.float16) * np.float16(2.0 ** -5)).astype(np.float64)      # an fp16 multiply: rounds where it lands in the subnormals
        wc = np.clip(W, np.float32(-65504.0), np.float32(65504.0))
        wh = f16(wc)
        wm = f16(np.float32(32.0) * (wc - wh))
        return (wh.astype(np.float64) @ (hi.astype(np.float64) + mid.astype(np.float64)) + wm.astype(np.float64) @ xh) / 32.0      # (hi + mid: exact in f64)
    if flavour == "h3p":
        W32 = np.float32(32.0) * W
        Wh = f16(W32)
        Wr = f16(W32 - Wh).astype(np.float64)
        hi = hi.astype(np.float64)
        return (Wr @ hi + Wh.astype(np.float64) @ (hi + mid.astype(np.float64))) / 1024.0
    raise ValueError(flavour)


def exact(x, W):
    return np.asarray(W, dtype=np.float64) @ np.asarray(x, dtype=np.float64)


def rms_error(got, ref):
    """max |got - ref| / max(|ref|, rms(ref)): the figure conftest.assert_close_rms bounds."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    return float((np.abs(got - ref) / np.maximum(np.maximum(np.abs(ref), rms), 1e-300)).max())


def column_ratio(W):
    """max over input columns of max|w[:, c]| / the smallest non-zero one: the quantity ops.h3_weight_ratio_flag tests."""
    cm = np.abs(np.asarray(W, dtype=np.float32)).max(axis=0)
    big = cm.max()
    small = np.where(cm > 0, cm, big).min()
    return float(big) / float(small) if small > 0 else 1.0


def ratio_limit(K):
    """Largest column ratio the weight-side guard admits for a layer of K input channels."""
    return float(ops.h3_column_ratio_limit(K))


def weights_admitted(W):
    W = np.asarray(W, dtype=np.float32)
    cm = np.abs(W).max(axis=0)
    big = cm.max()
    small = np.where(cm > 0, cm, big).min()
    if big == 0:
        return True
    # the comparisons of h3_weight_ratio_flag, in f32
    return bool(np.float32(big) <= np.float32(small) * np.float32(ratio_limit(W.shape[1]))) and bool(small >= np.float32(ops.H3_COLUMN_MIN))


def admitted(x, W, flavour):
    """Would the guard let this (x [K][L], W [Cout][K]) pair run on the fp16 split?"""
    mx = float(np.abs(np.asarray(x, dtype=np.float32)).max())
    mw = float(np.abs(np.asarray(W, dtype=np.float32)).max())
    if not (np.isfinite(mx) and np.isfinite(mw)):
        return False
    if mx > X_HIGH or 0 < mx < X_LOW:
        return False
    if mw > w_high(flavour) or 0 < mw < W_LOW:
        return False
    return weights_admitted(W)


# ---- corner families ---------------------------------------------------------------------------------------------------------------
X_MAX = {"xlow": X_LOW, "x1": 1.0, "x2047": X_HIGH}
FRACTIONS = {"f0": 1.0, "f4": 2.0 ** -4, "f8": 2.0 ** -8, "f12": 2.0 ** -12}          # f<n>: the remaining channels at 2^-n of max |x|
COUNTS = ("one", "allbut1")
RATIOS = ("r1", "r16", "rmax")
W_MAX = ("wlow", "w0.1", "whigh")


_BASES = {}


def _unit_rows(tag, n, m):
    """n x m normal draws, every row rescaled so that its largest magnitude is exactly 1 (float32); one draw per (tag, n, m), kept."""
    key = (tag, n, m)
    if key not in _BASES:
        a = np.random.default_rng(_seed(*key)).standard_normal((n, m))
        a = np.clip((a / np.abs(a).max(axis=1, keepdims=True)).astype(np.float32), np.float32(-1), np.float32(1))
        at = np.abs(a).argmax(axis=1)
        a[np.arange(n), at] = np.sign(a[np.arange(n), at])
        a.setflags(write=False)
        _BASES[key] = a
    return _BASES[key]


def _scaled_rows(base, target):
    """base (rows with maximum 1) times the per-row float32 ``target``, no element beyond its row's target."""
    t = np.asarray(target, dtype=np.float32).reshape(-1, 1)
    return np.clip(base * t, -t, t)


def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def make_case(K, xmax, frac, count, ratio, wmax, seed=0):
    """One corner of the admitted region -> (x [K][L] f32, W [COUT][K] f32).

    Channel 0 carries max |x| = xmax.  The "remaining" channels -- one of them, or all but channel 0 -- have their maximum at frac * xmax;
    any channel left over sits at xmax like channel 0.  The weight columns of the remaining channels are the LARGE ones (max |w| = wmax),
    the others are ``ratio`` times smaller: the weights make up for the small channels, the arrangement h3_weight_ok is about.
    Every row of x and every column of W is a normal draw rescaled to its maximum (peak-to-rms about 3.5)."""
    small = np.zeros(K, dtype=bool)
    if count == "one":
        small[K - 1] = True                                   # the last channel: inside the K tail / the narrow second panel
    else:
        small[1:] = True
    x = _scaled_rows(_unit_rows("x%d" % seed, K, L), np.where(small, np.float32(xmax) * np.float32(frac), np.float32(xmax)))
    W = _scaled_rows(_unit_rows("w%d" % seed, K, COUT), np.where(small, np.float32(wmax), np.float32(wmax) / np.float32(ratio)))
    return np.ascontiguousarray(x), np.ascontiguousarray(W.T)


def axis_values(K, flavour):
    """The table of the corner families for one K and flavour: name -> value, per axis."""
    rmax = ratio_limit(K)
    return {"xmax": dict(X_MAX), "frac": dict(FRACTIONS), "count": {c: c for c in COUNTS},
            "ratio": {"r1": 1.0, "r16": min(16.0, rmax), "rmax": rmax},           # (16 where the limit for this K is below 16: the limit)
            "wmax": {"wlow": None, "w0.1": 0.1, "whigh": w_high(flavour)}}


def w_low(ratio):
    """The smallest max |w| the guard admits at a column ratio: the launch log's threshold, and no column below H3_COLUMN_MIN."""
    return float(max(np.float32(W_LOW), np.float32(ops.H3_COLUMN_MIN) * np.float32(ratio) * np.float32(1.0 + 2.0 ** -20)))


def corner_cases(K, flavour, xmax_names=None):
    """Yield (name, x, W) for every corner family of one K: 3 x 4 x 2 x 3 x 3 = 216 cases (144 where the ratio limit is <= 16), deterministic."""
    ax = axis_values(K, flavour)
    for xn, xm in ax["xmax"].items():
        if xmax_names is not None and xn not in xmax_names:
            continue
        for fn, fr in ax["frac"].items():
            for cn in COUNTS:
                for rn, r in ax["ratio"].items():
                    if rn == "r16" and r == ax["ratio"]["rmax"]:
                        continue                              # the limit for this K is 16 or less: "r16" would repeat "rmax"
                    for wn, wm in ax["wmax"].items():
                        x, W = make_case(K, xm, fr, cn, r, w_low(r) if wm is None else max(wm, w_low(r)))
                        yield "K%d-%s-%s-%s-%s-%s" % (K, xn, fn, cn, rn, wn), x, W


def family_of(name):
    """Cases that differ only in K, max |w| and max |x| share a family (fraction, count, ratio): the rows of the envelope table."""
    p = name.split("-")
    return "-".join(p[2:5]) if len(p) >= 6 else name


def plain_case(K, seed=0, scale=1.0):
    """The middle of the region: normal activations, He-scaled normal weights (what every other accuracy test feeds)."""
    rng = np.random.default_rng(_seed("plain", K, seed))
    x = (rng.standard_normal((K, L)) * scale).astype(np.float32)
    W = (rng.standard_normal((COUT, K)) * (2.0 / K) ** 0.5).astype(np.float32)
    return x, W


def outside_cases(K, flavour):
    """Just outside the region: max |x| one float below the lower threshold; the column ratio one float above its limit."""
    ax = axis_values(K, flavour)
    below = float(np.nextafter(np.float32(X_LOW), np.float32(0)))
    x, W = make_case(K, below, 2.0 ** -8, "allbut1", 1.0, 0.1)
    yield "K%d-x_below_low" % K, "x", x, W
    over = float(np.nextafter(np.float32(ax["ratio"]["rmax"]), np.float32(np.inf))) * (1.0 + 2.0 ** -20)
    x, W = make_case(K, 1.0, 2.0 ** -8, "allbut1", over, max(0.1, w_low(over)))
    yield "K%d-ratio_above_max" % K, "w", x, W
