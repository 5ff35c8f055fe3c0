"""numpy float64 restatement of the cross-entropy contract (include/sonet_hip.h: sonet_ce_loss_f32 / sonet_ce_grad_f32), written from that
contract: the checker of tests/test_ce_loss_cpu.py, tests/test_gpu_ce_loss.py and tools/make_ce_golden.py.

Also the seeded input makers those share, the deliberate breaks of the restatement (``BREAKS``: each must turn the test meant for it red)
and the derived error bound of the gradient (``grad_bound``)."""
import numpy as np

from seg_metrics_ref import argmax_rule

BREAKS = ("no_onehot", "denominator_minus_one", "skip_last_class", "lse_without_max", "count_bad_target")


def as3(score, target):
    """B x C (+ B) or B x C x N (+ B x N) -> B x C x N float32-valued float64 scores, B x N int64 targets."""
    score, target = np.asarray(score), np.asarray(target, dtype=np.int64)
    if score.ndim == 2:
        score, target = score[:, :, None], target[:, None]
    assert score.ndim == 3 and target.shape == (score.shape[0], score.shape[2]), (score.shape, target.shape)
    return score, target


def ce_terms(score, target, brk=None):
    """Everything the forward entry returns: dict of lse, nll [B][N] f64 (nll 0 at a bad target), nll_sum [B] f64, pred [B][N] i64,
    correct, bad [B] i64, confusion [C][C] i64.  brk: one of BREAKS (a deliberately wrong restatement) or None."""
    assert brk is None or brk in BREAKS, brk
    s3, target = as3(score, target)
    B, C, N = s3.shape
    x = s3.astype(np.float64)
    xs = x[:, :C - 1] if (brk == "skip_last_class" and C > 1) else x
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.zeros((B, N)) if brk == "lse_without_max" else xs.max(axis=1)
        logS = np.log(np.exp(xs - m[:, None, :]).sum(axis=1))
        lse = m + logS
    ok = (target >= 0) & (target < C)
    t = np.where(ok, target, 0)
    with np.errstate(invalid="ignore"):
        # the contract's two non-negative terms: lse - x_t would lose a confident point's relative precision to cancellation
        nll = (m - np.take_along_axis(x, t[:, None, :], 1)[:, 0, :]) + logS
    if brk != "count_bad_target":
        nll = np.where(ok, nll, 0.0)
    pred = argmax_rule(s3)
    hit = ok & (pred == target)
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (target[ok], pred[ok]), 1)
    return dict(lse=lse, nll=nll, nll_sum=nll.sum(axis=1), pred=pred, correct=hit.sum(axis=1).astype(np.int64),
                bad=(~ok).sum(axis=1).astype(np.int64), confusion=confusion, ok=ok)


def ce_loss(score, target, reduction="mean", brk=None):
    """The float64 loss: sum of nll over all B N points, divided by B N for the mean (bad targets add 0, the denominator stays)."""
    r = ce_terms(score, target, brk)
    B, N = r["nll"].shape
    den = (B * N - 1 if brk == "denominator_minus_one" else B * N) if reduction == "mean" else 1
    return r["nll_sum"].sum() / den


def ce_grad(score, target, reduction="mean", gout=1.0, brk=None):
    """float64 d(gout * loss) / d score, score's shape: (exp(x - lse) - onehot) * gout * scale; zeros at a bad target."""
    s3, t3 = as3(score, target)
    r = ce_terms(score, target, brk)
    B, C, N = s3.shape
    den = (B * N - 1 if brk == "denominator_minus_one" else B * N) if reduction == "mean" else 1
    scale = 1.0 / den
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp(s3.astype(np.float64) - r["lse"][:, None, :])
    onehot = np.zeros((B, C, N))
    if brk != "no_onehot":
        b, n = np.nonzero(r["ok"])
        onehot[b, t3[b, n], n] = 1.0
    g = (p - onehot) * float(gout) * scale
    g = np.where(r["ok"][:, None, :], g, 0.0)
    return g.reshape(np.asarray(score).shape)


# ------------------------------------------------------------------------------------------------------------ derived bounds
def ulp_f32(v):
    """The spacing of float32 at |v| (float64 array): 2^(e - 23) with e = floor(log2 |v|) clamped to the normal range, 2^-149 below it."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -126.0) - 23.0)


def grad_K(C, xmax):
    """K of ``grad_bound``, counted from the kernel's chain of float64 roundings for p = exp(x - lse), in units of 2^-53 relative to p <= 1:

      S = sum of C terms exp(x - m)      each term: the difference, the exp (<= 1 ulp = 2 units); C - 1 additions; when the running maximum
                                         moves (at most C - 1 times) a product and an addition more  ->  at most 5 C units relative to S
      log(S)                             an absolute error of S's relative one, plus the log's own ulp of log(S) <= ln C  ->  5 C + ln C
      lse = m + log(S)                   one rounding of |lse| <= xmax + ln C                                             ->  xmax + ln C
      x - lse                            one rounding of |log p|; times p: p |log p| <= 1 / e                             ->  1
      exp(x - lse)                       <= 1 ulp                                                                          ->  2
      (p - onehot) * gout * scale        three roundings relative to |g| <= |gout| scale                                   ->  3

    K_kernel = 5 C + 2 ln C + xmax + 6.  The restatement walks the same chain in numpy's float64 (its pairwise sum is no worse than the
    sequential one), so the distance between the two is bounded by twice that."""
    return 2.0 * (5.0 * C + 2.0 * np.log(max(C, 1)) + float(xmax) + 6.0)


def grad_bound(g64, C, xmax, gout, scale):
    """|g - g64| <= ulp_f32(g64) + K 2^-53 |gout| scale: the one float32 rounding (half an ulp of the rounded value, which may sit one
    binade above g64: a whole ulp of g64's) plus the float64 chain."""
    return ulp_f32(g64) + grad_K(C, xmax) * 2.0 ** -53 * abs(float(gout)) * float(scale)


def f32_ulp_distance(a, b):
    """|a - b| in float32 ulps of b (both rounded to float32 first)."""
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(ulp_f32(float(b)))


# ------------------------------------------------------------------------------------------------------------ seeded inputs
def make_inputs(g, B, C, N=None, sigma=4.0, bump=3.0):
    """Seeded scores (sigma * normal, a bump on the target class) and targets: B x C x N / B x N, or B x C / B with N = None."""
    n = 1 if N is None else N
    score = (sigma * g.standard_normal((B, C, n))).astype(np.float32)
    target = g.randint(0, C, (B, n)).astype(np.int64)
    b, k = np.meshgrid(np.arange(B), np.arange(n), indexing="ij")
    score[b, target, k] += np.float32(bump)
    if N is None:
        return score[:, :, 0].copy(), target[:, 0].copy()
    return score, target


def exact_family(B, C, N, g):
    """Every score of a point equal (one seeded value per point, multiples of 1/4 in [-8, 8]), any targets.  With C and B N powers of two:
    m = x, every exp(x - m) = exp(0) = 1 exactly, S = C exactly; lse = x + log(C) is rounded (relative error d <= 2^-52 of a value
    below 16), so p = exp(x - lse) = (1 / C)(1 + e) with |e| <= 2^-47: p * gout * scale rounds to the float32 1 / (C B N) -- representable,
    and e is far below float32's 2^-25 -- and (p - 1) = -(C - 1) / C (1 - e / (C - 1)) rounds to the representable -(C - 1) / (C B N)
    (C = 1: log(1) = 0, exp(0) = 1, p - 1 = 0 exactly).  The gradient is exactly (1 / C - onehot) / (B N); the arg-max is class 0, the
    first of C equal maxima."""
    assert C & (C - 1) == 0 and (B * N) & (B * N - 1) == 0
    v = (g.randint(-32, 33, (B, 1, N)) / 4.0).astype(np.float32)
    score = np.repeat(v, C, axis=1)
    target = g.randint(0, C, (B, N)).astype(np.int64)
    onehot = np.zeros((B, C, N))
    b, n = np.meshgrid(np.arange(B), np.arange(N), indexing="ij")
    onehot[b, target, n] = 1.0
    grad = ((1.0 / C - onehot) / (B * N)).astype(np.float32)
    assert np.array_equal(grad.astype(np.float64), (1.0 / C - onehot) / (B * N))          # representable: nothing was rounded
    return score, target, grad


def cls_epoch(scores, labels):
    """The arithmetic of modelnet/train.py:70-90 over batches of B x C scores, accumulated in float64: dict of test_loss,
    test_accuracy, class_accuracy, confusion, count."""
    loss = correct = count = 0
    confusion = None
    for s, l in zip(scores, labels):
        r = ce_terms(s, l)
        loss += r["nll_sum"].sum()
        correct += int(r["correct"].sum())
        count += len(l)
        confusion = r["confusion"] if confusion is None else confusion + r["confusion"]
    per_class = confusion.sum(axis=1)
    seen = per_class > 0
    return dict(test_loss=loss / count, test_accuracy=correct / count, confusion=confusion, count=count,
                class_accuracy=float((confusion.diagonal()[seen] / per_class[seen]).mean()))
