"""numpy float64 restatement of the segmentation-metrics contract (include/sonet_hip.h: sonet_seg_metrics_f32), written from that
contract: the checker of tests/test_seg_metrics_cpu.py, tests/test_gpu_seg_metrics.py and tools/bench_seg_metrics.py.

Also the seeded input families the fixtures (tools/make_seg_metrics_golden.py) and the edge-shape tests share: labels drawn inside
the cloud's category, scores a bump on the true part plus noise -- so that the IoUs are neither 0 nor 1."""
import numpy as np

SHAPENET_PART_OFFSETS = (0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47, 50)


def argmax_rule(score):
    """score B x C x N -> B x N int64: the first of equal maxima wins, a NaN beats every number, the first NaN wins."""
    score = np.asarray(score)
    best = score[:, 0].copy()
    idx = np.zeros(best.shape, dtype=np.int64)
    for c in range(1, score.shape[1]):
        x = score[:, c]
        with np.errstate(invalid="ignore"):
            take = (x > best) | (np.isnan(x) & ~np.isnan(best))
        best = np.where(take, x, best)
        idx = np.where(take, c, idx)
    return idx


def seg_metrics(score, seg, label, part_offsets=SHAPENET_PART_OFFSETS):
    """Everything the entry point returns, per cloud: dict of pred [B][N] i64, correct [B] i64, nll_sum [B] f64, inter / pred_cnt /
    gt_cnt [B][C] i64, iou [B] f64, bad [B] i64."""
    score, seg, label = np.asarray(score), np.asarray(seg, dtype=np.int64), np.asarray(label, dtype=np.int64)
    B, C, N = score.shape
    off = [int(v) for v in part_offsets]
    n_cat = len(off) - 1
    pred = argmax_rule(score)
    x = score.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=1)
        lse = m + np.log(np.exp(x - m[:, None, :]).sum(axis=1))
    seg_ok = (seg >= 0) & (seg < C)
    target = np.where(seg_ok, seg, 0)
    with np.errstate(invalid="ignore"):
        nll = lse - np.take_along_axis(x, target[:, None, :], 1)[:, 0, :]
    out = dict(pred=pred, correct=np.zeros(B, np.int64), nll_sum=np.zeros(B), inter=np.zeros((B, C), np.int64),
               pred_cnt=np.zeros((B, C), np.int64), gt_cnt=np.zeros((B, C), np.int64), iou=np.zeros(B), bad=np.zeros(B, np.int64))
    for b in range(B):
        hit = seg_ok[b] & (pred[b] == seg[b])
        out["correct"][b] = hit.sum()
        out["pred_cnt"][b] = np.bincount(pred[b], minlength=C)
        out["gt_cnt"][b] = np.bincount(seg[b][seg_ok[b]], minlength=C)
        out["inter"][b] = np.bincount(pred[b][hit], minlength=C)
        out["bad"][b] = (~seg_ok[b]).sum()
        if 0 <= label[b] < n_cat:
            # sequential sum / number of parts: what numpy's mean does for fewer than 8 values (every ShapeNet category; a longer
            # array it adds pairwise -- the contract stays sequential there)
            total, parts = 0.0, range(off[label[b]], off[label[b] + 1])
            for p in parts:
                inter = int(out["inter"][b, p])
                union = int(out["pred_cnt"][b, p]) + int(out["gt_cnt"][b, p]) - inter
                total += 1.0 if union == 0 else inter / (union + 0.0001)
            out["iou"][b] = total / len(parts)
        else:
            out["bad"][b] += 1
            out["iou"][b] = np.nan
        out["nll_sum"][b] = np.nan if out["bad"][b] else nll[b][seg_ok[b]].sum()
    return out


def batch_report(score, seg, label, part_offsets=SHAPENET_PART_OFFSETS):
    """What the reference's test loop takes from one batch (part-seg/train.py:87-96): (mean loss f64, accuracy, mean IoU, per-cloud IoU)."""
    r = seg_metrics(score, seg, label, part_offsets)
    B, _, N = np.asarray(score).shape
    return r["nll_sum"].sum() / (B * N), r["correct"].sum() / (B * N), r["iou"].mean(), r["iou"]


class Accumulator:
    """The reference's epoch accumulation (part-seg/train.py:75-104): batch means weighted with the batch size, divided by the cloud count."""

    def __init__(self):
        self.loss = self.acc = self.iou = 0.0
        self.count = 0

    def add(self, loss, acc, iou, B):
        self.loss += loss * B
        self.acc += acc * B
        self.iou += iou * B
        self.count += B

    def result(self):
        return dict(test_loss_seg=self.loss / self.count, test_acc_seg=self.acc / self.count, test_iou=self.iou / self.count,
                    count=self.count)


# ------------------------------------------------------------------------------------------------------------ seeded inputs
def two_category_table(C):
    """A two-category table over C parts (C >= 2): [0, C // 2) and [C // 2, C); one category of one part for C == 1."""
    return (0, 1) if C == 1 else (0, C // 2, C)


def make_inputs(g, labels, N, C=50, part_offsets=SHAPENET_PART_OFFSETS, bump=2.0, noise=1.0, quantum=None, absent_part=(),
                stray=(), all_wrong=()):
    """Seeded scores / labels for the clouds ``labels`` (category per cloud), g a numpy RandomState.
    seg is drawn inside the cloud's category; score = bump on the true part + noise * normal.
    quantum: scores rounded to multiples of it (equal maxima become common).  absent_part: clouds whose LAST part occurs neither in
    seg nor -- pushed far down -- in the prediction.  stray: clouds where a third of the points get a bump on a part of another
    category.  all_wrong: clouds whose true part is pushed far down at every point."""
    off = list(part_offsets)
    B = len(labels)
    score = (noise * g.standard_normal((B, C, N))).astype(np.float32)
    seg = np.zeros((B, N), np.int64)
    for b, lab in enumerate(labels):
        lo, hi = off[lab], off[lab + 1]
        top = hi - 1 if (b in absent_part and hi - lo > 1) else hi
        seg[b] = g.randint(lo, top, N)
        score[b, seg[b], np.arange(N)] += np.float32(bump)
        if b in absent_part and hi - lo > 1:
            score[b, hi - 1] -= np.float32(50.0)
        if b in stray:
            outside = np.array([p for p in range(C) if not lo <= p < hi])
            pts = g.choice(N, max(1, N // 3), replace=False)
            score[b, outside[g.randint(0, len(outside), len(pts))], pts] += np.float32(2.0 * bump + 2.0)
        if b in all_wrong:
            score[b, seg[b], np.arange(N)] -= np.float32(50.0)
    if quantum:
        score = (np.round(score / np.float32(quantum)) * np.float32(quantum)).astype(np.float32)
    return score, seg, np.asarray(labels, np.int64)


def argmax_rule_inputs(g, C=7, N=96):
    """1 x C x N scores with ties, +-0, -inf columns and one or several NaNs per point (for the arg-max rule against torch.max)."""
    s = np.round(g.standard_normal((1, C, N)) * 2).astype(np.float32) / 2          # ties
    s[0, :, 0:8] = 0.0
    s[0, 1::2, 0:8] = -0.0                                                          # +-0 are equal
    s[0, :, 8:16] = -np.inf                                                         # a column of -inf
    s[0, 2, 12:16] = 1.0
    s[0, :, 16:24] = np.inf
    for n in range(24, 48):                                                         # one NaN per point, anywhere
        s[0, g.randint(0, C), n] = np.nan
    for n in range(48, 72):                                                         # several NaNs per point
        s[0, g.choice(C, 3, replace=False), n] = np.nan
    s[0, :, 72:76] = np.nan                                                         # all NaN
    s[0, 0, 76:80] = np.nan                                                         # NaN first, larger numbers after
    s[0, C - 1, 80:84] = np.nan                                                     # NaN last
    return s
