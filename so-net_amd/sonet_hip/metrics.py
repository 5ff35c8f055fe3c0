"""Evaluation loops on the device: per-epoch totals with one host transfer at the end (part segmentation: loss, accuracy and IoU;
autoencoder: the Chamfer test loss -- ``ChamferEvaluator`` / ``evaluate_autoencoder``; classification: loss, accuracy and the confusion
table -- ``ClsEvaluator`` / ``evaluate_classification`` at the end of this file).

The reference's test loop (part-seg/train.py:75-104) copies every batch's B x 50 x N score tensor to the host and runs
``losses.compute_iou``, a Python double loop over clouds and parts.  Here one ``sonet_seg_metrics_f32`` call per batch reads the
scores once (``ops.seg_metrics``) and ``SegEvaluator`` keeps the epoch's totals in a few device words.

In part-seg/train.py the test loop becomes

    evaluator = SegEvaluator()                                                         # before the loop, reset() per epoch
    evaluator.update(model.score_segmenter, model.input_seg, model.input_label)         # instead of lines 87-96

and ``evaluator.result()`` after the loop gives the three numbers of lines 102-104.
"""
import torch

from . import ops
from ._lib import SonetHipError


def seg_iou(score, seg, label, part_offsets=None):
    """Per-cloud mean IoU, B float64 on the device: the counterpart of models/losses.py:73-116 (compute_iou_np_array)."""
    return ops.seg_metrics(score, seg, label, part_offsets).iou


class SegEvaluator:
    """Epoch totals of the segmentation test loop.  ``update`` launches and returns (no sync, no ``.item()``); ``result`` makes the one
    device-to-host transfer and returns the names of models/segmenter.py:166-168, each as total / count."""

    def __init__(self, part_offsets=None):
        self.part_offsets = part_offsets
        self._sums = None              # f64 [3]: sum over clouds of nll_sum / N, correct / N, iou
        self._ints = None              # i64 [3]: clouds, clouds with bad != 0, sum of bad

    def reset(self):
        if self._sums is not None:
            self._sums.zero_()
            self._ints.zero_()

    def update(self, score, seg, label):
        m = ops.seg_metrics(score, seg, label, self.part_offsets)
        if self._sums is None or self._sums.device != score.device:
            self._sums = torch.zeros(3, dtype=torch.float64, device=score.device)
            self._ints = torch.zeros(3, dtype=torch.int64, device=score.device)
        self._sums += torch.stack([m.nll_sum.sum() / m.N, m.correct.sum(dtype=torch.float64) / m.N, m.iou.sum()])
        self._ints[0] += score.shape[0]
        self._ints[1:] += torch.stack([(m.bad != 0).sum(), m.bad.sum()])
        return m

    def result(self):
        if self._sums is None:
            raise SonetHipError("SegEvaluator.result() before any update()")
        host = torch.cat([self._sums, self._ints.to(torch.float64)]).cpu().tolist()       # the one transfer (counts < 2^53: exact)
        loss, acc, iou = host[:3]
        count, bad_clouds, bad = (int(v) for v in host[3:])
        if bad_clouds:
            raise SonetHipError("segmentation evaluation: %d bad cloud(s) of %d (%d part label(s) outside [0, C) or categories outside "
                                "the part table)" % (bad_clouds, count, bad))
        if count == 0:
            raise SonetHipError("SegEvaluator.result() without any cloud")
        if loss != loss:
            raise SonetHipError("segmentation evaluation: the loss of %d clouds is NaN (non-finite scores; no bad label)" % count)
        return {"test_loss_seg": loss / count, "test_acc_seg": acc / count, "test_iou": iou / count, "count": count}


def evaluate_segmentation(encoder, segmenter, assembler, batch_size, evaluator=None):
    """One pass over the split of a test-mode shapenet ``BatchAssembler``: forward + metrics per batch, no host sync inside the loop;
    returns ``SegEvaluator.result()``."""
    from models import networks
    if assembler.recipe != "shapenet" or assembler.mode == "train":
        raise SonetHipError("evaluate_segmentation needs a test-mode shapenet BatchAssembler, got recipe %r mode %r"
                            % (assembler.recipe, assembler.mode))
    ev = SegEvaluator() if evaluator is None else evaluator
    ev.reset()
    encoder.eval()
    segmenter.eval()
    with torch.no_grad():
        for pc, sn, label, seg, node, node_knn_I in assembler.epoch(0, batch_size, shuffle=False):
            score = networks.segmentation_forward(encoder, segmenter, pc, sn, label, node, node_knn_I)
            ev.update(score.float().contiguous(), seg.contiguous(), label.contiguous())
    return ev.result()


class ChamferEvaluator:
    """Epoch totals of the autoencoder test loop (autoencoder/train.py:79-99).  ``update`` launches ``ops.chamfer_terms`` without the
    index and element outputs and adds each cloud's forward and backward loss into float64 device words (no sync, no ``.item()``);
    ``result`` makes the one device-to-host transfer.  ``test_loss`` is the number of train.py:94-96, sum of (batch loss x batch size)
    / clouds: all clouds of an epoch share M and N, so it equals the mean over clouds of the per-cloud loss."""

    def __init__(self):
        self._sums = None              # f64 [2]: sum over clouds of forward loss, of backward loss
        self._ints = None              # i64 [2]: clouds, clouds whose loss is NaN

    def reset(self):
        if self._sums is not None:
            self._sums.zero_()
            self._ints.zero_()

    def update(self, predicted_pc, gt):
        t = ops.chamfer_terms(predicted_pc, gt, want_nn=False, want_elems=False)
        if self._sums is None or self._sums.device != gt.device:
            self._sums = torch.zeros(2, dtype=torch.float64, device=gt.device)
            self._ints = torch.zeros(2, dtype=torch.int64, device=gt.device)
        per_cloud = torch.stack([t.sums[:, 0] / t.M, t.sums[:, 1] / t.N], dim=1)          # B x 2 f64
        self._sums += per_cloud.sum(dim=0)
        self._ints[0] += gt.shape[0]
        self._ints[1] += torch.isnan(per_cloud).any(dim=1).sum()
        return per_cloud.sum(dim=1).float()                                                # loss_array (models/losses.py:289)

    def result(self):
        if self._sums is None:
            raise SonetHipError("ChamferEvaluator.result() before any update()")
        host = torch.cat([self._sums, self._ints.to(torch.float64)]).cpu().tolist()       # the one transfer (counts < 2^53: exact)
        fwd, bwd = host[:2]
        count, nan_clouds = int(host[2]), int(host[3])
        if count == 0:
            raise SonetHipError("ChamferEvaluator.result() without any cloud")
        if nan_clouds or fwd != fwd or bwd != bwd:
            raise SonetHipError("autoencoder evaluation: the Chamfer loss of %d cloud(s) of %d is NaN (non-finite coordinates)"
                                % (nan_clouds, count))
        return {"test_loss": (fwd + bwd) / count, "forward": fwd / count, "backward": bwd / count, "count": count}


def evaluate_autoencoder(encoder, decoder, assembler, batch_size, evaluator=None):
    """One pass over the split of a test-mode ``BatchAssembler``: encoder, decoder and ``ChamferEvaluator.update`` per batch under
    ``no_grad`` (models/autoencoder.py:105-119 without the pyramid terms the test loss does not read), no host sync inside the loop, the
    last batch may be short; returns ``ChamferEvaluator.result()``."""
    if assembler.mode == "train":
        raise SonetHipError("evaluate_autoencoder needs a test-mode BatchAssembler, got mode %r" % (assembler.mode,))
    ev = ChamferEvaluator() if evaluator is None else evaluator
    ev.reset()
    encoder.eval()
    decoder.eval()
    shapenet = assembler.recipe == "shapenet"            # (pc, sn, label, seg, node, knn) there; (pc, sn, label, node, knn[, idx]) otherwise
    with torch.no_grad():
        for batch in assembler.epoch(0, batch_size, shuffle=False):
            pc, sn = batch[0], batch[1]
            node, node_knn_I = (batch[4], batch[5]) if shapenet else (batch[3], batch[4])
            predicted_pc = decoder(encoder(pc, sn, node, node_knn_I, False, None))
            ev.update(predicted_pc.float().contiguous(), pc.contiguous())
    return ev.result()


class ClsEvaluator:
    """Epoch totals of the classification test loop (modelnet/train.py:70-90, which calls ``.cpu()`` on every batch).  ``update`` makes
    one ``ops.ce_terms`` call -- loss terms, arg-max by ``torch.max``'s rule, correct / bad counts and the confusion table from one read
    of the B x classes scores -- and a few device adds (no sync, no ``.item()``); ``result`` makes the one device-to-host transfer.
    ``test_loss`` is the number of train.py:81,89: a batch's mean loss times its batch size is that batch's sum, so the epoch's value
    is the sum of the per-cloud losses / clouds.  ``test_accuracy``: train.py:84-90."""

    def __init__(self, classes):
        self.classes = int(classes)
        if not ops.ce_supported(self.classes):
            raise SonetHipError("ClsEvaluator: classes must be in [1, %d], got %r" % (ops.CE_MAX_C, classes))
        self._loss = None              # f64 [1]: sum over clouds of the loss
        self._ints = None              # i64 [3]: clouds, correct, bad labels
        self._confusion = None         # i64 [classes][classes]: [label][prediction]

    def reset(self):
        if self._loss is not None:
            self._loss.zero_()
            self._ints.zero_()
            self._confusion.zero_()

    def update(self, score, label):
        if isinstance(score, torch.Tensor) and score.dim() == 2 and score.shape[1] != self.classes:
            raise SonetHipError("ClsEvaluator: scores of %d classes, the evaluator holds %d" % (score.shape[1], self.classes))
        if not isinstance(score, torch.Tensor) or score.dim() != 2:
            raise SonetHipError("ClsEvaluator.update: score must be a B x classes torch.Tensor")
        if self._loss is None or self._loss.device != score.device:
            ops._chk(score, "score", torch.float32)                   # (before the first allocation: a CPU tensor is refused as CUDA)
            C = self.classes
            self._loss = torch.zeros(1, dtype=torch.float64, device=score.device)
            self._ints = torch.zeros(3, dtype=torch.int64, device=score.device)
            self._confusion = torch.zeros((C, C), dtype=torch.int64, device=score.device)
        t = ops.ce_terms(score, label, confusion=self._confusion)
        self._loss += t.nll_sum.sum()
        self._ints[0] += score.shape[0]
        self._ints[1:] += torch.stack([t.correct.sum(), t.bad.sum()])
        return t

    def result(self):
        if self._loss is None:
            raise SonetHipError("ClsEvaluator.result() before any update()")
        C = self.classes
        host = torch.cat([self._loss, self._ints.to(torch.float64), self._confusion.view(-1).to(torch.float64)]).cpu()   # the one transfer
        loss = float(host[0])                                         # (counts < 2^53: exact)
        count, correct, bad = (int(v) for v in host[1:4].tolist())
        confusion = host[4:].view(C, C).to(torch.int64).numpy()
        if bad:
            raise SonetHipError("classification evaluation: %d label(s) of %d clouds outside [0, %d)" % (bad, count, C))
        if count == 0:
            raise SonetHipError("ClsEvaluator.result() without any cloud")
        if loss != loss:
            raise SonetHipError("classification evaluation: the loss of %d clouds is NaN (non-finite scores; no bad label)" % count)
        per_class = confusion.sum(axis=1)
        seen = per_class > 0
        class_acc = float((confusion.diagonal()[seen] / per_class[seen]).mean())
        return {"test_loss": loss / count, "test_accuracy": correct / count, "class_accuracy": class_acc, "confusion": confusion,
                "count": count}


def evaluate_classification(encoder, classifier, assembler, batch_size, evaluator=None):
    """One pass over the split of a test-mode modelnet or shrec ``BatchAssembler``: encoder, classifier and ``ClsEvaluator.update`` per
    batch under ``no_grad`` (models/classifier.py:101-107 without the host reads), no host sync inside the loop, the last batch may be
    short; returns ``ClsEvaluator.result()``."""
    if assembler.recipe not in ("modelnet", "shrec") or assembler.mode == "train":
        raise SonetHipError("evaluate_classification needs a test-mode modelnet or shrec BatchAssembler, got recipe %r mode %r"
                            % (assembler.recipe, assembler.mode))
    ev = ClsEvaluator(classifier.opt.classes) if evaluator is None else evaluator
    ev.reset()
    encoder.eval()
    classifier.eval()
    with torch.no_grad():
        for batch in assembler.epoch(0, batch_size, shuffle=False):
            pc, sn, label, node, node_knn_I = batch[:5]
            score = classifier(encoder(pc, sn, node, node_knn_I, False, None))
            ev.update(score.float().contiguous(), label.contiguous())
    return ev.result()
