"""Drop-in of the loss classes of the reference's models/losses.py that sit on the hot path's heads.

``ChamferLoss`` (models/losses.py:193-295) keeps its constructor, call signature and the attributes the
autoencoder reads (``forward_loss``, ``backward_loss``, ``forward_loss_array``, ``backward_loss_array``,
``loss_array``).  The reference builds two faiss ``IndexFlatL2`` per sample on the host (a D2H copy, an index
build and two searches per cloud, :237-263); here both nearest-neighbour directions of the whole batch are one
launch each of ``sonet_chamfer_nn_f32`` (exact brute force, distance ``(dx*dx+dy*dy)+dz*dz``, ties -> lowest
index), and the gathers / ``robust_norm`` / means are the reference's arithmetic on device tensors, so autograd
flows through the gathered predicted points and the predicted cloud exactly as at :269-290.

faiss is not vendored in the reference and not available here: at that boundary parity is pinned to the
restated exact search of the test suite's CPU checker, not to faiss itself -- near-tie
neighbours can legitimately differ from a BLAS-form faiss search.

This file shadows the reference's ``models/losses.py`` in the overlay, so every *other* public name of that
file (``compute_iou`` -- called by part-seg/train.py:95 --, ``compute_iou_np_array``, ``visualize_pc_seg``:
host-side numpy metrics / visdom plotting, off the hot path) is served lazily from the reference checkout's
own file through the module ``__getattr__`` below; nothing of it is restated here.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from sonet_hip import ops as _ops
from sonet_hip import overlay as _overlay

__getattr__ = _overlay.delegate(__package__, "losses.py", __file__, optional_imports=("faiss",))


def _reference_losses():
    return _overlay.reference_module(__package__, "losses.py", __file__, optional_imports=("faiss",))


def robust_norm(var):
    """B x k x 3 x N -> B x k x N: sqrt(sum over the coordinate axis + 1e-8) (models/losses.py:17-27)."""
    return ((var ** 2).sum(dim=2) + 1e-8).sqrt()


def _takes_ce_operator(fused, inputs, targets, weight, dims):
    """The routing rule of the two cross-entropy classes: the one-operator path (``ops.ce_loss``) when the option is set and the scores
    are CUDA float32 of ``dims`` dimensions with int64 targets, no class weight and a class count inside the operator's extent."""
    return (bool(fused) and weight is None and inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() == dims
            and targets.is_cuda and targets.dtype == torch.int64 and targets.dim() == dims - 1
            and _ops.ce_supported(inputs.shape[1], inputs.shape[0], inputs.shape[2] if dims == 3 else 1))


class CrossEntropyLossSeg(nn.Module):
    """Per-point NLL over B x classes x N scores (models/losses.py:30-43).

    ``fused=True``: CUDA float32 scores without a class weight go through ``ops.ce_loss`` -- one forward call (float64 after the load,
    deterministic by construction) and one gradient launch; ``last_bad`` then holds the B int32 counts of targets outside [0, C) of the
    last such call (a device tensor, never read on the host here).  Every other case -- ``fused=False`` included, which launches nothing
    new -- takes the path below."""

    def __init__(self, weight=None, size_average=True, fused=False):
        super().__init__()
        self.nll_loss = nn.NLLLoss(weight, reduction="mean" if size_average else "sum")
        self.size_average = size_average
        self.fused = fused
        self.last_bad = None

    def forward(self, inputs, targets):
        if _takes_ce_operator(self.fused, inputs, targets, self.nll_loss.weight, 3):
            loss, self.last_bad = _ops.ce_loss(inputs.contiguous(), targets.contiguous(), "mean" if self.size_average else "sum",
                                               want_bad=True)
            return loss
        logp = F.log_softmax(inputs.unsqueeze(3), dim=1)
        if logp.is_cuda and self.nll_loss.weight is None:
            # the same sum as a gather + a plain reduction: on the GPU NLLLoss's 4-D forward adds its block partials atomically, so its
            # last bit changes from run to run (the gather's backward writes every element once: deterministic)
            picked = -torch.gather(logp, 1, targets.unsqueeze(1).unsqueeze(3)).squeeze(1)
            return picked.mean() if self.size_average else picked.sum()
        return self.nll_loss(logp, targets.unsqueeze(2))


class CrossEntropyLossCls(nn.Module):
    """The classifier's criterion (models/classifier.py:95,105: ``torch.nn.CrossEntropyLoss()`` on B x classes scores and B labels).
    ``fused=True`` routes as ``CrossEntropyLossSeg`` does (``ops.ce_loss`` with N = 1, ``last_bad``); otherwise, and by default, it IS
    ``nn.CrossEntropyLoss``."""

    def __init__(self, fused=False):
        super().__init__()
        self.criterion = nn.CrossEntropyLoss()
        self.fused = fused
        self.last_bad = None

    def forward(self, inputs, targets):
        if _takes_ce_operator(self.fused, inputs, targets, None, 2):
            loss, self.last_bad = _ops.ce_loss(inputs.contiguous(), targets.contiguous(), "mean", want_bad=True)
            return loss
        return self.criterion(inputs, targets)


class ChamferLoss(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.dimension = 3
        self.k = 1
        self.forward_loss = torch.FloatTensor([0])
        self.backward_loss = torch.FloatTensor([0])

    @staticmethod
    def _select(src, idx):
        """src B x 3 x Ns, idx B x Nq (i32) -> B x 1 x 3 x Nq = src[b, :, idx[b, q]] (index_select per sample)."""
        B, C, _ = src.shape
        return torch.gather(src, 2, idx.long().unsqueeze(1).expand(B, C, idx.shape[1])).unsqueeze(1)

    def forward(self, predict_pc, gt_pc):
        """predict_pc B x 3 x M, gt_pc B x 3 x N (CUDA) -> scalar forward + backward Chamfer term."""
        if (getattr(self.opt, "chamfer_fused", False) and predict_pc.is_cuda and gt_pc.is_cuda
                and predict_pc.dtype == gt_pc.dtype == torch.float32 and not gt_pc.requires_grad):
            # opt.chamfer_fused: search, elements and sums in one launch, the gradient in one more (ops.chamfer_loss)
            (self.forward_loss, self.backward_loss, self.forward_loss_array,
             self.backward_loss_array) = _ops.chamfer_loss(predict_pc.contiguous(), gt_pc.contiguous())
            self.loss_array = self.forward_loss_array + self.backward_loss_array
            return self.forward_loss + self.backward_loss
        p = predict_pc.detach().contiguous().float()
        g = gt_pc.detach().contiguous().float()
        nn_gt = _ops.chamfer_nn(p, g)                          # predicted -> nearest gt      (:255)
        nn_pr = _ops.chamfer_nn(g, p)                          # gt        -> nearest predicted (:262)
        # (two launches on purpose: the one-sweep kernel sonet_chamfer_nn2_f32 -- row minima in registers, column minima as keys
        #  in LDS bins -- gives identical indices but measured 25x slower, 8.7 vs 0.34 ms at B = 64: a dependent LDS read and a
        #  divergent branch per pair, against two register-only loops that already run at 0.67 of the vector-issue roof)
        selected_gt_by_predict = self._select(gt_pc, nn_gt)
        selected_predict_by_gt = self._select(predict_pc, nn_pr)
        forward_loss_element = robust_norm(selected_gt_by_predict - predict_pc.unsqueeze(1))
        self.forward_loss = forward_loss_element.mean()
        self.forward_loss_array = forward_loss_element.mean(dim=1).mean(dim=1)
        backward_loss_element = robust_norm(selected_predict_by_gt - gt_pc.unsqueeze(1))
        self.backward_loss = backward_loss_element.mean()
        self.backward_loss_array = backward_loss_element.mean(dim=1).mean(dim=1)
        self.loss_array = self.forward_loss_array + self.backward_loss_array
        return self.forward_loss + self.backward_loss


class AutoencoderLoss(nn.Module):
    """The Chamfer terms that enter ``loss`` in ``Model.optimize`` (models/autoencoder.py:83-98): the final cloud alone at
    ``opt.output_conv_pc_num == 0``, plus ``decoder.conv_pc4`` at 1024, plus ``decoder.conv_pc5`` and ``decoder.conv_pc4`` at 4096, each
    against the same ground-truth cloud.  ``forward(predicted_pc, decoder, gt)`` returns ``loss`` and sets ``loss``, ``loss_chamfer``,
    ``loss_chamfer_conv4`` and ``loss_chamfer_conv5`` (None where the term does not enter the loss).

    With ``opt.chamfer_pyramid`` set, CUDA float32 clouds, a gt that asks for no gradient and sizes inside the operator's extents, every
    term comes from ONE ``ops.chamfer_pyramid_loss`` call (one loss launch, one deterministic gradient launch per step).  In every other
    case -- the option absent included -- the terms are ``ChamferLoss`` calls in the reference's order (conv5, conv4, the final cloud),
    and ``chamfer_criteria`` holds what the last of them left."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.chamfer_criteria = ChamferLoss(opt)
        self.loss = self.loss_chamfer = self.loss_chamfer_conv4 = self.loss_chamfer_conv5 = None

    @staticmethod
    def pyramid_enabled(opt):
        """``opt.chamfer_pyramid``: absent, None, False or 0 is off."""
        return bool(getattr(opt, "chamfer_pyramid", False))

    def terms(self, predicted_pc, decoder):
        """[(attribute name, predicted cloud)] in the order the reference adds them up (autoencoder.py:93-98)."""
        n = self.opt.output_conv_pc_num
        out = [("loss_chamfer", predicted_pc)]
        if n == 4096:
            out.append(("loss_chamfer_conv5", decoder.conv_pc5))
        if n in (1024, 4096):
            out.append(("loss_chamfer_conv4", decoder.conv_pc4))
        return out

    def _takes_pyramid(self, clouds, gt):
        if not self.pyramid_enabled(self.opt) or gt.requires_grad or gt.dim() != 3:
            return False
        for t in clouds + [gt]:
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[1] == 3 and t.shape[0] == gt.shape[0]):
                return False
        return 1 <= gt.shape[0] <= 65535 and _ops.chamfer_pyramid_supported([c.shape[2] for c in clouds], gt.shape[2])

    def forward(self, predicted_pc, decoder, gt):
        terms = self.terms(predicted_pc, decoder)
        self.loss_chamfer = self.loss_chamfer_conv4 = self.loss_chamfer_conv5 = None
        clouds = [c for _, c in terms]
        if self._takes_pyramid(clouds, gt):
            levels = _ops.chamfer_pyramid_loss([c.contiguous() for c in clouds], gt.contiguous())
            for (name, _), (fl, bl, _fa, _ba) in zip(terms, levels):
                setattr(self, name, fl + bl)
            (self.forward_loss, self.backward_loss, self.forward_loss_array, self.backward_loss_array) = levels[0]
            self.loss_array = self.forward_loss_array + self.backward_loss_array
        else:
            for name, cloud in terms[1:] + terms[:1]:                # the reference's order of calls: conv5, conv4, the final cloud
                setattr(self, name, self.chamfer_criteria(cloud, gt))
            c = self.chamfer_criteria
            (self.forward_loss, self.backward_loss, self.forward_loss_array, self.backward_loss_array, self.loss_array) = (
                c.forward_loss, c.backward_loss, c.forward_loss_array, c.backward_loss_array, c.loss_array)
        loss = self.loss_chamfer
        for name, _ in terms[1:]:                                    # loss_chamfer + loss_chamfer_conv5 + loss_chamfer_conv4
            loss = loss + getattr(self, name)
        self.loss = loss
        return loss
