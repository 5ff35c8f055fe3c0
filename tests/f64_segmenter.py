"""tests/f64_segmenter.py -- TEST INFRASTRUCTURE: one part-segmentation training step of the reference in float64, in plain torch autograd,
with the three arg-max pools and the ReLU patterns either FREE or FORCED, as tests/f64_classifier.py does for the classifier (whose
encoder it shares: ``f64_classifier.encoder_forward``).

Follows, line by line, what ``models/segmenter.py:113-124`` (``Model.optimize``) runs with dropout off:
  Encoder.forward           models/networks.py:111-199   (as in f64_classifier; KNNModule with som_k_type "center": the neighbourhood
                                                          centre is the node itself, models/layers.py:342-343; x_decentered / centers
                                                          :167-172 -- in stage-fed mode x_decentered is the stage's first three rows and
                                                          centers the node coordinates gathered at every column's node, which is what
                                                          the reference's one-hot sum over the nodes computes)
  Model.forward             models/segmenter.py:79-109   (node of every point copy = argmax of the one-hot mask = min_idx; the three
                                                          back-broadcast gathers of first_pn_out_masked_max, knn_feature_1, final_pn_out)
  Segmenter.forward         models/networks.py:272-344   (concat order x_decentered, x, centers, sn, one-hot label, first_pn_out, the
                                                          three gathers, feature; layers 1-3; the k copies averaged as (1/3)*(a+b+c);
                                                          layers 4, 5)
  CrossEntropyLossSeg       models/losses.py:30-43       (log_softmax over the classes + NLLLoss, mean over B x N)
BatchNorm in training mode as in f64_classifier.  ReLU masks of the head under "seg.layer1" .. "seg.layer4", gradients and batch statistics
of the head under "seg." + the reference key.
"""
import torch
import torch.nn.functional as F

import f64_classifier as F64

SEG_MASK_KEYS = ("seg.layer1", "seg.layer2", "seg.layer3", "seg.layer4")


def train_step(enc, seg, label, seg_target, node_knn_I, pc, sn, som_k=9, node=None, k=3, stage=None, route=None, masks=None):
    """One forward + backward.  ``enc`` / ``seg``: ``f64_classifier.leaf_params`` dictionaries (reference key names; ``seg``: the
    Segmenter's).  ``pc``, ``sn`` B x 3 x N: always needed (the head reads them); with ``node`` the SOM stage runs here, otherwise
    ``stage`` = dict(x_aug, min_idx, row_max, som_node) from the run under test as in f64_classifier -- in the ORIGINAL column order
    (copy c of point n at column c * N + n): the head's k-copy mean depends on it.  ``route`` / ``masks``: as in f64_classifier, ``masks``
    also holding "seg.layer1" .. "seg.layer4".
    -> dict(loss, score, grads {key: tensor; head keys "seg." + key}, route, masks, bn {layer prefix: (batch mean, biased batch variance,
    element count)})."""
    if stage is not None and stage.get("pos0") is not None:
        raise ValueError("the segmenter twin needs the stage in the original column order (pos0 must be None)")
    F64._TAKEN.clear()
    F64._STATS.clear()
    e = F64.encoder_forward(enc, node_knn_I, som_k, pc, sn, node, k, stage, route, masks, None, som_k_type="center")
    dt = e["first"].dtype
    x_dec = e["x_aug"][:, :3]
    min_idx = e["min_idx"]
    som_node = e["som_node"]
    B, N = pc.shape[0], pc.shape[2]
    kN = k * N
    assert min_idx.shape[1] == kN, (tuple(min_idx.shape), k, N)
    centers = som_node.gather(2, min_idx.unsqueeze(1).expand(B, 3, kN)).detach()                       # networks.py:167
    # models/segmenter.py:90-99: node of every copy, the three node-level maps gathered back to the copies
    idx = min_idx.unsqueeze(1)
    g1 = torch.gather(e["masked_max"], 2, idx.expand(B, e["masked_max"].shape[1], kN))
    g2 = torch.gather(e["knn_feature"], 2, idx.expand(B, e["knn_feature"].shape[1], kN))
    g3 = torch.gather(e["final"], 2, idx.expand(B, e["final"].shape[1], kN))
    feature = e["feature"]
    # networks.Segmenter.forward
    x = torch.cat([pc.to(dt)] * k, dim=2)
    sn_ = torch.cat([sn.to(dt)] * k, dim=2)
    onehot = torch.zeros(B, 16, dtype=dt, device=x.device)
    onehot.scatter_(1, label.long().unsqueeze(1), 1)
    onehot = onehot.unsqueeze(2).expand(B, 16, kN).detach()
    layer1_in = torch.cat((x_dec, x, centers, sn_, onehot, e["first"], g1, g2, g3, feature.unsqueeze(2).expand(B, feature.shape[1], kN)),
                          dim=1)
    sp = {"seg." + k_: v for k_, v in seg.items()}
    h = F64._conv(layer1_in, sp, "seg.layer1", True, True, masks)
    h = F64._conv(h, sp, "seg.layer2", True, True, masks)
    h = F64._conv(h, sp, "seg.layer3", True, True, masks)
    parts = torch.split(h, N, dim=2)
    assert len(parts) == k
    if k == 2:
        h = 0.5 * (parts[0] + parts[1])
    elif k == 3:
        h = (1.0 / 3.0) * (parts[0] + parts[1] + parts[2])
    else:
        raise ValueError("the reference averages k in {2, 3} only (networks.py:331-336), got k=%d" % k)
    h = F64._conv(h, sp, "seg.layer4", True, True, masks)
    score = F64._conv(h, sp, "seg.layer5", False, False)
    loss = F.nll_loss(F.log_softmax(score.unsqueeze(3), dim=1), seg_target.long().unsqueeze(2))                  # losses.py:41-43
    leaves = {k_: v for k_, v in list(enc.items()) + list(sp.items()) if v.requires_grad}
    gr = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return dict(loss=loss.detach(), score=score.detach(), feature=feature.detach(),
                grads={k_: g for k_, g in zip(leaves, gr) if g is not None},
                route=dict(pool1=e["pool1"], pool2=e["pool2"], pool3=e["pool3"]), masks=dict(F64._TAKEN), bn=dict(F64._STATS))
