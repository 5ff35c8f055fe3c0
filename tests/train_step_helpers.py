"""Helpers of the GPU training-step gates (tests/test_gpu_parity.py, tests/test_gpu_bf16_forced_routing.py, tests/test_gpu_seg_training.py):
what the run under test fed its first PointNet and which discrete decisions it took -- the arg-max positions of its three pools and the
ReLU pattern of every BatchNorm + ReLU layer -- read so that the float64 twins (tests/f64_classifier.py, tests/f64_segmenter.py) can be
run with them forced."""
import numpy as np
import torch

DEV = "cuda:0"


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def _capture_stage(enc):
    """Wrap ``first_pointnet.forward_pooled`` of this encoder instance: records what the first PointNet was fed (the node-sorted copy in
    the f32-class training path, the original column order otherwise), the node id of every column and the pool's positions."""
    cap = {}
    inner = enc.first_pointnet.forward_pooled

    def wrapped(x, ids, row_max, M, epoch=None, need_dense=True, pos0=None):
        out = inner(x, ids, row_max, M, epoch, need_dense=need_dense, pos0=pos0)
        if out is not None:
            cap.update(x_aug=x.detach(), min_idx=ids.detach(), row_max=row_max.detach(), pool1=out[2].detach().long(), pos0=pos0,
                       need_dense=need_dense)
        return out
    enc.first_pointnet.forward_pooled = wrapped
    return cap


def _lastdim_max_node(t):
    """The _LastDimMax autograd node that produced ``t`` -- through the casts behind it (bf16: ``feature.float()``, models/networks.py:436)."""
    node = t.grad_fn
    while node is not None and type(node).__name__ != "_LastDimMaxBackward":
        assert type(node).__name__.startswith("ToCopyBackward"), type(node).__name__
        node = node.next_functions[0][0]
    assert node is not None, "no _LastDimMax node behind the tensor"
    return node


def _routing_of(enc, feat):
    """The arg-max positions this forward took at pools 2 and 3 (saved by the two _LastDimMax nodes; read BEFORE backward frees them)."""
    p2 = _lastdim_max_node(enc.knn_feature_1).saved_tensors[0]
    p3 = _lastdim_max_node(feat).saved_tensors[0]
    return dict(pool2=p2.detach().long().clone(), pool3=p3.detach().long().clone(), som_node=enc.som_node.detach().clone())


def _relu_masks_of(loss, enc, cls=None, seg=None):
    """The ReLU pattern of every BatchNorm + ReLU layer of the step that produced ``loss``, read from what its autograd nodes saved for
    their backward (call BEFORE backward): the point-wise layers save either the activation (mask = y > 0) or the raw output with the
    normalisation coefficients (mask = raw * sc + sh > 0, the fma the kernels test: its sign is the sign of the exact value, which
    float64 reproduces), the heads' FC layers the activation.  ``cls``: the classifier (layers "cls.fc1" ..), ``seg``: the part
    segmenter (layers "seg.layer1" ..).  -> {reference layer prefix: bool tensor}."""
    by_ptr = {}
    for prefix, mod in (("", enc), ("cls.", cls), ("seg.", seg)):
        if mod is None:
            continue
        for k, p in mod.named_parameters():
            if k.endswith(("conv.weight", "linear.weight")):
                by_ptr[p.data_ptr()] = prefix + k.rsplit(".", 2)[0]
    masks, seen, stack = {}, set(), [loss.grad_fn]     # (seen holds the node OBJECTS: the id of a collected wrapper would be reused)
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        stack.extend(fn for fn, _ in node.next_functions)
        name = type(node).__name__
        if name == "_PointwiseFnBackward":
            sv = node.saved_tensors
            layer = by_ptr.get(sv[2].data_ptr())
            if layer is None:
                continue
            if len(sv) == 7:                                   # 'affine' mode: (x1, x2, weight2d, scale, y | empty, ones, zeros)
                if sv[4].numel():
                    masks[layer] = sv[4] > 0
            else:                                              # 'batch' mode: (x1, x2, weight2d, sc, sh, raw, mean, invstd, gamma, zeros)
                sc, sh, raw = sv[3].double(), sv[4].double(), sv[5].double()
                shp = [1, -1] + [1] * (raw.dim() - 2)
                masks[layer] = (raw * sc.view(shp) + sh.view(shp)) > 0
        elif name == "_FcFnBackward":
            sv = node.saved_tensors
            layer = by_ptr.get(sv[1].data_ptr())
            if layer is not None and sv[2].numel():
                masks[layer] = sv[2] > 0
    return masks


def _f64_step(enc, cls, g, cap, forced, rounding=None, stored=None, stored_grads=None, pooled_dgrad="mfma"):
    """tests/f64_classifier.py on the GPU in float64, fed with the SOM stage of the run under test; ``forced``: its routing too;
    ``rounding`` / ``stored`` / ``stored_grads`` / ``pooled_dgrad``: passed on (``"bf16"``: the twin rounds where the bf16 step rounds)."""
    import f64_classifier as F64
    assert "x_aug" in cap, "the training forward did not go through first_pointnet.forward_pooled"
    e64 = F64.leaf_params(enc.state_dict(), DEV)
    c64 = F64.leaf_params(cls.state_dict(), DEV)
    stage = dict(x_aug=cap["x_aug"], min_idx=cap["min_idx"], row_max=cap["row_max"], som_node=cap["som_node"], pos0=cap["pos0"])
    route = dict(pool1=cap["pool1"], pool2=cap["pool2"], pool3=cap["pool3"]) if forced else None
    return F64.train_step(e64, c64, cu(g["label"]), cu(g["node_knn_I"]), stage=stage, route=route, masks=cap.get("masks") if forced else None,
                          rounding=rounding, stored=stored,
                          stored_grads=stored_grads, pooled_dgrad=pooled_dgrad)
