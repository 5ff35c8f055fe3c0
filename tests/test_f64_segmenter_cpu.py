"""The float64 twin of the part-segmentation training step (tests/f64_segmenter.py) against the unmodified reference's own float64 run
(tests/golden/seg_train_step_b8_n512.npz, oracle/make_golden.py golden_seg_train_step): the twin the GPU suite forces the HIP path's
routing on (tests/test_gpu_seg_training.py) IS the reference's step."""
import json
import os
from argparse import Namespace

import numpy as np
import torch

from conftest import GOLDEN, golden

FIXTURE = "seg_train_step_b8_n512"


def _state_dicts(seed):
    """Encoder and Segmenter state_dicts with the reference key names and the fixture's weights (sonet_hip.synth seeds)."""
    from models import networks as NW
    from sonet_hip import synth
    shapes = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["encoder"]
    enc = {k: (torch.zeros(s, dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.zeros(s)) for k, s in shapes.items()}
    opt = Namespace(gpu_id=-1, device=torch.device("cpu"), batch_size=2, input_pc_num=256, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.0, node_num=64, k=3, som_k=9, som_k_type="center",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=50)
    seg = {k: v.clone() for k, v in NW.Segmenter(opt).state_dict().items()}
    return synth.fill_state_dict_(enc, seed), synth.fill_state_dict_(seg, seed + 1)


def test_f64_segmenter_twin_reproduces_the_reference_float64_run():
    """Run free on the fixture's inputs, the twin takes the very pool positions the reference took in float64 (pools 1 and 2 exactly,
    pool 3 as well: this fixture has no tied winner), its loss equals the reference's to 1e-14 and every stored gradient -- encoder and every segmenter
    layer -- agrees to 1e-12 rel-rms; with ``route64/`` forced it gives the same loss again."""
    import f64_classifier as F64
    import f64_segmenter as S64
    g = golden(FIXTURE)
    enc_sd, seg_sd = _state_dicts(int(g["seed"]))
    enc, seg = F64.leaf_params(enc_sd, "cpu"), F64.leaf_params(seg_sd, "cpu")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))                       # noqa: E731
    inputs = dict(pc=T(g["pc"]).double(), sn=T(g["sn"]).double(), node=T(g["node"]).double())
    r = S64.train_step(enc, seg, T(g["label"]), T(g["seg"]), T(g["node_knn_I"]), **inputs)
    assert abs(float(r["loss"]) - float(g["loss64"])) <= 1e-14 * abs(float(g["loss64"]))
    # pool 3 too: the classifier fixtures meet genuine ties there (two nodes with the same neighbour set in another order), this one none
    for pool in ("pool1", "pool2", "pool3"):
        np.testing.assert_array_equal(r["route"][pool].numpy(), g["route64/" + pool].astype(np.int64))
    assert sorted(r["masks"]) == sorted(["first_pointnet.layers.0", "first_pointnet.layers.1", "first_pointnet.layers.2", "knnlayer.layers.0",
                                         "knnlayer.layers.1", "final_pointnet.layers.0"] + list(S64.SEG_MASK_KEYS))
    n = int(g["sub_n"])

    def sub(t):
        f = t.detach().flatten()
        return f[::max(1, f.numel() // n)].numpy()
    checked = set()
    for k in [k[7:] for k in g.files if k.startswith("grad64/")]:
        truth = g["grad64/" + k].astype(np.float64)
        rms = float(np.sqrt(np.mean(truth ** 2)))
        if rms < 1e-12:                                  # (biases in front of a BatchNorm: the true gradient is 0)
            continue
        mine = sub(r["grads"][k])
        assert mine.shape == truth.shape, k
        assert float(np.sqrt(np.mean((mine - truth) ** 2))) <= 1e-12 * rms, k
        checked.add(k)
    assert len(checked) >= 20 and {"seg.layer%d.conv.weight" % i for i in range(1, 6)} <= checked, sorted(checked)
    forced = S64.train_step(enc, seg, T(g["label"]), T(g["seg"]), T(g["node_knn_I"]),
                            route={p: T(g["route64/" + p].astype(np.int64)) for p in ("pool1", "pool2", "pool3")}, **inputs)
    assert abs(float(forced["loss"]) - float(g["loss64"])) <= 1e-12 * abs(float(g["loss64"]))
    for k, gr in r["grads"].items():
        a, b = gr.double(), forced["grads"][k].double()
        if float(b.norm()) > 1e-10:
            assert float((a - b).norm() / b.norm()) <= 1e-9, k


def test_seg_fixture_reference_float32_routing_flips_are_few():
    """The yardstick of the GPU suite's free-routing check: the reference's own float32 run against its float64 run (``route32/`` holds
    the positions where the two differ)."""
    g = golden(FIXTURE)
    for pool in ("pool1", "pool2", "pool3"):
        at, val = g["route32/%s_at" % pool], g["route32/%s_val" % pool]
        assert at.shape == val.shape and at.size <= 4, (pool, at.size)
        assert np.all(g["route64/" + pool].ravel()[at] != val)


def test_f64_encoder_knn_centre_types():
    """f64_classifier.encoder_forward's two KNN neighbourhood centres: "center" is the node itself, "avg" (the classifier's) the neighbour
    mean; the first PointNet does not depend on the choice."""
    import f64_classifier as F64
    g = golden("train_step_b16_n512")
    seed = int(g["seed"])
    enc_sd, _ = _state_dicts(seed)
    enc = F64.leaf_params(enc_sd, "cpu")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))                       # noqa: E731
    B = 4
    pc, sn, node = T(g["pc"][:B]).double(), T(g["sn"][:B]).double(), T(g["node"][:B]).double()
    e_avg = F64.encoder_forward(enc, T(g["node_knn_I"][:B]), 9, pc, sn, node, 3, None, None, None, None)
    e_ctr = F64.encoder_forward(enc, T(g["node_knn_I"][:B]), 9, pc, sn, node, 3, None, None, None, None, som_k_type="center")
    assert torch.equal(e_ctr["knn_center"], e_ctr["som_node"])
    assert not torch.equal(e_avg["knn_center"], e_ctr["knn_center"])
    assert torch.equal(e_avg["first"], e_ctr["first"])                 # the first PointNet does not see the KNN centre
