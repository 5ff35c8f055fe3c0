"""Segmenter layer 1 in its node-wise form in training (``opt.seg_nodewise_train``), the parts that need no GPU:

* the float64 restatement of the split layer step (tests/seg_nodewise_ref.py) against float64 autograd of the dense expression
  relu(batch_norm(conv1x1(cat(...)))): forward and every gradient to 1e-12, on narrowed blocks in the model's block order with one
  empty node -- and five deliberately wrong steps, each of which the comparison sees;
* the numpy restatement of the device's ascending-order f32 node sum;
* the C entries and the wrappers refuse bad arguments before any launch;
* how the option is read, and that the blocks of ``Segmenter._layer1_split_train`` cover the weight's columns in order."""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

import seg_nodewise_ref as R

TOL = 1e-12        # float64 against float64: the two evaluation orders differ by a few ulp of sums of <= 240 terms of size <= 10


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("seed", [0, 1])
def test_split_step_is_the_dense_expression(seed, relu):
    c = R.make_case(seed)
    assert not (c["ids"] == 2).any() and (c["ids"] == 3).any() and c["L"] == 120 and c["M"] == 4           # one empty node
    y, want = R.dense_step(c, relu)
    y2, got = R.split_step(c, relu)
    assert float((y - y2).abs().max()) <= TOL * max(1.0, float(y.abs().max()))
    assert sorted(got) == sorted(R.WITH_GRAD + ("W", "gamma", "beta")) and got["W"].shape == (8, sum(R.SMALL_WIDTHS.values()))
    assert R.worst_difference(got, want) <= TOL, {k: float((got[k] - want[k]).abs().max()) for k in want}
    # the empty node's rows of the node-level gradients are exactly zero
    for k in ("fm_first", "fm_knn", "fm_final"):
        assert float(got[k][:, :, 2].abs().max()) == 0.0 and float(want[k][:, :, 2].abs().max()) == 0.0


@pytest.mark.parametrize("brk", R.BREAKS)
def test_every_deliberate_break_is_seen(brk):
    c = R.make_case(0)
    _, want = R.dense_step(c)
    _, got = R.split_step(c, brk=brk)
    assert R.worst_difference(got, want) > 1e-6, brk
    assert R.worst_difference(R.split_step(c)[1], want) <= TOL


def test_block_order_is_the_models():
    from models import networks as NW
    opt = Namespace(feature_num=1024, surface_normal=True, som_k=9, activation="relu", normalization="batch", dropout=0.0, classes=50,
                    k=3, input_pc_num=64)
    seg = NW.Segmenter(opt)
    blk = seg._layer1_blocks()
    assert tuple(blk) == R.ORDER
    full = dict(x_dec=3, x=3, centers=3, sn=3, onehot=16, first=384, fm_first=384, fm_knn=512, fm_final=1024, feature=1024)
    assert blk == R.blocks(full) and blk["feature"][1] == 3356 == seg.layer1.conv.in_channels
    assert sum(full[n] for n in R.PER_COLUMN) == 393 and sum(full[n] for n in R.PER_NODE) == 1923 and sum(full[n] for n in R.PER_CLOUD) == 1040


def test_node_sum_restatement():
    g = np.random.default_rng(5)
    B, C, L, M = 2, 3, 50, 5
    x = g.standard_normal((B, C, L)).astype(np.float32)
    ids = g.integers(-1, M + 1, (B, L)).astype(np.int32)                      # -1 and M: nowhere
    ids[ids == 2] = 3                                                         # node 2 stays empty
    gz = R.node_sum_f32(x, ids, M)
    assert gz.dtype == np.float32 and not gz[:, :, 2].any()
    ref = np.zeros((B, C, M))
    for b in range(B):
        for l in range(L):
            if 0 <= ids[b, l] < M:
                ref[b, :, ids[b, l]] += x[b, :, l]
    assert np.abs(gz - ref).max() <= L * 2.0 ** -24 * np.abs(x).sum(axis=2).max()
    # the order is part of the contract: one chain, ascending -- 1 + 2^-24 + 2^-24 stays 1 from the left, not from the right
    t = np.array([[[1.0, 2.0 ** -24, 2.0 ** -24]]], dtype=np.float32)
    assert R.node_sum_f32(t, np.zeros((1, 3), np.int32), 1)[0, 0, 0] == np.float32(1.0)
    assert R.node_sum_f32(t[:, :, ::-1], np.zeros((1, 3), np.int32), 1)[0, 0, 0] > np.float32(1.0)
    # a NaN stays in its own sum
    x[0, 1, 7] = np.nan
    ids[0, 7] = 1
    gz = R.node_sum_f32(x, ids, M)
    assert np.isnan(gz[0, 1, 1]) and np.isnan(gz).sum() == 1


def test_c_entries_refuse_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INV, UNS = 1, 2

    def refused(st, code, word):
        assert st == code and word in _lib.last_error(), (st, _lib.last_error())

    ns = lib.sonet_pointwise_bwd_apply_nodesum_f32
    good = [p, p, p, p, 1, p, p, p, p, 4, p, p, p, 1, 1, 1, None]
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12):                            # every pointer in turn
        refused(ns(*[None if j == i else a for j, a in enumerate(good)]), INV, "NULL")
    for i in (9, 13, 14, 15):                                                 # M, B, C, L
        for v in (0, -1):
            refused(ns(*[v if j == i else a for j, a in enumerate(good)]), INV, "bad size")
    refused(ns(*[1025 if j == 9 else a for j, a in enumerate(good)]), UNS, "1024")
    assert lib.sonet_pointwise_bwd_apply_nodesum_ws_size(2, 3, 5) == lib.sonet_node_gather_bwd_ws_size(2, 3, 5) == (2 * 4 + 2 * 5) * 4
    assert lib.sonet_pointwise_bwd_apply_nodesum_ws_size(0, 3, 5) == 0
    tile = lib.sonet_pointwise_bwd_apply_nodesum_tile()
    assert tile >= 64 and tile % 4 == 0

    fs = lib.sonet_pointmlp_h3_nodeadd_stats_f32
    good = [p, 16, None, 0, p, p, p, 0, p, 1, 32, 1, p, p, 1, p, p, p, None]
    for i in (0, 4, 5, 6, 8, 12, 13, 15, 16, 17):
        refused(fs(*[None if j == i else a for j, a in enumerate(good)]), INV, "NULL")
    refused(fs(*[0 if j == 14 else a for j, a in enumerate(good)]), INV, "ZM")
    for i in (1, 9, 10, 11):                                                  # C1, B, Cout, L
        refused(fs(*[0 if j == i else a for j, a in enumerate(good)]), INV, "")
    refused(fs(*[48 if j == 10 else a for j, a in enumerate(good)]), UNS, "multiple of 32")


def test_wrappers_refuse_wrong_tensors_without_a_device():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    gy, v = torch.zeros(2, 3, 8), torch.ones(3)
    ids = torch.zeros(2, 8, dtype=torch.int32)
    cases = [
        (lambda: ops.pointwise_bwd_apply_nodesum(gy, gy, v, v, True, v, v, v, ids, 1025), "1 <= M <= 1024"),
        (lambda: ops.pointwise_bwd_apply_nodesum(gy, gy, v, v, True, v, v, v, ids, 0), "1 <= M <= 1024"),
        (lambda: ops.pointwise_bwd_apply_nodesum(gy, gy, v, v, True, v, v, v, ids[:, :7], 4), "ids must have shape"),
        (lambda: ops.pointwise_bwd_apply_nodesum(gy, gy, v, v, True, v, v, v, ids.long(), 4), "ids must be torch.int32"),
        (lambda: ops.pointwise_bwd_apply_nodesum(gy[0], gy, v, v, True, v, v, v, ids, 4), "3-D"),
        (lambda: ops.pointwise_bwd_apply_nodesum(gy, gy, v, v, True, v, v, v, ids, 4), "CUDA"),          # everything right but the device
        (lambda: ops.pointmlp_nodeadd_stats(gy, torch.zeros(8, dtype=torch.uint8), v, 32, gy, ids), "an h3 pack"),      # an x3 pack
        (lambda: ops.pointmlp_nodeadd_stats(gy, torch.zeros(8, dtype=torch.int16), v, 32, gy, ids), "an h3 pack"),      # a bf16 pack
        (lambda: ops.pointmlp_nodeadd_stats(gy, torch.zeros(8, dtype=torch.int8), v, 32, gy, ids), "CUDA"),
    ]
    for n, (call, word) in enumerate(cases):
        with pytest.raises(SonetHipError) as e:
            call()
        assert word in str(e.value), (n, str(e.value))


def test_the_option_is_read_with_getattr_and_defaults_to_off():
    from models import networks as NW
    base = dict(feature_num=1024, surface_normal=True, som_k=9, activation="relu", normalization="batch", dropout=0.0, classes=50, k=3,
                input_pc_num=64)
    seg = NW.Segmenter(Namespace(**base)).train()
    assert not hasattr(seg.opt, "seg_nodewise_train") and seg._nodewise_train_ok() is False
    for value in (False, 0, None):
        assert NW.Segmenter(Namespace(seg_nodewise_train=value, **base)).train()._nodewise_train_ok() is False
    # set, but on a CPU model / in eval mode / without autograd: still the dense branch (the remaining conditions need the device)
    on = NW.Segmenter(Namespace(seg_nodewise_train=True, **base))
    assert on.train()._nodewise_train_ok() is False                          # (weights on the CPU)
    assert on.eval()._nodewise_train_ok() is False
    with torch.no_grad():
        assert on.train()._nodewise_train_ok() is False
