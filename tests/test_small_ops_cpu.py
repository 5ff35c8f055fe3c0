"""tests/small_ops_ref.py without a GPU: the restatements against the reference's torch expressions on the CPU, the float64 fma model's tie
counts on every seeded input, the restatements' deliberate breaks against the seeded inputs, and the argument checks of the C entries and
``ops`` wrappers (through the library, no device)."""
import ctypes

import numpy as np
import pytest
import torch

import small_ops_ref as R

T = torch.from_numpy


def _t64(a):
    return T(np.asarray(a, np.float64))


def _close64(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what


# ---------------------------------------------------------------------------------------------- restatements against torch
def _torch_knn_gather(x, I):
    """models/operations.py:38-54: the index expanded over the channels, torch.gather along the node axis."""
    B, C, M = x.shape
    K = I.shape[2]
    return torch.gather(x, 2, I.unsqueeze(1).expand(B, C, M, K).reshape(B, C, M * K)).view(B, C, M, K)


@pytest.mark.parametrize("B,C,M,K", [(3, 5, 85, 3), (1, 1, 1, 1), (2, 4, 29, 9)])
def test_gathers_and_grouping_equal_the_torch_expressions(B, C, M, K):
    coord, feat, I = R.knn_inputs(B, C, M, K, oor=False)
    assert R.same_bits(R.gather(feat, I), _torch_knn_gather(T(feat), T(I)).numpy())
    # models/layers.py:346-361, 'center': the same single subtraction -> bit-equal
    nb = _torch_knn_gather(T(coord), T(I))
    ctr, out = R.knn_group(coord, feat, I, avg=False)
    assert R.same_bits(ctr, coord)
    assert R.same_bits(out, torch.cat((nb - T(coord).unsqueeze(3), _torch_knn_gather(T(feat), T(I))), dim=1).numpy())
    # 'avg': torch.mean sums in its own order -> the same expression in float64, 1e-12
    c64, f64 = coord.astype(np.float64), feat.astype(np.float64)
    nb64 = _torch_knn_gather(T(c64), T(I))
    mean = torch.mean(nb64, dim=3, keepdim=True)
    ctr, out = R.knn_group(c64, f64, I, avg=True)
    assert ctr.dtype == np.float64
    _close64(ctr, mean.squeeze(3).numpy(), "centre")
    _close64(out, torch.cat((nb64 - mean, _torch_knn_gather(T(f64), T(I))), dim=1).numpy(), "grouped")
    # knn_prepare is knn_group's coordinate rows k-major
    for avg in (False, True):
        ctr, out = R.knn_group(coord, feat, I, avg)
        pc, dec, gidx = R.knn_prepare(coord, I, avg)
        assert R.same_bits(pc, ctr) and R.same_bits(dec.reshape(B, 3, K, M).transpose(0, 1, 3, 2), out[:, :3])
        assert np.array_equal(gidx.reshape(B, K, M).transpose(0, 2, 1), I)


def test_node_gather_and_mask_equal_the_torch_expressions():
    g = np.random.default_rng(0)
    B, C, M, kN = 3, 5, 7, 41
    feat, ids = g.standard_normal((B, C, M)).astype(np.float32), R.node_ids(g, B, kN, M, oor=False)
    # models/segmenter.py:90-98: arg-max of the one-hot mask, expanded over the channels, torch.gather
    mask = R.som_mask(ids, M)
    onehot = (T(ids).long().unsqueeze(2) == torch.arange(M).view(1, 1, M)).int()
    assert np.array_equal(mask, onehot.numpy()) and mask.dtype == np.int32
    _, idx = torch.max(T(mask), dim=2)
    ref = torch.gather(T(feat), 2, idx.unsqueeze(1).expand(B, C, kN))
    assert R.same_bits(R.gather(feat, ids), ref.numpy())
    assert not R.som_mask(np.array([[-1, M, R.INT32_MIN]], np.int32), M).any()


def test_fma_kernels_equal_the_float64_expressions():
    d = R.fma_case_inputs(3, 5, 300, 64, 3, False)
    d["ids"] = np.abs(d["ids"].astype(np.int64)) % 64          # in range
    B, C, L = d["t"].shape
    idx = T(d["ids"]).unsqueeze(1).expand(B, C, L)
    zg = torch.gather(_t64(d["z"]), 2, idx)
    sc, sh = _t64(d["sc"]).view(1, C, 1), _t64(d["sh"]).view(1, C, 1)
    # models/networks.py:296-326: the per-node block of layer 1 added to the per-point block, then BatchNorm's affine and ReLU
    ref = torch.clamp((_t64(d["t"]) + zg) * sc + sh, min=0)
    _close64(R.node_add_affine_act(d["t"], d["z"], d["ids"], d["sc"], d["sh"], True, dtype=np.float64), ref.numpy(), "node_add_affine_act")
    # models/layers.py:313-350: a layer over (de-centred coordinates | gathered features) = gathered W_f x + W_l . coordinates
    pre = (zg + torch.einsum("ci,bil->bcl", _t64(d["wl"]), _t64(d["lead"]))) * sc + sh
    for relu in (False, True):
        got = R.node_gather_lead(d["z"], d["ids"], d["lead"], d["wl"], d["sc"], d["sh"], relu, dtype=np.float64)
        _close64(got, (torch.clamp(pre, min=0) if relu else pre).numpy(), "node_gather_lead")
    # ... and the f32 restatement is that value to two / five roundings
    got = R.node_gather_lead(d["z"], d["ids"], d["lead"], d["wl"], d["sc"], d["sh"], False)
    mag = (zg.abs() + torch.einsum("ci,bil->bcl", _t64(d["wl"]).abs(), _t64(d["lead"]).abs())) * sc.abs() + sh.abs()
    assert (np.abs(got.astype(np.float64) - pre.numpy()) <= 5 * R.U24 * mag.numpy()).all()


def test_maxima_equal_torch_max():
    for rows, K in ((17, 9), (5, 64), (3, 1)):
        x = R.lastdim_inputs(rows, K)
        assert R.same_bits(R.lastdim_max(x), torch.max(T(x), dim=-1)[0].numpy())
    x = R.lastdim_inputs(6, 27).reshape(2, 3, 27)
    assert R.same_bits(R.planes_max(x, 9), torch.max(T(x).view(2, 3, 9, 3), dim=2)[0].numpy())
    for bf16 in (False, True):
        x = R.argmax_inputs(9, 7, bf16)
        val, idx = R.lastdim_argmax(x)
        tv, ti = torch.max(T(x), dim=-1)
        assert R.same_bits(val, tv.numpy())
        unique = ((x == val[:, None]) | (np.isnan(x) & np.isnan(val)[:, None])).sum(-1) == 1
        assert unique.sum() >= 4 and np.array_equal(idx[unique], ti.numpy()[unique])
        assert idx[0] == 1 and idx[1] == 0 and idx[2] == 0 and idx[3] == 0          # first NaN, -inf row, equal row, first of two maxima
        gy = np.arange(1, 10, dtype=np.float32)
        gx = R.lastdim_max_bwd(gy, idx, 7)
        assert gx.dtype == np.float32 and (gx.sum(-1) == gy).all() and (np.count_nonzero(gx, axis=-1) == 1).all()
        xt = T(x[unique]).clone().requires_grad_(True)
        torch.max(xt, dim=-1)[0].backward(T(gy[unique]))
        assert R.same_bits(gx[unique], xt.grad.numpy())


@pytest.mark.parametrize("B,C,M,K", [(2, 3, 64, 9), (3, 17, 30, 5), (1, 4, 1, 1)])
def test_backward_gathers_equal_scatter_add_in_float64(B, C, M, K):
    g = np.random.default_rng([B, C, M, K])
    _, _, I = R.knn_inputs(B, C, M, K, oor=False)
    gy = g.standard_normal((B, C, M, K))
    ref = torch.zeros(B, C, M, dtype=torch.float64)
    ref.scatter_add_(2, T(I).reshape(B, 1, M * K).expand(B, C, M * K), T(gy).reshape(B, C, M * K))
    got = R.knn_gather_bwd(gy, I, M)
    assert got.dtype == np.float64
    _close64(got, ref.numpy(), "knn_gather_bwd")
    ids = R.node_ids(g, B, M * K, M, oor=False)
    ref = torch.zeros(B, C, M, dtype=torch.float64)
    ref.scatter_add_(2, T(ids).long().unsqueeze(1).expand(B, C, M * K), T(gy).reshape(B, C, M * K))
    _close64(R.node_gather_bwd(gy.reshape(B, C, M * K), ids, M), ref.numpy(), "node_gather_bwd")
    # out-of-range entries belong to nobody, an empty node gives +0.0, f32 in -> f32 out
    I2 = np.full((1, 2, 2), 1, np.int64)
    I2[0, 0, 0], I2[0, 1, 1] = -1, 2 ** 32 + 1
    gx = R.knn_gather_bwd(np.array([[[[1, 2], [4, 8]]]], np.float32), I2, 2)
    assert gx.dtype == np.float32 and gx.tolist() == [[[0.0, 6.0]]] and not np.signbit(gx).any()


def test_adam_restatement_is_the_float64_expression_to_its_counted_roundings():
    """One step from the same f32 state, f32 against float64 (the scalars are the kernel's f32 values in both).  Roundings, u = 2^-24:
    m' = m + w1 (g - m): three (d, the product, the sum): |dm| <= u (2 w1 |d| + |m'|) <= 3 u (|m| + w1 |d|).
    v' = v b2 + (w2 g) g: every term is non-negative and passes through at most three roundings: |dv| <= 3 u v'.
    denom = sqrt(v') / bs + eps: 1.5 u from v', one each for sqrt, the division and the sum (all terms positive): 4.5 u, counted as 5.
    p' = p + (-ss) (m' / denom): the quotient carries dm / denom and (5 + 1) u of itself, the product one more, the sum u |p'|:
    |dp| <= ss (dm + 7 u |m'|) / denom + u |p'|.  1 % on top for the second-order terms."""
    params, grads = R.adam_inputs()
    u = R.U24
    for t in (0, 1, 4, 5):                                     # (the tensors without planted values)
        p, m, v = params[t], np.zeros_like(params[t]), np.zeros_like(params[t])
        for s in range(R.ADAM_STEPS):
            gr = grads[s][t]
            p32, m32, v32 = R.adam_step(p, gr, m, v, s + 1)
            p64, m64, v64 = R.adam_step(p, gr, m, v, s + 1, dtype=np.float64)
            assert p32.dtype == np.float32 and p64.dtype == np.float64
            c = R.adam_scalars(s + 1.0, 1e-3, 0.9, 0.999, 1e-8)
            bm = 3 * u * (np.abs(m) + float(c["w1"]) * np.abs(gr.astype(np.float64) - m)) * 1.01
            denom = np.sqrt(v64) / float(c["bs"]) + float(c["eps"])
            bp = (float(c["ss"]) * (bm + 7 * u * np.abs(m64)) / denom + u * np.abs(p64)) * 1.01
            assert (np.abs(m32 - m64) <= bm).all() and (np.abs(v32 - v64) <= 3.03 * u * v64).all()
            assert (np.abs(p32 - p64) <= bp).all(), (t, s, float((np.abs(p32 - p64) / bp).max()))
            p, m, v = p32, m32, v32


def test_adam_planted_elements():
    params, grads = R.adam_inputs()
    run = R.adam_run(params, grads)
    (th, eh), (to, eo), (tn, en) = R.ADAM_HUGE, R.ADAM_OVERFLOW, R.ADAM_NAN
    for s in range(R.ADAM_STEPS):
        p, m, v = run[s][to]
        assert np.isinf(v[eo]) and p[eo] == params[to][eo]      # g^2 overflows: the update is -ss (m / inf) = -+0
        assert np.isfinite(run[s][th][2][eh])                   # at g = 1e20 (w2 g) g = 1e37 is still finite in the kernel's order
        p, m, v = run[s][tn]
        assert np.isnan(p[en]) and np.isnan(m[en]) and np.isnan(v[en]) and np.isnan(p).sum() == 1
        p, m, v = run[s][R.ADAM_ZERO_GRAD]
        assert (m == 0).all() and (v == 0).all() and np.array_equal(p, params[R.ADAM_ZERO_GRAD])   # 0 / eps
    ts, ss = R.ADAM_SKIPS
    assert all(np.array_equal(a, b) for a, b in zip(run[ss][ts], run[ss - 1][ts]))    # the skipped step changes nothing ...
    p, m, v = run[ss][ts]
    want = R.adam_step(p, grads[ss + 1][ts], m, v, ss + 1)      # ... and the next one counts from where the tensor was (step ss + 1, not ss + 2)
    assert all(np.array_equal(a, b) for a, b in zip(run[ss + 1][ts], want))


# ---------------------------------------------------------------------------------------------- tie counts
def test_no_seeded_input_of_the_fma_kernels_sits_on_a_rounding_tie():
    for (B, C, L, M) in R.NODE_ADD_SHAPES:
        d = R.node_add_inputs(B, C, L, M)
        for relu in (False, True):
            out, ties = R.node_add_affine_act(d["t"], d["z"], d["ids"], d["sc"], d["sh"], relu, want_ties=True)
            assert ties == 0, (B, C, L, M)
            assert out[0, 0, 0] == 0 and np.signbit(out[0, 0, 0]) and (np.isnan(out).sum() == 1) == (d["nan_at"] != (0, 0, 0))
    for (B, C, L, M, NL) in R.LEAD_SHAPES:
        for bf16 in (False, True):
            d = R.fma_case_inputs(B, C, L, M, NL, bf16)
            assert R.node_gather_lead(d["z"], d["ids"], d["lead"], d["wl"], d["sc"], d["sh"], True, bf16, want_ties=True)[1] == 0, (B, C, L, M, NL)


# ---------------------------------------------------------------------------------------------- the breaks turn the comparisons red
def test_seeded_inputs_tell_every_break_from_the_contract():
    # a dropped last entry of an inverse list
    for (B, C, M, K) in ((2, 3, 64, 9), (1, 4, 1, 1)):
        _, _, I = R.knn_inputs(B, C, M, K)
        gy = np.random.default_rng(1).standard_normal((B, C, M, K)).astype(np.float32)
        assert not R.same_bits(R.knn_gather_bwd(gy, I, M), R.knn_gather_bwd(gy, I, M, drop_last=True)) or not R.in_range(I, M)[1].any()
    # a centre divided by the number of in-range neighbours; an index truncated to 32 bits -- on EVERY seeded table with out-of-range entries
    for (B, C, M, K) in R.KNN_SHAPES:
        coord, feat, I = R.knn_inputs(B, C, M, K)
        ok = R.in_range(I, M)[1]
        mixed = (ok.any(-1) & ~ok.all(-1)).any()                # a node with both kinds of neighbour
        a, b = R.knn_group(coord, feat, I, True), R.knn_group(coord, feat, I, True, count_in_range=True)
        assert mixed == (not R.same_bits(a[0], b[0])), (B, C, M, K)
        alias = R.in_range(I, M, trunc32=True)[1] & ~ok
        assert alias.any() == (not R.same_bits(R.gather(feat, I), R.gather(feat, I, trunc32=True)))
    assert sum((R.in_range(R.knn_inputs(*s)[2], s[2], True)[1] & ~R.in_range(R.knn_inputs(*s)[2], s[2])[1]).any() for s in R.KNN_SHAPES) >= 12
    # a max that skips one lane's share
    for K, tpr in ((6, 4), (47, 4), (48, 16), (64, 16), (1000, 16)):
        x = R.lastdim_inputs(65, K)
        for q in range(tpr):
            assert not R.same_bits(R.lastdim_max(x), R.lastdim_max(x, skip=(tpr, q))), (K, q)
    # Adam's v with a fused multiply-add
    params, grads = R.adam_inputs()
    a, b = R.adam_run(params, grads), R.adam_run(params, grads, fma_v=True)
    assert R.same_bits(a[0][4][2], b[0][4][2])                  # (first step: v = 0, nothing to fuse)
    assert not R.same_bits(a[1][4][2], b[1][4][2]) and not R.same_bits(a[-1][4][0], b[-1][4][0])
    # a dropped last float4 of a linear_act row
    for Cin in (5, 63, 65, 1023, 1025, 1793):
        d = R.linear_inputs(17, Cin, 9)
        y, bound = R.linear_act(d["x"], d["W"], d["sc"], d["sh"], False)
        assert (np.abs(R.linear_act(d["x"], d["W"], d["sc"], d["sh"], False, drop_tail=True)[0] - y) > bound).any(), Cin


def test_linear_bound_holds_for_a_plain_f32_evaluation_and_counts_the_chain():
    assert [R.linear_chain(c) for c in (1, 3, 4, 5, 17, 63, 64, 65, 1024, 4096)] == [1, 3, 4, 4, 4, 4, 4, 5, 64, 256]
    for Cin in (5, 65, 1025):
        d = R.linear_inputs(16, Cin, 8)
        y, bound = R.linear_act(d["x"], d["W"], d["sc"], d["sh"], True)
        acc = np.zeros((16, 8), np.float32)
        for k in range(Cin):                                    # one sequential f32 chain, products rounded: 2 Cin roundings, not chain + 16
            acc = acc + d["x"][:, k:k + 1] * d["W"][:, k][None, :]
        got = np.maximum(acc * d["sc"] + d["sh"], 0)            # (two more: the same form of bound with 2 Cin + 2 + 1 in place of chain + 16 + 2)
        assert (np.abs(got - y) <= bound * (2 * Cin + 3) / (R.linear_chain(Cin) + 18)).all()


# ---------------------------------------------------------------------------------------------- rejections, no device
def test_c_entries_refuse_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 4)                          # 4-byte offset into the buffer
    INV, UNS = 1, 2

    def refused(st, code, word):
        assert st == code and word in _lib.last_error(), (st, _lib.last_error())

    refused(lib.sonet_knn_gather_f32(None, p, p, 1, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_knn_gather_f32(p, p, p, 1, 1, 0, 1, None), INV, "non-positive")
    refused(lib.sonet_knn_group_f32(p, p, p, 1, 1, 1, 1, 1, None, p, None), INV, "NULL")
    refused(lib.sonet_knn_group_f32(p, p, p, 1, 1, 1, 0, 1, p, p, None), INV, "non-positive")
    refused(lib.sonet_knn_prepare_f32(p, p, 1, 1, 1, 1, p, p, None, None), INV, "NULL")
    refused(lib.sonet_knn_prepare_f32(p, p, 0, 1, 1, 1, p, p, p, None), INV, "non-positive")
    refused(lib.sonet_lastdim_max_f32(p, None, 1, 1, None), INV, "NULL")
    refused(lib.sonet_lastdim_max_f32(p, p, 0, 1, None), INV, "non-positive")
    refused(lib.sonet_planes_max_f32(None, p, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_planes_max_f32(p, p, 1, 0, 1, None), INV, "non-positive")
    refused(lib.sonet_lastdim_argmax_f32(p, p, None, 1, 1, None), INV, "NULL")
    refused(lib.sonet_lastdim_argmax_bf16(p, p, p, 1, 0, None), INV, "bad size")
    refused(lib.sonet_lastdim_max_bwd_f32(None, p, p, 1, 1, None), INV, "NULL")
    refused(lib.sonet_lastdim_max_bwd_bf16(p, p, p, -1, 1, None), INV, "bad size")
    refused(lib.sonet_som_mask_i32(p, None, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_som_mask_i32(p, p, 1, 1, 0, None), INV, "non-positive")
    refused(lib.sonet_node_gather_f32(p, None, p, 1, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_node_gather_f32(p, p, p, 1, 1, 1, 0, None), INV, "non-positive")
    for fn in (lib.sonet_knn_gather_bwd_f32, lib.sonet_knn_gather_bwd_bf16, lib.sonet_node_gather_bwd_f32, lib.sonet_node_gather_bwd_bf16):
        refused(fn(p, p, p, None, 1, 1, 1, 1, None), INV, "NULL")
        refused(fn(p, p, p, p, 1, 0, 1, 1, None), INV, "bad size")
        refused(fn(p, p, p, p, 1, 1, 1025, 1, None), UNS, "1024")
    for fn in (lib.sonet_knn_gather_bwd_f32, lib.sonet_knn_gather_bwd_bf16):
        refused(fn(p, p, p, p, 1, 1, 1024, 15, None), UNS, "LDS")           # 15360 indices: 60 KiB
        refused(fn(p, p, p, p, 1, 1, 243, 59, None), UNS, "LDS")            # M K = 14337: one index past 56 KiB
        refused(fn(p, p, p, p, 1, 1, 14337, 1, None), UNS, "1024")
    assert lib.sonet_knn_gather_bwd_ws_size(2, 3, 4) == (2 * 4 + 2 * 12) * 4 and lib.sonet_knn_gather_bwd_ws_size(0, 3, 4) == 0
    assert lib.sonet_node_gather_bwd_ws_size(2, 3, 5) == (2 * 4 + 2 * 5) * 4
    refused(lib.sonet_node_add_affine_act_f32(p, p, p, p, None, 1, 1, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_node_add_affine_act_f32(p, p, p, p, p, 1, 1, 1, 0, 1, None), INV, "bad size")
    refused(lib.sonet_node_add_affine_act_f32(p, p, p, p, p, 1, 1, 1, 1, 8193, None), INV, "M=8193")
    for fn in (lib.sonet_node_gather_lead_affine_act_f32, lib.sonet_node_gather_lead_affine_act_bf16):
        refused(fn(p, p, None, p, p, p, 1, p, 1, 1, 1, 1, 1, None), INV, "NULL")
        refused(fn(p, p, p, p, p, p, 1, p, 1, 1, 1, 1, 5, None), INV, "NL=5")
        refused(fn(p, p, p, p, p, p, 1, p, 1, 1, 1, 1025, 1, None), INV, "M=1025")
        refused(fn(p, off, p, p, p, p, 1, p, 1, 1, 4, 1, 1, None), INV, "misaligned")      # quad path: gidx at a 4-byte offset
        refused(fn(p, p, off, p, p, p, 1, p, 1, 1, 4, 1, 1, None), INV, "misaligned")      # ... lead
    refused(lib.sonet_linear_act_f32(p, p, p, p, 1, None, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_linear_act_f32(p, p, p, p, 1, p, 1, 0, 1, None), INV, "non-positive")
    refused(lib.sonet_linear_act_f32(p, p, p, p, 1, p, 1, 4097, 1, None), UNS, "4097")
    refused(lib.sonet_linear_act_f32(off, p, p, p, 1, p, 1, 4, 1, None), INV, "misaligned")
    refused(lib.sonet_linear_act_f32(p, off, p, p, 1, p, 1, 4, 1, None), INV, "misaligned")
    refused(lib.sonet_knn_self_f32(p, None, 1, 1, 1, None), INV, "NULL")
    refused(lib.sonet_knn_self_f32(p, p, 1, 20, 17, None), UNS, "K=17")
    refused(lib.sonet_knn_self_f32(p, p, 1, 4, 5, None), INV, "K=5")
    refused(lib.sonet_adam_multi_f32(p, p, p, p, p, None, 1, 0.9, 0.999, 0.1, 0.001, 1e-8, None), INV, "NULL")
    refused(lib.sonet_adam_multi_f32(p, p, p, p, p, p, 0, 0.9, 0.999, 0.1, 0.001, 1e-8, None), INV, "no chunks")
    assert lib.sonet_adam_chunk() == 4096


def test_ops_wrappers_refuse_wrong_tensors_without_a_device():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    f, i64, i32 = torch.zeros(1, 3, 4), torch.zeros(1, 4, 2, dtype=torch.int64), torch.zeros(1, 8, dtype=torch.int32)
    v = torch.ones(3)
    calls = [lambda: ops.knn_gather(f, i64), lambda: ops.knn_group(f, f, i64, True), lambda: ops.knn_prepare(f, i64, True),
             lambda: ops.lastdim_max(f), lambda: ops.planes_max(f, 2), lambda: ops.som_mask(i32, 4), lambda: ops.node_gather(f, i32),
             lambda: ops.knn_gather_bwd(torch.zeros(1, 3, 4, 2), i64, 4), lambda: ops.node_gather_bwd(torch.zeros(1, 3, 8), i32, 4),
             lambda: ops.node_add_affine_act_(torch.zeros(1, 3, 8), f, i32, v, v, True),
             lambda: ops.node_gather_lead_affine_act(f, i32, torch.zeros(1, 2, 8), torch.zeros(3, 2), v, v, True),
             lambda: ops.linear_act(torch.zeros(2, 4), torch.zeros(3, 4), v, v, True), lambda: ops.knn_self(f, 2),
             lambda: ops.knn_gather_bwd(torch.zeros(1, 3, 4, 2, dtype=torch.float16), i64, 4),
             lambda: ops.node_gather_bwd(torch.zeros(1, 3, 8, dtype=torch.float64), i32, 4)]
    for n, call in enumerate(calls):
        with pytest.raises(SonetHipError):
            call()
            pytest.fail("call %d went through on CPU tensors" % n)
    # the alignment helper: a contiguous view at a 4-byte offset is copied, an aligned tensor is handed through
    buf = torch.arange(64, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:33].view(4, 8)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    fixed = ops._aligned16(view)
    assert fixed.data_ptr() % 16 == 0 and torch.equal(fixed, view) and fixed.is_contiguous()
    assert ops._aligned16(buf) is buf and ops._aligned16(buf[4:]).data_ptr() == buf[4:].data_ptr()
