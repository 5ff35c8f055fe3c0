"""tests/fused_pointnet_ref.py without a GPU: the exact networks are exact by DERIVATION (every fp16 piece, every sum, every affine result
restated from the split of tests/h3_model.py, flavour "h3p"), the networks and layouts can see the mistakes they are meant to see, the
continuous network's split arithmetic keeps half of the project's 1e-5 gate, the restatements agree with torch and with the oracle's
grouping, and the C entries and ``ops`` wrappers of the fused first PointNet refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import fused_pointnet_ref as R
import h3_model as H
from conftest import assert_close_rms

NETS = [(fl, cin0, "half") for fl in "AB" for cin0 in R.CIN0S] + [("A", 6, "unit"), ("A", 6, "mixed")]
CUS = 256                                                   # (the layouts depend on the device only through the number of small clouds)


def _lowest_bit(a):
    """The largest power of two that divides every non-zero element of a float array (its granule); inf for an all-zero array."""
    a = np.asarray(a, np.float64)
    a = a[a != 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    return float(np.min(np.ldexp((mi & -mi).astype(np.float64), e - 53)))


# ---------------------------------------------------------------------------------------------- exact by derivation
@pytest.mark.parametrize("flavour,cin0,l4", NETS)
def test_exact_networks_are_exact_by_derivation(flavour, cin0, l4):
    net = R.exact_network(cin0, flavour, l4)
    x = net.pool[None]                                      # every column an input of this network can hold
    y, recs = R.split_forward(x, *net.Ws, net.affine)
    for i, r in enumerate(recs):
        what = "%s layer %d" % (net.name, i + 1)
        x64, w64 = r["x"].astype(np.float64), r["w"].astype(np.float64)
        Xh, Xm, Wh, Wr = (r[k].astype(np.float64) for k in ("Xh", "Xm", "Wh", "Wr"))
        # the two pieces of every operand are the operand: nothing is lost in either rounding
        assert np.array_equal(Xh + Xm, 32.0 * x64), what
        assert np.array_equal(Wh + Wr, 32.0 * w64), what
        # the term the kernel drops, Wr . Xm, is zero pair by pair: no (output row, input channel, column) has both residuals
        wr_rows, xm_rows = (Wr != 0).any(axis=0), (Xm != 0).any(axis=(0, 2))
        assert not (wr_rows & xm_rows).any(), what
        # operand range: inside the fp16 split's clamp and above the guard's lower limits (ops.py)
        assert np.abs(x64).max() <= 2047.0 and np.abs(w64).max() <= 2047.0, what
        assert np.abs(x64).max() >= H.X_LOW and np.abs(w64).max() >= H.W_LOW, what
        # every order of f32 accumulation is exact: all terms are multiples of one granule and the sum of their magnitudes stays below
        # 2^24 granules (so does every partial sum, in any order, inside an MFMA or between two)
        gran = min(_lowest_bit(Wh), _lowest_bit(Wr)) * min(_lowest_bit(Xh), _lowest_bit(Xm))
        assert r["sum_abs"].max() / gran < 2.0 ** 24, (what, r["sum_abs"].max() / gran)
        # the affine's fma rounds nothing: its exact result is a float32 (32 x for the hidden layers, y for layer 4)
        assert np.array_equal(r["pre"].astype(np.float32).astype(np.float64), r["pre"]), what
        if i < 3:                                            # ... and the hidden activations carry the residual pieces they are meant to
            act = np.maximum(r["pre"], 0.0) / 32.0
            assert act.max() <= 2047.0, what
    assert (recs[0]["Wr"] != 0).any() == (flavour == "B")                          # B: the weight residual slice of layer 1 is in use
    assert all((r["Wr"] == 0).all() for r in recs[1:])
    assert (recs[0]["Xm"] == 0).all() and all((r["Xm"] != 0).any() for r in recs[1:])   # the activation residual pieces are in use
    # so the kernel's arithmetic IS the float64 network, and the outputs are float32 numbers
    ref = net.ref(x)
    assert np.array_equal(y, ref)
    R.f32_exact(ref)
    assert np.abs(ref).max() <= 2047.0                      # (the P16 planes of y are not clamped either)


# ---------------------------------------------------------------------------------------------- the networks can see a mistake
@pytest.mark.parametrize("flavour,cin0,l4", NETS)
def test_exact_networks_tell_channels_apart(flavour, cin0, l4):
    net = R.exact_network(cin0, flavour, l4)
    x = net.make_x(2, 257, seed=1)                          # the smallest store case that runs every network
    y, hid = net.ref(x, hidden=True)
    for i, a in enumerate(hid):
        rows = np.transpose(a, (1, 0, 2)).reshape(a.shape[1], -1)
        assert len(np.unique(rows, axis=0)) == rows.shape[0], "%s: two channels of layer %d agree on every test column" % (net.name, i + 1)
        active = float((rows > 0).mean())
        assert 0.25 <= active <= 0.75, (net.name, i + 1, active)
    for i, W in enumerate(net.Ws[1:]):
        assert len(np.unique(W.T, axis=0)) == W.shape[1], "%s: two input channels of layer %d have the same weights" % (net.name, i + 2)
    for brk in R.BREAKS_FORWARD:
        assert not np.array_equal(net.ref(x, brk=brk), y), brk


@pytest.mark.parametrize("flavour,cin0,l4", [("A", 6, "mixed"), ("B", 9, "half")])
def test_the_gathered_reference_is_the_reference(flavour, cin0, l4):
    """x_and_ref (forward64 once over the pool's columns, gathered per case) == forward64 of the case's own input."""
    net = R.exact_network(cin0, flavour, l4)
    x, ref = net.x_and_ref(3, 300, seed=1)
    assert np.array_equal(x, net.make_x(3, 300, seed=1)) and ref.dtype == np.float32
    assert np.array_equal(ref.astype(np.float64), net.ref(x))


def test_pool_cases_hold_the_minus_1000_rule_and_see_every_break():
    net = R.exact_network(6, "A", "unit")
    seen = dict.fromkeys(R.BREAKS_POOL, 0)
    exact_m1000 = below = ge_rule = 0
    for name, (ids, pos0, M) in R.layouts(CUS).items():
        B, L = ids.shape
        assert (ids[:, 1:] >= ids[:, :-1]).all() and ids.min() >= 0 and ids.max() < M and (pos0 < L).all(), name
        y = net.ref(net.make_x(B, L, seed=3))
        out = R.pool64(y, ids, pos0, M)
        for brk in R.BREAKS_POOL:
            changed = (R.pool64(y, ids, pos0, M, brk=brk) != out).any(axis=(1, 2))
            seen[brk] += int(changed.sum())
            if brk == "boundary" and name == "two_nodes_every_boundary":
                assert changed.all(), "a boundary position the pooled values do not depend on"
            if brk == "slot16" and name == "tile_17_18_64_ids":
                assert changed.all()
        for b in range(B):
            for m in np.unique(ids[b]):
                mx = y[b][:, ids[b] == m].max(axis=1)
                exact_m1000 += int((mx == -1000.0).sum())
                below += int((mx < -1000.0).sum())
                # channel 0: the node's maximum is exactly -1000 while copy 0 holds another value -- '>=' would keep -1000
                if mx[0] == -1000.0 and y[b][0, pos0[b]] != -1000.0:
                    assert out[b][0, m] == y[b][0, pos0[b]]
                    assert R.pool64(y, ids, pos0, M, brk="ge")[b][0, m] == -1000.0
                    ge_rule += 1
        assert (out[:, 2] == -1000.0).all()                  # channel 2: pooled elements that equal -1000.0 exactly
    assert exact_m1000 > 0 and below > 0
    assert ge_rule > 0, "no node whose maximum is exactly -1000 while copy 0 holds another value: the rule at equality is never asked"
    assert all(n > 0 for n in seen.values()), seen


def test_layouts_reach_the_paths_they_name():
    lay = R.layouts(CUS)
    ids, _, _ = lay["tile_17_18_64_ids"]
    assert [len(np.unique(r)) for r in ids] == [17, 18, 64]
    ids, _, _ = lay["slot18_continues_as_slot0"]
    n = ids[0, R.TPTS]
    assert ids[0, R.TPTS - 1] == n and n - ids[0, 0] == 18 >= R.SEG_SLOTS          # slot = id - the tile's first id: beyond the LDS slots of tile 0, slot 0 of tile 1
    ids, _, _ = lay["ids_n_and_n_plus_20"]
    assert all(len(np.unique(r)) == 2 and r[-1] - r[0] == 20 for r in ids)
    ids, _, _ = lay["node_spans_four_tiles"]
    assert len({int(c) // R.TPTS for c in np.nonzero(ids[0] == 1)[0]}) == 4
    ids, _, M = lay["empty_nodes"]
    assert all(m not in ids for m in (0, 4, M - 1))
    ids, _, M = lay["persistent_small_clouds"]
    assert ids.shape == (CUS + 3, 40) and M == 4 and len({tuple(r) for r in ids}) > 3
    ids, _, _ = lay["ragged_last_tile"]
    assert ids.shape[1] % R.CTILE == 7 and len(np.unique(ids[0, 32:])) == 1 and len(np.unique(ids[1, 32:])) == 2


# ---------------------------------------------------------------------------------------------- the continuous case keeps the gate
@pytest.mark.parametrize("cin0,B,L", [(6, 2, 300), (6, 1, 1), (3, 2, 513)])
def test_continuous_split_arithmetic_keeps_half_the_gate(cin0, B, L):
    """The float64 model of the split, chained through the four layers, against the float64 network: 0.5e-5 of the project's 1e-5; the other
    half is left for the f32 accumulation of the matrix cores."""
    net, _ = R.continuous_network(cin0)
    x = net.make_x(B, L, seed=L)
    y, recs = R.split_forward(x, *net.Ws, net.affine)
    assert all(np.abs(r["x"]).max() <= 2047.0 for r in recs)
    print("split model %s: worst error / max(|ref|, rms) = %.3g" % ((B, cin0, L), R.rms_ratio(y, net.ref(x))))
    assert_close_rms(y, net.ref(x), 0.5e-5, "split model of the fused first PointNet %s" % ((B, cin0, L),))


@pytest.mark.parametrize("cin0", [6, 3])
def test_forward64_equals_the_torch_module_in_float64(cin0):
    net, pr = R.continuous_network(cin0)
    x = net.make_x(2, 77, seed=5)
    # the reference's data flow (models/layers.py:282-296, 419-432) in torch's own float64 operators: conv1d, eval-mode batch_norm, relu,
    # the skip channels first in the concatenation.  The module itself is NOT called: EquivariantLayer._prep raises on a CPU tensor and
    # there is no CPU path, so the order of the two panels is written by hand on both sides here.  The check that does not share that
    # hand is tests/test_gpu_fused_pointnet.py::test_forward64_is_the_module_layer_by_layer (PointResNet.forward on the device).
    import torch.nn.functional as F
    t = torch.from_numpy(x).double()

    def layer(lay, inp):
        v = F.conv1d(inp, lay.conv.weight, lay.conv.bias)
        if lay.normalization == "batch":
            v = F.batch_norm(v, lay.norm.running_mean, lay.norm.running_var, lay.norm.weight, lay.norm.bias, False, 0.0, lay.norm.eps)
        return F.relu(v) if lay.activation == "relu" else v
    with torch.no_grad():
        a1 = layer(pr.layers[0], t)
        a3 = layer(pr.layers[2], layer(pr.layers[1], a1))
        ref = layer(pr.layers[3], torch.cat((a1, a3), dim=1)).numpy()
    aff64 = _fold64(pr)                                     # (the network's float32 affine is this fold rounded once)
    got = R.forward64(x, *[l.conv.weight.detach().reshape(l.conv.out_channels, -1).numpy() for l in pr.layers], aff64)
    assert got.shape == ref.shape == (2, 384, 77)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(aff64 - net.affine).max() <= 2.0 ** -24 * np.abs(aff64).max()
    assert [tuple(W.shape) for W in net.Ws] == [(64, cin0), (128, 64), (256, 128), (384, 320)]


def _fold64(pr):
    sc, sh = [], []
    for lay in pr.layers:
        b = lay.conv.bias.detach() if lay.conv.bias is not None else torch.zeros(lay.conv.out_channels, dtype=torch.float64)
        if lay.normalization == "batch":
            s = lay.norm.weight.detach() / torch.sqrt(lay.norm.running_var + lay.norm.eps)
            h = (b - lay.norm.running_mean) * s + lay.norm.bias.detach()
        else:
            s, h = torch.ones_like(b), b
        sc.append(s.numpy())
        sh.append(h.numpy())
    return np.stack((np.concatenate(sc), np.concatenate(sh)), axis=1)


def test_sort_group_equals_the_oracle_grouping():
    from oracle import cpu_oracle as O
    from sonet_hip import synth
    B, N, M, k = 2, 200, 16, 3
    inp = synth.make_inputs(B, N, M=M, som_k=9, seed=11)
    pc, sn, node = inp["pc"].numpy(), inp["sn"].numpy(), inp["node"].numpy()
    min_idx, count, _ = O.som_query_topk(pc, node, k)
    _, _, xd = O.som_group(pc, min_idx, M, k)
    x_aug = np.concatenate((xd, np.tile(sn, (1, 1, k))), axis=1)                   # models/networks.py:160-171
    sg = R.sort_group(x_aug, min_idx, np.zeros(B, np.int64), M)
    ids = sg["ids_sorted"].numpy()
    assert sg["ids_sorted"].dtype == torch.int32 and (ids[:, 1:] >= ids[:, :-1]).all()
    assert np.array_equal(sg["count"].numpy(), count) and np.array_equal(np.sort(min_idx, axis=1), ids)
    assert np.array_equal(sg["node_off"].numpy(), np.cumsum(count, axis=1) - count)
    xs = sg["x_aug_sorted"].numpy()
    for b in range(B):
        assert np.array_equal(xs[b][:, int(sg["pos0"][b])], x_aug[b][:, 0])          # original copy 0
        off, cnt = sg["node_off"].numpy()[b], count[b]
        for m in range(M):                                                          # the node's columns, as a multiset
            got, ref = xs[b][:, off[m]:off[m] + cnt[m]], x_aug[b][:, min_idx[b] == m]
            assert np.array_equal(np.sort(got, axis=1), np.sort(ref, axis=1))
    # pool64 on the sorted copy == pool64 per node on the unsorted one
    y = np.random.default_rng(0).standard_normal((B, 5, k * N))
    ys = np.stack([y[b][:, np.argsort(min_idx[b], kind="stable")] for b in range(B)])
    ref = np.stack([np.stack([y[b][:, min_idx[b] == m].max(axis=1) if count[b, m] else y[b][:, 0] for m in range(M)], axis=1) for b in range(B)])
    assert np.array_equal(R.pool64(ys, ids, sg["pos0"].numpy(), M), ref)


def test_p16_planes_decode_to_the_values():
    y = np.random.default_rng(1).standard_normal((2, 40, 9)).astype(np.float32) * 50
    pl = R.p16_planes(y).view(np.float16).astype(np.float64)
    assert pl.shape == (2, 3, 2, 2, 9, 8)
    for h in range(2):
        for e in range(8):
            ch = 4 * h + (e & 3) + 8 * (e >> 2)
            dec = (pl[:, :, 0, h, :, e] + pl[:, :, 1, h, :, e]) / 32.0
            for kc in range(3):
                if 16 * kc + ch < 40:
                    assert np.abs(dec[:, kc] - y[:, 16 * kc + ch]).max() <= 2.0 ** -21 * 200
                else:
                    assert not dec[:, kc].any()


# ---------------------------------------------------------------------------------------------- refusals, no device
def test_c_entries_refuse_bad_arguments_before_any_launch():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INV, UNS = 1, 2

    def refused(st, code, word):
        assert st == code and word in _lib.last_error(), (st, _lib.last_error())

    store = lambda x=p, cin0=6, ws=p, aff=p, y=p, B=1, L=1: lib.sonet_pointresnet_fused_f32(x, cin0, ws, aff, y, B, L, None)
    p16 = lambda x=p, cin0=6, ws=p, aff=p, y=p, yp=p, B=1, L=1: lib.sonet_pointresnet_fused_p16_f32(x, cin0, ws, aff, y, yp, B, L, None)
    for name in ("x", "ws", "aff", "y"):
        refused(store(**{name: None}), INV, "NULL")
    for name in ("x", "ws", "aff", "yp"):                    # (y may be NULL there: only the planes are written)
        refused(p16(**{name: None}), INV, "NULL")
    for fn in (store, p16):
        refused(fn(B=0), INV, "bad size")
        refused(fn(L=0), INV, "bad size")
        refused(fn(cin0=0), INV, "Cin0=0")
        refused(fn(cin0=17), INV, "Cin0=17")
    # the first L whose 384-row panel reaches the limit: 4e9 bytes (2e9 where the P16 planes are addressed as well)
    refused(store(L=-(-4 * 10 ** 9 // 1536)), UNS, "4 GiB")
    refused(p16(L=-(-2 * 10 ** 9 // 1536)), UNS, "2 GiB")
    refused(p16(y=None, L=-(-2 * 10 ** 9 // 1536)), UNS, "2 GiB")

    def pool(fn, extra, **kw):
        a = dict(x=p, cin0=6, ws=p, aff=p, ids=p, pos0=p, off=p, cnt=p, wk=p, out=p, B=1, L=1, M=1)
        a.update(kw)
        return fn(a["x"], a["cin0"], a["ws"], a["aff"], a["ids"], a["pos0"], a["off"], a["cnt"], a["wk"], a["out"], *extra, a["B"], a["L"], a["M"], None)
    for fn, extra in ((lib.sonet_pointresnet_fused_pool_f32, ()), (lib.sonet_pointresnet_fused_pool_p16_f32, (p,))):
        for name in ("x", "ws", "aff", "ids", "pos0", "off", "cnt", "wk", "out"):
            refused(pool(fn, extra, **{name: None}), INV, "NULL")
        for name in ("B", "L", "M"):
            refused(pool(fn, extra, **{name: 0}), INV, "bad size")
        refused(pool(fn, extra, cin0=0), INV, "Cin0=0")
        refused(pool(fn, extra, cin0=17), INV, "Cin0=17")
        refused(pool(fn, extra, B=65536), UNS, "65535")
        refused(pool(fn, extra, L=-(-4 * 10 ** 9 // 64)), UNS, "4 GiB")             # 16 input rows of L floats: byte offsets in 32 bits
    refused(pool(lib.sonet_pointresnet_fused_pool_p16_f32, (None,)), INV, "NULL")
    refused(lib.sonet_pointresnet_pack(p, p, p, None, 6, p, None), INV, "NULL")
    refused(lib.sonet_pointresnet_pack(p, p, p, p, 17, p, None), INV, "Cin0=17")
    size = lib.sonet_pointresnet_pool_ws_size
    assert size(0, 5, 5) == size(5, 0, 5) == size(5, 5, 0) == size(-1, 5, 5) == size(5, -3, 5) == size(5, 5, -1) == 0
    # pooled keys B M 384 + partial keys of every 256-point tile (4 passes x 16 slots x 96) + copy 0's features B 384, 4 bytes each
    assert size(2, 257, 3) == (2 * 3 * 384 + 4 * 4 * 16 * 96 + 2 * 384) * 4


def test_ops_wrappers_refuse_wrong_members_before_any_launch():
    from sonet_hip import _lib, ops
    from sonet_hip._lib import SonetHipError
    lib = _lib.load()
    B, L, M = 2, 40, 4
    ws = torch.zeros(lib.sonet_pointresnet_pack_size(), dtype=torch.uint8)
    wsb = torch.zeros(lib.sonet_pointresnet_bf16_pack_size(), dtype=torch.uint8)
    aff = torch.zeros(832, 2)

    def sg(**kw):
        d = dict(x_aug_sorted=torch.zeros(B, 6, L), ids_sorted=torch.zeros(B, L, dtype=torch.int32), pos0=torch.zeros(B, dtype=torch.int32),
                 node_off=torch.zeros(B, M, dtype=torch.int32), count=torch.zeros(B, M, dtype=torch.int32))
        d.update(kw)
        return d
    bad = [("ids_sorted", torch.zeros(B, L, dtype=torch.int64), "int32"), ("ids_sorted", torch.zeros(B, L + 1, dtype=torch.int32), "shape"),
           ("ids_sorted", torch.zeros(B, 2 * L, dtype=torch.int32)[:, ::2], "contiguous"), ("ids_sorted", torch.zeros(B * L, dtype=torch.int32), "shape"),
           ("pos0", torch.zeros(B, dtype=torch.int64), "int32"), ("pos0", torch.zeros(B, 1, dtype=torch.int32), "shape"),
           ("node_off", torch.zeros(B, M, dtype=torch.int64), "int32"), ("node_off", torch.zeros(B, M + 1, dtype=torch.int32), "shape"),
           ("node_off", torch.zeros(M, B, dtype=torch.int32).t(), "contiguous"),
           ("count", torch.zeros(B, M, dtype=torch.float32), "int32"), ("count", torch.zeros(M, B, dtype=torch.int32), "shape"),
           ("count", torch.zeros(B, M, 2, dtype=torch.int32)[:, :, 0], "contiguous")]
    for pool, w in ((ops.pointresnet_fused_pool, ws), (ops.pointresnet_bf16_pool, wsb)):
        for name, t, word in bad:
            with pytest.raises(SonetHipError, match=name + ".*" + word):
                pool(sg(**{name: t}), w, aff, M)
        for wbad, word in ((w[:-1], "shape"), (w.view(torch.int8), "uint8"), (torch.zeros(2 * w.numel(), dtype=torch.uint8)[::2], "contiguous"),
                           (w.view(1, -1), "shape")):
            with pytest.raises(SonetHipError, match="wstream.*" + word):
                pool(sg(), wbad, aff, M)
        # a right grouping and stream pass these checks: what stops the call here is only that nothing is on a device
        with pytest.raises(SonetHipError, match="x_sorted must be a CUDA"):
            pool(sg(), w, aff, M)
    x = torch.zeros(B, 6, L)
    for fn, w in ((ops.pointresnet_fused, ws), (ops.pointresnet_bf16, wsb)):
        for wbad, word in ((w[:-1], "shape"), (w.view(torch.int8), "uint8"), (torch.zeros(2 * w.numel(), dtype=torch.uint8)[::2], "contiguous"),
                           (torch.zeros(w.numel() + 64, dtype=torch.uint8), "shape")):
            with pytest.raises(SonetHipError, match="wstream.*" + word):
                fn(x, wbad, aff)
        with pytest.raises(SonetHipError, match="x must be a CUDA"):
            fn(x, w, aff)
    # the two streams are not interchangeable
    assert ws.numel() != wsb.numel()
    with pytest.raises(SonetHipError, match="wstream.*shape"):
        ops.pointresnet_fused(x, wsb, aff)
