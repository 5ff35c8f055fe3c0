"""Segmenter layer 1 in its node-wise form in TRAINING (``opt.seg_nodewise_train``) on the MI355X:

* ``ops.pointwise_bwd_apply_nodesum``: g_raw the bits of ``ops.pointwise_bwd_apply``, gz the bits of ``ops.node_gather_bwd`` on it and of
  the numpy restatement (tests/seg_nodewise_ref.py), over the sizes at which the kernel takes another path (the 16-byte loads, a row
  group with fewer than its four rows, one / several column tiles, 1 .. 1024 nodes) and the id patterns that empty a list;
* ``ops.pointmlp_nodeadd_stats``: raw against float64 and, bit for bit, against ``ops.pointmlp_nodeadd``; the statistics against float64
  statistics of its own output; the range report;
* the training step with the option set: every gradient against the forced float64 twin (the helpers of tests/test_gpu_seg_training.py),
  option on against off, reproducibility, which launches ran, and the step after an optimizer step against a twin built from the
  ``state_dict()``."""
import ctypes
import re

import numpy as np
import pytest
import torch

import seg_nodewise_ref as R
import test_gpu_seg_training as T
from conftest import assert_close_rms, golden
from train_step_helpers import DEV, _relu_masks_of, cu

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31


def _tile():
    from sonet_hip import ops
    return ops.pointwise_bwd_apply_nodesum_tile()


def _operands(B, C, L, seed):
    g = torch.Generator().manual_seed(seed)
    gy, raw = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    vec = lambda lo, hi: torch.rand(C, generator=g) * (hi - lo) + lo
    # (scale, shift) put about half of the columns behind the ReLU; a, b, c0 of the size bn_bwd_coeffs gives
    return [cu(t) for t in (gy, raw, vec(0.5, 1.5), vec(-0.5, 0.5), vec(0.5, 2.0), vec(-0.1, 0.1), vec(-0.01, 0.01))]


def _ids(B, L, M, pattern, seed):
    """all_one: every column in one node; empty_first / empty_middle / empty_last: that node owns no column; ignored: -1, M and INT32_MIN
    among the ids; mixed: empty first, middle and last nodes AND ignored ids."""
    g = torch.Generator().manual_seed(seed)
    empty = {"empty_first": {0}, "empty_middle": {M // 2}, "empty_last": {M - 1}, "mixed": {0, M // 2, M - 1}}.get(pattern, set())
    allowed = [m for m in range(M) if m not in empty]
    if pattern == "all_one":
        allowed = [M - 1]
    if allowed:
        ids = torch.tensor(allowed, dtype=torch.int64)[torch.randint(0, len(allowed), (B, L), generator=g)]
    else:
        ids = torch.full((B, L), -1, dtype=torch.int64)
    if pattern in ("ignored", "mixed"):
        bad = torch.tensor([-1, M, INT32_MIN], dtype=torch.int64)[torch.randint(0, 3, (B, L), generator=g)]
        ids = torch.where(torch.rand(B, L, generator=g) < 0.2, bad, ids)
        if L >= 3:
            ids[0, 0], ids[0, L // 2], ids[0, L - 1] = -1, M, INT32_MIN
    return ids.to(torch.int32)


def _check_nodesum(B, C, L, M, relu, pattern, seed, numpy_too=True):
    from sonet_hip import ops
    gy, raw, sc, sh, a, b, c0 = _operands(B, C, L, seed)
    ids = _ids(B, L, M, pattern, seed + 1)
    idd = cu(ids)
    g_raw, gz = ops.pointwise_bwd_apply_nodesum(gy, raw, sc, sh, relu, a, b, c0, idd, M)
    want = ops.pointwise_bwd_apply(gy, raw, sc, sh, relu, a, b, c0)
    what = (B, C, L, M, relu, pattern)
    assert g_raw.shape == (B, C, L) and gz.shape == (B, C, M) and gz.dtype == torch.float32
    assert torch.equal(g_raw, want), what
    assert torch.equal(gz, ops.node_gather_bwd(want, idd, M)), what
    if numpy_too:
        assert R.same_bits(gz.cpu().numpy(), R.node_sum_f32(want.cpu().numpy(), ids.numpy(), M)), what
    return g_raw, gz


def _lengths():
    t = _tile()
    return [1, 63, 64, 65, 255, 257, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("li", range(10))
def test_apply_nodesum_is_the_two_launches_bit_for_bit(li):
    """B 1 / 3, C 1 / 5 / 32 / 33, M 1 / 3 / 64 / 65 / 1024, ReLU on and off at every length (parametrised by its place in the list:
    the tile extent is the library's); ids with empty first, middle and last nodes and ignored ids."""
    L = _lengths()[li]
    n = 0
    for B in (1, 3):
        for C in (1, 5, 32, 33):
            for M in (1, 3, 64, 65, 1024):
                for relu in (False, True):
                    n += 1
                    # (the numpy restatement where it is quick: the device's own node_gather_bwd is compared everywhere)
                    _check_nodesum(B, C, L, M, relu, "mixed", 1000 * li + n, numpy_too=(C <= 5 or B == 1))


@pytest.mark.parametrize("pattern", ["all_one", "empty_first", "empty_middle", "empty_last", "ignored"])
def test_apply_nodesum_id_patterns(pattern):
    t = _tile()
    n = 0
    for M in (1, 3, 64, 65, 1024):
        for L in (1, 65, 257, t + 1, 2 * t + 1):
            for B, C in ((1, 5), (3, 33)):
                n += 1
                g_raw, gz = _check_nodesum(B, C, L, M, True, pattern, 7000 + n, numpy_too=(B == 1))
                if pattern == "all_one":
                    assert not gz[:, :, :M - 1].any() and (M > 1 or L < 2 or gz.any())
                if pattern == "empty_last" and M > 1:
                    assert not gz[:, :, M - 1].any()


def test_apply_nodesum_confines_a_nan():
    from sonet_hip import ops
    t = _tile()
    B, C, L, M = 2, 6, t + 9, 5
    gy, raw, sc, sh, a, b, c0 = _operands(B, C, L, 31)
    ids = _ids(B, L, M, "empty_middle", 32)
    sc.fill_(1.0)
    sh.fill_(100.0)                                              # every column passes the ReLU
    gy[1, 4, t + 3] = float("nan")                               # (second tile, second row group)
    g_raw, gz = ops.pointwise_bwd_apply_nodesum(gy, raw, sc, sh, True, a, b, c0, cu(ids), M)
    bad = torch.isnan(g_raw).nonzero().tolist()
    assert bad == [[1, 4, t + 3]], bad
    assert torch.isnan(gz).nonzero().tolist() == [[1, 4, int(ids[1, t + 3])]]
    assert torch.equal(g_raw.nan_to_num(7.0), ops.pointwise_bwd_apply(gy, raw, sc, sh, True, a, b, c0).nan_to_num(7.0))


def _c_call(gy, raw, sc, sh, relu, a, b, c0, ids, M, g_raw, gz, ws):
    from sonet_hip import _lib
    B, C, L = gy.shape
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    st = _lib.load().sonet_pointwise_bwd_apply_nodesum_f32(p(gy), p(raw), p(sc), p(sh), int(relu), p(a), p(b), p(c0), p(ids), M, p(g_raw), p(gz),
                                                           p(ws), B, C, L, _lib.stream_ptr())
    assert st == 0, _lib.last_error()


@pytest.mark.parametrize("L", [64, 260, 1028])
def test_apply_nodesum_offsets_and_prefilled_buffers_give_the_same_bits(L):
    """L % 4 == 0 takes 16-byte loads when gy, raw and g_raw are 16-byte aligned and single elements otherwise: operands (and the output)
    at a 4-byte offset give the same bits; so do outputs and a workspace that held 0xFF bytes before the launch."""
    from sonet_hip import _lib, ops
    B, C, M = 3, 7, 65
    gy, raw, sc, sh, a, b, c0 = _operands(B, C, L, 40 + L)
    ids = cu(_ids(B, L, M, "mixed", 41))
    want_g, want_z = ops.pointwise_bwd_apply_nodesum(gy, raw, sc, sh, True, a, b, c0, ids, M)
    n = B * C * L
    nws = _lib.load().sonet_pointwise_bwd_apply_nodesum_ws_size(B, M, L)

    def shifted(t_, by):
        buf = torch.zeros(t_.numel() + by, dtype=t_.dtype, device=DEV)
        v = buf[by:by + t_.numel()].view(t_.shape)
        v.copy_(t_)
        assert v.data_ptr() % 16 == (4 * by) % 16 and v.is_contiguous()
        return v
    for og, orw, oo in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0)):
        obuf = torch.full((n + oo,), float("nan"), device=DEV)
        obuf.view(torch.int32).fill_(-1)                         # 0xFF bytes
        g_raw = obuf[oo:oo + n].view(B, C, L)
        gz = torch.empty(B, C, M, device=DEV)
        gz.view(torch.int32).fill_(-1)
        ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
        _c_call(shifted(gy, og), shifted(raw, orw), sc, sh, True, a, b, c0, ids, M, g_raw, gz, ws)
        assert torch.equal(g_raw, want_g) and torch.equal(gz, want_z), (L, og, orw, oo)
    # ids at a 4-byte offset too (read as single words everywhere)
    g2, z2 = ops.pointwise_bwd_apply_nodesum(gy, raw, sc, sh, True, a, b, c0, shifted(ids, 1), M)
    assert torch.equal(g2, want_g) and torch.equal(z2, want_z)


def test_apply_nodesum_two_runs_and_a_graph_replay_are_bit_identical():
    from sonet_hip import ops
    t = _tile()
    B, C, L, M = 3, 33, 2 * t + 4, 64
    gy, raw, sc, sh, a, b, c0 = _operands(B, C, L, 50)
    ids = cu(_ids(B, L, M, "mixed", 51))
    run = lambda: ops.pointwise_bwd_apply_nodesum(gy, raw, sc, sh, True, a, b, c0, ids, M)
    (g1, z1), (g2, z2) = run(), run()
    assert torch.equal(g1, g2) and torch.equal(z1, z2)
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        run()                                                    # (warm-up on the capture stream)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            g3, z3 = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g3, g1) and torch.equal(z3, z1)
    gy.mul_(-2.0).add_(1e-4)                                     # the graph reads the operands in place
    graph.replay()
    torch.cuda.synchronize()
    g4, z4 = run()
    assert not torch.equal(g3, g1) and torch.equal(g3, g4) and torch.equal(z3, z4)


# ------------------------------------------------------------------------------------------------------------------ the forward launch
def _fwd_case(B, C1, C2, Cout, L, ZM, seed):
    from sonet_hip import ops
    g = torch.Generator().manual_seed(seed)
    Cin = C1 + C2
    W = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    x1, x2 = torch.randn(B, C1, L, generator=g), (torch.randn(B, C2, L, generator=g) if C2 else None)
    z, bias = torch.randn(B, Cout, ZM, generator=g), torch.randn(Cout, generator=g)
    zidx = torch.randint(0, ZM, (B, L), generator=g, dtype=torch.int32)
    if L >= 31:                                                  # out of range: + 0
        zidx[0, 3], zidx[B - 1, L - 1], zidx[0, 17] = -1, ZM, INT32_MIN
    wp = ops.pointmlp_pack(cu(W), "h3")
    return W, x1, x2, z, bias, zidx, wp


def _fwd_f64(W, x1, x2, z, bias, zidx):
    B, ZM = z.shape[0], z.shape[2]
    x = torch.cat([x1] + ([x2] if x2 is not None else []), dim=1).double()
    ok = (zidx >= 0) & (zidx < ZM)
    zg = torch.gather(z.double(), 2, zidx.clamp(0, ZM - 1).long().unsqueeze(1).expand(B, z.shape[1], -1)) * ok.unsqueeze(1)
    return torch.einsum("oc,bcl->bol", W.double(), x) + zg + bias.double().view(1, -1, 1)


@pytest.mark.parametrize("C1,C2", [(16, 0), (16, 9), (384, 0), (384, 9)])
def test_nodeadd_stats_forward(C1, C2):
    """Cout 32 / 128 / 192, L 1 / 31 / 33 / 257, B 1 / 3, ZM 1 / 3 / 64.  raw to 1e-5 of float64 (|err| <= 1e-5 max(|ref|, rms)), the
    bits of ``pointmlp_nodeadd`` at unit scale, shift = bias, no ReLU.  The statistics against float64 statistics of the stored raw:
    the kernel sums a row's 32 columns in f32 (a five-level tree: <= 5 roundings of 2^-24 on a partial of size <= 32 rms) and carries
    the partials in f64, so the mean is held to 1e-6 of the channel's root mean square and the variance (mean square minus squared
    mean) to 1e-6 of its mean square."""
    from sonet_hip import ops
    n = 0
    for Cout in (32, 128, 192):
        for L in (1, 31, 33, 257):
            for B in (1, 3):
                for ZM in (1, 3, 64):
                    n += 1
                    W, x1, x2, z, bias, zidx, wp = _fwd_case(B, C1, C2, Cout, L, ZM, 100 * C1 + 10 * C2 + n)
                    d = [cu(t_) if t_ is not None else None for t_ in (x1, x2, z, bias, zidx)]
                    raw, mean, var = ops.pointmlp_nodeadd_stats(d[0], wp, d[3], Cout, d[2], d[4], x2=d[1])
                    what = (C1, C2, Cout, L, B, ZM)
                    assert_close_rms(raw.cpu().numpy(), _fwd_f64(W, x1, x2, z, bias, zidx).numpy(), 1e-5, "raw %s" % (what,))
                    ones = ops.const_vec(Cout, 1.0, raw.device)
                    assert torch.equal(raw, ops.pointmlp_nodeadd(d[0], wp, ones, d[3], False, Cout, d[2], d[4], x2=d[1])), what
                    r64 = raw.double()
                    m64, ms64 = r64.mean(dim=(0, 2)), (r64 ** 2).mean(dim=(0, 2))
                    v64 = ms64 - m64 ** 2
                    assert float(((mean.double() - m64).abs() / ms64.sqrt()).max()) <= 1e-6, what
                    assert float(((var.double() - v64).abs() / ms64).max()) <= 1e-6, what


def test_nodeadd_stats_reports_an_operand_out_of_range():
    from sonet_hip import ops
    W, x1, x2, z, bias, zidx, wp = _fwd_case(2, 384, 9, 128, 257, 64, 77)
    d = [cu(t_) for t_ in (x1, x2, z, bias, zidx)]
    with ops.range_scope(DEV) as rs:
        ops.pointmlp_nodeadd_stats(d[0], wp, d[3], 128, d[2], d[4], x2=d[1])
    assert rs.violations() == [] and rs.names == ["pointmlph3_nodeadd_stats_393x128_L257"]
    d[0][1, 5, 100] = 1e5
    with ops.range_scope(DEV) as rs:
        ops.pointmlp_nodeadd_stats(d[0], wp, d[3], 128, d[2], d[4], x2=d[1])
    bad = rs.violations()
    assert len(bad) == 1 and bad[0][0] == "pointmlph3_nodeadd_stats_393x128_L257" and "exceeds 2047" in bad[0][1], bad


def test_nodeadd_stats_consumes_the_rider():
    """``bn_rider`` armed for the launch: its finalize writes (invstd, scale, shift) and updates the running statistics as the layers'
    statistics launches do -- against the separate launches."""
    from sonet_hip import ops
    W, x1, x2, z, bias, zidx, wp = _fwd_case(3, 384, 9, 128, 257, 3, 78)
    d = [cu(t_) for t_ in (x1, x2, z, bias, zidx)]
    g = torch.Generator().manual_seed(5)
    gamma, beta = cu(torch.rand(128, generator=g) + 0.5), cu(torch.randn(128, generator=g))
    rm, rv = cu(torch.randn(128, generator=g)), cu(torch.rand(128, generator=g) + 0.5)
    rm0, rv0 = rm.clone(), rv.clone()
    n = 3 * 257
    invstd, sc, sh = ops.bn_rider(gamma, beta, 1e-5, rm, rv, 0.1, n / (n - 1))
    raw, mean, var = ops.pointmlp_nodeadd_stats(d[0], wp, d[3], 128, d[2], d[4], x2=d[1])
    i2, s2, h2 = ops.bn_fwd_coeffs(mean, var, gamma, beta, 1e-5)
    assert torch.equal(invstd, i2) and torch.equal(sc, s2) and torch.equal(sh, h2)
    ops.bn_running_update_(rm0, rv0, mean, var, 0.1, n / (n - 1))
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


# ------------------------------------------------------------------------------------------------------------------ the step
NEW = ("pointwise_bwd_apply_nodesum", r"pointmlph3_nodeadd_stats_393x1024_L\d+")
_steps = {}
_models = T._models                    # (the original: a test that takes several steps patches T._models once per step)


def _masks_with_layer1(loss, enc, cls=None, seg=None):
    """train_step_helpers._relu_masks_of plus the ReLU pattern of the node-wise layer 1, whose autograd node saves its first ten
    tensors in the order of the dense layer's: (x1, x2, weight2d, sc, sh, raw, ...)."""
    masks = _relu_masks_of(loss, enc, cls=cls, seg=seg)
    seen, stack = set(), [loss.grad_fn]
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        stack.extend(fn for fn, _ in node.next_functions)
        if type(node).__name__ == "_NodewiseLayerFnBackward":
            sv = node.saved_tensors
            assert seg is not None and sv[2].data_ptr() == seg.layer1.conv.weight.data_ptr()
            masks["seg.layer1"] = (sv[5].double() * sv[3].double().view(1, -1, 1) + sv[4].double().view(1, -1, 1)) > 0
    return masks


def _step(monkeypatch, option, mode="h3", variant=None, key=None):
    """test_gpu_seg_training.run_seg_step on the fixture with ``opt.seg_nodewise_train`` = option (None: absent); variant "eval": the
    segmenter in eval mode (autograd on), "instance": layer 1 with instance normalisation.  Results are shared under ``key``."""
    if key is not None and key in _steps:
        return _steps[key]
    def patched(g):
        enc, seg = _models(g)
        for m in (enc, seg):
            if option is not None:
                m.opt.seg_nodewise_train = option
            else:
                assert not hasattr(m.opt, "seg_nodewise_train")
        if variant == "eval":
            seg.eval()
        if variant == "instance":
            from models.layers import EquivariantLayer
            torch.manual_seed(3)
            seg.layer1 = EquivariantLayer(3356, 1024, activation="relu", normalization="instance").to(DEV).train()
        return enc, seg
    monkeypatch.setattr(T, "_models", patched)
    monkeypatch.setattr(T, "_relu_masks_of", _masks_with_layer1)
    res = T.run_seg_step(golden(T.FIXTURE), mode)
    if key is not None:
        _steps[key] = res
    return res


def _same_step(a, b, what):
    """test_gpu_seg_training._same_step, naming every tensor that differs."""
    assert torch.equal(a["score"], b["score"]), what
    assert torch.equal(a["loss"], b["loss"]), (what, float(a["loss"]), float(b["loss"]))
    bad = [k for k in a["running"] if not torch.equal(a["running"][k][1], b["running"][k][1])]
    assert not bad, (what, bad)
    assert sorted(a["mine"]) == sorted(b["mine"]), what
    bad = [(k, float((a["mine"][k] - b["mine"][k]).abs().max())) for k in a["mine"] if not torch.equal(a["mine"][k], b["mine"][k])]
    assert not bad, (what, len(bad), bad)


def _ran(names, pattern):
    rx = re.compile(pattern)
    return any(rx.fullmatch(n) for n in names)


def test_step_gradients_against_the_forced_float64_twin(monkeypatch):
    """The option on, ``seg_train_step_b8_n512``: loss to 1e-5, scores to 1e-4, every gradient to the existing 1e-4 rel-rms of the float64
    twin with the run's routing and ReLU masks (layer 1's read from the node-wise autograd node) forced, running statistics to 1e-5."""
    g = golden(T.FIXTURE)
    res = _step(monkeypatch, True, key="on_a")
    cap = res["cap"]
    assert sorted(cap["masks"]) == sorted(T.ENC_LAYERS + T.SEG_LAYERS), sorted(cap["masks"])
    assert _ran(res["names"], NEW[0]) and _ran(res["names"], NEW[1]), sorted(res["names"])
    r = T.f64_seg_step(res, g, forced=True)
    assert abs(float(res["loss"]) - float(r["loss"])) <= 1e-5 * abs(float(r["loss"])), (float(res["loss"]), float(r["loss"]))
    assert_close_rms(res["score"].cpu().numpy(), r["score"].cpu().numpy(), 1e-4, "score, same routing")
    rel = T.grad_residuals(res, r)
    worst = max(rel.items(), key=lambda kv: kv[1])
    print("seg node-wise forced routing: worst gradient %s %.3e (T %.0e); seg.layer1.conv.weight %.3e" % (
        worst[0], worst[1], T.SEG_FORCED_TOL, rel["seg.layer1.conv.weight"]))
    assert len(rel) == 34 and {"seg.layer%d.conv.weight" % i for i in range(1, 6)} <= set(rel), sorted(rel)
    assert worst[1] <= T.SEG_FORCED_TOL, sorted(rel.items(), key=lambda kv: -kv[1])[:6]
    assert res["dead"] == int(g["dead_grad_count"])
    run = T.expected_running(res, r)
    assert len(run) == 2 * 10, sorted(run)
    for k, (want, got) in run.items():
        assert_close_rms(got.cpu().numpy(), want.cpu().numpy(), 1e-5, "running stat " + k)


def test_step_option_on_against_off_and_reproducible(monkeypatch):
    on_a, on_b = _step(monkeypatch, True, key="on_a"), _step(monkeypatch, True, key="on_b")
    off = _step(monkeypatch, None, key="off_a")
    assert abs(float(on_a["loss"]) - float(off["loss"])) <= 1e-6 * abs(float(off["loss"])), (float(on_a["loss"]), float(off["loss"]))
    _same_step(on_a, on_b, "second run with the option on")
    assert sorted(on_a["mine"]) == sorted(off["mine"]) and on_a["dead"] == off["dead"]


def test_step_launch_names(monkeypatch):
    on, off_a, off_b = _step(monkeypatch, True, key="on_a"), _step(monkeypatch, None, key="off_a"), _step(monkeypatch, None, key="off_b")
    names = on["names"]
    assert _ran(names, NEW[0]) and _ran(names, NEW[1]), sorted(names)
    assert not any(n.startswith("node_gather") for n in names), sorted(names)
    wide = [n for n in names if re.search(r"(?<!\d)(3356|3456)(?!\d)", n)]
    assert not wide, wide
    # the split's own launches: the per-node block, the two input gradients, the two wide weight gradients
    assert _ran(names, r"pointmlph3_1923x1024_L64") and _ran(names, r"pointmlpx3_1024x384_L1536") and _ran(names, r"pointmlpx3_1024x1920_L64")
    assert _ran(names, r"wgradx3_1024x393_L1536"), sorted(names)
    # option absent: the dense branch as before, bit for bit
    for res in (off_a, off_b):
        assert not _ran(res["names"], NEW[0]) and not _ran(res["names"], NEW[1])
        assert {"node_gather", "node_gather_bwd"} <= res["names"] and _ran(res["names"], r"wgradx3_1024x3356_L1536")
    _same_step(off_a, off_b, "second run with the option absent")
    # option False is option absent
    _same_step(off_a, _step(monkeypatch, False), "option False")


@pytest.mark.parametrize("mode,variant", [("x3", None), ("h3", "eval"), ("h3", "instance")])
def test_step_keeps_the_dense_branch_elsewhere(monkeypatch, mode, variant):
    """The option set, but another arithmetic, the segmenter in eval mode with autograd on, or instance normalisation: no new launch."""
    res = _step(monkeypatch, True, mode=mode, variant=variant)
    assert not _ran(res["names"], NEW[0]) and not any("nodeadd_stats" in n for n in res["names"]), sorted(res["names"])
    assert any(re.search(r"(?<!\d)3356(?!\d)", n) for n in res["names"]) or any(3356 in a or 3356 in b for a, b in res["bmm"])
    assert torch.isfinite(res["loss"])


def _plain_step(enc, seg, g):
    from models import networks as NW
    from models.losses import CrossEntropyLossSeg
    pc, sn, node, knn_I, label = cu(g["pc"]), cu(g["sn"]), cu(g["node"]), cu(g["node_knn_I"]), cu(g["label"])
    score = NW.segmentation_forward(enc, seg, pc, sn, label, node, knn_I, is_train=True, epoch=0)
    enc.zero_grad()
    seg.zero_grad()
    loss = CrossEntropyLossSeg()(score, cu(g["seg"]))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    grads.update({"seg." + k: p.grad.clone() for k, p in seg.named_parameters() if p.grad is not None})
    return loss.detach().clone(), grads


def test_step_after_an_optimizer_step_equals_a_twin_from_the_state_dict():
    """The packs of the split (forward and transposed) follow the weight: after one Adam step the next step's loss and gradients are those
    of fresh models loaded from the ``state_dict()``, bit for bit."""
    from sonet_hip import ops
    g = golden(T.FIXTURE)
    enc, seg = _models(g)
    enc.opt.seg_nodewise_train = True
    assert seg.opt.seg_nodewise_train is True
    with ops.kernel_timing() as rec:
        loss1, _ = _plain_step(enc, seg, g)
    assert any(n == NEW[0] for n, _, _ in rec.records)
    opts = [torch.optim.Adam(m.parameters(), lr=0.001, betas=(0.9, 0.999), weight_decay=0) for m in (enc, seg)]
    for o in opts:
        o.step()
    sd_e, sd_s = ({k: v.detach().clone() for k, v in m.state_dict().items()} for m in (enc, seg))
    loss2, grads2 = _plain_step(enc, seg, g)
    enc2, seg2 = _models(g)
    enc2.opt.seg_nodewise_train = True
    enc2.load_state_dict(sd_e)
    seg2.load_state_dict(sd_s)
    loss3, grads3 = _plain_step(enc2, seg2, g)
    assert not torch.equal(loss1, loss2)
    assert torch.equal(loss2, loss3), (float(loss2), float(loss3))
    assert sorted(grads2) == sorted(grads3)
    bad = [(k, float((grads2[k] - grads3[k]).abs().max())) for k in grads2 if not torch.equal(grads2[k], grads3[k])]
    assert not bad, (len(bad), bad)
