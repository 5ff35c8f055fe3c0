"""GPU tests of the up-convolution's training path (sonet_upconv3x3_dgrad_f32, ops.upconv3x3_dgrad, layers._UpConvTrainFn,
opt.decoder_fused_train).

  * the input-gradient operator against float64 at the project's metric, |dx - ref| <= 1e-5 max(|ref|, rms(ref)) -- the gate the bf16-split
    kernels already meet -- on every map size that takes another path through the tile (one pixel, a single row, a single column, seams
    inside a tile, the largest map), K and row tails, the longest accumulation chain, g at gradient scale and 2^-30 below it;
  * an exact case (small integers; tests/test_upconv_train_cpu.py derives why) that must match float64 bit for bit;
  * reproducibility, HIP-graph capture, NaN isolation;
  * the layer and the decoder against the float64 twins of tests/upconv_train_ref.py with THIS run's ReLU masks forced, routing by launch
    names, the range guard, refusals.
"""
import contextlib
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

import upconv_ref as R
import upconv_train_ref as T
from conftest import assert_close_rms, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_dgrad(g, w):
    from sonet_hip import ops
    return ops.upconv3x3_dgrad(cu(g), ops.upconv3x3_dgrad_pack(cu(w)), w.shape[1])


# ------------------------------------------------------------------------------------------------------------ operator against float64
# (B, Cin, Cout, H, W)
OPERATOR = [
    (2, 16, 32, 1, 1), (2, 16, 32, 1, 2), (2, 16, 32, 2, 2), (1, 16, 32, 3, 5), (2, 16, 32, 8, 8), (1, 16, 32, 5, 30), (2, 16, 32, 1, 64),
    (2, 16, 32, 64, 1),                    # every map shape: one pixel, rows, columns, a seam inside a row (150 columns)
    (1, 16, 32, 64, 64),                   # the largest map: 32 column tiles, a halo of 65 columns on either side
    (127, 16, 32, 1, 1), (128, 16, 32, 1, 1), (129, 16, 32, 1, 1),         # one below, at and one above the tile extent
    (3, 16, 32, 3, 5),                     # 45 columns of three clouds in one tile: cloud seams inside it
    (2, 1, 32, 3, 5), (2, 15, 32, 3, 5), (2, 17, 32, 3, 5), (2, 33, 32, 3, 5), (2, 128, 32, 3, 5),     # row tails and several row blocks
    (2, 32, 32, 2, 2), (2, 32, 96, 2, 2), (2, 32, 1024, 2, 2),             # 2, 6 and 64 chunks: up to sixteen chains of 1024 products
]


@pytest.mark.parametrize("case", OPERATOR, ids=lambda c: "B%d_%dx%d_%dx%d" % c)
def test_operator_matches_float64(case):
    B, Cin, Cout, H, W = case
    w = T.make_w(Cin, Cout, seed=sum(case))
    g = T.make_g(B, Cout, H, W, seed=sum(case) + 1)
    ref = T.dgrad_folded(g, w)
    for e in (0, -30):                                           # (a power of two scales the float64 gradient exactly)
        dx = run_dgrad(np.ldexp(g, e).astype(np.float32), w)
        assert tuple(dx.shape) == (B, Cin, H, W) and dx.dtype == torch.float32
        print("upconv dgrad %s x 2^%d: err / bound %.3f" % (case, e, R.rms_error(dx.cpu().numpy(), np.ldexp(ref, e)) / 1e-5))
        assert_close_rms(dx.cpu().numpy(), np.ldexp(ref, e), 1e-5, "upconv3x3_dgrad %s x 2^%d" % (case, e))


def test_operator_cases_cover_the_tile_edges():
    from sonet_hip import ops
    TP = ops.UPCONV_TILE_PIXELS
    assert {TP - 1, TP, TP + 1} <= {c[0] * c[3] * c[4] for c in OPERATOR}
    assert {1, 15, 16, 17, 33, 128} <= {c[1] for c in OPERATOR} and {32, 96, 1024} <= {c[2] for c in OPERATOR}
    assert {(1, 1), (1, 2), (2, 2), (3, 5), (8, 8), (5, 30), (1, 64), (64, 1), (64, 64)} <= {(c[3], c[4]) for c in OPERATOR}


@pytest.mark.parametrize("shape", T.INT_SHAPES, ids=lambda s: "B%d_%dx%d_%dx%d" % s)
def test_integer_case_is_bit_identical(shape):
    """Integer g in [-2, 2] and w in [-3, 3]: every piece, product and partial sum is exact (test_the_integer_case_is_exact_by_derivation) --
    the output equals the float64 gradient.  A wrong tap, parity, shift or border shows here as a plain mismatch."""
    g, w = T.int_case(shape)
    dx = run_dgrad(g, w).cpu().numpy().astype(np.float64)
    ref = T.dgrad_folded(g, w)
    bad = np.argwhere(dx != ref)
    assert bad.size == 0, "%d mismatches, first at %s: got %r want %r" % (len(bad), bad[0], dx[tuple(bad[0])], ref[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------------------ reproducibility, isolation
def test_two_runs_and_a_graph_replay_are_bit_identical():
    from sonet_hip import ops
    B, Cin, Cout, H, W = 3, 40, 96, 8, 8
    w, g = T.make_w(Cin, Cout, 9), T.make_g(B, Cout, H, W, 10)
    wpt, gd = ops.upconv3x3_dgrad_pack(cu(w)), cu(g)
    a, b = ops.upconv3x3_dgrad(gd, wpt, Cin), ops.upconv3x3_dgrad(gd, wpt, Cin)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.upconv3x3_dgrad(gd, wpt, Cin)                        # (warm-up on the capture stream)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            out = ops.upconv3x3_dgrad(gd, wpt, Cin)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    gd.mul_(-2.0).add_(1e-4)                                     # the graph reads the operand in place
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, a) and torch.equal(out, ops.upconv3x3_dgrad(gd, wpt, Cin))


def test_a_nan_stays_inside_its_window_and_its_cloud():
    B, Cin, Cout, H, W = 3, 20, 32, 5, 6
    w, g = T.make_w(Cin, Cout, 3), T.make_g(B, Cout, H, W, 4)
    clean = run_dgrad(g, w).cpu().numpy()
    for (Y, X) in ((0, 0), (5, 6), (9, 11), (4, 7)):
        gb = g.copy()
        gb[1, 7, Y, X] = np.nan
        got = run_dgrad(gb, w).cpu().numpy()
        window = {((Y + ky - 1) // 2, (X + kx - 1) // 2) for ky in range(3) for kx in range(3)
                  if 0 <= Y + ky - 1 < 2 * H and 0 <= X + kx - 1 < 2 * W}
        hit = np.zeros((H, W), bool)
        for (u, v) in window:
            hit[u, v] = True
        assert np.array_equal(np.isnan(got[1]), np.broadcast_to(hit, (Cin, H, W))), (Y, X)
        assert np.array_equal(got[1][:, ~hit], clean[1][:, ~hit])
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])


# ------------------------------------------------------------------------------------------------------------ the layer
@contextlib.contextmanager
def _reproducible_aten():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = old


def _layer_case(name):
    """-> (Cin, Cout, act, norm, operands as float32 arrays)."""
    if name == "seeded_33x64_4x4":
        o = T.make_layer_case(3, 33, 64, 4, 4, seed=77)
        return 33, 64, "relu", "batch", o
    Cin, Cout, act, norm, B, H, W = T.FIXTURES[name]
    f = golden("upconv_train/" + name)
    o = dict(x=f["x"], w=f["conv__conv__weight"], b=f["conv__conv__bias"], g=f["g"], gamma=None, beta=None, running=None)
    if norm == "batch":
        o.update(gamma=f["conv__norm__weight"], beta=f["conv__norm__bias"], running=(f["conv__norm__running_mean"], f["conv__norm__running_var"]))
    return Cin, Cout, act, norm, o


def _run_layer(Cin, Cout, act, norm, o):
    from models import layers as L
    from sonet_hip import ops
    m = L.UpConv(Cin, Cout, activation=act, normalization=norm)
    with torch.no_grad():
        m.conv.conv.weight.copy_(torch.from_numpy(o["w"]))
        m.conv.conv.bias.copy_(torch.from_numpy(o["b"]))
        if norm == "batch":
            m.conv.norm.weight.copy_(torch.from_numpy(o["gamma"]))
            m.conv.norm.bias.copy_(torch.from_numpy(o["beta"]))
            m.conv.norm.running_mean.copy_(torch.from_numpy(o["running"][0]))
            m.conv.norm.running_var.copy_(torch.from_numpy(o["running"][1]))
    m.to(DEV).train()
    m.fused_train = True
    x = cu(o["x"]).requires_grad_(True)
    with ops.kernel_timing() as rec:
        y = m(x)
        y.backward(cu(o["g"]))
    names = [n for n, _a, _b in rec.records if n.startswith("upconv3x3")]
    out = dict(y=y.detach(), dx=x.grad, dW=m.conv.conv.weight.grad, db=m.conv.conv.bias.grad, names=names)
    if norm == "batch":
        out.update(dgamma=m.conv.norm.weight.grad, dbeta=m.conv.norm.bias.grad, running_mean=m.conv.norm.running_mean.detach().clone(),
                   running_var=m.conv.norm.running_var.detach().clone())
    return out


@pytest.mark.parametrize("name", ["upconv_16x32_3x5", "upconv_40x32_1x1", "seeded_33x64_4x4"])
def test_layer_step_matches_the_float64_twin(name):
    Cin, Cout, act, norm, o = _layer_case(name)
    relu, B, H, W = act == "relu", o["x"].shape[0], o["x"].shape[2], o["x"].shape[3]
    with _reproducible_aten():
        r, r2 = _run_layer(Cin, Cout, act, norm, o), _run_layer(Cin, Cout, act, norm, o)
    assert r["names"] == ["upconv3x3_%dx%d_%dx%d" % (Cin, Cout, H, W), "upconv3x3_dgrad_%dx%d_%dx%d" % (Cin, Cout, H, W)]
    for k in r:
        if k != "names":
            assert torch.equal(r[k], r2[k]), "%s is not reproducible" % k          # (dW: under the deterministic switch)
    free = T.layer_train64(o["x"], o["w"], o["b"], o["gamma"], o["beta"], 1e-5, relu, g=o["g"], running=o["running"])
    y = r["y"].cpu().numpy()
    assert_close_rms(y, free["y"], 1e-5, name + " y")
    if norm == "batch":
        assert_close_rms(r["running_mean"].cpu().numpy(), free["running_mean"], 1e-5, name + " running_mean")
        assert_close_rms(r["running_var"].cpu().numpy(), free["running_var"], 1e-5, name + " running_var")
    mask = None
    if relu:
        # the run's mask may differ from the twin's own only where the pre-activation is within rounding of zero
        mask = (y > 0).astype(np.float64)
        flipped = mask != free["mask"]
        rms = float(np.sqrt(np.mean(free["pre"] ** 2)))
        print("%s: %d of %d mask elements differ" % (name, int(flipped.sum()), mask.size))
        assert np.all(np.abs(free["pre"][flipped]) <= 1e-5 * rms)
    t = T.layer_train64(o["x"], o["w"], o["b"], o["gamma"], o["beta"], 1e-5, relu, mask=mask, g=o["g"], running=o["running"])
    keys = ["dx", "dW"] + (["dgamma", "dbeta"] if norm == "batch" else [])
    for k in keys:
        e = T.rel_rms(r[k].cpu().numpy(), t[k])
        print("%s %s: rel-rms %.3g" % (name, k, e))
        assert e <= 1e-4, (name, k, e)
    db = np.abs(r["db"].cpu().numpy() - t["db"])
    unit = np.abs(t["g_raw"]).sum(axis=(0, 2, 3))
    print("%s db: worst |err| / sum |g_raw| %.3g" % (name, float((db / unit).max())))
    assert np.all(db <= 1e-4 * unit)


# ------------------------------------------------------------------------------------------------------------ the decoder
def _decoder(train_opt, F=256, seed=31, fused=None):
    from models import networks as NW
    from sonet_hip import synth
    opt = Namespace(gpu_id=0, device=torch.device(DEV), feature_num=F, activation="relu", normalization="batch",
                    output_fc_pc_num=0, output_conv_pc_num=4096)
    if train_opt is not None:
        opt.decoder_fused_train = train_opt
    if fused is not None:
        opt.decoder_fused = fused
    dec = NW.Decoder(opt)
    synth.fill_state_dict_(dec.state_dict(), seed)
    return dec.to(DEV).train()


def _feature(B, F, seed=3):
    return torch.randn(B, F, generator=torch.Generator().manual_seed(seed)).abs().to(DEV)


def _cots(B, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return {i: (torch.randn(B, 3, n, generator=gen) * 1e-3) for i, n in ((4, 256), (5, 1024), (6, 4096))}


def _decoder_step(dec, f, cots):
    """One forward + backward with fixed cotangents on pc4, pc5, pc6 -> (launch names, {layer: output > 0})."""
    from sonet_hip import ops
    outs, hooks = {}, []
    dc = dec.conv_decoder
    for name in T.MASKED:
        mod = dc
        for part in name.split("."):
            mod = getattr(mod, part)
        hooks.append(mod.register_forward_hook(lambda _m, _i, out, name=name: outs.__setitem__(name, out.detach())))
    with ops.kernel_timing() as rec:
        dec(f)
        loss = sum((getattr(dec, "conv_pc%d" % i) * cots[i].to(DEV)).sum() for i in (4, 5, 6))
        loss.backward()
    for h in hooks:
        h.remove()
    return [n for n, _a, _b in rec.records if n.startswith("upconv3x3")], {k: (v > 0).double().cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("opt", [True, (4, 5, 6)], ids=["all", "layers456"])
def test_decoder_gradients_match_the_float64_chain_with_forced_masks(opt):
    B, F = 3, 256
    dec = _decoder(opt, F)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in dec.conv_decoder.state_dict().items()}
    f = _feature(B, F).requires_grad_(True)
    cots = _cots(B)
    names, masks = _decoder_step(dec, f, cots)
    n_layers = 6 if opt is True else 3
    assert len([n for n in names if "dgrad" in n]) == n_layers and len([n for n in names if "dgrad" not in n]) == n_layers
    shapes = {4: (B, 3, 16, 16), 5: (B, 3, 32, 32), 6: (B, 3, 64, 64)}
    ref = T.decoder_train64(sd, f.detach().cpu().numpy(), {i: cots[i].numpy().reshape(shapes[i]) for i in cots}, masks=masks)
    for i in (4, 5, 6):                                          # (up to eight layers, each within 1e-5 of float64 on its own input)
        assert_close_rms(getattr(dec, "conv_pc%d" % i).detach().cpu().numpy().reshape(shapes[i]), ref["pc"][i], 1e-4, "pc%d" % i)
    worst = ("", 0.0)
    for k, p in dec.conv_decoder.named_parameters():
        got, want = p.grad.cpu().numpy(), ref["grads"][k]
        layer = k.rsplit(".conv.bias", 1)[0]
        if k.endswith("conv.bias") and (layer in ref["graw_abs"] or layer.rsplit(".conv", 1)[0] in ref["graw_abs"]):
            # a bias in front of a BatchNorm: analytically zero, judged in units of sum |g_raw|
            unit = ref["graw_abs"][layer if layer in ref["graw_abs"] else layer.rsplit(".conv", 1)[0]]
            assert np.all(np.abs(got - want) <= 1e-4 * unit), k
            continue
        e = T.rel_rms(got, want)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= 1e-4, (k, e)
    e = T.rel_rms(f.grad.cpu().numpy(), ref["dfeature"])
    print("decoder %s: worst parameter %s rel-rms %.3g, feature %.3g" % (opt, worst[0], worst[1], e))
    assert e <= 1e-4, ("feature", e)


# ------------------------------------------------------------------------------------------------------------ routing
F256 = ("256x256_1x1", "256x128_2x2", "128x64_4x4", "64x32_8x8", "32x32_16x16", "32x32_32x32")


def test_option_absent_changes_nothing():
    """No up-convolution launch in training, and the parent's bits: the two aten lines per layer, by hand, on a second decoder."""
    off, hand = _decoder(None), _decoder(None)
    assert all(getattr(off.conv_decoder, "deconv%d" % i).fused_train is False for i in range(1, 7))
    f, f2 = _feature(3, 256).requires_grad_(True), _feature(3, 256).requires_grad_(True)
    cots = _cots(3)
    with _reproducible_aten():
        names, _ = _decoder_step(off, f, cots)
        assert names == []
        dc = hand.conv_decoder
        x = f2.view(-1, 256, 1, 1)
        pcs = {}
        for i in range(1, 7):
            m = getattr(dc, "deconv%d" % i)
            x = m.conv(m.up_sample(x))
            if i >= 4:
                pcs[i] = getattr(dc, "conv2pc%d" % i)(x)
        sum((pcs[i].view(3, 3, -1) * cots[i].to(DEV)).sum() for i in (4, 5, 6)).backward()
    assert torch.equal(off.conv_pc6, pcs[6].view(-1, 3, 4096)) and torch.equal(f.grad, f2.grad)
    for (k, p), (_k2, q) in zip(off.conv_decoder.named_parameters(), hand.conv_decoder.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, p), (_k2, q) in zip(off.conv_decoder.named_buffers(), hand.conv_decoder.named_buffers()):
        assert torch.equal(p, q), k


def test_option_on_launches_six_forwards_and_six_input_gradients():
    on = _decoder(True)
    names, _ = _decoder_step(on, _feature(3, 256).requires_grad_(True), _cots(3))
    assert sorted(names) == sorted(["upconv3x3_" + s for s in F256] + ["upconv3x3_dgrad_" + s for s in F256])
    # a feature that needs no gradient: the first layer has no input gradient to compute
    on.zero_grad()
    names, _ = _decoder_step(on, _feature(3, 256), _cots(3))
    assert sorted(names) == sorted(["upconv3x3_" + s for s in F256] + ["upconv3x3_dgrad_" + s for s in F256[1:]])
    # opt.decoder_fused stays inference only: in training it launches nothing
    names, _ = _decoder_step(_decoder(None, fused=True), _feature(3, 256).requires_grad_(True), _cots(3))
    assert names == []


def test_layer_keeps_the_aten_path_where_it_must():
    from models import layers as L
    from sonet_hip import ops

    def launches(m, x):
        m.fused_train = True
        with ops.kernel_timing() as rec:
            y = m(x)
            if y.requires_grad:
                y.sum().backward()
        assert tuple(y.shape) == (x.shape[0], m.conv.conv.out_channels, 2 * x.shape[2], 2 * x.shape[3])
        return len([n for n, _a, _b in rec.records if n.startswith("upconv3x3")])

    torch.manual_seed(0)
    x = torch.randn(2, 16, 3, 5, device=DEV)
    m = L.UpConv(16, 32, activation="relu", normalization="batch").to(DEV).train()
    assert m.fused_train is False
    with ops.kernel_timing() as rec:
        m(x).sum().backward()
    assert [n for n, _a, _b in rec.records if n.startswith("upconv3x3")] == []          # off by default
    assert launches(m, x) == 1                                   # forward; x needs no gradient
    assert launches(m, x.clone().requires_grad_(True)) == 2
    assert launches(m.eval(), x.clone().requires_grad_(True)) == 0          # eval mode with autograd
    m.train()
    with ops.precision("x3"):
        assert launches(m, x) == 0
    for kw in (dict(activation="relu", normalization="instance"), dict(activation="leakyrelu", normalization="batch")):
        assert launches(L.UpConv(16, 32, **kw).to(DEV).train(), x) == 0
    assert launches(L.UpConv(16, 48, activation="relu", normalization="batch").to(DEV).train(), x) == 0
    assert launches(m, torch.randn(1, 16, 2, 65, device=DEV)) == 0          # W = 65: outside the operator's shapes, quietly aten


def test_both_packs_are_rebuilt_after_an_optimizer_step():
    from models import layers as L
    torch.manual_seed(1)
    m = L.UpConv(24, 32, activation=None, normalization=None).to(DEV).train()
    m.fused_train = True
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    x = torch.randn(2, 24, 4, 4, device=DEV)
    g = cu(T.make_g(2, 32, 4, 4, 8))

    def step():
        xi = x.clone().requires_grad_(True)
        opt.zero_grad()
        y = m(xi)
        y.backward(g)
        return y.detach(), xi.grad

    step()
    fw, bw = m._wup.clone(), m._wupt.clone()
    opt.step()
    y, dx = step()
    assert not torch.equal(m._wup, fw) and not torch.equal(m._wupt, bw)
    w, b = m.conv.conv.weight.detach().cpu().numpy(), m.conv.conv.bias.detach().cpu().numpy()
    assert_close_rms(y.cpu().numpy(), R.reference(x.cpu().numpy(), w, np.ones(32), b, False), 1e-5, "forward after the step")
    assert_close_rms(dx.cpu().numpy(), T.dgrad_folded(g.cpu().numpy(), w), 1e-5, "input gradient after the step")


# ------------------------------------------------------------------------------------------------------------ range guard
def test_training_range_violation_switches_to_x3_one_step_late():
    from sonet_hip import ops
    dec = _decoder(True)
    f = _feature(2, 256)
    bad = f.clone()
    bad[1, 200] = 1e5
    cots = _cots(2)
    old = ops.POINTMLP_PRECISION
    ops.POINTMLP_PRECISION, ops._range_warned = "h3", False
    ops._range_pending.clear()
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            names, _ = _decoder_step(dec, bad.requires_grad_(True), cots)
            torch.cuda.synchronize()
            assert len(names) == 12 and ops.POINTMLP_PRECISION == "h3"         # ran fused; the log has not been looked at yet
            names, _ = _decoder_step(dec, f.clone().requires_grad_(True), cots)
            assert ops.POINTMLP_PRECISION == "x3" and any("x3" in str(x.message) for x in w)
            assert names == []                                   # ... and the layers are on aten from this call on
    finally:
        ops.POINTMLP_PRECISION = old
        ops._range_pending.clear()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_a_launch():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    w, g = T.make_w(16, 32, 2), T.make_g(2, 32, 3, 5, 3)
    wpt, gd = ops.upconv3x3_dgrad_pack(cu(w)), cu(g)
    assert tuple(ops.upconv3x3_dgrad(gd, wpt, 16).shape) == (2, 16, 3, 5)
    with pytest.raises(SonetHipError, match="float32"):
        ops.upconv3x3_dgrad(gd.double(), wpt, 16)
    with pytest.raises(SonetHipError, match="float32"):
        ops.upconv3x3_dgrad(gd.half(), wpt, 16)
    with pytest.raises(SonetHipError, match="contiguous"):
        ops.upconv3x3_dgrad(cu(np.zeros((2, 32, 10, 6), np.float32)).transpose(2, 3), wpt, 16)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_dgrad(gd.cpu(), wpt, 16)
    with pytest.raises(SonetHipError, match="4-D"):
        ops.upconv3x3_dgrad(gd[0], wpt, 16)
    for H2, W2 in ((0, 10), (6, 0), (130, 10), (6, 130), (5, 10), (6, 9)):
        with pytest.raises(SonetHipError, match="unsupported shape"):
            ops.upconv3x3_dgrad(torch.zeros(2, 32, H2, W2, device=DEV), wpt, 16)
    with pytest.raises(SonetHipError, match="unsupported shape"):
        ops.upconv3x3_dgrad(torch.zeros(2, 48, 6, 10, device=DEV), wpt, 16)
    with pytest.raises(SonetHipError, match="unsupported shape"):
        ops.upconv3x3_dgrad(gd, wpt, 0)
    with pytest.raises(SonetHipError, match="packed weight has"):                  # a pack built for another shape
        ops.upconv3x3_dgrad(gd, wpt, 40)
    with pytest.raises(SonetHipError, match="packed weight has"):
        ops.upconv3x3_dgrad(torch.zeros(2, 64, 6, 10, device=DEV), wpt, 16)
    with pytest.raises(SonetHipError, match="packed weight has"):                  # the forward's pack is not the gradient's
        ops.upconv3x3_dgrad(gd, ops.upconv3x3_pack(cu(w)), 16)
    with pytest.raises(SonetHipError, match="input-gradient pack"):
        ops.upconv3x3_dgrad(gd, wpt.float(), 16)
    buf = torch.zeros(gd.numel() + 1, device=DEV)
    view = buf[1:].view_as(gd)                                   # contiguous, at a 4-byte offset: the 8-byte loads would be misaligned
    with pytest.raises(SonetHipError, match="aligned"):
        ops.upconv3x3_dgrad(view, wpt, 16)
    pbuf = torch.zeros(wpt.numel() + 1, dtype=torch.int32, device=DEV)
    with pytest.raises(SonetHipError, match="aligned"):
        ops.upconv3x3_dgrad(gd, pbuf[1:], 16)
    with pytest.raises(SonetHipError, match="3x3"):
        ops.upconv3x3_dgrad_pack(torch.zeros(32, 16, 1, 1, device=DEV))
    with pytest.raises(SonetHipError, match="multiple of 32"):
        ops.upconv3x3_dgrad_pack(torch.zeros(48, 16, 3, 3, device=DEV))
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_dgrad_pack(torch.zeros(32, 16, 3, 3))
