"""GPU tests of the up-convolution's folded weight gradient (sonet_upconv3x3_wgrad_f32, ops.upconv3x3_wgrad, UpConv.fused_wgrad,
opt.decoder_fused_wgrad).

  * the operator against float64 (upconv_train_ref.wgrad64) at the project's f32-class gate, |dW - ref| <= 1e-5 max(|ref|, rms(ref)), on
    every map size that takes another path through the shifts (one pixel, single rows and columns, cloud seams inside an eight-column
    group, a 128-column seam inside a row), Cin tails and several blocks, one column count below, at and above every extent the kernel
    tiles by, one slice and 128 slices, g at gradient scale and 2^-30 below it;
  * an exact case (small integers; upconv_wgrad_ref.int_case derives why) that must match float64 bit for bit;
  * reproducibility, HIP-graph capture, a workspace and an output first filled with 0xFF bytes, NaN isolation;
  * the layer and the decoder against the float64 twins of tests/upconv_train_ref.py with THIS run's ReLU masks forced, routing by launch
    names, an optimizer step, refusals.
"""
import numpy as np
import pytest
import torch

import test_gpu_upconv_train as TR
import upconv_ref as R
import upconv_train_ref as T
import upconv_wgrad_ref as G
from conftest import assert_close_rms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
cu = TR.cu


def run_wgrad(g, x):
    from sonet_hip import ops
    return ops.upconv3x3_wgrad(cu(g), cu(x))


def _names(rec, prefix="upconv3x3"):
    return [n for n, _a, _b in rec.records if n.startswith(prefix)]


# ------------------------------------------------------------------------------------------------------------ operator against float64
# (B, Cin, Cout, H, W)
LONG = (64, 32, 32, 32, 32)                # K = 65 536: 128 slices of two chains each; g is 33 MB
OPERATOR = [
    (2, 16, 32, 1, 1), (2, 16, 32, 1, 2), (2, 16, 32, 2, 1), (2, 16, 32, 2, 2), (2, 16, 32, 1, 7), (2, 16, 32, 7, 1), (2, 16, 32, 8, 8),
    (2, 16, 32, 2, 64), (2, 16, 32, 64, 2),                      # every map shape: one pixel, rows, columns, the widest and the tallest
    (3, 16, 32, 3, 5),                     # 15 columns per cloud: cloud seams inside an eight-column group
    (1, 16, 32, 5, 30),                    # 150 columns in rows of 30: the 128-column seam falls inside a row
    (2, 1, 32, 3, 5), (2, 15, 32, 3, 5), (2, 17, 32, 3, 5), (2, 31, 32, 3, 5), (2, 32, 32, 3, 5), (2, 33, 32, 3, 5), (2, 128, 32, 3, 5),
    (2, 32, 96, 2, 2), (2, 32, 128, 2, 2), (64, 16, 32, 2, 2),
    (15, 16, 32, 1, 1), (16, 16, 32, 1, 1), (17, 16, 32, 1, 1),             # the 16-column step
    (255, 16, 32, 1, 1), (256, 16, 32, 1, 1), (257, 16, 32, 1, 1),          # the 256-column chain
    (511, 16, 32, 1, 1), (512, 16, 32, 1, 1), (513, 16, 32, 1, 1),          # the 512-column slice: one slice, one slice, two slices
    (4, 16, 32, 32, 32),                   # K = 4096: eight slices
    (1, 16, 32, 1, 4), (5, 16, 32, 1, 4), (3, 16, 32, 2, 4), (3, 17, 32, 4, 4),       # W % 4 == 0 (16-byte loads): 4, 20, 24, 48 columns
    LONG,
]


@pytest.mark.parametrize("case", OPERATOR, ids=lambda c: "B%d_%dx%d_%dx%d" % c)
def test_operator_matches_float64(case):
    B, Cin, Cout, H, W = case
    g, x = G.make_case(B, Cin, Cout, H, W, seed=sum(case))
    ref = T.wgrad64(np.asarray(g, np.float64), x)               # (the long case: nine einsums over 64 upsampled maps, two seconds)
    for e in (0, -30):                                           # (a power of two scales the float64 gradient exactly)
        dW = run_wgrad(np.ldexp(g, e).astype(np.float32), x)
        assert tuple(dW.shape) == (Cout, Cin, 3, 3) and dW.dtype == torch.float32
        print("upconv wgrad %s x 2^%d: err / bound %.3f" % (case, e, R.rms_error(dW.cpu().numpy(), np.ldexp(ref, e)) / 1e-5))
        assert_close_rms(dW.cpu().numpy(), np.ldexp(ref, e), 1e-5, "upconv3x3_wgrad %s x 2^%d" % (case, e))


def test_operator_cases_cover_the_tile_edges():
    from sonet_hip import ops
    cols = {c[0] * c[3] * c[4] for c in OPERATOR}
    for ext in (ops.UPWGRAD_K_STEP, ops.UPWGRAD_FLUSH_COLS, ops.UPWGRAD_SLICE_COLS):
        assert {ext - 1, ext, ext + 1} <= cols, ext
    CB = ops.UPWGRAD_CIN_BLOCK
    assert {1, CB // 2 - 1, CB // 2, CB // 2 + 1, CB - 1, CB, CB + 1, 4 * CB} <= {c[1] for c in OPERATOR}         # Cin tails, several blocks
    assert {ops.UPCONV_COUT_BLOCK, 3 * ops.UPCONV_COUT_BLOCK, 4 * ops.UPCONV_COUT_BLOCK} <= {c[2] for c in OPERATOR}
    assert {1, 3, 64} <= {c[0] for c in OPERATOR}
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (7, 1), (3, 5), (8, 8), (2, 64), (64, 2), (5, 30)} <= {(c[3], c[4]) for c in OPERATOR}
    slices = {c: G.plan(*c)[0] for c in OPERATOR}
    assert 1 in slices.values() and slices[LONG] == ops.UPWGRAD_MAX_SLICES                    # one slice, and as many as there can be
    assert G.plan(*LONG)[1] >= 2 * ops.UPWGRAD_FLUSH_COLS                                     # ... of several chains each
    assert slices[(513, 16, 32, 1, 1)] == 2 and slices[(512, 16, 32, 1, 1)] == 1
    assert any((c[3], c[4]) == (1, 1) for c in OPERATOR)         # the map on which four of the sixteen pairs are left


@pytest.mark.parametrize("shape", T.INT_SHAPES + ((9, 20, 32, 8, 8),), ids=lambda s: "B%d_%dx%d_%dx%d" % s)
def test_integer_case_is_bit_identical(shape):
    """Integer g in [-2, 2] and x in [-3, 3]: every piece, product and partial sum is exact (upconv_wgrad_ref.int_case) -- the output equals
    the float64 gradient.  A wrong tap, parity, shift, border or a slice left out shows here as a plain mismatch.  The last shape has two
    slices."""
    g, x = G.int_case(shape)
    dW = run_wgrad(g, x).cpu().numpy().astype(np.float64)
    ref = G.wgrad_folded(g, x)
    bad = np.argwhere(dW != ref)
    assert bad.size == 0, "%d mismatches, first at %s: got %r want %r" % (len(bad), bad[0], dW[tuple(bad[0])], ref[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------------------ reproducibility, isolation
def test_two_runs_and_a_graph_replay_are_bit_identical():
    from sonet_hip import ops
    B, Cin, Cout, H, W = 40, 40, 96, 4, 4                        # 640 columns: two slices, a Cin tail
    g, x = G.make_case(B, Cin, Cout, H, W, 9)
    gd, xd = cu(g), cu(x)
    a, b = ops.upconv3x3_wgrad(gd, xd), ops.upconv3x3_wgrad(gd, xd)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.upconv3x3_wgrad(gd, xd)                              # (warm-up on the capture stream)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            out = ops.upconv3x3_wgrad(gd, xd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    gd.mul_(-2.0).add_(1e-4)                                     # the graph reads the operand in place
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, a) and torch.equal(out, ops.upconv3x3_wgrad(gd, xd))


def test_operands_at_an_8_byte_offset_give_the_same_bits():
    """W % 4 == 0 takes 16-byte loads when g and x are 16-byte aligned and single elements otherwise: the same values in the same order."""
    from sonet_hip import ops
    for shape in ((3, 17, 32, 4, 4), (40, 20, 64, 2, 8)):
        B, Cin, Cout, H, W = shape
        g, x = G.make_case(B, Cin, Cout, H, W, 33)
        gd, xd = cu(g), cu(x)
        want = ops.upconv3x3_wgrad(gd, xd)
        gbuf, xbuf = torch.zeros(gd.numel() + 2, device=DEV), torch.zeros(xd.numel() + 1, device=DEV)
        g8, x4 = gbuf[2:].view_as(gd).copy_(gd), xbuf[1:].view_as(xd).copy_(xd)
        assert g8.data_ptr() % 16 == 8 and x4.data_ptr() % 16 == 4
        assert torch.equal(ops.upconv3x3_wgrad(g8, xd), want) and torch.equal(ops.upconv3x3_wgrad(gd, x4), want), shape


def test_workspace_and_output_are_fully_overwritten():
    """The C entry on a workspace and a dw first filled with 0xFF bytes (NaN bit patterns): the same bits as the wrapper's run."""
    from sonet_hip import _lib, ops
    from sonet_hip.ops import check, ptr, stream_ptr
    lib = _lib.load()
    for shape in ((40, 17, 32, 4, 4), (2, 33, 64, 1, 1)):        # two slices with a Cin tail; the four-pairs-only map, two Cin blocks
        B, Cin, Cout, H, W = shape
        g, x = G.make_case(B, Cin, Cout, H, W, 21)
        gd, xd = cu(g), cu(x)
        want = ops.upconv3x3_wgrad(gd, xd)
        ws = torch.full((lib.sonet_upconv3x3_wgrad_ws_size(B, Cin, Cout, H, W),), 0xFF, dtype=torch.uint8, device=DEV)
        dw = torch.full((Cout * Cin * 9 * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).view(Cout, Cin, 3, 3)
        assert torch.isnan(dw).all()
        check(lib.sonet_upconv3x3_wgrad_f32(ptr(gd), ptr(xd), ptr(dw), ptr(ws), B, Cin, Cout, H, W, stream_ptr()), "sonet_upconv3x3_wgrad_f32")
        torch.cuda.synchronize()
        assert torch.equal(dw, want), shape


def test_a_nan_stays_inside_its_row_or_its_column():
    B, Cin, Cout, H, W = 3, 20, 32, 5, 6
    g, x = G.make_case(B, Cin, Cout, H, W, 4)
    clean = run_wgrad(g, x).cpu().numpy()
    for (Y, X) in ((0, 0), (9, 11), (4, 7)):
        gb = g.copy()
        gb[1, 7, Y, X] = np.nan
        got = run_wgrad(gb, x).cpu().numpy()
        assert np.isnan(got[7]).any() and not np.isnan(np.delete(got, 7, axis=0)).any()
        assert np.array_equal(np.delete(got, 7, axis=0), np.delete(clean, 7, axis=0)), (Y, X)
    for (i, j) in ((0, 0), (4, 5), (2, 3)):
        xb = x.copy()
        xb[2, 13, i, j] = np.nan
        got = run_wgrad(g, xb).cpu().numpy()
        assert np.isnan(got[:, 13]).any() and not np.isnan(np.delete(got, 13, axis=1)).any()
        assert np.array_equal(np.delete(got, 13, axis=1), np.delete(clean, 13, axis=1)), (i, j)


# ------------------------------------------------------------------------------------------------------------ the layer
def _run_layer(Cin, Cout, act, norm, o, wgrad):
    """tests/test_gpu_upconv_train._run_layer with ``fused_wgrad`` set on the module it builds."""
    from models import layers as L
    init = L.UpConv.__init__

    def patched(self, *a, **kw):
        init(self, *a, **kw)
        self.fused_wgrad = wgrad

    L.UpConv.__init__ = patched
    try:
        return TR._run_layer(Cin, Cout, act, norm, o)
    finally:
        L.UpConv.__init__ = init


@pytest.mark.parametrize("name", ["upconv_16x32_3x5", "upconv_40x32_1x1", "seeded_33x64_4x4"])
def test_layer_step_with_the_folded_weight_gradient(name):
    Cin, Cout, act, norm, o = TR._layer_case(name)
    relu, H, W = act == "relu", o["x"].shape[2], o["x"].shape[3]
    r, r2 = _run_layer(Cin, Cout, act, norm, o, True), _run_layer(Cin, Cout, act, norm, o, True)          # (no deterministic-aten switch)
    base = _run_layer(Cin, Cout, act, norm, o, False)
    tag = "%dx%d_%dx%d" % (Cin, Cout, H, W)
    assert r["names"] == ["upconv3x3_" + tag, "upconv3x3_dgrad_" + tag, "upconv3x3_wgrad_" + tag]
    assert base["names"] == ["upconv3x3_" + tag, "upconv3x3_dgrad_" + tag]
    assert torch.equal(r["dW"], r2["dW"])
    for k in r:
        if k not in ("names", "dW"):
            assert torch.equal(r[k], base[k]), "%s differs from the layer with fused_train alone" % k
    mask = (r["y"].cpu().numpy() > 0).astype(np.float64) if relu else None
    t = T.layer_train64(o["x"], o["w"], o["b"], o["gamma"], o["beta"], 1e-5, relu, mask=mask, g=o["g"], running=o["running"])
    e, e0 = T.rel_rms(r["dW"].cpu().numpy(), t["dW"]), T.rel_rms(base["dW"].cpu().numpy(), t["dW"])
    print("%s dW: rel-rms %.3g folded, %.3g aten" % (name, e, e0))
    assert e <= 1e-4, (name, e)


# ------------------------------------------------------------------------------------------------------------ the decoder
def _decoder(train_opt, wgrad_opt, F=256, seed=31):
    from argparse import Namespace
    from models import networks as NW
    from sonet_hip import synth
    opt = Namespace(gpu_id=0, device=torch.device(DEV), feature_num=F, activation="relu", normalization="batch",
                    output_fc_pc_num=0, output_conv_pc_num=4096)
    if train_opt is not None:
        opt.decoder_fused_train = train_opt
    if wgrad_opt is not None:
        opt.decoder_fused_wgrad = wgrad_opt
    dec = NW.Decoder(opt)
    synth.fill_state_dict_(dec.state_dict(), seed)
    return dec.to(DEV).train()


@pytest.mark.parametrize("opt", [True, (4, 5, 6)], ids=["all", "layers456"])
def test_decoder_gradients_match_the_float64_chain_with_forced_masks(opt):
    B, F = 3, 256
    dec = _decoder(True, opt, F)
    sd = {k: v.detach().cpu().numpy().copy() for k, v in dec.conv_decoder.state_dict().items()}
    f = TR._feature(B, F).requires_grad_(True)
    cots = TR._cots(B)
    names, masks = TR._decoder_step(dec, f, cots)
    assert len([n for n in names if "wgrad" in n]) == (6 if opt is True else 3)
    shapes = {4: (B, 3, 16, 16), 5: (B, 3, 32, 32), 6: (B, 3, 64, 64)}
    ref = T.decoder_train64(sd, f.detach().cpu().numpy(), {i: cots[i].numpy().reshape(shapes[i]) for i in cots}, masks=masks)
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
    print("decoder wgrad %s: worst parameter %s rel-rms %.3g, feature %.3g" % (opt, worst[0], worst[1], e))
    assert e <= 1e-4, ("feature", e)


# ------------------------------------------------------------------------------------------------------------ routing
F256 = TR.F256


def _split(names):
    fw = sorted(n for n in names if "dgrad" not in n and "wgrad" not in n)
    return fw, sorted(n for n in names if "dgrad" in n), sorted(n for n in names if "wgrad" in n)


def test_both_options_launch_six_of_each():
    names, _ = TR._decoder_step(_decoder(True, True), TR._feature(3, 256).requires_grad_(True), TR._cots(3))
    assert _split(names) == (sorted("upconv3x3_" + s for s in F256), sorted("upconv3x3_dgrad_" + s for s in F256),
                             sorted("upconv3x3_wgrad_" + s for s in F256))
    names, _ = TR._decoder_step(_decoder(True, (4, 5, 6)), TR._feature(3, 256).requires_grad_(True), TR._cots(3))
    assert _split(names) == (sorted("upconv3x3_" + s for s in F256), sorted("upconv3x3_dgrad_" + s for s in F256),
                             sorted("upconv3x3_wgrad_" + s for s in F256[3:]))
    # a feature that needs no gradient: still six weight gradients, five input gradients
    names, _ = TR._decoder_step(_decoder(True, True), TR._feature(3, 256), TR._cots(3))
    assert len(_split(names)[2]) == 6 and _split(names)[1] == sorted("upconv3x3_dgrad_" + s for s in F256[1:])
    # a frozen weight has no gradient to compute
    dec = _decoder(True, True)
    dec.conv_decoder.deconv5.conv.conv.weight.requires_grad_(False)
    names, _ = TR._decoder_step(dec, TR._feature(3, 256).requires_grad_(True), TR._cots(3))
    assert _split(names)[2] == sorted("upconv3x3_wgrad_" + s for s in F256[:4] + F256[5:]) and len(_split(names)[1]) == 6
    assert dec.conv_decoder.deconv5.conv.conv.weight.grad is None


def test_weight_gradient_option_alone_changes_nothing():
    """``decoder_fused_wgrad`` without ``decoder_fused_train``: no launch, and the bits of a decoder built without either option."""
    on, off = _decoder(None, True), _decoder(None, None)
    assert all(getattr(on.conv_decoder, "deconv%d" % i).fused_wgrad is True for i in range(1, 7))
    f, f2 = TR._feature(3, 256).requires_grad_(True), TR._feature(3, 256).requires_grad_(True)
    cots = TR._cots(3)
    with TR._reproducible_aten():
        names, _ = TR._decoder_step(on, f, cots)
        names2, _ = TR._decoder_step(off, f2, cots)
    assert names == [] and names2 == []
    assert torch.equal(on.conv_pc6, off.conv_pc6) and torch.equal(f.grad, f2.grad)
    for (k, p), (_k2, q) in zip(on.conv_decoder.named_parameters(), off.conv_decoder.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, p), (_k2, q) in zip(on.conv_decoder.named_buffers(), off.conv_decoder.named_buffers()):
        assert torch.equal(p, q), k


def test_weight_gradient_follows_an_optimizer_step():
    from models import layers as L
    torch.manual_seed(1)
    m = L.UpConv(24, 32, activation=None, normalization=None).to(DEV).train()
    m.fused_train = m.fused_wgrad = True
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    g = cu(T.make_g(2, 32, 4, 4, 8))
    xs = [torch.randn(2, 24, 4, 4, device=DEV), torch.randn(2, 24, 4, 4, device=DEV)]
    for x in xs:                                                 # second step: new weights, new input -- nothing stale is reused
        opt.zero_grad()
        m(x.clone().requires_grad_(True)).backward(g)
        dW = m.conv.conv.weight.grad.cpu().numpy()
        assert_close_rms(dW, T.wgrad64(g.cpu().numpy().astype(np.float64), x.cpu().numpy()), 1e-5, "dW")
        opt.step()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_a_launch():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    g, x = G.make_case(2, 16, 32, 3, 5, 3)
    gd, xd = cu(g), cu(x)
    assert tuple(ops.upconv3x3_wgrad(gd, xd).shape) == (32, 16, 3, 3)
    with ops.kernel_timing() as rec:
        for bad_g, bad_x, what in ((gd.double(), xd, "float32"), (gd, xd.half(), "float32"), (gd.cpu(), xd, "CUDA"), (gd, xd.cpu(), "CUDA"),
                                   (gd[0], xd, "4-D"), (gd, xd[0], "4-D"),
                                   (cu(np.zeros((2, 32, 10, 6), np.float32)).transpose(2, 3), xd, "contiguous"),
                                   (gd, cu(np.zeros((2, 16, 5, 3), np.float32)).transpose(2, 3), "contiguous")):
            with pytest.raises(SonetHipError, match=what):
                ops.upconv3x3_wgrad(bad_g, bad_x)
        for gs, xs in (((2, 32, 6, 10), (3, 16, 3, 5)), ((2, 32, 6, 10), (2, 16, 3, 4)), ((2, 32, 5, 10), (2, 16, 3, 5)),
                       ((2, 48, 6, 10), (2, 16, 3, 5)), ((2, 32, 130, 10), (2, 16, 65, 5)), ((2, 32, 6, 130), (2, 16, 3, 65)),
                       ((2, 32, 0, 10), (2, 16, 0, 5)), ((0, 32, 6, 10), (0, 16, 3, 5)), ((2, 32, 6, 10), (2, 0, 3, 5))):
            with pytest.raises(SonetHipError, match="unsupported shape"):
                ops.upconv3x3_wgrad(torch.zeros(gs, device=DEV), torch.zeros(xs, device=DEV))
        buf = torch.zeros(gd.numel() + 1, device=DEV)
        with pytest.raises(SonetHipError, match="aligned"):      # contiguous, at a 4-byte offset: the 8-byte loads would be misaligned
            ops.upconv3x3_wgrad(buf[1:].view_as(gd), xd)
    assert _names(rec) == []
