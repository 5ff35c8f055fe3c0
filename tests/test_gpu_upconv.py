"""GPU tests of the fused up-convolution (sonet_upconv3x3_f32, ops.upconv3x3, opt.decoder_fused).

  * float64 parity of the operator at the project's metric, |y - ref| <= 1e-5 max(|ref|, rms(ref)), against upconv_ref.reference (the
    reference's upsample + conv in float64): every map size of the decoder, the edges of the kernel's tile extents, K tails, several
    Cout blocks, ReLU on and off, a non-trivial affine;
  * an exact case (small integers: every product and sum is exact in the fp16-split arithmetic) that must match bit for bit;
  * the operand-range guard, the reference's own outputs (tests/golden/upconv, the autoencoder fixtures), routing, reproducibility and
    HIP-graph capture, refusals.
"""
import contextlib
from argparse import Namespace

import numpy as np
import pytest
import torch

import h3_model
import upconv_ref as R
from conftest import assert_close_rms, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_op(x, w, scale, shift, relu):
    from sonet_hip import ops
    wp = ops.upconv3x3_pack(cu(w))
    return ops.upconv3x3(cu(x), wp, cu(scale), cu(shift), relu, w.shape[0])


def _tile():
    from sonet_hip import ops
    return ops.UPCONV_TILE_PIXELS, ops.UPCONV_K_CHUNK, ops.UPCONV_COUT_BLOCK


# (B, Cin, Cout, H, W, relu)
PARITY = [
    (64, 1024, 1024, 1, 1, True),          # deconv1 as shipped: three taps of four skipped, K = 1024 per parity
    (64, 1024, 96, 2, 2, True),            # deconv2's input (two column tiles), every tap live somewhere, K = 4 * 1024
    (3, 1024, 32, 2, 2, False),
    (1, 1, 32, 1, 1, False),               # the smallest launch there is
    (3, 1, 32, 3, 5, True),
    (1, 16, 32, 1, 2, True),
    (3, 24, 96, 2, 2, False),
    (3, 40, 32, 3, 5, True),               # K tail, odd map, 45 columns of three clouds in one tile
    (1, 24, 32, 4, 4, False),
    (3, 16, 96, 8, 8, True),               # 192 columns: the tile seam falls inside cloud 1
    (1, 40, 128, 16, 16, False),
    (3, 128, 128, 16, 16, True),           # deconv5's shape
    (1, 128, 128, 32, 32, True),           # deconv6's shape
    (3, 16, 32, 32, 32, False),
    (127, 16, 32, 1, 1, True),             # one column below the tile extent
    (2, 24, 32, 8, 8, False),              # exactly one tile
    (3, 16, 32, 1, 43, True),              # one column above: the second tile holds a single column
    (1, 15, 32, 2, 64, True),              # the widest row (halo of 65 columns on either side), one channel below the K chunk
    (1, 17, 96, 64, 64, False),            # the largest map, one channel above the K chunk
    (1, 16, 32, 5, 30, True),              # 150 columns: the seam falls inside a row
]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "B%d_%dx%d_%dx%d_%s" % (c[0], c[1], c[2], c[3], c[4], "relu" if c[5] else "lin"))
def test_operator_matches_float64(case):
    B, Cin, Cout, H, W, relu = case
    TP, KC, CB = _tile()
    assert Cout % CB == 0
    x, w, scale, shift = R.make_case(B, Cin, Cout, H, W, seed=sum(case) + 7 * H)
    y = run_op(x, w, scale, shift, relu)
    assert tuple(y.shape) == (B, Cout, 2 * H, 2 * W) and y.dtype == torch.float32
    ref = R.reference(x, w, scale, shift, relu)
    print("upconv %s: err / bound %.3f" % (case, R.rms_error(y.cpu().numpy(), ref) / 1e-5))
    assert_close_rms(y.cpu().numpy(), ref, 1e-5, "upconv3x3 %s" % (case,))


def test_tile_edges_are_covered():
    """The parity cases above sit one below, at and one above the exported pixel extent, and on both sides of the K chunk."""
    TP, KC, CB = _tile()
    cols = {c[0] * c[3] * c[4] for c in PARITY}
    assert {TP - 1, TP, TP + 1} <= cols
    assert {KC - 1, KC, KC + 1} <= {c[1] for c in PARITY}
    assert {CB, 3 * CB, 4 * CB} <= {c[2] for c in PARITY}


@pytest.mark.parametrize("shape", [(2, 64, 32, 1, 1), (3, 33, 64, 2, 2), (2, 20, 32, 3, 5), (3, 40, 32, 8, 8), (1, 64, 32, 5, 30)],
                         ids=lambda s: "B%d_%dx%d_%dx%d" % s)
def test_exact_case_is_bit_identical(shape):
    """Integer x in [-2, 2] and w in [-3, 3]: 32 x, 32 (sums of up to four w) are exact in fp16 with zero residuals, every product and
    every partial sum (below 2^24 / 1024) is exact in f32 -- the output must equal the reference bit for bit.  A wrong tap, parity or
    border shows here as a plain mismatch."""
    B, Cin, Cout, H, W = shape
    rng = np.random.default_rng(11 * Cin + H)
    x = rng.integers(-2, 3, (B, Cin, H, W)).astype(np.float32)
    w = rng.integers(-3, 4, (Cout, Cin, 3, 3)).astype(np.float32)
    one, zero = np.ones(Cout, np.float32), np.zeros(Cout, np.float32)
    for relu in (False, True):
        y = run_op(x, w, one, zero, relu).cpu().numpy()
        ref = R.reference(x, w, one, zero, relu)
        assert np.abs(ref).max() < 2 ** 14 and np.array_equal(ref, np.round(ref))
        bad = np.argwhere(y.astype(np.float64) != ref)
        assert bad.size == 0, "%d mismatches, first at %s: got %r want %r" % (len(bad), bad[0], y[tuple(bad[0])], ref[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------------------ range guard
def test_range_guard_reports_each_violation():
    from sonet_hip import ops
    x, w, scale, shift = R.make_case(3, 24, 32, 3, 5, seed=5)

    def bad_of(x, w):
        with ops.range_scope(DEV) as rs:
            run_op(x, w, scale, shift, True)
        return rs.violations()

    assert bad_of(x, w) == []
    for v, what in ((1e5, "exceeds 2047"), (-1e5, "exceeds 2047"), (np.nan, "exceeds 2047"), (np.inf, "exceeds 2047")):
        xb = x.copy()
        xb[2, 23, 2, 4] = v                                  # the last channel (inside the K tail), the last column
        bad = bad_of(xb, w)
        assert len(bad) == 1 and bad[0][0] == "upconv3x3_24x32_3x5" and "|x|" in bad[0][1] and what in bad[0][1], (v, bad)
    wb = w.copy()
    wb[31, 23, 1, 1] = np.float32(h3_model.w_high("h3p")) * np.float32(1.001)          # the centre tap: only ever inside a sum
    bad = bad_of(x, wb)
    assert len(bad) == 1 and "|w|" in bad[0][1] and "exceeds 2047" in bad[0][1], bad
    wb = w.copy()
    wb[0, 0, 0, 0] = np.float32(h3_model.w_high("h3p"))                                  # on the limit: admitted
    wb[0, 0, 0, 1:] = 0
    wb[0, 0, 1:, :] = 0
    assert bad_of(x, wb) == []
    wb[5, 3, 2, 2] = np.nan
    assert len(bad_of(x, wb)) == 1


def _small_decoder(fused, F=256, seed=31, fc=0):
    """Decoder at feature_num F (every Cout of its six up-convolutions a multiple of 32 for F = 256), seeded weights."""
    from models import networks as NW
    from sonet_hip import synth
    opt = Namespace(gpu_id=0, device=torch.device(DEV), feature_num=F, activation="relu", normalization="batch",
                    output_fc_pc_num=fc, output_conv_pc_num=4096)
    if fused is not None:
        opt.decoder_fused = fused
    dec = NW.Decoder(opt)
    synth.fill_state_dict_(dec.state_dict(), seed)
    return dec.to(DEV).eval()


def _feature(B, F, seed=3):
    return torch.randn(B, F, generator=torch.Generator().manual_seed(seed)).abs().to(DEV)


@contextlib.contextmanager
def _reproducible_aten():
    """The aten path is compared bit for bit with itself below.  With the library's default solver choice the 3x3 convolutions of
    deconv1 - deconv3 are not reproducible from one call to the next (the option-off decoder differs from itself in its last bits);
    under ``torch.backends.cudnn.deterministic`` they are, so both sides of every such comparison run under it."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = old


def _upconv_counts(rec):
    """launch name -> count of the up-convolution launches a kernel_timing record holds (no event is read: no synchronisation needed)."""
    out = {}
    for name, _e0, _e1 in rec.records:
        if name.startswith("upconv3x3"):
            out[name] = out.get(name, 0) + 1
    return out


def test_decoder_reruns_a_violating_batch_in_x3():
    """A feature outside the fp16-split range: run_guarded re-runs the forward under precision("x3"), where the layer takes the aten
    path -- the result is, bit for bit, what the option-off decoder returns under precision("x3")."""
    import warnings
    from sonet_hip import ops
    on, off = _small_decoder(True), _small_decoder(None)
    f = _feature(2, 256)
    f[1, 200] = 1e5
    with torch.no_grad(), _reproducible_aten(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with ops.kernel_timing() as rec:
            got = on(f)
        assert sum(_upconv_counts(rec).values()) == 6           # the first attempt ran fused; the re-run did not
        with ops.precision("x3"):
            want = off(f)
    assert torch.equal(got, want)
    for name in ("conv_pc4", "conv_pc5", "conv_pc6"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name


# ------------------------------------------------------------------------------------------------------------ the reference's outputs
def _load_upconv(g, Cin, Cout, act, norm):
    from models import layers as L
    m = L.UpConv(Cin, Cout, activation=act, normalization=norm)
    sd = m.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in g["keys"]]
    for k in sd:
        if not k.endswith("num_batches_tracked"):
            sd[k].copy_(torch.from_numpy(g[k.replace(".", "__")]))
    m.fused = True
    return m.to(DEV).eval()


@pytest.mark.parametrize("name,spec", [("upconv_16x32_3x5", (16, 32, "relu", "batch")), ("upconv_40x32_1x1", (40, 32, None, None))])
def test_reference_upconv_fixture(name, spec):
    from sonet_hip import ops
    g = golden("upconv/" + name)
    m = _load_upconv(g, *spec)
    with torch.no_grad(), ops.kernel_timing() as rec:
        y = m(cu(g["x"]))
    assert sum(_upconv_counts(rec).values()) == 1
    assert_close_rms(y.cpu().numpy(), g["y"], 1e-5, name)


def test_reference_decoderconv_fixture():
    """The reference's DecoderConv at feature_num 64: deconv1 / deconv2 (Cout 64, 32) run fused, the four narrower layers keep the aten path."""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden("upconv/decoderconv_f64")
    opt = Namespace(gpu_id=0, device=torch.device(DEV), feature_num=int(g["feature_num"]), activation="relu", normalization="batch",
                    output_fc_pc_num=0, output_conv_pc_num=4096, decoder_fused=True)
    dc = NW.DecoderConv(opt)
    assert sorted(dc.state_dict().keys()) == [str(k) for k in g["keys"]]
    synth.fill_state_dict_(dc.state_dict(), int(g["seed"]))
    dc.to(DEV).eval()
    with torch.no_grad(), ops.kernel_timing() as rec:
        pc6 = dc(cu(g["feature"]))
    assert _upconv_counts(rec) == {"upconv3x3_64x64_1x1": 1, "upconv3x3_64x32_2x2": 1}
    assert_close_rms(dc.pc4.cpu().numpy(), g["pc4"], 1e-5, "pc4")
    assert_close_rms(dc.pc5.cpu().numpy(), g["pc5"], 1e-5, "pc5")
    assert_close_rms(pc6.cpu().numpy(), g["pc6"], 1e-5, "pc6")


@pytest.mark.parametrize("case", ["autoencoder_b2_n1024", "autoencoder_b2_n5000"])
def test_decoder_fused_meets_the_autoencoder_fixtures(case):
    """Decoder(decoder_fused=True) on the stored feature of the reference's autoencoder run: predicted_pc and conv_pc4 at 1e-5."""
    from models import networks as NW
    from sonet_hip import ops, synth
    g = golden(case)
    B, N, seed = int(g["B"]), int(g["N"]), int(g["seed"])
    opt = Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg",
                    bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40,
                    output_fc_pc_num=256, output_conv_pc_num=1024, decoder_fused=True)
    dec = NW.Decoder(opt)
    assert sorted(dec.state_dict().keys()) == [str(k) for k in g["decoder_keys"]]
    synth.fill_state_dict_(dec.state_dict(), seed + 1)
    dec.to(DEV).eval()
    with torch.no_grad(), ops.kernel_timing() as rec:
        pred = dec(cu(g["feature"]))
    assert sum(_upconv_counts(rec).values()) == 6
    assert_close_rms(pred.cpu().numpy(), g["predicted_pc"], 1e-5, "predicted_pc")
    assert_close_rms(dec.conv_pc4.cpu().numpy(), g["conv_pc4"], 1e-5, "conv_pc4")


def test_evaluate_autoencoder_with_the_option_on():
    """11 clouds in batches of 4 (the last one of 3) through evaluate_autoencoder, option on against option off.  Both decoders are
    within 1e-5 of float64 per coordinate (coordinates of order 1) and the Chamfer terms are 1-Lipschitz in the points, so the two test
    losses (of order 0.1 - 1) differ by a few 1e-5 at most: bound 1e-4 relative."""
    from models import networks as NW
    from sonet_hip import metrics, ops, synth
    from sonet_hip.batch import BatchAssembler, DeviceClouds
    S, n, N, M, BS = 11, 300, 256, 16, 4
    g = np.random.RandomState(43)
    pts = [g.uniform(-1, 1, size=(n, 3)).astype(np.float32) for _ in range(S)]
    nrm = [(p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32) for p in pts]
    nodes = np.stack([p[g.choice(n, M, replace=False)] for p in pts]).astype(np.float32)
    res = {}
    for fused in (False, True):
        opt = Namespace(gpu_id=0, device=DEV, batch_size=BS, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
                        normalization="batch", dropout=0.7, node_num=M, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                        bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40, output_fc_pc_num=256, output_conv_pc_num=1024,
                        decoder_fused=fused)
        enc, dec = NW.Encoder(opt), NW.Decoder(opt)
        synth.fill_state_dict_(enc.state_dict(), 15)
        synth.fill_state_dict_(dec.state_dict(), 16)
        enc.to(DEV)
        dec.to(DEV)
        clouds = DeviceClouds(pts, nrm, np.zeros(S, np.int64), nodes=nodes, device=DEV)
        A = BatchAssembler(clouds, opt, "test", "modelnet", seed=4)
        with ops.kernel_timing() as rec:
            res[fused] = metrics.evaluate_autoencoder(enc, dec, A, BS)
            torch.cuda.synchronize()
        assert sum(_upconv_counts(rec).values()) == (18 if fused else 0)
    print("evaluate_autoencoder: fused", res[True], "aten", res[False])
    assert res[True]["count"] == S
    for k in ("test_loss", "forward", "backward"):
        assert abs(res[True][k] - res[False][k]) <= 1e-4 * res[False][k], (k, res)


# ------------------------------------------------------------------------------------------------------------ routing
def test_option_absent_changes_nothing_and_option_on_launches_six():
    from sonet_hip import ops
    off, on = _small_decoder(None), _small_decoder(True)
    assert all(getattr(off.conv_decoder, "deconv%d" % i).fused is False for i in range(1, 7))
    f = _feature(3, 256)
    with torch.no_grad(), _reproducible_aten():
        with ops.kernel_timing() as rec:
            got = off(f)
        assert _upconv_counts(rec) == {}
        # the parent's path, by hand: upsample, then the MyConv2d
        x = f.view(-1, 256, 1, 1)
        dc = off.conv_decoder
        for i in range(1, 7):
            m = getattr(dc, "deconv%d" % i)
            x = m.conv(m.up_sample(x))
        want = dc.conv2pc6(x).view(-1, 3, 4096)
        assert torch.equal(got, want)
        with ops.kernel_timing() as rec:
            fused = on(f)
        assert sorted(_upconv_counts(rec).items()) == sorted({"upconv3x3_256x256_1x1": 1, "upconv3x3_256x128_2x2": 1, "upconv3x3_128x64_4x4": 1,
                                                              "upconv3x3_64x32_8x8": 1, "upconv3x3_32x32_16x16": 1,
                                                              "upconv3x3_32x32_32x32": 1}.items())
    assert_close_rms(fused.cpu().numpy(), got.double().cpu().numpy(), 2e-5, "fused decoder vs aten decoder (each within 1e-5 of float64)")


def test_layer_keeps_the_aten_path_where_it_must():
    from models import layers as L
    from sonet_hip import ops

    def launches(m, x, grad=False):
        with ops.kernel_timing() as rec:
            if grad:
                y = m(x)
            else:
                with torch.no_grad():
                    y = m(x)
        assert tuple(y.shape) == (x.shape[0], m.conv.conv.out_channels, 2 * x.shape[2], 2 * x.shape[3])
        return sum(_upconv_counts(rec).values())

    torch.manual_seed(0)
    x = torch.randn(2, 16, 3, 5, device=DEV)
    m = L.UpConv(16, 32, activation="relu", normalization="batch").to(DEV).eval()
    assert launches(m, x) == 0                                   # fused is off by default
    m.fused = True
    assert launches(m, x) == 1
    assert launches(m, x, grad=True) == 0                        # autograd on, an untagged tensor
    assert launches(m, ops.mark_inference(x.clone()), grad=True) == 1
    assert launches(m, x.clone().requires_grad_(True), grad=True) == 0
    assert launches(m.train(), x) == 0                           # training mode
    m.eval()
    with ops.precision("x3"):
        assert launches(m, x) == 0
    inst = L.UpConv(16, 32, activation="relu", normalization="instance").to(DEV).eval()
    inst.fused = True
    assert launches(inst, x) == 0
    odd = L.UpConv(16, 48, activation="relu", normalization="batch").to(DEV).eval()
    odd.fused = True
    assert launches(odd, x) == 0
    wide = torch.randn(1, 16, 2, 65, device=DEV)
    assert launches(m, wide) == 0                                # W = 65: outside the operator's shapes, quietly aten
    leaky = L.UpConv(16, 32, activation="leakyrelu", normalization="batch").to(DEV).eval()
    leaky.fused = True
    assert launches(leaky, x) == 0


def test_weight_changed_in_place_is_repacked():
    from models import layers as L
    torch.manual_seed(1)
    m = L.UpConv(24, 32, activation=None, normalization=None).to(DEV).eval()
    m.fused = True
    x = torch.randn(2, 24, 4, 4, device=DEV)
    with torch.no_grad():
        y0 = m(x)
        m.conv.conv.weight.mul_(-2.0)
        m.conv.conv.bias.add_(0.5)
        y1 = m(x)
    w, b = m.conv.conv.weight.detach().cpu().numpy(), m.conv.conv.bias.detach().cpu().numpy()
    one = np.ones(32, np.float32)
    assert_close_rms(y1.cpu().numpy(), R.reference(x.cpu().numpy(), w, one, b, False), 1e-5, "after the in-place change")
    assert_close_rms(y0.cpu().numpy(), R.reference(x.cpu().numpy(), w / -2.0, one, b - 0.5, False), 1e-5, "before it")


# ------------------------------------------------------------------------------------------------------------ reproducibility, capture
def test_two_runs_and_a_graph_replay_are_bit_identical():
    from sonet_hip import ops
    from sonet_hip.graph import GraphedForward
    x, w, scale, shift = R.make_case(3, 40, 96, 8, 8, seed=9)
    a, b = run_op(x, w, scale, shift, True), run_op(x, w, scale, shift, True)
    assert torch.equal(a, b)
    dec = _small_decoder(True)
    f = _feature(2, 256)
    with torch.no_grad():
        eager = dec(f).clone()
        eager2 = dec(f).clone()
    assert torch.equal(eager, eager2)
    fwd = GraphedForward(lambda t: dec(t), (f,))
    out = fwd(f)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert fwd.range_violations() == []
    assert sum(1 for n in fwd.range.names if n.startswith("upconv3x3")) == 6
    f2 = _feature(2, 256, seed=4)
    with torch.no_grad():
        want = dec(f2).clone()
    assert torch.equal(fwd(f2), want)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_a_launch():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    x, w, scale, shift = R.make_case(2, 16, 32, 3, 5, seed=2)
    wp = ops.upconv3x3_pack(cu(w))
    xs, sc, sh = cu(x), cu(scale), cu(shift)
    assert tuple(ops.upconv3x3(xs, wp, sc, sh, True, 32).shape) == (2, 32, 6, 10)
    with pytest.raises(SonetHipError, match="float32"):
        ops.upconv3x3(xs.double(), wp, sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="float32"):
        ops.upconv3x3(xs.half(), wp, sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="contiguous"):
        ops.upconv3x3(cu(np.zeros((2, 16, 5, 3), np.float32)).transpose(2, 3), wp, sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3(xs.cpu(), wp, sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3(xs, wp, sc.cpu(), sh, True, 32)
    with pytest.raises(SonetHipError, match="4-D"):
        ops.upconv3x3(xs[0], wp, sc, sh, True, 32)
    for H, W in ((0, 5), (3, 0), (65, 5), (3, 65)):
        with pytest.raises(SonetHipError, match="unsupported shape"):
            ops.upconv3x3(torch.zeros(2, 16, H, W, device=DEV), wp, sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="unsupported shape"):
        ops.upconv3x3(xs, wp, sc[:16].contiguous(), sh[:16].contiguous(), True, 16)
    with pytest.raises(SonetHipError, match="unsupported shape"):
        ops.upconv3x3(xs, wp, torch.zeros(48, device=DEV), torch.zeros(48, device=DEV), True, 48)
    with pytest.raises(SonetHipError, match="C = 32 elements"):
        ops.upconv3x3(xs, wp, sc[:31].contiguous(), sh, True, 32)
    with pytest.raises(SonetHipError, match="packed weight has"):                  # a pack built for another shape
        ops.upconv3x3(torch.zeros(2, 40, 3, 5, device=DEV), wp, sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="packed weight has"):
        ops.upconv3x3(xs, wp, torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), True, 64)
    with pytest.raises(SonetHipError, match="up-convolution pack"):
        ops.upconv3x3(xs, wp.float(), sc, sh, True, 32)
    with pytest.raises(SonetHipError, match="3x3"):
        ops.upconv3x3_pack(torch.zeros(32, 16, 1, 1, device=DEV))
    with pytest.raises(SonetHipError, match="multiple of 32"):
        ops.upconv3x3_pack(torch.zeros(48, 16, 3, 3, device=DEV))
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_pack(torch.zeros(32, 16, 3, 3))
