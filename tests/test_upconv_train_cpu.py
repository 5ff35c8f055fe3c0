"""CPU tests of the up-convolution's training path (no GPU needed): the folded input gradient against float64 autograd and the mistakes it
must not make, the float64 twin of the layer step against autograd and against the fixtures made from the live reference, the float64
model of the bf16-split arithmetic at the input gradient's reduction depths, the derivation behind the GPU tests' exact case, and the
argument checks of the C entries and of the wrappers."""
import ctypes
import os

import numpy as np
import pytest
import torch

import upconv_ref as R
import upconv_train_ref as T
import x3_model
from conftest import GOLDEN

EPS = 1e-5


_operands = T.make_layer_case


# ------------------------------------------------------------------------------------------------------------ the folded gradient
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_folded_gradient_equals_float64_autograd(H, W):
    B, Cin, Cout = (3, 5, 4) if H * W <= 64 else (1, 3, 2)
    o = _operands(B, Cin, Cout, H, W, 300 + 7 * H + W)
    want = T.autograd64(o["x"], o["w"], o["b"], None, None, EPS, False, o["g"])["dx"]
    got = T.dgrad_folded(o["g"], o["w"])
    assert got.shape == (B, Cin, H, W)
    assert R.rms_error(got, want) <= 1e-12, (H, W)


@pytest.mark.parametrize("brk", T.BREAKS)
def test_each_break_of_the_folded_gradient_is_seen(brk):
    """A flipped shift sign in one axis, a dropped parity, the tap table transposed, a seam that is not zeroed: each is far from autograd
    on a 3 x 5 map of three clouds -- and on the 2 x 2 map, where every pixel is a border pixel."""
    for (B, H, W) in ((3, 3, 5), (3, 2, 2)):
        o = _operands(B, 5, 4, H, W, 17 + H)
        want = T.autograd64(o["x"], o["w"], o["b"], None, None, EPS, False, o["g"])["dx"]
        assert R.rms_error(T.dgrad_folded(o["g"], o["w"], brk), want) > 0.1, (brk, H, W)


# ------------------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("H,W", R.SHAPES[:5])
@pytest.mark.parametrize("norm,relu", [(True, True), (True, False), (False, True), (False, False)], ids=["bn_relu", "bn", "relu", "plain"])
def test_twin_equals_float64_autograd(H, W, norm, relu):
    B, Cin, Cout = 3, 5, 4
    o = _operands(B, Cin, Cout, H, W, 500 + 7 * H + W)
    gamma, beta, running = (o["gamma"], o["beta"], o["running"]) if norm else (None, None, None)
    a = T.autograd64(o["x"], o["w"], o["b"], gamma, beta, EPS, relu, o["g"], running=running)
    t = T.layer_train64(o["x"], o["w"], o["b"], gamma, beta, EPS, relu, g=o["g"], running=running)
    keys = ["y", "pre", "dx", "dW"] + (["dgamma", "dbeta", "running_mean", "running_var"] if norm else [])
    for k in keys:
        assert R.rms_error(t[k], a[k]) <= 1e-12, (k, H, W)
    # the bias gradient is analytically zero behind a BatchNorm: an absolute bound in units of sum |g_raw|
    assert np.all(np.abs(t["db"] - a["db"]) <= 1e-12 * np.abs(t["g_raw"]).sum(axis=(0, 2, 3))), "db"
    # a forced mask is what the twin uses: the complement of its own mask gives the complementary routing
    if relu:
        f = T.layer_train64(o["x"], o["w"], o["b"], gamma, beta, EPS, relu, mask=1.0 - t["mask"], g=o["g"], running=running)
        assert np.array_equal(f["mask"], 1.0 - t["mask"]) and np.abs(f["y"] + np.maximum(-t["pre"], 0.0)).max() <= 1e-15


FIXTURES = T.FIXTURES


def fixture(name):
    return np.load(os.path.join(GOLDEN, "upconv_train", name + ".npz"), allow_pickle=False)


def twin_of_fixture(g, norm, act, mask=None):
    gamma, beta, running = ((g["conv__norm__weight"], g["conv__norm__bias"], (g["conv__norm__running_mean"], g["conv__norm__running_var"]))
                            if norm == "batch" else (None, None, None))
    return T.layer_train64(g["x"], g["conv__conv__weight"], g["conv__conv__bias"], gamma, beta, EPS, act == "relu", mask=mask, g=g["g"],
                           running=running)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_twin_meets_the_reference_fixture(name):
    Cin, Cout, act, norm, B, H, W = FIXTURES[name]
    g = fixture(name)
    assert g["x"].shape == (B, Cin, H, W) and g["x"].dtype == np.float32 and g["g"].shape == (B, Cout, 2 * H, 2 * W)
    assert g["y"].dtype == np.float64 and g["dx"].shape == (B, Cin, H, W) and g["dW"].shape == (Cout, Cin, 3, 3)
    t = twin_of_fixture(g, norm, act)
    pairs = dict(y="y", dx="dx", dW="dW")
    if norm == "batch":
        pairs.update(dgamma="dgamma", dbeta="dbeta", running_mean_after="running_mean", running_var_after="running_var")
    for k, mine in pairs.items():
        assert R.rms_error(t[mine], g[k]) <= 1e-12, (name, k)
    assert np.all(np.abs(t["db"] - g["dbias"]) <= 1e-12 * np.abs(t["g_raw"]).sum(axis=(0, 2, 3)))


def test_fixture_files_are_small_and_complete():
    d = os.path.join(GOLDEN, "upconv_train")
    assert sorted(os.listdir(d)) == [n + ".npz" for n in sorted(FIXTURES)]
    for f in os.listdir(d):
        assert os.path.getsize(os.path.join(d, f)) < 200 * 1024, f
    g = fixture("upconv_16x32_3x5")
    assert 1e-4 < float(np.abs(g["g"]).mean()) < 1e-2                      # gradient scale
    assert not np.array_equal(g["running_mean_after"], g["conv__norm__running_mean"])


# ------------------------------------------------------------------------------------------------------------ arithmetic model
@pytest.mark.parametrize("Cout,H,W,B", [(32, 3, 5, 3), (128, 3, 3, 2), (512, 2, 2, 4), (1024, 1, 1, 16)],
                         ids=["K16x32", "K16x128", "K9x512", "K4x1024"])
@pytest.mark.parametrize("e", [0, -20, -40])
def test_float64_model_of_the_bf16_split_stays_within_half_the_bound(Cout, H, W, B, e):
    """x3_model.model on the ONE GEMM of the input gradient -- the transposed folded weights rounded to f32 as the pack rounds them, the
    shifted parity planes of g -- with g at gradient scale times 2^e: the arithmetic has no operand range to leave."""
    Cin = 32
    w = T.make_w(Cin, Cout, seed=Cout + H)
    g = np.ldexp(T.make_g(B, Cout, H, W, seed=Cout + W + 1), e).astype(np.float32)
    Wg, Gg = T.dgrad_gemm(g, w)
    assert Wg.shape == (Cin, 16 * Cout) and Gg.shape == (16 * Cout, B * H * W)
    live = int((np.abs(Gg).reshape(16, Cout, -1).max(axis=1) > 0).sum(axis=0).max())          # (parity, tap) pairs the busiest pixel sees
    assert live == {1: 4, 2: 9}.get(min(H, W), 16)
    exact = T.dgrad_folded(g, w).transpose(1, 0, 2, 3).reshape(Cin, -1)
    assert x3_model.rms_error(x3_model.exact(Wg, Gg), exact) <= 1e-6                          # the GEMM is the folded form (f32-rounded sums)
    err = x3_model.model_error(Wg, Gg)
    print("K = %d x %d, g x 2^%d: model error %.3g" % (live, Cout, e, err))
    assert err <= x3_model.CAP


INT_SHAPES, int_case = T.INT_SHAPES, T.int_case


@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "B%d_%dx%d_%dx%d" % s)
def test_the_integer_case_is_exact_by_derivation(shape):
    """g in [-2, 2] and w in [-3, 3], integers: a folded weight is a sum of at most four w, |wf| <= 12, an integer below 2^8 -- its h piece
    is the value itself and the m, l pieces are zero; the same for g.  Each of the six products of the kernel is then either wf g (an
    integer) or zero, and every partial sum of an output is an integer bounded by sum |wf| |g| <= 9 . 3 . 2 . Cout < 2^24: exact in f32
    whatever the order.  The kernel's output must therefore EQUAL the float64 gradient."""
    g, w = int_case(shape)
    Cout = shape[2]
    Wg, Gg = T.dgrad_gemm(g, w)
    for v in (Wg, Gg):
        h, m, l = x3_model.split3(v)
        assert np.array_equal(h, v) and not m.any() and not l.any()
    assert np.abs(Wg).max() <= 12 and np.abs(Gg).max() <= 2
    worst = (np.abs(Wg).astype(np.float64) @ np.abs(Gg).astype(np.float64)).max()
    assert worst <= 9 * 3 * 2 * Cout < 2 ** 24
    ref = T.dgrad_folded(g, w)
    assert np.array_equal(ref, np.round(ref)) and np.array_equal(x3_model.model(Wg, Gg).reshape(ref.transpose(1, 0, 2, 3).shape), ref.transpose(1, 0, 2, 3))


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_c_entries_validate_before_touching_the_device():
    from sonet_hip import _lib
    lib = _lib.load()
    assert lib.sonet_upconv3x3_dgrad_pack_size(16, 32) == 1 * 2 * 16 * 3072
    assert lib.sonet_upconv3x3_dgrad_pack_size(33, 64) == 2 * 4 * 16 * 3072
    assert lib.sonet_upconv3x3_dgrad_pack_size(1024, 1024) == 32 * 64 * 16 * 3072
    for Cin, Cout in ((0, 32), (16, 0), (16, 48), (-1, 32), (16, 16)):
        assert lib.sonet_upconv3x3_dgrad_pack_size(Cin, Cout) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 15) & ~15)
    inv, uns = 1, 2
    assert lib.sonet_upconv3x3_dgrad_pack_f32(None, p, 16, 32, None) == inv and "NULL" in _lib.last_error()
    assert lib.sonet_upconv3x3_dgrad_pack_f32(p, None, 16, 32, None) == inv
    assert lib.sonet_upconv3x3_dgrad_pack_f32(p, p, 0, 32, None) == inv and "non-positive" in _lib.last_error()
    assert lib.sonet_upconv3x3_dgrad_pack_f32(p, p, 16, 48, None) == uns and "multiple of 32" in _lib.last_error()
    assert lib.sonet_upconv3x3_dgrad_pack_f32(p, ctypes.c_void_p(p.value + 4), 16, 32, None) == inv and "misaligned" in _lib.last_error()

    def call(g=p, wpt=p, dx=p, B=2, Cin=16, Cout=32, H=3, W=5):
        return lib.sonet_upconv3x3_dgrad_f32(g, wpt, dx, B, Cin, Cout, H, W, None)

    for name in ("g", "wpt", "dx"):
        assert call(**{name: None}) == inv and "NULL" in _lib.last_error(), name
    for kw in (dict(B=0), dict(Cin=0), dict(Cout=0), dict(H=0), dict(W=0), dict(B=-3)):
        assert call(**kw) == inv and "non-positive" in _lib.last_error(), kw
    for kw in (dict(Cout=48), dict(Cout=16), dict(H=65), dict(W=65), dict(H=1000)):                # the forward's refusals
        assert call(**kw) == uns and "Cout" in _lib.last_error(), kw
    assert call(B=2 ** 30, H=64, W=64) == uns and "too large" in _lib.last_error()
    odd = ctypes.c_void_p(p.value + 4)
    assert call(wpt=odd) == inv and "misaligned" in _lib.last_error()
    assert call(g=odd) == inv and "misaligned" in _lib.last_error()                               # the two px of a row are one 8-byte load
    assert call(dx=ctypes.c_void_p(p.value + 2)) == inv and "misaligned" in _lib.last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_shapes_without_a_gpu():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    g, w = torch.zeros(2, 32, 6, 10), torch.zeros(32, 16, 3, 3)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_dgrad_pack(w)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_dgrad(g, torch.zeros(8, dtype=torch.int32), 16)
    with pytest.raises(SonetHipError, match="torch.Tensor"):
        ops.upconv3x3_dgrad(g.numpy(), None, 16)
    with pytest.raises(SonetHipError, match="torch.Tensor"):
        ops.upconv3x3_dgrad_pack(w.numpy())


def test_layer_on_the_cpu_behaves_as_today():
    """``fused_train`` on a CPU tensor: the two aten lines, in training and in eval mode, gradients included."""
    from models import layers as L
    torch.manual_seed(5)
    m = L.UpConv(6, 32, activation="relu", normalization="batch")
    assert m.fused_train is False
    ref = L.UpConv(6, 32, activation="relu", normalization="batch")
    ref.load_state_dict(m.state_dict())
    m.fused_train = True
    x = torch.randn(2, 6, 3, 5)
    outs = []
    for mod in (m, ref):
        mod.train()
        xi = x.clone().requires_grad_(True)
        y = mod(xi)
        y.square().sum().backward()
        outs.append((y.detach(), xi.grad, mod.conv.conv.weight.grad, mod.conv.norm.running_mean.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(m.eval()(x), ref.eval()(x))


def test_decoder_option_sets_the_layer_attribute():
    from argparse import Namespace
    from models import networks as NW
    base = dict(feature_num=64, activation="relu", normalization="batch", output_conv_pc_num=4096, output_fc_pc_num=0)
    flags = lambda dc: [getattr(dc, "deconv%d" % i).fused_train for i in range(1, 7)]
    assert flags(NW.DecoderConv(Namespace(**base))) == [False] * 6
    assert flags(NW.DecoderConv(Namespace(decoder_fused_train=True, **base))) == [True] * 6
    assert flags(NW.DecoderConv(Namespace(decoder_fused_train=(4, 5, 6), **base))) == [False, False, False, True, True, True]
    assert flags(NW.DecoderConv(Namespace(decoder_fused_train=[2], decoder_fused=True, **base))) == [False, True, False, False, False, False]
    dc = NW.DecoderConv(Namespace(decoder_fused=True, **base))
    assert flags(dc) == [False] * 6 and all(getattr(dc, "deconv%d" % i).fused for i in range(1, 7))      # decoder_fused stays inference only
