"""CPU tests of the fused up-convolution (no GPU needed): the folded four-parity form against the reference's expression, the float64
model of its fp16-split arithmetic at the decoder's reduction depths, the fixtures made from the live reference, and the argument
checks of the C entries and of the wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import h3_model
import upconv_ref as R
from conftest import GOLDEN, ROOT, assert_close_rms

CAP = 0.5e-5                           # the arithmetic's half of the project's 1e-5 (tests/test_h3_envelope_cpu.py)


# ------------------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_folded_form_equals_the_reference_expression(H, W):
    B, Cin, Cout = (2, 5, 4) if H * W <= 64 else (1, 3, 2)
    x, w, scale, shift = R.make_case(B, Cin, Cout, H, W, seed=100 + H * 7 + W)
    for relu in (False, True):
        ref = R.reference(x, w, scale, shift, relu)
        got = R.folded(x, w, scale, shift, relu)
        assert ref.shape == (B, Cout, 2 * H, 2 * W)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (H, W, relu)


def test_a_fold_with_one_swapped_tap_breaks_the_agreement():
    x, w, scale, shift = R.make_case(2, 5, 4, 3, 5, seed=1)
    ref = R.reference(x, w, scale, shift, False)
    wrong = (((0,), (1, 2)), ((0,), (1, 2)))                                          # parity 1 given parity 0's taps
    swapped = (((1, 2), (0,)), ((0, 1), (2,)))                                        # parity 0's two taps exchanged
    for fold in (wrong, swapped):
        assert np.abs(R.folded(x, w, scale, shift, False, fold=fold) - ref).max() > 1e-2 * np.abs(ref).max()
    # ... and at 1 x 1 every output pixel sees the whole 2 x 2 block of the kernel that overlaps the single input pixel
    x1, w1, s1, h1 = R.make_case(1, 2, 2, 1, 1, seed=2, affine=False)
    y = R.reference(x1, w1, s1, h1, False)
    assert y.shape == (1, 2, 2, 2)
    for py in range(2):
        for px in range(2):
            blk = w1[:, :, 1 - py:3 - py, 1 - px:3 - px].astype(np.float64).sum(axis=(2, 3))         # taps that land on the one real pixel
            assert np.allclose(y[0, :, py, px], blk @ x1[0, :, 0, 0].astype(np.float64), rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------------------ arithmetic model
@pytest.mark.parametrize("Cin,Cout,H,W,B", [(1024, 32, 2, 2, 16), (128, 32, 8, 8, 4), (24, 32, 8, 8, 4)],
                         ids=["K4x1024", "K4x128", "K4x24_tail"])
def test_float64_model_of_the_split_stays_within_half_the_bound(Cin, Cout, H, W, B):
    """h3_model.model(..., "h3p") on the folded weights (rounded to f32 as the pack rounds them) and the shifted activations of each
    output parity, decoder-scaled operands: weights of standard deviation sqrt(2 / (9 Cout)), activations of order 1."""
    x, w, _, _ = R.make_case(B, Cin, Cout, H, W, seed=Cin + H)
    assert abs(float(w.std()) / np.sqrt(2.0 / (9 * Cout)) - 1) < 0.05 and 0.9 < float(x.std()) < 1.1
    exact = R.conv_folded(x, w)
    got = np.zeros_like(exact)
    for py in range(2):
        for px in range(2):
            Wg, Xg = R.parity_gemm(x, w, py, px)
            assert Wg.shape == (Cout, 4 * Cin) and Xg.shape == (4 * Cin, B * H * W)
            # inside the launch-side limits of the guard (what the kernel's range log is held to)
            assert h3_model.X_LOW <= np.abs(Xg).max() <= h3_model.X_HIGH and h3_model.W_LOW <= np.abs(Wg).max() <= h3_model.w_high("h3p")
            y = h3_model.model(Xg, Wg, "h3p")
            got[:, :, py::2, px::2] = y.reshape(Cout, B, H, W).transpose(1, 0, 2, 3)
    err = h3_model.rms_error(got, exact)
    print("K = 4 x %d: model error %.3g" % (Cin, err))
    assert err <= CAP


# ------------------------------------------------------------------------------------------------------------ reference fixtures
UPCONV_FIXTURES = {"upconv_16x32_3x5": (16, 32, "relu", "batch", 3, 3, 5), "upconv_40x32_1x1": (40, 32, None, None, 5, 1, 1)}


def _fixture(name):
    return np.load(os.path.join(GOLDEN, "upconv", name + ".npz"), allow_pickle=False)


@pytest.mark.parametrize("name", sorted(UPCONV_FIXTURES))
def test_restatement_meets_the_reference_fixture(name):
    Cin, Cout, act, norm, B, H, W = UPCONV_FIXTURES[name]
    g = _fixture(name)
    assert g["x"].shape == (B, Cin, H, W) and g["y"].shape == (B, Cout, 2 * H, 2 * W) and g["y"].dtype == np.float32
    assert ("conv__norm__running_var" in g.files) == (norm == "batch")
    scale, shift = R.eval_affine(g, Cout)
    for fn in (R.reference, R.folded):
        assert_close_rms(g["y"], fn(g["x"], g["conv__conv__weight"], scale, shift, act == "relu"), 1e-6, "%s vs %s" % (name, fn.__name__))


def test_fixture_files_are_small_and_complete():
    d = os.path.join(GOLDEN, "upconv")
    assert sorted(os.listdir(d)) == ["decoderconv_f64.npz", "upconv_16x32_3x5.npz", "upconv_40x32_1x1.npz"]
    for f in os.listdir(d):
        assert os.path.getsize(os.path.join(d, f)) < 200 * 1024, f
    g = _fixture("decoderconv_f64")
    assert g["feature"].shape == (2, 64) and g["pc4"].shape == (2, 3, 16, 16) and g["pc5"].shape == (2, 3, 32, 32) and g["pc6"].shape == (2, 3, 64, 64)
    for k in ("pc4", "pc5", "pc6"):
        assert g[k].dtype == np.float32 and np.isfinite(g[k]).all() and float(np.abs(g[k]).max()) > 0.1
    # the keys the fixture was made with are the keys of this project's DecoderConv: the seed fills both alike
    from argparse import Namespace
    from models import networks as NW
    dc = NW.DecoderConv(Namespace(feature_num=64, activation="relu", normalization="batch", output_conv_pc_num=4096, output_fc_pc_num=0))
    assert sorted(dc.state_dict().keys()) == [str(k) for k in g["keys"]]


def test_decoderconv_fixture_on_the_cpu_aten_path():
    """The decoder fixture against this project's DecoderConv on the CPU -- the aten path every unsupported case keeps."""
    from argparse import Namespace
    from models import networks as NW
    from sonet_hip import synth
    g = _fixture("decoderconv_f64")
    opt = Namespace(feature_num=64, activation="relu", normalization="batch", output_conv_pc_num=4096, output_fc_pc_num=0, decoder_fused=True)
    dc = NW.DecoderConv(opt)
    synth.fill_state_dict_(dc.state_dict(), int(g["seed"]))
    dc.eval()
    assert all(getattr(dc, "deconv%d" % i).fused for i in range(1, 7))
    x = torch.from_numpy(g["feature"]).view(-1, 64, 1, 1)
    with torch.no_grad():
        for i in range(1, 5):                                # the 3x3 layers run on aten on a CPU tensor (the point heads are GPU-only)
            x = getattr(dc, "deconv%d" % i)(x)
    assert tuple(x.shape) == (2, 8, 16, 16) and torch.isfinite(x).all()


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_exported_extents_match_the_header():
    from sonet_hip import ops
    src = open(os.path.join(ROOT, "include", "sonet_hip.h")).read()
    macros = dict(re.findall(r"#define (SONET_UPCONV_[A-Z_]+) (\d+)", src))
    assert {k: int(v) for k, v in macros.items()} == {"SONET_UPCONV_TILE_PIXELS": ops.UPCONV_TILE_PIXELS, "SONET_UPCONV_K_CHUNK": ops.UPCONV_K_CHUNK,
                                                      "SONET_UPCONV_COUT_BLOCK": ops.UPCONV_COUT_BLOCK, "SONET_UPCONV_MAX_HW": ops.UPCONV_MAX_HW}
    assert ops.upconv3x3_supported(1, 32, 1, 1) and ops.upconv3x3_supported(1024, 1024, 64, 64) and ops.upconv3x3_supported(40, 96, 3, 5)
    for bad in ((0, 32, 1, 1), (16, 0, 1, 1), (16, 48, 1, 1), (16, 16, 1, 1), (16, 32, 0, 1), (16, 32, 1, 0), (16, 32, 65, 1), (16, 32, 1, 65)):
        assert not ops.upconv3x3_supported(*bad), bad


def test_c_entries_validate_before_touching_the_device():
    from sonet_hip import _lib
    lib = _lib.load()
    assert lib.sonet_upconv3x3_pack_size(16, 32) == 1 * 1 * 16 * 2048 + 64
    assert lib.sonet_upconv3x3_pack_size(17, 64) == 2 * 2 * 16 * 2048 + 64
    assert lib.sonet_upconv3x3_pack_size(1024, 1024) == 32 * 64 * 16 * 2048 + 64
    for Cin, Cout in ((0, 32), (16, 0), (16, 48), (-1, 32), (16, 16)):
        assert lib.sonet_upconv3x3_pack_size(Cin, Cout) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok, inv, uns = 0, 1, 2
    assert lib.sonet_upconv3x3_pack_f32(None, p, 16, 32, None) == inv and "NULL" in _lib.last_error()
    assert lib.sonet_upconv3x3_pack_f32(p, None, 16, 32, None) == inv
    assert lib.sonet_upconv3x3_pack_f32(p, p, 0, 32, None) == inv and "non-positive" in _lib.last_error()
    assert lib.sonet_upconv3x3_pack_f32(p, p, 16, 48, None) == uns and "multiple of 32" in _lib.last_error()

    def call(x=p, wp=p, sc=p, sh=p, y=p, B=2, Cin=16, Cout=32, H=3, W=5):
        return lib.sonet_upconv3x3_f32(x, wp, sc, sh, 1, y, B, Cin, Cout, H, W, None, None)

    for name in ("x", "wp", "sc", "sh", "y"):
        assert call(**{name: None}) == inv and "NULL" in _lib.last_error(), name
    for kw in (dict(B=0), dict(Cin=0), dict(Cout=0), dict(H=0), dict(W=0), dict(B=-3)):
        assert call(**kw) == inv and "non-positive" in _lib.last_error(), kw
    for kw in (dict(Cout=48), dict(Cout=16), dict(H=65), dict(W=65), dict(H=1000)):
        assert call(**kw) == uns and "Cout" in _lib.last_error(), kw
    assert call(B=2 ** 30, H=64, W=64) == uns and "too large" in _lib.last_error()
    odd = ctypes.c_void_p(p.value + 4)
    assert call(wp=odd) == inv and "misaligned" in _lib.last_error()
    assert call(y=odd) == inv and "misaligned" in _lib.last_error()
    assert ok == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes_without_a_gpu():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    x, w = torch.zeros(2, 16, 3, 5), torch.zeros(32, 16, 3, 3)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_pack(w)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3(x, torch.zeros(8, dtype=torch.int32), torch.ones(32), torch.zeros(32), True, 32)
    with pytest.raises(SonetHipError, match="torch.Tensor"):
        ops.upconv3x3(x.numpy(), None, None, None, True, 32)


def test_layer_on_the_cpu_keeps_the_aten_path_with_the_attribute_set():
    from models import layers as L
    torch.manual_seed(3)
    m = L.UpConv(6, 32, activation="relu", normalization="batch").eval()
    assert m.fused is False
    x = torch.randn(2, 6, 3, 5)
    with torch.no_grad():
        want = m(x)
        m.fused = True
        got = m(x)
    assert torch.equal(got, want) and tuple(got.shape) == (2, 32, 6, 10)
    sd = m.state_dict()
    scale = (sd["conv.norm.weight"] / torch.sqrt(sd["conv.norm.running_var"] + 1e-5)).double().numpy()
    shift = ((sd["conv.conv.bias"] - sd["conv.norm.running_mean"]).double().numpy() * scale + sd["conv.norm.bias"].double().numpy())
    assert_close_rms(got.numpy(), R.reference(x.numpy(), sd["conv.conv.weight"].numpy(), scale, shift, True), 1e-5, "aten UpConv on the CPU")
