"""CPU tests of the up-convolution's folded weight gradient (no GPU needed): the folded form against float64 autograd and the mistakes it
must not make, the float64 model of the bf16-split arithmetic chained as the kernel chains it at the reduction depths the GPU tests use,
the workspace size as a function of the shape, the argument checks of the C entry and of the wrapper, and the decoder option."""
import ctypes

import numpy as np
import pytest
import torch

import upconv_ref as R
import upconv_train_ref as T
import upconv_wgrad_ref as G
import x3_model

SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (4, 4), (8, 8), (5, 30))


def _case(H, W, B=3, seed=0):
    Cin, Cout = (5, 4) if H * W <= 64 else (3, 2)
    g, x = G.make_case(B, Cin, Cout, H, W, seed=900 + 7 * H + W + seed)
    return g, x, Cin, Cout


# ------------------------------------------------------------------------------------------------------------ the folded gradient
@pytest.mark.parametrize("H,W", SHAPES)
def test_folded_gradient_equals_wgrad64_and_float64_autograd(H, W):
    g, x, Cin, Cout = _case(H, W)
    got = G.wgrad_folded(g, x)
    assert got.shape == (Cout, Cin, 3, 3)
    assert R.rms_error(got, T.wgrad64(np.asarray(g, np.float64), x)) <= 1e-12, (H, W)
    w, b = np.zeros((Cout, Cin, 3, 3), np.float32), np.zeros(Cout, np.float32)
    assert R.rms_error(got, T.autograd64(x, w, b, None, None, 1e-5, False, g)["dW"]) <= 1e-12, (H, W)
    Gg, Xg = G.wgrad_gemm(g, x)
    assert Gg.shape == (Cout, 16 * 3 * H * W) and Xg.shape == (16 * 3 * H * W, 9 * Cin)
    assert R.rms_error(x3_model.exact(Gg, Xg).reshape(got.shape), got) <= 1e-12          # the one GEMM is the folded form


@pytest.mark.parametrize("brk", G.BREAKS)
def test_each_break_of_the_folded_gradient_is_seen(brk):
    """A flipped shift sign, a dropped parity, the unfold table with parity and tap exchanged, a seam that is not zeroed, a slice that is
    never added: each is far from float64 on at least one of the shapes -- the last one on a map of 40 clouds, which has two slices."""
    red = []
    for (H, W) in SHAPES + ((3, 5),):
        B = 40 if len(red) == len(SHAPES) else 3
        g, x, _, _ = _case(H, W, B=B)
        if R.rms_error(G.wgrad_folded(g, x, brk), T.wgrad64(np.asarray(g, np.float64), x)) > 0.05:
            red.append((B, H, W))
        else:
            red.append(None)
    assert any(r is not None for r in red), brk
    if brk == "last_slice_dropped":
        assert G.plan(40, 5, 4, 3, 5)[0] == 2 and red[-1] == (40, 3, 5)
    if brk == "seam":
        assert red[SHAPES.index((1, 1))] is not None and red[SHAPES.index((3, 5))] is not None


# ------------------------------------------------------------------------------------------------------------ arithmetic model
# K = B H W of the GPU tests: one column, a partial step, whole steps, eight slices, the long case (128 slices of two chains)
MODEL_K = {1: (1, 1, 1), 15: (1, 3, 5), 64: (1, 8, 8), 4096: (4, 32, 32), 65536: (64, 32, 32)}


@pytest.mark.parametrize("K", sorted(MODEL_K))
@pytest.mark.parametrize("e", [0, -20, -40])
def test_float64_model_of_the_chained_bf16_split_stays_within_half_the_bound(K, e):
    """``wgrad_model``: the six piece products in float64, one f32 rounding per chain of 256 products, the chains of a slice added in f32,
    slices and unfold in float64 -- with g at gradient scale times 2^e.  Eight channels either side: the error is a matter of the
    reduction depth, not of the block count.  It meets 0.5e-5 at every K, the long case included: that GPU case is not shrunk."""
    B, H, W = MODEL_K[K]
    Cin = Cout = 8
    g, x = G.make_case(B, Cin, Cout, H, W, seed=K)
    g = np.ldexp(g, e).astype(np.float32)
    nslice, cols, _ = G.plan(B, Cin, Cout, H, W)
    assert B * H * W == K and nslice == max(1, min(-(-K // 512), 128))
    exact = G.wgrad_folded(g, x)
    err = max(R.rms_error(G.wgrad_model(g, x, flush), exact) for flush in (False, True))
    print("K = %d (%d slices of %d columns), g x 2^%d: model error %.3g" % (K, nslice, cols, e, err))
    assert err <= x3_model.CAP


@pytest.mark.parametrize("shape", T.INT_SHAPES + ((9, 20, 32, 8, 8),), ids=lambda s: "B%d_%dx%d_%dx%d" % s)
def test_the_integer_case_is_exact_by_derivation(shape):
    g, x = G.int_case(shape)                                     # (asserts the split and the 2^24 bound itself)
    ref = G.wgrad_folded(g, x)
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 2 ** 24
    assert np.array_equal(G.wgrad_model(g, x), ref)
    assert np.array_equal(ref, T.wgrad64(np.asarray(g, np.float64), x))
    if shape[0] == 9:
        assert G.plan(*shape)[0] == 2


# ------------------------------------------------------------------------------------------------------------ workspace, argument checks
def test_workspace_size_is_a_function_of_the_shape():
    from sonet_hip import _lib
    lib = _lib.load()
    size = lib.sonet_upconv3x3_wgrad_ws_size
    for args in ((2, 16, 48, 3, 5), (2, 16, 32, 65, 5), (2, 16, 32, 3, 65), (0, 16, 32, 3, 5), (2, 0, 32, 3, 5), (2, 16, 16, 3, 5),
                 (2 ** 30, 16, 32, 64, 64)):
        assert size(*args) == 0, args
    for args in ((1, 1, 32, 1, 1), (2, 16, 32, 3, 5), (3, 33, 64, 4, 4), (64, 32, 32, 32, 32), (64, 256, 256, 1, 1), (513, 17, 96, 1, 1),
                 (64, 1024, 1024, 32, 32)):
        n = size(*args)
        assert n > 0 and n % 16 == 0 and n == G.plan(*args)[2] and n == size(*args), args
    assert G.plan(1, 16, 32, 8, 8)[0] == 1 and G.plan(512, 16, 32, 1, 1)[0] == 1 and G.plan(513, 16, 32, 1, 1)[0] == 2
    assert G.plan(64, 32, 32, 32, 32)[:2] == (128, 512) and G.plan(64, 1024, 1024, 32, 32)[0] == 1          # the 64 MiB cap


def test_c_entry_validates_before_touching_the_device():
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 15) & ~15)
    inv, uns = 1, 2

    def call(g=p, x=p, dw=p, ws=p, B=2, Cin=16, Cout=32, H=3, W=5):
        return lib.sonet_upconv3x3_wgrad_f32(g, x, dw, ws, B, Cin, Cout, H, W, None)

    for name in ("g", "x", "dw", "ws"):
        assert call(**{name: None}) == inv and "NULL" in _lib.last_error(), name
    for kw in (dict(B=0), dict(Cin=0), dict(Cout=0), dict(H=0), dict(W=0), dict(B=-3)):
        assert call(**kw) == inv and "non-positive" in _lib.last_error(), kw
    for kw in (dict(Cout=48), dict(Cout=16), dict(H=65), dict(W=65), dict(H=1000)):
        assert call(**kw) == uns and "Cout" in _lib.last_error(), kw
    assert call(B=2 ** 30, H=64, W=64) == uns and "too large" in _lib.last_error()
    assert call(g=ctypes.c_void_p(p.value + 4)) == inv and "misaligned" in _lib.last_error()      # the two px of a row are one 8-byte load
    assert call(x=ctypes.c_void_p(p.value + 2)) == inv and "misaligned" in _lib.last_error()
    assert call(dw=ctypes.c_void_p(p.value + 2)) == inv and "misaligned" in _lib.last_error()
    assert call(ws=ctypes.c_void_p(p.value + 8)) == inv and "misaligned" in _lib.last_error()


def test_wrapper_refuses_cpu_tensors_and_bad_arguments_without_a_gpu():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    g, x = torch.zeros(2, 32, 6, 10), torch.zeros(2, 16, 3, 5)
    with pytest.raises(SonetHipError, match="CUDA"):
        ops.upconv3x3_wgrad(g, x)
    with pytest.raises(SonetHipError, match="torch.Tensor"):
        ops.upconv3x3_wgrad(g.numpy(), x)
    with pytest.raises(SonetHipError, match="torch.Tensor"):
        ops.upconv3x3_wgrad(None, x)
    assert (ops.UPWGRAD_K_STEP, ops.UPWGRAD_CIN_BLOCK, ops.UPWGRAD_FLUSH_COLS, ops.UPWGRAD_SLICE_COLS,
            ops.UPWGRAD_MAX_SLICES) == (G.K_STEP, G.CIN_BLOCK, G.FLUSH_COLS, G.SLICE_COLS, G.MAX_SLICES)


def test_header_exports_the_tile_extents_the_wrapper_names():
    import os
    import re
    from sonet_hip import ops
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "sonet_hip.h")) as f:
        defs = dict(re.findall(r"#define SONET_(UPWGRAD_\w+) (\d+)", f.read()))
    assert len(defs) == 5
    for k, v in defs.items():
        assert getattr(ops, k) == int(v), k


# ------------------------------------------------------------------------------------------------------------ the option
def test_decoder_option_sets_the_layer_attribute():
    from argparse import Namespace
    from models import layers as L
    from models import networks as NW
    assert L.UpConv(4, 32).fused_wgrad is False
    base = dict(feature_num=64, activation="relu", normalization="batch", output_conv_pc_num=4096, output_fc_pc_num=0)
    flags = lambda dc, a="fused_wgrad": [getattr(getattr(dc, "deconv%d" % i), a) for i in range(1, 7)]
    assert flags(NW.DecoderConv(Namespace(**base))) == [False] * 6
    assert flags(NW.DecoderConv(Namespace(decoder_fused_wgrad=False, **base))) == [False] * 6
    assert flags(NW.DecoderConv(Namespace(decoder_fused_wgrad=True, decoder_fused_train=True, **base))) == [True] * 6
    assert flags(NW.DecoderConv(Namespace(decoder_fused_wgrad=(4, 5, 6), **base))) == [False, False, False, True, True, True]
    dc = NW.DecoderConv(Namespace(decoder_fused_wgrad=[6], decoder_fused_train=(5, 6), **base))
    assert flags(dc) == [False] * 5 + [True] and flags(dc, "fused_train") == [False] * 4 + [True, True]
    dc = NW.DecoderConv(Namespace(decoder_fused_wgrad=True, **base))             # given without decoder_fused_train: set, and inert
    assert flags(dc) == [True] * 6 and flags(dc, "fused_train") == [False] * 6


def test_layer_on_the_cpu_behaves_as_today():
    """``fused_wgrad`` (with ``fused_train``) on a CPU tensor: the two aten lines, gradients included."""
    from models import layers as L
    torch.manual_seed(6)
    m = L.UpConv(6, 32, activation="relu", normalization="batch")
    ref = L.UpConv(6, 32, activation="relu", normalization="batch")
    ref.load_state_dict(m.state_dict())
    m.fused_train = m.fused_wgrad = True
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
