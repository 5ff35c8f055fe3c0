"""KNNModule's second layer in one launch (so-net_amd/csrc/knn_layer.hip, ``sonet_knn_layer2_gmax_p16``): h1 -- the first layer per neighbour
copy -- is built in LDS instead of being written by ``sonet_knn_stage_input_p16`` and read back by ``sonet_pointmlp_h3p_gmax``.  The launch
promises the planes and the range words of those two launches BIT FOR BIT (one copy of the h1 arithmetic, the same accumulation order, the
same epilogue), so every check here is ``torch.equal`` against the two-launch path; the encoder route is also held to the CPU oracle."""
import warnings
from argparse import Namespace

import pytest
import torch

from conftest import assert_close_rms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SONET_ERR_UNSUPPORTED = 2            # include/sonet_hip.h


def cu(t):
    return t.to(DEV).contiguous()


def _case(B, M, K, KI, Cin, Cout, avg, seed=0):
    """Inputs as test_knn_stage_prepare_and_input_equal_prepare_gather_lead builds them (neighbour ids at -1 and at M included) + a random
    second layer with some negative scales."""
    from sonet_hip import ops
    g = torch.Generator().manual_seed(B + M + K + Cin + Cout + seed)
    coord = cu(torch.randn(B, 3, M, generator=g))
    I = torch.randint(0, M, (B, M, KI), generator=g)
    I[:, :, 0] = torch.arange(M)
    I[0, 3, 1] = M                                                   # ids nobody owns
    I[B - 1, M - 1, K - 1] = -1
    I = cu(I)
    Lm = ops.node_stage_columns(B, M)
    zf = torch.zeros(1, Cin, Lm)
    zf[0, :, :B * M] = torch.randn(Cin, B * M, generator=g)
    zp = ops.p16_from_f32(cu(zf))
    wl = cu(torch.randn(Cin, 3, generator=g))
    s1, t1 = cu(torch.rand(Cin, generator=g) + 0.5), cu(torch.randn(Cin, generator=g) * 0.2)
    W2 = cu(torch.randn(Cout, Cin, generator=g) * (1.0 / Cin ** 0.5))
    s2 = torch.rand(Cout, generator=g) + 0.5
    s2[::5] *= -1.0
    s2, t2 = cu(s2), cu(torch.randn(Cout, generator=g) * 0.3)
    prep = ops.knn_stage_prepare(coord, I, K, avg)
    return dict(prep=prep, zp=zp, wl=wl, s1=s1, t1=t1, wp=ops.pointmlp_h3p_pack(W2), s2=s2, t2=t2, B=B, M=M, K=K, Cin=Cin, Cout=Cout, Lm=Lm)


def _words(rs, n):
    """The first three words of the first n slots of a scope's range log, as unsigned."""
    w = rs.log.cpu().view(-1, 8)[:n, :3].tolist()
    return [[v & 0xFFFFFFFF for v in row] for row in w]


def _two_launches(c, relu1, relu2):
    """-> (planes, the three range words one slot would hold: word 1 = the pack's weight word, word 2 = the larger of h1's and the output
    planes' maxima, word 0 untouched)"""
    from sonet_hip import ops
    with ops.range_scope(torch.device(DEV)) as rs:
        h1 = ops.knn_stage_input(c["prep"], c["zp"], c["wl"], c["s1"], c["t1"], relu1)
        out = ops.pointmlp_h3p_gmax(h1, c["wp"], c["s2"], c["t2"], relu2, c["Cout"], c["K"], c["prep"]["G"], c["B"] * c["M"], out="p16", Lout=c["Lm"])
    (a0, a1, a2), (b0, b1, b2) = _words(rs, 2)
    assert a0 == 0 and a1 == 0 and b0 == 0
    return out, [0, b1, max(a2, b2)], rs.violations()


def _one_launch(c, relu1, relu2):
    from sonet_hip import ops
    with ops.range_scope(torch.device(DEV)) as rs:
        out = ops.knn_layer2_gmax(c["prep"], c["zp"], c["wl"], c["s1"], c["t1"], relu1, c["wp"], c["s2"], c["t2"], relu2, c["Cout"], c["Lm"])
    assert rs.names == ["pointmlph3p_knn_gmax%d_%dx%d_L%d" % (c["K"], c["Cin"], c["Cout"], c["B"] * c["M"] * c["K"])]
    return out, _words(rs, 1)[0], rs.violations()


# 19 blocks, the last one partial, MT 4 | KI > K, flat axis padded 192 -> 256, MT 1, one K stage only partly filled |
# M 128, G 16, 48 pad columns per block, three chunks | G 8, MT 3
SHAPES = [(4, 64, 9, 9, 512, 512, True, True, True), (3, 64, 9, 12, 64, 128, False, True, False),
          (2, 128, 5, 5, 48, 256, True, False, True), (1, 64, 16, 16, 32, 384, True, True, True)]


@pytest.mark.parametrize("B,M,K,KI,Cin,Cout,avg,relu1,relu2", SHAPES)
def test_one_launch_equals_two_launches_bit_for_bit(B, M, K, KI, Cin, Cout, avg, relu1, relu2):
    c = _case(B, M, K, KI, Cin, Cout, avg)
    ref, ref_words, ref_bad = _two_launches(c, relu1, relu2)
    got, got_words, got_bad = _one_launch(c, relu1, relu2)
    assert got.shape == ref.shape and got.data.numel() == ref.data.numel()
    assert torch.equal(got.data, ref.data)                           # the whole buffer: pad columns included
    assert got_words == ref_words and got_words[1] != 0 and got_words[2] != 0
    assert got_bad == [] and ref_bad == []


def test_nan_in_z_and_in_the_affine_give_the_same_planes():
    """A NaN in the z planes (written into the raw fp16 words: the split of an f32 NaN is a finite number) and a NaN shift of the second
    layer: the same planes and the same range words as the two launches."""
    c = _case(2, 64, 9, 9, 64, 128, True, seed=1)
    raw = c["zp"].data.view(torch.int16)
    # hi plane of chunk 1, half 0: column 5, element 2 <- fp16 NaN
    raw[((1 * 2 + 0) * 2 + 0) * c["Lm"] * 8 + 5 * 8 + 2] = 0x7E00
    for relu1, relu2 in ((True, True), (False, False)):
        ref, ref_words, _ = _two_launches(c, relu1, relu2)
        got, got_words, _ = _one_launch(c, relu1, relu2)
        assert torch.equal(got.data, ref.data) and got_words == ref_words
    assert got_words[2] > 0x44FFE000                                  # the NaN reached the log (its bits, less the factor 32, are beyond 2047)
    c["t2"][7] = float("nan")
    ref, ref_words, _ = _two_launches(c, True, False)
    got, got_words, _ = _one_launch(c, True, False)
    assert torch.equal(got.data, ref.data) and got_words == ref_words


def test_h1_beyond_the_range_gives_the_same_range_words():
    c = _case(2, 64, 9, 9, 64, 128, True, seed=2)
    c["s1"][40] = 1.0e5                                              # one channel of h1 leaves 2047
    ref, ref_words, ref_bad = _two_launches(c, True, True)
    got, got_words, got_bad = _one_launch(c, True, True)
    assert torch.equal(got.data, ref.data) and got_words == ref_words
    assert got_words[2] > 0x44FFE000                                 # bits of 2047
    assert ref_bad and got_bad and all("2047" in what for _, what in got_bad)


def _opt(B, N, som_k=9, som_k_type="avg", node_num=64):
    return Namespace(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024,
                     activation="relu", normalization="batch", dropout=0.7, node_num=node_num, k=3, som_k=som_k, som_k_type=som_k_type,
                     bn_momentum=0.1, bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=40)


def _encoder(B, N, som_k=9, ktype="avg", seed=21, inp_seed=4):
    from models import networks as NW
    from sonet_hip import synth
    opt = _opt(B, N, som_k, ktype)
    enc = NW.Encoder(opt)
    sd = synth.fill_state_dict_(enc.state_dict(), seed)
    cpu_sd = {k: v.clone() for k, v in sd.items()}
    enc.to(DEV).eval()
    inp = synth.make_inputs(B, N, seed=inp_seed)
    args = [inp[k].to(DEV) for k in ("pc", "sn", "node", "node_knn_I")]
    return enc, cpu_sd, inp, args, opt


def _names(enc, args):
    from sonet_hip import ops
    with torch.no_grad(), ops.kernel_timing() as rec:
        f = enc(*args).clone()
    torch.cuda.synchronize()
    return f, [n for n, _, _ in rec.records]


def test_encoder_range_guard_recomputes_with_the_one_launch_route():
    """test_encoder_node_stage_range_guard_recomputes with the route on: the guarded forward recomputes in x3."""
    from sonet_hip import ops
    assert ops.KNN_FUSED_LAYER2
    enc, _, _, _, _ = _encoder(2, 512, seed=5, inp_seed=2)
    sd = enc.state_dict()
    sd["first_pointnet.layers.3.conv.bias"][11] = 6000.0            # pooled channel 11 ~ 6000 > 2047
    enc.load_state_dict(sd)
    from sonet_hip import synth
    inp = synth.make_inputs(2, 512, seed=2)
    args = [inp[k].to(DEV) for k in ("pc", "sn", "node", "node_knn_I")]
    ops._range_warned = False
    with torch.no_grad(), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        f = enc(*args).clone()
    assert any("range" in str(x.message) for x in w)
    with torch.no_grad(), ops.precision("x3"):
        f_x3 = enc(*args).clone()
    assert torch.equal(f, f_x3)


@pytest.mark.parametrize("B,N,som_k,ktype", [(2, 512, 9, "avg"), (3, 700, 9, "avg"), (1, 300, 5, "center")])
def test_encoder_route_on_equals_route_off_and_the_oracle(B, N, som_k, ktype):
    from oracle import cpu_oracle as O
    from sonet_hip import ops
    enc, cpu_sd, inp, args, opt = _encoder(B, N, som_k, ktype)
    assert ops.KNN_FUSED_LAYER2
    f_on, names_on = _names(enc, args)
    knn_on = enc.knn_feature_1.clone()
    assert enc.__dict__["_stage"]["knn_p16"] is not None
    assert sum(n.startswith("pointmlph3p_knn_gmax") for n in names_on) == 1 and not any(n.startswith("knn_stage_input") for n in names_on)
    ops.KNN_FUSED_LAYER2 = False
    try:
        f_off, names_off = _names(enc, args)
        knn_off = enc.knn_feature_1.clone()
    finally:
        ops.KNN_FUSED_LAYER2 = True
    assert sum(n.startswith("knn_stage_input") for n in names_off) == 1 and not any(n.startswith("pointmlph3p_knn_gmax") for n in names_off)
    assert torch.equal(f_on, f_off) and torch.equal(knn_on, knn_off)
    ref = O.encoder_forward(cpu_sd, inp["pc"], inp["sn"], inp["node"], inp["node_knn_I"], k=opt.k, som_k=som_k, som_k_type=ktype)
    assert_close_rms(f_on.cpu().numpy(), ref["feature"].numpy(), 1e-5, "feature vs oracle")


def test_graph_replays_equal_the_eager_forward():
    from sonet_hip import ops
    from sonet_hip.graph import GraphedForward
    assert ops.KNN_FUSED_LAYER2
    enc, _, _, args, _ = _encoder(2, 512)
    with torch.no_grad():
        eager = enc(*args).clone()
    fwd = GraphedForward(lambda pc, sn, node, knn: enc(pc, sn, node, knn), tuple(t.clone() for t in args))
    assert sum(n.startswith("pointmlph3p_knn_gmax") for n in fwd.range.names) == 1
    for _ in range(3):
        out = fwd(*args)
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert fwd.range_violations() == []


def test_unsupported_shape_is_refused_before_the_launch_and_the_encoder_falls_back():
    from sonet_hip import _lib, ops
    from sonet_hip._lib import ptr, stream_ptr
    c = _case(2, 64, 9, 9, 64, 96, True)
    assert not ops.knn_layer2_supported(64, 96, 9)
    yp = ops.p16_flat(96, c["Lm"], c["B"] * c["M"], torch.device(DEV))
    yp.data.fill_(0x5A)
    lib = _lib.load()
    with ops.range_scope(torch.device(DEV)) as rs:
        ops._range_arm("refused")
        rc = lib.sonet_knn_layer2_gmax_p16(ptr(c["prep"]["rec"]), ptr(c["zp"].data), ptr(c["wl"]), ptr(c["s1"]), ptr(c["t1"]), 1, c["B"], c["M"], c["K"], 64,
                                           ptr(c["wp"]), ptr(c["s2"]), ptr(c["t2"]), 1, 96, c["K"], c["prep"]["G"], c["B"] * c["M"], c["Lm"],
                                           ptr(yp.data), stream_ptr())
    torch.cuda.synchronize()
    assert rc == SONET_ERR_UNSUPPORTED and "Cout=96" in _lib.last_error()
    assert bool((yp.data == 0x5A).all()) and _words(rs, 1)[0] == [0, 0, 0]           # nothing ran
    # the encoder, told that its 512 -> 512 layer is not supported: the two launches, the same feature
    enc, _, _, args, _ = _encoder(2, 512)
    f_on, names_on = _names(enc, args)
    assert any(n.startswith("pointmlph3p_knn_gmax") for n in names_on)
    old = ops.KNN_LAYER2_MAX_C
    ops.KNN_LAYER2_MAX_C = 256
    try:
        f_fb, names_fb = _names(enc, args)
    finally:
        ops.KNN_LAYER2_MAX_C = old
    assert any(n.startswith("knn_stage_input") for n in names_fb) and not any(n.startswith("pointmlph3p_knn_gmax") for n in names_fb)
    assert torch.equal(f_on, f_fb)
