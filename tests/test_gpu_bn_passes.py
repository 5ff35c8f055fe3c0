"""The BatchNorm / ReLU passes on every dispatch path against tests/bn_passes_ref.py (float64; pinned to float64 autograd of F.batch_norm by
tests/test_bn_passes_cpu.py, which also asserts what the bit-equality below rests on: no seeded float64 result near a rounding midpoint).

These kernels are the reference side of the suite's bit-identity tests (normalise-on-load, BatchNorm-backward-on-load, the statistics
epilogues, the BatchNorm rider of the training goldens); here they are the side under test.  The kernel a shape selects cannot be observed
from Python: it follows from the dispatch rules of csrc/bn_passes.hip, restated next to the shapes in bn_passes_ref.py (``Case.path``), and
tests/test_bn_passes_cpu.py holds every ``Case.path`` to the kernel the launch recorder names for that call.

Bounds (none measured): element-wise results bit-equal; sums within 1e-12 (scalar kernels: every term in f64) resp. (log2 N + 1) 2^-24
(16-byte kernels: one product rounding + a pairwise f32 sum of N = 4 / 8 values) of the sum of the terms' magnitudes; mean / var through
``stats_bounds``; coefficient kernels in f32 ulps as derived at each assertion."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_passes_ref as R
from conftest import assert_close_rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ID = lambda c: c.id


def put(arr, case):
    """Host array -> device tensor of the case's storage type; case.k > 0: a contiguous view k elements into a larger flat buffer."""
    t = torch.from_numpy(np.ascontiguousarray(arr, np.float32))
    if case.bf16:
        t = t.to(torch.bfloat16)                               # (the values are bf16 already: exact)
    if case.k == 0:
        out = t.to(DEV)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    out = buf[case.k:case.k + t.numel()].view(t.shape)
    out.copy_(t)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == case.k * t.element_size() and out.is_contiguous()
    return out


def vec(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def assert_bits(got, ref, bf16, what):
    """got (device tensor) holds exactly the restatement's values (f32 array; bf16: bf16 values widened); NaN matches NaN."""
    ref = np.ascontiguousarray(ref, np.float32)
    assert tuple(got.shape) == ref.shape, what
    g, e = bits(got), (R.bf16_bits(ref) if bf16 else ref.view(np.uint32))
    ok = (g == e) | (np.isnan(ref) & np.isnan(got.float().cpu().numpy()))
    assert ok.all(), "%s: %d / %d elements differ, first at %s" % (what, int((~ok).sum()), ok.size, tuple(np.argwhere(~ok)[0]))


def _coef(d, *names):
    return [vec(d[n]) for n in names]


# ------------------------------------------------------------------------------------------ element-wise passes
@pytest.mark.parametrize("case", R.ELEMENTWISE, ids=_ID)
def test_elementwise_passes_equal_the_float64_restatement_bit_for_bit(case):
    from sonet_hip import ops
    d = R.elementwise_inputs(case)
    raw, gy = put(d["raw"], case), put(d["gy"], case)
    sc, sh, a, b, c0 = _coef(d, "sc", "sh", "a", "b", "c0")
    for relu in (False, True):
        want = R.affine_act(d["raw"], d["sc"], d["sh"], relu, case.bf16)
        assert_bits(ops.channel_affine_act(raw, sc, sh, relu), want, case.bf16, "channel_affine_act relu=%d (%s)" % (relu, case.path))
        if not case.bf16:
            y = put(d["raw"], case)
            assert ops.channel_affine_act_(y, sc, sh, relu) is y
            assert_bits(y, want, False, "channel_affine_act_ relu=%d" % relu)
        assert_bits(ops.pointwise_bwd_apply(gy, raw, sc, sh, relu, a, b, c0),
                    R.bwd_apply(d["gy"], d["raw"], d["sc"], d["sh"], relu, d["a"], d["b"], d["c0"], case.bf16), case.bf16,
                    "pointwise_bwd_apply relu=%d (%s)" % (relu, case.path))
    assert_bits(raw, d["raw"], case.bf16, "raw is left alone")
    assert_bits(gy, d["gy"], case.bf16, "gy is left alone")


@pytest.mark.parametrize("case", R.MASK_EDGE, ids=_ID)
def test_relu_mask_agrees_between_forward_and_backward_at_its_edge(case):
    """Pre-activation +0, -0.0 and the nearest f32 below 0: the forward stores a zero, the backward passes drop the gradient; the nearest
    f32 above 0: neither.  (forward ``v < 0 ? 0 : v``, backward ``!(fma > 0)``.)"""
    from sonet_hip import ops
    d = R.mask_edge_inputs(case)
    raw, gy = put(d["raw"], case), put(d["gy"], case)
    sc, sh, a, b, c0 = _coef(d, "sc", "sh", "a", "b", "c0")
    y = ops.channel_affine_act(raw, sc, sh, True)
    g = ops.pointwise_bwd_apply(gy, raw, sc, sh, True, a, b, c0)
    assert_bits(y, R.affine_act(d["raw"], d["sc"], d["sh"], True, case.bf16), case.bf16, "forward")
    assert_bits(g, R.bwd_apply(d["gy"], d["raw"], d["sc"], d["sh"], True, d["a"], d["b"], d["c0"], case.bf16), case.bf16, "backward")
    yh, gh = y.float().cpu().numpy(), g.float().cpu().numpy()
    for (bi, c, l, masked) in d["planted"]:
        inner = np.float32(np.float64(d["b"][c]) * np.float64(d["raw"][bi, c, l]) + np.float64(d["c0"][c]))     # fma(a, 0, inner) = inner
        inner = R.round_bf16(np.float32([inner]))[0] if case.bf16 else inner
        if masked:
            assert yh[bi, c, l] == 0 and gh[bi, c, l] == inner, (bi, c, l)
        else:
            assert (yh[bi, c, l] == (0 if case.bf16 else np.float32(R.TINY))) and gh[bi, c, l] != inner, (bi, c, l)
    if not case.bf16:
        y2 = put(d["raw"], case)
        ops.channel_affine_act_(y2, sc, sh, True)
        assert_bits(y2, yh, False, "in place")
    # the statistics pass masks the same elements: a planted gradient of 0.75 is far outside the bound of a sum of ~1e-2 terms
    s1, s2 = ops.pointwise_bwd_stats(gy, raw, sc, sh, True)
    e1, e2, a1, a2 = R.bwd_sums(d["gy"], d["raw"], d["sc"], d["sh"], True)
    tol = R.stats_tol(case, "bwd")
    assert (np.abs(s1.cpu().numpy() - e1) <= tol * a1).all() and (np.abs(s2.cpu().numpy() - e2) <= tol * a2).all()


@pytest.mark.parametrize("case", R.MASK_EDGE, ids=_ID)
def test_one_nan_stays_where_it_is(case):
    """A NaN in raw: the forward stores NaN there; the backward treats its mask as 0 (s1 leaves its gradient out; b * NaN makes g_raw and
    the channel's s2 NaN, with or without ReLU); no other element and no other channel changes."""
    from sonet_hip import ops
    d = R.nan_inputs(case)
    bi, c, l = d["at"]
    raw, gy = put(d["raw"], case), put(d["gy"], case)
    sc, sh, a, b, c0 = _coef(d, "sc", "sh", "a", "b", "c0")
    tol = R.stats_tol(case, "bwd")
    for relu in (False, True):
        y = ops.channel_affine_act(raw, sc, sh, relu)
        g = ops.pointwise_bwd_apply(gy, raw, sc, sh, relu, a, b, c0)
        assert_bits(y, R.affine_act(d["raw"], d["sc"], d["sh"], relu, case.bf16), case.bf16, "forward")
        assert_bits(g, R.bwd_apply(d["gy"], d["raw"], d["sc"], d["sh"], relu, d["a"], d["b"], d["c0"], case.bf16), case.bf16, "backward")
        assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[bi, c, l])) and int(torch.isnan(g).sum()) == 1 and bool(torch.isnan(g[bi, c, l]))
        s1, s2 = (t.cpu().numpy() for t in ops.pointwise_bwd_stats(gy, raw, sc, sh, relu))
        e1, e2, a1, a2 = R.bwd_sums(d["gy"], d["raw"], d["sc"], d["sh"], relu)
        assert np.isnan(e2[c]) and np.isnan(s2[c]) and np.isfinite(np.delete(s2, c)).all()
        assert (np.abs(np.delete(s2 - e2, c)) <= tol * np.delete(a2, c)).all()
        assert (np.abs(s1 - e1) <= tol * a1).all()          # (relu: gy at the NaN is not in e1; its 1e-2 is far outside the bound)


# ------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("case", R.STATS, ids=_ID)
def test_backward_sums_within_the_bound_of_their_arithmetic(case):
    from sonet_hip import ops
    d = R.stats_inputs(case)
    raw, gy = put(d["raw"], case), put(d["gy"], case)
    sc, sh = _coef(d, "sc", "sh")
    tol = R.stats_tol(case, "bwd")
    for relu in (False, True):
        sums = ops.pointwise_bwd_stats(gy, raw, sc, sh, relu, want_sums=True)
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (2 * case.C,)
        s = sums.cpu().numpy()
        e1, e2, a1, a2 = R.bwd_sums(d["gy"], d["raw"], d["sc"], d["sh"], relu)
        r1, r2 = np.abs(s[:case.C] - e1) / np.maximum(tol * a1, 1e-300), np.abs(s[case.C:] - e2) / np.maximum(tol * a2, 1e-300)
        print("bwd_stats %s relu=%d (%s): worst error / bound s1 %.3g s2 %.3g" % (case.id, relu, case.path, r1.max(), r2.max()))
        assert (np.abs(s[:case.C] - e1) <= tol * a1).all(), "s1 (%s): %.3g x bound" % (case.path, r1.max())
        assert (np.abs(s[case.C:] - e2) <= tol * a2).all(), "s2 (%s): %.3g x bound" % (case.path, r2.max())


@pytest.mark.parametrize("case", R.STATS, ids=_ID)
def test_channel_stats_within_the_bound_of_its_arithmetic(case):
    """Channel 0 has its mean at 1000 sigma (f32) / 8 sigma (bf16), the last channel is constant: the derived bound holds there too, and
    the variance is never negative or NaN."""
    from sonet_hip import ops
    d = R.stats_inputs(case)
    mean, var = (t.cpu().numpy().astype(np.float64) for t in ops.channel_stats(put(d["y"], case)))
    n = case.B * case.L
    s, s2, sabs = R.channel_stats(d["y"])
    em, ev = R.mean_var(s, s2, n)
    bm, bv = R.stats_bounds(s, s2, sabs, n, R.stats_tol(case, "channel"))
    print("channel_stats %s (%s): worst error / bound mean %.3g var %.3g" % (case.id, case.path, (np.abs(mean - em) / bm).max(),
                                                                              (np.abs(var - ev) / np.maximum(bv, 1e-300)).max()))
    assert np.isfinite(var).all() and (var >= 0).all()
    assert (np.abs(mean - em) <= bm).all(), (np.abs(mean - em) / bm).max()
    assert (np.abs(var - ev) <= bv).all(), (np.abs(var - ev) / np.maximum(bv, 1e-300)).max()


@pytest.mark.parametrize("case", R.CONSTANT, ids=_ID)
def test_constant_channel_has_zero_variance(case):
    """(power-of-two counts: every step of the kernels' arithmetic is exact there -- bn_passes_ref.CONSTANT)"""
    from sonet_hip import ops
    d = R.stats_inputs(case)
    mean, var = (t.cpu().numpy() for t in ops.channel_stats(put(d["y"], case)))
    assert mean[-1] == np.float32(-3.25) and var[-1] == 0 and not np.signbit(var[-1])


# ------------------------------------------------------------------------------------------ per-channel coefficient kernels
def _ulps(got, ref):
    return np.abs(got.astype(np.float64) - ref) / R.ulp32(ref)


@pytest.mark.parametrize("C", R.COEFF_C)
def test_bn_fwd_coeffs_vs_float64(C):
    from sonet_hip import ops
    d = R.coeff_inputs(C)
    invstd, scale, shift = (t.cpu().numpy() for t in ops.bn_fwd_coeffs(*_coef(d, "mean", "var", "gamma", "beta"), R.EPS))
    e_is, e_sc, e_sh = R.fwd_coeffs(d["mean"], d["var"], d["gamma"], d["beta"], float(np.float32(R.EPS)))      # (eps crosses the C ABI as a float)
    # add, sqrt, divide, multiply, each correctly rounded: 1/2 + 1/4 + 1/2 (+ 1/2) half-ulp units of relative error, an ulp being 1 to 2 of them
    print("bn_fwd_coeffs C=%d: worst ulps invstd %.3g scale %.3g" % (C, _ulps(invstd, e_is).max(), _ulps(scale, e_sc).max()))
    assert (_ulps(invstd, e_is) <= 4).all() and (_ulps(scale, e_sc) <= 4).all()
    assert (np.abs(shift - e_sh) <= 4 * R.U24 * (np.abs(d["beta"]) + np.abs(d["mean"] * e_sc))).all()
    if C > 1:
        assert abs(float(invstd[0]) - float(np.float32(R.EPS)) ** -0.5) <= 4 * R.ulp32(R.EPS ** -0.5)


@pytest.mark.parametrize("C", R.COEFF_C)
def test_bn_bwd_coeffs_vs_float64(C):
    from sonet_hip import ops
    d = R.coeff_inputs(C)
    invstd = R.to_f32(R.fwd_coeffs(d["mean"], d["var"], d["gamma"], d["beta"], R.EPS)[0])
    sums = vec(np.concatenate([d["s1"], d["s2"]]), torch.float64)
    got = [t.cpu().numpy() for t in ops.bn_bwd_coeffs(sums, vec(d["mean"]), vec(invstd), vec(d["gamma"]), d["n"])]
    a, b, c0, gg, gb = R.bwd_coeffs(d["s1"], d["s2"], d["mean"], invstd, d["gamma"], d["n"])
    # the kernel works in f64 and rounds once: half an ulp, and the f64 evaluation's own error (<< an f32 ulp at these magnitudes)
    for name, g, e in (("a", got[0], a), ("b", got[1], b), ("g_gamma", got[3], gg), ("g_beta", got[4], gb)):
        assert (_ulps(g, e) <= 1).all(), (name, _ulps(g, e).max())
    assert (np.abs(got[2] - c0) <= R.U24 * (np.abs(a * d["s1"] / d["n"]) + np.abs(b * d["mean"]))).all()


@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("C", R.COEFF_C)
def test_bn_running_update_vs_float64_and_batch_norm(C, momentum):
    from sonet_hip import ops
    d = R.running_inputs(C, momentum)
    rm, rv = vec(d["rmean"]), vec(d["rvar"])
    v0 = rm._version, rv._version
    ops.bn_running_update_(rm, rv, vec(d["mean"]), vec(d["var"]), d["momentum"], d["unbias"])
    assert rm._version > v0[0] and rv._version > v0[1]
    e_m, e_v = R.running_update_f32(d["rmean"], d["rvar"], d["mean"], d["var"], d["momentum"], d["unbias"])
    assert_bits(rm, e_m, False, "running_mean")
    assert_bits(rv, e_v, False, "running_var")
    bm, bv = torch.from_numpy(d["rmean"].astype(np.float64)), torch.from_numpy(d["rvar"].astype(np.float64))
    F.batch_norm(torch.from_numpy(d["x"]), bm, bv, None, None, True, d["momentum"], R.EPS)
    # (3 ulps: derived in test_bn_passes_cpu.test_running_update_is_what_batch_norm_does_to_float64_buffers)
    assert (_ulps(rm.cpu().numpy(), bm.numpy()) <= 3).all() and (_ulps(rv.cpu().numpy(), bv.numpy()) <= 3).all()


# ------------------------------------------------------------------------------------------ the rider
RIDER = [R.Case("f32", 3, 5, 1030, 0, "scalar, one chunk", 21), R.Case("bf16", 3, 5, 1030, 0, "pair, one chunk", 21),
         R.Case("bf16", 3, 257, 8, 0, "vec; C past one finalize block", 21)]


def _rider_setup(case, running):
    d = R.stats_inputs(case)
    g = case.rng(9)
    f = lambda v: vec(np.asarray(v, np.float32))
    gamma, beta = f(g.random(case.C) + 0.5), f(g.standard_normal(case.C) * 0.3)
    rm, rv = (f(g.standard_normal(case.C)), f(g.random(case.C) + 0.5)) if running else (None, None)
    n = case.B * case.L
    return put(d["y"], case), gamma, beta, rm, rv, float(np.float32(0.1)), n / (n - 1.0)


@pytest.mark.parametrize("running", [False, True])
@pytest.mark.parametrize("case", RIDER, ids=_ID)
def test_rider_equals_the_three_launches_it_replaces_bit_for_bit(case, running):
    from sonet_hip import ops
    y, gamma, beta, rm, rv, mom, unb = _rider_setup(case, running)
    rm0, rv0 = (rm.clone(), rv.clone()) if running else (None, None)
    ver = (rm._version, rv._version) if running else None
    invstd, sc, sh = ops.bn_rider(gamma, beta, R.EPS, rm, rv, mom, unb)
    if running:
        assert rm._version > ver[0] and rv._version > ver[1]
    mean, var = ops.channel_stats(y)
    i2, s2, h2 = ops.bn_fwd_coeffs(mean, var, gamma, beta, R.EPS)
    for name, got, want in (("invstd", invstd, i2), ("scale", sc, s2), ("shift", sh, h2)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
    if running:
        ops.bn_running_update_(rm0, rv0, mean, var, mom, unb)
        assert torch.equal(rm.view(torch.int32), rm0.view(torch.int32)) and torch.equal(rv.view(torch.int32), rv0.view(torch.int32))
        assert not torch.equal(rm, _rider_setup(case, True)[3])
    # consumed once: a second statistics call (of other data) touches neither the rider's outputs nor the running buffers, and returns
    # what a call without any rider returns
    snap = [t.clone() for t in (invstd, sc, sh) + ((rm, rv) if running else ())]
    m2, v2 = ops.channel_stats((y.float() * 2 + 1).to(y.dtype))
    for t, s in zip((invstd, sc, sh) + ((rm, rv) if running else ()), snap):
        assert torch.equal(t.view(torch.int32), s.view(torch.int32))
    assert not torch.equal(m2, mean)
    m3, v3 = ops.channel_stats(y)
    if "one chunk" in case.path:                               # (one workgroup per channel: the f64 sum has one order)
        assert torch.equal(m3, mean) and torch.equal(v3, var)


@pytest.mark.parametrize("case", RIDER[:2], ids=_ID)
def test_rider_does_not_outlive_a_rejected_statistics_call(case):
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    y, gamma, beta, rm, rv, mom, unb = _rider_setup(case, True)
    rm0, rv0 = rm.clone(), rv.clone()
    outs = ops.bn_rider(gamma, beta, R.EPS, rm, rv, mom, unb)
    for t in outs:
        t.fill_(-7.0)
    with pytest.raises(SonetHipError):
        ops.channel_stats(y.double())                          # rejected before any launch
    mean, var = ops.channel_stats(y)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs) and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    m2, v2 = ops.channel_stats(y)
    assert torch.equal(mean, m2) and torch.equal(var, v2)


# ------------------------------------------------------------------------------------------ the composed backward
def _autograd64(raw, gy, gamma, beta, relu):
    r = torch.from_numpy(raw.astype(np.float64)).requires_grad_(True)
    g, b = (torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (gamma, beta))
    act = F.batch_norm(r, None, None, g, b, True, 0.1, R.EPS)
    act = torch.relu(act) if relu else act
    return [t.numpy() for t in torch.autograd.grad(act, (r, g, b), torch.from_numpy(gy.astype(np.float64)))]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.COMPOSED, ids=_ID)
def test_composed_backward_vs_float64_autograd(case, relu):
    """channel_stats -> bn_fwd_coeffs -> pointwise_bwd_stats -> bn_bwd_coeffs -> pointwise_bwd_apply = backward of act(batch_norm(raw))."""
    from sonet_hip import ops
    d = R.composed_inputs(case)
    raw, gy, gamma, beta = put(d["raw"], case), put(d["gy"], case), vec(d["gamma"]), vec(d["beta"])
    mean, var = ops.channel_stats(raw)
    invstd, sc, sh = ops.bn_fwd_coeffs(mean, var, gamma, beta, R.EPS)
    sums = ops.pointwise_bwd_stats(gy, raw, sc, sh, relu, want_sums=True)
    a, b, c0, g_gamma, g_beta = ops.bn_bwd_coeffs(sums, mean, invstd, gamma, float(case.B * case.L))
    g_raw = ops.pointwise_bwd_apply(gy, raw, sc, sh, relu, a, b, c0).float().cpu().numpy().astype(np.float64)
    ref_raw, ref_gamma, ref_beta = _autograd64(d["raw"], d["gy"], d["gamma"], d["beta"], relu)
    if case.bf16:
        # every element within one bf16 ulp of the float64 value; rel-rms at the rounding-noise bound of tests/test_gpu_bf16_forced_routing.py
        worst = (np.abs(g_raw - ref_raw) / R.ulp_bf16(ref_raw)).max()
        rel_rms = np.sqrt(np.mean((g_raw - ref_raw) ** 2) / np.mean(ref_raw ** 2))
        print("composed %s relu=%d: worst %.3g bf16 ulps, rel-rms %.3g" % (case.id, relu, worst, rel_rms))
        assert worst <= 1 and rel_rms <= 2.2e-3
    else:
        assert_close_rms(g_raw, ref_raw, 1e-6, "g_raw")
        assert_close_rms(g_gamma.cpu().numpy(), ref_gamma, 1e-6, "g_gamma")
        assert_close_rms(g_beta.cpu().numpy(), ref_beta, 1e-6, "g_beta")


@pytest.mark.parametrize("case", [R.COMPOSED[1]], ids=_ID)
def test_affine_mode_backward_vs_float64(case):
    """The 'affine' mode of models.layers._PointwiseFn.backward: y = relu(z * scale + shift) was stored by the forward; the mask is taken
    from y itself with unit scale and zero shift, g_z = scale * (gy * mask), g_bias = scale * s1."""
    from sonet_hip import ops
    d = R.composed_inputs(case)
    g = case.rng(4)
    scale, shift = np.float32((g.random(case.C) + 0.5) * g.choice([-1.0, 1.0], case.C)), np.float32(g.standard_normal(case.C) * 0.4)
    z, gy, sc = put(d["raw"], case), put(d["gy"], case), vec(scale)
    y = ops.channel_affine_act(z, sc, vec(shift), True)
    ones, zeros = ops.const_vec(case.C, 1.0, DEV), ops.const_vec(case.C, 0.0, DEV)
    s1, _ = ops.pointwise_bwd_stats(gy, y, ones, zeros, True)
    g_bias = (sc.double() * s1).float()
    g_z = ops.pointwise_bwd_apply(gy, y, ones, zeros, True, sc, zeros, zeros)
    live = R.pre64(d["raw"], scale, shift) > 0
    ref = np.where(live, d["gy"].astype(np.float64), 0.0) * scale.astype(np.float64).reshape(1, -1, 1)
    assert_close_rms(g_z.cpu().numpy(), ref, 1e-6, "g_z")
    assert_close_rms(g_bias.cpu().numpy(), ref.sum(axis=(0, 2)), 1e-6, "g_bias")
    assert 0.2 < live.mean() < 0.8


# ------------------------------------------------------------------------------------------ argument checks
def test_bad_operands_are_rejected_before_a_launch():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    B, C, L = 2, 5, 8
    x = torch.randn(B, C, L, device=DEV)
    good = torch.ones(C, device=DEV)
    sums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)

    def rejected(fn, *args):
        with pytest.raises(SonetHipError):
            fn(*args)

    # storage types: float32 or bfloat16, nothing else is read as bf16 bits; raw matches gy
    for bad in (x.half(), x.double()):
        rejected(ops.channel_affine_act, bad, good, good, True)
        rejected(ops.pointwise_bwd_stats, bad, bad, good, good, True)
        rejected(ops.pointwise_bwd_apply, bad, bad, good, good, True, good, good, good)
    rejected(ops.channel_affine_act_, x.bfloat16(), good, good, True)
    rejected(ops.pointwise_bwd_stats, x, x.bfloat16(), good, good, True)
    rejected(ops.pointwise_bwd_apply, x.bfloat16(), x, good, good, True, good, good, good)
    rejected(ops.pointwise_bwd_stats, x, x[:, :, :4].contiguous(), good, good, True)
    rejected(ops.pointwise_bwd_apply, x, x[:1], good, good, True, good, good, good)
    # per-channel vectors: contiguous float32 of exactly C elements on the tensor's device
    bads = (torch.ones(C - 1, device=DEV), torch.ones(C + 1, device=DEV), torch.ones(C, device=DEV, dtype=torch.float64),
            torch.ones(C, device=DEV, dtype=torch.bfloat16), torch.ones(2 * C, device=DEV)[::2], torch.ones(C))
    for bad in bads:
        for i in range(2):
            v = [good, good]
            v[i] = bad
            rejected(ops.channel_affine_act, x, v[0], v[1], True)
            rejected(ops.channel_affine_act, x.bfloat16(), v[0], v[1], True)
            rejected(ops.channel_affine_act_, x.clone(), v[0], v[1], True)
            rejected(ops.pointwise_bwd_stats, x, x, v[0], v[1], True)
        for i in range(5):
            v = [good] * 5
            v[i] = bad
            rejected(ops.pointwise_bwd_apply, x, x, v[0], v[1], True, v[2], v[3], v[4])
        for i in range(4):                                     # (a short vector in the slot that sets C disagrees with the others)
            v = [good.clone(), good.clone(), good, good]
            v[i] = bad
            rejected(ops.bn_fwd_coeffs, v[0], v[1], v[2], v[3], R.EPS)
            rejected(ops.bn_running_update_, v[0], v[1], v[2], v[3], 0.1, 1.0)
        for i in range(3):
            v = [good] * 3
            v[i] = bad
            rejected(ops.bn_bwd_coeffs, sums, v[0], v[1], v[2], 16.0)
    rejected(ops.bn_fwd_coeffs, torch.ones(C + 1, device=DEV), good, good, good, R.EPS)
    rejected(ops.bn_bwd_coeffs, sums.float(), good, good, good, 16.0)
    rejected(ops.bn_bwd_coeffs, sums[:C].contiguous(), good, good, good, 16.0)
    rejected(ops.bn_bwd_coeffs, torch.zeros(2 * C + 2, dtype=torch.float64, device=DEV), good, good, good, 16.0)
    rejected(ops.bn_bwd_coeffs, torch.zeros(4 * C, dtype=torch.float64, device=DEV)[::2], good, good, good, 16.0)
    torch.cuda.synchronize()
    # ... and what is accepted still runs
    assert ops.channel_affine_act(x, good, torch.zeros(C, device=DEV), False).equal(x)
