"""tests/bn_passes_ref.py -- the float64 restatement tests/test_gpu_bn_passes.py holds the BatchNorm / ReLU kernels to -- against float64
autograd of F.batch_norm, and the properties of the seeded inputs the GPU tests rely on: no float64 result near a rounding midpoint (so
that a float64 emulation of an fma may be compared bit for bit), bf16 inputs that hold bf16 values, and sum bounds that a single dropped
element breaks at every shape.  And the one thing the GPU tests cannot see from Python -- which kernel a shape selects -- against the recorded
dispatch of the entry points (tests/golden/launch, held to the tree by tests/test_launch_log_cpu.py)."""
import lzma
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_passes_ref as R


def _rel_rms(got, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), np.sqrt(np.mean(ref ** 2)))).max())


def _autograd(raw, gy, gamma, beta, relu):
    r = torch.from_numpy(np.asarray(raw, np.float64)).requires_grad_(True)
    g, b = (torch.from_numpy(np.asarray(t, np.float64)).requires_grad_(True) for t in (gamma, beta))
    act = F.batch_norm(r, None, None, g, b, True, 0.1, R.EPS)
    act = torch.relu(act) if relu else act
    return [t.numpy() for t in torch.autograd.grad(act, (r, g, b), torch.from_numpy(np.asarray(gy, np.float64)))]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.COMPOSED, ids=lambda c: c.id)
def test_chained_restatement_is_float64_autograd_of_batch_norm(case, relu):
    d = R.composed_inputs(case)
    raw, gy, gamma, beta = d["raw"], d["gy"], d["gamma"], d["beta"]
    n = raw.shape[0] * raw.shape[2]
    s, s2, _ = R.channel_stats(raw)
    mean, var = R.mean_var(s, s2, n)
    invstd, sc, sh = R.fwd_coeffs(mean, var, gamma, beta, R.EPS)
    s1, s2b, _, _ = R.bwd_sums(gy, raw, sc, sh, relu)
    a, b, c0, g_gamma, g_beta = R.bwd_coeffs(s1, s2b, mean, invstd, gamma, float(n))
    g_raw = R.apply64(gy, raw, sc, sh, relu, a, b, c0, exact=True)[1]
    ref_raw, ref_gamma, ref_beta = _autograd(raw, gy, gamma, beta, relu)
    assert _rel_rms(g_raw, ref_raw) <= 1e-12
    assert _rel_rms(g_gamma, ref_gamma) <= 1e-12
    assert _rel_rms(g_beta, ref_beta) <= 1e-12
    # the forward of the same chain
    y = torch.from_numpy(np.asarray(raw, np.float64))
    y = F.batch_norm(y, None, None, torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), True, 0.1, R.EPS)
    pre = R.pre64(raw, sc, sh)
    assert _rel_rms(np.maximum(pre, 0.0) if relu else pre, (torch.relu(y) if relu else y).numpy()) <= 1e-12


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", R.COMPOSED, ids=lambda c: c.id)
def test_f32_chain_meets_the_bounds_the_gpu_test_sets(case, relu):
    """The restatement with the kernels' roundings (``chain``) against float64 autograd, at the bounds of the composed GPU test: the seeds are
    chosen here, on reference arithmetic, never on a kernel's output."""
    d = R.composed_inputs(case)
    g_raw, g_gamma, g_beta = R.chain(d["raw"], d["gy"], d["gamma"], d["beta"], relu, case.bf16)
    ref_raw, ref_gamma, ref_beta = _autograd(d["raw"], d["gy"], d["gamma"], d["beta"], relu)
    if case.bf16:
        assert (np.abs(g_raw.astype(np.float64) - ref_raw) <= R.ulp_bf16(ref_raw)).all()
        assert np.sqrt(np.mean((g_raw - ref_raw) ** 2) / np.mean(ref_raw ** 2)) <= 2.2e-3
    else:
        assert _rel_rms(g_raw, ref_raw) <= 1e-6
    assert _rel_rms(g_gamma, ref_gamma) <= 1e-6 and _rel_rms(g_beta, ref_beta) <= 1e-6


@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("C", R.COEFF_C)
def test_running_update_is_what_batch_norm_does_to_float64_buffers(C, momentum):
    d = R.running_inputs(C, momentum)
    rm, rv = torch.from_numpy(d["rmean"].astype(np.float64)), torch.from_numpy(d["rvar"].astype(np.float64))
    F.batch_norm(torch.from_numpy(d["x"]), rm, rv, None, None, True, d["momentum"], R.EPS)
    got_m, got_v = R.running_update(d["rmean"], d["rvar"], d["mean"], d["var"], d["momentum"], d["unbias"])
    np.testing.assert_allclose(got_m, rm.numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(got_v, rv.numpy(), rtol=1e-14, atol=0)
    # the f32 evaluation stays within 3 f32 ulps of it: (1 - m) and r (1 - m) round once each (2 x 2^-24 on a (1 - m) share), the unbias
    # factor and var * unbias once each (2 x 2^-24 on an m share), the fma once: at most 3 x 2^-24 relative, and 2^-24 |x| <= 1 ulp(x)
    f_m, f_v = R.running_update_f32(d["rmean"], d["rvar"], d["mean"], d["var"], d["momentum"], d["unbias"])
    assert (np.abs(f_m - got_m) <= 3 * R.ulp32(got_m)).all() and (np.abs(f_v - got_v) <= 3 * R.ulp32(got_v)).all()
    # and its own fma sums stay clear of the f32 midpoints
    assert sum(R.tie_count(t, False, ix) for t, ix in R.running_update_f32(d["rmean"], d["rvar"], d["mean"], d["var"], d["momentum"], d["unbias"], want64=True)) == 0


def _elementwise_ties(d, bf16):
    n = 0
    for relu in (False, True):
        pre, ix_p = R.pre64(d["raw"], d["sc"], d["sh"], want_inexact=True)
        inner, outer, ix_i, ix_o = R.apply64(d["gy"], d["raw"], d["sc"], d["sh"], relu, d["a"], d["b"], d["c0"], want_inexact=True)
        n += R.tie_count(pre, False, ix_p) + R.tie_count(inner, False, ix_i) + R.tie_count(outer, False, ix_o)
        if bf16:
            n += R.tie_count(pre, True, ix_p) + R.tie_count(outer, True, ix_o)
    return n


@pytest.mark.parametrize("case", R.ELEMENTWISE + R.MASK_EDGE, ids=lambda c: c.id)
def test_no_seeded_result_lies_near_a_rounding_midpoint(case):
    assert _elementwise_ties(R.elementwise_inputs(case), case.bf16) == 0
    if case in R.MASK_EDGE:
        assert _elementwise_ties(R.mask_edge_inputs(case), case.bf16) == 0
        assert _elementwise_ties(R.nan_inputs(case), case.bf16) == 0


def test_tie_count_sees_a_midpoint():
    one = np.float64(1.0)
    assert R.tie_count(np.array([one + 2.0 ** -24])) == 1 and R.tie_count(np.array([one + 2.0 ** -24 + 2.0 ** -52])) == 1
    assert R.tie_count(np.array([one + 2.0 ** -24 + 2.0 ** -45])) == 0 and R.tie_count(np.array([one, 0.0, 3.5])) == 0
    assert R.tie_count(np.array([one + 2.0 ** -8]), True) == 1 and R.tie_count(np.array([one + 2.0 ** -8 + 2.0 ** -30]), True) == 0
    assert R.tie_count(np.array([one + 2.0 ** -24]), True) == 0
    # an exactly computed sum is the fma's own exact value: not counted; a rounded one is
    s, ix = R.add64(np.array([one, one]), np.array([2.0 ** -24, 2.0 ** -24 + 2.0 ** -60]))
    assert list(ix) == [False, True] and R.tie_count(s, False, ix) == 1


def test_bf16_rounding_is_nearest_even_and_matches_torch():
    g = np.random.default_rng(1)
    x = np.concatenate([g.standard_normal(4096).astype(np.float32) * 3, np.float32([0.0, -0.0, 1.00390625, 1.01171875, R.TINY, np.inf])])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(R.bf16_bits(x), want)
    assert np.isnan(R.round_bf16(np.float32([np.nan]))).all()


def test_bf16_inputs_hold_bf16_values():
    seen = 0
    for cases, make in ((R.ELEMENTWISE, R.elementwise_inputs), (R.MASK_EDGE, R.mask_edge_inputs), (R.MASK_EDGE, R.nan_inputs),
                        (R.STATS + R.CONSTANT, R.stats_inputs), (R.COMPOSED, R.composed_inputs)):
        for case in cases:
            if case.bf16:
                d = make(case)
                for k in ("raw", "gy", "y"):
                    if k in d:
                        v = d[k][np.isfinite(d[k])]
                        assert d[k].dtype == np.float32 and R.holds_bf16(v) and np.abs(v).max() > 0, (case.id, k)
                        seen += 1
    assert seen > 60


@pytest.mark.parametrize("case", R.STATS, ids=lambda c: c.id)
def test_one_dropped_element_breaks_each_sum_bound(case):
    """Dropping (or doubling) one element moves a sum by that element's term.  At every shape and for every sum the GPU tests bound, the
    typical (median) live term and at least 90 % of all live terms are larger than the bound (the rest: values next to zero, whose squares and
    products add next to nothing): a kernel that loses one element fails it."""
    d = R.stats_inputs(case)
    n = case.B * case.L

    def check(terms, bound, what):                           # terms [B][C][L] float64, bound [C]
        for c in range(min(case.C, 8)):
            t = np.abs(terms[:, c, :].ravel())
            t = t[t > 0]
            if t.size == 0:
                continue
            assert np.median(t) > bound[c] and (t > bound[c]).mean() >= 0.90, (what, c, float(np.median(t)), float(bound[c]))

    for relu in (False, True):
        tol = R.stats_tol(case, "bwd")
        s1, s2, a1, a2 = R.bwd_sums(d["gy"], d["raw"], d["sc"], d["sh"], relu)
        g = np.where(R.mask(d["raw"], d["sc"], d["sh"], relu), d["gy"].astype(np.float64), 0.0)
        check(g, tol * a1, "s1")
        check(g * d["raw"], tol * a2, "s2")
    tol = R.stats_tol(case, "channel")
    s, s2, sabs = R.channel_stats(d["y"])
    y = d["y"].astype(np.float64)
    check(y, tol * sabs, "sum")
    check(y * y, tol * s2, "sum of squares")
    # ... and shows in what channel_stats returns: the mean moves by |x| / n, against its bound
    bm, bv = R.stats_bounds(s, s2, sabs, n, tol)
    if n > 1:
        for c in range(min(case.C, 8)):
            x = np.abs(y[:, c, :].ravel())
            m_drop = np.abs((s[c] - y[:, c, :].ravel()) / n - s[c] / n)
            assert np.median(m_drop) > bm[c] or np.median(x) == 0, (c, float(np.median(m_drop)), float(bm[c]))


def test_sum_bounds_are_the_derived_ones():
    assert R.SCALAR_TOL == 1e-12 and R.vector_tol(False) == 3 * 2.0 ** -24 and R.vector_tol(True) == 4 * 2.0 ** -24
    paths = {(c.dt, c.path.split(":")[0].split(",")[0].split(" ")[0]) for c in R.STATS}
    assert paths == {("f32", "vec"), ("f32", "scalar"), ("bf16", "vec"), ("bf16", "pair"), ("bf16", "scalar")}


def test_coefficient_inputs_cover_the_edges():
    for C in R.COEFF_C:
        d = R.coeff_inputs(C)
        assert d["var"].min() >= 0 and d["var"].max() > 1e7
        if C > 1:
            assert d["var"][0] == 0 and d["mean"][C // 2] * np.sqrt(d["var"][C // 2] + R.EPS) ** -1 > 1000
        invstd, scale, shift = R.fwd_coeffs(d["mean"], d["var"], d["gamma"], d["beta"], R.EPS)
        assert np.isfinite(invstd).all() and (C == 1 or abs(invstd[0] - R.EPS ** -0.5) < 1e-9)


# kernel (as the recording names it: a piece of the mangled name, template arguments included) -> flavour of ``Case.path``
FLAVOUR = [("stats_vec_kernel", "vec"), ("rowwise_vec_kernel", "vec"),
           ("bwd_stats_bf16_kernelILb1E", "pair"), ("rowwise_bf16_kernelILi0ELb1E", "pair"), ("rowwise_bf16_kernelILi1ELb1E", "pair"),
           ("bwd_stats_bf16_kernelILb0E", "scalar"), ("rowwise_bf16_kernelILi0ELb0E", "scalar"), ("rowwise_bf16_kernelILi1ELb0E", "scalar"),
           ("20channel_stats_kernel", "scalar"), ("16bwd_stats_kernel", "scalar"), ("16bwd_apply_kernel", "scalar"), ("21affine_act_out_kernel", "scalar")]
# the ops of tests/test_gpu_bn_passes.py that run each list (channel_affine_act_ is one flat kernel whatever the shape: no flavour)
RUNS = [(R.ELEMENTWISE, ("channel_affine_act_out", "pointwise_bwd_apply")),
        (R.MASK_EDGE, ("channel_affine_act_out", "pointwise_bwd_apply", "pointwise_bwd_stats")),
        (R.STATS, ("pointwise_bwd_stats", "channel_stats"))]


def test_every_case_takes_the_kernel_its_path_names():
    """``Case.path`` starts with the flavour (vec / pair / scalar) the dispatch rules give the shape; the launch recorder's line for the same
    call -- entry point, dtype, B, C, L, every operand k elements into its allocation -- must name a kernel of that flavour.  A Case the
    recorder's sweep does not hold fails, so the two cannot drift apart.  (channel_stats f32 has no 16-byte kernel: always scalar.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import launch_log
    with lzma.open(os.path.join(root, "tests", "golden", "launch", "product.txt.xz"), "rt") as f:
        text = f.read()
    recorded, group = {}, None                               # (group, case) -> the launches of the line
    for line in launch_log.expand(text[text.index("== bn passes: kernels and refusal texts"):]):
        if line.startswith("# "):
            group = line[2:]
        elif line.startswith("  ") and " | " in line:
            head, launches = line[2:].split(" | ")
            recorded[(group, head.rsplit(" ", 1)[0])] = launches.split()
    checked = 0
    for cases, ops in RUNS:
        for case in cases:
            for op in ops:
                key = ("sonet_%s_%s k=%d" % (op, case.dt, case.k), "%dx%dx%d" % (case.B, case.C, case.L))
                assert key in recorded, "the recorder's sweep (tools/launch_driver.cpp) does not hold %s %s" % key
                flavours = [fl for item in recorded[key] for piece, fl in FLAVOUR if piece in item]
                assert len(flavours) == 1, (key, recorded[key])
                want = re.split(r"[ ,:]", case.path)[0]
                if op == "channel_stats" and not case.bf16:
                    want = "scalar"
                assert flavours[0] == want, (key, case.path, recorded[key])
                checked += 1
    assert checked == 2 * len(R.ELEMENTWISE) + 3 * len(R.MASK_EDGE) + 2 * len(R.STATS)
