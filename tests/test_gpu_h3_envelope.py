"""The fp16-split ("h3") kernels on the corner families of the region their operand-range guard admits (tests/h3_model.py).

The contract (docs/findings.md 7a, ops.h3_weight_ok): whatever the guard admits meets float64 at 1e-5 in the suite's metric
|err| <= 1e-5 max(|ref|, rms(ref)); everything else runs in, or is packed for, x3.  Every other accuracy test feeds operands from the
middle of the region; these walk its corners.  The affine of a case rescales the layer's output to rms ~1, as the BatchNorm that follows
every shipped layer does (so that P16 outputs, which have an operand range of their own, are compared inside it).
Each test prints kernel error / model error per family: how much of the 1e-5 the f32 accumulation uses on top of the arithmetic."""
import warnings

import numpy as np
import pytest
import torch

import h3_model as H
from conftest import assert_close_rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-5


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _err(got, ref):
    rms = ref.pow(2).mean().sqrt()
    return float(((got.double() - ref).abs() / torch.maximum(ref.abs(), rms)).max())


class _Case:
    """One corner on the device: operands, the float64 product, and an affine that brings the output to rms ~1."""

    def __init__(self, name, x, W, n, flavour):
        self.name, self.fam, self.flavour = name, H.family_of(name), flavour
        self.host = (x, W)
        self.x, self.W = cu(x), cu(W)
        self.y64 = self.W.double() @ self.x.double()
        g = torch.Generator().manual_seed(n)
        rms = float(self.y64.pow(2).mean().sqrt())
        self.scale = ((0.5 + torch.rand(H.COUT, generator=g)) / rms).to(DEV)
        self.shift = (0.3 * torch.randn(H.COUT, generator=g)).to(DEV)
        self.relu = bool(n & 1)

    def ref(self, affine=True, relu=None):
        if not affine:
            return self.y64
        r = self.y64 * self.scale.double().view(-1, 1) + self.shift.double().view(-1, 1)
        return torch.relu(r) if (self.relu if relu is None else relu) else r


def _cases(K, flavour):
    for n, (name, x, W) in enumerate(H.corner_cases(K, flavour)):
        assert H.admitted(x, W, flavour), name
        yield n, _Case(name, x, W, n, flavour)


def _report(tag, worst):
    """Per family: the kernel's worst case, and the model's error (tests/h3_model.py, on the host) on that same case."""
    for fam, (e, c) in sorted(worst.items()):
        m, name = H.rms_error(H.model(*c.host, c.flavour), H.exact(*c.host)), c.name
        print("envelope %s %-18s kernel %.3g  model %.3g  kernel/model %.2f  (%s)" % (tag, fam, e, m, e / max(m, 1e-12), name))


def _note(worst, c, e):
    if e > worst.get(c.fam, (-1.0,))[0]:
        worst[c.fam] = (e, c)


@pytest.mark.parametrize("K", H.KS)
def test_second_generation_layer_on_every_admitted_corner(K):
    """ops.pointmlp with an "h3" pack: one panel, and two (384 + 3) at K = 387; plain (identity affine, no ReLU) and with affine (+ ReLU on
    every other case)."""
    from sonet_hip import ops
    one, zero = ops.const_vec(H.COUT, 1.0, DEV), ops.const_vec(H.COUT, 0.0, DEV)
    C1 = 384 if K == 387 else K
    worst = {}
    for n, c in _cases(K, "h3"):
        wp = ops.pointmlp_pack(c.W, "h3")
        x1 = c.x[:C1].unsqueeze(0).contiguous()
        x2 = c.x[C1:].unsqueeze(0).contiguous() if C1 < K else None
        with ops.range_scope(DEV) as rs:
            y0 = ops.pointmlp(x1, wp, one, zero, False, H.COUT, x2=x2)
            y1 = ops.pointmlp(x1, wp, c.scale, c.shift, c.relu, H.COUT, x2=x2)
        assert rs.violations() == [], c.name
        _note(worst, c, _err(y0[0], c.y64))
        assert_close_rms(y0[0].cpu().numpy(), c.ref(False).cpu().numpy(), TOL, "h3 layer, plain, " + c.name)
        assert_close_rms(y1[0].cpu().numpy(), c.ref().cpu().numpy(), TOL, "h3 layer, affine, " + c.name)
    _report("pointmlp/h3 K=%d" % K, worst)


@pytest.mark.parametrize("K", H.KS)
def test_third_generation_layer_on_every_admitted_corner(K):
    """ops.pointmlp_h3p on P16 planes made by ops.p16_from_f32, in its three output modes; the group-max epilogue at K' = 9."""
    from sonet_hip import ops
    C1 = 384 if K == 387 else K
    GK, G = 9, 14
    nblk = H.L // 128
    Lout = (nblk * G + 127) // 128 * 128                          # (K' = 9 leaves through P16 planes: the f32 output wants K' % 4 == 0)
    worst = {}
    for n, c in _cases(K, "h3p"):
        wp = ops.pointmlp_h3p_pack(c.W)
        with ops.range_scope(DEV) as rs:
            x1 = ops.p16_from_f32(c.x[:C1].unsqueeze(0).contiguous())
            x2 = ops.p16_from_f32(c.x[C1:].unsqueeze(0).contiguous()) if C1 < K else None
            y = ops.pointmlp_h3p(x1, wp, c.scale, c.shift, c.relu, H.COUT, x2=x2, out="f32")
            yp = ops.pointmlp_h3p(x1, wp, c.scale, c.shift, c.relu, H.COUT, x2=x2, out="p16")
            yb, ybp = ops.pointmlp_h3p(x1, wp, c.scale, c.shift, c.relu, H.COUT, x2=x2, out="both")
            gm = ops.pointmlp_h3p_gmax(x1, wp, c.scale, c.shift, c.relu, H.COUT, GK, G, nblk * G, x2=x2, out="p16", Lout=Lout)
        assert rs.violations() == [], (c.name, rs.violations())
        ref = c.ref()
        _note(worst, c, _err(y[0], ref))
        refn = ref.cpu().numpy()
        assert_close_rms(y[0].cpu().numpy(), refn, TOL, "h3p f32, " + c.name)
        assert_close_rms(ops.p16_to_f32(yp)[0].cpu().numpy(), refn, TOL, "h3p p16, " + c.name)
        assert_close_rms(yb[0].cpu().numpy(), refn, TOL, "h3p both (f32), " + c.name)
        assert_close_rms(ops.p16_to_f32(ybp)[0].cpu().numpy(), refn, TOL, "h3p both (p16), " + c.name)
        gref = ref.view(H.COUT, nblk, 128)[:, :, :G * GK].reshape(H.COUT, nblk * G, GK).amax(dim=2)
        bound = TOL * np.maximum(np.abs(gref.cpu().numpy()), float(ref.pow(2).mean().sqrt()))       # the layer's bound, at the maxima
        got = ops.p16_to_f32(gm)[0][:, :nblk * G].double().cpu().numpy()
        assert (np.abs(got - gref.cpu().numpy()) <= bound).all(), "h3p gmax, " + c.name
    _report("pointmlp_h3p K=%d" % K, worst)


@pytest.mark.parametrize("K", [k for k in H.KS if k != 387] + [387])
def test_segment_pool_layer_on_one_family_per_K(K):
    """ops.pointmlp_h3_segpool (the layer + per-node arg-max on node-sorted columns) on the family with the largest model error, over its
    corners in max |x| and max |w|: the pooled value is the float64 layer's at the chosen column, and that column holds its node's maximum."""
    from sonet_hip import ops
    C1 = 384 if K == 387 else K
    M = 8
    ids = torch.sort(torch.arange(H.L, dtype=torch.int32) % M).values.view(1, H.L).contiguous().to(DEV)
    pos0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    seen = 0
    for n, c in _cases(K, "h3"):
        if c.fam != "f8-allbut1-rmax":
            continue
        seen += 1
        wp = ops.pointmlp_pack(c.W, "h3")
        x1 = c.x[:C1].unsqueeze(0).contiguous()
        x2 = c.x[C1:].unsqueeze(0).contiguous() if C1 < K else None
        assert ops.pointmlp_h3_segpool_ok(x1, x2, wp, H.COUT, M)
        with ops.range_scope(DEV) as rs:
            idx, val = ops.pointmlp_h3_segpool(x1, wp, c.scale, c.shift, False, H.COUT, ids, pos0, M, None, x2=x2)
        assert rs.violations() == [], c.name
        ref = c.ref(relu=False)
        rms = float(ref.pow(2).mean().sqrt())
        at = ref.gather(1, idx[0].long())
        print("envelope segpool K=%d %s kernel %.3g" % (K, c.name, float(((val[0].double() - at).abs() / at.abs().clamp_min(rms)).max())))
        assert bool(((val[0].double() - at).abs() <= TOL * at.abs().clamp_min(rms)).all()), c.name
        seg_max = ref.view(H.COUT, M, H.L // M).amax(dim=2)
        assert bool((at >= seg_max - 2 * TOL * seg_max.abs().clamp_min(rms)).all()), c.name
        assert bool((ids[0].long()[idx[0].long()] == torch.arange(M, device=DEV).view(1, M)).all()), c.name
    assert seen == 9


@pytest.mark.parametrize("K", H.KS)
def test_just_outside_cases_are_reported_and_the_layer_runs_them_in_x3(K):
    from models import layers as Lm
    from sonet_hip import ops
    for name, side, x, W in H.outside_cases(K, "h3"):
        lyr = Lm.EquivariantLayer(K, H.COUT, activation=None, normalization=None)
        with torch.no_grad():
            lyr.conv.weight.copy_(torch.from_numpy(W).view(H.COUT, K, 1))
            lyr.conv.bias.zero_()
        lyr.to(DEV).eval()
        xd = cu(x).unsqueeze(0).contiguous()
        ref = (cu(W).double() @ cu(x).double()).cpu().numpy()
        if side == "w":
            assert not ops.h3_weight_ok(lyr.conv.weight.reshape(H.COUT, K)), name
        else:
            assert ops.h3_weight_ok(lyr.conv.weight.reshape(H.COUT, K)), name
            with ops.range_scope(DEV) as rs:
                ops.pointmlp(xd, ops.pointmlp_pack(cu(W), "h3"), ops.const_vec(H.COUT, 1.0, DEV), ops.const_vec(H.COUT, 0.0, DEV), False, H.COUT)
            bad = rs.violations()
            assert len(bad) == 1 and "max |x|" in bad[0][1] and "below" in bad[0][1], (name, bad)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            with torch.no_grad(), ops.precision("h3"), ops.kernel_timing() as rec:
                y = ops.run_guarded(lambda: lyr(xd), DEV, True)
        names = [n for n, _, _ in rec.records]
        assert any(n.startswith("pointmlpx3") for n in names), (name, names)
        assert_close_rms(y[0].cpu().numpy(), ref, TOL, "guarded layer, " + name)
