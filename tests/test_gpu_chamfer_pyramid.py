"""The Chamfer loss pyramid on the MI355X (sonet_chamfer_pyramid_loss_f32, sonet_chamfer_pyramid_grad_f32, ops.chamfer_pyramid_loss,
models.losses.AutoencoderLoss with opt.chamfer_pyramid): every output bit-equal to the single-level operator called once per level
(ops.chamfer_terms / ops.chamfer_grad), the indices and elements equal to the restatement, the gradient inside chamfer_ref.GATE of
float64 at the kernel's own indices, forged indices, dirty buffers, offset views, two runs and a graph replay, the extents, the
autograd operator and the module against the present path."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import assert_close_rms, golden
import chamfer_ref as R
import chamfer_pyramid_ref as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
AE_CASES = ("autoencoder_b2_n1024", "autoencoder_b2_n5000")
KEYS = ("nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "sums")
I32_MIN = -2 ** 31


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    """The bit pattern of a device tensor, as integers of its element size."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _same_f32(a, b):
    """Bit-equal, a NaN matching any NaN (chamfer_ref's elements against the device's)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def _clouds(kind, B, Ms, N, seed=0):
    """One gt cloud and a predicted cloud per level (two levels of equal size hold different points)."""
    gt = R.make(kind, B, max(Ms), N)[1]
    if kind == "lattice":
        return [R.make(kind, B, M, N)[0] for M in Ms], gt
    return [R.make(kind, B, M, N, seed=seed + 100 * l)[0] for l, M in enumerate(Ms)], gt


def _check_forward(preds, gt, what, restate=True):
    """The pyramid against one ops.chamfer_terms call per level (every output, bits of the sums included; equal indices and
    elements on a NaN too: the same kernel code) and against the restatement."""
    from sonet_hip import ops
    dps, dg = [_cu(p) for p in preds], _cu(gt)
    t = ops.chamfer_pyramid_terms(dps, dg)
    assert tuple(t.sums.shape) == (gt.shape[0], len(preds), 2) and t.sums.dtype == torch.float64 and t.N == gt.shape[2]
    for l, dp in enumerate(dps):
        one = ops.chamfer_terms(dp, dg)
        lv = t.levels[l]
        assert (lv.M, lv.N) == (one.M, one.N)
        for k in KEYS:
            assert _same(getattr(lv, k), getattr(one, k)), "%s level %d: %s differs from the single-level operator" % (what, l, k)
        if restate:
            ref = R.terms(preds[l], gt)
            assert np.array_equal(lv.nn_pg.cpu().numpy(), ref["nn_pg"]) and np.array_equal(lv.nn_gp.cpu().numpy(), ref["nn_gp"]), (what, l)
            assert _same_f32(lv.elem_fwd.cpu().numpy(), ref["elem_fwd"]) and _same_f32(lv.elem_bwd.cpu().numpy(), ref["elem_bwd"]), (what, l)
    return t, dps, dg


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("Ms,N", P.FWD_SHAPES)
def test_forward_is_the_single_level_operator_per_level(Ms, N):
    for B in (1, 3):
        for kind in ("lattice", "continuous"):
            _check_forward(*_clouds(kind, B, Ms, N), "%s B%d M%s N%d" % (kind, B, Ms, N))


def test_forward_at_the_autoencoder_size():
    preds, gt = _clouds("continuous", 2, (1280, 256), 5000)
    _check_forward(preds, gt, "B2 (1280, 256) x 5000")


def test_forward_with_outputs_absent():
    from sonet_hip import _lib, ops
    preds, gt = _clouds("continuous", 3, (257, 2, 300), 1025)
    full, dps, dg = _check_forward(preds, gt, "full", restate=False)
    for want_nn in (False, True):
        for want_elems in (False, True):
            t = ops.chamfer_pyramid_terms(dps, dg, want_nn=want_nn, want_elems=want_elems)
            assert _same(t.sums, full.sums)
            for lv, fl in zip(t.levels, full.levels):
                assert (lv.nn_pg is not None) == (lv.nn_gp is not None) == want_nn
                assert (lv.elem_fwd is not None) == (lv.elem_bwd is not None) == want_elems
                for k in KEYS[:4]:
                    assert getattr(lv, k) is None or _same(getattr(lv, k), getattr(fl, k)), k
    # through ctypes: a whole output array absent, and single entries of the arrays absent
    lib = _lib.load()
    B, L, Ms, N = 3, 3, [257, 2, 300], 1025
    import ctypes
    for mask in ((0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0)):
        for hole in (None, 1):
            outs = [[torch.full((B, M if k in (0, 2) else N), -7, dtype=torch.int32 if k < 2 else torch.float32, device=DEV) for M in Ms]
                    for k in range(4)]
            arrs = [None if not mask[k] else (ctypes.c_void_p * 3)(*[None if l == hole else o.data_ptr() for l, o in enumerate(outs[k])])
                    for k in range(4)]
            sums = torch.full((B, L, 2), -7.0, dtype=torch.float64, device=DEV)
            ws = torch.empty((lib.sonet_chamfer_pyramid_ws_size(B, L, *Ms, N),), dtype=torch.uint8, device=DEV)
            with torch.cuda.device(DEV):
                _lib.check(lib.sonet_chamfer_pyramid_loss_f32((ctypes.c_void_p * 3)(*[p.data_ptr() for p in dps]), _lib.ptr(dg), *arrs, _lib.ptr(sums),
                                                              _lib.ptr(ws), B, L, (ctypes.c_int * 3)(*Ms), N, _lib.stream_ptr()), "pyramid loss")
            assert _same(sums, full.sums), (mask, hole)
            for k in range(4):
                for l in range(L):
                    if mask[k] and l != hole:
                        assert _same(outs[k][l], getattr(full.levels[l], KEYS[k])), (mask, hole, k, l)
                    else:
                        assert (outs[k][l] == -7).all(), (mask, hole, k, l)          # an absent output is not written


def test_nan_and_overflowing_coordinates_as_the_single_level_operator():
    preds, gt = _clouds("continuous", 3, (300, 257), 1100)
    bad = [p.copy() for p in preds]
    bad[0][1, 1, 257] = np.nan
    bad[1][2, 0, 256] = np.nan
    t, _, _ = _check_forward(bad, gt, "NaN coordinate")
    s = t.sums.cpu().numpy()
    assert np.isnan(s[1, 0, 0]) and np.isnan(s[2, 1, 0]) and np.isnan(s).sum() == 2
    assert int(t.levels[0].nn_pg[1, 257]) == 0 and int(t.levels[1].nn_pg[2, 256]) == 0
    badg = gt.copy()
    badg[0, 2, 1024] = np.nan
    _check_forward(preds, badg, "NaN gt coordinate")
    far = [p.copy() for p in preds]
    far_g = gt.copy()
    far[0][0, 0, [0, 255, 256, 299]] = np.float32(3e19)
    far[1][2, 1, [1, 128]] = np.float32(-3e19)
    far_g[0, 0, [3, 1023, 1024]] = np.float32(3e19)
    far_g[1, 2, [5, 1099]] = np.float32(-3e19)
    t, _, _ = _check_forward(far, far_g, "overflow")
    assert np.isinf(t.sums.cpu().numpy()).any()


# ------------------------------------------------------------------------------------------------------------ gradient
def _check_grad(preds, gt, gscale, what, gate=True):
    """The pyramid's gradient against ops.chamfer_grad per level (bits) and against float64 at the kernel's indices (GATE)."""
    from sonet_hip import ops
    dps, dg = [_cu(p) for p in preds], _cu(gt)
    t = ops.chamfer_pyramid_terms(dps, dg)
    gs = torch.tensor(gscale, dtype=torch.float32, device=DEV)
    dpreds, bad = ops.chamfer_pyramid_grad(dps, dg, t, gs)
    assert bad.dtype == torch.int32 and tuple(bad.shape) == (len(preds),) and (bad == 0).all()
    for l, dp in enumerate(dps):
        one, bad1 = ops.chamfer_grad(dp, dg, t.levels[l], gs[l])
        assert int(bad1) == 0 and _same(dpreds[l], one), "%s level %d: differs from the single-level gradient" % (what, l)
        if gate:
            gf, gb = (float(v) for v in gs[l].cpu().numpy())
            ref64, mag = R.grad(preds[l], gt, t.levels[l].nn_pg.cpu().numpy(), t.levels[l].nn_gp.cpu().numpy(), gf, gb)
            got = dpreds[l].cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all() and (np.abs(got - ref64) <= R.GATE * mag).all(), "%s level %d: outside the float64 gate" % (what, l)
            assert (got[mag == 0] == 0).all()
    return t, dps, dg, gs, dpreds


SCALES = ([0.7, -1.3], [1.0, 1.0], [0.25, 3.0])


@pytest.mark.parametrize("Ms,N", P.GRAD_SHAPES)
def test_gradient_is_the_single_level_gradient_per_level(Ms, N):
    for B in (1, 3):
        for kind in ("lattice", "continuous"):
            preds, gt = _clouds(kind, B, Ms, N)
            _check_grad(preds, gt, SCALES[:len(Ms)], "%s B%d M%s N%d" % (kind, B, Ms, N))
    zero = [list(s) for s in SCALES[:len(Ms)]]
    zero[-1] = [0.0, 0.0]                                                        # a level nobody asked a gradient of: zeros
    *_, dpreds = _check_grad(preds, gt, zero, "zero gscale on the last level")
    assert (dpreds[-1] == 0).all()


def test_gradient_lists_one_owner_empty_lists_and_coincident_points():
    from sonet_hip import ops
    N = 1025
    gt = None
    preds = []
    for l, (M, owner) in enumerate(((300, 0), (7, 3), (257, 256))):              # the owner first, in the middle, last
        p, g = R.one_owner(2, M, N, 77, owner=owner)
        gt = g if gt is None else gt
        assert np.array_equal(g, gt)                                             # (the gt cloud depends on the seed and N alone)
        preds.append(p)
    t, *_ = _check_grad(preds, gt, SCALES, "one owner")
    for lv, owner in zip(t.levels, (0, 3, 256)):
        assert (lv.nn_gp == owner).all()                                         # one list of N entries, every other list empty
    p1, _ = R.one_owner(2, 1, N, 77, owner=0)                                    # a level of one point owns everything
    _check_grad([p1, preds[0]], gt, ([1.0, 1.0], [0.0, 1.0]), "M = 1")
    # a predicted point no gt point chooses keeps its forward term alone
    preds, gt = _clouds("continuous", 2, (257, 64), 300)
    preds[0][:, :, 100] = np.float32(5.0)
    t, _, _, _, dpreds = _check_grad(preds, gt, ([0.0, 1.0], [1.0, 1.0]), "unchosen point")
    assert not (t.levels[0].nn_gp == 100).any() and (dpreds[0][:, :, 100] == 0).all()
    # coincident points: elements at the 1e-4 floor, terms of exactly zero
    pa, gt = R.make("coincident", 2, 257, 600)
    pb = R.make("coincident", 2, 64, 600)[0]
    *_, dpreds = _check_grad([pa, pb], gt, ([1.0, 0.0], [0.7, -1.3]), "coincident")
    assert (dpreds[0][:, :, ::2] == 0).all() and (dpreds[0][:, :, 1::2] != 0).any()


def test_forged_indices_are_counted_and_never_addresses():
    from sonet_hip import ops
    Ms, N, B = (300, 64), 1100, 2
    preds, gt = _clouds("continuous", B, Ms, N)
    t, dps, dg, gs, clean = _check_grad(preds, gt, SCALES[:2], "clean")
    forged, counts, touched = [], [], []
    for l, M in enumerate(Ms):
        nn_pg, nn_gp = t.levels[l].nn_pg.cpu().numpy().copy(), t.levels[l].nn_gp.cpu().numpy().copy()
        forged_m = {(0, 0): -1, (0, M - 1): N, (1, 17): I32_MIN, (1, M - 2): 2 ** 31 - 1}
        forged_n = {(0, 5): -1, (0, 1023): M, (0, 1024): I32_MIN, (1, 1099): 2 ** 31 - 1, (1, 0): 65535, (1, 1): 1 << 16}
        mark = np.zeros((B, M), bool)
        for (b, n), v in forged_n.items():
            mark[b, nn_gp[b, n]] = True
            nn_gp[b, n] = v
        for (b, m), v in forged_m.items():
            mark[b, m] = True
            nn_pg[b, m] = v
        f = ops.ChamferTerms()
        f.nn_pg, f.nn_gp, f.elem_fwd, f.elem_bwd, f.M, f.N = _cu(nn_pg), _cu(nn_gp), t.levels[l].elem_fwd, t.levels[l].elem_bwd, M, N
        forged.append(f)
        counts.append(len(forged_m) + len(forged_n))
        touched.append(mark)
    got, bad = ops.chamfer_pyramid_grad(dps, dg, forged, gs)
    assert bad.cpu().tolist() == counts
    for l in range(2):
        one, bad1 = ops.chamfer_grad(dps[l], dg, forged[l], gs[l])
        assert int(bad1) == counts[l] and _same(got[l], one)                     # the single-level kernel skips the same entries
        a, c = got[l].cpu().numpy().transpose(0, 2, 1), clean[l].cpu().numpy().transpose(0, 2, 1)
        assert np.isfinite(a).all() and np.array_equal(a[~touched[l]].view(np.int32), c[~touched[l]].view(np.int32))
    # only one level forged: the other level's count stays zero
    got, bad = ops.chamfer_pyramid_grad(dps, dg, [t.levels[0], forged[1]], gs)
    assert bad.cpu().tolist() == [0, counts[1]] and _same(got[0], clean[0])


def test_dirty_buffers_offset_views_two_runs_and_a_graph_replay():
    from sonet_hip import _lib, ops
    import ctypes
    Ms, N, B, L = [257, 1025, 2], 1025, 3, 3
    preds, gt = _clouds("continuous", B, Ms, N)
    t, dps, dg, gs, clean = _check_grad(preds, gt, SCALES, "clean")
    again, _ = ops.chamfer_pyramid_grad(dps, dg, t, gs)
    for a, c in zip(again, clean):
        assert _same(a, c), "two runs differ"
    # every operand viewed at a 4-byte offset of its allocation (the kernels use 4-byte accesses only: no copy is needed)
    def shifted(x):
        buf = torch.empty((x.numel() + 1,), dtype=x.dtype, device=DEV)
        v = buf[1:].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 8 == 4 and v.is_contiguous()
        return v
    sp, sg = [shifted(p) for p in dps], shifted(dg)
    st = ops.chamfer_pyramid_terms(sp, sg)
    for lv, fl in zip(st.levels, t.levels):
        for k in KEYS:
            assert _same(getattr(lv, k), getattr(fl, k)), k
    sl = []
    for lv in t.levels:
        f = ops.ChamferTerms()
        f.nn_pg, f.nn_gp, f.elem_fwd, f.elem_bwd, f.M, f.N = shifted(lv.nn_pg), shifted(lv.nn_gp), shifted(lv.elem_fwd), shifted(lv.elem_bwd), lv.M, lv.N
        sl.append(f)
    off, bad = ops.chamfer_pyramid_grad(sp, sg, sl, shifted(gs))
    assert (bad == 0).all()
    for a, c in zip(off, clean):
        assert _same(a, c), "offset views differ"
    # outputs and workspace pre-filled with 0xFF, through ctypes
    lib = _lib.load()
    arr = lambda ts: (ctypes.c_void_p * 3)(*[x.data_ptr() for x in ts])          # noqa: E731

    def ff(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(shape)

    outs = [[ff((B, M if k in (0, 2) else N), torch.int32 if k < 2 else torch.float32) for M in Ms] for k in range(4)]
    sums = ff((B, L, 2), torch.float64)
    ws = torch.full((lib.sonet_chamfer_pyramid_ws_size(B, L, *Ms, N),), 0xFF, dtype=torch.uint8, device=DEV)
    dpr, bad = [ff((B, 3, M), torch.float32) for M in Ms], ff((L,), torch.int32)
    cm = (ctypes.c_int * 3)(*Ms)
    with torch.cuda.device(DEV):
        _lib.check(lib.sonet_chamfer_pyramid_loss_f32(arr(dps), _lib.ptr(dg), *[arr(o) for o in outs], _lib.ptr(sums), _lib.ptr(ws), B, L, cm, N,
                                                      _lib.stream_ptr()), "pyramid loss")
        _lib.check(lib.sonet_chamfer_pyramid_grad_f32(arr(dps), _lib.ptr(dg), *[arr(o) for o in outs], _lib.ptr(gs), arr(dpr), _lib.ptr(bad), B, L,
                                                      cm, N, _lib.stream_ptr()), "pyramid grad")
    assert _same(sums, t.sums) and (bad == 0).all()
    for l in range(L):
        for k in range(4):
            assert _same(outs[k][l], getattr(t.levels[l], KEYS[k])), (k, l)
        assert _same(dpr[l], clean[l]), l
    # a captured graph, replayed twice, gives the bits of the plain calls
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        for _ in range(2):
            ops.chamfer_pyramid_grad(dps, dg, ops.chamfer_pyramid_terms(dps, dg), gs)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        gt_terms = ops.chamfer_pyramid_terms(dps, dg)
        g_out, g_bad = ops.chamfer_pyramid_grad(dps, dg, gt_terms, gs)
    for _ in range(2):
        for o in g_out:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(gt_terms.sums, t.sums) and (g_bad == 0).all()
        for a, c in zip(g_out, clean):
            assert _same(a, c), "graph replay differs"


def test_n_at_the_extent_passes_and_one_beyond_is_refused_before_a_launch():
    from sonet_hip import _lib, ops
    from sonet_hip._lib import SonetHipError
    import ctypes
    N = ops.CHAMFER_PYRAMID_MAX_N
    preds, gt = _clouds("continuous", 1, (3, 300), N)
    _check_grad(preds, gt, SCALES[:2], "N at the extent", gate=False)
    dps, dg = [_cu(p) for p in preds], torch.zeros(1, 3, N + 1, device=DEV)
    with ops.kernel_timing() as rec:
        with pytest.raises(SonetHipError, match="N <= %d" % N):
            ops.chamfer_pyramid_terms(dps, dg)
        with pytest.raises(SonetHipError, match="N <= %d" % N):
            ops.chamfer_pyramid_loss(dps, dg)
    assert not rec.records
    # the C entries themselves: nothing is read or written (every pointer is one word)
    lib = _lib.load()
    word = torch.zeros(2, dtype=torch.float64, device=DEV)
    p = _lib.ptr(word)
    a = (ctypes.c_void_p * 3)(*[word.data_ptr()] * 3)
    cm = (ctypes.c_int * 3)(1, 1, 1)
    assert lib.sonet_chamfer_pyramid_loss_f32(a, p, a, a, a, a, p, p, 1, 2, cm, N + 1, None) == 2 and "N=%d" % (N + 1) in _lib.last_error()
    assert lib.sonet_chamfer_pyramid_grad_f32(a, p, a, a, a, a, p, a, p, 1, 2, cm, N + 1, None) == 2 and "N=%d" % (N + 1) in _lib.last_error()
    cm = (ctypes.c_int * 3)(1, ops.CHAMFER_PYRAMID_MAX_M + 1, 1)
    assert lib.sonet_chamfer_pyramid_grad_f32(a, p, a, a, a, a, p, a, p, 1, 2, cm, 8, None) == 2 and "M[1]" in _lib.last_error()
    torch.cuda.synchronize()
    assert (word == 0).all()


# ------------------------------------------------------------------------------------------------------------ operator and module
def test_operator_backward_twice_and_unused_outputs():
    from sonet_hip import ops
    Ms, N, B = (257, 64, 300), 1025, 3
    preds, gt = _clouds("continuous", B, Ms, N)
    dg = _cu(gt)
    ps = [_cu(p).requires_grad_(True) for p in preds]
    with ops.kernel_timing() as rec:
        levels = ops.chamfer_pyramid_loss(ps, dg)
        torch.cuda.synchronize()
    assert {k: v["count"] for k, v in rec.summary().items()} == {"chamfer_pyramid_loss": 1}
    ref = P.terms(preds, gt)
    for (fl, bl, fa, ba), r in zip(levels, P.losses(ref)):
        assert fl.dtype == bl.dtype == fa.dtype == ba.dtype == torch.float32 and fl.dim() == bl.dim() == 0 and tuple(fa.shape) == (B,)
        assert fl.requires_grad and bl.requires_grad and not fa.requires_grad and not ba.requires_grad
        for got, want in ((fl, r["forward_loss"]), (bl, r["backward_loss"])):
            assert abs(float(got.detach()) - want) <= 2.0 ** -24 * want * 1.001
        np.testing.assert_allclose(fa.cpu().numpy(), r["forward_loss_array"], rtol=2.0 ** -23)
        np.testing.assert_allclose(ba.cpu().numpy(), r["backward_loss_array"], rtol=2.0 ** -23)
    w = [(0.7, -1.3), (1.0, 1.0), (0.25, 3.0)]
    total = sum(a * lv[0] + b * lv[1] for (a, b), lv in zip(w, levels))
    with ops.kernel_timing() as rec:
        total.backward(retain_graph=True)
        torch.cuda.synchronize()
    assert {k: v["count"] for k, v in rec.summary().items()} == {"chamfer_pyramid_grad": 1}
    first = [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    total.backward(retain_graph=True)
    for l, p in enumerate(ps):
        assert _same(first[l], p.grad), "second backward through the retained graph differs"
        gf, gb = (float(np.float32(v)) for v in w[l])
        ref64, mag = R.grad(preds[l], gt, ref[l]["nn_pg"], ref[l]["nn_gp"], gf, gb)
        assert (np.abs(first[l].cpu().numpy().astype(np.float64) - ref64) <= R.GATE * mag).all(), l
        p.grad = None
    # one output of one level used: every other scale is zero, the other levels get a gradient of zeros (or none)
    levels[1][1].backward(retain_graph=True)
    ref64, mag = R.grad(preds[1], gt, ref[1]["nn_pg"], ref[1]["nn_gp"], 0.0, 1.0)
    assert (np.abs(ps[1].grad.cpu().numpy().astype(np.float64) - ref64) <= R.GATE * mag).all()
    assert all(p.grad is None or (p.grad == 0).all() for p in (ps[0], ps[2]))
    # a level that asks for no gradient
    q = [_cu(preds[0]).requires_grad_(True), _cu(preds[1])]
    lv = ops.chamfer_pyramid_loss(q, dg)
    (lv[0][0] + lv[0][1] + lv[1][0]).backward()
    one = _cu(preds[0]).requires_grad_(True)
    fl, bl, _, _ = ops.chamfer_loss(one, dg)
    (fl + bl).backward()
    assert _same(q[0].grad, one.grad) and q[1].grad is None


def _opt(**kw):
    base = dict(gpu_id=0, device=DEV, batch_size=2, input_pc_num=1024, surface_normal=True, feature_num=1024, activation="relu",
                normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1, bn_momentum_decay_step=None,
                bn_momentum_decay=0.6, classes=40, output_fc_pc_num=256, output_conv_pc_num=1024)
    base.update(kw)
    return Namespace(**base)


def _step(crit, clouds, dec, gt):
    """loss + backward on fresh leaves -> (module, gradients, launch counts)."""
    from sonet_hip import ops
    leaves = [c.detach().clone().requires_grad_(True) for c in clouds]
    d = Namespace(conv_pc4=leaves[-1] if len(leaves) > 1 else None, conv_pc5=leaves[1] if len(leaves) > 2 else None)
    with ops.kernel_timing() as rec:
        loss = crit(leaves[0], d, gt)
        loss.backward()
        torch.cuda.synchronize()
    return loss.detach(), [x.grad for x in leaves], {k: v["count"] for k, v in rec.summary().items()}


@pytest.mark.parametrize("conv", [0, 1024, 4096])
def test_autoencoder_loss_option_on_against_option_off_and_routing(conv):
    from models import losses as LS
    B, N = 2, 1100
    Ms = {0: (256,), 1024: (1280, 256), 4096: (4352, 1024, 256)}[conv]
    preds, gt = _clouds("continuous", B, Ms, N)
    clouds, dg = [_cu(p) for p in preds], _cu(gt)
    on, off, absent = (LS.AutoencoderLoss(_opt(output_conv_pc_num=conv, **kw)) for kw in (dict(chamfer_pyramid=True), dict(chamfer_pyramid=False), dict()))
    l_on, g_on, k_on = _step(on, clouds, None, dg)
    l_off, g_off, k_off = _step(off, clouds, None, dg)
    l_abs, g_abs, k_abs = _step(absent, clouds, None, dg)
    assert k_on == {"chamfer_pyramid_loss": 1, "chamfer_pyramid_grad": 1}       # one loss launch, one gradient launch, no chamfer_nn
    assert k_off == k_abs == {"chamfer_nn": 2 * len(Ms)}
    # option absent: the parent's bits -- ChamferLoss called per term by hand, in the reference's order of calls and of the sum
    crit = LS.ChamferLoss(_opt())
    leaves = [c.detach().clone().requires_grad_(True) for c in clouds]
    terms = [crit(x, dg) for x in leaves[1:] + leaves[:1]]
    terms = terms[-1:] + terms[:-1]
    hand = terms[0]
    for x in terms[1:]:
        hand = hand + x
    assert _same(hand.detach(), l_abs) and _same(l_off, l_abs)
    names = {1: ("loss_chamfer",), 2: ("loss_chamfer", "loss_chamfer_conv4"), 3: ("loss_chamfer", "loss_chamfer_conv5", "loss_chamfer_conv4")}
    for l, name in enumerate(names[len(Ms)]):
        a, b = float(getattr(on, name).detach()), float(getattr(absent, name).detach())
        assert abs(a - b) <= 2e-6 * b, (name, a, b)
        assert _same(getattr(absent, name).detach(), terms[l].detach()), name
    assert abs(float(l_on) - float(l_abs)) <= 2e-6 * float(l_abs)
    assert (on.loss_chamfer_conv5 is None) == (absent.loss_chamfer_conv5 is None) == (conv != 4096)
    assert (on.loss_chamfer_conv4 is None) == (absent.loss_chamfer_conv4 is None) == (conv == 0)
    for a, b in zip(g_on, g_abs):
        assert_close_rms(a.cpu().numpy(), b.cpu().numpy(), 1e-5, "d loss / d predicted cloud, option on against absent")
    # with the option on, these keep the present path: another dtype, a gt that asks for a gradient, a gt past the extent
    _, _, k = _step(on, [c.bfloat16() for c in clouds], None, dg.bfloat16())
    assert "chamfer_pyramid_loss" not in k and k["chamfer_nn"] == 2 * len(Ms)
    _, _, k = _step(on, clouds, None, dg.clone().requires_grad_(True))
    assert "chamfer_pyramid_loss" not in k and k["chamfer_nn"] == 2 * len(Ms)


def test_autoencoder_loss_past_the_extent_takes_the_present_path():
    from models import losses as LS
    from sonet_hip import ops
    preds, gt = _clouds("continuous", 1, (64,), ops.CHAMFER_PYRAMID_MAX_N + 1)
    on = LS.AutoencoderLoss(_opt(output_conv_pc_num=0, chamfer_pyramid=True))
    _, _, k = _step(on, [_cu(preds[0])], None, _cu(gt))
    assert k == {"chamfer_nn": 2}


@pytest.mark.parametrize("case", AE_CASES)
def test_decoder_and_autoencoder_loss_on_the_reference_fixtures(case):
    """The stored feature of the reference's run through Decoder + AutoencoderLoss, option on and absent: the reference's loss terms."""
    from models import losses as LS, networks as NW
    from sonet_hip import synth
    g = golden(case)
    opt = _opt(batch_size=int(g["B"]), input_pc_num=int(g["N"]))
    dec = NW.Decoder(opt)
    synth.fill_state_dict_(dec.state_dict(), int(g["seed"]) + 1)
    dec.to(DEV).eval()
    gt = _cu(g["pc"])
    for kw in (dict(chamfer_pyramid=True), dict()):
        crit = LS.AutoencoderLoss(_opt(**kw))
        with torch.no_grad():
            pred = dec(_cu(g["feature"]))
            loss = crit(pred, dec, gt)
        for k in ("loss", "loss_chamfer", "loss_chamfer_conv4"):
            assert abs(float(getattr(crit, k)) - float(g[k])) <= 2e-5 * float(g[k]), (kw, k, float(getattr(crit, k)), float(g[k]))
        assert float(loss) == float(crit.loss) and crit.loss_chamfer_conv5 is None
        # on the reference's own clouds the terms are held to the loss's own gate
        ref_dec = Namespace(conv_pc4=_cu(g["conv_pc4"]), conv_pc5=None)
        p = _cu(g["predicted_pc"]).requires_grad_(True)
        crit(p, ref_dec, gt).backward()
        for k in ("loss", "loss_chamfer", "loss_chamfer_conv4"):
            assert abs(float(getattr(crit, k).detach()) - float(g[k])) <= 2e-6 * float(g[k]), (kw, k)
        assert abs(float(crit.forward_loss.detach()) - float(g["forward_loss"])) <= 2e-6 * float(g["forward_loss"])
        assert abs(float(crit.backward_loss.detach()) - float(g["backward_loss"])) <= 2e-6 * float(g["backward_loss"])
        np.testing.assert_allclose(crit.loss_array.detach().cpu().numpy(), g["loss_array"], rtol=5e-6)
        assert_close_rms(p.grad.cpu().numpy(), g["grad_predicted"], 1e-5, "d loss / d predicted_pc")
