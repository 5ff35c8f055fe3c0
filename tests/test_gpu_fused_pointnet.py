"""The fused first PointNet (so-net_amd/csrc/pointresnet_fused.hip), every variant, against tests/fused_pointnet_ref.py.

Exact networks (tests/test_fused_pointnet_cpu.py derives that the kernel's arithmetic rounds nothing on them): the store variants, their P16
planes and the pooled variants are compared BIT FOR BIT with the float64 network -- no tolerance; a permuted channel, a stale register, a
missed flush of the pool bins or a tail error changes bits.  The continuous network (the parity tests' seeded PointResNet) covers the
arithmetic that exact inputs cannot reach, at the project's 1e-5 gate, and the properties that need no reference: a column's result does not
depend on where it sits, nor on what its neighbours hold, and the pooled variant is the pool of what the store variant writes."""
import functools

import numpy as np
import pytest
import torch

import fused_pointnet_ref as R
from conftest import assert_close_rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P16_SETTINGS = (False, True, "only")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_PACKS = {}


def packed(net):
    from sonet_hip import ops
    key = (net.name, net.affine.tobytes())
    if key not in _PACKS:
        _PACKS[key] = (ops.pointresnet_pack(*[cu(W) for W in net.Ws]), cu(net.affine))
    return _PACKS[key]


def planes_of(p):
    return p.data.cpu().numpy().view(np.uint16).reshape(p.B, (p.C + 15) // 16, 2, 2, p.L, 8)


def run_store(net, x, clean=True):
    """All three ``want_p16`` settings of ops.pointresnet_fused -> y float32 [B][384][L]; the planes written alongside y and those written
    alone must be the split of y (tests/test_gpu_h3p.py's layout, restated in R.p16_planes)."""
    from sonet_hip import ops
    ws, aff = packed(net)
    xd = cu(x)
    got = {}
    for want in P16_SETTINGS:
        with ops.range_scope(torch.device(DEV)) as rs:
            got[want] = ops.pointresnet_fused(xd, ws, aff, want_p16=want)
        bad = rs.violations()
        if clean:
            assert bad == [], (net.name, x.shape, want, bad)
    y = got[False].cpu().numpy()
    y2, yp = got[True]
    none, yp_only = got["only"]
    assert none is None and np.array_equal(y2.cpu().numpy().view(np.uint32), y.view(np.uint32))
    if clean:
        want_planes = R.p16_planes(y)
        assert np.array_equal(planes_of(yp), want_planes), "P16 planes written with y"
        assert np.array_equal(planes_of(yp_only), planes_of(yp)), "P16 planes written alone"
    return y


def check_store_exact(net, B, L, seed=0):
    x, ref = net.x_and_ref(B, L, seed)
    y = run_store(net, x)
    bad = y.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s B=%d L=%d: %d elements differ, first at %s" % (net.name, B, L, int(bad.sum()), tuple(np.argwhere(bad)[0]))


# ---------------------------------------------------------------------------------------------- store variants, exact networks
@pytest.mark.parametrize("flavour", ["A", "B"])
@pytest.mark.parametrize("L", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513])
def test_store_exact_at_the_tile_edges(L, flavour):
    check_store_exact(R.exact_network(6, flavour, "half"), 2, L)


@pytest.mark.parametrize("flavour", ["A", "B"])
@pytest.mark.parametrize("cin0", R.CIN0S)
def test_store_exact_every_input_width(cin0, flavour):
    check_store_exact(R.exact_network(cin0, flavour, "half"), 2, 257)


@pytest.mark.parametrize("flavour", ["A", "B"])
@pytest.mark.parametrize("case", ["cus-1", "cus", "cus+1", "2cus+1", "3x600", "cus+1_tiles_of_600"])
def test_store_exact_on_the_persistent_walk(case, flavour):
    """Tile counts on both sides of the grid (one workgroup per compute unit), one and several rounds, and workgroups whose successive tiles
    belong to different clouds."""
    n = cus()
    B, L = {"cus-1": (n - 1, 1), "cus": (n, 1), "cus+1": (n + 1, 1), "2cus+1": (2 * n + 1, 1), "3x600": (3, 600),
            "cus+1_tiles_of_600": (-(-(n + 1) // 3), 600)}[case]
    ntiles = B * -(-L // R.TPTS)
    if case in ("cus+1", "2cus+1", "cus+1_tiles_of_600"):
        assert ntiles > n, "the case is meant to reach the persistent loop"
    check_store_exact(R.exact_network(6, flavour, "half"), B, L, seed=1)


def test_store_exact_with_mixed_layer4_scales():
    check_store_exact(R.exact_network(6, "A", "mixed"), 2, 300)


# ---------------------------------------------------------------------------------------------- store variant, continuous network
@pytest.mark.parametrize("B,cin0,L", [(2, 6, 300), (1, 6, 1), (2, 3, 513)])
def test_store_continuous_meets_the_gate(B, cin0, L):
    net, _ = R.continuous_network(cin0)
    x = net.make_x(B, L, seed=L)
    y, ref = run_store(net, x), net.ref(x)
    print("store %s: worst error / max(|ref|, rms) = %.3g" % ((B, cin0, L), R.rms_ratio(y, ref)))
    assert_close_rms(y, ref, 1e-5, "fused first PointNet %s" % ((B, cin0, L),))


@pytest.mark.parametrize("cin0", [6, 3])
def test_forward64_is_the_module_layer_by_layer(cin0):
    """The restatement against PointResNet.forward ITSELF (the module has no CPU path: tests/test_fused_pointnet_cpu.py can only restate its
    data flow in torch operators): four layer-wise launches in the exact-f32 arithmetic, which never takes the fused kernel, so the order
    of the skip and main panels in layer 4 is the module's own.  1e-5 is the project's gate for a float32 path against float64; a
    panel exchanged or a layer skipped is off by the size of the values."""
    from sonet_hip import ops
    net, pr64 = R.continuous_network(cin0)
    import copy
    pr = copy.deepcopy(pr64).float().to(DEV).eval()
    x = net.make_x(2, 77, seed=5)
    with torch.no_grad(), ops.precision("f32"), ops.kernel_timing() as rec:
        y = pr(cu(x)).cpu().numpy()
    assert not any(n.startswith("pointresnet_fused") for n, _, _ in rec.records), "the fused kernel ran"
    ref = net.ref(x)
    print("module, layer by layer, Cin0 = %d: worst error / max(|ref|, rms) = %.3g" % (cin0, R.rms_ratio(y, ref)))
    assert_close_rms(y, ref, 1e-5, "PointResNet layer by layer against forward64")
    assert not np.allclose(net.ref(x, brk="panels"), ref, rtol=1e-3, atol=0)


def test_store_result_does_not_depend_on_the_position():
    net, _ = R.continuous_network(6)
    block = net.make_x(1, 37, seed=2)
    L = 3 * R.TPTS + 37
    x = np.ascontiguousarray(np.broadcast_to(block[:, :, np.arange(L) % 37], (2, 6, L)))
    y = run_store(net, x).view(np.uint32)
    assert np.array_equal(y, np.broadcast_to(y[:1, :, :37][:, :, np.arange(L) % 37], y.shape)), "a copy of a column came out with other bits"


def test_store_columns_are_isolated_from_their_neighbours():
    from sonet_hip import ops
    net, _ = R.continuous_network(6)
    x = net.make_x(2, 300, seed=4)
    y = run_store(net, x)
    xb = x.copy()
    hit = [(0, 5), (0, 290), (1, 31)]
    xb[0, :, 5], xb[0, 2, 290], xb[1, 4, 31] = np.nan, np.inf, 1e5
    ws, aff = packed(net)
    with ops.range_scope(torch.device(DEV)) as rs:
        yb = ops.pointresnet_fused(cu(xb), ws, aff).cpu().numpy()
    bad = rs.violations()
    assert bad and any("max |x|" in what for _, what in bad), bad
    keep = np.ones((2, 300), bool)
    for b, l in hit:
        keep[b, l] = False
    assert np.array_equal(np.transpose(yb, (0, 2, 1))[keep].view(np.uint32), np.transpose(y, (0, 2, 1))[keep].view(np.uint32))


# ---------------------------------------------------------------------------------------------- pool variants
LAYOUTS = ("two_nodes_every_boundary", "three_nodes_and_one_point_nodes", "ragged_last_tile", "tile_17_18_64_ids", "slot18_continues_as_slot0",
           "ids_n_and_n_plus_20", "node_spans_four_tiles", "empty_nodes", "pos0_0_31_32", "pos0_255_256_last", "M1", "M33", "M64", "M65",
           "persistent_small_clouds")


def layout(name):
    lay = R.layouts(cus())
    assert set(lay) == set(LAYOUTS)
    return lay[name]


def group(x, ids, pos0, M):
    sg = R.sort_group(x, ids, pos0, M)
    return {k: v.to(DEV) for k, v in sg.items()}


def run_pool(net, sg, M, B):
    """Both ``want_p16`` settings of ops.pointresnet_fused_pool, each twice -> out float32 [B][384][M]: bit-identical from run to run and
    between the settings, the planes are the split of ``out`` on the flat node axis."""
    from sonet_hip import ops
    ws, aff = packed(net)
    outs = []
    for want in (False, True, False, True):
        with ops.range_scope(torch.device(DEV)) as rs:
            r = ops.pointresnet_fused_pool(sg, ws, aff, M, want_p16=want)
        assert rs.violations() == [], (net.name, rs.violations())
        outs.append(r)
    out = outs[0].cpu().numpy()
    Lm = ops.node_stage_columns(B, M)
    want_planes = R.p16_planes_flat(out, Lm)
    for r in outs[1:]:
        o = (r[0] if isinstance(r, tuple) else r).cpu().numpy()
        assert np.array_equal(o.view(np.uint32), out.view(np.uint32)), "the pooled result changed from one run to the next"
        if isinstance(r, tuple):
            pl = r[1].data.cpu().numpy().view(np.uint16).reshape(24, 2, 2, Lm, 8)
            assert np.array_equal(pl[:, :, :, :B * M], want_planes), "P16 planes of the pooled map"
            assert not pl[:, :, :, B * M:].any()
    return out


@pytest.mark.parametrize("l4", ["unit", "mixed"])
@pytest.mark.parametrize("name", LAYOUTS)
def test_pool_exact_on_every_layout(name, l4):
    """Flavour A, Cin0 = 6: the pooled map equals pool64(forward64) bit for bit; "mixed" = layer-4 scales other than 1 (negative ones too) on a
    third of the channels, the pool's general branch."""
    ids, pos0, M = layout(name)
    B, L = ids.shape
    if name == "persistent_small_clouds":
        assert B > cus()
    net = R.exact_network(6, "A", l4)
    x, y = net.x_and_ref(B, L, seed=3)
    ref = R.pool64(y, ids, pos0, M)
    out = run_pool(net, group(x, ids, pos0, M), M, B)
    bad = ~((out + np.float32(0)).view(np.uint32) == ref.view(np.uint32))
    assert not bad.any(), "%s: %d pooled elements differ, first at (cloud, channel, node) %s" % (name, int(bad.sum()), tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("name", LAYOUTS)
def test_pool_continuous_is_the_pool_of_the_store_variant(name):
    ids, pos0, M = layout(name)
    B, L = ids.shape
    net, _ = R.continuous_network(6)
    x = net.make_x(B, L, seed=6)
    y = run_store(net, x)
    out = run_pool(net, group(x, ids, pos0, M), M, B)
    ref = R.pool64(net.ref(x), ids, pos0, M)
    print("pool %s: worst error / max(|ref|, rms) = %.3g" % (name, R.rms_ratio(out, ref)))
    assert_close_rms(out, ref, 1e-5, "fused pool %s" % name)
    assert R.same_bits(out, R.pool64(y, ids, pos0, M)), "the pooled variant is not the pool of what the store variant writes"


@pytest.mark.parametrize("name", LAYOUTS)
def test_bf16_pool_is_the_pool_of_the_bf16_store_variant(name):
    from sonet_hip import ops
    ids, pos0, M = layout(name)
    B, L = ids.shape
    net, _ = R.continuous_network(6)
    x = net.make_x(B, L, seed=6)
    key = ("bf16", net.name)
    if key not in _PACKS:
        _PACKS[key] = (ops.pointresnet_bf16_pack(*[cu(W) for W in net.Ws]), cu(net.affine))
    ws, aff = _PACKS[key]
    y = ops.pointresnet_bf16(cu(x), ws, aff).float().cpu().numpy()
    sg = group(x, ids, pos0, M)
    out = [ops.pointresnet_bf16_pool(sg, ws, aff, M).cpu().numpy() for _ in range(2)]
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), "the pooled result changed from one run to the next"
    assert R.same_bits(out[0], R.pool64(y, ids, pos0, M))
