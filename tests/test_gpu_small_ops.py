"""The node-level gather, max, FC and Adam kernels against tests/small_ops_ref.py, bit for bit (linear_act: within its derived bound), at
the block / grid / dispatch edges of each kernel and with indices outside [0, M).  The shapes and what each reaches are listed next to the
inputs in small_ops_ref.py; tests/test_small_ops_cpu.py pins that file to the reference's torch expressions.

Measured on the MI355X (docs/findings.md): every comparison below is bit-equal; linear_act's worst error is 0.09 of its bound (Cin = 4)
and 0.002 at Cin = 4096."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "so-net_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import small_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def bits(got, ref, what=""):
    got = host(got) if isinstance(got, torch.Tensor) else got
    assert R.same_bits(got, ref), "%s: %s" % (what, R.first_diff(got, ref))


def ids_of(shape):
    return "x".join(str(s) for s in shape)


# ---------------------------------------------------------------------------------------------- gathers and grouping
@pytest.mark.parametrize("shape", R.KNN_SHAPES, ids=ids_of)
def test_knn_gather_group_prepare_bits(shape):
    from sonet_hip import ops
    B, C, M, K = shape
    coord, feat, I = R.knn_inputs(B, C, M, K)
    ok = R.in_range(I, M)[1]
    assert not ok[B - 1, M // 2].any() and (M * K == 1 or (~ok).sum() >= min(5, M * K - 1))
    dc, df, dI = dev(coord), dev(feat), dev(I)
    bad = []                                                     # (every comparison is made before any is asserted: the message names them all)

    def cmp(got, ref, what):
        if not R.same_bits(host(got), ref):
            bad.append("%s: %s" % (what, R.first_diff(host(got), ref)))

    cmp(ops.knn_gather(df, dI), R.gather(feat, I), "knn_gather")
    for avg in (True, False):
        rc, ro = R.knn_group(coord, feat, I, avg)
        center, out = ops.knn_group(dc, df, dI, avg)
        cmp(center, rc, "knn_group centre avg=%d" % avg)
        cmp(out, ro, "knn_group out avg=%d" % avg)
        pc, dec, gidx = ops.knn_prepare(dc, dI, avg)
        qc, qd, qg = R.knn_prepare(coord, I, avg)
        cmp(pc, qc, "knn_prepare centre avg=%d" % avg)
        cmp(dec, qd, "knn_prepare dec avg=%d" % avg)
        if not np.array_equal(host(gidx), qg):
            bad.append("knn_prepare gidx")
        # ... and the two kernels agree with each other: the same numbers, transposed
        cmp(dec.view(B, 3, K, M).transpose(2, 3).contiguous(), host(out)[:, :3], "knn_prepare vs knn_group avg=%d" % avg)
        cmp(pc, host(center), "knn_prepare vs knn_group centre avg=%d" % avg)
        if avg:                                                  # the node whose K neighbours are all out of range: 0 / K, rows 0 - 0
            assert not host(center)[B - 1, :, M // 2].any() and not host(out)[B - 1, :, M // 2, :].any()
            assert not np.signbit(host(center)[B - 1, :, M // 2]).any()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,C,kN", [(1, 1, 1), (2, 3, 2), (2, 3, 3), (3, 85, 4), (1, 256, 4), (1, 257, 4), (2, 3, 5), (2, 3, 1021), (2, 3, 1022),
                                    (2, 3, 1023), (1, 5, 1024)])
def test_node_gather_bits(B, C, kN):
    """kN around the quad (the last quad of a row is partial unless kN % 4 == 0; rows of 1021 .. 1023 floats start off a 16-byte boundary:
    the kernel's address test) and B C ceil(kN / 4) = 255, 256, 257 around the block edge; ids -1, M, INT32_MIN read as 0."""
    from sonet_hip import ops
    for M in (1, 7):
        g = np.random.default_rng([B, C, kN, M])
        feat, ids = (g.standard_normal((B, C, M)) + 3).astype(np.float32), R.node_ids(g, B, kN, M)
        bits(ops.node_gather(dev(feat), dev(ids)), R.gather(feat, ids), "node_gather M=%d" % M)


@pytest.mark.parametrize("B,kN,M", [(1, 5, 1), (2, 7, 3), (1, 255, 4), (1, 256, 4), (1, 257, 4), (1, 16, 64), (1, 17, 64), (3, 11, 65), (2, 4, 65)])
def test_som_mask_bits(B, kN, M):
    """M % 4 == 0: one thread per 4 entries (rows M / 4 = 255, 256, 257 and 256, 272), else per entry; out-of-range ids give empty rows."""
    from sonet_hip import ops
    ids = R.node_ids(np.random.default_rng([B, kN, M]), B, kN, M)
    got = host(ops.som_mask(dev(ids), M))
    assert got.dtype == np.int32 and np.array_equal(got, R.som_mask(ids, M))


# ---------------------------------------------------------------------------------------------- maxima
@pytest.mark.parametrize("K", R.LASTDIM_K)
def test_lastdim_max_bits(K):
    from sonet_hip import ops
    for rows in R.LASTDIM_ROWS:
        x = R.lastdim_inputs(rows, K)
        ref = R.lastdim_max(x)
        got = ops.lastdim_max(dev(x))
        bits(got, ref, "lastdim_max rows=%d K=%d" % (rows, K))
        assert torch.equal(got.view(torch.int32), ops.lastdim_max(dev(x)).view(torch.int32))           # run to run
    xb = R.round_bf16(np.nan_to_num(R.lastdim_inputs(65, K), nan=0.25))
    bits(ops.lastdim_max(dev(xb, torch.bfloat16).view(5, 13, K)), R.lastdim_max(xb).reshape(5, 13), "lastdim_max bf16 K=%d" % K)


@pytest.mark.parametrize("K", [1, 2, 9])
def test_planes_max_bits(K):
    from sonet_hip import ops
    for (B, C, M) in ((3, 85, 1), (1, 256, 1), (1, 257, 1), (1, 37, 7), (2, 2, 64), (1, 5, 64)):
        g = np.random.default_rng([B, C, M, K])
        x = g.standard_normal((B, C, K * M)).astype(np.float32)
        for n, k in enumerate(sorted({0, K // 2, K - 1})):       # a NaN in the first, a middle and the last plane, one (row, m) each
            x[B - 1, n % C, k * M + (n % M)] = np.nan
        x[0, C - 1, :] = -np.inf
        ref = R.planes_max(x, K)
        assert np.isnan(ref).sum() >= 1
        got = ops.planes_max(dev(x), K)
        bits(got, ref, "planes_max %s" % ((B, C, M, K),))
        assert torch.equal(got.view(torch.int32), ops.planes_max(dev(x), K).view(torch.int32))
        xb = R.round_bf16(np.nan_to_num(x, nan=0.5, neginf=-3.0))
        bits(ops.planes_max(dev(xb, torch.bfloat16), K), R.planes_max(xb, K), "planes_max bf16")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,K", [(255, 1), (256, 9), (257, 64), (7, 3), (1, 1000)])
def test_lastdim_max_autograd_bits(rows, K, dtype):
    """Forward value, the saved arg-max (FIRST maximum, FIRST NaN) and the backward against the restatement: K = 1, a row with two NaNs, a
    -inf row, an all-equal row, rows around the block edge."""
    from sonet_hip import ops
    bf16 = dtype == torch.bfloat16
    x = R.argmax_inputs(rows, K, bf16)
    val, idx = R.lastdim_argmax(x)
    xt = dev(x, dtype).requires_grad_(True)
    y = ops.lastdim_max_autograd(xt)
    assert y.dtype == dtype
    bits(y.detach(), val, "value")
    (saved,) = y.grad_fn.saved_tensors
    assert np.array_equal(host(saved), idx)
    gy = np.random.default_rng([rows, K]).standard_normal(rows).astype(np.float32)
    gy = R.round_bf16(gy) if bf16 else gy
    y.backward(dev(gy, dtype))
    assert xt.grad.dtype == dtype
    bits(xt.grad, R.lastdim_max_bwd(gy, idx, K), "gradient")


# ---------------------------------------------------------------------------------------------- backward gathers
def _knn_bwd_tables():
    cs = [("existing-%d" % n, s, "seeded") for n, s in enumerate([(4, 384, 64, 9), (2, 3, 64, 9), (3, 17, 30, 5), (1, 8, 1000, 4),
                                                                   (2, 5, 1024, 3), (1, 4, 1024, 14)])]    # (the last: M K = 14336, the limit)
    cs += [("self-first", (2, 3, 64, 9), "self"), ("one-owner", (2, 3, 64, 9), "owner"), ("M1", (3, 2, 1, 4), "seeded"),
           ("K1", (2, 3, 257, 1), "seeded")]
    return cs


def _knn_table(shape, kind):
    B, C, M, K = shape
    I = R.knn_inputs(B, C, M, K, oor=(kind == "seeded"))[2]
    if kind == "self":
        I[:, :, 0] = np.arange(M)
    if kind == "owner":
        I[:] = 5                                                 # node 5 owns all M K entries, every other list is empty
    return I


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,shape,kind", _knn_bwd_tables(), ids=[c[0] for c in _knn_bwd_tables()])
def test_knn_gather_bwd_bits(name, shape, kind, dtype):
    from models import operations
    from sonet_hip import ops
    B, C, M, K = shape
    I = _knn_table(shape, kind)
    gy = np.random.default_rng([B, C, M, K]).standard_normal((B, C, M, K)).astype(np.float32)
    gy = R.round_bf16(gy) if dtype == torch.bfloat16 else gy
    ref = R.knn_gather_bwd(gy, I, M)
    dI, dg = dev(I), dev(gy, dtype)
    got = ops.knn_gather_bwd(dg, dI, M)
    assert got.dtype == torch.float32
    bits(got, ref, "knn_gather_bwd %s" % name)
    assert torch.equal(got.view(torch.int32), ops.knn_gather_bwd(dg, dI, M).view(torch.int32))      # run to run
    if dtype == torch.float32:                                   # autograd's route against the RESTATEMENT, not against the kernel itself
        x = torch.randn(B, C, M, device=DEV).requires_grad_(True)
        operations.knn_gather_by_indexing(x, dI).backward(dg)
        bits(x.grad, ref, "autograd %s" % name)


def test_knn_gather_bwd_past_the_lds_limit():
    """M K = 14337, one index past 56 KiB: the C entry refuses, the autograd node takes scatter_add (atomic order: float64 compare)."""
    from models import operations
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    B, C, M, K = 1, 2, 243, 59
    I = R.knn_inputs(B, C, M, K, oor=False)[2]
    gy = np.random.default_rng(3).standard_normal((B, C, M, K)).astype(np.float32)
    with pytest.raises(SonetHipError, match="LDS"):
        ops.knn_gather_bwd(dev(gy), dev(I), M)
    x = torch.randn(B, C, M, device=DEV).requires_grad_(True)
    operations.knn_gather_by_indexing(x, dev(I)).backward(dev(gy))
    ref = R.knn_gather_bwd(gy.astype(np.float64), I, M)
    # an f32 sum of n terms in any order: at most (n - 1) roundings, each at most 2^-24 of the sum of the magnitudes
    n, mag = R.knn_gather_bwd(np.ones_like(gy, np.float64), I, M), R.knn_gather_bwd(np.abs(gy).astype(np.float64), I, M)
    assert (np.abs(host(x.grad) - ref) <= n * R.U24 * mag).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C,L,M", [(2, 3, 13, 7), (2, 3, 8193, 64), (1, 2, 8193, 1024), (1, 1, 1, 1)])
def test_node_gather_bwd_bits(B, C, L, M, dtype):
    """L = 8193: one id past the 8192-id chunk of the inverse-list kernel; ids -1, M, INT32_MIN belong to nobody; M = 1024: the limit."""
    from sonet_hip import ops
    g = np.random.default_rng([B, C, L, M])
    ids = R.node_ids(g, B, L, M)
    gy = g.standard_normal((B, C, L)).astype(np.float32)
    gy = R.round_bf16(gy) if dtype == torch.bfloat16 else gy
    got = ops.node_gather_bwd(dev(gy, dtype), dev(ids), M)
    bits(got, R.node_gather_bwd(gy, ids, M), "node_gather_bwd")
    assert torch.equal(got.view(torch.int32), ops.node_gather_bwd(dev(gy, dtype), dev(ids), M).view(torch.int32))


# ---------------------------------------------------------------------------------------------- the two fma kernels
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", R.NODE_ADD_SHAPES, ids=ids_of)
def test_node_add_affine_act_bits(shape, relu):
    from sonet_hip import ops
    B, C, L, M = shape
    d = R.node_add_inputs(B, C, L, M)
    ref = R.node_add_affine_act(d["t"], d["z"], d["ids"], d["sc"], d["sh"], relu)
    t = dev(d["t"])
    got = ops.node_add_affine_act_(t, dev(d["z"]), dev(d["ids"]), dev(d["sc"]), dev(d["sh"]), relu)
    assert got is t
    bits(got, ref, "node_add_affine_act")
    out = host(got)
    assert out[0, 0, 0] == 0 and np.signbit(out[0, 0, 0]) and np.isnan(out).sum() == 1 and np.isnan(out[d["nan_at"]])


def test_node_add_affine_act_refuses_m_8193():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    t, z, ids, v = torch.zeros(1, 1, 4, device=DEV), torch.zeros(1, 1, 8193, device=DEV), torch.zeros(1, 4, dtype=torch.int32, device=DEV), \
        torch.ones(1, device=DEV)
    with pytest.raises(SonetHipError, match="M=8193"):
        ops.node_add_affine_act_(t, z, ids, v, v, True)
    with pytest.raises(SonetHipError, match="C = 1"):
        ops.node_add_affine_act_(t, z[:, :, :4].contiguous(), ids, torch.ones(2, device=DEV), v, True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", R.LEAD_SHAPES, ids=ids_of)
def test_node_gather_lead_affine_act_bits(shape, dtype):
    from sonet_hip import ops
    B, C, L, M, NL = shape
    bf16 = dtype == torch.bfloat16
    d = R.fma_case_inputs(B, C, L, M, NL, bf16)
    assert (d["ids"] == -1).any() or B * L < 8                   # gidx = -1, as knn_prepare emits it
    for relu in (False, True):
        ref = R.node_gather_lead(d["z"], d["ids"], d["lead"], d["wl"], d["sc"], d["sh"], relu, bf16)
        got = ops.node_gather_lead_affine_act(dev(d["z"], dtype), dev(d["ids"]), dev(d["lead"]), dev(d["wl"]), dev(d["sc"]), dev(d["sh"]), relu)
        assert got.dtype == dtype
        bits(got, ref, "node_gather_lead relu=%d" % relu)


# ---------------------------------------------------------------------------------------------- linear_act
def _linear_ratio(ops, B, Cin, Cout, relu):
    d = R.linear_inputs(B, Cin, Cout)
    y, bound = R.linear_act(d["x"], d["W"], d["sc"], d["sh"], relu)
    args = (dev(d["x"]), dev(d["W"]), dev(d["sc"]), dev(d["sh"]), relu)
    got = ops.linear_act(*args)
    assert torch.equal(got.view(torch.int32), ops.linear_act(*args).view(torch.int32))               # run to run
    ratio = np.abs(host(got).astype(np.float64) - y) / bound
    assert (ratio <= 1.0).all(), "linear_act B=%d Cin=%d Cout=%d: %.3g x bound" % (B, Cin, Cout, ratio.max())
    return float(ratio.max())


@pytest.mark.parametrize("Cin", R.LINEAR_CIN)
def test_linear_act_within_its_derived_bound(Cin):
    """Every element within (chain + 16 + 2) 2^-24 (|scale| sum |x w| + |shift|) of float64 (small_ops_ref.linear_act), over every B and
    Cout edge (16 rows x 8 outputs per workgroup) at each Cin: the scalar load path (Cin % 4 != 0), one pass (Cin <= 1024), several, the
    raised LDS limit (Cin > 1792) and the largest admitted."""
    from sonet_hip import ops
    worst = max(_linear_ratio(ops, B, Cin, Cout, (B + Cout) % 2 == 0) for B in R.LINEAR_B for Cout in R.LINEAR_COUT)
    print("linear_act Cin=%d: worst error / bound = %.4f" % (Cin, worst))


def test_linear_act_nan_row_stays_in_its_row_and_4097_is_refused():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    for Cin in (5, 1024, 1793):
        d = R.linear_inputs(17, Cin, 9)
        d["x"][3, Cin // 2] = np.nan
        got = host(ops.linear_act(dev(d["x"]), dev(d["W"]), dev(d["sc"]), dev(d["sh"]), True))
        assert np.isnan(got[3]).all() and np.isnan(got).sum() == 9
    v = torch.ones(2, device=DEV)
    with pytest.raises(SonetHipError, match="4097"):
        ops.linear_act(torch.zeros(1, 4097, device=DEV), torch.zeros(2, 4097, device=DEV), v, v, False)
    with pytest.raises(SonetHipError, match="Cout x Cin"):
        ops.linear_act(torch.zeros(1, 8, device=DEV), torch.zeros(2, 12, device=DEV), v, v, False)
    with pytest.raises(SonetHipError, match="Cout|C = 2"):
        ops.linear_act(torch.zeros(1, 8, device=DEV), torch.zeros(2, 8, device=DEV), torch.ones(3, device=DEV), v, False)


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import small_ops_ref as R
from sonet_hip import ops
d = R.linear_inputs(17, 1793, 9)
y, bound = R.linear_act(d["x"], d["W"], d["sc"], d["sh"], True)
t = lambda a: torch.from_numpy(a).to("cuda:0")
got = ops.linear_act(t(d["x"]), t(d["W"]), t(d["sc"]), t(d["sh"]), True).cpu().numpy().astype(np.float64)   # the process's FIRST linear_act
print("RATIO %%.6f" %% float((np.abs(got - y) / bound).max()))
"""


def test_linear_act_first_wide_call_of_a_fresh_process():
    """The dynamic-LDS limit is raised once per process, at the first call with Cin > 1792: here that call is the process's first launch of
    the kernel at all (in the tests above narrower calls came first)."""
    src = _CHILD % (os.path.join(ROOT, "so-net_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "RATIO" in out, out[-2000:]
    ratio = float(out.split("RATIO")[1].split()[0])
    assert ratio <= 1.0, "first wide call: %.3g x bound" % ratio


# ---------------------------------------------------------------------------------------------- alignment
def _offset_view(t):
    """The same values as a contiguous view that starts 4 bytes (one element) into a fresh allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_operands_at_a_4_byte_offset_are_copied_by_the_wrappers_and_refused_by_the_c_entries():
    """linear_act (Cin % 4 == 0) and node_gather_lead (L % 4 == 0) read x, W resp. gidx, lead with 16-byte loads on a length test alone:
    the wrappers hand the kernels an aligned copy, the C entries refuse the misaligned pointer before any launch (docs/findings.md)."""
    from sonet_hip import _lib, ops
    from sonet_hip.ops import ptr
    d = R.linear_inputs(5, 64, 9)
    x, W, sc, sh = dev(d["x"]), dev(d["W"]), dev(d["sc"]), dev(d["sh"])
    want = ops.linear_act(x, W, sc, sh, True)
    assert torch.equal(ops.linear_act(_offset_view(x), W, sc, sh, True), want)
    assert torch.equal(ops.linear_act(x, _offset_view(W), sc, sh, True), want)
    lib = _lib.load()
    y = torch.empty(5, 9, device=DEV)
    assert lib.sonet_linear_act_f32(ptr(_offset_view(x)), ptr(W), ptr(sc), ptr(sh), 1, ptr(y), 5, 64, 9, None) == 1
    assert "misaligned" in _lib.last_error()
    e = R.fma_case_inputs(2, 9, 8, 64, 3, False)
    z, gidx, lead, wl, sc, sh = (dev(e[k]) for k in ("z", "ids", "lead", "wl", "sc", "sh"))
    want = ops.node_gather_lead_affine_act(z, gidx, lead, wl, sc, sh, True)
    assert torch.equal(ops.node_gather_lead_affine_act(z, _offset_view(gidx), lead, wl, sc, sh, True), want)
    assert torch.equal(ops.node_gather_lead_affine_act(z, gidx, _offset_view(lead), wl, sc, sh, True), want)
    out = torch.empty(2, 9, 8, device=DEV)
    st = lib.sonet_node_gather_lead_affine_act_f32(ptr(z), ptr(_offset_view(gidx)), ptr(lead), ptr(wl), ptr(sc), ptr(sh), 1, ptr(out),
                                                   2, 9, 8, 64, 3, None)
    assert st == 1 and "misaligned" in _lib.last_error()


def test_wrappers_refuse_wrong_dtypes_and_shapes():
    from sonet_hip import ops
    from sonet_hip._lib import SonetHipError
    f, I = torch.zeros(1, 3, 4, device=DEV), torch.zeros(1, 4, 2, dtype=torch.int64, device=DEV)
    i32 = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    bad = [lambda: ops.knn_gather(f, I.int()), lambda: ops.knn_gather(f.double(), I), lambda: ops.knn_gather(f, I[:, :3]),
           lambda: ops.knn_group(f, f, I.int(), True), lambda: ops.knn_prepare(f[:, :2].contiguous(), I, True),
           lambda: ops.lastdim_max(f.transpose(1, 2)), lambda: ops.lastdim_max(f.double()), lambda: ops.planes_max(f, 3),
           lambda: ops.som_mask(i32.long(), 4), lambda: ops.node_gather(f, i32.long()), lambda: ops.node_gather(f.half(), i32),
           lambda: ops.knn_gather_bwd(torch.zeros(1, 3, 4, 2, device=DEV), I, 5), lambda: ops.knn_gather_bwd(torch.zeros(1, 3, 4, 2, device=DEV).half(), I, 4),
           lambda: ops.node_gather_bwd(torch.zeros(1, 3, 7, device=DEV), i32, 4), lambda: ops.knn_self(f, 17),
           lambda: ops.node_gather_lead_affine_act(f, i32, torch.zeros(1, 5, 8, device=DEV), torch.zeros(3, 5, device=DEV), torch.ones(3, device=DEV), torch.ones(3, device=DEV), True)]
    for n, call in enumerate(bad):
        with pytest.raises(SonetHipError):
            call()
            pytest.fail("call %d went through" % n)


# ---------------------------------------------------------------------------------------------- FusedAdam
def test_fused_adam_bits_over_five_steps():
    """Parameters and both moments bit-equal to the restatement after EVERY step: sizes around the 256-thread stride and the 4096-element
    chunk, one tensor that skips a step (its own step count), an all-zero gradient (denominator eps), g = 1e20, g = 1e30 (g^2 overflows: the
    parameter must not move) and one NaN gradient element (stays in its element).  torch.optim.Adam is NOT the reference here: it
    contracts into fmas (tests/test_gpu_optim.py keeps that comparison at its tolerance)."""
    from sonet_hip.optim import FusedAdam
    params, grads = R.adam_inputs()
    ref = R.adam_run(params, grads)
    ps = [torch.nn.Parameter(dev(p)) for p in params]
    opt = FusedAdam(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    steps = [0] * len(ps)
    for s, row in enumerate(grads):
        for t, (p, gr) in enumerate(zip(ps, row)):
            p.grad = None if gr is None else dev(gr)
            steps[t] += gr is not None
        opt.step()
        for t, p in enumerate(ps):
            st = opt.state[p]
            assert float(st["step"]) == steps[t]
            for name, got, want in (("p", p.detach(), ref[s][t][0]), ("exp_avg", st["exp_avg"], ref[s][t][1]),
                                    ("exp_avg_sq", st["exp_avg_sq"], ref[s][t][2])):
                bits(got, want, "step %d tensor %d (n = %d) %s" % (s + 1, t, R.ADAM_SIZES[t], name))
    (to, eo), (tn, en) = R.ADAM_OVERFLOW, R.ADAM_NAN
    assert float(ps[to].detach()[eo]) == float(params[to][eo])
    assert int(torch.isnan(ps[tn].detach()).sum()) == 1 and bool(torch.isnan(ps[tn].detach()[en]))
