"""Tensor-level wrappers over the C ABI: validate, allocate outputs with torch, launch on the
current stream.  Everything here requires CUDA (ROCm) tensors on an MI355X and raises otherwise
(mirroring the reference's CHECK_CUDA / CHECK_CONTIGUOUS -> RuntimeError convention,
models/index_max_ext/index_max.cpp:119-121)."""
import numpy as np
import torch

from . import _lib
from ._lib import SonetHipError, check, ptr, stream_ptr
import functools as _functools
import threading as _threading

# per-THREAD host state: the C side's BatchNorm rider is thread_local, so is the record of having armed it.  (The deferred side-stream
# joins are NOT: autograd runs backward nodes on its per-device worker thread and the end-of-pass callback on whichever thread finished
# the pass -- they share one locked table, and joining a stream somebody else registered is only a wait.)
_tls = _threading.local()
_join_lock = _threading.Lock()


def _consumes_rider(fn):
    """A statistics-producing call: whatever happens inside it -- a failed argument check included -- the BatchNorm rider armed for it
    (``bn_rider``) is disarmed when it returns, so that it can never ride on an unrelated later launch."""
    @_functools.wraps(fn)
    def wrapped(*a, **k):
        try:
            return fn(*a, **k)
        finally:
            _rider_done()
    return wrapped


# ---- optional per-launch timing with HIP events on the launch stream (used by bench.py) ----------
_TIMING = None


class kernel_timing:
    """``with ops.kernel_timing() as rec:`` records one (name, start, end) event pair per C-ABI launch
    on the current stream; ``rec.summary()`` (after a synchronize) gives per-name count and mean ms."""

    def __enter__(self):
        global _TIMING
        self.records = []
        _TIMING = self.records
        return self

    def __exit__(self, *exc):
        global _TIMING
        _TIMING = None
        return False

    def summary(self):
        out = {}
        for name, e0, e1 in self.records:
            d = out.setdefault(name, [0, 0.0])
            d[0] += 1
            d[1] += e0.elapsed_time(e1)
        return {k: dict(count=v[0], total_ms=v[1], mean_ms=v[1] / v[0]) for k, v in out.items()}


def _launch(dev, label, fn, *args, what=None):
    """One C-ABI launch: ``fn(*args, stream)`` on the current stream of ``dev``, its status checked (``what``: the name the error message
    carries, by default the entry point's own).  Under ``kernel_timing`` an event pair goes around it under ``label`` (None: never timed).
    The device is exchanged inline -- no context-manager objects on a path that runs a hundred times per training step."""
    prev = torch.cuda._exchange_device(dev.index if dev.index is not None else -1)
    try:
        if _TIMING is None or label is None:
            check(fn(*args, stream_ptr()), what or fn.__name__)
            return
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        try:
            check(fn(*args, stream_ptr()), what or fn.__name__)
        finally:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _TIMING.append((label, e0, e1))
    finally:
        torch.cuda._maybe_exchange_device(prev)


def _chk(t, name, dtype=None, dim=None):
    if not isinstance(t, torch.Tensor):
        raise SonetHipError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise SonetHipError("%s must be a CUDA tensor/variable" % name)          # CHECK_CUDA
    if not t.is_contiguous():
        raise SonetHipError("%s must be contiguous" % name)                      # CHECK_CONTIGUOUS
    if dtype is not None and t.dtype != dtype:
        raise SonetHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if dim is not None and t.dim() != dim:
        raise SonetHipError("%s must be %d-D, got shape %s" % (name, dim, tuple(t.shape)))


def _chk_cvec(C, dim=None, **vecs):
    """Per-channel operands (the coefficients of the BatchNorm / ReLU passes, the scale / shift / bias of a layer): the kernels index them
    by channel with no length of their own, so each must be a contiguous float32 tensor of exactly C elements -- ``dim``-D where the
    wrapper has always asked for that (attribute checks only: no launch, no sync)."""
    for name, t in vecs.items():
        _chk(t, name, torch.float32, dim)
        if t.numel() != C:
            raise SonetHipError("%s must hold C = %d elements, got %d" % (name, C, t.numel()))


def _chk_member(t, name, dtype, shape):
    """A tensor that a kernel indexes on the strength of the launch sizes alone (the members of a sorted grouping, a packed weight stream):
    dtype, shape and contiguity must be exactly what the kernel reads -- an int64 or strided id tensor would be read as int32 words.
    Attribute checks only (no launch, no sync); the device is checked with the other operands (``_same_device``)."""
    if not isinstance(t, torch.Tensor):
        raise SonetHipError("%s must be a torch.Tensor" % name)
    if t.dtype != dtype:
        raise SonetHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise SonetHipError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise SonetHipError("%s must be contiguous" % name)


def _chk_sort_group(sg, M):
    """The members of a ``som_sort_group`` result that the pooled first PointNet reads unchecked: int32, contiguous, B x L / B / B x M."""
    x = sg["x_aug_sorted"]
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise SonetHipError("x_aug_sorted must be a 3-D torch.Tensor")
    B, _, L = x.shape
    for name, shape in (("ids_sorted", (B, L)), ("pos0", (B,)), ("node_off", (B, int(M))), ("count", (B, int(M)))):
        _chk_member(sg[name], name, torch.int32, shape)


def _aligned16(t):
    """``t`` itself when its first element sits on a 16-byte boundary, else a fresh copy (allocations are aligned far beyond 16 bytes).  For
    the operands a kernel reads with 16-byte loads on the strength of a LENGTH test alone (linear_act: x and W when Cin % 4 == 0;
    node_gather_lead: gidx and lead when L % 4 == 0): a contiguous view such as ``buf[1:1 + n]`` passes every contiguity check at a 4-byte
    offset."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _chk_f32_or_bf16(t, name):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise SonetHipError("%s must be float32 or bfloat16, got %s" % (name, t.dtype))


def _same_device(*ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t is not None and t.device != dev:
            raise SonetHipError("tensors are on different devices: %s vs %s" % (dev, t.device))
    _lib.require_device(dev)
    return dev


def _by_dtype(lib, stem, t):
    """The f32 or bf16 entry point of a pair: ``lib.<stem>_f32`` / ``lib.<stem>_bf16`` by the storage of ``t``."""
    return getattr(lib, stem + ("_bf16" if t.dtype == torch.bfloat16 else "_f32"))


def _ws(size, dev, *dims):
    """The byte workspace of a launch on ``dev``: ``size`` bytes, or what the library's size query ``size(*dims)`` asks for."""
    return torch.empty((size(*dims) if callable(size) else size,), dtype=torch.uint8, device=dev)


def _idx_val(B, C, K, dev):
    """The (arg-max position i32, value f32) outputs of a pooled call, B x C x K each."""
    return torch.empty((B, C, int(K)), dtype=torch.int32, device=dev), torch.empty((B, C, int(K)), dtype=torch.float32, device=dev)


def _layer_inputs(x1, x2, dtype, L=None):
    """-> (B, C1, C2, L) of a layer call on x1 B x C1 x L (checked by the caller) and, when given, x2 B x C2 x L: a contiguous CUDA tensor of
    ``dtype`` (None: ``P16`` planes, which carry their own sizes).  L: the column count x2 is held to when x1 is gathered (``gidx``)."""
    B, C1, L1 = x1.shape
    L = L1 if L is None else L
    C2 = 0
    if x2 is not None:
        if dtype is not None:
            _chk(x2, "x2", dtype, 3)
        if x2.shape[0] != B or x2.shape[2] != L:
            raise SonetHipError("x2 must be B x C2 x L")
        C2 = x2.shape[1]
    return B, C1, C2, L


# kind of weight pack -> (tensor dtype that marks the flavour, size query, bytes per unit of the query's result)
_PACKS = {"f32": (torch.float32, "sonet_pointmlp_pack_size", 4), "x3": (torch.uint8, "sonet_pointmlp_x3_pack_size", 1),
          "h3": (torch.int8, "sonet_pointmlp_x3_pack_size", 1), "bf16": (torch.int16, "sonet_pointmlp_bf16_pack_size", 1),
          "h3p": (torch.int32, "sonet_pointmlp_h3p_pack_size", 1), "upconv": (torch.int32, "sonet_upconv3x3_pack_size", 1),
          "upconv-dgrad": (torch.int32, "sonet_upconv3x3_dgrad_pack_size", 1)}


def _pack_bytes(lib, kind, Cin, Cout):
    _, query, unit = _PACKS[kind]
    return getattr(lib, query)(Cin, Cout) * unit


def _pack_empty(lib, kind, Cin, Cout, dev):
    """An uninitialised pack of ``kind`` for a Cout x Cin weight."""
    dtype = _PACKS[kind][0]
    return torch.empty((_pack_bytes(lib, kind, Cin, Cout) // dtype.itemsize,), dtype=dtype, device=dev)


def _chk_pack(lib, wp, kind, Cin, Cout, say=None):
    """``wp`` (its dtype already told the caller the kind) has the length of a ``kind`` pack for Cin x Cout, compared in bytes.
    say: None -> the short message, "elements" / "bytes" -> the message with both sizes in that unit."""
    want, item = _pack_bytes(lib, kind, Cin, Cout), _PACKS[kind][0].itemsize
    if wp.numel() * item != want:
        if say is None:
            raise SonetHipError("packed weight does not match Cin=%d Cout=%d" % (Cin, Cout))
        unit = item if say == "elements" else 1
        raise SonetHipError("packed weight has %d %s, expected %d for Cin=%d Cout=%d" % (wp.numel() * item // unit, say, want // unit, Cin, Cout))


def _chk_index(index, B, Np, row_max=None):
    """The node ids of an ``index_max*`` call (int32, checked by the caller) are B x N'; row_max, when given, is a 2-D int32 tensor."""
    if tuple(index.shape) != (B, Np):
        raise SonetHipError("index must be B x N' = %s, got %s" % ((B, Np), tuple(index.shape)))
    if row_max is not None:
        _chk(row_max, "row_max", torch.int32, 2)


# ------------------------------------------------------------------------------------------ index_max
def index_max(data, index, K):
    """data BxCxN' f32|bf16, index BxN' i32 -> BxCxK i32 (include/sonet_hip.h: sonet_index_max_*)."""
    _chk(data, "data", dim=3)
    _chk(index, "index", torch.int32, 2)
    _chk_f32_or_bf16(data, "data")
    B, C, Np = data.shape
    _chk_index(index, B, Np)
    dev = _same_device(data, index)
    out = torch.empty((B, C, int(K)), dtype=torch.int32, device=dev)
    if out.numel() == 0 or Np == 0:
        return out.zero_()
    _launch(dev, "index_max", _by_dtype(_lib.load(), "sonet_index_max", data), ptr(data), ptr(index), ptr(out), B, C, Np, int(K), what="sonet_index_max")
    return out


def index_max_gather(data, index, K, row_max=None):
    """index_max + the masked gather of models/networks.py:185 in one pass -> (idx i32, val f32) BxCxK."""
    _chk(data, "data", dim=3)
    _chk_f32_or_bf16(data, "data")
    _chk(index, "index", torch.int32, 2)
    B, C, Np = data.shape
    _chk_index(index, B, Np, row_max)
    dev = _same_device(data, index, row_max)
    idx, val = _idx_val(B, C, K, dev)
    fn = _by_dtype(_lib.load(), "sonet_index_max_gather", data)
    _launch(dev, "index_max_gather" if data.dtype == torch.float32 else "index_max_gather_bf16", fn, ptr(data), ptr(index), ptr(row_max), ptr(idx), ptr(val), B,
            C, Np, int(K), what="sonet_index_max_gather")
    return idx, val


def pointmlp_bf16_pool_ok(x1, x2, Cout, M):
    """The shapes ``pointmlp_bf16_pool`` takes (the rest raise SONET_ERR_UNSUPPORTED): bf16 CUDA inputs, even L, (C1 + C2) % 64 == 0,
    C1 % 16 == 0 with a second input, Cout % 32 == 0, M <= 255, and the LDS budget of a (cloud, slab) workgroup."""
    if not (POOLED_TRAIN_EPILOGUE and x1.is_cuda and x1.dtype == torch.bfloat16 and (x2 is None or x2.dtype == torch.bfloat16)):
        return False
    B, C1, L = x1.shape
    C2 = x2.shape[1] if x2 is not None else 0
    if L % 2 or L > 65534 or (C1 + C2) % 64 or (C2 and C1 % 16) or Cout % 32 or not 0 < M <= 255 or B > 65535:
        return False
    KC, CT = (C1 + C2) // 16, Cout // 32
    for ns in range(1, CT + 1):                       # (the launcher's slab search: any slab whose W rows + bins + ids fit 158 KiB)
        if CT % ns:
            continue
        tps = CT // ns
        if tps % 2 and tps % 3:
            continue
        if tps * KC * 1024 + tps * 32 * 8 + tps * 32 * M * 8 + tps * 32 * 4 + ((L + 15) & ~15) <= 158 * 1024:
            return True
    return False


def pointmlp_bf16_pool(x1, wp, scale, shift, relu, Cout, ids, M, row_max=None, x2=None, xaff=None):
    """The bf16 layer and the per-node arg-max pool of its output in one launch (``sonet_pointmlp_bf16_pool``); the B x Cout x L output is
    never written.  -> (idx i32, val f32) B x Cout x M: exactly ``index_max_gather(pointmlp(...), ids, M, row_max)``.
    xaff = (s1, h1, relu1[, s2, h2, relu2]): x1 / x2 are RAW outputs of BatchNorm layers, normalised by the operand load."""
    _chk(x1, "x", torch.bfloat16, 3)
    B, C1, C2, L = _layer_inputs(x1, x2, torch.bfloat16)
    if wp.dtype != torch.int16:
        raise SonetHipError("pointmlp_bf16_pool: a bf16 pack")
    _chk(ids, "ids", torch.int32, 2)
    if tuple(ids.shape) != (B, L):
        raise SonetHipError("ids must be B x L")
    if row_max is not None:
        _chk(row_max, "row_max", torch.int32, 2)
    _chk_cvec(Cout, 1, scale=scale, shift=shift)
    dev = _same_device(x1, x2, wp, scale, shift, ids, row_max)
    lib = _lib.load()
    _chk_pack(lib, wp, "bf16", C1 + C2, Cout)
    idx, val = _idx_val(B, Cout, M, dev)
    args = (ptr(x1), C1, ptr(x2), C2, ptr(wp), ptr(scale), ptr(shift), int(bool(relu)), ptr(ids), ptr(row_max), ptr(idx), ptr(val), B, Cout, L, int(M))
    name = "pointmlpbf16_pool_%dx%d_L%d" % (C1 + C2, Cout, L)
    if xaff is not None:
        _launch(dev, name + "_xaff", lib.sonet_pointmlp_bf16_pool_xaff, *args, *_xaff_args(xaff, C1, C2, dev))
    else:
        _launch(dev, name, lib.sonet_pointmlp_bf16_pool, *args)
    return idx, val


def pointmlp_h3_segpool_ok(x1, x2, wp, Cout, M):
    """The shapes ``pointmlp_h3_segpool`` takes: f32 CUDA inputs, an h3 pack, Cout % 32 == 0, C1 % 16 == 0 with a second input."""
    if not (POOLED_TRAIN_EPILOGUE and H3_SEGPOOL and x1.is_cuda and x1.dtype == torch.float32 and (x2 is None or x2.dtype == torch.float32)
            and wp.dtype == torch.int8):
        return False
    return Cout % 32 == 0 and (x2 is None or x1.shape[1] % 16 == 0) and 0 < M <= 1024


def pointmlp_h3_segpool(x1, wp, scale, shift, relu, Cout, ids_sorted, pos0, M, row_max=None, x2=None, xaff=None):
    """The fp16-split layer and the per-node arg-max pool of its output in one pass over NODE-SORTED columns (``sonet_pointmlp_h3_segpool_f32``);
    the B x Cout x L output is never written.  ids_sorted B x L i32 (``som_sort_group``), pos0 B i32 = sorted position of original column 0.
    -> (idx i32, val f32) B x Cout x M: ``index_max_gather(pointmlp(...), ids_sorted, M, row_max)`` with pos0[b] (and the value there) in
    place of position 0 for bins nothing beat and for masked nodes."""
    _chk(x1, "x", torch.float32, 3)
    B, C1, C2, L = _layer_inputs(x1, x2, torch.float32)
    if wp.dtype != torch.int8:
        raise SonetHipError("pointmlp_h3_segpool: an h3 pack")
    _chk(ids_sorted, "ids_sorted", torch.int32, 2)
    _chk(pos0, "pos0", torch.int32, 1)
    if tuple(ids_sorted.shape) != (B, L) or pos0.shape[0] != B:
        raise SonetHipError("ids_sorted must be B x L and pos0 B")
    if row_max is not None:
        _chk(row_max, "row_max", torch.int32, 2)
    _chk_cvec(Cout, 1, scale=scale, shift=shift)
    dev = _same_device(x1, x2, wp, scale, shift, ids_sorted, pos0, row_max)
    lib = _lib.load()
    _chk_pack(lib, wp, "h3", C1 + C2, Cout)
    idx, val = _idx_val(B, Cout, M, dev)
    ws = _ws(lib.sonet_pointmlp_h3_segpool_ws_size, dev, B, Cout, int(M))
    name = "pointmlph3_segpool_%dx%d_L%d" % (C1 + C2, Cout, L)
    _range_arm(name)
    xa = _xaff_args(xaff, C1, C2, dev) if xaff is not None else (None, None, None, None, 0)
    _launch(dev, name + ("_xaff" if xaff is not None else ""), lib.sonet_pointmlp_h3_segpool_f32, ptr(x1), C1, ptr(x2), C2, ptr(wp), ptr(scale), ptr(shift),
            int(bool(relu)), ptr(ids_sorted), ptr(pos0), ptr(row_max), int(M), ptr(ws), ptr(idx), ptr(val), B, Cout, L, *xa)
    return idx, val


def index_max_gather_p16(planes, index, K, row_max=None):
    """index_max_gather on an activation that exists only as P16 planes (``P16``): values (hi + mid) / 32, the 22-bit values the next
    layer multiplies -> (idx i32, val f32) B x C x K."""
    _chk(index, "index", torch.int32, 2)
    B, C, Np = planes.shape
    _chk_index(index, B, Np, row_max)
    dev = _same_device(planes.data, index, row_max)
    idx, val = _idx_val(B, C, K, dev)
    _launch(dev, "index_max_gather_p16", _lib.load().sonet_index_max_gather_p16, ptr(planes.data), ptr(index), ptr(row_max), ptr(idx), ptr(val), B, C, Np,
            int(K))
    return idx, val


# ------------------------------------------------------------------------------------------ SOM
class SomAssignment:
    """Result of som_assign: node ids per point copy plus the per-node count / sum state."""
    __slots__ = ("B", "N", "M", "k", "min_idx_i32", "min_idx_i64", "count", "sum_ws")


def som_assign(x, node, k, want_i64=False):
    _chk(x, "x", torch.float32, 3)
    _chk(node, "node", torch.float32, 3)
    B, D, N = x.shape
    if D != 3 or node.shape[0] != B or node.shape[1] != 3:
        raise SonetHipError("x must be B x 3 x N and node B x 3 x M, got %s and %s" % (tuple(x.shape), tuple(node.shape)))
    M = node.shape[2]
    dev = _same_device(x, node)
    r = SomAssignment()
    r.B, r.N, r.M, r.k = B, N, M, int(k)
    r.min_idx_i32 = torch.empty((B, r.k * N), dtype=torch.int32, device=dev)
    r.min_idx_i64 = torch.empty((B, r.k * N), dtype=torch.int64, device=dev) if want_i64 else None
    # one allocation, sums first (8-byte aligned), counts right behind: the library clears both with a single memset
    ws = _ws(B * 3 * M * 8 + B * M * 4, dev)
    r.sum_ws = ws[:B * 3 * M * 8].view(torch.float64).view(B, 3, M)
    r.count = ws[B * 3 * M * 8:].view(torch.int32).view(B, M)
    _launch(dev, "som_assign", _lib.load().sonet_som_assign_f32, ptr(x), ptr(node), B, N, M, r.k, ptr(r.min_idx_i32), ptr(r.min_idx_i64), ptr(r.count),
            ptr(r.sum_ws))
    return r


SOM_TRAIN_MAX_NODES = 1024             # include/sonet_hip.h SONET_SOM_TRAIN_MAX_NODES / _MAX_POINTS
SOM_TRAIN_MAX_POINTS = 1 << 28


def som_train_supported(N, M):
    """Does ``som_train`` take clouds of N points and M nodes?"""
    return 1 <= N <= SOM_TRAIN_MAX_POINTS and 1 <= M <= SOM_TRAIN_MAX_NODES


def som_train(x, node0, w, lr):
    """T SOM iterations (util/som.py:295-352) for every cloud in ONE launch (``sonet_som_train_f32``).

    x B x 3 x N f32; node0 B x 3 x M (per cloud) or 3 x M (shared) f32; w T x M x M (or T x M x rows x cols) f32, w[t, i, j] = weight of
    node j around centre node i; lr T f32 -> nodes B x 3 x M f32.  Bit-identical from run to run and independent of the batch."""
    _chk(x, "x", torch.float32, 3)
    _chk(node0, "node0", torch.float32)
    _chk(w, "w", torch.float32)
    _chk(lr, "lr", torch.float32, 1)
    B, D, N = x.shape
    shared = node0.dim() == 2
    if D != 3 or node0.dim() not in (2, 3) or node0.shape[-2] != 3 or (not shared and node0.shape[0] != B):
        raise SonetHipError("x must be B x 3 x N and node0 B x 3 x M or 3 x M, got %s and %s" % (tuple(x.shape), tuple(node0.shape)))
    M = node0.shape[-1]
    T = lr.shape[0]
    if w.dim() < 3 or w.shape[0] != T or w.shape[1] != M or w.numel() != T * M * M:
        raise SonetHipError("w must be T x M x M (or T x M x rows x cols) with T = len(lr) = %d, M = %d, got %s" % (T, M, tuple(w.shape)))
    dev = _same_device(x, node0, w, lr)
    out = torch.empty((B, 3, M), dtype=torch.float32, device=dev)
    _launch(dev, "som_train", _lib.load().sonet_som_train_f32, ptr(x), ptr(node0), int(shared), ptr(w) if T else None, ptr(lr) if T else None, T, B, N, M,
            ptr(out))
    return out


def som_group(x, sn, a, want_centers=False, want_decentered=False, want_augmented=False):
    """-> dict(som_node Bx3xM, row_max BxM i32, [centers], [x_decentered] Bx3xkN, [x_augmented] Bx6xkN)."""
    _chk(x, "x", torch.float32, 3)
    if sn is not None:
        _chk(sn, "sn", torch.float32, 3)
        if sn.shape != x.shape:
            raise SonetHipError("sn must have the shape of x")
    dev = _same_device(x, sn, a.min_idx_i32)
    B, N, M, k = a.B, a.N, a.M, a.k
    kN = k * N
    out = dict(som_node=torch.empty((B, 3, M), dtype=torch.float32, device=dev),
               row_max=torch.empty((B, M), dtype=torch.int32, device=dev))
    out["centers"] = torch.empty((B, 3, kN), dtype=torch.float32, device=dev) if want_centers else None
    out["x_decentered"] = torch.empty((B, 3, kN), dtype=torch.float32, device=dev) if want_decentered else None
    out["x_augmented"] = torch.empty((B, 6, kN), dtype=torch.float32, device=dev) if want_augmented else None
    _launch(dev, "som_group", _lib.load().sonet_som_group_f32, ptr(x), ptr(sn), ptr(a.min_idx_i32), ptr(a.count), ptr(a.sum_ws), B, N, M, k,
            ptr(out["som_node"]), ptr(out["row_max"]), ptr(out["centers"]), ptr(out["x_decentered"]), ptr(out["x_augmented"]))
    return out


def som_sort_group(x, sn, a):
    """Node-sorted grouping for the fused no-grad path -> dict(som_node, row_max, x_aug_sorted Bx6xkN, ids_sorted BxkN, pos0 B)."""
    _chk(x, "x", torch.float32, 3)
    _chk(sn, "sn", torch.float32, 3)
    dev = _same_device(x, sn, a.min_idx_i32)
    B, N, M, k = a.B, a.N, a.M, a.k
    kN = k * N
    out = dict(som_node=torch.empty((B, 3, M), dtype=torch.float32, device=dev),
               row_max=torch.empty((B, M), dtype=torch.int32, device=dev),
               x_aug_sorted=torch.empty((B, 6, kN), dtype=torch.float32, device=dev),
               ids_sorted=torch.empty((B, kN), dtype=torch.int32, device=dev),
               pos0=torch.empty((B,), dtype=torch.int32, device=dev),
               node_off=torch.empty((B, M), dtype=torch.int32, device=dev), count=a.count)
    cursor = torch.empty((B, M), dtype=torch.int32, device=dev)
    _launch(dev, "som_sort_group", _lib.load().sonet_som_sort_group_f32, ptr(x), ptr(sn), ptr(a.min_idx_i32), ptr(a.count), ptr(a.sum_ws), B, N, M, k,
            ptr(out["som_node"]), ptr(out["row_max"]), ptr(out["x_aug_sorted"]), ptr(out["ids_sorted"]), ptr(out["pos0"]), ptr(out["node_off"]), ptr(cursor))
    return out


def som_assign_sort(x, sn, node, k, want_i64=False, knn=None, deterministic=False):
    """som_assign + som_sort_group of the no-grad pooled path in two launches (``sonet_som_assign_sort_f32``): -> (SomAssignment,
    dict(som_node, row_max, x_aug_sorted, ids_sorted, pos0, node_off, count)).  Node ids / counts bit-identical to the separate calls.
    knn = (knn_I B x M x KI int64, K, center_avg): the second launch also does ``knn_stage_prepare`` on the cluster means
    (``sonet_som_assign_sort_knn_f32``); its result is the dict's "knn_prep".
    deterministic (without knn): the order INSIDE a node does not depend on the arrival order of atomics (``sonet_som_assign_sort_det_f32``):
    the same sorted copy in every run."""
    _chk(x, "x", torch.float32, 3)
    _chk(sn, "sn", torch.float32, 3)
    _chk(node, "node", torch.float32, 3)
    B, D, N = x.shape
    if D != 3 or node.shape[0] != B or node.shape[1] != 3 or sn.shape != x.shape:
        raise SonetHipError("x, sn must be B x 3 x N and node B x 3 x M, got %s, %s and %s" % (tuple(x.shape), tuple(sn.shape), tuple(node.shape)))
    M = node.shape[2]
    dev = _same_device(x, sn, node)
    k = int(k)
    kN = k * N
    lib = _lib.load()
    r = SomAssignment()
    r.B, r.N, r.M, r.k = B, N, M, k
    r.min_idx_i32 = torch.empty((B, kN), dtype=torch.int32, device=dev)
    r.min_idx_i64 = torch.empty((B, kN), dtype=torch.int64, device=dev) if want_i64 else None
    r.sum_ws = torch.empty((B, 3, M), dtype=torch.float64, device=dev)
    r.count = torch.empty((B, M), dtype=torch.int32, device=dev)
    out = dict(som_node=torch.empty((B, 3, M), dtype=torch.float32, device=dev),
               row_max=torch.empty((B, M), dtype=torch.int32, device=dev),
               x_aug_sorted=torch.empty((B, 6, kN), dtype=torch.float32, device=dev),
               ids_sorted=torch.empty((B, kN), dtype=torch.int32, device=dev),
               pos0=torch.empty((B,), dtype=torch.int32, device=dev),
               node_off=torch.empty((B, M), dtype=torch.int32, device=dev), count=r.count)
    ws = _ws(lib.sonet_som_assign_sort_ws_size, dev, B, N, M, k)
    if knn is not None:
        knn_I, K, avg = knn
        _chk(knn_I, "knn_I", torch.int64, 3)
        KI = knn_I.shape[2]
        if tuple(knn_I.shape[:2]) != (B, M) or KI < K or not 1 <= K <= 128:
            raise SonetHipError("som_assign_sort: knn_I B x M x (>= K), 1 <= K <= 128")
        _same_device(x, knn_I)
        Lm = node_stage_columns(B, M)
        Lp = int(lib.sonet_knn_stage_columns(B, M, int(K)))
        prep = dict(center=torch.empty((B, 3, M), dtype=torch.float32, device=dev), center_p16=p16_flat(3, Lm, B * M, dev),
                    rec=torch.empty((Lp, 4), dtype=torch.int32, device=dev), B=B, M=M, K=int(K), G=min(16, 128 // int(K)), Lp=Lp)
        _launch(dev, "som_assign_sort", lib.sonet_som_assign_sort_knn_f32, ptr(x), ptr(sn), ptr(node), B, N, M, k, ptr(r.min_idx_i32), ptr(r.min_idx_i64),
                ptr(r.count), ptr(r.sum_ws), ptr(out["som_node"]), ptr(out["row_max"]), ptr(out["x_aug_sorted"]), ptr(out["ids_sorted"]), ptr(out["pos0"]),
                ptr(out["node_off"]), ptr(ws), ptr(knn_I), KI, int(K), int(bool(avg)), ptr(prep["center"]), ptr(prep["center_p16"].data), ptr(prep["rec"]))
        out["knn_prep"] = prep
        return r, out
    fn = lib.sonet_som_assign_sort_det_f32 if deterministic else lib.sonet_som_assign_sort_f32
    _launch(dev, "som_assign_sort_det" if deterministic else "som_assign_sort", fn, ptr(x), ptr(sn), ptr(node), B, N, M, k, ptr(r.min_idx_i32),
            ptr(r.min_idx_i64), ptr(r.count), ptr(r.sum_ws), ptr(out["som_node"]), ptr(out["row_max"]), ptr(out["x_aug_sorted"]), ptr(out["ids_sorted"]),
            ptr(out["pos0"]), ptr(out["node_off"]), ptr(ws), what="sonet_som_assign_sort_f32")
    return r, out


def som_mask(min_idx_i32, M):
    _chk(min_idx_i32, "min_idx", torch.int32, 2)
    dev = _same_device(min_idx_i32)
    B, kN = min_idx_i32.shape
    mask = torch.empty((B, kN, int(M)), dtype=torch.int32, device=dev)
    _launch(dev, "som_mask", _lib.load().sonet_som_mask_i32, ptr(min_idx_i32), ptr(mask), B, kN, int(M))
    return mask


def node_gather(feat, min_idx_i32):
    """feat B x C x M f32, min_idx B x kN i32 -> B x C x kN (models/segmenter.py:90-98)."""
    _chk(feat, "feat", torch.float32, 3)
    _chk(min_idx_i32, "min_idx", torch.int32, 2)
    dev = _same_device(feat, min_idx_i32)
    B, C, M = feat.shape
    kN = min_idx_i32.shape[1]
    out = torch.empty((B, C, kN), dtype=torch.float32, device=dev)
    _launch(dev, "node_gather", _lib.load().sonet_node_gather_f32, ptr(feat), ptr(min_idx_i32), ptr(out), B, C, M, kN)
    return out


def node_gather_bwd(g, min_idx_i32, M):
    """Backward of ``node_gather``: g B x C x kN (f32 / bf16), min_idx B x kN i32 -> B x C x M f32, every node's columns summed in
    ascending column order (bitwise reproducible: torch.gather's backward scatter-adds atomically)."""
    if g.dtype not in (torch.float32, torch.bfloat16):
        raise SonetHipError("node_gather_bwd: f32 or bf16 gradient")
    _chk(g, "g", g.dtype, 3)
    _chk(min_idx_i32, "min_idx", torch.int32, 2)
    dev = _same_device(g, min_idx_i32)
    B, C, L = g.shape
    if tuple(min_idx_i32.shape) != (B, L):
        raise SonetHipError("node_gather_bwd: min_idx must be B x kN with the kN of the gradient")
    lib = _lib.load()
    gx = torch.empty((B, C, M), dtype=torch.float32, device=dev)
    ws = _ws(lib.sonet_node_gather_bwd_ws_size, dev, B, M, L)
    fn = _by_dtype(lib, "sonet_node_gather_bwd", g)
    _launch(dev, "node_gather_bwd", fn, ptr(g), ptr(min_idx_i32), ptr(gx), ptr(ws), B, C, M, L, what="sonet_node_gather_bwd")
    return gx


class _NodeGather(torch.autograd.Function):
    """feat[:, :, min_idx] (models/segmenter.py:96-98) with a fixed-order backward (``node_gather_bwd``)."""

    @staticmethod
    def forward(ctx, feat, min_idx_i32):
        ctx.save_for_backward(min_idx_i32)
        ctx.M, ctx.dtype = feat.shape[2], feat.dtype
        if feat.dtype == torch.float32:
            return node_gather(feat.contiguous(), min_idx_i32)
        # (bf16 node-level maps: the gather moves values, torch.gather's forward is exact)
        return torch.gather(feat, 2, min_idx_i32.long().unsqueeze(1).expand(-1, feat.shape[1], -1))

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        g = g.contiguous()
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        return node_gather_bwd(g, ids, ctx.M).to(ctx.dtype), None


def node_gather_autograd(feat, min_idx_i32):
    """Differentiable ``node_gather``: B x C x M, B x kN i32 -> B x C x kN; its backward sums every node's copies in a fixed order."""
    return _NodeGather.apply(feat, min_idx_i32.contiguous())


def node_add_affine_act_(t, z, min_idx_i32, scale, shift, relu):
    """t B x C x L <- act((t + z[:, :, min_idx]) * scale + shift) in place; z B x C x M."""
    _chk(t, "t", torch.float32, 3)
    _chk(z, "z", torch.float32, 3)
    _chk(min_idx_i32, "min_idx", torch.int32, 2)
    dev = _same_device(t, z, min_idx_i32, scale, shift)
    B, C, L = t.shape
    if z.shape[0] != B or z.shape[1] != C or min_idx_i32.shape != (B, L):
        raise SonetHipError("z must be B x C x M and min_idx B x L")
    _chk_cvec(C, scale=scale, shift=shift)
    _launch(dev, "node_add_affine_act", _lib.load().sonet_node_add_affine_act_f32, ptr(t), ptr(z), ptr(min_idx_i32), ptr(scale), ptr(shift), int(bool(relu)), B,
            C, L, z.shape[2])
    return t


def _xaff3(xaff, C, who, ref):
    """xaff = (scale, shift, relu) of ONE operand with C channels -> the C ABI's three arguments; ``who``: the start of the length message."""
    xs, xh, xr = xaff
    _chk(xs, "xaff scale", torch.float32, 1)
    _chk(xh, "xaff shift", torch.float32, 1)
    if xs.numel() != C or xh.numel() != C:
        raise SonetHipError("%s = %d coefficients" % (who, C))
    _same_device(ref, xs, xh)
    return ptr(xs), ptr(xh), int(bool(xr))


def _wgrad(g, x, xaff, dtype, who, ws_size, fn, fn_xaff, label):
    """The dense weight gradient sum_b g[b] . x[b]^T of ``wgrad_x3`` / ``wgrad_bf16`` (``label``: a format with a %s for the sizes)."""
    _chk(g, "g", dtype, 3)
    _chk(x, "x", dtype, 3)
    dev = _same_device(g, x)
    B, Cout, L = g.shape
    if x.shape[0] != B or x.shape[2] != L:
        raise SonetHipError("%s: g B x Cout x L and x B x Cin x L" % who)
    Cin = x.shape[1]
    dw = torch.empty((Cout, Cin), dtype=torch.float32, device=dev)
    if g.numel() == 0 or x.numel() == 0:
        return dw.zero_()
    args = (ptr(g), ptr(x), ptr(dw), ptr(_ws(ws_size, dev, B, Cout, Cin, L)), B, Cout, Cin, L)
    if xaff is not None:
        _launch(dev, label[1] % (Cout, Cin, L), fn_xaff, *args, *_xaff3(xaff, Cin, who + ": xaff needs Cin", x))
    else:
        _launch(dev, label[0] % (Cout, Cin, L), fn, *args)
    return dw


def wgrad_x3(g, x, xaff=None):
    """sum_b g[b] . x[b]^T: g B x Cout x L, x B x Cin x L (f32) -> Cout x Cin f32, bf16 x 3 split of both operands on the matrix cores.
    xaff = (scale, shift, relu): x holds the RAW output of a BatchNorm layer, the operand split applies act(x * scale[c] + shift[c]) first."""
    lib = _lib.load()
    return _wgrad(g, x, xaff, torch.float32, "wgrad_x3", lib.sonet_wgrad_x3_ws_size, lib.sonet_wgrad_x3_f32, lib.sonet_wgrad_x3_xaff_f32,
                  ("wgradx3_%dx%d_L%d", "wgradx3_xaff_%dx%d_L%d"))


def wgrad_bf16_xaff_ok(B, Cout, Cin, L):
    """Shapes ``wgrad_bf16(..., xaff=...)`` takes: the streaming generation of the kernel (16-byte aligned 8-column groups, a long reduction)."""
    return L % 8 == 0 and B * ((L + 63) // 64) >= 2048


def wgrad_bf16(g, x, xaff=None):
    """sum_b g[b] . x[b]^T for bfloat16 operands: g B x Cout x L, x B x Cin x L -> Cout x Cin f32 (one bf16 MFMA per product, f32
    accumulation and partials, fixed-order reduction: ``sonet_wgrad_bf16``).  xaff = (scale, shift, relu): x holds the RAW output of a
    BatchNorm layer, normalised by the operand path (``sonet_wgrad_bf16_xaff``; ``wgrad_bf16_xaff_ok`` shapes)."""
    lib = _lib.load()
    return _wgrad(g, x, xaff, torch.bfloat16, "wgrad_bf16", lib.sonet_wgrad_bf16_ws_size, lib.sonet_wgrad_bf16, lib.sonet_wgrad_bf16_xaff,
                  ("wgradbf16_%dx%d_L%d", "wgradbf16_%dx%d_L%d_xaff"))


def node_gather_lead_affine_act(z, gidx, lead, wl, scale, shift, relu):
    """act((z[:, :, gidx] + wl . lead) * scale + shift): z B x C x M (the layer on the M node features), gidx B x L i32 (out of
    range -> 0), lead B x NL x L (NL <= 4 per-column channels), wl C x NL.  -> B x C x L f32."""
    _chk(z, "z", dim=3)
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise SonetHipError("node_gather_lead_affine_act: z float32 or bfloat16")
    _chk(gidx, "gidx", torch.int32, 2)
    _chk(lead, "lead", torch.float32, 3)
    _chk(wl, "wl", torch.float32, 2)
    dev = _same_device(z, gidx, lead, wl, scale, shift)
    B, C, M = z.shape
    L, NL = gidx.shape[1], lead.shape[1]
    if gidx.shape[0] != B or lead.shape[0] != B or lead.shape[2] != L or tuple(wl.shape) != (C, NL) or scale.numel() != C or shift.numel() != C:
        raise SonetHipError("node_gather_lead_affine_act: z B x C x M, gidx B x L, lead B x NL x L, wl C x NL, scale / shift C")
    _chk_cvec(C, scale=scale, shift=shift)
    gidx, lead = _aligned16(gidx), _aligned16(lead)              # (16-byte loads when L % 4 == 0; the C entry refuses misaligned ones)
    out = torch.empty((B, C, L), dtype=z.dtype, device=dev)
    lib = _lib.load()
    fn = _by_dtype(lib, "sonet_node_gather_lead_affine_act", z)
    _launch(dev, "node_gather_lead%s_%dx%d_L%d" % ("" if z.dtype == torch.float32 else "bf16", NL, C, L), fn, ptr(z), ptr(gidx), ptr(lead), ptr(wl), ptr(scale),
            ptr(shift), int(bool(relu)), ptr(out), B, C, L, M, NL, what="sonet_node_gather_lead_affine_act")
    return out


def knn_self(node, K):
    """node B x 3 x M f32 -> B x M x K i64: the K nearest nodes of every node (itself first)."""
    _chk(node, "node", torch.float32, 3)
    dev = _same_device(node)
    B, _, M = node.shape
    out = torch.empty((B, M, int(K)), dtype=torch.int64, device=dev)
    _launch(dev, "knn_self", _lib.load().sonet_knn_self_f32, ptr(node), ptr(out), B, M, int(K))
    return out


BATCH_SHAPENET, BATCH_TRAIN, BATCH_ROT_HORIZONTAL, BATCH_ROT_PERTURBATION, BATCH_TRANSLATION = 1, 2, 4, 8, 16   # SONET_BATCH_*
BATCH_DRAW_SCALARS = 8
BATCH_MAX_K = 16


def _i64(v):
    v = int(v) & (2 ** 64 - 1)                  # the 64-bit pattern, as the signed long long of the C entry
    return v - 2 ** 64 if v >= 2 ** 63 else v


def batch_draw_size(N, M):
    """float64 values in one slot's draw record (include/sonet_hip.h, sonet_assemble_batch_f32)."""
    return BATCH_DRAW_SCALARS + 6 * N + 3 * M


def assemble_batch(src, offsets, nodes_src, idx, N, K, flags, seed, step, replay_idx=None, replay_draws=None, want_draws=False,
                   sizes=None):
    """Subsample + augment B clouds of a device-resident dataset in one launch, then the node self-kNN (``sonet_assemble_batch_f32``).

    src 6 x P f32 (planar x, y, z, nx, ny, nz); offsets S+1 i64 (CSR); nodes_src S x M x 3 f32; idx B i64 -> dict(pc, sn B x 3 x N f32,
    node B x 3 x M f32, chosen B x N i64 (global source index), knn_I B x M x K i64, bad B i32 [, draws B x D f64]).
    replay_idx B x N i64 (local indices) / replay_draws B x D f64 replace the generator.  ``sizes`` (host: the S cloud sizes) makes idx
    and N <= n_s (modelnet / shrec) checked here before the launch; idx is then read back to the host when it lives on the device."""
    _chk(src, "src", torch.float32, 2)
    _chk(offsets, "offsets", torch.int64, 1)
    _chk(nodes_src, "nodes_src", torch.float32, 3)
    _chk(idx, "idx", torch.int64, 1)
    S, M = nodes_src.shape[0], nodes_src.shape[1]
    B, N, K, flags = idx.shape[0], int(N), int(K), int(flags)
    if src.shape[0] != 6 or nodes_src.shape[2] != 3 or offsets.shape[0] != S + 1:
        raise SonetHipError("src must be 6 x P, nodes_src S x M x 3 and offsets S+1, got %s, %s, %s"
                            % (tuple(src.shape), tuple(nodes_src.shape), tuple(offsets.shape)))
    if B < 1 or N < 1 or not 1 <= K <= min(M, BATCH_MAX_K):
        raise SonetHipError("need B >= 1, N >= 1 and 1 <= K <= min(M, %d), got B=%d N=%d K=%d M=%d" % (BATCH_MAX_K, B, N, K, M))
    if sizes is not None:
        ii, sizes = idx.cpu().numpy(), np.asarray(sizes)
        if ii.min() < 0 or ii.max() >= S:
            raise SonetHipError("idx out of range [0, %d): min %d max %d" % (S, ii.min(), ii.max()))
        smallest = int(sizes[ii].min())
        if not flags & BATCH_SHAPENET and smallest < N:
            raise SonetHipError("N=%d > n_s=%d points of a cloud in the batch (modelnet / shrec sample without replacement)" % (N, smallest))
    dev = _same_device(src, offsets, nodes_src, idx, replay_idx, replay_draws)
    D = batch_draw_size(N, M)
    if replay_idx is not None:
        _chk(replay_idx, "replay_idx", torch.int64)
        if tuple(replay_idx.shape) != (B, N):
            raise SonetHipError("replay_idx must be B x N = %s, got %s" % ((B, N), tuple(replay_idx.shape)))
    if replay_draws is not None:
        _chk(replay_draws, "replay_draws", torch.float64)
        if tuple(replay_draws.shape) != (B, D):
            raise SonetHipError("replay_draws must be B x D = %s, got %s" % ((B, D), tuple(replay_draws.shape)))
    f32 = dict(dtype=torch.float32, device=dev)
    r = dict(pc=torch.empty((B, 3, N), **f32), sn=torch.empty((B, 3, N), **f32), node=torch.empty((B, 3, M), **f32),
             chosen=torch.empty((B, N), dtype=torch.int64, device=dev), knn_I=torch.empty((B, M, K), dtype=torch.int64, device=dev),
             bad=torch.empty((B,), dtype=torch.int32, device=dev))
    if want_draws:
        r["draws"] = torch.zeros((B, D), dtype=torch.float64, device=dev)
    _launch(dev, "assemble_batch", _lib.load().sonet_assemble_batch_f32, ptr(src), src.shape[1], ptr(offsets), S, ptr(nodes_src), ptr(idx), B, N, M, K, flags,
            _i64(seed), _i64(step), ptr(replay_idx) if replay_idx is not None else None, ptr(replay_draws) if replay_draws is not None else None,
            ptr(r["draws"]) if want_draws else None, ptr(r["pc"]), ptr(r["sn"]), ptr(r["node"]), ptr(r["chosen"]), ptr(r["knn_I"]), ptr(r["bad"]))
    return r


def knn_group(coord, feat, knn_I, center_avg):
    """coord B x 3 x M, feat B x C x M, knn_I B x M x K i64 -> (center B x 3 x M, out B x (3+C) x M x K)."""
    _chk(coord, "coord", torch.float32, 3)
    _chk(feat, "feat", torch.float32, 3)
    _chk(knn_I, "knn_I", torch.int64, 3)
    dev = _same_device(coord, feat, knn_I)
    B, C, M = feat.shape
    K = knn_I.shape[2]
    center = torch.empty((B, 3, M), dtype=torch.float32, device=dev)
    out = torch.empty((B, 3 + C, M, K), dtype=torch.float32, device=dev)
    _launch(dev, "knn_group", _lib.load().sonet_knn_group_f32, ptr(coord), ptr(feat), ptr(knn_I), B, C, M, K, int(bool(center_avg)), ptr(center), ptr(out))
    return center, out


def lastdim_max(x):
    """max over the last (contiguous) axis, values only; NaN propagates like torch.amax."""
    if x.dtype == torch.bfloat16:                     # node-level tensors (B x C x M): widening is exact and cheap
        x = x.float()
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise SonetHipError("lastdim_max needs a contiguous float32 tensor")
    dev = _same_device(x)
    K = x.shape[-1]
    out = torch.empty(x.shape[:-1], dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    _launch(dev, "lastdim_max", _lib.load().sonet_lastdim_max_f32, ptr(x), ptr(out), out.numel(), K)
    return out


def knn_gather(x, knn_I):
    """x BxCxM f32, knn_I BxMxK i64 -> BxCxMxK (models/operations.py:38-54)."""
    _chk(x, "som_node", torch.float32, 3)
    _chk(knn_I, "som_node_knn_I", torch.int64, 3)
    B, C, M = x.shape
    if knn_I.shape[0] != B or knn_I.shape[1] != M:
        raise SonetHipError("knn_I must be B x M x K, got %s for x %s" % (tuple(knn_I.shape), tuple(x.shape)))
    K = knn_I.shape[2]
    dev = _same_device(x, knn_I)
    out = torch.empty((B, C, M, K), dtype=torch.float32, device=dev)
    _launch(dev, "knn_gather", _lib.load().sonet_knn_gather_f32, ptr(x), ptr(knn_I), ptr(out), B, C, M, K)
    return out


def knn_gather_bwd(g, knn_I, M):
    """Backward of knn_gather: g B x C x M' x K (f32 / bf16), knn_I B x M' x K i64 -> B x C x M f32 (fixed summation order)."""
    if g.dtype not in (torch.float32, torch.bfloat16):
        raise SonetHipError("knn_gather_bwd: f32 or bf16 gradient")
    _chk(g, "g", g.dtype, 4)
    _chk(knn_I, "som_node_knn_I", torch.int64, 3)
    B, C, Mq, K = g.shape
    if tuple(knn_I.shape) != (B, Mq, K) or Mq != M:
        raise SonetHipError("knn_gather_bwd: knn_I must be B x M x K with the M of the gathered tensor")
    dev = _same_device(g, knn_I)
    lib = _lib.load()
    gx = torch.empty((B, C, M), dtype=torch.float32, device=dev)
    ws = _ws(lib.sonet_knn_gather_bwd_ws_size, dev, B, M, K)
    fn = _by_dtype(lib, "sonet_knn_gather_bwd", g)
    _launch(dev, "knn_gather_bwd", fn, ptr(g), ptr(knn_I), ptr(gx), ptr(ws), B, C, M, K, what="sonet_knn_gather_bwd")
    return gx


class _LastDimMax(torch.autograd.Function):
    """torch.max(x, dim=-1).values with its single-arg-max routing: forward = one kernel (value + index of the first maximum),
    backward = one kernel that writes the whole gradient (no fill + scatter)."""

    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous()
        K = xc.shape[-1]
        rows = xc.numel() // K
        out = torch.empty(xc.shape[:-1], dtype=xc.dtype, device=xc.device)
        idx = torch.empty(xc.shape[:-1], dtype=torch.int32, device=xc.device)
        lib = _lib.load()
        fn = _by_dtype(lib, "sonet_lastdim_argmax", xc)
        _launch(xc.device, "lastdim_argmax", fn, ptr(xc), ptr(out), ptr(idx), rows, K, what="sonet_lastdim_argmax")
        ctx.save_for_backward(idx)
        ctx.K = K
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        gc = g.contiguous()
        gx = torch.empty(tuple(gc.shape) + (ctx.K,), dtype=gc.dtype, device=gc.device)
        lib = _lib.load()
        fn = _by_dtype(lib, "sonet_lastdim_max_bwd", gc)
        _launch(gc.device, "lastdim_max_bwd", fn, ptr(gc), ptr(idx), ptr(gx), gc.numel(), ctx.K, what="sonet_lastdim_max_bwd")
        return gx


def lastdim_max_autograd(x):
    """max over the last dimension of a CUDA f32 / bf16 tensor, differentiable (gradient to the FIRST maximum, as torch.max)."""
    if not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16) or x.numel() == 0:
        return torch.max(x, dim=-1)[0]
    return _LastDimMax.apply(x)


# ------------------------------------------------------------------------------------------ pointmlp
import os as _os


def _env(name, default):
    return _os.environ.get("SONET_" + name, default)


def _flag(name, default="1"):
    """A SONET_<name> switch of the environment: on unless it reads "0"."""
    return _env(name, default) != "0"

# arithmetic of the fused point-wise layer:
#   "f32": exact-f32 MFMA (v_mfma_f32_32x32x2_f32), bitwise an f32 fma chain
#   "x3" : bf16 MFMA on a 3-way bf16 split of both operands (six terms), f32 accumulate: f32-class accuracy (the
#          reference fixtures are met at the same 1e-5 tolerance), f32 operand range, 1.4-1.7x faster than "f32"
#   "bf16": bf16 STORAGE of the activations and one bf16 MFMA per product, f32 accumulate (BASELINE configs[1]); reduced
#          precision by design (features within ~1e-2 of the f32 reference), indices bit-exact on the same bf16 data
#   "h3" : fp16 MFMA on a two-piece fp16 split with scaled residuals (three terms): the same accuracy at half the
#          matrix work, fp16 operand RANGE (|x| <= 2047 clamped, relative precision fades below ~1e-4) -- DEFAULT for
#          the forward layers (coordinates, normalised activations); gradients (dgrad) always use "x3"
POINTMLP_PRECISION = _env("POINTMLP_PRECISION", "h3")


# run the encoder's first PointNet (eval mode, "x3" arithmetic) as one fused kernel
FUSE_POINTRESNET = _flag("FUSE_POINTRESNET")
# ... and pool it per node in the same kernel (no first_pn_out in HBM unless a caller reads the attribute)
FUSE_POOL = _flag("FUSE_POOL")
# no-grad node-level stage (KNNModule + final PointNet) without the gathered tensor and without concats: the neighbour
# gather happens in the first layer's operand loads, narrow leading panels go last through a rotated weight pack (h3 only)
GATHER_NODE_STAGE = _flag("GATHER_NODE_STAGE")
# KNNModule layer 1 as (layer on the M node features) + gather + coordinate channels instead of a layer over K * M gathered columns
NODE_LINEAR_SPLIT = _flag("NODE_LINEAR_SPLIT")
# no-grad h3 chains of point-wise layers hand their activations on pre-split (P16 planes, csrc/pointmlp_h3p.hip) instead of as f32
P16_CHAINS = _flag("P16_CHAINS")
# no-grad node-level stage (KNNModule + final PointNet + global max) on the third-generation layer, flat column axis, max-over-group
# epilogues (csrc/node_stage.hip): 5 launches instead of 8 (4 with KNN_FUSED_LAYER2 below).  0 = the round-4 stage (second-generation layers + planes_max / lastdim_max)
NODE_STAGE_P16 = _flag("NODE_STAGE_P16")
# ... with KNNModule's second layer building its own input in LDS (csrc/knn_layer.hip): 4 launches, h1 never written.  0 = knn_stage_input +
# pointmlp_h3p_gmax; the same planes and range words either way
KNN_FUSED_LAYER2 = _flag("KNN_FUSED_LAYER2")
# bf16 training: the last layer of the first PointNet + the per-node arg-max pool in one launch, first_pn_out never written (0 = store + index_max)
POOLED_TRAIN_EPILOGUE = _flag("POOLED_TRAIN_EPILOGUE")
# f32-class training: the same on node-sorted columns (sonet_pointmlp_h3_segpool_f32; 0 = store + index_max)
H3_SEGPOOL = _flag("H3_SEGPOOL")
# ... and the hidden layers of the first PointNet hand their RAW outputs on: normalise + ReLU is applied by the consumers' operand loads
# (next layer, weight gradient, pooled weight gradient); the normalised activations are never written (0 = a normalise pass per layer)
H3_NORM_ON_LOAD = _flag("H3_NORM_ON_LOAD")
# the sorted training path takes its assignment + node-sorted grouping from the two-launch SOM stage of the no-grad path (0 = som_assign + som_sort_group)
TRAIN_ASSIGN_SORT = _flag("TRAIN_ASSIGN_SORT")
WGRAD_KERNEL = _flag("WGRAD_KERNEL")       # 0: torch.bmm (hipBLASLt f32) for the dense weight gradients


# ---- operand-range guard of the fp16-split ("h3") arithmetic ------------------------------------------------------------------
# h3 has an fp16 operand RANGE (include/sonet_hip.h, "Range log"): every h3 launch inside a ``range_scope`` reports max |x|,
# max |w| (and, for the fused first PointNet, the largest hidden activation) into its own 8-word slot of a per-device log;
# ``violations()`` reads the log back (ONE 1 KiB copy, synchronising) and names the launches whose results are not f32-class.
# Encoder.forward (models/networks.py) wraps itself in a scope and recomputes the batch in the range-safe "x3" arithmetic when
# the log says so -- so the default arithmetic can never hand back clamped features silently.  SONET_RANGE_GUARD=0 turns the
# whole mechanism off (no log, no read-back).
RANGE_GUARD = _flag("RANGE_GUARD")
_RANGE_SLOTS = 32
_B_2047, _B_65504, _B_XLOW, _B_WLOW, _B_WLOW32 = 0x44FFE000, 0x477FE000, 0x3E800000, 0x3B800000, 0x3E000000   # bits of 2047, 65504, 2^-2, 2^-8, 2^-3
_range_logs = {}            # device index -> int32[_RANGE_SLOTS * 8]
_range_active = None        # the innermost open scope
_range_ptr_set = False      # whether the library currently holds a non-NULL slot pointer for this thread


def _bits_to_float(u):
    import struct
    return struct.unpack("<f", struct.pack("<I", int(u) & 0xFFFFFFFF))[0]


class range_scope:
    """``with ops.range_scope(device) as rs: <h3 launches>`` then ``rs.violations()`` (synchronises; [] = all launches in range).
    Eager scopes of one device share its log: read a scope's result before opening the next one on that device;
    ``private=True`` gives the scope a log of its own (sonet_hip.graph.GraphedForward)."""

    def __init__(self, device, private=False):
        self.device = torch.device(device)
        self.names = []
        self.enabled = RANGE_GUARD and self.device.type == "cuda"
        self.log = None
        self._prev = None
        # private: this scope owns its 1 KiB log (a captured forward bakes the clear and the slot pointers into its HIP graph:
        # graphs replayed concurrently, or an eager scope in between, must not clear or overwrite each other's slots)
        self._own = torch.zeros((_RANGE_SLOTS * 8,), dtype=torch.int32, device=self.device) if (private and self.enabled) else None

    def __enter__(self):
        global _range_active
        self._prev = _range_active
        if self.enabled:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            log = self._own if self._own is not None else _range_logs.get(idx)
            if log is None:
                log = torch.zeros((_RANGE_SLOTS * 8,), dtype=torch.int32, device=self.device)
                _range_logs[idx] = log
            else:
                log.zero_()                                   # one memset node (captured like any launch under a HIP graph)
            self.log = log
            _range_active = self
        return self

    def __exit__(self, *exc):
        global _range_active
        _range_active = self._prev
        _range_unset()
        return False

    def _slot(self, name):
        i = min(len(self.names), _RANGE_SLOTS - 1)            # more launches than slots: the last slot is shared (max still holds)
        self.names.append(name)
        return self.log.data_ptr() + i * 32

    def violations(self):
        """-> list of (launch name, what) for the launches of this scope whose operands left the fp16-split range."""
        if not self.enabled or not self.names:
            return []
        w = self.log.cpu().view(_RANGE_SLOTS, 8).tolist()     # synchronises with the launches
        shared = {}
        out = []
        for n, name in enumerate(self.names):
            i = min(n, _RANGE_SLOTS - 1)
            if i in shared:
                continue
            shared[i] = True
            x, wt, hid = (v & 0xFFFFFFFF for v in w[i][:3])
            low_ok = n < _RANGE_SLOTS - 1                     # a shared slot cannot tell which launch was small
            if x > _B_2047:
                out.append((name, "max |x| = %g exceeds 2047" % _bits_to_float(x)))
            elif low_ok and 0 < x < _B_XLOW:
                out.append((name, "max |x| = %g is below %g (fp16 residuals go subnormal)" % (_bits_to_float(x), _bits_to_float(_B_XLOW))))
            # Weight side.  The second-generation layer keeps fp16(w) (limits 65504 and 2^-8).  The fused first PointNet and the third
            # generation (pointmlph3p*; the up-convolution upconv3x3* on its folded weights) keep fp16(32 w) + fp16(32 w - hi): |w| <= 2047,
            # and max |w| >= 2^-8 -- below that the residual piece is an fp16 subnormal with absolute error 2^-30 on w, i.e. up to 2^-22
            # relative (the fused kernel logs 32 |w|).
            if name.startswith("pointresnet_fused"):
                if wt > _B_65504:
                    out.append((name, "max |w| = %g exceeds %g" % (_bits_to_float(wt) / 32.0, 65504.0 / 32.0)))
                elif low_ok and 0 < wt < _B_WLOW32:
                    out.append((name, "max |w| = %g is below 2^-8" % (_bits_to_float(wt) / 32.0)))
            elif name.startswith("pointmlph3p") or name.startswith("upconv3x3"):
                if wt > _B_2047:
                    out.append((name, "max |w| = %g exceeds 2047" % _bits_to_float(wt)))
                elif low_ok and 0 < wt < _B_WLOW:
                    out.append((name, "max |w| = %g is below 2^-8" % _bits_to_float(wt)))
            elif wt > _B_65504:
                out.append((name, "max |w| = %g exceeds 65504" % _bits_to_float(wt)))
            elif low_ok and 0 < wt < _B_WLOW:
                out.append((name, "max |w| = %g is below 2^-8" % _bits_to_float(wt)))
            if hid > _B_2047:
                out.append((name, "a hidden activation reaches %g > 2047" % _bits_to_float(hid)))
        return out


_range_warned = False
_range_pending = []         # training: (event, pinned host copy, names) of steps whose log has not been looked at yet


def range_warn(bad):
    global _range_warned
    if not _range_warned:
        import warnings
        warnings.warn("sonet_hip: fp16-split (h3) operand range left by %d launch(es), e.g. %s: %s -- recomputing in the "
                      "range-safe x3 arithmetic (SONET_POINTMLP_PRECISION=x3 selects it from the start)"
                      % (len(bad), bad[0][0], bad[0][1]), RuntimeWarning, stacklevel=3)
        _range_warned = True


def _range_defer(scope):
    """Queue a scope's log for a later look: async copy to pinned memory + an event, no host wait."""
    if not scope.enabled or not scope.names or torch.cuda.is_current_stream_capturing():
        return
    host = torch.empty((_RANGE_SLOTS * 8,), dtype=torch.int32, pin_memory=True)
    host.copy_(scope.log, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _range_pending.append((ev, host, list(scope.names)))


range_scope.defer = _range_defer


def range_deferred_check():
    """Look at every queued log whose copy has completed (no waiting).  A violation switches the process to the x3
    arithmetic (with a warning): the steps already taken ran on clamped activations, the following ones do not."""
    global POINTMLP_PRECISION
    while _range_pending and _range_pending[0][0].query():
        _, host, names = _range_pending.pop(0)
        probe = range_scope.__new__(range_scope)
        probe.enabled, probe.names, probe.log = True, names, host
        bad = probe.violations()
        if bad:
            range_warn(bad)
            POINTMLP_PRECISION = "x3"
            _range_pending.clear()
            return bad
    return []


def run_guarded(call, device, can_rerun):
    """Run ``call()`` (a forward made of h3 launches) inside an operand-range scope.

    can_rerun (no-grad forwards): the log is read right away -- one small synchronising copy -- and, if any launch left the
    fp16 range, ``call()`` runs again in the range-safe x3 arithmetic: the caller always gets f32-class results.
    not can_rerun (training forwards, which update BatchNorm statistics and must not run twice): the log is queued and
    looked at, without waiting for the GPU, at the next guarded training call; a violation switches the process to x3.
    Nested calls (an encoder inside a guarded model-level forward, anything inside a HIP-graph capture that opened
    its own scope) join the outer scope."""
    device = torch.device(device)
    if POINTMLP_PRECISION != "h3" or not RANGE_GUARD or device.type != "cuda" or _range_active is not None:
        return call()
    if not can_rerun:
        range_deferred_check()                                           # may switch POINTMLP_PRECISION to "x3"
        if POINTMLP_PRECISION != "h3":
            return call()
        with range_scope(device) as rs:
            out = call()
        rs.defer()
        return out
    with range_scope(device) as rs:
        out = call()
    if torch.cuda.is_current_stream_capturing():
        return out
    bad = rs.violations()
    if bad:
        range_warn(bad)
        with precision("x3"):
            out = call()
    return out


def mark_inference(t):
    """Tag a tensor as the product of an inference call (Encoder.forward(is_train=False) on an eval() encoder): eval-mode
    layers that receive it run their no-autograd kernels even when the caller left autograd enabled."""
    if isinstance(t, torch.Tensor) and not t.requires_grad:
        t._sonet_inference = True
    return t


def is_inference(*ts):
    """True when autograd is off, or every given tensor carries the inference tag and none requires grad."""
    if not torch.is_grad_enabled():
        return True
    return bool(ts) and all(isinstance(t, torch.Tensor) and getattr(t, "_sonet_inference", False) and not t.requires_grad for t in ts)


def _range_unset():
    global _range_ptr_set
    if _range_ptr_set:
        _lib.load().sonet_range_log_set(None)
        _range_ptr_set = False


def _range_arm(name):
    """Right before an h3 launch: point the library at this launch's slot (or at nothing outside a scope)."""
    global _range_ptr_set
    if _range_active is None:
        _range_unset()
        return
    import ctypes
    _lib.load().sonet_range_log_set(ctypes.c_void_p(_range_active._slot(name)))
    _range_ptr_set = True


class precision:
    """``with ops.precision("x3"): ...`` -- temporarily select the point-wise arithmetic (the range guard's fallback)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        global POINTMLP_PRECISION
        self.prev = POINTMLP_PRECISION
        POINTMLP_PRECISION = self.mode
        return self

    def __exit__(self, *exc):
        global POINTMLP_PRECISION
        POINTMLP_PRECISION = self.prev
        return False


H3_COLUMN_RATIO = 128.0      # an fp16-split layer of K >= 16 input channels may have max|w[:, c]| / min_c max|w[:, c]| up to H3_COLUMN_RATIO / sqrt(K)
H3_COLUMN_MIN = 2.0 ** -8    # ... and no non-zero input column whose largest weight is below this (see h3_weight_ok)
_h3_ratio_warned = False


def h3_column_ratio_limit(K):
    """Largest admitted ratio between the input columns' maxima of an fp16-split layer with K input channels."""
    return max(1.0, H3_COLUMN_RATIO / float(max(int(K), 16)) ** 0.5)       # (below one 16-channel chunk: the limit of K = 16)


def h3_weight_ok(weight2d):
    """Per-channel side of the h3 operand-range guard, decided on the WEIGHTS (once per pack, one small reduction).

    The range log checks each launch's max |x| (>= X = 2^-2) -- per launch, not per channel.  Both operands are kept as fp16(32 v) plus the
    fp16 of the residual; once the residual is an fp16 subnormal its ABSOLUTE error is up to 2^-25, i.e. up to e = 2^-30 on v (rms e / sqrt 3)
    whatever v's magnitude.  An output sums K products, so it carries the error  sum_c (w_c ex_c + x_c ew_c)  against a value whose rms over
    the launch is  sqrt(sum_c w_c^2 x_c^2)  with w_c, x_c the typical (rms) magnitudes of column c and channel c.
      * x side.  The worst layout lets ONE channel at max |x| carry the output through a SMALL column (w_max / ratio) while the other K - 1
        channels, far below max |x|, meet the LARGE columns: error rms sqrt(K) w_max e / sqrt 3 against a value of rms (w_max / ratio) x_rms.
        The errors of the K - 1 channels add like sqrt(K) -- the count the ratio-only test (128, any K) left out.  With a peak-to-rms of
        about 3.5 on both operands and 4.5 sigma for the largest of 10^5 outputs the relative error is about
        ratio sqrt(K) (2^-30 / X) 3.5^2 4.5 / sqrt 3 <= 2.5e-6 for ratio sqrt(K) <= H3_COLUMN_RATIO = 128 and X = 2^-2: half of the 5e-6 the
        arithmetic may use (the other half of the project's 1e-5 belongs to the kernels' f32 accumulation).
      * w side.  The same with the roles swapped cannot be bounded through max |w| alone (the launch log's 2^-8): a whole matrix may sit a
        ratio below its largest column.  What counts is the SMALLEST column: every non-zero column's maximum must reach H3_COLUMN_MIN = 2^-8,
        which keeps the relative error of a column that carries an output below 2^-30 3.5 4.5 / (sqrt 3 2^-8) = 2.2e-6.
    So: a K-channel weight whose input columns differ by more than H3_COLUMN_RATIO / sqrt(max(K, 16)), or which has a non-zero column below
    H3_COLUMN_MIN, is packed for the range-safe x3 arithmetic (one warning).  Everything the two sides admit stays within 5e-6 of float64 in
    a float64 model of the split on the corner families of the admitted region (tests/test_h3_envelope_cpu.py), and within 1e-5 on the
    kernels (tests/test_gpu_h3_envelope.py); tests/test_gpu_round2.py::test_h3_per_channel_range_case is the far-out adversarial pair."""
    return bool(h3_weight_ratio_flag(weight2d).item())


def h3_weight_ratio_flag(weight2d):
    """The test of h3_weight_ok as a one-element device tensor (1 = fine), without a host synchronisation: the training path
    (weights change every step) reads it one check late through pinned memory (models/layers.py::_h3_ok)."""
    cm = weight2d.detach().abs().amax(dim=0)
    big = cm.max()
    small = torch.where(cm > 0, cm, big).min()                 # smallest non-zero column (all-zero weight: big == small == 0)
    ok = (big <= small * h3_column_ratio_limit(weight2d.shape[1])) & ((small >= H3_COLUMN_MIN) | (big == 0))
    return ok.to(torch.int32).reshape(1)


def h3_ratio_warn(what):
    global _h3_ratio_warned
    if not _h3_ratio_warned:
        import warnings
        warnings.warn("sonet_hip: %s has input columns more than %g / sqrt(K) apart in magnitude, or one below %g -- it runs in the range-safe "
                      "x3 arithmetic instead of the fp16 split (sonet_hip.ops.h3_weight_ok)" % (what, H3_COLUMN_RATIO, H3_COLUMN_MIN),
                      RuntimeWarning, stacklevel=3)
        _h3_ratio_warned = True


def x3_supported(C1, C2, Cout):
    return Cout % 32 == 0 and (C2 == 0 or C1 % 16 == 0)


def pointmlp_pack(weight2d, mode="f32"):
    """[Cout][Cin] f32 -> packed MFMA A-fragment order (device tensor: float32 for "f32", uint8 bytes for "x3")."""
    _chk(weight2d, "weight", torch.float32, 2)
    dev = _same_device(weight2d)
    Cout, Cin = weight2d.shape
    lib = _lib.load()
    kind = mode if mode in ("x3", "h3", "bf16") else "f32"     # (the dtype of the pack marks its flavour: ``_PACKS``)
    wp = _pack_empty(lib, kind, Cin, Cout, dev)
    _launch(dev, None, lib.sonet_pointmlp_pack_f32 if kind == "f32" else getattr(lib, "sonet_pointmlp_%s_pack" % kind), ptr(weight2d), ptr(wp), Cin, Cout)
    return wp


def _pack_strided(lib, kind, src, rs, cs, Cin_p, Cout_p, rows, dev):
    """-> the bf16 / x3 / h3 pack of the rows x Cin_p f32 matrix at address ``src`` (row and column strides rs, cs in elements), with zero
    rows up to Cout_p."""
    wp = _pack_empty(lib, kind, Cin_p, Cout_p, dev)
    _launch(dev, None, getattr(lib, "sonet_pointmlp_%s_pack_strided" % kind), src, rs, cs, ptr(wp), Cin_p, Cout_p, rows,
            what="sonet_pointmlp_%s_pack_strided" % ("bf16" if kind == "bf16" else "x3"))
    return wp


def pointmlp_pack_transposed(weight2d, lo, Ci, Cp, mode):
    """The pack of W[:, lo:lo + Ci]^T (Ci x Cout, zero rows up to Cp) -- the dgrad's weights -- read from ``weight2d`` (Cout x Cin f32,
    contiguous) in place: no transposed copy, and the pack kernel's lanes run along W's rows.  mode "x3" / "h3" / "bf16"."""
    _chk(weight2d, "weight", torch.float32, 2)
    dev = _same_device(weight2d)
    Cout, Cin = weight2d.shape
    if not (0 <= lo and lo + Ci <= Cin and Ci <= Cp):
        raise SonetHipError("pointmlp_pack_transposed: bad block lo=%d Ci=%d Cp=%d of %d columns" % (lo, Ci, Cp, Cin))
    lib = _lib.load()
    if mode not in ("bf16", "x3", "h3"):
        raise SonetHipError("pointmlp_pack_transposed: mode %r" % (mode,))
    return _pack_strided(lib, mode, weight2d.data_ptr() + 4 * lo, 1, Cin, Cout, Cp, Ci, dev)


# ---- every stale weight pack of a step in one launch -------------------------------------------------------------------------------
PACK_REGISTRY = _flag("PACK_REGISTRY")     # 0: a pack launch per layer and flavour (the round-4 behaviour)


class _PackRegistry:
    """The packed copies of the layers' weights (``pointmlp_pack`` / ``pointmlp_pack_transposed`` results), keyed on (weight storage,
    what is packed).  ``get`` returns the current pack; when the weight has changed since it was built (``_version``: the optimizer bumps
    it once per step) EVERY stale pack of that device is refreshed by one ``sonet_pack_multi`` launch -- the layers' forward packs and
    the transposed packs of their dgrads alike -- into the buffers the entries already own.  Entries die with their weight tensor."""

    def __init__(self):
        self.entries = {}            # key -> dict(ref, version, buf, rec)
        self.tables = {}             # device -> (tuple of keys, device table, total blocks)

    @staticmethod
    def _spec(w2d, what):
        """-> (flavour, byte offset into w2d, rs, cs, Cin_pack, rows, Cout_pack) of ("fwd", mode) or ("t", mode, lo, Ci, Cp)."""
        Cout, Cin = w2d.shape
        fl = {"bf16": 0, "x3": 1, "h3": 2}[what[1]]
        if what[0] == "fwd":
            return fl, 0, Cin, 1, Cin, Cout, Cout
        _, _, lo, Ci, Cp = what
        if not (0 <= lo and lo + Ci <= Cin and Ci <= Cp):
            raise SonetHipError("pack registry: bad block lo=%d Ci=%d Cp=%d of %d columns" % (lo, Ci, Cp, Cin))
        return fl, 4 * lo, 1, Cin, Cout, Ci, Cp                       # W[:, lo:lo + Ci]^T: element (o, c) = W[c][lo + o]

    def get(self, w2d, what):
        """w2d: the layer's weight as a contiguous Cout x Cin f32 CUDA tensor (a view of the parameter: same version counter)."""
        key = (w2d.data_ptr(), w2d.device.index, tuple(w2d.shape), what)
        e = self.entries.get(key)
        if e is not None and e["ref"]() is None:                       # the storage was recycled by another tensor
            e = None
        if e is None:
            self._drop_moved(w2d._base if w2d._base is not None else w2d)
            e = self._create(key, w2d, what)
        elif e["version"] != w2d._version:
            self.refresh(w2d.device)
        return e["buf"]

    def _create(self, key, w2d, what):
        import weakref
        _chk(w2d, "weight", torch.float32, 2)
        lib = _lib.load()
        fl, off, rs, cs, Cin_p, rows, Cout_p = self._spec(w2d, what)
        dev = w2d.device
        buf = _pack_strided(lib, ("bf16", "x3", "h3")[fl], w2d.data_ptr() + off, rs, cs, Cin_p, Cout_p, rows, dev)
        KC = int(lib.sonet_pack_multi_kc(fl, Cin_p))
        total = 64 * ((Cout_p + 31) // 32) * KC
        # (the weakref is to the view's base when there is one: views come and go, the parameter stays)
        base = w2d._base if w2d._base is not None else w2d
        # (no strong reference to the weight: only its address, its base's address and the weakref)
        e = dict(ref=weakref.ref(base), base_ptr=base.data_ptr(), version=w2d._version, buf=buf,
                 rec=(w2d.data_ptr() + off, buf.data_ptr(), rs, cs, total, Cin_p, rows, KC, fl))
        self.entries[key] = e
        self.tables.pop(dev.index, None)
        # the entry (and its GPU buffer) goes when the weight goes -- not when some other weight next turns stale (a sweep that builds
        # model after model would otherwise pile up packs of dead weights)
        weakref.finalize(base, self._drop, key, e)
        return e

    def _drop(self, key, e):
        if self.entries.get(key) is e:
            del self.entries[key]
            self.tables.pop(key[1], None)

    def _drop_moved(self, base):
        """``module.cpu()`` / ``.to(device)`` and ``p.data = ...`` keep the Parameter -- the weakref stays alive, the version counter goes
        on -- but give it another storage: an entry made from the old one records an address that may be freed by now.  Such entries go
        (host bookkeeping only; the new address gets entries of its own)."""
        here = base.data_ptr()
        for key, e in [(k, e) for k, e in self.entries.items() if e["ref"]() is base and e["base_ptr"] != here]:
            self._drop(key, e)

    def refresh(self, device):
        """One ``sonet_pack_multi`` launch over every stale entry of ``device``."""
        import numpy as np
        di = device.index
        live, dead = [], []
        for key, e in self.entries.items():
            if key[1] != di:
                continue
            t = e["ref"]()
            if t is None or t.data_ptr() != e["base_ptr"]:              # the weight is gone, or lives elsewhere now (see _drop_moved)
                dead.append(key)
            elif e["version"] != t._version:
                live.append((key, e, t))
        for key in dead:
            del self.entries[key]
        if dead:
            self.tables.pop(di, None)
        if not live:
            return
        keys = tuple(k for k, _, _ in live)
        tab = self.tables.get(di)
        if tab is None or tab[0] != keys:
            rec = np.zeros((len(live), 9), dtype=np.int64)              # 72 bytes per entry
            blk = 0
            for i, (_, e, _) in enumerate(live):
                src, dst, rs, cs, total, Cin_p, rows, KC, fl = e["rec"]
                nblk = (total + 255) // 256
                rec[i, 0], rec[i, 1], rec[i, 2], rec[i, 3], rec[i, 4] = src, dst, rs, cs, total
                rec[i, 5] = (Cin_p & 0xFFFFFFFF) | (rows << 32)
                rec[i, 6] = (KC & 0xFFFFFFFF) | (fl << 32)
                rec[i, 7] = (blk & 0xFFFFFFFF) | (nblk << 32)
                blk += nblk
            with _lib.on_device(device):
                tab = (keys, torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(device), blk)
            self.tables[di] = tab
        _launch(device, "pack_multi_%d" % len(live), _lib.load().sonet_pack_multi, ptr(tab[1]), len(live), tab[2])
        for _, e, t in live:
            e["version"] = t._version


packs = _PackRegistry()


def pointmlp(x1, wp, scale, shift, relu, Cout, x2=None, out=None, gidx=None, acc=None):
    """y = act((W . cat(x1, x2)) * scale + shift); x B x C x L f32.  The kernel follows the packing of ``wp``.
    ``acc`` (bf16 packs, B x Cout x L bf16, even L): another gradient of the same tensor -- y = bf16(float(y) + float(acc)) from the store
    of the launch (``sonet_pointmlp_bf16_acc``: autograd's accumulation without its pass).
    ``gidx`` (B x L i32, h3 packs only): column l of x1 (B x C1 x L1) is taken from x1[:, :, gidx[b, l]] -- zeros when the
    index is out of range -- i.e. the layer runs on the gathered tensor without materialising it."""
    bf16 = wp.dtype == torch.int16
    xdt = torch.bfloat16 if bf16 else torch.float32
    _chk(x1, "x", xdt, 3)
    B, C1, L = x1.shape
    L1 = L
    if gidx is not None:
        _chk(gidx, "gidx", torch.int32, 2)
        if wp.dtype not in (torch.int8, torch.int16) or gidx.shape[0] != B:
            raise SonetHipError("pointmlp: a gather index needs an h3 or bf16 pack and B rows")
        L = gidx.shape[1]
    _, _, C2, _ = _layer_inputs(x1, x2, xdt, L)
    _chk_cvec(Cout, 1, scale=scale, shift=shift)
    dev = _same_device(x1, x2, wp, scale, shift, gidx)
    lib = _lib.load()
    h3 = wp.dtype == torch.int8
    x3 = wp.dtype == torch.uint8 or h3
    _chk_pack(lib, wp, "bf16" if bf16 else "x3" if x3 else "f32", C1 + C2, Cout, "elements")
    y = out if out is not None else torch.empty((B, Cout, L), dtype=xdt, device=dev)
    if y.numel() == 0:
        return y
    head = (ptr(x1), C1, L1, ptr(gidx)) if gidx is not None else (ptr(x1), C1)
    args = head + (ptr(x2), C2, ptr(wp), ptr(scale), ptr(shift), int(bool(relu)))
    if bf16:
        if y.dtype != torch.bfloat16:
            raise SonetHipError("pointmlp: a bf16 pack writes a bfloat16 output")
        if acc is not None:
            _chk(acc, "acc", torch.bfloat16, 3)
            if tuple(acc.shape) != (B, Cout, L) or gidx is not None or L % 2:
                raise SonetHipError("pointmlp: acc must be B x Cout x L (even L, no gather index)")
            _same_device(x1, acc)
            _launch(dev, "pointmlpbf16_acc_%dx%d_L%d" % (C1 + C2, Cout, L), lib.sonet_pointmlp_bf16_acc, *args, ptr(acc), ptr(y), B, Cout, L)
            return y
        _launch(dev, "pointmlpbf16_%dx%d_L%d" % (C1 + C2, Cout, L), lib.sonet_pointmlp_bf16_gather if gidx is not None else lib.sonet_pointmlp_bf16,
                *args, ptr(y), B, Cout, L)
        return y
    name = "pointmlp%s_%dx%d_L%d" % ("h3" if h3 else "x3" if x3 else "", C1 + C2, Cout, L)
    if h3:
        _range_arm(name)
    if gidx is not None:
        _launch(dev, name, lib.sonet_pointmlp_h3_gather_f32, *args, ptr(y), B, Cout, L)
    else:
        _launch(dev, name, lib.sonet_pointmlp_h3_f32 if h3 else lib.sonet_pointmlp_x3_f32 if x3 else lib.sonet_pointmlp_f32, *args, ptr(y), B, Cout, L,
                what="sonet_pointmlp")
    return y


# f32-class training backward: the BatchNorm / ReLU backward of a layer is applied by the operand load of its input-gradient launch, which also
# writes g_raw for the weight gradient (sonet_pointmlp_x3_bnb_f32; 0 = a pass of its own, sonet_pointwise_bwd_apply_f32)
BNB_ON_LOAD = _flag("BNB_ON_LOAD")


# ... and, when the layer BELOW handed its raw output on (normalise-on-load), the same launch's epilogue can compute that layer's BatchNorm-backward
# sums from its output (no statistics pass over (gy, raw) of the layer below).  OFF: measured slower -- the reduction costs the dgrad launch 0.33-0.44 ms
# for the 0.2-0.3 ms pass it replaces (docs/findings.md R5.9); kept as a tested record.
# VARIANTS build only (the product library compiles neither this epilogue nor the tail below: ``variants_only()``).
BWD_STATS_EPILOGUE = _flag("BWD_STATS_EPILOGUE", "0")


def variants_only():
    """True when the loaded library is the variants build (tools/, tests/variants): the measured-slower records are callable."""
    return hasattr(_lib.load(), "sonet_pooled_dgrad_tail_f32")


# a tensor with two consumers in the first PointNet (the first layer's output): the gradient of the consumer whose backward runs first is added by
# the store of the other's input-gradient launch (models/layers.py ``_GradCarry``; 0 = autograd's accumulation, a pass over three tensors)
GRAD_CARRY = _flag("GRAD_CARRY")


def _bnb_inputs(who, kind, dtype, gy, raw, wpt, scale, shift, coeffs, Cout):
    """The operands ``pointmlp_x3_bnb`` and ``pointmlp_bf16_bnb`` share: (gy, raw) B x C x L of ``dtype``, a ``kind`` pack for C -> Cout, Cout
    output coefficients (scale, shift) and C input coefficients each -> (B, C, L, device, library)."""
    _chk(gy, "gy", dtype, 3)
    _chk(raw, "raw", dtype, 3)
    if raw.shape != gy.shape:
        raise SonetHipError("%s: gy and raw must have the same shape" % who)
    B, C, L = gy.shape
    if wpt.dtype != _PACKS[kind][0]:
        raise SonetHipError("%s: %s %s pack" % (who, "an" if kind == "x3" else "a", kind))
    for t in (scale, shift):
        _chk(t, "scale / shift", torch.float32, 1)
        if t.numel() != Cout:
            raise SonetHipError("%s: %d output coefficients expected" % (who, Cout))
    for t in coeffs:
        _chk(t, "coefficient", torch.float32, 1)
        if t.numel() != C:
            raise SonetHipError("%s: %d coefficients expected" % (who, C))
    dev = _same_device(gy, raw, wpt, scale, shift, *coeffs)
    lib = _lib.load()
    _chk_pack(lib, wpt, kind, C, Cout)
    return B, C, L, dev, lib


def pointmlp_x3_bnb(gy, raw, wpt, scale, shift, a, b, c0, sc, sh, relu, Cout, want_g_raw=True, below=None, acc=None):
    """(W . g_raw) * scale + shift with g_raw = a * (gy masked by raw * sc + sh > 0 when relu) + b * raw + c0 per input channel, in one pass
    over (gy, raw) -- ``pointwise_bwd_apply`` + ``pointmlp`` on an x3 pack, bit for bit.  -> (y B x Cout x L, g_raw or None[, sums]).
    below = (praw B x Cout x L, psc, psh, prelu): y is gy of the layer below; -> also its BatchNorm-backward sums (float64 [2 Cout], the
    layout of ``pointwise_bwd_stats(..., want_sums=True)``) from the epilogue.
    acc (B x Cout x L, f32): another gradient of the same tensor, computed earlier -- y = the product + acc from the store of this launch (what
    autograd's accumulation of the two would hold, bit for bit); not together with ``below``."""
    B, C, L, dev, lib = _bnb_inputs("pointmlp_x3_bnb", "x3", torch.float32, gy, raw, wpt, scale, shift, (a, b, c0, sc, sh), Cout)
    y = torch.empty((B, Cout, L), dtype=torch.float32, device=dev)
    g_raw = torch.empty_like(gy) if want_g_raw else None
    if y.numel() == 0:
        return y, g_raw
    praw = psc = psh = pws = sums = None
    prelu = False
    if acc is not None:
        _chk(acc, "acc", torch.float32, 3)
        if below is not None or tuple(acc.shape) != (B, Cout, L):
            raise SonetHipError("pointmlp_x3_bnb: acc must be B x Cout x L and does not combine with the sums of the layer below")
        _same_device(gy, acc)
        _launch(dev, "pointmlpx3_bnba_%dx%d_L%d" % (C, Cout, L), lib.sonet_pointmlp_x3_bnb_acc_f32, ptr(gy), ptr(raw), C, ptr(wpt), ptr(scale), ptr(shift),
                ptr(a), ptr(b), ptr(c0), ptr(sc), ptr(sh), int(bool(relu)), ptr(g_raw), ptr(acc), ptr(y), B, Cout, L)
        return y, g_raw
    if below is not None:
        praw, psc, psh, prelu = below
        _chk(praw, "praw", torch.float32, 3)
        if tuple(praw.shape) != (B, Cout, L) or psc.numel() != Cout or psh.numel() != Cout:
            raise SonetHipError("pointmlp_x3_bnb: the layer below must be B x Cout x L with Cout coefficients")
        _chk(psc, "psc", torch.float32, 1)
        _chk(psh, "psh", torch.float32, 1)
        _same_device(gy, praw, psc, psh)
        pws = _ws(lib.sonet_pointmlp_stats_ws_size, dev, B, Cout, L)
        sums = torch.empty((2 * Cout,), dtype=torch.float64, device=dev)
    _launch(dev, "pointmlpx3_bnb%s_%dx%d_L%d" % ("s" if below is not None else "", C, Cout, L), lib.sonet_pointmlp_x3_bnb_f32, ptr(gy), ptr(raw), C, ptr(wpt),
            ptr(scale), ptr(shift), ptr(a), ptr(b), ptr(c0), ptr(sc), ptr(sh), int(bool(relu)), ptr(g_raw), ptr(y), B, Cout, L, ptr(praw), ptr(psc), ptr(psh),
            int(bool(prelu)), ptr(pws), ptr(sums))
    if below is not None:
        return y, g_raw, sums
    return y, g_raw


def pointmlp_bf16_bnb_ok(C, Cout, L):
    """Shapes ``pointmlp_bf16_bnb`` takes (``sonet_pointmlp_bf16_bnb``)."""
    return C % 16 == 0 and 32 <= C <= 512 and Cout % 64 == 0 and L % 2 == 0


def pointmlp_bf16_bnb(gy, raw, wpt, scale, shift, a, b, c0, sc, sh, relu, Cout, want_g_raw=True, acc=None):
    """bf16((W . g_raw) * scale + shift) [+ acc] with g_raw = bf16(a * (gy masked by raw * sc + sh > 0 when relu) + b * raw + c0) per input
    channel, in one pass over (gy, raw) -- ``pointwise_bwd_apply`` + ``pointmlp`` (or its ``acc`` form) on a bf16 pack, bit for bit
    (``sonet_pointmlp_bf16_bnb``).  -> (y B x Cout x L bf16, g_raw or None)."""
    B, C, L, dev, lib = _bnb_inputs("pointmlp_bf16_bnb", "bf16", torch.bfloat16, gy, raw, wpt, scale, shift, (a, b, c0, sc, sh), Cout)
    if not pointmlp_bf16_bnb_ok(C, Cout, L):
        raise SonetHipError("pointmlp_bf16_bnb: needs C %% 16 == 0, 32 <= C <= 512, Cout %% 64 == 0, even L (got C=%d Cout=%d L=%d)" % (C, Cout, L))
    if acc is not None:
        _chk(acc, "acc", torch.bfloat16, 3)
        if tuple(acc.shape) != (B, Cout, L):
            raise SonetHipError("pointmlp_bf16_bnb: acc must be B x Cout x L")
        _same_device(gy, acc)
    y = torch.empty((B, Cout, L), dtype=torch.bfloat16, device=dev)
    g_raw = torch.empty_like(gy) if want_g_raw else None
    if y.numel() == 0:
        return y, g_raw
    _launch(dev, "pointmlpbf16_bnb%s_%dx%d_L%d" % ("a" if acc is not None else "", C, Cout, L), lib.sonet_pointmlp_bf16_bnb, ptr(gy), ptr(raw), C, ptr(wpt),
            ptr(scale), ptr(shift), ptr(a), ptr(b), ptr(c0), ptr(sc), ptr(sh), int(bool(relu)), ptr(g_raw), ptr(acc), ptr(y), B, Cout, L)
    return y, g_raw


def pointmlp_nodeadd(x1, wp, scale, shift, relu, Cout, z, zidx, x2=None):
    """act((W . cat(x1, x2) + z[:, :, zidx]) * scale + shift) in one launch: z B x Cout x M f32 (the per-node block of the layer's
    pre-activation), zidx B x L i32 (out of range: + 0).  h3 packs only."""
    if wp.dtype != torch.int8:
        raise SonetHipError("pointmlp_nodeadd: an h3 pack")
    _chk(x1, "x", torch.float32, 3)
    _chk(z, "z", torch.float32, 3)
    _chk(zidx, "zidx", torch.int32, 2)
    B, C1, C2, L = _layer_inputs(x1, x2, torch.float32)
    dev = _same_device(x1, x2, wp, scale, shift, z, zidx)
    lib = _lib.load()
    if wp.numel() != _pack_bytes(lib, "h3", C1 + C2, Cout) or tuple(z.shape[:2]) != (B, Cout) or tuple(zidx.shape) != (B, L):
        raise SonetHipError("pointmlp_nodeadd: pack for Cin=%d Cout=%d, z B x Cout x M, zidx B x L" % (C1 + C2, Cout))
    _chk_cvec(Cout, scale=scale, shift=shift)
    y = torch.empty((B, Cout, L), dtype=torch.float32, device=dev)
    name = "pointmlph3_nodeadd_%dx%d_L%d" % (C1 + C2, Cout, L)
    _range_arm(name)
    _launch(dev, name, lib.sonet_pointmlp_h3_nodeadd_f32, ptr(x1), C1, ptr(x2), C2, ptr(wp), ptr(scale), ptr(shift), int(bool(relu)), ptr(y), B, Cout, L,
            ptr(z), ptr(zidx), z.shape[2])
    return y


# backward: the weight gradient of a layer does not depend on its input gradient -- the two run on two HIP streams
BWD_SIDE_STREAM = _flag("BWD_SIDE_STREAM")
# ... of the pooled last layer in particular: its sparse weight gradient beside its sparse input gradient (0 = one after the other)
POOLED_SIDE_STREAM = _flag("POOLED_SIDE_STREAM")
_side_streams = {}


class side_stream:
    """``with ops.side_stream(device) as s: <launches>`` -- the launches go to a per-device side stream that first waits for everything
    queued on the current stream; ``s.join()`` (after the block) makes the current stream wait for them.  Tensors ALLOCATED inside the
    block and used afterwards must be passed to ``s.keep(t)`` (record_stream: the caching allocator then knows the consumer stream).
    Disabled (everything on the current stream) when BWD_SIDE_STREAM is off, on CPU, or while a HIP graph is being captured."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.on = (BWD_SIDE_STREAM and self.device.type == "cuda" and not torch.cuda.is_current_stream_capturing())
        self.main = self.side = self._ctx = None

    def __enter__(self):
        if self.on:
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.side = _side_streams.get(idx)
            if self.side is None:
                self.side = _side_streams[idx] = torch.cuda.Stream(device=self.device)
            self.main = torch.cuda.current_stream(self.device)
            self.side.wait_stream(self.main)
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.on:
            self._ctx.__exit__(*exc)
        return False

    def keep(self, t):
        if self.on and t is not None:
            t.record_stream(self.main)
        return t

    def reads(self, *ts):
        """Tensors the launches of the block READ that were allocated on the main stream and may be released before the side stream is
        joined (``join(defer=True)``): the caching allocator must not hand their memory out again before the side stream has passed this point."""
        if self.on:
            for t in ts:
                if t is not None and t.is_cuda:
                    t.record_stream(self.side)

    def join(self, defer=False):
        """The current stream waits for the side stream.  ``defer=True`` (from an autograd backward only, ``ops.DEFER_WGRAD_JOIN``): the wait is
        left to the END of the backward pass (an engine callback) -- or to whoever reads a gradient earlier and calls
        ``ops.join_side_streams()`` first (the gradient all-reducer's bucket hooks do) --, so that the launches behind this point on the
        current stream (the next layer's backward) run beside the side stream's instead of waiting for them.  Everything the side-stream
        launches read must have gone through ``reads()``."""
        if not self.on:
            return
        idx = self.side.device.index
        task = _graph_task_id() if _graph_task_id is not None else -1     # (-1: not inside an autograd pass, or a torch without the query)
        if defer and DEFER_WGRAD_JOIN and task != -1:
            with _join_lock:
                _pending_join[idx] = (self.main, self.side)
                queue = _join_queued[0] != task              # (once per backward pass; a pass that died with an exception never ran its callback)
                _join_queued[0] = task
            if queue:
                torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward_join)
            return
        self.main.wait_stream(self.side)
        with _join_lock:
            _pending_join.pop(idx, None)


# weight gradients are not needed before the backward pass is over: their side-stream launches are joined there (0 = at the end of every
# layer's backward, the behaviour up to round 5's first session)
DEFER_WGRAD_JOIN = _flag("DEFER_WGRAD_JOIN")
_graph_task_id = getattr(torch._C, "_current_graph_task_id", None)
_pending_join = {}               # device index -> (main stream, side stream) with launches nobody has waited for yet (under _join_lock)
_join_queued = [-1]             # id of the autograd graph task whose end-of-pass callback is queued


def join_side_streams():
    """Every stream that handed work to a side stream with a deferred join waits for it now (a no-op when nothing is pending).  Call it
    before reading a weight gradient INSIDE a backward pass (gradient hooks); after ``backward()`` has returned it has already happened."""
    with _join_lock:
        pairs = list(_pending_join.values())
        _pending_join.clear()
    for main, side in pairs:
        main.wait_stream(side)


def _end_of_backward_join():
    with _join_lock:
        _join_queued[0] = -1
    join_side_streams()


STATS_EPILOGUE = _flag("STATS_EPILOGUE")   # 0: BatchNorm batch statistics by a separate pass (channel_stats)


# bf16 training (BASELINE configs[1]): the same for the bf16 layers -- the normalise + ReLU pass of the first PointNet's hidden layers (three
# streams over B x C x kN bf16 tensors per step) is gone; the streaming layer kernel, the pooled last layer and the two weight-gradient kernels
# apply act(raw * scale + shift) to their operands (sonet_pointmlp_bf16_stats_xaff / _pool_xaff, sonet_wgrad_bf16_xaff, sonet_pooled_wgrad_xaff_xbf16)
BF16_NORM_ON_LOAD = _flag("BF16_NORM_ON_LOAD")
# ... and the BatchNorm / ReLU backward of the bf16 hidden layers rides on the operand load of the input-gradient launch (sonet_pointmlp_bf16_bnb)
# instead of being a pass over (gy, raw) that writes g_raw for the launch to read back
BF16_BNB_ON_LOAD = _flag("BF16_BNB_ON_LOAD")


def bf16_xaff_ok(B, C1, C2, Cout, L):
    """Shapes the normalise-on-load form of the bf16 layer takes (the streaming kernel: ``sonet_pointmlp_bf16_stats_xaff``)."""
    return ((C1 + C2) % 64 == 0 and (C2 == 0 or C1 % 16 == 0) and Cout % 64 == 0 and L % 2 == 0 and B * ((L + 63) // 64) >= 8192
            and B * L * Cout * 4 >= (32 << 20))


def xaff_ok(C1, C2, Cout):
    """Shapes the normalise-on-load form of the h3 layer takes (``sonet_pointmlp_h3_stats_xaff_f32`` / the xaff arguments of
    ``sonet_pointmlp_h3_segpool_f32``)."""
    return C1 + C2 <= 1024 and Cout % 128 == 0 and (C2 == 0 or C1 % 16 == 0)


def _xaff_args(xaff, C1, C2, dev):
    """xaff = (s1, h1, relu1[, s2, h2, relu2]) -> the C ABI's five arguments."""
    s1, h1, r1 = xaff[:3]
    s2, h2, r2 = (xaff[3:6] if len(xaff) >= 6 else (None, None, False))
    for t, n in ((s1, C1), (h1, C1), (s2, C2), (h2, C2)):
        if t is None:
            continue
        _chk(t, "xaff", torch.float32, 1)
        if t.numel() != n or t.device != dev:
            raise SonetHipError("xaff: %d coefficients on %s expected" % (n, dev))
    if C2 and (s2 is None or h2 is None):
        raise SonetHipError("xaff: a second input needs its coefficients")
    return ptr(s1), ptr(h1), ptr(s2), ptr(h2), int(bool(r1)) | (int(bool(r2)) << 1)


@_consumes_rider
def pointmlp_stats(x1, wp, scale, shift, relu, Cout, x2=None, xaff=None):
    """pointmlp(...) plus the per-channel (mean, biased var) of its output over (B, L), from the kernel's epilogue.  h3 / x3 packs
    (f32 storage) only; -> (y, mean, var).  xaff (h3 packs): the inputs are RAW outputs of BatchNorm layers, normalised by the operand load."""
    h3 = wp.dtype == torch.int8
    bf16 = wp.dtype == torch.int16
    if not (h3 or bf16 or wp.dtype == torch.uint8):
        raise SonetHipError("pointmlp_stats: an h3, x3 or bf16 pack")
    xdt = torch.bfloat16 if bf16 else torch.float32
    _chk(x1, "x", xdt, 3)
    B, C1, C2, L = _layer_inputs(x1, x2, xdt)
    dev = _same_device(x1, x2, wp, scale, shift)
    lib = _lib.load()
    _chk_pack(lib, wp, "bf16" if bf16 else "h3", C1 + C2, Cout)
    _chk_cvec(Cout, scale=scale, shift=shift)
    y = torch.empty((B, Cout, L), dtype=xdt, device=dev)
    mean = torch.empty((Cout,), dtype=torch.float32, device=dev)
    var = torch.empty((Cout,), dtype=torch.float32, device=dev)
    ws = _ws(lib.sonet_pointmlp_bf16_stats_ws_size if bf16 else lib.sonet_pointmlp_stats_ws_size, dev, B, Cout, L)
    args = (ptr(x1), C1, ptr(x2), C2, ptr(wp), ptr(scale), ptr(shift), int(bool(relu)), ptr(y), B, Cout, L, ptr(ws), ptr(mean), ptr(var))
    name = "pointmlp%s_stats_%dx%d_L%d" % ("bf16" if bf16 else "h3" if h3 else "x3", C1 + C2, Cout, L)
    if h3:
        _range_arm(name)
    if xaff is not None:
        if not (h3 or bf16):
            raise SonetHipError("pointmlp_stats: normalise-on-load needs an h3 pack")
        _launch(dev, name + "_xaff", lib.sonet_pointmlp_bf16_stats_xaff if bf16 else lib.sonet_pointmlp_h3_stats_xaff_f32, *args,
                *_xaff_args(xaff, C1, C2, dev))
    elif bf16:
        _launch(dev, name, lib.sonet_pointmlp_bf16_stats, *args)
    else:
        _launch(dev, name, lib.sonet_pointmlp_h3_stats_f32 if h3 else lib.sonet_pointmlp_x3_stats_f32, *args, what="sonet_pointmlp_stats")
    return y, mean, var


@_consumes_rider
def pointmlp_nodeadd_stats(x1, wp, bias, Cout, z, zidx, x2=None):
    """raw = W . cat(x1, x2) + z[:, :, zidx] + bias and the per-channel (mean, biased var) of raw over (B, L) from the kernel's epilogue,
    in one launch: the TRAINING forward of a BatchNorm layer whose per-node and per-cloud input channels were multiplied once per node
    (z B x Cout x M f32, zidx B x L i32, out of range: + 0) -- ``pointmlp_nodeadd`` with the epilogue of ``pointmlp_stats``.  h3 packs
    only; consumes an armed ``bn_rider``.  -> (raw, mean, var)."""
    if not isinstance(wp, torch.Tensor) or wp.dtype != torch.int8:
        raise SonetHipError("pointmlp_nodeadd_stats: an h3 pack")
    _chk(x1, "x", torch.float32, 3)
    _chk(z, "z", torch.float32, 3)
    _chk(zidx, "zidx", torch.int32, 2)
    B, C1, C2, L = _layer_inputs(x1, x2, torch.float32)
    _chk_cvec(Cout, bias=bias)
    dev = _same_device(x1, x2, wp, bias, z, zidx)
    lib = _lib.load()
    if wp.numel() != _pack_bytes(lib, "h3", C1 + C2, Cout) or tuple(z.shape[:2]) != (B, Cout) or tuple(zidx.shape) != (B, L):
        raise SonetHipError("pointmlp_nodeadd_stats: pack for Cin=%d Cout=%d, z B x Cout x M, zidx B x L" % (C1 + C2, Cout))
    raw = torch.empty((B, Cout, L), dtype=torch.float32, device=dev)
    mean = torch.empty((Cout,), dtype=torch.float32, device=dev)
    var = torch.empty((Cout,), dtype=torch.float32, device=dev)
    ws = _ws(lib.sonet_pointmlp_stats_ws_size, dev, B, Cout, L)
    name = "pointmlph3_nodeadd_stats_%dx%d_L%d" % (C1 + C2, Cout, L)
    _range_arm(name)
    _launch(dev, name, lib.sonet_pointmlp_h3_nodeadd_stats_f32, ptr(x1), C1, ptr(x2), C2, ptr(wp), ptr(const_vec(Cout, 1.0, dev)), ptr(bias), 0, ptr(raw),
            B, Cout, L, ptr(z), ptr(zidx), z.shape[2], ptr(ws), ptr(mean), ptr(var))
    return raw, mean, var


# ---- third generation of the fp16-split layer: pre-split activations ("P16" planes, csrc/pointmlp_h3p.hip) -------------------------
class P16:
    """A B x C x L activation in the P16 layout (include/sonet_hip.h): two fp16 planes per value, in MFMA B-fragment order.
    ``data`` is the raw byte tensor (64 * ceil(C / 16) * L bytes per cloud).  Produced by ``p16_from_f32`` or by ``pointmlp_h3p(...,
    out="p16")``, consumed by ``pointmlp_h3p``; ``float()`` decodes it."""

    __slots__ = ("data", "B", "C", "L")

    def __init__(self, data, B, C, L):
        self.data, self.B, self.C, self.L = data, B, C, L

    @property
    def shape(self):
        return (self.B, self.C, self.L)

    @property
    def device(self):
        return self.data.device

    def float(self):
        return p16_to_f32(self)


def p16_empty(B, C, L, device):
    n = _lib.load().sonet_p16_size(B, C, L)
    return P16(torch.empty((n,), dtype=torch.uint8, device=device), B, C, L)


def p16_from_f32(x, scale=None, shift=None, relu=False):
    """f32 B x C x L -> P16 planes of act(x * scale + shift) (scale / shift per channel, both or none).  Inside a range scope the
    launch logs the largest magnitude it split (word 2 of its slot: the consumers of the planes cannot check it any more)."""
    _chk(x, "x", torch.float32, 3)
    B, C, L = x.shape
    dev = _same_device(x, scale, shift)
    out = p16_empty(B, C, L, dev)
    if x.numel() == 0:
        return out
    if scale is not None:
        _chk(scale, "scale", torch.float32, 1)
        _chk(shift, "shift", torch.float32, 1)
    name = "p16_from_f32_%d_L%d" % (C, L)
    _range_arm(name)
    _launch(dev, name, _lib.load().sonet_p16_from_f32, ptr(x), ptr(out.data), B, C, L, ptr(scale), ptr(shift), int(bool(relu)))
    return out


def p16_to_f32(p):
    x = torch.empty((p.B, p.C, p.L), dtype=torch.float32, device=p.device)
    if x.numel():
        _launch(p.device, "p16_to_f32", _lib.load().sonet_p16_to_f32, ptr(p.data), ptr(x), p.B, p.C, p.L)
    return x


def pointmlp_h3p_pack(weight2d):
    """[Cout][Cin] f32 -> the h3p pack (int32 tensor marks the flavour): K slots in P16 channel order, fp16(32 w) + residual."""
    _chk(weight2d, "weight", torch.float32, 2)
    dev = _same_device(weight2d)
    Cout, Cin = weight2d.shape
    lib = _lib.load()
    wp = _pack_empty(lib, "h3p", Cin, Cout, dev)
    _launch(dev, None, lib.sonet_pointmlp_h3p_pack, ptr(weight2d), ptr(wp), Cin, Cout)
    return wp


@_consumes_rider
def pointmlp_h3p(x1, wp, scale, shift, relu, Cout, x2=None, out="f32", gidx=None, z=None, zidx=None, stats=False, tag=None):
    """y = act((W . cat(x1, x2) [+ z[:, :, zidx]]) * scale + shift) on P16 inputs (x1, x2: ``P16``).
    out: "f32" -> B x Cout x L f32 tensor, "p16" -> ``P16``, "both" -> (f32, P16).  gidx (B x L i32): column l of x1 is x1[:, :, gidx[b, l]].
    stats=True (out "f32" only): also the per-channel (mean, biased var) of y over (B, L) -> (y, mean, var)."""
    if not isinstance(x1, P16) or (x2 is not None and not isinstance(x2, P16)):
        raise SonetHipError("pointmlp_h3p: P16 inputs (ops.p16_from_f32)")
    if wp.dtype != torch.int32:
        raise SonetHipError("pointmlp_h3p: an h3p pack (ops.pointmlp_h3p_pack)")
    B, C1, L1 = x1.shape
    L = L1
    if gidx is not None:
        _chk(gidx, "gidx", torch.int32, 2)
        if gidx.shape[0] != B:
            raise SonetHipError("pointmlp_h3p: gidx must have B rows")
        L = gidx.shape[1]
    _, _, C2, _ = _layer_inputs(x1, x2, None, L)
    if x2 is not None and C1 % 16 != 0:
        raise SonetHipError("pointmlp_h3p: with a second input C1 must be a multiple of 16")
    _chk_cvec(Cout, 1, scale=scale, shift=shift)
    if (z is None) != (zidx is None):
        raise SonetHipError("pointmlp_h3p: z and zidx come together")
    ZM = 0
    if z is not None:
        _chk(z, "z", torch.float32, 3)
        _chk(zidx, "zidx", torch.int32, 2)
        if tuple(z.shape[:2]) != (B, Cout) or tuple(zidx.shape) != (B, L):
            raise SonetHipError("pointmlp_h3p: z must be B x Cout x M and zidx B x L")
        ZM = z.shape[2]
    if out not in ("f32", "p16", "both") or (stats and out != "f32"):
        raise SonetHipError("pointmlp_h3p: out is 'f32', 'p16' or 'both' (statistics: 'f32')")
    dev = _same_device(x1.data, x2.data if x2 is not None else None, wp, scale, shift, gidx, z, zidx)
    lib = _lib.load()
    # the pack's K range is the concatenation of the inputs' 16-channel chunks
    cin_pack = (C1 + C2) if C2 else C1
    _chk_pack(lib, wp, "h3p", cin_pack, Cout, "bytes")
    y = torch.empty((B, Cout, L), dtype=torch.float32, device=dev) if out in ("f32", "both") else None
    yp = p16_empty(B, Cout, L, dev) if out in ("p16", "both") else None
    mean = var = ws = None
    if stats:
        mean = torch.empty((Cout,), dtype=torch.float32, device=dev)
        var = torch.empty((Cout,), dtype=torch.float32, device=dev)
        ws = _ws(lib.sonet_pointmlp_h3p_stats_ws_size, dev, B, Cout, L)
    if B * L * Cout != 0:
        name = "pointmlph3p%s_%dx%d_L%d" % ("_nodeadd" if z is not None else "_stats" if stats else ("_" + tag) if tag else "", C1 + C2, Cout, L)
        _range_arm(name)
        _launch(dev, name, lib.sonet_pointmlp_h3p, ptr(x1.data), C1, L1, ptr(gidx), ptr(x2.data) if x2 is not None else None, C2, ptr(wp), ptr(scale),
                ptr(shift), int(bool(relu)), ptr(y), ptr(yp.data) if yp is not None else None, B, Cout, L, ptr(z), ptr(zidx), ZM, ptr(ws), ptr(mean), ptr(var))
    if stats:
        return y, mean, var
    return y if out == "f32" else yp if out == "p16" else (y, yp)


def node_stage_columns(B, M):
    """Column count Lm of the M-level tensors of the flat node-level stage: B * M rounded up to a multiple of 128."""
    return (B * M + 127) // 128 * 128


def p16_flat(C, L, nvalid, device):
    """P16 planes of a flat 1 x C x L activation whose first ``nvalid`` columns a kernel will write: the pad columns must read as zeros
    (garbage there would reach the range log), so a padded axis starts zero-filled."""
    if nvalid == L:
        return p16_empty(1, C, L, device)
    n = _lib.load().sonet_p16_size(1, C, L)
    return P16(torch.zeros((n,), dtype=torch.uint8, device=device), 1, C, L)


def pointmlp_h3p_gmax(x1, wp, scale, shift, relu, Cout, GK, G, ngout, x2=None, out="p16", Lout=None):
    """The layer followed by a max over groups of GK consecutive columns, one launch (``sonet_pointmlp_h3p_gmax``): x1 (x2) ``P16`` with
    B == 1 and L % 128 == 0, G groups per 128-column block.  out "p16" -> ``P16`` 1 x Cout x Lout (Lout >= ngout columns, default ngout;
    pad columns zero), "f32" -> f32 tensor ngout x Cout."""
    if not isinstance(x1, P16) or (x2 is not None and not isinstance(x2, P16)):
        raise SonetHipError("pointmlp_h3p_gmax: P16 inputs")
    if wp.dtype != torch.int32:
        raise SonetHipError("pointmlp_h3p_gmax: an h3p pack (ops.pointmlp_h3p_pack)")
    if x1.B != 1 or (x2 is not None and (x2.B != 1 or x2.L != x1.L)):
        raise SonetHipError("pointmlp_h3p_gmax: one flat cloud (B == 1), x2 with the columns of x1")
    if out not in ("p16", "f32"):
        raise SonetHipError("pointmlp_h3p_gmax: out is 'p16' or 'f32'")
    C1, L = x1.C, x1.L
    C2 = x2.C if x2 is not None else 0
    _chk_cvec(Cout, 1, scale=scale, shift=shift)
    dev = _same_device(x1.data, x2.data if x2 is not None else None, wp, scale, shift)
    lib = _lib.load()
    _chk_pack(lib, wp, "h3p", C1 + C2, Cout, "bytes")
    Lout = int(ngout if Lout is None else Lout)
    y = torch.empty((ngout, Cout), dtype=torch.float32, device=dev) if out == "f32" else None
    yp = p16_flat(Cout, Lout, ngout, dev) if out == "p16" else None
    name = "pointmlph3p_gmax%d_%dx%d_L%d" % (GK, C1 + C2, Cout, int(ngout) * int(GK))      # (the columns that count: without the blocks' padding)
    _range_arm(name)
    _launch(dev, name, lib.sonet_pointmlp_h3p_gmax, ptr(x1.data), C1, ptr(x2.data) if x2 is not None else None, C2, ptr(wp), ptr(scale), ptr(shift),
            int(bool(relu)), Cout, L, int(GK), int(G), int(ngout), Lout, ptr(y), ptr(yp.data) if yp is not None else None)
    return y if out == "f32" else yp


def knn_stage_prepare(coord, knn_I, K, center_avg):
    """Index / coordinate side of KNNModule on the flat column axis (``sonet_knn_stage_prepare_f32``; needs only the node coordinates):
    coord B x 3 x M f32, knn_I B x M x KI int64 (first K columns used) -> dict(center B x 3 x M f32, center_p16 ``P16`` 1 x 3 x Lm,
    rec int32 Lp x 4, B, M, K, G) with G = min(16, 128 // K) nodes per 128-column block of the K-level tensor."""
    _chk(coord, "coord", torch.float32, 3)
    _chk(knn_I, "knn_I", torch.int64, 3)
    B, three, M = coord.shape
    KI = knn_I.shape[2]
    if three != 3 or tuple(knn_I.shape[:2]) != (B, M) or KI < K or not 1 <= K <= 128:
        raise SonetHipError("knn_stage_prepare: coord B x 3 x M, knn_I B x M x (>= K), 1 <= K <= 128")
    dev = _same_device(coord, knn_I)
    lib = _lib.load()
    Lm = node_stage_columns(B, M)
    Lp = int(lib.sonet_knn_stage_columns(B, M, int(K)))
    center = torch.empty((B, 3, M), dtype=torch.float32, device=dev)
    cp = p16_flat(3, Lm, B * M, dev)
    rec = torch.empty((Lp, 4), dtype=torch.int32, device=dev)
    _range_arm("knn_stage_prepare")
    _launch(dev, "knn_stage_prepare", lib.sonet_knn_stage_prepare_f32, ptr(coord), ptr(knn_I), KI, int(bool(center_avg)), B, M, int(K), ptr(center),
            ptr(cp.data), ptr(rec))
    return dict(center=center, center_p16=cp, rec=rec, B=B, M=M, K=int(K), G=min(16, 128 // int(K)), Lp=Lp)


def knn_stage_input(prep, z, wl, scale, shift, relu):
    """KNNModule's first layer per neighbour copy (``sonet_knn_stage_input_p16``): prep from ``knn_stage_prepare``, z ``P16`` 1 x C x Lm
    (the layer's feature block applied per node), wl C x 3 -> h1 ``P16`` 1 x C x Lp."""
    if not isinstance(z, P16) or z.B != 1 or z.L != node_stage_columns(prep["B"], prep["M"]):
        raise SonetHipError("knn_stage_input: z is a P16 1 x C x Lm activation")
    _chk(wl, "wl", torch.float32, 2)
    _chk(scale, "scale", torch.float32, 1)
    _chk(shift, "shift", torch.float32, 1)
    C = z.C
    if tuple(wl.shape) != (C, 3) or scale.numel() != C or shift.numel() != C:
        raise SonetHipError("knn_stage_input: wl C x 3, scale / shift C")
    dev = _same_device(prep["rec"], z.data, wl, scale, shift)
    h1 = p16_empty(1, C, prep["Lp"], dev)            # (every column is written: pad columns as zeros)
    name = "knn_stage_input_%dx%d" % (C, prep["B"] * prep["M"] * prep["K"])
    _range_arm(name)
    _launch(dev, name, _lib.load().sonet_knn_stage_input_p16, ptr(prep["rec"]), ptr(z.data), ptr(wl), ptr(scale), ptr(shift), int(bool(relu)), prep["B"],
            prep["M"], prep["K"], C, ptr(h1.data))
    return h1


KNN_LAYER2_MAX_C = 512                # csrc/knn_layer.hip: Cin and Cout at most (its coefficient tables are static LDS)


def knn_layer2_supported(Cin, Cout, K, B=1, M=1, Lout=None):
    """The shapes ``sonet_knn_layer2_gmax_p16`` takes (it refuses the others with SONET_ERR_UNSUPPORTED before launching), its panel
    limits included: a caller that gets False takes ``knn_stage_input`` + ``pointmlp_h3p_gmax``."""
    if not (Cout % 128 == 0 and 0 < Cout <= KNN_LAYER2_MAX_C and Cin % 16 == 0 and 0 < Cin <= KNN_LAYER2_MAX_C
            and 1 <= K <= 128 and min(16, 128 // K) * K <= 128 and B > 0 and M > 0):
        return False
    G = min(16, 128 // K)
    Lm = node_stage_columns(B, M)
    Lout = Lm if Lout is None else int(Lout)
    nblk = (B * M + G - 1) // G
    KCP = (Cin + 127) // 128 * 8
    return (nblk <= 0x7FFFFFFF and (Cin // 16) * 64.0 * Lm < 2.0e9 and (Cout // 16) * 64.0 * Lout < 2.0e9
            and (Cout // 32) * KCP * 2048.0 < 2.0e9)


def knn_layer2_gmax(prep, z, wl, s1, t1, relu1, wp, s2, t2, relu2, Cout, Lout):
    """``knn_stage_input`` + ``pointmlp_h3p_gmax(..., out="p16")`` in one launch (``sonet_knn_layer2_gmax_p16``): h1 is built in LDS.
    prep, z, wl, s1, t1, relu1 as ``knn_stage_input`` takes them; wp, s2, t2, relu2 = KNNModule's second layer (h3p pack C x Cout)
    -> ``P16`` 1 x Cout x Lout, the maxima over each node's K neighbour copies in columns 0 .. B M - 1, pad columns zero."""
    if not isinstance(z, P16) or z.B != 1 or z.L != node_stage_columns(prep["B"], prep["M"]):
        raise SonetHipError("knn_layer2_gmax: z is a P16 1 x C x Lm activation")
    if wp.dtype != torch.int32:
        raise SonetHipError("knn_layer2_gmax: an h3p pack (ops.pointmlp_h3p_pack)")
    _chk(wl, "wl", torch.float32, 2)
    for n_, v_ in (("s1", s1), ("t1", t1), ("s2", s2), ("t2", t2)):
        _chk(v_, n_, torch.float32, 1)
    C = z.C
    if tuple(wl.shape) != (C, 3) or s1.numel() != C or t1.numel() != C or s2.numel() != Cout or t2.numel() != Cout:
        raise SonetHipError("knn_layer2_gmax: wl C x 3, s1 / t1 C, s2 / t2 Cout")
    dev = _same_device(prep["rec"], z.data, wl, s1, t1, wp, s2, t2)
    lib = _lib.load()
    _chk_pack(lib, wp, "h3p", C, Cout, "bytes")
    B, M, K, G = prep["B"], prep["M"], prep["K"], prep["G"]
    ngout, Lout = B * M, int(Lout)
    yp = p16_flat(Cout, Lout, ngout, dev)
    name = "pointmlph3p_knn_gmax%d_%dx%d_L%d" % (K, C, Cout, ngout * K)
    _range_arm(name)
    _launch(dev, name, lib.sonet_knn_layer2_gmax_p16, ptr(prep["rec"]), ptr(z.data), ptr(wl), ptr(s1), ptr(t1), int(bool(relu1)), B, M, K, C, ptr(wp), ptr(s2),
            ptr(t2), int(bool(relu2)), int(Cout), K, G, ngout, Lout, ptr(yp.data))
    return yp


def p16_flat_to_bcm(p, B, M):
    """``P16`` 1 x C x Lm on the flat column axis of the node-level stage -> f32 B x C x M."""
    if p.B != 1 or p.L != node_stage_columns(B, M):
        raise SonetHipError("p16_flat_to_bcm: a 1 x C x (B M) activation")
    x = torch.empty((B, p.C, M), dtype=torch.float32, device=p.device)
    _launch(p.device, "p16_flat_to_bcm", _lib.load().sonet_p16_flat_to_bcm_f32, ptr(p.data), ptr(x), B, p.C, M)
    return x


def _pointresnet_pack(ws, who, size_fn, fn):
    for i, w in enumerate(ws):
        _chk(w, "w%d" % (i + 1), torch.float32, 2)
    w1, w2, w3, w4 = ws
    if (w1.shape[0], tuple(w2.shape), tuple(w3.shape), tuple(w4.shape)) != (64, (128, 64), (256, 128), (384, 320)) or w1.shape[1] > 16:
        raise SonetHipError("%s supports Cin0<=16 -> 64 -> 128 -> 256 -> [320] -> 384 only" % who)
    dev = _same_device(w1, w2, w3, w4)
    stream = _ws(size_fn, dev)
    _launch(dev, None, fn, ptr(w1), ptr(w2), ptr(w3), ptr(w4), w1.shape[1], ptr(stream))
    return stream


def pointresnet_pack(w1, w2, w3, w4):
    """Pack the four [Cout][Cin] f32 weights of the first PointNet into the fused kernel's weight stream."""
    lib = _lib.load()
    return _pointresnet_pack((w1, w2, w3, w4), "pointresnet_fused", lib.sonet_pointresnet_pack_size, lib.sonet_pointresnet_pack)


def _chk_pointresnet(x, name, wstream, size_fn, affine):
    """The operands of a fused first PointNet: the weight stream of ``size_fn()`` bytes, the f32 points and the folded 832 x 2 affine."""
    _chk_member(wstream, "wstream", torch.uint8, (size_fn(),))
    _chk(x, name, torch.float32, 3)
    _chk(affine, "affine", torch.float32, 2)
    if tuple(affine.shape) != (832, 2):
        raise SonetHipError("affine must be 832 x 2 (scale, shift)")


def pointresnet_fused(x, wstream, affine, want_p16=False):
    """x B x Cin0 x L f32 -> B x 384 x L f32 (whole first PointNet, eval BN folded into ``affine`` 832 x 2).
    want_p16: -> (y, P16 planes of y), written by the same launch (the operand format of ``pointmlp_h3p``)."""
    _chk_pointresnet(x, "x", wstream, _lib.load().sonet_pointresnet_pack_size, affine)
    dev = _same_device(x, wstream, affine)
    B, Cin0, L = x.shape
    only = want_p16 == "only"                   # -> (None, planes): y is never written in f32 (P16.float() decodes the planes)
    y = None if only else torch.empty((B, 384, L), dtype=torch.float32, device=dev)
    yp = p16_empty(B, 384, L, dev) if want_p16 else None
    if B * L == 0:
        return (y, yp) if want_p16 else y
    _range_arm("pointresnet_fused_L%d" % L)
    name = "pointresnet_fused%s_L%d" % ("_p16only" if only else "_p16" if want_p16 else "", L)
    if want_p16:
        _launch(dev, name, _lib.load().sonet_pointresnet_fused_p16_f32, ptr(x), Cin0, ptr(wstream), ptr(affine), ptr(y), ptr(yp.data), B, L)
    else:
        _launch(dev, name, _lib.load().sonet_pointresnet_fused_f32, ptr(x), Cin0, ptr(wstream), ptr(affine), ptr(y), B, L)
    return (y, yp) if want_p16 else y


def pointresnet_fused_pool(sg, wstream, affine, M, want_p16=False):
    """First PointNet + per-node max-pool in one pass over node-sorted points (``sg`` = som_sort_group result)
    -> B x 384 x M f32.  want_p16: -> (that, ``P16`` 1 x 384 x Lm): the same map pre-split on the flat column axis of the node-level stage."""
    x_sorted = sg["x_aug_sorted"]
    _chk_sort_group(sg, M)
    _chk_pointresnet(x_sorted, "x_sorted", wstream, _lib.load().sonet_pointresnet_pack_size, affine)
    dev = _same_device(x_sorted, wstream, affine, sg["ids_sorted"], sg["pos0"], sg["node_off"], sg["count"])
    B, Cin0, L = x_sorted.shape
    lib = _lib.load()
    ws = _ws(lib.sonet_pointresnet_pool_ws_size, dev, B, L, int(M))
    out = torch.empty((B, 384, int(M)), dtype=torch.float32, device=dev)
    outp = p16_flat(384, node_stage_columns(B, int(M)), B * int(M), dev) if want_p16 else None
    _range_arm("pointresnet_fused_pool_L%d" % L)
    args = (ptr(x_sorted), Cin0, ptr(wstream), ptr(affine), ptr(sg["ids_sorted"]), ptr(sg["pos0"]), ptr(sg["node_off"]), ptr(sg["count"]), ptr(ws), ptr(out))
    if want_p16:
        _launch(dev, "pointresnet_fused_pool_L%d" % L, lib.sonet_pointresnet_fused_pool_p16_f32, *args, ptr(outp.data), B, L, int(M))
    else:
        _launch(dev, "pointresnet_fused_pool_L%d" % L, lib.sonet_pointresnet_fused_pool_f32, *args, B, L, int(M))
    return (out, outp) if want_p16 else out


def pointresnet_bf16_pack(w1, w2, w3, w4):
    """Weight stream of the fused bf16 first PointNet (``sonet_pointresnet_bf16_pack``)."""
    lib = _lib.load()
    return _pointresnet_pack((w1, w2, w3, w4), "pointresnet_bf16", lib.sonet_pointresnet_bf16_pack_size, lib.sonet_pointresnet_bf16_pack)


def pointresnet_bf16(x, wstream, affine):
    """x B x Cin0 x L f32 -> B x 384 x L bfloat16: whole first PointNet in bf16 (eval BN folded into ``affine`` 832 x 2)."""
    _chk_pointresnet(x, "x", wstream, _lib.load().sonet_pointresnet_bf16_pack_size, affine)
    dev = _same_device(x, wstream, affine)
    B, Cin0, L = x.shape
    y = torch.empty((B, 384, L), dtype=torch.bfloat16, device=dev)
    if y.numel() == 0:
        return y
    _launch(dev, "pointresnet_bf16_L%d" % L, _lib.load().sonet_pointresnet_bf16, ptr(x), Cin0, ptr(wstream), ptr(affine), ptr(y), B, L)
    return y


def pointresnet_bf16_pool(sg, wstream, affine, M):
    """bf16 first PointNet + per-node max-pool in one pass over node-sorted points (``sg`` = som_sort_group result)
    -> B x 384 x M f32 holding bf16-representable values (the maxima of the bf16 features the store variant writes)."""
    x_sorted = sg["x_aug_sorted"]
    _chk_sort_group(sg, M)
    _chk_pointresnet(x_sorted, "x_sorted", wstream, _lib.load().sonet_pointresnet_bf16_pack_size, affine)
    dev = _same_device(x_sorted, wstream, affine, sg["ids_sorted"], sg["pos0"], sg["node_off"], sg["count"])
    B, Cin0, L = x_sorted.shape
    lib = _lib.load()
    ws = _ws(lib.sonet_pointresnet_bf16_pool_ws_size, dev, B, L, int(M))
    out = torch.empty((B, 384, int(M)), dtype=torch.float32, device=dev)
    _launch(dev, "pointresnet_bf16_pool_L%d" % L, lib.sonet_pointresnet_bf16_pool, ptr(x_sorted), Cin0, ptr(wstream), ptr(affine), ptr(sg["ids_sorted"]),
            ptr(sg["pos0"]), ptr(sg["node_off"]), ptr(sg["count"]), ptr(ws), ptr(out), B, L, int(M))
    return out


@_consumes_rider
def channel_stats(y):
    """per-channel (mean, biased var) over (B, L) of y B x C x L (f32 or bf16 storage; f64 sums either way)."""
    _chk(y, "y", dim=3)
    if y.dtype not in (torch.float32, torch.bfloat16):
        raise SonetHipError("channel_stats: float32 or bfloat16, got %s" % y.dtype)
    dev = _same_device(y)
    B, C, L = y.shape
    ws = torch.empty((2 * C,), dtype=torch.float64, device=dev)
    mean = torch.empty((C,), dtype=torch.float32, device=dev)
    var = torch.empty((C,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    fn = _by_dtype(lib, "sonet_channel_stats", y)
    _launch(dev, "channel_stats" if y.dtype == torch.float32 else "channel_stats_bf16", fn, ptr(y), B, C, L, ptr(ws), ptr(mean), ptr(var),
            what="sonet_channel_stats")
    return mean, var


def channel_affine_act_(y, scale, shift, relu):
    _chk(y, "y", torch.float32, 3)
    B, C, L = y.shape
    _chk_cvec(C, scale=scale, shift=shift)
    dev = _same_device(y, scale, shift)
    _launch(dev, "channel_affine_act", _lib.load().sonet_channel_affine_act_f32, ptr(y), ptr(scale), ptr(shift), int(bool(relu)), B, C, L)
    return y


def channel_affine_act(x, scale, shift, relu):
    """y = act(x * scale[c] + shift[c]) out of place, x B x C x L (f32 or bf16 storage)."""
    _chk(x, "x", dim=3)
    _chk_f32_or_bf16(x, "x")
    B, C, L = x.shape
    _chk_cvec(C, scale=scale, shift=shift)
    dev = _same_device(x, scale, shift)
    y = torch.empty_like(x)
    lib = _lib.load()
    fn = _by_dtype(lib, "sonet_channel_affine_act_out", x)
    _launch(dev, "channel_affine_act" if x.dtype == torch.float32 else "channel_affine_act_bf16", fn, ptr(x), ptr(scale), ptr(shift), int(bool(relu)), ptr(y),
            B, C, L, what="sonet_channel_affine_act_out")
    return y


def chunk_mean(h, k):
    """Mean over the k copies of a point: h B x C x (k N) f32 -> B x C x N = c * ((h[..., :N] + h[..., N:2N]) + h[..., 2N:]), c = 1/3 or 0.5
    (models/networks.py:331-336, the reference's order of operations)."""
    _chk(h, "h", torch.float32, 3)
    B, C, L = h.shape
    if k not in (1, 2, 3) or L % k:
        raise SonetHipError("chunk_mean: k in {1, 2, 3} and a length divisible by k")
    dev = _same_device(h)
    out = torch.empty((B, C, L // k), dtype=torch.float32, device=dev)
    _launch(dev, "chunk_mean", _lib.load().sonet_chunk_mean_f32, ptr(h), ptr(out), B * C, L // k, int(k))
    return out


_CONST = {}


def const_vec(C, value, device):
    """Cached constant [C] f32 vector (ones / zeros for the kernels' scale / shift arguments)."""
    key = (int(C), float(value), str(device))
    t = _CONST.get(key)
    if t is None:
        t = torch.full((int(C),), float(value), dtype=torch.float32, device=device)
        _CONST[key] = t
    return t


def _rider_done():
    """After a statistics-producing call: the rider was consumed by its finalize launch -- or, if the call failed before launching,
    must not linger for an unrelated later launch."""
    if getattr(_tls, "rider_armed", None) is not None:
        _lib.load().sonet_bn_rider_set(None, None, 0.0, 0.0, 0.0, None, None, None, None, None)
        _tls.rider_armed = None


def bn_rider(gamma, beta, eps, running_mean=None, running_var=None, momentum=0.0, unbias=1.0):
    """Arm the "BatchNorm rider" (``sonet_bn_rider_set``) for the NEXT statistics-producing call of this thread (``pointmlp_stats``,
    ``pointmlp_h3p(stats=True)``, ``channel_stats``): its finalize launch also writes (invstd, scale, shift) -- ``bn_fwd_coeffs`` -- and,
    given the running statistics, updates them in place -- ``bn_running_update_`` --, operation for operation.  -> (invstd, scale, shift)
    tensors that call will fill."""
    dev = _same_device(gamma, beta, running_mean, running_var)
    C = gamma.numel()
    out = torch.empty((3, C), dtype=torch.float32, device=dev)
    if running_mean is not None:
        for t, n in ((running_mean, "running_mean"), (running_var, "running_var")):
            _chk(t, n, torch.float32, 1)
    g_, b_ = gamma.detach().contiguous(), beta.detach().contiguous()
    check(_lib.load().sonet_bn_rider_set(ptr(g_), ptr(b_), float(eps), float(momentum), float(unbias),
                                         ptr(running_mean), ptr(running_var), ptr(out[0]), ptr(out[1]), ptr(out[2])), "sonet_bn_rider_set")
    _tls.rider_armed = (g_, b_, out)                   # (keeps the operands alive until the statistics call has consumed the rider)
    if running_mean is not None:
        # written through raw pointers by the coming launch: move the version counters as an in-place aten op would
        torch.autograd.graph.increment_version(running_mean)
        torch.autograd.graph.increment_version(running_var)
    return out[0], out[1], out[2]


def bn_fwd_coeffs(mean, var, gamma, beta, eps):
    """-> (invstd, scale, shift) of training BatchNorm, one launch."""
    _chk(mean, "mean")
    C = mean.numel()
    _chk_cvec(C, mean=mean, var=var, gamma=gamma, beta=beta)
    dev = _same_device(mean, var, gamma, beta)
    out = torch.empty((3, C), dtype=torch.float32, device=dev)
    _launch(dev, None, _lib.load().sonet_bn_fwd_coeffs_f32, ptr(mean), ptr(var), ptr(gamma.detach().contiguous()), ptr(beta.detach().contiguous()), float(eps),
            C, ptr(out[0]), ptr(out[1]), ptr(out[2]))
    return out[0], out[1], out[2]


def bn_bwd_coeffs(sums, mean, invstd, gamma, n):
    """sums [2C] f64 of pointwise_bwd_stats -> (a, b, c0, g_gamma, g_beta), one launch."""
    _chk(mean, "mean")
    C = mean.numel()
    _chk_cvec(C, mean=mean, invstd=invstd, gamma=gamma)
    _chk(sums, "sums", torch.float64)
    if sums.numel() != 2 * C:
        raise SonetHipError("sums must hold 2 C = %d elements, got %d" % (2 * C, sums.numel()))
    dev = _same_device(sums, mean, invstd, gamma)
    out = torch.empty((5, C), dtype=torch.float32, device=dev)
    _launch(dev, None, _lib.load().sonet_bn_bwd_coeffs_f32, ptr(sums), ptr(mean), ptr(invstd), ptr(gamma.detach().contiguous()), float(n), C, ptr(out[0]),
            ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(out[4]))
    return out[0], out[1], out[2], out[3], out[4]


def pointwise_bwd_stats(gy, raw, scale, shift, relu, want_sums=False):
    """-> (s1, s2) float64 [C]: sum gy*mask, sum gy*mask*raw over (b, l); mask = (raw*scale+shift > 0) if relu."""
    _chk(gy, "gy", dim=3)
    _chk_f32_or_bf16(gy, "gy")
    _chk(raw, "raw", gy.dtype, 3)
    if raw.shape != gy.shape:
        raise SonetHipError("raw must have gy's shape %s, got %s" % (tuple(gy.shape), tuple(raw.shape)))
    B, C, L = gy.shape
    _chk_cvec(C, scale=scale, shift=shift)
    dev = _same_device(gy, raw, scale, shift)
    sums = torch.empty((2 * C,), dtype=torch.float64, device=dev)
    lib = _lib.load()
    fn = _by_dtype(lib, "sonet_pointwise_bwd_stats", gy)
    _launch(dev, "pointwise_bwd_stats" if gy.dtype == torch.float32 else "pointwise_bwd_stats_bf16", fn, ptr(gy), ptr(raw), ptr(scale), ptr(shift),
            int(bool(relu)), B, C, L, ptr(sums), what="sonet_pointwise_bwd_stats")
    if want_sums:
        return sums
    return sums[:C], sums[C:]


def pointwise_bwd_apply(gy, raw, scale, shift, relu, a, b, c0):
    """g_raw = a[c] * (gy * mask) + b[c] * raw + c0[c]."""
    _chk(gy, "gy", dim=3)
    _chk_f32_or_bf16(gy, "gy")
    _chk(raw, "raw", gy.dtype, 3)
    if raw.shape != gy.shape:
        raise SonetHipError("raw must have gy's shape %s, got %s" % (tuple(gy.shape), tuple(raw.shape)))
    B, C, L = gy.shape
    _chk_cvec(C, scale=scale, shift=shift, a=a, b=b, c0=c0)
    dev = _same_device(gy, raw, scale, shift, a, b, c0)
    out = torch.empty_like(gy)
    lib = _lib.load()
    fn = _by_dtype(lib, "sonet_pointwise_bwd_apply", gy)
    _launch(dev, "pointwise_bwd_apply" if gy.dtype == torch.float32 else "pointwise_bwd_apply_bf16", fn, ptr(gy), ptr(raw), ptr(scale), ptr(shift),
            int(bool(relu)), ptr(a), ptr(b), ptr(c0), ptr(out), B, C, L, what="sonet_pointwise_bwd_apply")
    return out


NODESUM_MAX_NODES = 1024               # include/sonet_hip.h: sonet_pointwise_bwd_apply_nodesum_f32 (as sonet_node_gather_bwd_*)


def pointwise_bwd_apply_nodesum_tile():
    """Columns per tile of ``pointwise_bwd_apply_nodesum``'s pass (the per-node sums are carried from tile to tile)."""
    return int(_lib.load().sonet_pointwise_bwd_apply_nodesum_tile())


def pointwise_bwd_apply_nodesum(gy, raw, scale, shift, relu, a, b, c0, ids, M):
    """``pointwise_bwd_apply`` and ``node_gather_bwd`` of its result in one pass over (gy, raw): -> (g_raw B x C x L, gz B x C x M) with
    gz[b][c][m] = the sum of g_raw[b][c][l] over the columns with ids[b][l] == m in ascending column order (ids B x L i32; outside
    [0, M): nowhere).  The bits of the two launches; f32 only; M <= 1024."""
    # (sizes first -- attribute checks that need no device --, then the tensors themselves)
    if not isinstance(gy, torch.Tensor) or gy.dim() != 3:
        raise SonetHipError("gy must be a 3-D torch.Tensor")
    B, C, L = gy.shape
    M = int(M)
    if M <= 0 or M > NODESUM_MAX_NODES:
        raise SonetHipError("pointwise_bwd_apply_nodesum: 1 <= M <= %d, got %d" % (NODESUM_MAX_NODES, M))
    _chk_member(ids, "ids", torch.int32, (B, L))
    _chk(gy, "gy", torch.float32, 3)
    _chk(raw, "raw", torch.float32, 3)
    if raw.shape != gy.shape:
        raise SonetHipError("raw must have gy's shape %s, got %s" % (tuple(gy.shape), tuple(raw.shape)))
    _chk_cvec(C, scale=scale, shift=shift, a=a, b=b, c0=c0)
    dev = _same_device(gy, raw, scale, shift, a, b, c0, ids)
    lib = _lib.load()
    g_raw = torch.empty_like(gy)
    gz = torch.empty((B, C, M), dtype=torch.float32, device=dev)
    ws = _ws(lib.sonet_pointwise_bwd_apply_nodesum_ws_size, dev, B, M, L)
    _launch(dev, "pointwise_bwd_apply_nodesum", lib.sonet_pointwise_bwd_apply_nodesum_f32, ptr(gy), ptr(raw), ptr(scale), ptr(shift), int(bool(relu)), ptr(a),
            ptr(b), ptr(c0), ptr(ids), M, ptr(g_raw), ptr(gz), ptr(ws), B, C, L)
    return g_raw, gz


P16_ONLY = _flag("P16_ONLY")        # segmenter: the fused first PointNet writes only the P16 planes of first_pn_out
POOLED_DGRAD_MFMA = _flag("POOLED_DGRAD_MFMA")        # bf16 outputs: the dense-tile product on the matrix cores (sonet_pooled_dgrad_mfma_bf16) when the shape allows


def pooled_dgrad_mfma_ok(C, C1, C2, L):
    ct = (C1 + C2 + 31) // 32
    return POOLED_DGRAD_MFMA and L % 2 == 0 and C % 16 == 0 and C <= 384 and ct % 2 == 0 and ct <= 12


# the sparse input gradient of the pooled layer on node-sorted columns (f32-class training): the column-0 part of the gradient (empty nodes) and
# the BatchNorm-backward sums of the layer that produced x2 can ride on the store of the launch (sonet_pooled_dgrad_tail_f32) instead of being two
# scatter_add launches and a statistics pass over (gy, raw) of that layer.  OFF: measured slower -- 1.24 ms against 1.00 ms for the three
# launches apart (the store phase reads raw in 128-byte pieces from five workgroups per CU; docs/findings.md R5.14); kept as a tested record.
POOLED_DGRAD_TAIL = _flag("POOLED_DGRAD_TAIL", "0")


def pooled_dgrad_tail_ok(C1, C2, out_dtype):
    return POOLED_DGRAD_TAIL and out_dtype == torch.float32 and (C1 + C2) % 4 == 0 and variants_only()


def pooled_dgrad(g_pooled, pos_i32, weight2d, C1, C2, L, out_dtype=torch.float32, wt_pack=None, col0=None, pos0=None, below=None):
    """Sparse W^T . g for a gradient that exists only at the pooled positions: g_pooled, pos B x C x M -> (gx1 B x C1 x L, gx2 B x C2 x L).
    wt_pack (bf16 outputs only): pointmlp_pack(W^T, "bf16") -> the matrix-core kernel (g and W rounded to bf16).
    col0 (B x (C1 + C2), f32) with pos0 (B, i32): gx[b][:, pos0[b]] += col0[b], by the store of the launch (``pooled_dgrad_tail_ok``).
    below = (raw B x C2 x L, sc, sh, relu): gx2 is gy of the BatchNorm layer whose raw output is ``raw`` -> a third result, its
    BatchNorm-backward sums (float64 [2 C2], the layout of ``pointwise_bwd_stats(..., want_sums=True)``), taken from the tiles as they are stored."""
    _chk(g_pooled, "g_pooled", torch.float32, 3)
    _chk(pos_i32, "pos", torch.int32, 3)
    _chk(weight2d, "weight", torch.float32, 2)
    dev = _same_device(g_pooled, pos_i32, weight2d)
    B, C, M = g_pooled.shape
    # (the kernels index pos by g's extents and W by C x (C1 + C2): a short pos or weight would be read past its end)
    if tuple(pos_i32.shape) != (B, C, M):
        raise SonetHipError("pooled_dgrad: pos must have g_pooled's shape %s, got %s" % ((B, C, M), tuple(pos_i32.shape)))
    if int(C1) <= 0 or int(C2) < 0 or int(L) <= 0:
        raise SonetHipError("pooled_dgrad: C1 > 0, C2 >= 0 and L > 0, got C1=%d C2=%d L=%d" % (C1, C2, L))
    if tuple(weight2d.shape) != (C, C1 + C2):
        raise SonetHipError("pooled_dgrad: weight must be C x (C1 + C2) = %s, got %s" % ((C, C1 + C2), tuple(weight2d.shape)))
    weight2d = _aligned16(weight2d)                               # (16-byte loads of W when (C1 + C2) % 4 == 0)
    lib = _lib.load()
    ws = _ws(lib.sonet_pooled_dgrad_ws_size, dev, B, C, M, int(L))
    gx1 = torch.empty((B, C1, int(L)), dtype=out_dtype, device=dev)
    gx2 = torch.empty((B, C2, int(L)), dtype=out_dtype, device=dev) if C2 else None
    if col0 is not None or pos0 is not None or below is not None:
        if not variants_only():
            raise SonetHipError("pooled_dgrad: col0 / below ride on sonet_pooled_dgrad_tail_f32, a measured-slower record of the variants build "
                                "(SONET_HIP_LIB=%s)" % _lib.VARIANTS_PATH)
        if out_dtype != torch.float32 or (C1 + C2) % 4 or wt_pack is not None:
            raise SonetHipError("pooled_dgrad: col0 / below need f32 outputs and C1 + C2 a multiple of 4")
        if (col0 is None) != (pos0 is None):
            raise SonetHipError("pooled_dgrad: col0 and pos0 come together")
        if col0 is not None:
            _chk(col0, "col0", torch.float32, 2)
            _chk(pos0, "pos0", torch.int32, 1)
            if tuple(col0.shape) != (B, C1 + C2) or pos0.numel() != B:
                raise SonetHipError("pooled_dgrad: col0 must be B x (C1 + C2), pos0 B")
            _same_device(g_pooled, col0, pos0)
        raw = sc = sh = tws = sums = None
        relu = False
        if below is not None:
            raw, sc, sh, relu = below
            _chk(raw, "below raw", torch.float32, 3)
            _chk(sc, "below sc", torch.float32, 1)
            _chk(sh, "below sh", torch.float32, 1)
            if C2 == 0 or tuple(raw.shape) != (B, C2, int(L)) or sc.numel() != C2 or sh.numel() != C2:
                raise SonetHipError("pooled_dgrad: below = (raw B x C2 x L, sc, sh, relu) with C2 coefficients")
            _same_device(g_pooled, raw, sc, sh)
            tws = _ws(lib.sonet_pooled_dgrad_tail_ws_size, dev, B, C2, int(L))
            sums = torch.empty((2 * C2,), dtype=torch.float64, device=dev)
        _launch(dev, "pooled_dgrad_tail%s" % ("_sums" if below is not None else ""), lib.sonet_pooled_dgrad_tail_f32, ptr(g_pooled), ptr(pos_i32),
                ptr(weight2d), B, C, M, C1, C2, int(L), ptr(ws), ptr(gx1), ptr(gx2), ptr(col0), ptr(pos0), ptr(raw), ptr(sc), ptr(sh), int(bool(relu)),
                ptr(tws), ptr(sums))
        return (gx1, gx2, sums) if below is not None else (gx1, gx2)
    if wt_pack is not None and out_dtype == torch.bfloat16 and pooled_dgrad_mfma_ok(C, C1, C2, int(L)):
        if wt_pack.dtype != torch.int16 or wt_pack.numel() != lib.sonet_pointmlp_bf16_pack_size(C, (C1 + C2 + 31) // 32 * 32) // 2:
            raise SonetHipError("pooled_dgrad: wt_pack is not the bf16 pack of W^T")
        _launch(dev, "pooled_dgrad_mfma", lib.sonet_pooled_dgrad_mfma_bf16, ptr(g_pooled), ptr(pos_i32), ptr(wt_pack), B, C, M, C1, C2, int(L), ptr(ws),
                ptr(gx1), ptr(gx2))
        return gx1, gx2
    fn = lib.sonet_pooled_dgrad_f32 if out_dtype == torch.float32 else lib.sonet_pooled_dgrad_obf16
    _launch(dev, "pooled_dgrad", fn, ptr(g_pooled), ptr(pos_i32), ptr(weight2d), B, C, M, C1, C2, int(L), ptr(ws), ptr(gx1), ptr(gx2),
            what="sonet_pooled_dgrad")
    return gx1, gx2


def pooled_wgrad(g_pooled_t, pos_i32_t, x, xaff=None):
    """Sparse wgrad of the pooled last layer: g_pooled_t, pos_t B x M x C (TRANSPOSED entries), x B x Ci x L -> g_W C x Ci
    (= sum over clouds and entries of g * x[:, pos]; per-cloud partials summed in a fixed order).
    xaff = (scale, shift, relu) (f32 x): x holds the RAW output of a BatchNorm layer, normalised on its way into the LDS."""
    _chk(g_pooled_t, "g_pooled_t", torch.float32, 3)
    _chk(pos_i32_t, "pos_t", torch.int32, 3)
    _chk(x, "x", dim=3)
    dev = _same_device(g_pooled_t, pos_i32_t, x)
    B, M, C = g_pooled_t.shape
    Ci, L = x.shape[1], x.shape[2]
    # (the kernel indexes pos by g's extents and x by g's cloud count: a short pos or x would be read past its end)
    if tuple(pos_i32_t.shape) != (B, M, C):
        raise SonetHipError("pooled_wgrad: pos_t must have g_pooled_t's shape %s, got %s" % ((B, M, C), tuple(pos_i32_t.shape)))
    if x.shape[0] != B:
        raise SonetHipError("pooled_wgrad: x must hold B = %d clouds, got shape %s" % (B, tuple(x.shape)))
    part = torch.empty((B, C, Ci), dtype=torch.float32, device=dev)
    lib = _lib.load()
    if xaff is not None:
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise SonetHipError("pooled_wgrad: float32 or bfloat16 rows")
        fnx = lib.sonet_pooled_wgrad_xaff_f32 if x.dtype == torch.float32 else lib.sonet_pooled_wgrad_xaff_xbf16
        _launch(dev, "pooled_wgrad_xaff", fnx, ptr(g_pooled_t), ptr(pos_i32_t), ptr(x), B, C, M, Ci, L, ptr(part),
                *_xaff3(xaff, Ci, "pooled_wgrad: xaff needs Ci", x), what="sonet_pooled_wgrad_xaff")
        return part.sum(0)
    fn = lib.sonet_pooled_wgrad_f32 if x.dtype == torch.float32 else lib.sonet_pooled_wgrad_xbf16
    _launch(dev, "pooled_wgrad", fn, ptr(g_pooled_t), ptr(pos_i32_t), ptr(x), B, C, M, Ci, L, ptr(part), what="sonet_pooled_wgrad")
    return part.sum(0)


def linear_act(x, weight, scale, shift, relu):
    """x B x Cin, weight Cout x Cin -> act((x @ weight^T) * scale + shift), B x Cout (exact f32)."""
    _chk(x, "x", torch.float32, 2)
    _chk(weight, "weight", torch.float32, 2)
    dev = _same_device(x, weight, scale, shift)
    B, Cin = x.shape
    Cout = weight.shape[0]
    if weight.shape[1] != Cin:
        raise SonetHipError("linear_act: x B x Cin, weight Cout x Cin, got %s and %s" % (tuple(x.shape), tuple(weight.shape)))
    if scale.numel() != Cout or shift.numel() != Cout or scale.dtype != torch.float32 or shift.dtype != torch.float32:
        raise SonetHipError("linear_act: scale / shift must hold Cout = %d float32 elements" % Cout)
    x, weight = _aligned16(x), _aligned16(weight)                 # (16-byte loads when Cin % 4 == 0; the C entry refuses misaligned ones)
    y = torch.empty((B, Cout), dtype=torch.float32, device=dev)
    _launch(dev, "linear_act_%dx%d" % (Cin, Cout), _lib.load().sonet_linear_act_f32, ptr(x), ptr(weight), ptr(scale), ptr(shift), int(bool(relu)), ptr(y), B,
            Cin, Cout)
    return y


FC_HEAD = _flag("FC_HEAD")          # training: the heads' B x C layers on sonet_fc_* (one forward, two backward launches per layer)


def fc_head_ok(x, weight):
    """The training kernels of the heads' FC layers take this (x B x Cin, weight Cout x Cin)?"""
    return (FC_HEAD and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.is_cuda
            and 1 <= x.shape[0] <= 128 and x.shape[1] % 4 == 0 and weight.shape[0] % 4 == 0 and x.shape[1] >= 4 and weight.shape[0] >= 4)


def fc_bn_act_fwd(x, weight, bias, gamma, beta, running_mean, running_var, momentum, eps, relu):
    """Linear + BatchNorm1d (batch statistics; gamma None: no normalisation) + ReLU, training forward: -> (y, xhat, invstd); the running
    statistics are updated in place (models/layers.py:123-166)."""
    _chk(x, "x", torch.float32, 2)
    _chk(weight, "weight", torch.float32, 2)
    dev = _same_device(x, weight)
    B, Cin = x.shape
    Cout = weight.shape[0]
    y = torch.empty((B, Cout), dtype=torch.float32, device=dev)
    xhat = torch.empty((B, Cout), dtype=torch.float32, device=dev) if gamma is not None else None
    invstd = torch.empty((Cout,), dtype=torch.float32, device=dev) if gamma is not None else None
    _launch(dev, "fc_bn_act_fwd_%dx%d" % (Cin, Cout), _lib.load().sonet_fc_bn_act_fwd_f32, ptr(x), ptr(weight), ptr(bias), ptr(gamma), ptr(beta),
            ptr(running_mean), ptr(running_var), float(momentum), float(eps), int(bool(relu)), B, Cin, Cout, ptr(y), ptr(xhat), ptr(invstd))
    return y, xhat, invstd


def fc_bn_act_bwd(gy, y, xhat, invstd, gamma, x, relu, want_dw=True):
    """-> (dz, dW, dbias, dgamma, dbeta): the layer's backward up to its own parameters (dgamma / dbeta None without a norm)."""
    _chk(gy, "gy", torch.float32, 2)
    dev = _same_device(gy, x)
    B, Cout = gy.shape
    Cin = x.shape[1]
    dz = torch.empty((B, Cout), dtype=torch.float32, device=dev)
    dW = torch.empty((Cout, Cin), dtype=torch.float32, device=dev) if want_dw else None
    vec = torch.empty((3, Cout), dtype=torch.float32, device=dev)
    has_bn = gamma is not None
    _launch(dev, "fc_bn_act_bwd_%dx%d" % (Cin, Cout), _lib.load().sonet_fc_bn_act_bwd_f32, ptr(gy), ptr(y), ptr(xhat), ptr(invstd), ptr(gamma), ptr(x),
            int(bool(relu)), B, Cin, Cout, ptr(dz), ptr(dW), ptr(vec[0]), ptr(vec[1]) if has_bn else None, ptr(vec[2]) if has_bn else None)
    return dz, dW, vec[0], (vec[1] if has_bn else None), (vec[2] if has_bn else None)


def fc_dx(dz, weight):
    """dx B x Cin = dz (B x Cout) . weight (Cout x Cin)."""
    _chk(dz, "dz", torch.float32, 2)
    _chk(weight, "weight", torch.float32, 2)
    dev = _same_device(dz, weight)
    B, Cout = dz.shape
    Cin = weight.shape[1]
    dx = torch.empty((B, Cin), dtype=torch.float32, device=dev)
    _launch(dev, "fc_dx_%dx%d" % (Cin, Cout), _lib.load().sonet_fc_dx_f32, ptr(dz), ptr(weight), B, Cin, Cout, ptr(dx))
    return dx


def chamfer_nn(q, db):
    """q B x 3 x Nq, db B x 3 x Nd -> B x Nq i32 nearest database index."""
    _chk(q, "q", torch.float32, 3)
    _chk(db, "db", torch.float32, 3)
    dev = _same_device(q, db)
    B, _, Nq = q.shape
    Nd = db.shape[2]
    nn = torch.empty((B, Nq), dtype=torch.int32, device=dev)
    _launch(dev, "chamfer_nn", _lib.load().sonet_chamfer_nn_f32, ptr(q), ptr(db), ptr(nn), B, Nq, Nd)
    return nn


# ------------------------------------------------------------------------------------------ fused Chamfer loss
class ChamferTerms:
    """Device tensors of one ``chamfer_terms`` call: nn_pg B x M i32 and nn_gp B x N i32 (None unless asked for), elem_fwd B x M f32 and
    elem_bwd B x N f32 (None unless asked for), sums B x 2 f64 (per cloud: sum of elem_fwd, sum of elem_bwd); M and N the point counts."""
    __slots__ = ("nn_pg", "nn_gp", "elem_fwd", "elem_bwd", "sums", "M", "N")


def _chk_clouds(pred, gt):
    """pred B x 3 x M, gt B x 3 x N: contiguous f32 CUDA tensors on one device; only the predicted cloud may ask for a gradient."""
    _chk(pred, "pred", torch.float32, 3)
    _chk(gt, "gt", torch.float32, 3)
    if pred.shape[1] != 3 or gt.shape[1] != 3:
        raise SonetHipError("pred and gt must have 3 channels (B x 3 x points), got %s and %s" % (tuple(pred.shape), tuple(gt.shape)))
    if pred.shape[0] != gt.shape[0]:
        raise SonetHipError("pred and gt must hold the same number of clouds, got B = %d and %d" % (pred.shape[0], gt.shape[0]))
    if gt.requires_grad:
        raise SonetHipError("gt must not require a gradient: the Chamfer loss differentiates the predicted cloud only")
    B, _, M = pred.shape
    N = gt.shape[2]
    if B < 1 or M < 1 or N < 1 or B > 65535:
        raise SonetHipError("chamfer: need 1 <= B <= 65535, M >= 1, N >= 1, got B=%d M=%d N=%d" % (B, M, N))
    return _same_device(pred, gt), B, M, N


def chamfer_terms(pred, gt, want_nn=True, want_elems=True):
    """pred B x 3 x M, gt B x 3 x N f32 -> ``ChamferTerms`` (include/sonet_hip.h: sonet_chamfer_loss_f32): both nearest-neighbour
    directions, the robust_norm elements and their per-cloud float64 sums from one launch plus a small one for the sums."""
    dev, B, M, N = _chk_clouds(pred, gt)
    lib = _lib.load()
    r = ChamferTerms()
    r.M, r.N = M, N
    r.nn_pg = r.nn_gp = r.elem_fwd = r.elem_bwd = None
    if want_nn:
        nn = torch.empty((B * (M + N),), dtype=torch.int32, device=dev)
        r.nn_pg, r.nn_gp = nn[:B * M].view(B, M), nn[B * M:].view(B, N)
    if want_elems:
        el = torch.empty((B * (M + N),), dtype=torch.float32, device=dev)
        r.elem_fwd, r.elem_bwd = el[:B * M].view(B, M), el[B * M:].view(B, N)
    f64 = torch.empty((2 * B + lib.sonet_chamfer_loss_ws_size(B, M, N) // 8,), dtype=torch.float64, device=dev)
    r.sums = f64[:2 * B].view(B, 2)
    _launch(dev, "chamfer_loss", lib.sonet_chamfer_loss_f32, ptr(pred), ptr(gt), ptr(r.nn_pg), ptr(r.nn_gp), ptr(r.elem_fwd), ptr(r.elem_bwd), ptr(r.sums),
            ptr(f64[2 * B:]), B, M, N)
    return r


def chamfer_grad(pred, gt, terms, gscale):
    """d(gf * forward_loss + gb * backward_loss) / d pred at the indices and elements of ``terms``; gscale: the two f32 (gf, gb) on the
    device -> (dpred B x 3 x M f32, bad 1 i32: index entries outside their range, which contribute nothing).  No host sync."""
    dev, B, M, N = _chk_clouds(pred, gt)
    if terms.nn_pg is None or terms.elem_fwd is None:
        raise SonetHipError("chamfer_grad needs the indices and the elements (chamfer_terms(want_nn=True, want_elems=True))")
    for t, name, dtype, shape in ((terms.nn_pg, "nn_pg", torch.int32, (B, M)), (terms.nn_gp, "nn_gp", torch.int32, (B, N)),
                                  (terms.elem_fwd, "elem_fwd", torch.float32, (B, M)), (terms.elem_bwd, "elem_bwd", torch.float32, (B, N)),
                                  (gscale, "gscale", torch.float32, (2,))):
        _chk(t, name, dtype)
        if tuple(t.shape) != shape:
            raise SonetHipError("%s must have shape %s, got %s" % (name, shape, tuple(t.shape)))
    _same_device(pred, terms.nn_pg, terms.nn_gp, terms.elem_fwd, terms.elem_bwd, gscale)
    dpred = torch.empty((B, 3, M), dtype=torch.float32, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    _launch(dev, "chamfer_grad", _lib.load().sonet_chamfer_grad_f32, ptr(pred), ptr(gt), ptr(terms.nn_pg), ptr(terms.nn_gp), ptr(terms.elem_fwd),
            ptr(terms.elem_bwd), ptr(gscale), ptr(dpred), ptr(bad), B, M, N)
    return dpred, bad


class _ChamferLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        t = chamfer_terms(pred, gt)
        B = pred.shape[0]
        tot = t.sums.sum(dim=0)                                       # f64 [2], on the device
        forward_loss, backward_loss = (tot[0] / (B * t.M)).float(), (tot[1] / (B * t.N)).float()
        forward_arr, backward_arr = (t.sums[:, 0] / t.M).float(), (t.sums[:, 1] / t.N).float()
        ctx.save_for_backward(pred, gt, t.nn_pg, t.nn_gp, t.elem_fwd, t.elem_bwd)
        ctx.mark_non_differentiable(forward_arr, backward_arr)
        return forward_loss, backward_loss, forward_arr, backward_arr

    @staticmethod
    def backward(ctx, gf, gb, _ga, _gb):
        pred, gt, nn_pg, nn_gp, elem_fwd, elem_bwd = ctx.saved_tensors
        t = ChamferTerms()
        t.nn_pg, t.nn_gp, t.elem_fwd, t.elem_bwd, t.M, t.N = nn_pg, nn_gp, elem_fwd, elem_bwd, pred.shape[2], gt.shape[2]
        zero = None
        if gf is None or gb is None:
            zero = torch.zeros((), dtype=torch.float32, device=pred.device)
        gscale = torch.stack([zero if gf is None else gf.float(), zero if gb is None else gb.float()])
        dpred, _bad = chamfer_grad(pred, gt, t, gscale)
        return dpred, None


def chamfer_loss(pred, gt):
    """The Chamfer loss of models/losses.py:237-290 as one operator: pred B x 3 x M (may require a gradient), gt B x 3 x N ->
    (forward_loss, backward_loss: f32 scalars, differentiable with respect to pred; forward_loss_array, backward_loss_array: B f32, not
    differentiable).  The sums are float64 on the device and rounded once; the backward is one ``sonet_chamfer_grad_f32`` call."""
    _chk_clouds(pred, gt)
    return _ChamferLoss.apply(pred, gt)


# ------------------------------------------------------------------------------------------ Chamfer loss pyramid
# Extents of csrc/chamfer.hip (sonet_chamfer_pyramid_max_n / _max_m): a cloud's gt keys are sorted in one LDS array, and a predicted
# point's index sits in the upper 16 bits of a key.
CHAMFER_PYRAMID_MAX_LEVELS = 3
CHAMFER_PYRAMID_MAX_N = 8192
CHAMFER_PYRAMID_MAX_M = 65535


def chamfer_pyramid_supported(Ms, N):
    """Sizes the pyramid operator takes: 1 to 3 levels of 1 <= M_l <= CHAMFER_PYRAMID_MAX_M points, 1 <= N <= CHAMFER_PYRAMID_MAX_N."""
    return (1 <= len(Ms) <= CHAMFER_PYRAMID_MAX_LEVELS and all(1 <= int(M) <= CHAMFER_PYRAMID_MAX_M for M in Ms)
            and 1 <= int(N) <= CHAMFER_PYRAMID_MAX_N)


class ChamferPyramidTerms:
    """One ``chamfer_pyramid_terms`` call: ``levels`` a list of ``ChamferTerms`` (level l's ``sums`` is the B x 2 view ``sums[:, l]``),
    ``sums`` B x L x 2 f64, ``N`` the gt point count."""
    __slots__ = ("levels", "sums", "N")


def _chk_pyramid(preds, gt):
    """preds: 1 to 3 clouds B x 3 x M_l, gt B x 3 x N, each as ``_chk_clouds`` asks; sizes inside the exported extents."""
    if not isinstance(preds, (list, tuple)) or not 1 <= len(preds) <= CHAMFER_PYRAMID_MAX_LEVELS:
        raise SonetHipError("chamfer_pyramid: preds must be a list of 1 to %d predicted clouds" % CHAMFER_PYRAMID_MAX_LEVELS)
    dev = B = N = None
    for p in preds:
        dev, B, _, N = _chk_clouds(p, gt)
    _same_device(gt, *preds)
    Ms = [int(p.shape[2]) for p in preds]
    if not chamfer_pyramid_supported(Ms, N):
        raise SonetHipError("chamfer_pyramid: need M_l <= %d and N <= %d, got M=%s N=%d" % (CHAMFER_PYRAMID_MAX_M, CHAMFER_PYRAMID_MAX_N, Ms, N))
    return dev, B, Ms, N


def _ptr_array(ts):
    """The host array of device pointers a pyramid entry reads (None: a NULL entry)."""
    import ctypes
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _int_array(vs):
    import ctypes
    return (ctypes.c_int * len(vs))(*vs)


def chamfer_pyramid_terms(preds, gt, want_nn=True, want_elems=True):
    """preds: 1 to 3 clouds B x 3 x M_l, gt B x 3 x N f32 -> ``ChamferPyramidTerms`` (include/sonet_hip.h: sonet_chamfer_pyramid_loss_f32):
    what ``chamfer_terms(preds[l], gt)`` gives for every level, bit for bit, from one launch plus a small one for the sums."""
    dev, B, Ms, N = _chk_pyramid(preds, gt)
    L = len(Ms)
    lib = _lib.load()
    r = ChamferPyramidTerms()
    r.N, r.levels = N, []
    tot = B * (sum(Ms) + L * N)
    nn = torch.empty((tot,), dtype=torch.int32, device=dev) if want_nn else None
    el = torch.empty((tot,), dtype=torch.float32, device=dev) if want_elems else None
    f64 = torch.empty((2 * B * L + lib.sonet_chamfer_pyramid_ws_size(B, L, *(Ms + [0, 0])[:3], N) // 8,), dtype=torch.float64, device=dev)
    r.sums = f64[:2 * B * L].view(B, L, 2)
    off = 0
    for l, M in enumerate(Ms):
        t = ChamferTerms()
        t.M, t.N, t.sums = M, N, r.sums[:, l]
        t.nn_pg = t.nn_gp = t.elem_fwd = t.elem_bwd = None
        if want_nn:
            t.nn_pg, t.nn_gp = nn[off:off + B * M].view(B, M), nn[off + B * M:off + B * (M + N)].view(B, N)
        if want_elems:
            t.elem_fwd, t.elem_bwd = el[off:off + B * M].view(B, M), el[off + B * M:off + B * (M + N)].view(B, N)
        off += B * (M + N)
        r.levels.append(t)
    lv = r.levels
    _launch(dev, "chamfer_pyramid_loss", lib.sonet_chamfer_pyramid_loss_f32, _ptr_array(preds), ptr(gt), _ptr_array([t.nn_pg for t in lv]),
            _ptr_array([t.nn_gp for t in lv]), _ptr_array([t.elem_fwd for t in lv]), _ptr_array([t.elem_bwd for t in lv]), ptr(r.sums),
            ptr(f64[2 * B * L:]), B, L, _int_array(Ms), N)
    return r


def chamfer_pyramid_grad(preds, gt, terms, gscale):
    """d(sum over l of gf_l * forward_loss_l + gb_l * backward_loss_l) / d preds[l] at the indices and elements of ``terms`` (a
    ``ChamferPyramidTerms`` or a list of ``ChamferTerms``); gscale: L x 2 f32 (gf_l, gb_l) on the device -> (list of dpred_l B x 3 x M_l
    f32, bad L i32: per level the index entries outside their range, which contribute nothing).  One launch, no host sync; level l is
    ``chamfer_grad(preds[l], gt, terms.levels[l], gscale[l])`` bit for bit."""
    dev, B, Ms, N = _chk_pyramid(preds, gt)
    L = len(Ms)
    lv = terms.levels if isinstance(terms, ChamferPyramidTerms) else list(terms)
    if len(lv) != L:
        raise SonetHipError("chamfer_pyramid_grad: %d levels of terms for %d predicted clouds" % (len(lv), L))
    for t, M in zip(lv, Ms):
        if t.nn_pg is None or t.elem_fwd is None:
            raise SonetHipError("chamfer_pyramid_grad needs the indices and the elements (chamfer_pyramid_terms(want_nn=True, want_elems=True))")
        for x, name, dtype, shape in ((t.nn_pg, "nn_pg", torch.int32, (B, M)), (t.nn_gp, "nn_gp", torch.int32, (B, N)),
                                      (t.elem_fwd, "elem_fwd", torch.float32, (B, M)), (t.elem_bwd, "elem_bwd", torch.float32, (B, N))):
            _chk(x, name, dtype)
            if tuple(x.shape) != shape:
                raise SonetHipError("%s must have shape %s, got %s" % (name, shape, tuple(x.shape)))
        _same_device(gt, t.nn_pg, t.nn_gp, t.elem_fwd, t.elem_bwd)
    _chk(gscale, "gscale", torch.float32)
    if tuple(gscale.shape) != (L, 2):
        raise SonetHipError("gscale must have shape %s, got %s" % ((L, 2), tuple(gscale.shape)))
    _same_device(gt, gscale)
    flat = torch.empty((3 * B * sum(Ms),), dtype=torch.float32, device=dev)
    dpreds, off = [], 0
    for M in Ms:
        dpreds.append(flat[off:off + 3 * B * M].view(B, 3, M))
        off += 3 * B * M
    bad = torch.empty((L,), dtype=torch.int32, device=dev)
    _launch(dev, "chamfer_pyramid_grad", _lib.load().sonet_chamfer_pyramid_grad_f32, _ptr_array(preds), ptr(gt),
            _ptr_array([t.nn_pg for t in lv]), _ptr_array([t.nn_gp for t in lv]), _ptr_array([t.elem_fwd for t in lv]),
            _ptr_array([t.elem_bwd for t in lv]), ptr(gscale), _ptr_array(dpreds), ptr(bad), B, L, _int_array(Ms), N)
    return dpreds, bad


_pyramid_denominators = {}


def _pyramid_den(dev, Ms, N):
    """L x 2 f64 on ``dev``: (M_l, N) per level, what a cloud's two sums are divided by (made once per set of sizes: an H2D copy)."""
    key = (dev, tuple(Ms), N)
    den = _pyramid_denominators.get(key)
    if den is None:
        den = _pyramid_denominators[key] = torch.tensor([[float(M), float(N)] for M in Ms], dtype=torch.float64).to(dev)
    return den


class _ChamferPyramidLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, *preds):
        t = chamfer_pyramid_terms(list(preds), gt)
        B, L = gt.shape[0], len(preds)
        den = _pyramid_den(gt.device, [p.shape[2] for p in preds], t.N)
        arrays = (t.sums / den).float()                                  # B x L x 2: per cloud, the mean of its elements
        scalars = (t.sums.sum(dim=0) / (den * B)).float()                # L x 2: f64 sums on the device, rounded once
        saved = [gt]
        out = []
        for l in range(L):
            lv = t.levels[l]
            saved += [preds[l], lv.nn_pg, lv.nn_gp, lv.elem_fwd, lv.elem_bwd]
            out += [scalars[l, 0], scalars[l, 1], arrays[:, l, 0], arrays[:, l, 1]]
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(*[o for k, o in enumerate(out) if k % 4 >= 2])
        ctx.set_materialize_grads(False)
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        gt, L = saved[0], (len(saved) - 1) // 5
        preds, levels = [], []
        for l in range(L):
            p, nn_pg, nn_gp, elem_fwd, elem_bwd = saved[1 + 5 * l:6 + 5 * l]
            t = ChamferTerms()
            t.nn_pg, t.nn_gp, t.elem_fwd, t.elem_bwd, t.M, t.N = nn_pg, nn_gp, elem_fwd, elem_bwd, p.shape[2], gt.shape[2]
            preds.append(p)
            levels.append(t)
        gs = [grads[4 * l + d] for l in range(L) for d in (0, 1)]
        if any(g is None for g in gs):
            zero = torch.zeros((), dtype=torch.float32, device=gt.device)
            gs = [zero if g is None else g for g in gs]
        gscale = torch.stack([g.float() for g in gs]).view(L, 2)
        dpreds, _bad = chamfer_pyramid_grad(preds, gt, levels, gscale)
        return (None,) + tuple(dpreds)


def chamfer_pyramid_loss(preds, gt):
    """Every Chamfer term of an autoencoder step (models/autoencoder.py:83-98) as one operator: preds a list of 1 to 3 clouds
    B x 3 x M_l (each may require a gradient), gt B x 3 x N -> a list with, per level, (forward_loss, backward_loss: f32 scalars,
    differentiable with respect to preds[l]; forward_loss_array, backward_loss_array: B f32, not differentiable).  One
    ``sonet_chamfer_pyramid_loss_f32`` call forward, one ``sonet_chamfer_pyramid_grad_f32`` call backward, whatever outputs are used."""
    _chk_pyramid(preds, gt)
    out = _ChamferPyramidLoss.apply(gt, *preds)
    return [tuple(out[4 * l:4 * l + 4]) for l in range(len(preds))]


# ------------------------------------------------------------------------------------------ upconv3x3
# Tile extents of csrc/upconv.hip (include/sonet_hip.h SONET_UPCONV_*): a workgroup covers UPCONV_TILE_PIXELS consecutive low-resolution
# pixels of the flattened (b, i, j) axis and UPCONV_COUT_BLOCK output channels, and stages UPCONV_K_CHUNK input channels at a time.
UPCONV_TILE_PIXELS = 128
UPCONV_K_CHUNK = 16
UPCONV_COUT_BLOCK = 32
UPCONV_MAX_HW = 64


def upconv3x3_supported(Cin, Cout, H, W):
    """Shapes the fused up-convolution takes: any Cin >= 1, Cout a multiple of UPCONV_COUT_BLOCK, 1 <= H, W <= UPCONV_MAX_HW."""
    return Cin >= 1 and Cout >= UPCONV_COUT_BLOCK and Cout % UPCONV_COUT_BLOCK == 0 and 1 <= H <= UPCONV_MAX_HW and 1 <= W <= UPCONV_MAX_HW


def upconv3x3_pack(weight4d):
    """[Cout][Cin][3][3] f32 -> the up-convolution's pack (int32 tensor): the sixteen (parity, tap) 2x2 weights folded in float64, split
    into fp16(32 w) + residual, in MFMA A-fragment order; its trailer carries the largest magnitude for the range guard."""
    _chk(weight4d, "weight", torch.float32, 4)
    Cout, Cin, kh, kw = weight4d.shape
    if (kh, kw) != (3, 3):
        raise SonetHipError("upconv3x3_pack: a 3x3 kernel, got %dx%d" % (kh, kw))
    if not upconv3x3_supported(Cin, Cout, 1, 1):
        raise SonetHipError("upconv3x3_pack: Cout = %d is not a multiple of %d" % (Cout, UPCONV_COUT_BLOCK))
    dev = _same_device(weight4d)
    lib = _lib.load()
    wp = _pack_empty(lib, "upconv", Cin, Cout, dev)
    _launch(dev, None, lib.sonet_upconv3x3_pack_f32, ptr(weight4d), ptr(wp), Cin, Cout)
    return wp


def upconv3x3(x, wp, scale, shift, relu, Cout):
    """y = act(conv3x3_pad1(upsample2_nearest(x), w) * scale + shift) in one launch (models/layers.py:214-240, inference):
    x B x Cin x H x W f32 -> B x Cout x 2H x 2W f32; wp from ``upconv3x3_pack``; scale / shift per output channel (bias and eval-mode
    BatchNorm folded in).  fp16-split arithmetic: inside a ``range_scope`` the launch logs max |x| and the pack's max |w|."""
    _chk(x, "x", torch.float32, 4)
    B, Cin, H, W = x.shape
    Cout = int(Cout)
    if B < 1 or not upconv3x3_supported(Cin, Cout, H, W):
        raise SonetHipError("upconv3x3: unsupported shape B=%d Cin=%d Cout=%d H=%d W=%d (Cout %% %d == 0, 1 <= H, W <= %d)"
                            % (B, Cin, Cout, H, W, UPCONV_COUT_BLOCK, UPCONV_MAX_HW))
    if not isinstance(wp, torch.Tensor) or wp.dtype != torch.int32:
        raise SonetHipError("upconv3x3: an up-convolution pack (ops.upconv3x3_pack)")
    _chk(wp, "wp", torch.int32, 1)
    _chk_cvec(Cout, scale=scale, shift=shift)
    dev = _same_device(x, wp, scale, shift)
    lib = _lib.load()
    _chk_pack(lib, wp, "upconv", Cin, Cout, "bytes")
    y = torch.empty((B, Cout, 2 * H, 2 * W), dtype=torch.float32, device=dev)
    name = "upconv3x3_%dx%d_%dx%d" % (Cin, Cout, H, W)
    slot = None
    if _range_active is not None:
        import ctypes
        slot = ctypes.c_void_p(_range_active._slot(name))
    _launch(dev, name, lib.sonet_upconv3x3_f32, ptr(x), ptr(wp), ptr(scale), ptr(shift), int(bool(relu)), ptr(y), B, Cin, Cout, H, W, slot)
    return y


def upconv3x3_dgrad_pack(weight4d):
    """[Cout][Cin][3][3] f32 -> the pack of the up-convolution's input gradient (int32 tensor): the sixteen folded (parity, tap) weights,
    transposed (rows = Cin), summed in float64, split into three bf16 pieces, in MFMA A-fragment order."""
    _chk(weight4d, "weight", torch.float32, 4)
    Cout, Cin, kh, kw = weight4d.shape
    if (kh, kw) != (3, 3):
        raise SonetHipError("upconv3x3_dgrad_pack: a 3x3 kernel, got %dx%d" % (kh, kw))
    if not upconv3x3_supported(Cin, Cout, 1, 1):
        raise SonetHipError("upconv3x3_dgrad_pack: Cout = %d is not a multiple of %d" % (Cout, UPCONV_COUT_BLOCK))
    dev = _same_device(weight4d)
    lib = _lib.load()
    wpt = _pack_empty(lib, "upconv-dgrad", Cin, Cout, dev)
    _launch(dev, None, lib.sonet_upconv3x3_dgrad_pack_f32, ptr(weight4d), ptr(wpt), Cin, Cout)
    return wpt


def upconv3x3_dgrad(g, wpt, Cin):
    """The input gradient of conv3x3_pad1(upsample2_nearest(x), w) in one launch (training): g B x Cout x 2H x 2W f32 (the gradient of
    the convolution's output) -> B x Cin x H x W f32; wpt from ``upconv3x3_dgrad_pack``.  bf16-split (x3) arithmetic: no operand range to
    guard, so the launch takes no range-log slot."""
    _chk(g, "g", torch.float32, 4)
    B, Cout, H2, W2 = g.shape
    Cin = int(Cin)
    H, W = H2 // 2, W2 // 2
    if B < 1 or H2 % 2 or W2 % 2 or not upconv3x3_supported(Cin, Cout, H, W):
        raise SonetHipError("upconv3x3_dgrad: unsupported shape B=%d Cin=%d Cout=%d 2H=%d 2W=%d (Cout %% %d == 0, 1 <= H, W <= %d)"
                            % (B, Cin, Cout, H2, W2, UPCONV_COUT_BLOCK, UPCONV_MAX_HW))
    if not isinstance(wpt, torch.Tensor) or wpt.dtype != torch.int32:
        raise SonetHipError("upconv3x3_dgrad: an input-gradient pack (ops.upconv3x3_dgrad_pack)")
    _chk(wpt, "wpt", torch.int32, 1)
    dev = _same_device(g, wpt)
    lib = _lib.load()
    _chk_pack(lib, wpt, "upconv-dgrad", Cin, Cout, "bytes")
    if g.data_ptr() % 8 or wpt.data_ptr() % 16:
        raise SonetHipError("upconv3x3_dgrad: g must be 8-byte and the pack 16-byte aligned")
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=dev)
    _launch(dev, "upconv3x3_dgrad_%dx%d_%dx%d" % (Cin, Cout, H, W), lib.sonet_upconv3x3_dgrad_f32, ptr(g), ptr(wpt), ptr(dx), B, Cin, Cout, H, W)
    return dx


# Tile extents of csrc/upconv_wgrad.hip (include/sonet_hip.h SONET_UPWGRAD_*): a workgroup covers UPCONV_COUT_BLOCK output channels x
# UPWGRAD_CIN_BLOCK input channels over one slice of the flat column axis in steps of UPWGRAD_K_STEP columns; an accumulation
# chain ends every UPWGRAD_FLUSH_COLS columns; one slice per UPWGRAD_SLICE_COLS columns, at most UPWGRAD_MAX_SLICES.
UPWGRAD_K_STEP = 16
UPWGRAD_CIN_BLOCK = 32
UPWGRAD_FLUSH_COLS = 256
UPWGRAD_SLICE_COLS = 512
UPWGRAD_MAX_SLICES = 128


def upconv3x3_wgrad(g, x):
    """The weight gradient of conv3x3_pad1(upsample2_nearest(x), w) in the folded form (training): g B x Cout x 2H x 2W f32 (the gradient
    of the convolution's output), x B x Cin x H x W f32 -> Cout x Cin x 3 x 3 f32.  Two launches under one name: sixteen (parity, tap)
    products over the B H W columns per slice of that axis, then the float64 sum of the slices and the four-term unfold.  bf16-split (x3)
    arithmetic: no operand range to guard.  No atomics: bit-reproducible; the call can be captured into a graph."""
    _chk(g, "g", torch.float32, 4)
    _chk(x, "x", torch.float32, 4)
    B, Cout, H2, W2 = g.shape
    Bx, Cin, H, W = x.shape
    if B < 1 or Bx != B or H2 != 2 * H or W2 != 2 * W or not upconv3x3_supported(Cin, Cout, H, W):
        raise SonetHipError("upconv3x3_wgrad: unsupported shape g %s, x %s (g B x Cout x 2H x 2W, x B x Cin x H x W, Cout %% %d == 0, "
                            "1 <= H, W <= %d)" % (tuple(g.shape), tuple(x.shape), UPCONV_COUT_BLOCK, UPCONV_MAX_HW))
    dev = _same_device(g, x)
    lib = _lib.load()
    nbytes = lib.sonet_upconv3x3_wgrad_ws_size(B, Cin, Cout, H, W)
    if nbytes == 0:
        raise SonetHipError("upconv3x3_wgrad: unsupported shape B=%d Cin=%d Cout=%d H=%d W=%d" % (B, Cin, Cout, H, W))
    if g.data_ptr() % 8 or x.data_ptr() % 4:
        raise SonetHipError("upconv3x3_wgrad: g must be 8-byte and x 4-byte aligned")
    dw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=dev)
    ws = _ws(nbytes, dev)
    _launch(dev, "upconv3x3_wgrad_%dx%d_%dx%d" % (Cin, Cout, H, W), lib.sonet_upconv3x3_wgrad_f32, ptr(g), ptr(x), ptr(dw), ptr(ws), B, Cin, Cout, H, W)
    return dw


# ------------------------------------------------------------------------------------------ segmentation metrics
SHAPENET_PART_OFFSETS = (0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47, 50)    # models/losses.py:126-143 as a CSR table
SEG_METRICS_MAX_C = 256
_part_tables = {}


class SegMetrics:
    """Device tensors of one ``seg_metrics`` call: pred B x N i32 (None unless asked for), correct B i32, nll_sum B f64, inter / pred_cnt /
    gt_cnt B x C i32, iou B f64, bad B i32; N the points per cloud."""
    __slots__ = ("pred", "correct", "nll_sum", "inter", "pred_cnt", "gt_cnt", "iou", "bad", "N")

    @property
    def union(self):
        return self.pred_cnt + self.gt_cnt - self.inter


def _part_offsets(part_offsets, C):
    off = tuple(int(v) for v in (SHAPENET_PART_OFFSETS if part_offsets is None else part_offsets))
    if len(off) < 2 or off[0] != 0 or any(b <= a for a, b in zip(off, off[1:])) or off[-1] > C:
        raise SonetHipError("part_offsets must start at 0, increase strictly (no empty category) and end at most at C = %d, got %s"
                            % (C, off))
    return off


def _part_table(off, dev):
    key = (off, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _part_tables.get(key)
    if t is None:
        t = _part_tables[key] = torch.tensor(off, dtype=torch.int32).to(dev)
    return t


def seg_metrics(score, seg, label, part_offsets=None, want_pred=False):
    """score B x C x N f32 (score_segmenter's layout), seg B x N i64, label B i64 -> ``SegMetrics`` (include/sonet_hip.h:
    sonet_seg_metrics_f32).  part_offsets: host sequence of n_cat + 1 part boundaries (default: the ShapeNet-part table)."""
    if not isinstance(score, torch.Tensor) or score.dim() != 3:
        raise SonetHipError("score must be a B x C x N torch.Tensor")
    off = _part_offsets(part_offsets, score.shape[1])         # (host data: checked first, no device needed)
    _chk(score, "score", torch.float32, 3)
    _chk(seg, "seg", torch.int64, 2)
    _chk(label, "label", torch.int64, 1)
    B, C, N = score.shape
    if tuple(seg.shape) != (B, N) or label.shape[0] != B:
        raise SonetHipError("seg must be B x N = %s and label B, got %s and %s" % ((B, N), tuple(seg.shape), tuple(label.shape)))
    if B < 1 or C < 1 or N < 1 or C > SEG_METRICS_MAX_C or B > 65535:
        raise SonetHipError("seg_metrics: need 1 <= B <= 65535, 1 <= C <= %d, N >= 1, got B=%d C=%d N=%d" % (SEG_METRICS_MAX_C, B, C, N))
    dev = _same_device(score, seg, label)
    table, n_cat = _part_table(off, dev), len(off) - 1
    lib = _lib.load()
    r = SegMetrics()
    r.N = N
    r.pred = torch.empty((B, N), dtype=torch.int32, device=dev) if want_pred else None
    ints = torch.empty((2 + 3 * C, B), dtype=torch.int32, device=dev)
    r.correct, r.bad = ints[0], ints[1]
    r.inter, r.pred_cnt, r.gt_cnt = (ints[2 + k * C:2 + (k + 1) * C].view(B, C) for k in range(3))
    f64 = torch.empty((2, B), dtype=torch.float64, device=dev)
    r.nll_sum, r.iou = f64[0], f64[1]
    ws = torch.empty((max(1, lib.sonet_seg_metrics_ws_size(B, C, N) // 8),), dtype=torch.float64, device=dev)
    _launch(dev, "seg_metrics", lib.sonet_seg_metrics_f32, ptr(score), ptr(seg), ptr(label), ptr(table), n_cat, ptr(r.pred), ptr(r.correct), ptr(r.nll_sum),
            ptr(r.inter), ptr(r.pred_cnt), ptr(r.gt_cnt), ptr(r.iou), ptr(r.bad), ptr(ws), B, C, N)
    return r


# ------------------------------------------------------------------------------------------ cross-entropy
# Extents of csrc/ce_loss.hip (sonet_ce_max_c / sonet_ce_block_points): the classes a call takes, the points of one forward workgroup.
CE_MAX_C = 256
CE_BLOCK_POINTS = 256


class CeTerms:
    """Device tensors of one ``ce_terms`` call: nll_sum B f64, correct B i32, bad B i32, pred B x N i32 and lse B x N f64 (None unless
    asked for), confusion (the caller's C x C i64 table, added to, or None); N the points per cloud."""
    __slots__ = ("nll_sum", "correct", "bad", "pred", "lse", "confusion", "N")


def ce_supported(C, B=1, N=1):
    """Sizes the cross-entropy operator takes: 1 <= C <= CE_MAX_C, B N < 2^31, and B <= 65535 unless N == 1."""
    B, C, N = int(B), int(C), int(N)
    return 1 <= C <= CE_MAX_C and B >= 1 and N >= 1 and B * N < 1 << 31 and (N == 1 or B <= 65535)


def _chk_ce(score, target):
    """score B x C x N or B x C f32, target B x N or B i64 -> (score as B x C x N, target as B x N, dev, B, C, N).  (A torch tensor's
    first element sits on a multiple of its element size, so the 8-byte alignment the C entries ask of target and lse always holds.)"""
    if not isinstance(score, torch.Tensor) or score.dim() not in (2, 3):
        raise SonetHipError("score must be a B x C x N or B x C torch.Tensor")
    _chk(score, "score", torch.float32)
    _chk(target, "target", torch.int64, score.dim() - 1)
    if score.dim() == 2:
        score, target = score.unsqueeze(2), target.unsqueeze(1)
    B, C, N = score.shape
    if tuple(target.shape) != (B, N):
        raise SonetHipError("target must be B x N = %s, got %s" % ((B, N), tuple(target.shape)))
    if not ce_supported(C, B, N):
        raise SonetHipError("cross-entropy: need 1 <= C <= %d, B, N >= 1, B N < 2^31 (B <= 65535 unless N == 1), got B=%d C=%d N=%d"
                            % (CE_MAX_C, B, C, N))
    return score, target, _same_device(score, target), B, C, N


def _ce_forward(score, target, dev, B, C, N, want_pred, want_lse, confusion):
    """The forward launch on operands ``_chk_ce`` has seen: two allocations (float64: sums, lse, workspace; int32: counts, pred)."""
    lib = _lib.load()
    r = CeTerms()
    r.N, r.confusion = N, confusion
    n_lse = B * N if want_lse else 0
    f64 = torch.empty((B + n_lse + lib.sonet_ce_loss_ws_size(B, C, N) // 8,), dtype=torch.float64, device=dev)
    r.nll_sum = f64[:B]
    r.lse = f64[B:B + n_lse].view(B, N) if want_lse else None
    ints = torch.empty((2 * B + (B * N if want_pred else 0),), dtype=torch.int32, device=dev)
    r.correct, r.bad = ints[:B], ints[B:2 * B]
    r.pred = ints[2 * B:].view(B, N) if want_pred else None
    _launch(dev, "ce_loss", lib.sonet_ce_loss_f32, ptr(score), ptr(target), ptr(r.lse), ptr(r.nll_sum), ptr(r.pred), ptr(r.correct), ptr(r.bad),
            ptr(confusion), ptr(f64[B + n_lse:]), B, C, N)
    return r


def ce_terms(score, target, want_pred=False, want_lse=False, confusion=None):
    """score B x C x N f32 (score_segmenter's layout) or B x C, target B x N or B i64 -> ``CeTerms`` (include/sonet_hip.h:
    sonet_ce_loss_f32).  confusion: a contiguous C x C i64 device table the call ADDS its counts to.  Nothing is read back."""
    score, target, dev, B, C, N = _chk_ce(score, target)
    if confusion is not None:
        _chk(confusion, "confusion", torch.int64, 2)
        if tuple(confusion.shape) != (C, C):
            raise SonetHipError("confusion must be C x C = %s, got %s" % ((C, C), tuple(confusion.shape)))
        _same_device(score, confusion)
    return _ce_forward(score, target, dev, B, C, N, want_pred, want_lse, confusion)


def _ce_grad_launch(score, target, lse, gout, scale, dev, B, C, N, shape):
    grad = torch.empty(shape, dtype=torch.float32, device=dev)
    _launch(dev, "ce_grad", _lib.load().sonet_ce_grad_f32, ptr(score), ptr(target), ptr(lse), ptr(gout), scale, ptr(grad), B, C, N)
    return grad


def ce_grad(score, target, lse, gout, scale):
    """d(scale * gout * sum of nll) / d score at the ``lse`` of a ``ce_terms(want_lse=True)`` call: gout one f32 on the device, scale a
    host float -> f32 of score's shape (include/sonet_hip.h: sonet_ce_grad_f32).  One launch, no host sync."""
    shape = score.shape if isinstance(score, torch.Tensor) else None
    score, target, dev, B, C, N = _chk_ce(score, target)
    _chk(lse, "lse", torch.float64)
    _chk(gout, "gout", torch.float32)
    if lse.numel() != B * N or gout.numel() != 1:
        raise SonetHipError("lse must hold B N = %d elements and gout one, got %d and %d" % (B * N, lse.numel(), gout.numel()))
    _same_device(score, lse, gout)
    return _ce_grad_launch(score, target, lse, gout, float(scale), dev, B, C, N, shape)


class _CeLoss(torch.autograd.Function):
    """``checked``: what ``_chk_ce`` returned for (score, target) -- the operands are looked at once per call, not once per layer of
    wrappers, and not again in the backward."""

    @staticmethod
    def forward(ctx, score, mean, checked):
        score3, target, dev, B, C, N = checked
        needs = ctx.needs_input_grad[0]
        t = _ce_forward(score3, target, dev, B, C, N, False, needs, None)
        scale = 1.0 / (B * N) if mean else 1.0
        if needs:
            ctx.save_for_backward(score, target, t.lse)            # (score3 is score's memory: the same pointer)
            ctx.ce = (scale, dev, B, C, N, score.shape)
        ctx.mark_non_differentiable(t.bad)
        total = t.nll_sum.sum()                                       # f64, on the device
        return (total / (B * N) if mean else total).float(), t.bad

    @staticmethod
    def backward(ctx, gout, _gbad):
        score, target, lse = ctx.saved_tensors
        if gout.dtype != torch.float32 or not gout.is_contiguous():
            gout = gout.float().contiguous()
        return _ce_grad_launch(score, target, lse, gout, *ctx.ce), None, None


def ce_loss(score, target, reduction="mean", want_bad=False):
    """Softmax cross-entropy as one operator: score B x C x N or B x C f32 (may require a gradient), target B x N or B i64 -> the f32
    scalar mean (or ``reduction="sum"``) over all B N points of lse - score[target], summed in float64 on the device and rounded once;
    differentiable in ``score``.  A target outside [0, C) adds nothing and gets a zero gradient; the denominator stays B N
    (``want_bad=True``: also the B i32 counts of such targets, not differentiable).  Forward one ``sonet_ce_loss_f32`` call, which keeps
    lse only when ``score`` requires a gradient; backward one ``sonet_ce_grad_f32`` call, whatever the upstream gradient."""
    if reduction not in ("mean", "sum"):
        raise SonetHipError("ce_loss: reduction must be 'mean' or 'sum', got %r" % (reduction,))
    loss, bad = _CeLoss.apply(score, reduction == "mean", _chk_ce(score, target))
    return (loss, bad) if want_bad else loss


# ------------------------------------------------------------------------------------------ retrieval lists
RETRIEVAL_MAX_TOP = 1024
RETRIEVAL_MAX_D = 1024
RETRIEVAL_MAX_LABEL = 65535
RETRIEVAL_MAX_N = (1 << 24) - 1


class RetrievalLists:
    """Device tensors of one ``retrieval_lists`` call: nn_id Q x top i64, nn_dist Q x top f32, nn_pos Q x top i32 (None unless asked
    for), count Q i32, labels N i32 (the labels used, -1 for one outside [0, n_label)), bad 1 i32; top the list length."""
    __slots__ = ("nn_id", "nn_dist", "nn_pos", "count", "labels", "bad", "top")


def retrieval_lists(feat, labels=None, ids=None, query=None, top=1000, n_label=None, want_pos=False):
    """feat N x D f32, labels N i64 (None: the arg-max of every row, and n_label = D), ids N i64 (None: the gallery index), query: a
    device i32 tensor of gallery indices (values checked by the kernel, which counts the bad ones), or a host sequence / CPU tensor
    (values checked here, then copied), or None for every shape -> ``RetrievalLists`` (include/sonet_hip.h: sonet_retrieval_lists_f32).
    Nothing is read back: the call returns with the launches queued."""
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2:
        raise SonetHipError("feat must be an N x D torch.Tensor")
    N, D = feat.shape
    # attribute and host-value checks first (no device needed), then _chk: CUDA and contiguous
    for name, t, dtype in (("feat", feat, torch.float32), ("labels", labels, torch.int64), ("ids", ids, torch.int64)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise SonetHipError("%s must be a %s torch.Tensor, got %s" % (name, dtype, getattr(t, "dtype", type(t).__name__)))
        if name != "feat" and tuple(t.shape) != (N,):
            raise SonetHipError("%s must hold N = %d elements, got shape %s" % (name, N, tuple(t.shape)))
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= RETRIEVAL_MAX_TOP:
        raise SonetHipError("top must be an int in [1, %d], got %r" % (RETRIEVAL_MAX_TOP, top))
    if not 1 <= N <= RETRIEVAL_MAX_N or not 1 <= D <= RETRIEVAL_MAX_D:
        raise SonetHipError("retrieval_lists: need 1 <= N < 2^24 and 1 <= D <= %d, got N=%d D=%d" % (RETRIEVAL_MAX_D, N, D))
    if labels is None:
        if n_label is not None and n_label != D:
            raise SonetHipError("n_label=%r but labels derived from the features are the arg-max over D = %d columns" % (n_label, D))
        n_label = D
    elif n_label is None:
        raise SonetHipError("n_label is needed with given labels")
    if isinstance(n_label, bool) or not isinstance(n_label, int) or not 1 <= n_label <= RETRIEVAL_MAX_LABEL:
        raise SonetHipError("n_label must be an int in [1, %d], got %r" % (RETRIEVAL_MAX_LABEL, n_label))
    host_query = None
    if isinstance(query, torch.Tensor) and query.is_cuda:
        if query.dtype != torch.int32 or query.dim() != 1 or query.shape[0] < 1:
            raise SonetHipError("a device query must be a non-empty 1-D int32 tensor, got %s %s" % (tuple(query.shape), query.dtype))
    elif query is not None:
        host_query = np.asarray(query.numpy() if isinstance(query, torch.Tensor) else query)
        if host_query.ndim != 1 or host_query.size < 1 or host_query.dtype.kind not in "iu":
            raise SonetHipError("query must be a non-empty 1-D sequence of integers")
        if host_query.min() < 0 or host_query.max() >= N:
            raise SonetHipError("query index outside [0, N = %d): min %d max %d" % (N, host_query.min(), host_query.max()))
    _chk(feat, "feat")
    if labels is not None:
        _chk(labels, "labels")
    if ids is not None:
        _chk(ids, "ids")
    dev = _same_device(feat, labels, ids)
    if host_query is not None:
        query = torch.from_numpy(host_query.astype(np.int32)).to(dev)
    if query is not None:
        _chk(query, "query")
        _same_device(feat, query)
    Q = N if query is None else query.shape[0]
    lib = _lib.load()
    r = RetrievalLists()
    r.top = top
    r.nn_id = torch.empty((Q, top), dtype=torch.int64, device=dev)
    r.nn_dist = torch.empty((Q, top), dtype=torch.float32, device=dev)
    r.nn_pos = torch.empty((Q, top), dtype=torch.int32, device=dev) if want_pos else None
    ints = torch.empty((Q + N + 1,), dtype=torch.int32, device=dev)
    r.count, r.labels, r.bad = ints[:Q], ints[Q:Q + N], ints[Q + N:]
    ws = torch.empty((lib.sonet_retrieval_ws_size(N, D, Q, top) // 4,), dtype=torch.int32, device=dev)
    _launch(dev, "retrieval_lists", lib.sonet_retrieval_lists_f32, ptr(feat), ptr(labels), ptr(ids), ptr(query), n_label, top, ptr(r.nn_id), ptr(r.nn_dist),
            ptr(r.nn_pos), ptr(r.count), ptr(r.labels), ptr(r.bad), ptr(ws), N, D, Q)
    return r


def mfma_f16_sustained_rate(random_operands=True, iters=4000, device=None):
    """(TFLOP/s, shader GHz) a pure fp16 MFMA loop holds on the whole chip -- the measuring stick beside the nominal
    matrix peak (``sonet_diag_mfma_f16_rate``; with random operands the rate is power-limited, DESIGN.md finding 8)."""
    import ctypes
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    tf, ghz = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _lib.require_device(dev)
    _launch(dev, None, _lib.load().sonet_diag_mfma_f16_rate, 1 if random_operands else 0, int(iters), ctypes.byref(tf), ctypes.byref(ghz))
    return tf.value, ghz.value


def knn_prepare(coord, knn_I, center_avg):
    """coord B x 3 x M, knn_I B x M x K i64 -> (center B x 3 x M, de-centred neighbour coordinates B x 3 x (K*M) K-MAJOR,
    gather index B x (K*M) i32) -- what the gathering KNNModule layer needs beside the features (models/layers.py:313-350)."""
    _chk(coord, "coord", torch.float32, 3)
    _chk(knn_I, "knn_I", torch.int64, 3)
    dev = _same_device(coord, knn_I)
    B, _, M = coord.shape
    K = knn_I.shape[2]
    if coord.shape[1] != 3 or knn_I.shape[0] != B or knn_I.shape[1] != M:
        raise SonetHipError("knn_prepare: coord must be B x 3 x M and knn_I B x M x K")
    center = torch.empty((B, 3, M), dtype=torch.float32, device=dev)
    dec = torch.empty((B, 3, K * M), dtype=torch.float32, device=dev)
    gidx = torch.empty((B, K * M), dtype=torch.int32, device=dev)
    _launch(dev, "knn_prepare", _lib.load().sonet_knn_prepare_f32, ptr(coord), ptr(knn_I), B, M, K, int(bool(center_avg)), ptr(center), ptr(dec), ptr(gidx))
    return center, dec, gidx



def planes_max(x, K):
    """x B x C x (K*M) with k-major columns -> B x C x M, max over the K planes (values only, NaN-propagating)."""
    if x.dtype == torch.bfloat16:
        x = x.float()
    _chk(x, "x", torch.float32, 3)
    B, C, L = x.shape
    if K <= 0 or L % K:
        raise SonetHipError("planes_max: L=%d is not %d planes" % (L, K))
    dev = _same_device(x)
    out = torch.empty((B, C, L // K), dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    _launch(dev, "planes_max", _lib.load().sonet_planes_max_f32, ptr(x), ptr(out), B * C, K, L // K)
    return out


def bn_running_update_(running_mean, running_var, mean, var, momentum, unbias):
    """running = running*(1-momentum) + momentum*stat in place (variance entering as var*unbias): F.batch_norm's update."""
    for t, n in ((running_mean, "running_mean"), (running_var, "running_var"), (mean, "mean"), (var, "var")):
        _chk(t, n, torch.float32, 1)
    _chk_cvec(running_mean.numel(), running_var=running_var, mean=mean, var=var)
    dev = _same_device(running_mean, running_var, mean, var)
    _launch(dev, None, _lib.load().sonet_bn_running_update_f32, ptr(running_mean), ptr(running_var), ptr(mean), ptr(var), float(momentum), float(unbias),
            running_mean.numel())
    # written through raw pointers: move the version counters as an in-place aten op would (caches keyed on versions must notice)
    torch.autograd.graph.increment_version(running_mean)
    torch.autograd.graph.increment_version(running_var)
