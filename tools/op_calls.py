#!/usr/bin/env python
"""tools/op_calls.py TREE [--real] -- every C-ABI call the Python op wrappers of TREE/so-net_amd/sonet_hip/ops.py make, without a GPU.

The wrappers run on fake CUDA tensors (torch._subclasses.FakeTensorMode: device, dtype, shape, strides and allocation behave, nothing is
computed) against a stand-in for the library: ``ops.ptr`` returns the operand's role name (``new:<dtype>[<shape>]`` for a tensor the
wrapper allocated itself), ``ops.stream_ptr`` the word ``stream``, the device switch does nothing, and ``_lib.load()`` hands out a proxy
that forwards the host-arithmetic queries to the real library and records every other entry point as one line -- name and arguments in
order -- before returning 0; ``timed`` lists the labels the launches carry under ``ops.kernel_timing()``.  Queries are told from launches by NAME (the patterns of ``QUERIES``; ``*_chunk`` and ``*_chunk_keys`` and
not ``*_chunk*``, which would take ``sonet_chunk_mean_f32`` for one), not by ``_lib._RESTYPES``: five of them return a plain int.  Per case the output holds the call, the recorded lines and either the dtypes and shapes returned (``->``) or
the exception with its message (``!!``).  ``MUTANTS`` are applied to every tensor argument of the cases marked for it: that is where the
refusals, their texts and their order come from.  The module caches that would keep a tensor from one case to the next (``ops._CONST``,
the pack registry) are emptied before each case.  Wrappers that read tensor VALUES on the host cannot run this way; they are listed
under ``not recorded`` with the call that stopped them, and the GPU suite owns them.

--real: the layer family only, at B = 2, 32 -> 64 and 48 + 16 -> 64, L in {8, 33}, on real CUDA tensors with the same stand-in library
(nothing is launched; no second device is asked for): tests/test_gpu_op_calls.py holds a fake tensor to what a real one answers.
``summarise(text)`` is the outline committed beside the fixture (tests/golden/ops): lines and digest per wrapper."""
import contextlib
import fnmatch
import hashlib
import os
import sys
import warnings

import torch

QUERIES = ("*_size", "*_columns", "*_chunk", "*_chunk_keys", "*_tile", "*_max_rows", "sonet_pack_multi_kc")
F, H, D, I, J, I8, U8, I16 = torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.int8, torch.uint8, torch.int16
SHORT = {F: "f32", H: "bf16", D: "f64", I: "i32", J: "i64", I8: "i8", U8: "u8", I16: "i16"}
WRONG = {F: D, H: F, D: F, I: J, J: I, I8: U8, U8: I8, I16: I}
REAL_SHAPES = [(2, 32, 0, 64, 8), (2, 32, 0, 64, 33), (2, 48, 16, 64, 8), (2, 48, 16, 64, 33)]
SHAPES = REAL_SHAPES + [(1, 64, 0, 128, 1), (1, 3, 64, 128, 2), (2, 64, 0, 128, 64)]
NAMES, KEEP, LINES, TIMED = {}, [], [], []
REAL = "--real" in sys.argv
TREE = os.path.abspath(sys.argv[1]) if __name__ == "__main__" else ""
ops = None


def sh(x):
    return "%s[%s]" % (SHORT.get(x.dtype, x.dtype), ",".join(str(int(v)) for v in x.shape))


def show(r, names=False):
    if isinstance(r, torch.Tensor):
        flags = ("" if r.is_contiguous() else "!strided") + ("" if r.device.index in (0, None) else "@%s" % r.device)
        return (NAMES[id(r)] + ":" if names and id(r) in NAMES else "") + sh(r) + (flags if names else "")
    if isinstance(r, (tuple, list)):
        return "(" + ", ".join(show(v, names) for v in r) + ")"
    if isinstance(r, dict):
        return "{" + ", ".join("%s: %s" % (k, show(v, names)) for k, v in r.items()) + "}"
    if hasattr(type(r), "__slots__") and not isinstance(r, (torch.dtype, torch.device)):
        return type(r).__name__ + "(" + ", ".join("%s=%s" % (k, show(getattr(r, k, None), names)) for k in type(r).__slots__) + ")"
    return getattr(r, "__name__", None) or repr(r)


class Proxy:
    def __init__(self, real):
        self.real = real

    def __getattr__(self, name):
        fn = getattr(self.real, name)                     # (AttributeError as the real library gives it: hasattr() answers alike)
        if any(fnmatch.fnmatchcase(name, p) for p in QUERIES):
            return fn

        def record(*a):
            LINES.append("  %s(%s)" % (name, ", ".join(v if isinstance(v, str) else repr(v) if isinstance(v, (int, float, type(None)))
                                                        else type(v).__name__ for v in a)))
            return 0
        return record


def setup(tree):
    global ops
    sys.path.insert(0, os.path.join(tree, "so-net_amd"))
    from sonet_hip import _lib, ops as o
    ops = o
    proxy = Proxy(_lib.load())
    _lib.load = lambda: proxy
    _lib.require_device = lambda dev: None
    _lib.on_device = lambda dev: contextlib.nullcontext()
    torch.cuda._exchange_device = torch.cuda._maybe_exchange_device = lambda idx: -1
    torch.cuda.current_device, torch.cuda.is_current_stream_capturing = (lambda: 0), (lambda: False)    # (the same with and without a GPU)
    torch.cuda.Event = type("Event", (), dict(__init__=lambda self, **k: None, record=lambda self: None))
    ops._TIMING = TIMED                                      # (as under ``ops.kernel_timing()``: the label of every timed launch)
    ops.ptr = lambda x: None if x is None else NAMES.get(id(x)) or "new:" + sh(x)
    ops.stream_ptr = lambda: "stream"


def named(name, x):
    NAMES[id(x)] = name
    KEEP.append(x)
    return x


def t(name, *shape, dt=F, dev="cuda:0"):
    return named(name, torch.empty(shape, dtype=dt, device=dev))


def case(fn, **kw):
    print("== %s(%s)" % (fn.__name__, ", ".join("%s=%s" % (n, show(v, True)) for n, v in kw.items())))
    del LINES[:], TIMED[:]
    ops._CONST.clear()
    ops.packs.entries.clear()
    ops.packs.tables.clear()
    try:
        out = "-> " + show(fn(**kw))
    except Exception as e:
        del TIMED[:]                                          # (a refused call has nothing to time)
        out = "!! %s: %s" % (type(e).__name__, str(e).split("\n")[0].replace(TREE, "TREE"))
    print("\n".join(LINES + ["  timed %s" % ", ".join(n for n, _, _ in TIMED)] * bool(TIMED) + ["  " + out]))


def mutants(name, v):
    s = tuple(v.shape)
    yield t(name, *s, dt=WRONG[v.dtype])
    yield t(name, 1, *s, dt=v.dtype)
    yield named(name, t(name, *s[:-1], 2 * s[-1], dt=v.dtype)[..., ::2])
    if not REAL:
        yield t(name, *s, dt=v.dtype, dev="cuda:1")
    if len(s) > 1:
        yield t(name, s[0] + 1, *s[1:], dt=v.dtype)
    yield t(name, *s[:-1], s[-1] + 1, dt=v.dtype)
    yield "x"


def run(fn, mut=False, **kw):
    """One case; mut: and the same call with each tensor argument in turn of another dtype, rank, stride, device, first and last extent,
    and replaced by a string."""
    case(fn, **kw)
    for n, v in (kw.items() if mut else ()):
        if isinstance(v, torch.Tensor) and v.dim():
            for m in mutants(n, v):
                case(fn, **dict(kw, **{n: m}))
    NAMES.clear()
    del KEEP[:]


def table(fn, rows):
    for a in rows:
        print("== %s%s\n  -> %r" % (fn.__name__, show(a, True), fn(*a)))
    NAMES.clear()
    del KEEP[:]


def wpk(mode, Cin, Cout, name="wp"):
    w = t("w", Cout, Cin)
    return named(name, ops.pointmlp_h3p_pack(w) if mode == "h3p" else ops.pointmlp_pack(w, mode))


def p16(name, B, C, L):
    p = ops.p16_empty(B, C, L, "cuda:0")
    named(name, p.data)
    return p


def xaff(C1, C2, six):
    return (t("s1", C1), t("h1", C1), True) + ((t("s2", C2), t("h2", C2), False) if six else ())


def ss(Co):
    return dict(scale=t("scale", Co), shift=t("shift", Co), relu=True, Cout=Co)


def stale_pack(w2d):
    """The pack registry's refresh: a pack, a weight update, the pack again."""
    ops.packs.get(w2d, ("fwd", "h3"))
    torch.autograd.graph.increment_version(w2d)
    return ops.packs.get(w2d, ("fwd", "h3"))


def h3_launch():
    return ops.p16_from_f32(t("x", 1, 16, 8))


def layers(shapes):
    print("# layers")
    for B, C1, C2, Co, L in shapes:
        mut = (B, C1, L) == (2, 48, 8)
        Ci, M = C1 + C2, 4
        x = lambda dt=F, n="x1": t("x" if n == "x1" else n, B, C1, L, dt=dt)
        x2 = lambda dt=F: t("x2", B, C2, L, dt=dt) if C2 else None
        ids = lambda n="ids": t(n, B, L, dt=I)
        for mode, dt in (("f32", F), ("x3", F), ("h3", F), ("bf16", H)):
            run(ops.pointmlp, mut and mode != "x3", x1=x(dt), wp=wpk(mode, Ci, Co), **ss(Co), x2=x2(dt))
            if mode == "f32":
                continue
            run(ops.pointmlp_stats, mut and mode != "x3", x1=x(dt), wp=wpk(mode, Ci, Co), **ss(Co), x2=x2(dt))
            for six in ((False, True) if mode != "x3" else (False,)):
                run(ops.pointmlp_stats, x1=x(dt), wp=wpk(mode, Ci, Co), **ss(Co), x2=x2(dt), xaff=xaff(C1, C2, six))
        run(ops.pointmlp, x1=x(), wp=wpk("h3", Ci, Co), **ss(Co), x2=x2(), out=t("out", B, Co, L))
        for mode, dt in (("h3", F), ("bf16", H), ("x3", F)):
            run(ops.pointmlp, mut and mode == "h3", x1=t("x", B, C1, 5, dt=dt), wp=wpk(mode, Ci, Co), **ss(Co), x2=x2(dt), gidx=ids("gidx"))
        run(ops.pointmlp, mut, x1=x(H), wp=wpk("bf16", Ci, Co), **ss(Co), x2=x2(H), acc=t("acc", B, Co, L, dt=H))
        z = lambda: dict(z=t("z", B, Co, M), zidx=ids("zidx"))
        run(ops.pointmlp_nodeadd, mut, x1=x(), wp=wpk("h3", Ci, Co), **ss(Co), **z(), x2=x2())
        run(ops.pointmlp_nodeadd_stats, mut, x1=x(), wp=wpk("h3", Ci, Co), bias=t("bias", Co), Cout=Co, **z(), x2=x2())
        for rm, xa in ((False, None), (True, False), (True, True)):
            o = lambda: dict(row_max=t("row_max", B, M, dt=I) if rm else None, x2=x2(), xaff=None if xa is None else xaff(C1, C2, xa))
            run(ops.pointmlp_h3_segpool, mut and not rm, x1=x(), wp=wpk("h3", Ci, Co), **ss(Co), ids_sorted=ids("ids_sorted"),
                pos0=t("pos0", B, dt=I), M=M, **o())
            o = lambda: dict(row_max=t("row_max", B, M, dt=I) if rm else None, x2=x2(H), xaff=None if xa is None else xaff(C1, C2, xa))
            run(ops.pointmlp_bf16_pool, mut and not rm, x1=x(H), wp=wpk("bf16", Ci, Co), **ss(Co), ids=ids(), M=M, **o())
        co = lambda: dict(zip("a b c0 sc sh".split(), (t(n, Co) for n in "a b c0 sc sh".split())), relu=True, Cout=Ci)
        g = lambda mode, dt: dict(gy=t("gy", B, Co, L, dt=dt), raw=t("raw", B, Co, L, dt=dt), wpt=wpk(mode, Co, Ci, "wpt"), scale=t("scale", Ci),
                                  shift=t("shift", Ci), **co())
        for fn, mode, dt in ((ops.pointmlp_x3_bnb, "x3", F), (ops.pointmlp_bf16_bnb, "bf16", H)):
            run(fn, mut, **g(mode, dt))
            run(fn, mut, **g(mode, dt), want_g_raw=False, acc=t("acc", B, Ci, L, dt=dt))
        run(ops.pointmlp_x3_bnb, mut, **g("x3", F), below=(t("praw", B, Ci, L), t("psc", Ci), t("psh", Ci), True))
        p2 = lambda: p16("x2", B, C2, L) if C2 else None
        for out in ("f32", "p16", "both"):
            run(ops.pointmlp_h3p, mut and out == "f32", x1=p16("x", B, C1, L), wp=wpk("h3p", Ci, Co), **ss(Co), x2=p2(), out=out, tag="t")
        run(ops.pointmlp_h3p, mut, x1=p16("x", B, C1, 5), wp=wpk("h3p", Ci, Co), **ss(Co), x2=p2(), gidx=ids("gidx"), **z(), stats=True)
        run(ops.pointmlp_h3p, x1=p16("x", B, C1, L), wp=wpk("h3p", Ci, Co), **ss(Co), x2=p2(), out="p16", stats=True)
        run(ops.p16_from_f32, mut, x=x())
        run(ops.p16_from_f32, mut, x=x(), scale=t("scale", C1), shift=t("shift", C1), relu=True)
        table(ops.pointmlp_bf16_pool_ok, [(x(H), x2(H), Co, M), (x(), x2(), Co, M)])
        table(ops.pointmlp_h3_segpool_ok, [(x(), x2(), wpk("h3", Ci, Co), Co, M), (x(), x2(), wpk("x3", Ci, Co), Co, M)])
        table(ops.pointmlp_bf16_bnb_ok, [(Co, Ci, L)])
        table(ops.x3_supported, [(C1, C2, Co)])
        table(ops.xaff_ok, [(C1, C2, Co)])
        table(ops.bf16_xaff_ok, [(B, C1, C2, Co, L), (8192, C1, C2, Co, 64 * L)])
    run(ops.pointmlp, x1=t("x", 0, 32, 8), wp=wpk("h3", 32, 64), **ss(64))
    run(ops.pointmlp_x3_bnb, gy=t("gy", 2, 64, 0), raw=t("raw", 2, 64, 0), wpt=wpk("x3", 64, 32, "wpt"), scale=t("scale", 32), shift=t("shift", 32),
        **{n: t(n, 64) for n in "a b c0 sc sh".split()}, relu=True, Cout=32)


def rest():
    B, C, L, M, K, N = 2, 32, 8, 4, 3, 16
    i = lambda n, *s: t(n, *s, dt=I)
    print("# packs")
    for mode in ("f32", "x3", "h3", "bf16"):
        run(ops.pointmlp_pack, mode == "h3", weight2d=t("w", 64, 48), mode=mode)
        run(ops.pointmlp_pack_transposed, mode == "h3", weight2d=t("w", 64, 48), lo=16, Ci=32, Cp=32, mode=mode)
        if mode != "f32":
            run(ops.packs.get, mode == "h3", w2d=t("w", 64, 48), what=("fwd", mode))
            run(ops.packs.get, w2d=t("w", 64, 48), what=("t", mode, 16, 32, 32))
    run(ops.pointmlp_pack_transposed, weight2d=t("w", 64, 48), lo=32, Ci=32, Cp=32, mode="h3")
    run(stale_pack, w2d=t("w", 64, 48))
    run(ops.pointmlp_h3p_pack, True, weight2d=t("w", 64, 48))
    w4 = lambda: dict(w1=t("w1", 64, 6), w2=t("w2", 128, 64), w3=t("w3", 256, 128), w4=t("w4", 384, 320))
    run(ops.pointresnet_pack, True, **w4())
    run(ops.pointresnet_bf16_pack, True, **w4())
    run(ops.upconv3x3_pack, True, weight4d=t("w", 32, 5, 3, 3))
    run(ops.upconv3x3_dgrad_pack, True, weight4d=t("w", 32, 5, 3, 3))
    run(ops.upconv3x3_pack, weight4d=t("w", 16, 5, 3, 3))
    print("# pooling, gathers, SOM, node stage")
    for dt in (F, H):
        run(ops.index_max, dt == F, data=t("data", B, C, L, dt=dt), index=i("index", B, L), K=M)
        run(ops.index_max_gather, dt == F, data=t("data", B, C, L, dt=dt), index=i("index", B, L), K=M, row_max=i("row_max", B, M))
        run(ops.index_max_gather, data=t("data", B, C, L, dt=dt), index=i("index", B, L), K=M)
        run(ops.node_gather_bwd, dt == F, g=t("g", B, C, L, dt=dt), min_idx_i32=i("min_idx", B, L), M=M)
        run(ops.knn_gather_bwd, dt == F, g=t("g", B, C, M, K, dt=dt), knn_I=t("knn_I", B, M, K, dt=J), M=M)
        run(ops.node_gather_lead_affine_act, dt == F, z=t("z", B, C, M, dt=dt), gidx=i("gidx", B, L), lead=t("lead", B, 3, L), wl=t("wl", C, 3),
            scale=t("scale", C), shift=t("shift", C), relu=True)
        run(ops.lastdim_max, dt == F, x=t("x", B, C, M, K, dt=dt))
        run(ops.lastdim_max_autograd, x=t("x", B, C, M, K, dt=dt))
        run(ops.planes_max, dt == F, x=t("x", B, C, K * M, dt=dt), K=K)
        run(ops.channel_stats, dt == F, y=t("y", B, C, L, dt=dt))
        run(ops.channel_affine_act, dt == F, x=t("x", B, C, L, dt=dt), scale=t("scale", C), shift=t("shift", C), relu=True)
        bw = lambda: dict(gy=t("gy", B, C, L, dt=dt), raw=t("raw", B, C, L, dt=dt), scale=t("scale", C), shift=t("shift", C), relu=True)
        run(ops.pointwise_bwd_stats, dt == F, **bw())
        run(ops.pointwise_bwd_stats, **bw(), want_sums=True)
        run(ops.pointwise_bwd_apply, dt == F, **bw(), a=t("a", C), b=t("b", C), c0=t("c0", C))
        run(ops.wgrad_bf16 if dt == H else ops.wgrad_x3, True, g=t("g", B, 64, L, dt=dt), x=t("x", B, C, L, dt=dt))
        run(ops.wgrad_bf16 if dt == H else ops.wgrad_x3, True, g=t("g", B, 64, L, dt=dt), x=t("x", B, C, L, dt=dt), xaff=(t("xs", C), t("xh", C), True))
        run(ops.pooled_wgrad, dt == F, g_pooled_t=t("g", B, M, 64), pos_i32_t=i("pos", B, M, 64), x=t("x", B, C, L, dt=dt))
        run(ops.pooled_wgrad, dt == F, g_pooled_t=t("g", B, M, 64), pos_i32_t=i("pos", B, M, 64), x=t("x", B, C, L, dt=dt), xaff=(t("xs", C), t("xh", C), 1))
        pd = lambda: dict(g_pooled=t("g", B, 64, M), pos_i32=i("pos", B, 64, M), weight2d=t("w", 64, 64), C1=48, C2=16, L=L, out_dtype=dt)
        run(ops.pooled_dgrad, dt == F, **pd())
        run(ops.pooled_dgrad, **dict(pd(), C1=64, C2=0), wt_pack=wpk("bf16", 64, 64, "wt_pack"))
        run(ops.pooled_dgrad, **pd(), col0=t("col0", B, 64), pos0=i("pos0", B))
    run(ops.index_max, data=t("data", B, C, 0), index=i("index", B, 0), K=M)
    run(ops.index_max_gather_p16, True, planes=p16("planes", B, C, L), index=i("index", B, L), K=M, row_max=i("row_max", B, M))
    run(ops.pointwise_bwd_apply_nodesum, True, **bw(), a=t("a", C), b=t("b", C), c0=t("c0", C), ids=i("ids", B, L), M=M)
    run(ops.wgrad_x3, g=t("g", B, 64, 0), x=t("x", B, C, 0))
    run(ops.wgrad_bf16, g=t("g", 0, 64, L, dt=H), x=t("x", 0, C, L, dt=H))
    run(ops.node_gather, True, feat=t("feat", B, C, M), min_idx_i32=i("min_idx", B, L))
    run(ops.node_gather_autograd, feat=t("feat", B, C, M), min_idx_i32=i("min_idx", B, L))
    run(ops.node_add_affine_act_, True, t=t("t", B, C, L), z=t("z", B, C, M), min_idx_i32=i("min_idx", B, L), scale=t("scale", C), shift=t("shift", C), relu=1)
    run(ops.channel_affine_act_, True, y=t("y", B, C, L), scale=t("scale", C), shift=t("shift", C), relu=True)
    run(ops.chunk_mean, True, h=t("h", B, C, 3 * L), k=3)
    run(ops.knn_self, True, node=t("node", B, 3, M), K=K)
    run(ops.knn_group, True, coord=t("coord", B, 3, M), feat=t("feat", B, C, M), knn_I=t("knn_I", B, M, K, dt=J), center_avg=True)
    run(ops.knn_gather, True, x=t("x", B, C, M), knn_I=t("knn_I", B, M, K, dt=J))
    run(ops.knn_prepare, True, coord=t("coord", B, 3, M), knn_I=t("knn_I", B, M, K, dt=J), center_avg=False)
    run(ops.som_mask, True, min_idx_i32=i("min_idx", B, N), M=M)
    xs = lambda: dict(x=t("x", B, 3, N), sn=t("sn", B, 3, N))
    for i64 in (False, True):
        run(ops.som_assign, not i64, x=t("x", B, 3, N), node=t("node", B, 3, M), k=2, want_i64=i64)
        run(ops.som_assign_sort, not i64, **xs(), node=t("node", B, 3, M), k=2, want_i64=i64, deterministic=i64)
    run(ops.som_assign_sort, **xs(), node=t("node", B, 3, M), k=1, knn=(t("knn_I", B, M, K, dt=J), K, True))
    run(ops.som_train, True, x=t("x", B, 3, N), node0=t("node0", B, 3, M), w=t("w", 5, M, M), lr=t("lr", 5))
    run(ops.som_train, x=t("x", B, 3, N), node0=t("node0", 3, M), w=t("w", 0, M, 2, 2), lr=t("lr", 0))
    def a():
        r = ops.som_assign(t("x", B, 3, N), t("node", B, 3, M), 1)
        return [named(n, getattr(r, n)) for n in ("min_idx_i32", "count", "sum_ws")] and r
    run(ops.som_group, True, **xs(), a=a(), want_centers=True, want_decentered=True, want_augmented=True)
    run(ops.som_group, x=t("x", B, 3, N), sn=None, a=a())
    run(ops.som_sort_group, True, **xs(), a=a())
    table(ops.som_train_supported, [(N, M), (0, M), (N, 1025), (1 << 29, M)])
    sg = lambda: dict(x_aug_sorted=t("x_sorted", B, 6, N), ids_sorted=i("ids_sorted", B, N), pos0=i("pos0", B), node_off=i("node_off", B, M),
                      count=i("count", B, M))
    for fn, pk in ((ops.pointresnet_fused, ops.pointresnet_pack), (ops.pointresnet_bf16, ops.pointresnet_bf16_pack)):
        for p in ((False, True, "only") if fn is ops.pointresnet_fused else (None,)):
            run(fn, not p, x=t("x", B, 6, N), wstream=named("wstream", pk(**w4())), affine=t("affine", 832, 2), **({} if p is None else dict(want_p16=p)))
        run(fn, x=t("x", 0, 6, N), wstream=named("wstream", pk(**w4())), affine=t("affine", 832, 2))
    for p in (False, True):
        run(ops.pointresnet_fused_pool, not p, sg=sg(), wstream=named("wstream", ops.pointresnet_pack(**w4())), affine=t("affine", 832, 2), M=M, want_p16=p)
    run(ops.pointresnet_fused_pool, sg=dict(sg(), pos0=t("pos0", B, dt=J)), wstream=named("wstream", ops.pointresnet_pack(**w4())), affine=t("affine", 832, 2), M=M)
    run(ops.pointresnet_bf16_pool, True, sg=sg(), wstream=named("wstream", ops.pointresnet_bf16_pack(**w4())), affine=t("affine", 832, 2), M=M)
    Lm = ops.node_stage_columns(B, M)
    def prep():
        d = ops.knn_stage_prepare(t("coord", B, 3, M), t("knn_I", B, M, K, dt=J), K, True)
        named("rec", d["rec"])
        return d
    run(ops.knn_stage_prepare, True, coord=t("coord", B, 3, M), knn_I=t("knn_I", B, M, K + 1, dt=J), K=K, center_avg=True)
    run(ops.knn_stage_input, True, prep=prep(), z=p16("z", 1, C, Lm), wl=t("wl", C, 3), scale=t("scale", C), shift=t("shift", C), relu=True)
    run(ops.knn_layer2_gmax, True, prep=prep(), z=p16("z", 1, C, Lm), wl=t("wl", C, 3), s1=t("s1", C), t1=t("t1", C), relu1=True,
        wp=wpk("h3p", C, 128), s2=t("s2", 128), t2=t("t2", 128), relu2=True, Cout=128, Lout=Lm)
    for out in ("p16", "f32"):
        run(ops.pointmlp_h3p_gmax, out == "p16", x1=p16("x", 1, C, 128), wp=wpk("h3p", C + 16, 64), **ss(64), GK=K, G=16, ngout=B * M,
            x2=p16("x2", 1, 16, 128), out=out, Lout=Lm if out == "p16" else None)
    run(ops.p16_flat_to_bcm, p=p16("p", 1, C, Lm), B=B, M=M)
    run(ops.p16_to_f32, p=p16("p", B, C, L))
    table(ops.knn_layer2_supported, [(32, 128, 3), (32, 64, 3), (528, 128, 3), (32, 128, 129), (384, 512, 9, 8, 64)])
    print("# BatchNorm, heads, losses, decoder, metrics")
    v = lambda *ns: {n: t(n, C) for n in ns}
    run(ops.bn_rider, True, **v("gamma", "beta"), eps=1e-5, **v("running_mean", "running_var"), momentum=0.1, unbias=1.5)
    run(ops.bn_rider, **v("gamma", "beta"), eps=1e-5)
    run(ops.bn_fwd_coeffs, True, **v("mean", "var", "gamma", "beta"), eps=1e-5)
    run(ops.bn_bwd_coeffs, True, sums=t("sums", 2 * C, dt=D), **v("mean", "invstd", "gamma"), n=16)
    run(ops.bn_running_update_, True, **v("running_mean", "running_var", "mean", "var"), momentum=0.1, unbias=1.5)
    run(ops.linear_act, True, x=t("x", B, C), weight=t("weight", 64, C), scale=t("scale", 64), shift=t("shift", 64), relu=True)
    for bn in (True, False):
        g = lambda *ns: {n: t(n, 64) if bn else None for n in ns}
        run(ops.fc_bn_act_fwd, bn, x=t("x", B, C), weight=t("weight", 64, C), bias=t("bias", 64), **g("gamma", "beta", "running_mean", "running_var"),
            momentum=0.1, eps=1e-5, relu=True)
        run(ops.fc_bn_act_bwd, bn, gy=t("gy", B, 64), y=t("y", B, 64), xhat=t("xhat", B, 64) if bn else None, **g("invstd", "gamma"), x=t("x", B, C),
            relu=True, want_dw=bn)
    run(ops.fc_dx, True, dz=t("dz", B, 64), weight=t("weight", 64, C))
    table(ops.fc_head_ok, [(t("x", B, C), t("w", 64, C)), (t("x", 129, C), t("w", 64, C)), (t("x", B, 30), t("w", 64, 30)), (t("x", B, C, dt=H), t("w", 64, C))])
    pg = lambda: dict(pred=t("pred", B, 3, M), gt=t("gt", B, 3, N))
    run(ops.chamfer_nn, True, q=t("q", B, 3, M), db=t("db", B, 3, N))
    run(ops.chamfer_terms, True, **pg())
    run(ops.chamfer_terms, **pg(), want_nn=False, want_elems=False)
    run(ops.chamfer_loss, True, **pg())
    def terms():
        r = ops.chamfer_terms(t("pred", B, 3, M), t("gt", B, 3, N))
        return [named(n, getattr(r, n)) for n in ("nn_pg", "nn_gp", "elem_fwd", "elem_bwd")] and r
    run(ops.chamfer_grad, True, **pg(), terms=terms(), gscale=t("gscale", 2))
    run(ops.upconv3x3, True, x=t("x", B, 5, 4, 3), wp=named("wp", ops.upconv3x3_pack(t("w", 32, 5, 3, 3))), scale=t("scale", 32), shift=t("shift", 32), relu=True, Cout=32)
    run(ops.upconv3x3, x=t("x", B, 5, 65, 3), wp=named("wp", ops.upconv3x3_pack(t("w", 32, 5, 3, 3))), scale=t("scale", 32), shift=t("shift", 32), relu=True, Cout=32)
    run(ops.upconv3x3_dgrad, True, g=t("g", B, 32, 8, 6), wpt=named("wpt", ops.upconv3x3_dgrad_pack(t("w", 32, 5, 3, 3))), Cin=5)
    run(ops.upconv3x3_wgrad, True, g=t("g", B, 32, 8, 6), x=t("x", B, 5, 4, 3))
    table(ops.upconv3x3_supported, [(5, 32, 4, 3), (5, 48, 4, 3), (0, 32, 4, 3), (5, 32, 65, 3)])
    for wp in (False, True):
        run(ops.seg_metrics, not wp, score=t("score", B, 50, N), seg=t("seg", B, N, dt=J), label=t("label", B, dt=J), want_pred=wp)
    run(ops.seg_metrics, score=t("score", B, 6, N), seg=t("seg", B, N, dt=J), label=t("label", B, dt=J), part_offsets=(0, 2, 2, 6))
    rl = lambda: dict(feat=t("feat", N, C), labels=t("labels", N, dt=J), ids=t("ids", N, dt=J))
    run(ops.retrieval_lists, True, **rl(), query=i("query", 3), top=5, n_label=7, want_pos=True)
    run(ops.retrieval_lists, feat=t("feat", N, C), top=5)
    run(ops.retrieval_lists, **rl(), top=5)
    run(ops.retrieval_lists, **rl(), query=[0, 1], top=5, n_label=7)
    run(ops.retrieval_lists, **rl(), query=[0, 16], top=5, n_label=7)
    ab = lambda: dict(src=t("src", 6, 99), offsets=t("offsets", 4, dt=J), nodes_src=t("nodes_src", 3, M, 3), idx=t("idx", B, dt=J), N=N, K=K,
                      flags=ops.BATCH_TRAIN, seed=-1, step=2 ** 63)
    run(ops.assemble_batch, True, **ab())
    run(ops.assemble_batch, True, **ab(), replay_idx=t("replay_idx", B, N, dt=J), replay_draws=t("replay_draws", B, ops.batch_draw_size(N, M), dt=D),
        want_draws=True)
    run(ops.mfma_f16_sustained_rate)
    print("# not recorded")
    run(ops.h3_weight_ok, weight2d=t("w", 64, C))
    run(ops.assemble_batch, **ab(), sizes=[33, 33, 33])
    run(ops.run_guarded, call=h3_launch, device="cuda:0", can_rerun=True)


def summarise(text):
    out, cur = [], {}
    for line in text.splitlines():
        if line.startswith("# "):
            out.append([line, cur := {}])
        elif line.startswith("== "):
            name = line[3:].split("(")[0]
            cur.setdefault(name, []).append(line)
        else:
            cur[name].append(line)
    return "".join("%s\n%s" % (h, "".join("  %s: %d lines, %s\n" % (k, len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()[:12])
                                           for k, v in c.items())) for h, c in out)


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    setup(TREE)
    with contextlib.nullcontext() if REAL else torch._subclasses.FakeTensorMode():
        layers(REAL_SHAPES if REAL else SHAPES)
        if not REAL:
            rest()
