#!/usr/bin/env python
"""tools/layer_calls.py TREE [--real] -- what the modules and autograd nodes of TREE/so-net_amd/models/layers.py (and the parts of
networks.py built on them) call, without a GPU.  Built on tools/op_calls.py: the same fake CUDA tensors, the same recording stand-in
for the library (``setup``, ``Proxy``), the same naming of operands (``named``, ``show``) and the same outline (``summarise``).

Per case the output holds, in order: the C-ABI calls with their arguments as op_calls.py prints them; the side stream's ``enter`` /
``keep`` / ``reads`` / ``join(defer=...)`` (a recording stand-in for ``ops.side_stream``: no stream is created); the aten operators that
move data between the launches (a TorchDispatchMode: name and output shapes; pure views, allocations and metadata queries -- ``QUIET``
-- and 0-dim results, which a machine without a device places by a copy and one with a device directly, are left out), so that an
added copy or cast shows; then what comes back (``->``) or the refusal with its text (``!!``).

``loss.backward()`` needs a device, so the backward pass is WALKED here (``walk``): every node reachable from the roots runs once, in
decreasing ``_sequence_nr()`` -- the engine's order on one device --, Python nodes through ``apply``, C++ nodes by calling them; the
gradients of a tensor with two consumers are summed (``add``, as the engine's input buffer does here); a leaf stores its first gradient
-- through a copy into the parameter's layout where its strides differ -- and adds later ones in place, as AccumulateGrad does in a
no-grad pass, without running hooks.  ``ops._graph_task_id`` counts the walks (``_GradCarry``
and ``_grad_slot_empty`` tell passes apart by it) and ``ops.h3_weight_ok`` -- the one host read on the way -- answers ``H3[0]``.
Cases that read tensor VALUES on the host are listed under ``not recorded`` with the call that stopped them; the GPU suite owns them.

--real: the training cases of the layers, ``forward_pooled``, ``MyLinear`` and ``UpConv`` whose route depends on no size threshold
(B = 2, 32 -> 64 and 48 + 16 -> 64, L in {8, 33}; the up-convolution 2 x 16 x 4 x 4), first on fake tensors with the walked backward
(``#### fake``), then on real CUDA tensors through ``loss.backward()`` (``#### real``), both against the stand-in library: nothing is
launched.  tests/test_gpu_layer_calls.py holds the walker and the fake tensors to what the real engine does."""
import contextlib
import os
import re
import sys
import types
import warnings

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import op_calls
from op_calls import F, H, I, J, LINES, NAMES, KEEP, Proxy, named, setup, sh, show, summarise      # noqa: F401 (Proxy: the stand-in's class)

TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ""
REAL = "--real" in sys.argv
FAKE = [True]                        # the tensors of the running pass are fake (the backward is walked)
H3 = [True]                          # what the stand-in for ops.h3_weight_ok answers
WALK = [0, -1]                       # walks so far, id of the running one (-1: outside a walk)
FLAGS = ("BNB_ON_LOAD", "BF16_BNB_ON_LOAD", "STATS_EPILOGUE", "PACK_REGISTRY", "WGRAD_KERNEL", "GRAD_CARRY", "DEFER_WGRAD_JOIN")
# views, allocations and metadata: not data movement
QUIET = set("""view _unsafe_view reshape _reshape_alias t transpose permute expand slice select narrow unsqueeze squeeze detach alias as_strided
    empty empty_like empty_strided new_empty new_empty_strided zeros zeros_like new_zeros ones ones_like new_ones full full_like new_full
    unbind split split_with_sizes chunk view_as expand_as lift_fresh is_pinned sym_size sym_stride sym_numel sym_storage_offset is_same_size
    dim numel size stride is_contiguous arange _pin_memory record_stream detach_ unsafe_split resize_ set_ _has_compatible_shallow_copy_type
    is_non_overlapping_and_dense sym_is_contiguous device""".split())
ops = L = N = None


class Aten(TorchDispatchMode):
    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func._schema.name.split("::")[1]
        if name not in QUIET and not (isinstance(out, torch.Tensor) and out.dim() == 0):
            LINES.append("  aten.%s -> %s" % (name, show(out)))
        return out


class SideStream:
    """Recording stand-in for ``ops.side_stream``: the same ``on`` test, every call one line, no stream."""

    def __init__(self, device):
        self.on = bool(ops.BWD_SIDE_STREAM) and torch.device(device).type == "cuda"

    def line(self, text):
        if self.on:
            LINES.append("  side_stream " + text)

    def __enter__(self):
        self.line("enter")
        return self

    def __exit__(self, *exc):
        self.line("exit")
        return False

    def keep(self, t):
        self.line("keep %s" % show(t))
        return t

    def reads(self, *ts):
        self.line("reads %s" % show(tuple(t for t in ts if t is not None)))

    def join(self, defer=False):
        self.line("join(defer=%r)" % bool(defer))


def prepare(tree):
    global ops, L, N
    setup(tree)
    ops = op_calls.ops
    from models import layers, networks
    L, N = layers, networks
    ops.side_stream = SideStream
    ops.h3_weight_ok = lambda weight2d: H3[0]
    ops._TIMING = None                                   # (the labels of timed launches are op_calls.py's subject)
    torch.cuda.Event = type("Event", (), dict(__init__=lambda self, **k: None, record=lambda self: None, query=lambda self: False))


# ---------------------------------------------------------------------------------------------------------------------------------
# the backward pass, walked
# ---------------------------------------------------------------------------------------------------------------------------------
def walk(roots):
    """roots: [(tensor, gradient)].  See the module docstring for the rule."""
    WALK[0] += 1
    WALK[1] = WALK[0]
    try:
        nodes, stack = {}, [y.grad_fn for y, _ in roots if y.grad_fn is not None]
        while stack:
            n = stack.pop()
            if n is None or n in nodes:
                continue
            nodes[n] = [None] * max(1, len(getattr(n, "_input_metadata", ())) or 1)
            stack.extend(f for f, _ in n.next_functions)

        def feed(n, nr, g):
            if g is None or n is None:
                return
            want = n.variable.shape if type(n).__name__ == "AccumulateGrad" else n._input_metadata[nr].shape
            if tuple(g.shape) != tuple(want):                 # (a broadcast operand: the engine's validate_outputs)
                g = g.sum_to_size(want)
            dt = n.variable.dtype if type(n).__name__ == "AccumulateGrad" else n._input_metadata[nr].dtype
            if g.dtype != dt:
                g = g.to(dt)
            if type(n).__name__ == "AccumulateGrad":
                p = n.variable
                with torch.no_grad():
                    if p.grad is None:
                        p.grad = g.detach() if g.stride() == p.stride() else torch.empty_strided(p.size(), p.stride(), dtype=g.dtype, device=g.device).copy_(g)
                    else:
                        p.grad.add_(g)
                return
            buf = nodes[n]
            if nr >= len(buf):
                buf.extend([None] * (nr + 1 - len(buf)))
            if buf[nr] is None:
                buf[nr] = g
            else:
                with torch.no_grad():
                    buf[nr] = buf[nr] + g

        for y, g in roots:
            feed(y.grad_fn, y.output_nr, g)
        for n in sorted((n for n in nodes if type(n).__name__ != "AccumulateGrad"), key=lambda n: -n._sequence_nr()):
            with torch.no_grad():
                out = n.apply(*nodes[n]) if hasattr(n, "apply") and hasattr(n, "saved_tensors") else n(*nodes[n])
            out = out if isinstance(out, (tuple, list)) else (out,)
            if hasattr(n, "needs_input_grad"):              # (a Python node answers for every argument, its edges are the tensors' only)
                out = [g for g, need in zip(out, n.needs_input_grad) if need]
                edges = [e for e in n.next_functions if e[0] is not None]
            else:
                edges = n.next_functions
            for (f, nr), g in zip(edges, out):
                feed(f, nr, g)
    finally:
        WALK[1] = -1


def backward(roots, leaves):
    """The backward pass from ``roots`` ([(tensor, gradient shape donor or None)]) -> the gradients the named leaves hold afterwards."""
    roots = [(y, torch.ones_like(y)) for y in roots if y is not None and y.requires_grad]
    LINES.append("  backward")
    if roots:
        if FAKE[0]:
            walk(roots)
        else:
            torch.autograd.backward([y for y, _ in roots], [g for _, g in roots], retain_graph=True)
            torch.cuda.synchronize()
    LINES.append("  grads %s" % ", ".join("%s=%s" % (n, show(t.grad) if t.grad is not None else None) for n, t in leaves))


def case(label, fn):
    """One case: ``fn()`` -> what to show after ``->``."""
    print("== " + label)
    del LINES[:]
    ops._CONST.clear()
    ops.packs.entries.clear()
    ops.packs.tables.clear()
    H3[0] = True
    try:
        with Aten():
            out = "-> " + show(fn())
    except Exception as e:
        out = "!! %s: %s" % (type(e).__name__, str(e).split("\n")[0].replace(TREE, "TREE"))
    print("\n".join((LINES if FAKE[0] else [unpointer(l) for l in LINES]) + ["  " + out]))
    NAMES.clear()
    del KEEP[:]


def unpointer(line):
    """Real tensors: an address inside a named tensor's storage (the pack registry hands the library the weight's) -> its byte offset, which is
    what a fake tensor's ``data_ptr()`` is."""
    def offset(m):
        v = int(m.group())
        for x in KEEP:
            base = x.untyped_storage().data_ptr()
            if base <= v <= base + x.untyped_storage().nbytes():
                return str(v - base)
        return m.group()
    return re.sub(r"\b\d{11,}\b", offset, line)


@contextlib.contextmanager
def setting(**kw):
    old = {k: getattr(ops, k) for k in kw}
    for k, v in kw.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def t(name, *shape, dt=F, grad=False, dev="cuda:0"):
    x = torch.empty(shape, dtype=dt, device=dev)
    if grad:
        x.requires_grad_(True)
    return named(name, x)


def module(make, train=True, wgrad=True, prefix=""):
    """A module built on the device, its parameters and buffers named after their state_dict keys."""
    with torch.device("cuda:0"):
        m = make()
    m.train(train)
    for n, p in list(m.named_parameters()) + list(m.named_buffers()):
        named(prefix + n, p)
        if isinstance(p, torch.nn.Parameter):
            p.requires_grad_(wgrad)
    return m


def leaves(m, *xs):
    return [(NAMES[id(x)], x) for x in xs if x is not None and x.requires_grad] + [(n, p) for n, p in m.named_parameters() if p.requires_grad]


def grad_mode(phase):
    return torch.no_grad() if phase == "nograd" else contextlib.nullcontext()


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def layer_case(cls, prec, phase, norm, act, shape, skip, xg, wg, dt=F):
    B, C1, C2, Co, Lc = shape
    if not skip:
        C1, C2 = C1 + C2, 0
    label = "%s(%s %s norm=%s act=%s %dx%d%s->%dx%d grad=%s%s)" % (cls.__name__, prec, phase, norm, act, B, C1, "+%d" % C2 if C2 else "", Co, Lc,
                                                                   "x" * xg + "w" * wg or "-", "" if dt == F else " " + op_calls.SHORT[dt])

    def run():
        with setting(POINTMLP_PRECISION=prec):
            if cls is L.EquivariantLayer:
                m = module(lambda: cls(C1 + C2, Co, act, norm), phase == "train", wg)
                x = t("x", B, C1, Lc, dt=dt, grad=xg)
                xs = t("x_skip", B, C2, Lc, dt=dt, grad=xg) if C2 else None
                with grad_mode(phase):
                    y = m(x, None, x_skip=xs) if C2 else m(x)
                x1, x2 = (xs, x) if C2 else (x, None)
            else:
                m = module(lambda: cls(C1, Co, 1, activation=act, normalization=norm), phase == "train", wg)
                x1, x2 = t("x", B, C1, Lc, 1, dt=dt, grad=xg), None
                with grad_mode(phase):
                    y = m(x1)
            if phase != "nograd":
                backward([y], leaves(m, x1, x2))
            return y
    case(label, run)


SMALL = op_calls.REAL_SHAPES                                        # (B, C1, C2, Cout, L): 32 -> 64 and 48 + 16 -> 64, L in {8, 33}
# the workload's shapes on either side of each threshold of layers.py: _stats_epilogue_ok's 32 MB (8 x 128 x 8192 x 4 bytes) and the
# 65536 columns of the bf16 bnb path; _wgrad's four size tests; _F32_DGRAD_ROWS; the 387 / 515 input channels _pack_transposed pads
SIZES = [(8, 64, 0, 128, 8192), (8, 64, 0, 128, 8190), (8, 64, 0, 128, 16384), (8, 384, 0, 512, 64), (8, 128, 0, 256, 512), (8, 128, 0, 256, 504),
         (2, 1056, 0, 64, 8), (2, 1024, 0, 64, 8), (2, 387, 0, 64, 8), (2, 515, 0, 64, 8), (2, 387, 0, 512, 64)]


def layer_cases(real):
    print("# layers")
    EL, MC = L.EquivariantLayer, L.MyConv2d
    for shape in SMALL:
        for prec in ("h3", "x3", "bf16", "f32"):
            layer_case(EL, prec, "train", "batch", "relu", shape, True, True, True)
            layer_case(EL, prec, "train", None, "relu", shape, True, True, True)
    layer_case(MC, "h3", "train", "batch", "relu", SMALL[0], False, True, True)
    if real:
        return
    shape = SMALL[2]
    for prec in ("h3", "x3", "bf16", "f32"):
        for phase in ("train", "eval", "nograd"):
            for norm in (None, "batch", "instance"):
                for act in (None, "relu", "elu"):
                    if prec != "h3" and (act == "elu" or norm == "instance") and phase != "train":
                        continue
                    for skip in (False, True):
                        for xg, wg in ((True, True),) if phase == "nograd" else ((True, False), (False, True), (True, True)):
                            if (xg, wg) != (True, True) and (act == "elu" or norm == "instance"):
                                continue
                            layer_case(EL, prec, phase, norm, act, shape, skip, xg, wg)
            for norm in (None, "batch"):
                layer_case(MC, prec, phase, norm, "relu", SMALL[1], False, True, True)
        layer_case(EL, prec, "train", "batch", "relu", shape, True, True, True, dt=H if prec != "bf16" else F)
        for s in SIZES:
            layer_case(EL, prec, "train", "batch", "relu", s, False, True, True)
            if s[1] in (387, 515):
                layer_case(EL, prec, "train", None, None, s, False, True, True)
    case("EquivariantLayer(CPU tensor)", lambda: module(lambda: EL(32, 64, "relu", "batch"))(named("x", torch.empty(2, 32, 8, device="cpu"))))
    case("MyConv2d(CPU tensor)", lambda: module(lambda: MC(32, 64, 1))(named("x", torch.empty(2, 32, 8, 1, device="cpu"))))
    case("MyConv2d(3x3)", lambda: module(lambda: MC(8, 16, 3, padding=1, normalization="batch", activation="relu"))(t("x", 2, 8, 4, 4)))


def resnet(train=True, channels=(64, 128, 256, 384)):
    return module(lambda: L.PointResNet(6, list(channels), "relu", "batch"), train)


def pooled_case(label, prec, B, Lc, M, sorted_, need_dense, g_y, prep=None, **flags):
    def run():
        with setting(POINTMLP_PRECISION=prec, **flags):
            net = resnet()
            x = t("x", B, 6, Lc, grad=True)
            ids, row_max = t("ids", B, Lc, dt=I), t("row_max", B, M, dt=I)
            pos0 = t("pos0", B, dt=I) if sorted_ else None
            if prep is not None:
                prep(net)
            out = net.forward_pooled(x, ids, row_max, M, None, need_dense, pos0)
            if out is None:
                return None
            backward([out[1]] + ([out[0]] if g_y else []), leaves(net, x))
            return out
    case("forward_pooled(%s %s %dx6x%d M=%d sorted=%s need_dense=%s g_y=%s%s)" % (
        label, prec, B, Lc, M, sorted_, need_dense, g_y, "".join(" %s=%s" % kv for kv in flags.items())), run)


def flip(after):
    """A verdict that holds for ``after`` questions and is False from then on (the weight side of the range guard between check and use)."""
    left = [after]

    def ok():
        left[0] -= 1
        return left[0] >= 0
    return ok


def force_last_x3(net):
    net.layers[-1]._h3_ok = flip(0)


def force_hidden_x3(net):
    net.layers[2]._h3_ok = flip(1)


def pooled_cases(real):
    print("# PointResNet")
    for prec in ("h3", "bf16", "x3", "f32"):
        for Lc in (8, 33):
            for sorted_ in (False, True):
                pooled_case("small", prec, 2, Lc, 4, sorted_, not sorted_, not sorted_)
        pooled_case("small", prec, 2, 8, 4, False, False, False)
    pooled_case("small, last layer to x3", "h3", 2, 8, 4, True, False, False, prep=force_last_x3)
    if real:
        return
    for prec in ("h3", "bf16"):
        for sorted_ in (False, True):
            for need_dense in (False, True):
                for g_y in ((False, True) if need_dense else (False,)):
                    pooled_case("workload", prec, 8, 8192, 64, sorted_, need_dense, g_y)
        pooled_case("below the statistics epilogue", prec, 8, 8190, 64, prec == "h3", False, False)
        for flag in FLAGS:
            pooled_case("workload", prec, 8, 8192, 64, prec == "h3", False, False, **{flag: False})
    pooled_case("workload, last layer to x3", "h3", 8, 8192, 64, True, False, False, prep=force_last_x3)
    pooled_case("workload, hidden layer to x3", "h3", 8, 8192, 64, True, False, False, prep=force_hidden_x3)
    pooled_case("workload, odd first width", "h3", 8, 8192, 64, True, False, False, prep=lambda net: net.out_channels_list.__setitem__(0, 63))
    for prec in ("h3", "bf16", "x3"):
        for phase in ("train", "eval", "nograd"):
            for emit in (False, True, "only"):
                if emit and (phase != "nograd" or prec != "h3"):
                    continue

                def run(prec=prec, phase=phase, emit=emit):
                    with setting(POINTMLP_PRECISION=prec):
                        net = resnet(phase == "train")
                        net.emit_p16 = emit
                        x = t("x", 2, 6, 64, grad=phase != "nograd")
                        with grad_mode(phase):
                            y = net(x)
                        if phase != "nograd":
                            backward([y], leaves(net, x))
                        return y, net.last_p16
                case("PointResNet.forward(%s %s emit_p16=%s)" % (prec, phase, emit), run)

    def other(channels):
        net = resnet(True, channels)
        x = t("x", 2, 6, 8, grad=True)
        y = net(x)
        backward([y], leaves(net, x))
        return y
    case("PointResNet.forward(skip of 12 channels: concatenated)", lambda: other((12, 32, 64)))

    def fn_refusal(pos0, wp_mode):
        net = resnet()
        last = net.layers[-1]
        with setting(POINTMLP_PRECISION=wp_mode):
            wp = last._packed(64, 256)
        aff = tuple(v for _ in range(2) for v in (t("s", 64 if _ == 0 else 256), t("h", 64 if _ == 0 else 256), True))
        return L._PooledLastLayerFn.apply(t("x1", 2, 64, 8), t("x2", 2, 256, 8), last._weight2d(), last._bias(), wp, t("ids", 2, 8, dt=I),
                                          t("row_max", 2, 4, dt=I), 4, False, t("pos0", 2, dt=I) if pos0 else None, aff, None)
    case("_PooledLastLayerFn(xaff without the sorted form)", lambda: fn_refusal(False, "h3"))
    case("_PooledLastLayerFn(xaff, sorted, x3 pack)", lambda: fn_refusal(True, "x3"))


def pointwise_cases():
    print("# _PointwiseFn")
    def run_defer(prec, Lc, dt, xaff, carry, wg=True, **flags):
        def run():
            with setting(POINTMLP_PRECISION=prec, **flags):
                m = module(lambda: L.EquivariantLayer(64, 128, "relu", "batch"), True, wg)
                x = t("x", 8, 64, Lc, dt=dt, grad=True)
                c = L._GradCarry() if carry else None
                (raw, sc, sh_), act = m._run(x, None, None, xaff=(t("s1", 64), t("h1", 64), True) if xaff else None, defer=True, carry=c)
                LINES.append("  backward")
                WALK[0] += 1
                WALK[1] = WALK[0]
                try:
                    if carry:
                        c.put(t("carried", 8, 64, Lc, dt=dt))
                    with torch.no_grad():
                        g = raw.grad_fn.apply(torch.ones_like(raw), None, None, None, None)
                finally:
                    WALK[1] = -1
                return (raw, sc, sh_), act, g
        case("_run(defer %s 8x64x%d xaff=%s carry=%s%s%s)" % (prec, Lc, xaff, carry, "" if wg else " weight frozen",
                                                              "".join(" %s=%s" % kv for kv in flags.items())), run)
    for prec, dt in (("h3", F), ("bf16", H)):
        for Lc in (8192, 8190):
            for xaff in (False, True):
                for carry in (False, True):
                    run_defer(prec, Lc, dt, xaff, carry)
        run_defer(prec, 8192, dt, True, True, wg=False)
        for flag in FLAGS:
            run_defer(prec, 8192, dt, True, True, **{flag: False})

    def eval_defer():
        m = module(lambda: L.EquivariantLayer(64, 128, "relu", "batch"), False)
        return m._run(t("x", 8, 64, 8192), None, None, defer=True)
    case("_run(defer on an eval-mode layer)", eval_defer)

    def fn_xaff_small():
        m = module(lambda: L.EquivariantLayer(32, 64, "relu", "batch"))
        bn = m.norm
        return L._PointwiseFn.apply(t("x", 2, 32, 8), None, m._weight2d(), m._bias(), bn.weight, bn.bias, m._packed(32, 0), None, None, True,
                                    "batch", bn.eps, None, (t("s1", 32), t("h1", 32), True), False, None)
    case("_PointwiseFn(xaff below the statistics epilogue)", fn_xaff_small)

    def unused_output():
        m = module(lambda: L.EquivariantLayer(32, 64, "relu", "batch"))
        c = L._GradCarry()
        y = m._run(t("x", 2, 32, 8, grad=True), None, None)[0]
        WALK[1] = WALK[0] = WALK[0] + 1
        c.put(t("carried", 2, 32, 8))
        y.grad_fn.carry = c
        try:
            return y.grad_fn.apply(None, None, None)
        finally:
            WALK[1] = -1
    case("_PointwiseFn.backward(output unused, gradient in the carry)", unused_output)


def heads_cases(real):
    print("# MyLinear")
    def lin(B, norm, act, phase, dt=F):
        def run():
            m = module(lambda: L.MyLinear(32, 64, act, norm), phase == "train")
            x = t("x", B, 32, dt=dt, grad=phase != "nograd")
            with grad_mode(phase):
                y = m(x)
            if phase != "nograd":
                backward([y], leaves(m, x))
            return y
        case("MyLinear(%s norm=%s act=%s B=%d %s)" % (phase, norm, act, B, op_calls.SHORT[dt]), run)
    lin(2, "batch", "relu", "train")
    lin(2, None, None, "train")
    print("# UpConv")
    def up(phase, norm, act, fused, fused_train, fused_wgrad, xg=True):
        def run():
            m = module(lambda: L.UpConv(16, 32, activation=act, normalization=norm), phase == "train")
            m.fused, m.fused_train, m.fused_wgrad = fused, fused_train, fused_wgrad
            x = t("x", 2, 16, 4, 4, grad=xg and phase != "nograd")
            with grad_mode(phase):
                y = m(x)
            if phase != "nograd":
                backward([y], leaves(m, x))
            return y
        case("UpConv(%s norm=%s act=%s fused=%s fused_train=%s fused_wgrad=%s%s)" % (phase, norm, act, fused, fused_train, fused_wgrad,
                                                                                 "" if xg else " input without grad"), run)
    for norm in ("batch", None):
        for wgrad in (False, True):
            up("train", norm, "relu", False, True, wgrad)
    up("train", "batch", "relu", False, True, True, xg=False)
    if real:
        return
    up("nograd", "batch", "relu", True, False, False)
    up("nograd", None, None, True, False, False)
    up("train", "batch", "elu", True, True, True)
    up("eval", "batch", "relu", False, False, False)
    print("# MyLinear, the other paths")
    lin(1, "batch", "relu", "train")
    lin(2, "batch", "relu", "nograd")
    lin(2, None, "relu", "eval")
    lin(2, "batch", "elu", "train")
    lin(2, "instance", "relu", "train")
    lin(2, "batch", "relu", "train", dt=H)
    lin(200, "batch", "relu", "train")


def stack_cases():
    print("# PointNet.forward_cat, KNNModule")
    for prec in ("h3", "bf16", "x3"):
        for phase in ("nograd", "train"):
            def cat(prec=prec, phase=phase):
                with setting(POINTMLP_PRECISION=prec):
                    m = module(lambda: L.PointNet(3 + 32, [64, 128], "relu", "batch"), phase == "train")
                    with grad_mode(phase):
                        return m.forward_cat(t("lead", 2, 3, 8), t("x", 2, 32, 8))
            case("PointNet.forward_cat(%s %s)" % (prec, phase), cat)
            for split in (True, False):
                def knn(prec=prec, phase=phase, split=split, dt=F):
                    with setting(POINTMLP_PRECISION=prec, NODE_LINEAR_SPLIT=split):
                        m = module(lambda: L.KNNModule(3 + 32, [64, 128], "relu", "batch"), phase == "train")
                        x = t("x", 2, 32, 8, grad=phase == "train")
                        with grad_mode(phase):
                            out = m(t("coord", 2, 3, 8), x, t("knn_I", 2, 8, 4, dt=J), 3, "avg")
                        if phase == "train":
                            backward([out[1]], leaves(m, x))
                        return out
                case("KNNModule(%s %s NODE_LINEAR_SPLIT=%s)" % (prec, phase, split), knn)
    def knn_other(**kw):
        with setting(**kw):
            m = module(lambda: L.KNNModule(3 + 32, [64, 128], "relu", "batch"), False)
            with torch.no_grad():
                return m(t("coord", 2, 3, 8), t("x", 2, 32, 8), None, 3, "center")
    case("KNNModule(nograd, GATHER_NODE_STAGE off, own neighbour search)", lambda: knn_other(GATHER_NODE_STAGE=False))


def seg_opt():
    return types.SimpleNamespace(feature_num=64, surface_normal=True, som_k=2, activation="relu", normalization="batch", dropout=0.0, classes=50,
                                 k=2, input_pc_num=16, seg_nodewise_train=True)


def nodewise_cases():
    print("# _NodewiseLayerFn")
    def inputs(B, n, k, M, grad):
        kN = k * n
        return dict(x_decentered=t("x_dec", B, 3, kN), x=t("x", B, 3, n), sn=t("sn", B, 3, n), label=t("label", B, dt=J),
                    first_pn_out=t("first", B, 384, kN, grad=grad), som_node=t("som_node", B, 3, M), masked_max=t("masked_max", B, 384, M, grad=grad),
                    knn_feature_1=t("knn_feature_1", B, 512, M, grad=grad), final_pn_out=t("final", B, 64, M, grad=grad),
                    feature=t("feature", B, 64, grad=grad), min_idx_i32=t("ids", B, kN, dt=I))

    def through_segmenter():
        seg = module(lambda: N.Segmenter(seg_opt()))
        kw = inputs(2, 16, 2, 4, True)
        y = seg.forward_nodewise_train(**kw)
        backward([y], leaves(seg, *[v for v in kw.values() if v.requires_grad]))
        return y
    case("Segmenter.forward_nodewise_train", through_segmenter)

    def direct(relu):
        seg = module(lambda: N.Segmenter(seg_opt()))
        lyr, bn = seg.layer1, seg.layer1.norm
        B, kN, M = 2, 32, 4
        a = [t("x1", B, 384, kN, grad=True), t("x2", B, 9, kN), t("node_lead", B, 3, M), t("node_maps", B, 960, M, grad=True), t("glob_lead", B, 16),
             t("glob", B, 64, grad=True)]
        y, mean, var = L._NodewiseLayerFn.apply(*a, lyr._weight2d(), lyr._bias(), bn.weight, bn.bias, t("ids", B, kN, dt=I), seg._layer1_split_train(),
                                                relu, bn.eps, None)
        backward([y], leaves(lyr, a[0], a[3], a[5]))
        return y, mean, var
    case("_NodewiseLayerFn(relu, no running statistics)", lambda: direct(True))
    case("_NodewiseLayerFn(no activation)", lambda: direct(False))

    def nodewise_eval(prec):
        with setting(POINTMLP_PRECISION=prec):
            seg = module(lambda: N.Segmenter(seg_opt()), False)
            with torch.no_grad():
                return seg.forward_nodewise(**inputs(2, 16, 2, 4, False))
    for prec in ("h3", "bf16", "x3"):
        case("Segmenter.forward_nodewise(%s)" % prec, lambda prec=prec: nodewise_eval(prec))


def cache_cases():
    print("# caches")
    def thrice(label, make, call, weight, between=None):
        def run():
            m = make()
            out = []
            for step in ("first", "again", "after an update"):
                LINES.append("  -- " + step)
                if step == "after an update":
                    torch.autograd.graph.increment_version(weight(m))
                with torch.no_grad():
                    out.append(call(m))
            if between is not None:
                LINES.append("  -- after a training forward")
                between(m)
                with torch.no_grad():
                    out.append(call(m))
            return out[0]
        case(label, run)
    el = lambda: module(lambda: L.EquivariantLayer(35, 64, "relu", "batch"), False)
    w = lambda m: m.conv.weight
    for prec in ("h3", "bf16"):
        with setting(POINTMLP_PRECISION=prec):
            thrice("_packed(%s)" % prec, el, lambda m: m._packed(), w)
            with setting(PACK_REGISTRY=False):
                thrice("_packed(%s PACK_REGISTRY=False)" % prec, el, lambda m: m._packed(), w)
            thrice("_packed_rotated(%s)" % prec, el, lambda m: m._packed_rotated(3), w)
            thrice("_packed_split(%s)" % prec, el, lambda m: m._packed_split(3), w)
    thrice("_packed_p16", el, lambda m: m._packed_p16(), w)
    thrice("_packed_p16(tag)", el, lambda m: (m._packed_p16(), m._packed_p16(lambda: m._weight2d().detach()[:, :32], "point")), w)
    thrice("_lead_cols", el, lambda m: m._lead_cols(3), w)

    def train_forward(m):
        m.train()
        m(t("x", 2, 35, 8) if isinstance(m, L.EquivariantLayer) else t("x", 2, 32))
        m.eval()
    thrice("_FusedPointwise._eval_affine", el, lambda m: m._eval_affine(), lambda m: m.norm.weight, train_forward)
    thrice("_FusedPointwise._eval_affine(no norm)", lambda: module(lambda: L.EquivariantLayer(35, 64, None, None), False), lambda m: m._eval_affine(),
           lambda m: m.conv.bias)
    lin = lambda: module(lambda: L.MyLinear(32, 64, "relu", "batch"), False)
    thrice("MyLinear._eval_affine", lin, lambda m: m._eval_affine(), lambda m: m.norm.weight, train_forward)
    thrice("MyLinear._eval_affine(no norm)", lambda: module(lambda: L.MyLinear(32, 64, None, None), False), lambda m: m._eval_affine(),
           lambda m: m.linear.bias)
    up = lambda: module(lambda: L.UpConv(16, 32, activation="relu", normalization="batch"), False)
    wu = lambda m: m.conv.conv.weight
    thrice("_packed_upconv", up, lambda m: m._packed_upconv(), wu)
    thrice("_packed_upconv_dgrad", up, lambda m: m._packed_upconv_dgrad(), wu)
    for prec in ("h3", "bf16"):
        with setting(POINTMLP_PRECISION=prec):
            thrice("_fused_state(%s)" % prec, lambda: resnet(False), lambda m: m._fused_state(), lambda m: m.layers[1].conv.weight)
            thrice("_layer1_split(%s)" % prec, lambda: module(lambda: N.Segmenter(seg_opt()), False), lambda m: m._layer1_split(),
                   lambda m: m.layer1.conv.weight)
    thrice("_layer1_split_train", lambda: module(lambda: N.Segmenter(seg_opt())), lambda m: m._layer1_split_train(), lambda m: m.layer1.conv.weight)


def slot_cases():
    print("# _grad_slot_empty")
    def run(label, twice=False, grad=False, hook=None, second_walk=False):
        def go():
            m = module(lambda: L.EquivariantLayer(32, 64, "relu", "batch"))
            p = m.conv.weight
            if grad:
                p.grad = t("w.grad", 64, 32, 1)
            if hook == "tensor":
                p.register_hook(lambda g: g)
            elif hook is not None:
                def h(param):
                    return None
                h._sonet_joins_side_streams = hook == "joins"
                p.register_post_accumulate_grad_hook(h)
            x = t("x", 2, 32, 8, grad=True)
            y = m(x) + m(x) if twice else m(x)
            backward([y], leaves(m, x))
            if second_walk:
                p.grad = None
                y2 = m(x)                                     # (``y`` and its graph stay alive)
                backward([y2], leaves(m, x))
                LINES.append("  -- the first graph again")
                backward([y], leaves(m, x))
            return y
        case("_grad_slot_empty(%s)" % label, go)
    run("one use")
    run("a weight used twice in one graph", twice=True)
    run(".grad already present", grad=True)
    run("a tensor hook", hook="tensor")
    run("a post-accumulate hook", hook="plain")
    run("a post-accumulate hook that joins the side streams", hook="joins")
    run("a second walk, the first graph kept alive", second_walk=True)
    with setting(BWD_SIDE_STREAM=False):
        run("BWD_SIDE_STREAM off")


def not_recorded():
    print("# not recorded")
    def real_verdict():
        m = module(lambda: L.EquivariantLayer(32, 64, "relu", "batch"), False)
        ops.h3_weight_ok, stand_in = (lambda w: bool(ops.h3_weight_ratio_flag(w).item())), ops.h3_weight_ok
        try:
            return m._h3_ok()
        finally:
            ops.h3_weight_ok = stand_in
    case("_FusedPointwise._h3_ok(the real ops.h3_weight_ok)", real_verdict)

    def seg_forward():
        seg = module(lambda: N.Segmenter(seg_opt()), False)
        e = types.SimpleNamespace()
        return N.segmentation_forward(e, seg, t("pc", 2, 3, 16), t("sn", 2, 3, 16), t("label", 2, dt=J), t("node", 2, 3, 4), None)
    case("segmentation_forward(needs an Encoder: the SOM search reads values)", seg_forward)


def subset():
    layer_cases(True)
    pooled_cases(True)
    heads_cases(True)


def everything():
    layer_cases(False)
    pointwise_cases()
    pooled_cases(False)
    stack_cases()
    heads_cases(False)
    nodewise_cases()
    cache_cases()
    slot_cases()
    not_recorded()


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    prepare(TREE)
    ops._graph_task_id = lambda: WALK[1]
    if REAL:
        print("#### fake")
    with torch._subclasses.FakeTensorMode():
        subset() if REAL else everything()
    if REAL:
        print("#### real")
        FAKE[0] = False
        ops._graph_task_id = getattr(torch._C, "_current_graph_task_id", None)
        subset()
