"""The life cycle of ``ops.packs`` (sonet_hip.ops._PackRegistry) through ``layers.EquivariantLayer`` and ``layers._pack_transposed``: what a
weight update of any visible kind leaves in the packs, one refresh launch per step, the device table, entries dying with their weight, a
Parameter whose storage moved, and the ``.data`` contract.  Pack bytes are compared with tests/pack_ref.py; no tolerance."""
import gc
import weakref

import numpy as np
import pytest
import torch

import pack_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(64, 128), (387, 512), (3, 64)]
FLAVOUR_OF = {torch.int16: "bf16", torch.uint8: "x3", torch.int8: "h3"}


def _layer(cin, cout, seed=0):
    from models import layers as L
    lay = L.EquivariantLayer(cin, cout, "relu", "batch")
    g = torch.Generator().manual_seed(1000 * cin + cout + seed)
    with torch.no_grad():
        lay.conv.weight.copy_((torch.randn(cout, cin, 1, generator=g) * (2.0 / cin) ** 0.5))
    return lay.to(DEV).train()


def _packs(lay):
    """The registry's packs of one layer in the current precision: [(what, buffer, pack_ref arguments)] -- the forward pack and, where
    ``_pack_transposed`` takes the registry, the pack of W^T with its zero rows."""
    from models import layers as L
    cin = lay.conv.in_channels
    w2 = lay._weight2d()
    out = [("fwd", lay._packed(cin), dict(Cin=cin, Cout=w2.shape[0], rows=w2.shape[0], rs=cin, cs=1))]
    t = L._pack_transposed(w2, cin, 0)[0]
    if torch.is_tensor(t[0]) and t[0].dtype in FLAVOUR_OF:
        out.append(("t", t[0], dict(Cin=w2.shape[0], Cout=t[2], rows=t[1], rs=1, cs=cin)))
    return out


def _bytes(buf):
    return buf.view(torch.uint8).cpu().numpy()


def _assert_current(lay, what, weight=None):
    """Every pack of the layer equals pack_ref of ``weight`` (default: the layer's weight as it is now)."""
    w = (lay.conv.weight if weight is None else weight).detach().float().cpu().numpy().reshape(lay.conv.out_channels, -1)
    got = _packs(lay)
    for kind, buf, a in got:
        ref = R.PACKS[FLAVOUR_OF[buf.dtype]](w.reshape(-1), **a)
        assert np.array_equal(_bytes(buf)[:ref.size], ref), (what, kind, FLAVOUR_OF[buf.dtype], tuple(w.shape))
    return got


def _stale():
    from sonet_hip import ops
    return [k for k, e in ops.packs.entries.items() if e["ref"]() is not None and e["version"] != e["ref"]()._version]


def _settle():
    """Start from a registry without dead or stale entries, whatever ran before (other tests' models may still be alive)."""
    from sonet_hip import ops
    gc.collect()
    ops.packs.refresh(torch.device(DEV, torch.cuda.current_device()))
    torch.cuda.synchronize()
    assert not _stale()


def _names(fn):
    from sonet_hip import ops
    with ops.kernel_timing() as rec:
        out = fn()
    return [n for n, _, _ in rec.records], out


def _set_grads(lays, seed=0):
    g = torch.Generator().manual_seed(seed)
    for lay in lays:
        for p in lay.parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(DEV)


UPDATES = ["fused_adam", "sgd", "copy_", "mul_", "load_state_dict", "detach_add_"]


def _apply(kind, lay):
    from sonet_hip.optim import FusedAdam
    w = lay.conv.weight
    if kind in ("fused_adam", "sgd"):
        _set_grads([lay], 7)
        opt = FusedAdam(lay.parameters(), lr=1e-2) if kind == "fused_adam" else torch.optim.SGD(lay.parameters(), lr=0.5)
        opt.step()
    elif kind == "copy_":
        with torch.no_grad():
            w.copy_(torch.randn(w.shape, generator=torch.Generator().manual_seed(8)).to(DEV) * 0.1)
    elif kind == "mul_":
        with torch.no_grad():
            w.mul_(0.75)
    elif kind == "load_state_dict":
        sd = {k: v.clone() for k, v in lay.state_dict().items()}
        sd["conv.weight"] = sd["conv.weight"] * 0.5 + 0.01
        lay.load_state_dict(sd)
    elif kind == "detach_add_":
        w.detach().add_(0.03125)
    else:
        raise ValueError(kind)


@pytest.mark.parametrize("mode", ["h3", "x3", "bf16"])
@pytest.mark.parametrize("kind", UPDATES)
def test_packs_follow_every_visible_update(kind, mode):
    from sonet_hip import ops
    with ops.precision(mode):
        for cin, cout in SHAPES:
            lay = _layer(cin, cout)
            before = [(_bytes(b).copy(), b.data_ptr()) for _, b, _ in _assert_current(lay, "created")]
            old_w = lay.conv.weight.detach().clone()
            _apply(kind, lay)
            assert not torch.equal(old_w, lay.conv.weight.detach())
            after = _assert_current(lay, kind)
            for (ob, optr), (_, b, _a) in zip(before, after):
                assert b.data_ptr() == optr                              # refreshed into the buffer the entry owns
                assert not np.array_equal(ob, _bytes(b))


@pytest.mark.parametrize("mode", ["h3", "bf16"])
def test_one_refresh_launch_per_step_and_the_device_table(mode):
    from sonet_hip import ops
    from sonet_hip.optim import FusedAdam
    _settle()
    with ops.precision(mode):
        lays = [_layer(cin, cout) for cin, cout in SHAPES]
        made = sum(len(_packs(lay)) for lay in lays)
        assert made == 5                                             # three forward packs, two transposed ones (3 rows: the f32 kernel's)
        assert not _stale()
        opt = FusedAdam([p for lay in lays for p in lay.parameters()], lr=1e-2)
        _set_grads(lays, 1)
        opt.step()
        assert len(_stale()) == made
        names, _ = _names(lambda: lays[1]._packed(SHAPES[1][0]))
        assert names == ["pack_multi_%d" % made], names
        assert not _stale()                                          # every other entry of the device is fresh as well
        names, _ = _names(lambda: [_packs(lay) for lay in lays])
        assert names == [], names
        for lay in lays:
            _assert_current(lay, "after the step")
        _check_table(lays, made)
        # a frozen layer is not stepped: the table is rebuilt with its entries gone
        frozen = len(_packs(lays[0]))
        lays[0].requires_grad_(False)
        _set_grads(lays[1:], 2)
        for p in lays[0].parameters():
            p.grad = None
        opt.step()
        names, _ = _names(lambda: lays[2]._packed(SHAPES[2][0]))
        assert names == ["pack_multi_%d" % (made - frozen)], names
        _check_table(lays[1:], made - frozen)
        for lay in lays:
            _assert_current(lay, "after the second step")


def _check_table(lays, n):
    """The registry's device table against pack_ref.pack_table of the same entries, described from the layers (not from the registry's own
    records): source = the weight's address (+ the block's column offset), destination = the buffer ``get`` hands out."""
    from sonet_hip import ops
    keys, tab, blocks = ops.packs.tables[torch.cuda.current_device()]
    assert len(keys) == n
    by_ptr = {lay.conv.weight.data_ptr(): lay for lay in lays}
    entries = []
    for ptr_, _dev, shape, what in keys:
        lay = by_ptr[ptr_]
        cout, cin = shape
        assert (cout, cin) == (lay.conv.out_channels, lay.conv.in_channels)
        dst = ops.packs.entries[(ptr_, _dev, shape, what)]["buf"].data_ptr()
        if what[0] == "fwd":
            entries.append(dict(src=ptr_, dst=dst, rs=cin, cs=1, Cin=cin, rows=cout, Cout=cout, flavour=what[1]))
        else:
            _, fl, lo, Ci, Cp = what
            entries.append(dict(src=ptr_ + 4 * lo, dst=dst, rs=1, cs=cin, Cin=cout, rows=Ci, Cout=Cp, flavour=fl))
    want, want_blocks = R.pack_table(entries)
    assert blocks == want_blocks
    assert np.array_equal(tab.cpu().numpy(), want)


def _enc_setup():
    import test_gpu_after_update as AU
    s = AU.Setup("classifier", 8, 512, 16)
    return s, s.modules(seeds=(3, 4))


def test_steady_state_of_a_small_encoder():
    """Five training steps: the registry does not grow after the first, and every later step shows one pack_multi and no other pack launch."""
    from sonet_hip import ops
    from sonet_hip.optim import FusedAdam
    _settle()
    with ops.precision("h3"):
        s, mods = _enc_setup()
        opts = [FusedAdam(m.parameters(), lr=1e-3) for m in mods]
        base, sizes = len(ops.packs.entries), []
        for it in range(5):
            stale = len(_stale())
            names, _ = s.train_step(mods)
            for o in opts:
                o.step()
            sizes.append(len(ops.packs.entries) - base)
            packs = [n for n in names if "pack" in n]
            if it:
                assert stale == sizes[0] and packs == ["pack_multi_%d" % stale], (it, packs, stale, sizes)
            else:
                assert stale == 0 and not any(n.startswith("pack_multi") for n in names)
        assert sizes[0] > 0 and sizes == [sizes[0]] * 5, sizes


def test_entries_die_with_their_weight():
    from sonet_hip import ops
    gc.collect()
    base = len(ops.packs.entries)
    with ops.precision("h3"):
        lay = _layer(64, 128)
        n = len(_packs(lay))
        assert len(ops.packs.entries) == base + n
        ref = weakref.ref(lay.conv.weight)
        del lay
        gc.collect()
        assert ref() is None and len(ops.packs.entries) == base
        for i in range(20):                                          # a sweep that builds model after model leaves nothing behind
            lay = _layer(64, 128, seed=i)
            _assert_current(lay, "model %d" % i)
            del lay
        gc.collect()
        assert len(ops.packs.entries) == base
        # a new weight on a dead weight's address gets a pack of its own values
        lay = _layer(64, 128, seed=100)
        _assert_current(lay, "first tenant")
        addr = lay.conv.weight.data_ptr()
        del lay
        gc.collect()
        for i in range(8):
            lay = _layer(64, 128, seed=101 + i)
            if lay.conv.weight.data_ptr() == addr:
                break
            del lay
            gc.collect()
        assert lay.conv.weight.data_ptr() == addr, "the allocator never handed the dead weight's block out again"
        _assert_current(lay, "second tenant")


def _recorded_sources_are_inside_their_weights():
    """No live entry records a source address outside the current storage of the Parameter it belongs to."""
    from sonet_hip import ops
    bad = []
    for key, e in ops.packs.entries.items():
        t = e["ref"]()
        if t is None:
            continue
        src = e["rec"][0]
        if not (t.is_cuda and t.data_ptr() <= src < t.data_ptr() + 4 * t.numel()):
            bad.append((key, hex(src), hex(t.data_ptr()) if t.is_cuda else "cpu"))
    return bad


class _HostCheckBeforeLaunch:
    """Asserts the registry's bookkeeping on the HOST in front of every pack launch the registry issues (a new entry's first pack, the
    refresh launch): with an entry that still records a moved weight's old address the assertion fails before anything reads it."""

    def __init__(self, monkeypatch):
        from sonet_hip import _lib, ops
        lib = _lib.load()
        self.checked = 0
        create, multi = ops.packs._create, lib.sonet_pack_multi

        def checked_create(*a, **kw):
            self.check()
            return create(*a, **kw)

        def checked_multi(*a, **kw):
            self.check()
            return multi(*a, **kw)
        monkeypatch.setattr(ops.packs, "_create", checked_create)
        monkeypatch.setattr(lib, "sonet_pack_multi", checked_multi)

    def check(self):
        bad = _recorded_sources_are_inside_their_weights()
        assert not bad, "entries of a moved weight: %s" % (bad[:3],)
        self.checked += 1


@pytest.mark.parametrize("move", ["cpu_and_back", "data_assignment"])
@pytest.mark.parametrize("first", ["own_forward", "another_layers_refresh"])
def test_moved_storage_leaves_no_entry_behind(move, first, monkeypatch):
    from sonet_hip import ops
    _settle()
    with ops.precision("h3"):
        lay, other = _layer(387, 512), _layer(64, 128, seed=5)
        _assert_current(lay, "created")
        _assert_current(other, "created")
        w = lay.conv.weight
        old_ptr, old_version = w.data_ptr(), w._version
        if move == "cpu_and_back":
            lay.cpu()
            hog = []                                                 # (holds the freed block, so that the way back lands elsewhere)
            while len(hog) < 64 and not any(h.data_ptr() <= old_ptr < h.data_ptr() + 4 * h.numel() for h in hog):
                hog.append(torch.empty(w.numel(), device=DEV))
            lay.to(DEV)
            del hog
        else:
            w.data = w.data.clone()
        assert lay.conv.weight is w and w.data_ptr() != old_ptr and w._version == old_version
        guard = _HostCheckBeforeLaunch(monkeypatch)
        if first == "own_forward":
            _assert_current(lay, "after the move")                   # new entries at the new address; the old ones are gone first
        else:
            _set_grads([other], 3)
            torch.optim.SGD(other.parameters(), lr=0.5).step()
            names, _ = _names(lambda: other._packed(64))
            assert names == ["pack_multi_%d" % len(_packs(other))], names       # the moved weight's stale entries are not refreshed
        assert guard.checked >= 1 and not _recorded_sources_are_inside_their_weights()
        _set_grads([lay, other], 4)
        torch.optim.SGD(list(lay.parameters()) + list(other.parameters()), lr=0.5).step()
        _assert_current(lay, "after a step")
        _assert_current(other, "after a step")
        assert sum(1 for e in ops.packs.entries.values() if e["ref"]() is w) == len(_packs(lay))


def test_data_writes_need_increment_version():
    """an in-place write must be visible to the version counter, or be followed by increment_version."""
    from sonet_hip import ops
    with ops.precision("h3"):
        lay = _layer(64, 128)
        _assert_current(lay, "created")
        w = lay.conv.weight
        old, v = w.detach().clone(), w._version
        w.data.add_(1)
        assert w._version == v                                       # no cache can see this write
        names, _ = _names(lambda: _assert_current(lay, "stale by contract", weight=old))
        assert names == []
        torch.autograd.graph.increment_version(w)
        names, _ = _names(lambda: lay._packed(64))
        assert names == ["pack_multi_%d" % len(_packs(lay))]
        _assert_current(lay, "after increment_version")


@pytest.mark.parametrize("mode", ["h3", "x3", "bf16"])
def test_registry_off_yields_the_same_bytes(mode):
    from sonet_hip import ops
    with ops.precision(mode):
        for cin, cout in SHAPES:
            lay = _layer(cin, cout)
            on = [(_bytes(b).copy(), a) for _, b, a in _assert_current(lay, "registry on")]
            old = ops.PACK_REGISTRY
            ops.PACK_REGISTRY = False
            try:
                off = _assert_current(lay, "registry off")
                assert len(off) == len(on)
                for (ob, _a), (_, b, _a2) in zip(on, off):
                    n = R.written_size(FLAVOUR_OF[b.dtype], _a["Cin"], _a["Cout"])
                    assert np.array_equal(ob[:n], _bytes(b)[:n])
            finally:
                ops.PACK_REGISTRY = old
