"""The weight-pack kernels against their host restatement (tests/pack_ref.py), byte for byte: the five plain entries, the three ``_strided``
entries and ``sonet_pack_multi`` driven directly with tables from ``pack_ref.pack_table``.  Every destination sits inside a larger buffer filled
with 0xA5: nothing outside the bytes a pack writes may change.  No tolerance anywhere; the lanes of a NaN weight are masked (a NaN's payload is
nobody's contract) and checked to decode to NaN."""
import numpy as np
import pytest
import torch

import pack_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 512
FILL = 0xA5
CINS = (1, 15, 16, 17, 127, 128, 129)
COUTS = (1, 31, 32, 33, 96)
PLAIN = {"f32": "sonet_pointmlp_pack_f32", "bf16": "sonet_pointmlp_bf16_pack", "x3": "sonet_pointmlp_x3_pack", "h3": "sonet_pointmlp_h3_pack",
         "h3p": "sonet_pointmlp_h3p_pack"}
STRIDED = {"bf16": "sonet_pointmlp_bf16_pack_strided", "x3": "sonet_pointmlp_x3_pack_strided", "h3": "sonet_pointmlp_h3_pack_strided"}
# which subnormal model the conversions follow: every subnormal case of the run must match one of the two, the same one throughout
_SUBNORMAL = {"kept", "flushed"}


class Matrix:
    """A matrix as the ``_strided`` entries take it: a flat f32 buffer and (offset, rows, rs, cs, Cin, padded Cout)."""

    def __init__(self, buf, off, rows, rs, cs, Cin, Cout):
        self.host = np.ascontiguousarray(buf, dtype=np.float32).reshape(-1)
        self.off, self.rows, self.rs, self.cs, self.Cin, self.Cout = off, rows, rs, cs, Cin, Cout
        assert 0 < rows <= Cout and off + (rows - 1) * rs + (Cin - 1) * cs < self.host.size          # every read stays inside the buffer
        self.dev = torch.from_numpy(self.host.copy()).to(DEV)

    @classmethod
    def plain(cls, W):
        return cls(W, 0, W.shape[0], W.shape[1], 1, W.shape[1], W.shape[0])

    @classmethod
    def transposed(cls, W, lo, Ci, Cp):
        """W[:, lo:lo + Ci]^T with zero rows up to Cp, read in place: what models/layers.py::_pack_transposed asks for."""
        assert lo + Ci <= W.shape[1] and Ci <= Cp
        return cls(W, lo, Ci, 1, W.shape[1], W.shape[0], Cp)

    def ref(self, flavour, **kw):
        return R.PACKS[flavour](self.host[self.off:], Cin=self.Cin, Cout=self.Cout, rows=self.rows, rs=self.rs, cs=self.cs, **kw)

    def nan_mask(self, flavour):
        return R.nan_lane_mask(flavour, self.host[self.off:], Cin=self.Cin, Cout=self.Cout, rows=self.rows, rs=self.rs, cs=self.cs)

    def src(self):
        return self.dev.data_ptr() + 4 * self.off

    def set(self, values):
        self.host[:] = np.asarray(values, dtype=np.float32).reshape(-1)
        self.dev.copy_(torch.from_numpy(self.host.copy()))


def _arena(flavour, Cin, Cout):
    return torch.full((GUARD + R.pack_size(flavour, Cin, Cout) + GUARD,), FILL, dtype=torch.uint8, device=DEV)


def _dst(arena):
    assert (arena.data_ptr() + GUARD) % 16 == 0
    return arena.data_ptr() + GUARD


def _single(flavour, m, strided):
    from sonet_hip import _lib, ops
    lib = _lib.load()
    arena = _arena(flavour, m.Cin, m.Cout)
    if strided:
        ops.check(getattr(lib, STRIDED[flavour])(m.src(), m.rs, m.cs, _dst(arena), m.Cin, m.Cout, m.rows, ops.stream_ptr()), STRIDED[flavour])
    else:
        assert (m.off, m.rs, m.cs, m.rows) == (0, m.Cin, 1, m.Cout)
        ops.check(getattr(lib, PLAIN[flavour])(m.src(), _dst(arena), m.Cin, m.Cout, ops.stream_ptr()), PLAIN[flavour])
    return arena


def _check(arena, flavour, m, what):
    """The whole buffer: guard bands and the bytes behind the trailer untouched, data and trailer equal to the restatement."""
    got = arena.cpu().numpy()
    n = R.written_size(flavour, m.Cin, m.Cout)
    assert n <= got.size - 2 * GUARD
    assert (got[:GUARD] == FILL).all() and (got[GUARD + n:] == FILL).all(), "%s: a byte outside the pack changed" % (what,)
    got = got[GUARD:GUARD + n]
    mask = m.nan_mask(flavour)
    if mask.any():
        T = {"bf16": 1, "x3": 3, "h3": 2, "h3p": 2}[flavour]
        data = n - (0 if flavour == "bf16" else 64)
        pieces = got[:data].view("<u2").reshape(-1, T, 64, 8)[:, 0][mask[:data:2].reshape(-1, T, 64, 8)[:, 0]]
        val = R.bf16_value(pieces) if flavour in ("bf16", "x3") else R.f16_value(pieces)
        assert pieces.size and np.isnan(val).all(), "%s: the high piece of a NaN weight is not a NaN" % (what,)
        if flavour != "bf16":
            assert (int(got[data:].view("<u4")[0]) & 0x7FFFFFFF) > 0x7F800000, "%s: trailer word 0 is no NaN pattern" % (what,)
    refs = {"kept": m.ref(flavour, flush=False), "flushed": m.ref(flavour, flush=True)}
    same = {name: bool((got == r)[~mask].all()) for name, r in refs.items()}
    if not np.array_equal(refs["kept"][~mask], refs["flushed"][~mask]):          # a subnormal case: the two models tell themselves apart
        _SUBNORMAL.intersection_update(k for k, v in same.items() if v)
        print("%s: subnormals kept %s, flushed %s -> model so far: %s" % (what, same["kept"], same["flushed"], sorted(_SUBNORMAL)))
        assert _SUBNORMAL, "%s: neither subnormal model matches every subnormal case of this run" % (what,)
    else:
        bad = np.flatnonzero((got != refs["kept"]) & ~mask)
        assert not bad.size, "%s: %d bytes differ, first at %s" % (what, bad.size, bad[:4])
    return got


# ---- every single-pack entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.WEIGHT_SETS)
@pytest.mark.parametrize("flavour", list(PLAIN))
def test_plain_pack_equals_the_restatement(flavour, kind):
    for Cin in CINS:
        for Cout in COUTS:
            m = Matrix.plain(R.weights(kind, Cout, Cin, 11))
            _check(_single(flavour, m, False), flavour, m, (flavour, kind, Cin, Cout))


def _strided_cases(kind):
    for Cin in CINS:
        for Cout in COUTS:
            # rows = Cout of a matrix stored transposed with a leading dimension of its own, packed into whole 32-row tiles
            W = R.weights(kind, Cin, Cout + 3, 12)
            yield Matrix.transposed(W, 2, Cout, (Cout + 31) // 32 * 32)
    yield Matrix.transposed(R.weights(kind, 512, 3 + 387, 13), 3, 387, 512)      # the KNN module's 387 channels behind 3 coordinates
    yield Matrix.transposed(R.weights(kind, 64, 3 + 515, 14), 3, 515, 640)       # the final PointNet's 515


@pytest.mark.parametrize("kind", R.WEIGHT_SETS)
@pytest.mark.parametrize("flavour", list(STRIDED))
def test_strided_pack_equals_the_restatement(flavour, kind):
    for m in _strided_cases(kind):
        _check(_single(flavour, m, True), flavour, m, (flavour, kind, m.Cin, m.rows, m.Cout))


def test_the_subnormal_model_is_one_and_the_same():
    """(after the subnormal cases above when the file runs in order; on its own it packs one case per flavour)"""
    for flavour in PLAIN:
        m = Matrix.plain(R.weights("subnormal", 33, 17, 11))
        _check(_single(flavour, m, False), flavour, m, (flavour, "subnormal"))
    print("pack conversions follow the subnormal model: %s" % sorted(_SUBNORMAL))
    assert len(_SUBNORMAL) >= 1


# ---- sonet_pack_multi ----------------------------------------------------------------------------------------------------------------
def _multi(specs, arenas=None):
    """specs: (flavour, Matrix) -> the arenas after one sonet_pack_multi launch over a table from pack_ref.pack_table."""
    from sonet_hip import _lib, ops
    if arenas is None:
        arenas = [_arena(f, m.Cin, m.Cout) for f, m in specs]
    tab, blocks = R.pack_table([dict(src=m.src(), dst=_dst(a), rs=m.rs, cs=m.cs, Cin=m.Cin, rows=m.rows, Cout=m.Cout, flavour=f)
                                for (f, m), a in zip(specs, arenas)])
    assert blocks == sum(-(-64 * R.tiles(f, m.Cout) * R.chunks(f, m.Cin) // 256) for f, m in specs)
    dtab = torch.from_numpy(tab).to(DEV)
    ops.check(_lib.load().sonet_pack_multi(ops.ptr(dtab), len(specs), blocks, ops.stream_ptr()), "sonet_pack_multi")
    torch.cuda.synchronize()
    return arenas


def _blocks(f, m):
    return -(-64 * R.tiles(f, m.Cout) * R.chunks(f, m.Cin) // 256)


def _fwd(kind, Cout, Cin, seed):
    return Matrix.plain(R.weights(kind, Cout, Cin, seed))


def _t(kind, Cout, Cin, lo, Ci, Cp, seed):
    return Matrix.transposed(R.weights(kind, Cout, Cin, seed), lo, Ci, Cp)


def _mixed(n):
    """n entries: the three flavours, forward and transposed sources, ordinary and edge weights in turn."""
    shapes = [(64, 128), (128, 129), (33, 17), (96, 127), (32, 16), (31, 15), (1, 1), (96, 128)]
    out = []
    for i in range(n):
        f = R.FLAVOURS[i % 3]
        Cout, Cin = shapes[i % len(shapes)]
        kind = ("ordinary", "edge", "edge_inf")[(i // 3) % 3]
        if i % 2:
            out.append((f, _t(kind, Cin + 5, Cout + 4, 3, Cout, (Cout + 31) // 32 * 32, 20 + i)))
        else:
            out.append((f, _fwd(kind, Cout, Cin, 20 + i)))
    return out


def _table_cases():
    one_wave = ("x3", _fwd("edge", 32, 16, 31))                                  # total = 64: 192 idle threads in its only workgroup
    many_a, many_b = ("h3", _fwd("ordinary", 128, 129, 32)), ("x3", _t("edge", 64, 3 + 387, 3, 387, 512, 33))
    one_blk_a, one_blk_b = ("bf16", _fwd("ordinary", 64, 32, 34)), ("x3", _fwd("ordinary", 33, 17, 35))
    return {
        "n1": [("h3", _fwd("edge", 96, 129, 30))],
        "n2": [("x3", _fwd("edge", 33, 127, 36)), ("bf16", _t("ordinary", 40, 50, 7, 35, 64, 37))],
        "one wave between two many-block entries": [many_a, one_wave, many_b],
        "two one-block entries side by side": [many_a, one_blk_a, one_blk_b, many_b],
        "last entry one block long": [many_b, many_a, one_blk_b],
        "n40": _mixed(40),
    }


@pytest.mark.parametrize("case", ["n1", "n2", "one wave between two many-block entries", "two one-block entries side by side",
                                  "last entry one block long", "n40"])
def test_pack_multi_equals_the_restatement_and_the_single_entries(case):
    specs = _table_cases()[case]
    if case == "one wave between two many-block entries":
        assert [_blocks(f, m) > 1 for f, m in specs] == [True, False, True] and 64 * R.tiles("x3", 32) * R.chunks("x3", 16) == 64
    if case == "two one-block entries side by side":
        assert [_blocks(f, m) for f, m in specs][1:3] == [1, 1]
    if case == "last entry one block long":
        assert _blocks(*specs[-1]) == 1
    if case == "n40":
        assert len(specs) == 40 and {f for f, _ in specs} == set(R.FLAVOURS)
    arenas = _multi(specs)
    for i, ((f, m), a) in enumerate(zip(specs, arenas)):
        _check(a, f, m, (case, i, f))
        assert torch.equal(a, _single(f, m, True)), (case, i, f)
    again = _multi(specs)                                                         # repeatability: fresh buffers, the same bytes
    for i, (a, b) in enumerate(zip(arenas, again)):
        assert torch.equal(a, b), (case, i)


def test_pack_multi_trailer_after_a_refresh():
    """The trailer is raised by atomicMax and lowered by nothing but the clear launch: pack max |w| = 8, refresh the same entries with
    max |w| = 0.5 -- word 0 must read 0.5.  The bf16 flavour has no trailer: its buffer's last byte is pack data and survives the clear."""
    specs = [("x3", _fwd("ordinary", 64, 128, 40)), ("bf16", _fwd("ordinary", 32, 16, 41)), ("h3", _t("ordinary", 64, 40, 4, 33, 64, 42)),
             ("x3", _fwd("ordinary", 32, 16, 43))]

    def fill(m, f, big):
        w = np.clip(m.host, -big / 2, big / 2)
        w[m.off] = -big                                                          # element (0, 0) of the packed matrix
        if f == "bf16":
            w[-1] = 1.0                                                          # W[31][15]: the pack's last two bytes, 0x3F80
        m.set(w)

    for f, m in specs:
        fill(m, f, 8.0)
    arenas = _multi(specs)
    for (f, m), a in zip(specs, arenas):
        got = _check(a, f, m, ("first", f))
        if f != "bf16":
            assert got[-64:].view("<u4")[0] == 0x41000000
    for f, m in specs:
        fill(m, f, 0.5)
    arenas = _multi(specs, arenas)
    for (f, m), a in zip(specs, arenas):
        got = _check(a, f, m, ("refreshed", f))
        if f == "bf16":
            assert got[-1] == 0x3F and got[-2] == 0x80
        else:
            t = got[-64:].view("<u4")
            assert t[0] == 0x3F000000 and not t[1:].any(), (f, hex(int(t[0])))
