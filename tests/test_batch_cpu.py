"""Batch assembler (sonet_assemble_batch_f32, sonet_hip.batch) -- host side, no GPU: the numpy Philox against the known-answer
vectors, the documented draw mapping, the C entry's argument checks, DeviceClouds.from_modelnet on a synthetic directory, the
fixtures against the float64 restatement, and (reference mounted) the fixture generator's self-check."""
import ctypes
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest

from conftest import ROOT, golden

CASES = ("modelnet_train_all_flags", "modelnet_train_no_flags", "modelnet_test", "shrec_train_4x4_k1", "shapenet_train_ragged",
         "modelnet_train_bench_shape")


def test_philox_known_answers():
    from sonet_hip.batch import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in philox4x32_10(ctr, key)) == want
    # vectorised over counters = one at a time
    ctr = np.array([k[0] for k in kat[:2]], dtype=np.uint32)
    assert (philox4x32_10(ctr, (0, 0))[0] == philox4x32_10(ctr[0], (0, 0))).all()


def _block(seed, step, b, stream, e):
    from sonet_hip.batch import philox4x32_10
    return [int(v) for v in philox4x32_10((step & 0xFFFFFFFF, b, stream, e), (seed & 0xFFFFFFFF, seed >> 32))]


def _normals(w):
    import math
    ra, rb = math.sqrt(-2 * math.log((w[0] + 1) * 2.0 ** -32)), math.sqrt(-2 * math.log((w[2] + 1) * 2.0 ** -32))
    ta, tb = 2 * math.pi * (w[1] * 2.0 ** -32), 2 * math.pi * (w[3] * 2.0 ** -32)
    return [ra * math.cos(ta), ra * math.sin(ta), rb * math.cos(tb)]


def test_draw_mapping_as_documented():
    """slot_draws against a scalar reading of include/sonet_hip.h: counter (step, b, stream, element), key = seed."""
    from sonet_hip import batch as BA
    seed, step, b, n_s, N, M = (5 << 32) | 77, 2 ** 32 + 9, 3, 37, 20, 4
    chosen, d = BA.slot_draws(seed, step, b, n_s, N, M)
    keys = [_block(seed, step, b, 0, i >> 2)[i & 3] for i in range(n_s)]
    assert chosen.tolist() == sorted(sorted(range(n_s), key=lambda i: (keys[i], i))[:N])
    w0, w2 = _block(seed, step, b, 2, 0), _block(seed, step, b, 2, 2)
    assert d[0] == w0[0] * 2.0 ** -32
    assert d[4] == 0.8 + (1.2 - 0.8) * (w0[1] * 2.0 ** -32)
    assert d[5:8].tolist() == [-0.1 + 0.2 * (w2[c] * 2.0 ** -32) for c in range(3)]
    np.testing.assert_allclose(d[1:4], _normals(_block(seed, step, b, 2, 1)), rtol=1e-14, atol=1e-15)
    j, m = 7, 2
    np.testing.assert_allclose(d[8 + 3 * j:8 + 3 * j + 3], _normals(_block(seed, step, b, 3, j)), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(d[8 + 3 * N + 3 * j:8 + 3 * N + 3 * j + 3], _normals(_block(seed, step, b, 4, j)), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(d[8 + 6 * N + 3 * m:8 + 6 * N + 3 * m + 3], _normals(_block(seed, step, b, 5, m)), rtol=1e-14, atol=1e-15)
    # shapenet: N >= n_s takes every point in order, then (w * n_s) >> 32 from stream 1; N == n_s draws nothing
    c2, _ = BA.slot_draws(seed, step, b, 10, 15, M, "shapenet")
    ext = [(_block(seed, step, b, 1, t >> 2)[t & 3] * 10) >> 32 for t in range(5)]
    assert c2.tolist() == list(range(10)) + ext
    assert BA.slot_draws(seed, step, b, 15, 15, M, "shapenet")[0].tolist() == list(range(15))
    assert len(set(BA.slot_draws(seed, step, b, 16, 15, M, "shapenet")[0].tolist())) == 15
    # a slot's draws depend on (seed, step, b) only; other steps / slots / seeds differ
    assert np.array_equal(BA.slot_draws(seed, step, b, n_s, N, M)[1], d)
    for other in ((seed, step + 1, b), (seed, step, b + 1), (seed + 1, step, b)):
        assert not np.array_equal(BA.slot_draws(*other, n_s, N, M)[1], d)


def test_c_abi_batch_argument_validation_without_gpu():
    """Host-visible bad arguments give a status and message before any launch (no device needed)."""
    from sonet_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.sonet_assemble_batch_f32

    def call(src=p, P=10, S=1, B=1, N=4, M=8, K=3, flags=2):
        return f(src, P, p, S, p, p, B, N, M, K, flags, 1, 0, None, None, None, p, p, p, p, p, None, None)

    assert call(src=None) == 1 and "NULL" in _lib.last_error()
    assert call(K=17, M=64) == 2 and "16" in _lib.last_error()
    assert call(K=9, M=8) == 1 and "K=9" in _lib.last_error()
    assert call(K=0) == 1
    assert call(N=0) == 1 and "N=0" in _lib.last_error()
    assert call(B=0) == 1 and call(P=0) == 1 and call(S=0) == 1
    assert call(flags=64) == 1 and "flag" in _lib.last_error()
    assert call(flags=1 | 2 | 4) == 1 and "shapenet" in _lib.last_error()


def test_from_modelnet_reads_the_reference_layout(tmp_path):
    from sonet_hip.batch import DeviceClouds
    g = np.random.RandomState(0)
    names = ["airplane", "bed", "chair"]
    (tmp_path / "modelnet40_shape_names.txt").write_text("\n".join(names) + "\n")
    lines = ["chair_0003", "airplane_0001", "chair_0011"]
    (tmp_path / "modelnet40_train.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "modelnet40_test.txt").write_text("bed_0002\n")
    data, nodes = {}, {}
    for name in lines + ["bed_0002"]:
        folder = name[:-5]
        for sub in (folder, os.path.join("4x4_som_nodes", folder)):
            os.makedirs(tmp_path / sub, exist_ok=True)
        data[name] = g.normal(size=(50, 6)).astype(np.float32)
        nodes[name] = g.normal(size=(16, 3)).astype(np.float32)
        np.save(tmp_path / folder / (name + ".npy"), data[name])
        np.save(tmp_path / "4x4_som_nodes" / folder / (name + ".npy"), nodes[name])
    opt = Namespace(classes=40, node_num=16)
    c = DeviceClouds.from_modelnet(str(tmp_path), "train", opt, device="cpu")
    assert len(c) == 3 and c.node_num == 16
    assert c.labels.tolist() == [2, 0, 2]
    assert c.offsets.tolist() == [0, 50, 100, 150]
    want = np.concatenate([data[n] for n in lines], 0).T
    assert np.array_equal(c.src.numpy(), want)
    assert np.array_equal(c.nodes.numpy(), np.stack([nodes[n] for n in lines]))
    t = DeviceClouds.from_modelnet(str(tmp_path), "test", opt, device="cpu")
    assert t.labels.tolist() == [1] and np.array_equal(t.src.numpy(), data["bed_0002"].T)
    with pytest.raises(Exception, match="mode"):
        DeviceClouds.from_modelnet(str(tmp_path), "val", opt, device="cpu")


def test_device_clouds_ragged_needs_nodes():
    from sonet_hip.batch import DeviceClouds
    from sonet_hip._lib import SonetHipError
    pts = [np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)]
    with pytest.raises(SonetHipError, match="ragged"):
        DeviceClouds(pts, pts, [0, 1], device="cpu")
    c = DeviceClouds(pts, pts, [0, 1], nodes=np.zeros((2, 4, 3), np.float32), seg=[np.arange(5), np.arange(7)], device="cpu")
    assert c.sizes.tolist() == [5, 7] and c.seg.tolist() == list(range(5)) + list(range(7))


@pytest.mark.parametrize("case", CASES)
def test_fixture_equals_restatement(case):
    """The recorded draws fed to the float64 restatement give the reference loader's outputs bit for bit."""
    from sonet_hip import batch as BA
    g = golden("batch/" + case)
    off = g["offsets"]
    recipe, train = str(g["recipe"]), str(g["mode"]) == "train"
    fl = int(g["flags"])
    kw = dict(rot_horizontal=bool(fl & 4), rot_perturbation=bool(fl & 8), translation_perturbation=bool(fl & 16))
    for b, s in enumerate(g["idx"]):
        data = g["src"][:, off[s]:off[s + 1]].T
        pc, sn, node = BA.augment_np(data, g["nodes_src"][s], g["replay_idx"][b], g["replay_draws"][b], train, recipe, **kw)
        for got, want in ((pc, g["pc"][b]), (sn, g["sn"][b]), (node, g["node"][b])):
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert all(os.path.getsize(os.path.join(ROOT, "tests", "golden", "batch", c + ".npz")) < 700 * 1024 for c in CASES)


@pytest.mark.skipif(not os.path.isdir("/root/reference/data"), reason="reference checkout not mounted")
def test_golden_tool_self_check_and_regeneration():
    """tools/make_batch_golden.py runs the reference loaders, checks its recorded draws bit for bit and regenerates the fixtures."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_batch_golden.py"), "--check"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    assert b"bit-identically" in r.stdout
