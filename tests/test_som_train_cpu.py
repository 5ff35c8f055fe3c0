"""SOM trainer (BatchSOM.optimize / sonet_som_train_f32) -- host side, no GPU: the potential-field initialiser restated in
util/som.py against the live reference and the golden fixtures, the schedule tables against the reference's formulas, the
C entry's argument checks, and the fixture generator's reproducibility."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden

REF_PF = "/root/reference/util/potential_field.py"
GOLDEN_SOM = ("som/som_optimize_8x8_n5000", "som/som_optimize_4x4_n1024", "som/som_optimize_8x8_n40")


def _ref_potential_field():
    spec = importlib.util.spec_from_file_location("_ref_potential_field", REF_PF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.skipif(not os.path.isfile(REF_PF), reason="reference checkout not mounted")
@pytest.mark.parametrize("side", [4, 8, 11])
def test_potential_field_equals_live_reference(side):
    from util import som
    M = side * side
    state = np.random.get_state()
    mine = som.potential_field_nodes(M, 3)
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state, after)), "the restatement touched numpy's global generator"
    pf = _ref_potential_field().PotentialField(M, 3)
    pf.optimize()
    np.testing.assert_array_equal(mine, pf.node)


def test_node_init_value_equals_golden():
    from util import som
    state = np.random.get_state()
    for name in GOLDEN_SOM:
        g = golden(name)
        s = som.BatchSOM(int(g["rows"]), int(g["cols"]), 3, 0, 2)
        assert s._node_init_value is None                              # lazy
        np.testing.assert_array_equal(s.node_init_value.numpy(), g["node_init"])
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state, after))


def test_potential_field_non_square_layout():
    """The reference reorders on a sqrt(M) grid only; other M use the instance's rows x cols."""
    from util import som
    node = som.potential_field_nodes(24, 3, 4, 6)
    assert node.shape == (24, 3) and np.isfinite(node).all()
    grid = node.reshape(4, 6, 3)
    assert (np.diff(grid[:, :, 1], axis=1) >= 0).all()


def _ref_schedule(max_iteration, learning_rate, sigma):
    """util/som.py:355-366, literally."""
    out = []
    for it in range(int(max_iteration / 3)):
        out.append((learning_rate, sigma))
    for it in range(max_iteration):
        out.append((learning_rate / (1 + 2 * it / max_iteration), sigma / (1 + 2 * it / max_iteration)))
    return out


@pytest.mark.parametrize("attrs", [None, dict(max_iteration=9, learning_rate=0.3, sigma=0.55)])
def test_schedule_tables_equal_reference_formulas(attrs):
    from util import som
    s = som.BatchSOM(8, 8, 3, 0, 2)
    if attrs:
        for k, v in attrs.items():
            setattr(s, k, v)
    sched = _ref_schedule(s.max_iteration, s.learning_rate, s.sigma)
    lrs, sigmas = s.train_schedule()
    assert list(zip(lrs, sigmas)) == sched
    lr, w, node0 = s.train_tables("cpu")
    assert lr.dtype == torch.float32 and w.dtype == torch.float32 and tuple(w.shape) == (len(sched), 64, 64)
    assert torch.equal(node0, s.node_init_value)
    w0 = s.init_weighting_matrix
    for t, (l, sg) in enumerate(sched):
        assert lr[t].item() == np.float32(l)
        scale = 1.0 / ((sg / s.sigma) ** 2)                                         # util/som.py:229-232
        ref = torch.exp(torch.log(w0) * scale).reshape(64, 64)
        assert torch.equal(w[t], ref), t
    assert s.train_tables("cpu")[1] is w                                            # cached
    s.max_iteration = 3
    assert s.train_tables("cpu")[1].shape[0] == 1 + 3                                 # read at call time


def test_c_entry_rejects_bad_arguments_without_gpu():
    from sonet_hip import _lib
    lib = _lib.load()
    f = lib.sonet_som_train_f32
    p = ctypes.c_void_p(256)                          # never dereferenced: every call below fails its argument check first
    bad = [
        (None, p, 0, p, p, 1, 1, 16, 64, p),          # x NULL
        (p, None, 0, p, p, 1, 1, 16, 64, p),          # node0 NULL
        (p, p, 0, None, p, 1, 1, 16, 64, p),          # w NULL with T > 0
        (p, p, 0, p, None, 1, 1, 16, 64, p),          # lr NULL with T > 0
        (p, p, 0, p, p, 1, 1, 16, 64, None),          # out NULL
        (p, p, 0, p, p, 1, 0, 16, 64, p),             # B < 1
        (p, p, 0, p, p, 1, 1, 0, 64, p),              # N < 1
        (p, p, 0, p, p, 1, 1, 16, 0, p),              # M < 1
        (p, p, 0, p, p, -1, 1, 16, 64, p),            # T < 0
        (p, p, 0, p, p, 1, 1, 16, 1025, p),           # M above the limit
        (p, p, 0, p, p, 1, 1, (1 << 28) + 1, 64, p),  # N above the limit
    ]
    for args in bad:
        assert f(*args, None) == 1, args                # SONET_ERR_INVALID_ARG
        assert b"sonet_som_train_f32" in lib.sonet_last_error()
    assert lib.sonet_abi_version() == 1


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="reference checkout not mounted")
def test_make_som_golden_regenerates_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_som_golden.py"), str(tmp_path)])
    for name in GOLDEN_SOM:
        new = np.load(os.path.join(str(tmp_path), os.path.basename(name) + ".npz"))
        old = golden(name)
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), (name, k)
