"""The float64 twin's bf16-mirroring mode (tests/f64_classifier.py, ``rounding="bf16"``), on the CPU: the wiring the GPU gate
tests/test_gpu_bf16_forced_routing.py relies on.  Every forward site holds bf16 values, every backward site rounded a gradient that arrived,
the sites are the documented ones, and the mirrored step still lands near the reference's float64 gradients (``grad64/``)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_oracle_golden import _reference_keyed_state_dict


@pytest.fixture(scope="module")
def runs():
    import f64_classifier as F64
    g = golden("train_step_b16_n512")
    seed = int(g["seed"])
    enc = F64.leaf_params(_reference_keyed_state_dict("encoder", seed), "cpu")
    cls = F64.leaf_params(_reference_keyed_state_dict("classifier", seed + 1), "cpu")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))                       # noqa: E731
    inputs = dict(pc=T(g["pc"]).double(), sn=T(g["sn"]).double(), node=T(g["node"]).double())
    out = {}
    out["bf16"] = F64.train_step(enc, cls, T(g["label"]), T(g["node_knn_I"]), rounding="bf16", **inputs)
    out["f32_dgrad"] = F64.train_step(enc, cls, T(g["label"]), T(g["node_knn_I"]), rounding="bf16", pooled_dgrad="f32", **inputs)
    out["plain"] = p = F64.train_step(enc, cls, T(g["label"]), T(g["node_knn_I"]), **inputs)
    out["forced"] = F64.train_step(enc, cls, T(g["label"]), T(g["node_knn_I"]), rounding="bf16", route=p["route"], masks=p["masks"], **inputs)
    return g, out


def test_bf16_twin_sites_hold_bf16_values(runs):
    import f64_classifier as F64
    _, out = runs
    r = out["bf16"]
    assert sorted(r["sites"]) == sorted(F64.BF16_FORWARD_SITES + F64.BF16_BACKWARD_SITES)
    assert sorted(out["f32_dgrad"]["sites"]) == sorted(set(F64.BF16_FORWARD_SITES + F64.BF16_BACKWARD_SITES) - {"first_pointnet.layers.3.g_out"})
    assert out["plain"]["sites"] == {}
    # the pooled layer's input-gradient path changes its input gradient only, never its forward or its own weight gradient
    k = "first_pointnet.layers.3.conv.weight"
    assert torch.equal(out["f32_dgrad"]["loss"], r["loss"]) and torch.equal(out["f32_dgrad"]["grads"][k], r["grads"][k])
    assert not torch.equal(out["f32_dgrad"]["grads"]["first_pointnet.layers.2.conv.weight"], r["grads"]["first_pointnet.layers.2.conv.weight"])
    for name, t in r["sites"].items():
        assert t.dtype == torch.float64, name
        assert torch.equal(t, t.to(torch.bfloat16).double()), name
        assert t.abs().sum() > 0, name                     # (a site that saw nothing -- a gradient that never arrived -- is not wired)
    # the forward sites are the values the step computed with: the twin's feature is the pooled value
    assert torch.equal(r["feature"], r["sites"]["pool3"])
    # weight gradients stay unrounded (f32 out in the step)
    for k in ("first_pointnet.layers.3.conv.weight", "knnlayer.layers.0.conv.weight"):
        assert not torch.equal(r["grads"][k], r["grads"][k].to(torch.bfloat16).double()), k


def test_bf16_twin_rounding_is_visible_and_small(runs):
    """With the plain run's routing and ReLU patterns forced, the mirrored step differs from the plain one by bf16 rounding alone (several
    1e-2 of a gradient, measured 3e-2 .. 0.12: the heads amplify the features' rounding) -- and the batch statistics it reports are those of its rounded raw outputs."""
    _, out = runs
    r, p = out["forced"], out["plain"]
    assert set(r["bn"]) == set(p["bn"]) and len(r["bn"]) == 8
    for prefix, (mean, var, n) in r["bn"].items():
        if prefix.startswith(("first", "knn", "final")):
            raw = r["sites"][prefix + ".raw"]
            dims = [0] + list(range(2, raw.dim()))
            assert n == raw.numel() // raw.shape[1]
            assert torch.allclose(mean, raw.mean(dim=dims), rtol=0, atol=1e-12) and torch.allclose(var, raw.var(dim=dims, unbiased=False), rtol=1e-12)
    diffs = [float((r["grads"][k] - p["grads"][k]).norm() / p["grads"][k].norm()) for k in p["grads"] if float(p["grads"][k].norm()) > 1e-6]
    assert 1e-3 < max(diffs) < 0.3, max(diffs)


def test_bf16_twin_free_run_stays_near_the_reference_float64_gradients(runs):
    """Free routing (its own pools and ReLUs on bf16 values): a sanity check, the cosine floors of the bf16 step's own gate
    (tests/test_gpu_bf16.py::test_classifier_training_step_bf16: 0.80 at this fixture)."""
    g, out = runs
    r = out["bf16"]
    cos = {}
    for k in [k[7:] for k in g.files if k.startswith("grad64/") and not k.startswith("grad64/cls.")]:
        truth = g["grad64/" + k].astype(np.float64)
        if np.sqrt(np.mean(truth ** 2)) < 1e-5 or not k.endswith("conv.weight"):
            continue
        f = r["grads"][k].flatten()
        mine = f[::max(1, f.numel() // 16384)].numpy()
        cos[k] = float(np.dot(mine, truth) / (np.linalg.norm(mine) * np.linalg.norm(truth)))
    assert len(cos) >= 5 and min(cos.values()) > 0.80, cos
