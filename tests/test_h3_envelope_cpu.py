"""CPU pin of the fp16-split ("h3") contract: whatever the operand-range guard admits stays within 0.5e-5 of float64 in a float64 model
of the split (tests/h3_model.py) -- half of the project's 1e-5, the other half is left to the kernels' f32 accumulation
(tests/test_gpu_h3_envelope.py runs the kernels on the same families).  The 0.5e-5 is a condition on the guard, not a measurement:
docs/findings.md 7a holds the envelope before and after the guard was tightened to meet it."""
import numpy as np
import pytest

import h3_model as H
from conftest import golden

CAP = 0.5e-5


@pytest.mark.parametrize("flavour", H.FLAVOURS)
@pytest.mark.parametrize("K", H.KS)
def test_model_meets_half_the_bound_on_every_admitted_corner(K, flavour):
    worst, n = {}, 0
    for name, x, W in H.corner_cases(K, flavour):
        assert H.admitted(x, W, flavour), "%s (%s) is not inside the guard's region" % (name, flavour)
        e = H.rms_error(H.model(x, W, flavour), H.exact(x, W))
        fam = H.family_of(name)
        if e > worst.get(fam, (0.0, ""))[0]:
            worst[fam] = (e, name)
        n += 1
    assert n == (216 if H.ratio_limit(K) > 16.0 else 144)
    for fam, (e, name) in sorted(worst.items()):
        print("envelope %s K=%d %-18s %.3g  (%s)" % (flavour, K, fam, e, name))
    bad = {f: v for f, v in worst.items() if not v[0] <= CAP}
    assert not bad, bad


@pytest.mark.parametrize("flavour", H.FLAVOURS)
@pytest.mark.parametrize("K", H.KS)
def test_model_on_plain_operands_stays_below_1e_6(K, flavour):
    for scale in (1.0, 8.0):
        x, W = H.plain_case(K, scale=scale)
        assert H.admitted(x, W, flavour)
        assert H.rms_error(H.model(x, W, flavour), H.exact(x, W)) < 1e-6


@pytest.mark.parametrize("flavour", H.FLAVOURS)
@pytest.mark.parametrize("K", H.KS)
def test_just_outside_cases_are_rejected(K, flavour):
    sides = []
    for name, side, x, W in H.outside_cases(K, flavour):
        assert not H.admitted(x, W, flavour), name
        assert H.weights_admitted(W) == (side == "x"), name
        sides.append(side)
    assert sides == ["x", "w"]


def test_the_former_guard_admitted_corners_the_split_cannot_hold():
    """The pair the guard admitted before (any K: max |x| >= 2^-6, column ratio <= 128): the model is several times beyond 1e-5 there, and
    the present guard turns both of its sides down."""
    for K in H.KS:
        x, W = H.make_case(K, 2.0 ** -6, 2.0 ** -8, "allbut1", 128.0, 0.1)
        for flavour in H.FLAVOURS:
            assert H.rms_error(H.model(x, W, flavour), H.exact(x, W)) > 3e-5
            assert not H.admitted(x, W, flavour) and not H.weights_admitted(W)


# ---- headroom of the shipped weights and shapes ------------------------------------------------------------------------------------------
def _state_dict(kind, seed, classes=40):
    from argparse import Namespace
    import torch
    from models import networks as NW
    from sonet_hip import synth
    opt = Namespace(gpu_id=0, device=torch.device("cpu"), batch_size=2, input_pc_num=256, surface_normal=True, feature_num=1024,
                    activation="relu", normalization="batch", dropout=0.7, node_num=64, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1,
                    bn_momentum_decay_step=None, bn_momentum_decay=0.6, classes=classes)
    m = {"encoder": NW.Encoder, "segmenter": NW.Segmenter}[kind](opt)
    return {k: v.clone() for k, v in synth.fill_state_dict_(m.state_dict(), seed).items()}


def _assert_weights_inside(tag, sd, rows):
    for k, v in sd.items():
        if k.endswith("conv.weight") and not k.startswith("transformer."):
            w = v.reshape(v.shape[0], -1).numpy()
            cm = np.abs(w).max(axis=0)
            rows.append((tag, k, w.shape[1], H.column_ratio(w), H.ratio_limit(w.shape[1]), float(cm.min())))
            assert H.weights_admitted(w), rows[-1]
            assert H.column_ratio(w) <= H.ratio_limit(w.shape[1]) and cm.min() >= H.ops.H3_COLUMN_MIN, rows[-1]


# every model fixture under tests/golden: (file, the options its forward ran with where they differ from k = 3, som_k = 9, "avg")
MODEL_FIXTURES = [("classifier_b2_n256", {}), ("classifier_b8_n1024", {}), ("classifier_b2_n5000", {}), ("classifier_b2_n300_k1_center", {}),
                  ("autoencoder_b2_n1024", {}), ("autoencoder_b2_n5000", {}), ("train_step_b16_n512", {}), ("train_step_b8_n5000", {}),
                  ("segmenter_b2_n256", {"som_k_type": "center", "segmenter": True}), ("segmenter_b2_n1024", {"som_k_type": "center", "segmenter": True}),
                  ("seg_train_step_b8_n512", {"som_k_type": "center", "segmenter": True})]


@pytest.mark.parametrize("name,extra", MODEL_FIXTURES, ids=[f for f, _ in MODEL_FIXTURES])
def test_fixture_weights_and_oracle_activations_sit_inside_the_guard(name, extra):
    """A model fixture's weights are synth.fill_state_dict_(seed) for the encoder and (seed + 1) for its head: every point-wise layer passes
    the weight-side test, and every point-wise launch of the oracle's encoder forward on the fixture's clouds (the first two clouds of the
    large batches) has max |x| between the guard's thresholds.  The segmenter's own five launches have no eval-mode oracle here: their
    weights are checked, their activations are not.  The printed rows are the table in docs/findings.md 7a."""
    import torch
    from oracle import cpu_oracle as O
    fx = golden(name)
    seed = int(fx["seed"])
    rows = []
    sd = _state_dict("encoder", seed)
    _assert_weights_inside("encoder", sd, rows)
    if extra.get("segmenter"):
        _assert_weights_inside("segmenter", _state_dict("segmenter", seed + 1, classes=50), rows)
    for r in rows:
        print("headroom %s seed %d %-9s %-40s K=%-4d ratio %.2f (limit %.2f)  smallest column %.3f" % ((name, seed) + r))
    k = int(fx["k"]) if "k" in fx.files else 3
    som_k = int(fx["som_k"]) if "som_k" in fx.files else 9
    kind = str(fx["som_k_type"]) if "som_k_type" in fx.files else extra.get("som_k_type", "avg")
    seen, orig = [], O._eq_layer

    def rec(sd_, prefix, x, *a, **kw):
        seen.append((prefix, x.shape[1], float(x.abs().max())))
        return orig(sd_, prefix, x, *a, **kw)

    O._eq_layer = rec
    try:
        O.encoder_forward(sd, *(torch.from_numpy(np.ascontiguousarray(fx[key][:2])) for key in ("pc", "sn", "node", "node_knn_I")),
                          k=k, som_k=som_k, som_k_type=kind, use_ref_index_max=False)
    finally:
        O._eq_layer = orig
    assert len(seen) == 8
    for prefix, K, mx in seen:
        print("headroom %s launch %-28s K=%-4d max |x| = %.3g (limits %g .. %g)" % (name, prefix, K, mx, H.X_LOW, H.X_HIGH))
        assert H.X_LOW <= mx <= H.X_HIGH, (prefix, mx)


def test_benchmark_weights_sit_inside_the_guard():
    """The seeds the other tests and the benchmark fill their models with."""
    rows = []
    for seed in (1, 2, 11, 12, 21, 22):
        _assert_weights_inside("encoder %d" % seed, _state_dict("encoder", seed), rows)
        _assert_weights_inside("segmenter %d" % seed, _state_dict("segmenter", seed, classes=50), rows)
