"""tools/make_ce_golden.py -- fixtures of the cross-entropy operator (sonet_ce_loss_f32 / sonet_ce_grad_f32) from the LIVE reference.

Run where the reference checkout is mounted, in its own process:   python tools/make_ce_golden.py [out_dir] [--check]
(default out_dir: tests/golden/ce).  Written per case, data only:

  seg_4x50x64, seg_2x6x257      the reference's OWN models.losses.CrossEntropyLossSeg on seeded CPU scores (tests/ce_ref.py: make_inputs):
      score [B][C][N] f32, target [B][N] i64                                          the inputs;
      loss_f32 f32                                                                    the reference on the float32 scores;
      loss_f64 f64, grad_f64 [B][C][N] f64                                            the reference on float64 copies, and autograd's gradient.
  cls_16_16_8                   the test loop of modelnet/train.py:70-90, compiled and executed FROM THE REFERENCE'S FILE against a small
                                stand-in model, over three test batches of 16, 16 and 8 clouds at C = 40, with the criterion of the
                                reference's classifier Model (models/classifier.py:38, nn.CrossEntropyLoss):
      score [40][40] f32, label [40] i64, sizes [3] i64                               the inputs (batches in order);
      test_loss f32, test_accuracy f32                                                what the loop leaves in model.test_loss / test_accuracy;
      loss_f64 [3] f64, grad_f64 [40][40] f64                                         the criterion on float64 copies per batch, and its gradient.

The batch sizes are powers of two on purpose: the reference's accuracy is a float32 mean of the correct mask, exact only then.
--check regenerates into a temporary directory and compares with out_dir array by array, then holds the restatement of tests/ce_ref.py
to the live reference on fresh seeded inputs of odd sizes (FRESH).
"""
import os
import sys
import tempfile
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ce_ref as R  # noqa: E402

from oracle import ref_harness  # noqa: E402

SEG_CASES = {"seg_4x50x64": (21, 4, 50, 64), "seg_2x6x257": (22, 2, 6, 257)}           # name: seed, B, C, N
CLS_CASE = ("cls_16_16_8", 23, (16, 16, 8), 40)                                         # name, seed, batch sizes, C
FRESH = [(201, 3, 50, 33), (202, 1, 1, 5), (203, 5, 7, 1), (204, 2, 40, 300)]           # seed, B, C, N


def seg_reference(ref, score, target):
    """(loss f32, loss f64, grad f64) from the reference's own CrossEntropyLossSeg."""
    import torch
    crit = ref.losses.CrossEntropyLossSeg()
    tt = torch.from_numpy(target)
    loss32 = crit(torch.from_numpy(score), tt)
    s64 = torch.from_numpy(score.astype(np.float64)).requires_grad_(True)
    loss64 = crit(s64, tt)
    loss64.backward()
    assert loss32.dtype == torch.float32 and loss64.dtype == torch.float64
    return np.float32(loss32.item()), np.float64(loss64.item()), s64.grad.numpy().copy()


def make_seg_case(ref, seed, B, C, N):
    score, target = R.make_inputs(np.random.RandomState(seed), B, C, N)
    loss32, loss64, grad64 = seg_reference(ref, score, target)
    return dict(score=score, target=target, loss_f32=loss32, loss_f64=loss64, grad_f64=grad64)


FIRST, LAST = "batch_amount = 0", "model.test_accuracy /= batch_amount"


def reference_test_loop():
    """The code object of the reference's classification test loop (modelnet/train.py:70-90), compiled from its file."""
    path = os.path.join(ref_harness.REF_ROOT, "modelnet", "train.py")
    src = open(path).read()
    assert src.count(FIRST) == 1 and src.count(LAST) == 1, "the test loop of %s is not where it was" % path
    start, end = src.rindex("\n", 0, src.index(FIRST)) + 1, src.index(LAST) + len(LAST)
    return compile(textwrap.dedent(src[start:end]) + "\n", path, "exec")


class StandInModel:
    """What the loop asks of ``model``: two one-element float32 accumulators, ``set_input``, ``test_model`` (which leaves ``loss``) and
    ``score`` / ``input_label``.  The batch's scores travel in the loader's first slot; the criterion is the reference classifier's."""

    def __init__(self, criterion):
        import torch
        self.criterion = criterion
        self.test_loss, self.test_accuracy = torch.zeros(1), torch.zeros(1)

    def set_input(self, score, _sn, label, _node, _knn):
        self.score, self.input_label = score, label

    def test_model(self):
        self.loss = self.criterion(self.score, self.input_label)


def cls_reference(ref, score, label, sizes):
    """The reference's own test loop, executed from its file on CPU tensors, with the criterion of its classifier Model; then that
    criterion on float64 copies per batch -> (test_loss f32, test_accuracy f32, loss f64 [batches], grad f64)."""
    import inspect
    import torch
    import torch.nn as nn
    assert "self.softmax_criteria = nn.CrossEntropyLoss()" in inspect.getsource(ref.classifier.Model.__init__)
    crit = nn.CrossEntropyLoss()
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    batches = [(torch.from_numpy(score[a:b]), torch.from_numpy(label[a:b])) for a, b in zip(bounds[:-1], bounds[1:])]
    model = StandInModel(crit)
    exec(reference_test_loop(), dict(torch=torch, model=model, testloader=[(s, None, lab, None, None) for s, lab in batches]))
    loss64, grad64 = [], []
    for s, lab in batches:
        s64 = s.double().requires_grad_(True)
        l64 = crit(s64, lab)
        l64.backward()
        loss64.append(l64.item())
        grad64.append(s64.grad.numpy().copy())
    return (np.float32(model.test_loss.item()), np.float32(model.test_accuracy.item()), np.asarray(loss64, np.float64),
            np.concatenate(grad64))


def make_cls_case(ref, seed, sizes, C):
    score, label = R.make_inputs(np.random.RandomState(seed), sum(sizes), C, sigma=1.5, bump=4.0)
    tl, ta, loss64, grad64 = cls_reference(ref, score, label, sizes)
    assert 0.3 < ta < 0.95, ta                                                            # the fixture must pin something
    return dict(score=score, label=label, sizes=np.asarray(sizes, np.int64), test_loss=tl, test_accuracy=ta, loss_f64=loss64,
                grad_f64=grad64)


def check_restatement(ref):
    for seed, B, C, N in FRESH:
        score, target = R.make_inputs(np.random.RandomState(seed), B, C, N)
        loss32, loss64, grad64 = seg_reference(ref, score, target)
        mine, g = R.ce_loss(score, target), R.ce_grad(score, target)
        assert abs(mine - loss64) <= 1e-12 * max(abs(loss64), 1.0), (seed, mine, loss64)
        assert np.abs(g - grad64).max() <= 1e-12 * np.abs(grad64).max(), seed
        assert abs(mine - float(loss32)) <= 1e-5 * max(abs(float(loss32)), 1.0), (seed, mine, loss32)
    print("restatement == live reference on %d fresh inputs" % len(FRESH))


def generate(out_dir):
    ref = ref_harness.import_reference()
    assert ref.losses.__file__.startswith(ref_harness.REF_ROOT)
    os.makedirs(out_dir, exist_ok=True)
    cases = {name: make_seg_case(ref, *spec) for name, spec in SEG_CASES.items()}
    name, seed, sizes, C = CLS_CASE
    cases[name] = make_cls_case(ref, seed, sizes, C)
    for name, d in cases.items():
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **d)
        print("%-20s %7.1f KB  %s" % (name + ".npz", os.path.getsize(path) / 1024,
                                       "  ".join("%s %.6f" % (k, float(d[k])) for k in ("loss_f32", "test_loss", "test_accuracy") if k in d)))
    return list(cases)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "ce")
    if "--check" not in sys.argv:
        generate(out_dir)
        return
    with tempfile.TemporaryDirectory() as tmp:
        for name in generate(tmp):
            a, b = np.load(os.path.join(tmp, name + ".npz")), np.load(os.path.join(out_dir, name + ".npz"))
            assert sorted(a.files) == sorted(b.files), name
            for k in a.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: %s differs" % (name, k)
    print("fixtures regenerate bit-identically")
    check_restatement(ref_harness.import_reference())


if __name__ == "__main__":
    main()
