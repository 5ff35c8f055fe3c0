"""tools/make_upconv_train_golden.py -- fixtures of the up-convolution's TRAINING step (opt.decoder_fused_train) from the LIVE reference.

Run where the reference checkout is mounted, in its own process:   python tools/make_upconv_train_golden.py [out_dir] [--check]
(default out_dir: tests/golden/upconv_train).

The reference's OWN models.layers.UpConv (through oracle.ref_harness.import_reference, unmodified) runs ONE training step in train mode
and float64 on the CPU: seeded parameters (sonet_hip.synth.fill_state_dict_, BatchNorm statistics included), a seeded input and a seeded
cotangent at gradient scale.  Written per case (data only, float64 unless noted):
  upconv_16x32_3x5    UpConv(16 -> 32, 'relu', 'batch'), B = 3, 3 x 5:  x, the parameters and buffers BEFORE the step under their state_dict
                      keys (dots as "__"), the cotangent g, y, dx, dW, dbias, dgamma, dbeta, running_mean / running_var AFTER the step;
  upconv_40x32_1x1    UpConv(40 -> 32, no activation, no normalization), B = 5, 1 x 1:  x, weight and bias, g, y, dx, dW, dbias.
x, g and the parameters are float32 values (stored as float32): the GPU layer is fed exactly what the reference was.

--check regenerates into a temporary directory and compares with out_dir array by array.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
from make_upconv_golden import MAX_BYTES, _key, _synth  # noqa: E402

# name: (Cin, Cout, activation, normalization, B, H, W, seed)
CASES = {
    "upconv_16x32_3x5": (16, 32, "relu", "batch", 3, 3, 5, 711),
    "upconv_40x32_1x1": (40, 32, None, None, 5, 1, 1, 712),
}


def make_case(ref, Cin, Cout, act, norm, B, H, W, seed):
    import torch
    synth = _synth()
    m = ref.layers.UpConv(Cin, Cout, activation=act, normalization=norm)
    synth.fill_state_dict_(m.state_dict(), seed)
    d = dict(keys=np.array(sorted(m.state_dict().keys())))
    for k, v in m.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            d[_key(k)] = v.numpy().copy()                                  # float32, before the step
    gen = torch.Generator().manual_seed(seed)
    x32 = torch.randn(B, Cin, H, W, generator=gen)
    g32 = torch.randn(B, Cout, 2 * H, 2 * W, generator=gen) * 1e-3          # a Chamfer gradient behind the point heads: order 1e-3
    m.double().train()
    x = x32.double().requires_grad_(True)
    y = m(x)
    y.backward(g32.double())
    conv = m.conv.conv
    d.update(x=x32.numpy(), g=g32.numpy(), y=y.detach().numpy(), dx=x.grad.numpy(), dW=conv.weight.grad.numpy(), dbias=conv.bias.grad.numpy())
    if norm == "batch":
        bn = m.conv.norm
        d.update(dgamma=bn.weight.grad.numpy(), dbeta=bn.bias.grad.numpy(), running_mean_after=bn.running_mean.numpy().copy(),
                 running_var_after=bn.running_var.numpy().copy())
    assert tuple(y.shape) == (B, Cout, 2 * H, 2 * W) and y.dtype == torch.float64 and x.grad.dtype == torch.float64
    return d


def generate(out_dir):
    ref = ref_harness.import_reference()
    assert ref.layers.__file__.startswith(ref_harness.REF_ROOT)
    os.makedirs(out_dir, exist_ok=True)
    for name, spec in CASES.items():
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **make_case(ref, *spec))
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (name, size)
        print("%-24s %7.1f KB" % (name + ".npz", size / 1024))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "upconv_train")
    if "--check" not in sys.argv:
        generate(out_dir)
        return
    with tempfile.TemporaryDirectory() as tmp:
        generate(tmp)
        for name in CASES:
            a, b = np.load(os.path.join(tmp, name + ".npz")), np.load(os.path.join(out_dir, name + ".npz"))
            assert sorted(a.files) == sorted(b.files), name
            for k in a.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: %s differs" % (name, k)
    print("fixtures regenerate bit-identically")


if __name__ == "__main__":
    main()
