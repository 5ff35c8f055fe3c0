"""tools/make_upconv_golden.py -- fixtures of the fused up-convolution (sonet_upconv3x3_f32, opt.decoder_fused) from the LIVE reference.

Run where the reference checkout is mounted, in its own process:   python tools/make_upconv_golden.py [out_dir] [--check]
(default out_dir: tests/golden/upconv).

The reference's OWN models.layers.UpConv and models.networks.DecoderConv (through oracle.ref_harness.import_reference, unmodified) run
in eval mode on seeded CPU inputs with the seeded parameters of sonet_hip.synth.fill_state_dict_ (BatchNorm statistics included).
Written per case (data only):
  upconv_16x32_3x5    UpConv(16 -> 32, 'relu', 'batch'), B = 3, 3 x 5:   x, the six parameter / buffer tensors under their state_dict
                      keys (dots as "__"), y;
  upconv_40x32_1x1    UpConv(40 -> 32, no activation, no normalization), B = 5, 1 x 1 (a K tail, three taps of four in the padding):
                      x, weight and bias, y;
  decoderconv_f64     DecoderConv at feature_num 64 ('relu', 'batch'), B = 2: feature, seed -- the parameters are
                      fill_state_dict_(state_dict, seed), 62 k floats that would not fit the size limit of a fixture --, state_dict keys,
                      pc4 [2][3][16][16], pc5 [2][3][32][32], pc6 [2][3][64][64].

The two UpConv cases keep their operands on a dyadic grid -- x in multiples of 2^-6, the 3x3 weights in multiples of 2^-12 -- so that every
product (22 bits) and every partial sum of the at most 360 products (below 2^6 in magnitude, quantum 2^-18) is exact in float32 whatever
order the reference's convolution adds them in: its output then differs from float64 only through the handful of roundings of the bias
add and the BatchNorm (a few 2^-24), and the float64 restatement of tests/upconv_ref.py can be held to it at 1e-6.  With full-precision
operands the reference's own f32 accumulation sits at 0.9 - 1.4e-6 of the restatement in the BatchNorm case (measured over six seeds),
i.e. on the bound itself.  The bias and the BatchNorm tensors are not rounded.

--check regenerates into a temporary directory and compares with out_dir array by array, then prints for every case the gap between the
reference's f32 outputs and the float64 restatement (tests/upconv_ref.py) in the project's metric.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

# name: (Cin, Cout, activation, normalization, B, H, W, seed)
UPCONV_CASES = {
    "upconv_16x32_3x5": (16, 32, "relu", "batch", 3, 3, 5, 701),
    "upconv_40x32_1x1": (40, 32, None, None, 5, 1, 1, 702),
}
DECODER_CASE = ("decoderconv_f64", 64, 2, 703)               # name, feature_num, B, seed
CASES = tuple(UPCONV_CASES) + (DECODER_CASE[0],)
MAX_BYTES = 200 * 1024


def _synth():
    """sonet_hip/synth.py by file (torch only): so-net_amd/ must stay off sys.path, its ``models`` / ``util`` would shadow the reference's."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_sonet_synth", os.path.join(ROOT, "so-net_amd", "sonet_hip", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _key(k):
    return k.replace(".", "__")


def make_upconv(ref, Cin, Cout, act, norm, B, H, W, seed):
    import torch
    synth = _synth()
    m = ref.layers.UpConv(Cin, Cout, activation=act, normalization=norm)
    sd = synth.fill_state_dict_(m.state_dict(), seed)
    sd["conv.conv.weight"].copy_(torch.round(sd["conv.conv.weight"] * 4096.0) / 4096.0)          # (state_dict tensors alias the parameters)
    m.eval()
    x = torch.round(torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(seed)) * 64.0) / 64.0
    with torch.no_grad():
        y = m(x)
    d = dict(x=x.numpy(), y=y.numpy(), keys=np.array(sorted(m.state_dict().keys())))
    for k, v in m.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            d[_key(k)] = v.numpy().copy()
    assert tuple(y.shape) == (B, Cout, 2 * H, 2 * W) and y.dtype == torch.float32
    return d


def make_decoder(ref, F, B, seed):
    import torch
    synth = _synth()
    opt = ref_harness.make_opt(feature_num=F, output_conv_pc_num=4096, output_fc_pc_num=0)
    m = ref.networks.DecoderConv(opt)
    synth.fill_state_dict_(m.state_dict(), seed)
    m.eval()
    feature = torch.randn(B, F, generator=torch.Generator().manual_seed(seed)).abs()      # an encoder feature is a max over ReLU outputs
    with torch.no_grad():
        pc6 = m(feature)
    assert tuple(pc6.shape) == (B, 3, 64, 64) and tuple(m.pc4.shape) == (B, 3, 16, 16) and tuple(m.pc5.shape) == (B, 3, 32, 32)
    return dict(feature=feature.numpy(), seed=np.int64(seed), feature_num=np.int64(F), keys=np.array(sorted(m.state_dict().keys())),
                pc4=m.pc4.numpy(), pc5=m.pc5.numpy(), pc6=pc6.numpy())


def generate(out_dir):
    ref = ref_harness.import_reference()
    assert ref.layers.__file__.startswith(ref_harness.REF_ROOT)
    os.makedirs(out_dir, exist_ok=True)
    made = {name: make_upconv(ref, *spec) for name, spec in UPCONV_CASES.items()}
    made[DECODER_CASE[0]] = make_decoder(ref, *DECODER_CASE[1:])
    for name, d in made.items():
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (name, size)
        print("%-24s %7.1f KB" % (name + ".npz", size / 1024))


def report(out_dir):
    import upconv_ref as R
    for name, (Cin, Cout, act, norm, B, H, W, seed) in UPCONV_CASES.items():
        g = np.load(os.path.join(out_dir, name + ".npz"))
        scale, shift = R.eval_affine(g, Cout)
        got = R.reference(g["x"], g["conv__conv__weight"], scale, shift, act == "relu")
        print("%s: reference f32 output vs float64 restatement %.3g" % (name, R.rms_error(g["y"], got)))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "upconv")
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
    report(out_dir)


if __name__ == "__main__":
    main()
