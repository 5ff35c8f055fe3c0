"""tools/make_chamfer_golden.py -- fixtures of the fused Chamfer loss (sonet_chamfer_loss_f32 / sonet_chamfer_grad_f32) from the LIVE
reference.

Run where the reference checkout is mounted, in its own process:   python tools/make_chamfer_golden.py [out_dir] [--check]
(default out_dir: tests/golden/chamfer).

For every case the reference's OWN models.losses.ChamferLoss (through oracle.ref_harness.import_reference(with_faiss_shim=True): its
gathers, robust_norm and means unmodified, the exact flat-L2 search of the oracle in place of faiss) and autograd run on seeded CPU
inputs (tests/chamfer_ref.py).  Written per case (data only):
  pred [B][3][M] f32, gt [B][3][N] f32                                          the inputs;
  nn_pg [B][M] i32, nn_gp [B][N] i32                                             the indices its two searches returned;
  elem_fwd [B][M] f32, elem_bwd [B][N] f32                                       the reference's robust_norm on its own selections;
  forward_loss, backward_loss f32, forward_loss_array, backward_loss_array, loss_array [B] f32      the five attributes;
  grad_predicted [B][3][M] f32                                                   d (forward_loss + backward_loss) / d pred.

--check regenerates into a temporary directory and compares with out_dir array by array, then prints for every case the worst gap
between the reference's f32 gradient and the float64 restatement in units of 2^-24 * sum|term|, and the worst gap between the
reference's elements and the restatement's in float32 ulps.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chamfer_ref as R  # noqa: E402

from oracle import ref_harness  # noqa: E402

# name: (maker, B, M, N, seed)
CASES = {
    "continuous_b3_m257_n1000": (R.continuous, 3, 257, 1000, 501),
    "lattice_ties": (lambda B, M, N, seed: R.lattice(B, M, N), 2, 257, 1025, 0),
    "coincident_half": (R.coincident, 2, 256, 600, 503),
}
assert tuple(CASES) == R.GOLDEN_CASES


def make_case(ref, name, maker, B, M, N, seed):
    import torch
    pred, gt = maker(B, M, N, seed)
    crit = ref.losses.ChamferLoss(ref_harness.make_opt())                         # (device cpu: its .to(device) calls are no-ops)
    found = []
    search_nn = crit.search_nn

    def recording_search(index, query, k):
        D, I = search_nn(index, query, k)
        found.append(I[:, 0].numpy().astype(np.int32))
        return D, I

    crit.search_nn = recording_search
    p = torch.from_numpy(pred).requires_grad_(True)
    g = torch.from_numpy(gt)
    loss = crit(p, g)
    loss.backward()
    nn_pg, nn_gp = np.stack(found[0::2]), np.stack(found[1::2])                  # per sample: predicted -> gt, then gt -> predicted
    assert nn_pg.shape == (B, M) and nn_gp.shape == (B, N)
    with torch.no_grad():                                                        # the reference's robust_norm on its own selections
        sel_gt = torch.stack([g[b].index_select(1, torch.from_numpy(nn_pg[b].astype(np.int64))) for b in range(B)]).unsqueeze(1)
        sel_pr = torch.stack([p[b].index_select(1, torch.from_numpy(nn_gp[b].astype(np.int64))) for b in range(B)]).unsqueeze(1)
        elem_fwd = ref.losses.robust_norm(sel_gt - p.unsqueeze(1))[:, 0].numpy()
        elem_bwd = ref.losses.robust_norm(sel_pr - g.unsqueeze(1))[:, 0].numpy()
    d = dict(pred=pred, gt=gt, nn_pg=nn_pg, nn_gp=nn_gp, elem_fwd=elem_fwd, elem_bwd=elem_bwd,
             forward_loss=np.float32(crit.forward_loss.item()), backward_loss=np.float32(crit.backward_loss.item()),
             forward_loss_array=crit.forward_loss_array.detach().numpy(), backward_loss_array=crit.backward_loss_array.detach().numpy(),
             loss_array=crit.loss_array.detach().numpy(), grad_predicted=p.grad.numpy())
    for k in ("elem_fwd", "elem_bwd", "forward_loss_array", "backward_loss_array", "loss_array", "grad_predicted"):
        assert d[k].dtype == np.float32, k
    assert np.isfinite(d["grad_predicted"]).all()
    # the fixtures must pin what they are named for
    if name == "lattice_ties":
        dist = np.sort(R.E.dist_f32(pred, gt), axis=2)
        assert (dist[:, :, 0] == dist[:, :, 1]).mean() > 0.3, "few exact ties"
    if name == "coincident_half":
        assert (elem_fwd[:, ::2] == np.float32(1e-4)).all() and (elem_fwd[:, 1::2] > np.float32(1e-3)).all()
    return d


def generate(out_dir):
    ref = ref_harness.import_reference(with_faiss_shim=True)
    assert ref.losses.__file__.startswith(ref_harness.REF_ROOT)
    os.makedirs(out_dir, exist_ok=True)
    for name, (maker, B, M, N, seed) in CASES.items():
        d = make_case(ref, name, maker, B, M, N, seed)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **d)
        print("%-32s %7.1f KB  forward %.6f  backward %.6f" % (name + ".npz", os.path.getsize(path) / 1024, d["forward_loss"],
                                                                d["backward_loss"]))


def report(out_dir):
    """Per case: worst |reference f32 gradient - float64 restatement| / (2^-24 * sum|term|), worst element gap in ulps."""
    for name in CASES:
        g = np.load(os.path.join(out_dir, name + ".npz"))
        ref64, mag = R.grad(g["pred"], g["gt"], g["nn_pg"], g["nn_gp"])
        nz = mag > 0
        gap = np.abs(g["grad_predicted"].astype(np.float64) - ref64)
        assert (gap[~nz] == 0).all()
        worst = float((gap[nz] / (2.0 ** -24 * mag[nz])).max())
        t = R.terms(g["pred"], g["gt"], g["nn_pg"], g["nn_gp"])
        u = max(float(R.ulps(t["elem_fwd"], g["elem_fwd"]).max()), float(R.ulps(t["elem_bwd"], g["elem_bwd"]).max()))
        print("%s: reference gradient gap %.3f x 2^-24 sum|term|, element gap %.1f ulp" % (name, worst, u))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "chamfer")
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
