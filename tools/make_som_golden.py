"""tools/make_som_golden.py -- fixtures of the SOM trainer (BatchSOM.optimize, util/som.py:355-366) from the LIVE reference.

Run where the reference checkout is mounted, in its own process:   python tools/make_som_golden.py [out_dir]
(default out_dir: tests/golden/som -- a directory of its own: tests/golden/*.npz are exactly the fixtures of
oracle/make_golden.py, which tests/test_overlay_reference.py regenerates).  Imports the unmodified reference through oracle.ref_harness (read-only) and writes
tests/golden/som/som_optimize_*.npz, data only:
  x [B][3][N] f32          seeded clouds;
  node_init [3][M] f32     the reference's node_init_value (util/potential_field.py);
  ref32 [B][3][M] f32      the reference's BatchSOM.optimize result in float32;
  ref64 [B][3][M] f64      the same in float64 (the instance's node, init_weighting_matrix and node_init_value cast to double);
  ref32_dev [B] f64        per cloud rms(ref32 - ref64): the SOM trajectory follows Voronoi-boundary decisions, so this measured
                           spread of the reference's own float32 run is the yardstick of a float32 implementation;
  rows, cols, max_iteration.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402


def clouds_8x8(N, seed):
    """uniform cube, sphere surface, three tight clusters (most nodes stay empty), N copies of 12 distinct points."""
    g = np.random.RandomState(seed)
    cube = g.uniform(-1, 1, (3, N))
    s = g.normal(size=(3, N))
    sphere = s / np.linalg.norm(s, axis=0, keepdims=True)
    centres = g.uniform(-0.7, 0.7, (3, 3))
    clusters = centres[:, g.randint(0, 3, N)] + 0.02 * g.normal(size=(3, N))
    distinct = g.uniform(-1, 1, (3, 12))
    dups = distinct[:, np.arange(N) % 12]
    return np.stack([cube, sphere, clusters, dups]).astype(np.float32)


def run(ref, rows, cols, x, max_iteration=60):
    s = ref.som.BatchSOM(rows, cols, 3, 0, x.shape[0])
    s.max_iteration = max_iteration
    node_init = s.node_init_value.clone()
    s.optimize(torch.from_numpy(x))
    ref32 = s.node.clone().numpy()
    s.node = s.node.double()
    s.init_weighting_matrix = s.init_weighting_matrix.double()
    s.node_init_value = s.node_init_value.double()
    s.optimize(torch.from_numpy(x).double())
    ref64 = s.node.clone().numpy()
    dev = np.sqrt(np.mean((ref32.astype(np.float64) - ref64) ** 2, axis=(1, 2)))
    return dict(x=x, node_init=node_init.numpy(), ref32=ref32, ref64=ref64, ref32_dev=dev,
                rows=np.int32(rows), cols=np.int32(cols), max_iteration=np.int32(max_iteration))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "som")
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = ref_harness.import_reference()
    g = np.random.RandomState(5)
    cases = {
        "som_optimize_8x8_n5000": (8, 8, clouds_8x8(5000, 11)),
        "som_optimize_4x4_n1024": (4, 4, g.uniform(-1, 1, (2, 3, 1024)).astype(np.float32)),
        "som_optimize_8x8_n40": (8, 8, g.uniform(-1, 1, (2, 3, 40)).astype(np.float32)),        # N < M
    }
    for name, (rows, cols, x) in cases.items():
        d = run(ref, rows, cols, x)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **d)
        print("%-30s %8.1f KB  ref32_dev %s" % (name + ".npz", os.path.getsize(path) / 1024,
                                                 " ".join("%.2e" % v for v in d["ref32_dev"])))


if __name__ == "__main__":
    main()
