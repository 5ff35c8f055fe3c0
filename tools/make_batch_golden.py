"""tools/make_batch_golden.py -- fixtures of the batch assembler (sonet_assemble_batch_f32) from the LIVE reference loaders.

Run where the reference checkout is mounted, in its own process:   python tools/make_batch_golden.py [out_dir] [--check]
(default out_dir: tests/golden/batch -- a directory of its own: tests/golden/*.npz are exactly the fixtures of oracle/make_golden.py).

For every case the reference's OWN ModelNet_Shrec_Loader.__getitem__ / ShapeNetLoader.__getitem__ runs on synthetic clouds written
to a temporary directory in the reference's file layout; only the dataset list is bypassed (``self.dataset`` is set directly).
torchvision and h5py are empty modules; faiss is an exact flat L2 search (f32 distance (dx*dx + dy*dy) + dz*dz, ties to the lower
index: oracle/ref_harness.py's stand-in answers k = 1 only).  Before each item numpy is seeded; the tool then re-seeds and repeats the
loader's np.random calls in the same order (choice, uniform(), randn(3), randn(N,3) x 2, randn(M,3), uniform(.8, 1.2),
uniform(-.1, .1, (1, 3))) to record the raw draws, and checks that sonet_hip.batch.augment_np fed with them reproduces the loader's
output bit for bit -- so the recorded draws are the ones the loader used.  Written per case (data only):
  src [6][P] f32, offsets [S+1] i64, nodes_src [S][M][3] f32, labels [S] i64 (, seg [P] i64)    the dataset;
  idx [B] i64, N, M, K, flags, recipe, mode                                                     the batch;
  replay_idx [B][N] i64 (local), replay_draws [B][D] f64                                        the reference's draws;
  pc, sn [B][3][N] f32, node [B][3][M] f32, knn_I [B][M][K] i64, label [B] i64 (, seg_out [B][N] i64)   its output.
--check regenerates into a temporary directory and compares with out_dir array by array.
"""
import os
import sys
import tempfile
import types
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# sonet_hip (the restatement and the draw layout) is imported first; so-net_amd then leaves sys.path again, because its util / models
# packages carry the very names of the reference's, which ref_harness imports next
sys.path.insert(0, os.path.join(ROOT, "so-net_amd"))
from sonet_hip import batch as BA  # noqa: E402
from sonet_hip import ops  # noqa: E402
sys.path.remove(os.path.join(ROOT, "so-net_amd"))

from oracle import ref_harness  # noqa: E402

FOLDERS = ['02691156', '02773838', '02954340', '02958343', '03001627', '03261776', '03467517', '03624134',
           '03636649', '03642806', '03790512', '03797390', '03948459', '04099429', '04225987', '04379243']   # shapenet_loader.py


def _faiss_knn():
    m = types.ModuleType("faiss")

    class IndexFlatL2(object):
        def __init__(self, d):
            assert d == 3

        def add(self, x):
            self.db = np.ascontiguousarray(x, dtype=np.float32)

        def search(self, q, k):
            q = np.ascontiguousarray(q, dtype=np.float32)
            dd = q[:, None, :] - self.db[None, :, :]
            d = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
            ar = np.broadcast_to(np.arange(self.db.shape[0]), d.shape)
            I = np.stack([np.lexsort((ar[r], d[r]))[:k] for r in range(d.shape[0])]).astype(np.int64)
            return np.take_along_axis(d, I, 1), I

    m.IndexFlatL2 = IndexFlatL2
    return m


def import_loaders():
    import importlib
    sys.modules["faiss"] = _faiss_knn()
    ref_harness.import_reference()                      # empty torchvision / h5py, reference on sys.path
    ms = importlib.import_module("data.modelnet_shrec_loader")
    sl = importlib.import_module("data.shapenet_loader")
    assert ms.__file__.startswith(ref_harness.REF_ROOT) and sl.__file__.startswith(ref_harness.REF_ROOT)
    return ms, sl


def clouds(g, sizes, M):
    """points on a noisy sphere-ish shell, unit normals, nodes near the points (float32, the datasets' dtype)."""
    out = []
    for n in sizes:
        p = g.normal(size=(n, 3)) * g.uniform(0.3, 1.0, 3)
        nr = p / np.linalg.norm(p, axis=1, keepdims=True)
        node = p[g.choice(n, M, replace=n < M)] + 0.05 * g.normal(size=(M, 3))
        out.append((np.concatenate([p, nr], 1).astype(np.float32), node.astype(np.float32)))
    return out


def record_draws(seed, recipe, train, flags, n_s, N, M):
    """Re-seed and repeat the loader's np.random calls in its order -> (chosen local [N], draw record [D])."""
    np.random.seed(seed)
    d = np.zeros(ops.batch_draw_size(N, M))
    if recipe == "shapenet":
        if N < n_s:
            chosen = np.random.choice(n_s, N, replace=False)
        else:
            chosen = np.concatenate([np.arange(n_s), np.random.choice(n_s, N - n_s, replace=True)])
    else:
        chosen = np.random.choice(n_s, N, replace=False)
    if train:
        if recipe != "shapenet" and flags["rot_horizontal"]:
            d[0] = np.random.uniform()
        if recipe != "shapenet" and flags["rot_perturbation"]:
            d[1:4] = np.random.randn(3)
        o = ops.BATCH_DRAW_SCALARS
        d[o:o + 3 * N] = np.random.randn(N, 3).reshape(-1)
        d[o + 3 * N:o + 6 * N] = np.random.randn(N, 3).reshape(-1)
        d[o + 6 * N:] = np.random.randn(M, 3).reshape(-1)
        d[4] = np.random.uniform(low=0.8, high=1.2)
        if recipe != "shapenet" and flags["translation_perturbation"]:
            d[5:8] = np.random.uniform(-0.1, 0.1, (1, 3)).reshape(-1)
    return chosen.astype(np.int64), d


def make_case(ms, sl, tmp, name, recipe, mode, sizes, idx, N, M, K, flags, seed):
    g = np.random.RandomState(seed)
    cl = clouds(g, sizes, M)
    S = len(sizes)
    labels = g.randint(0, 16, S).astype(np.int64)
    segs = [g.randint(0, 50, n).astype(np.int64) for n in sizes]
    rows = round(np.sqrt(M))
    opt = Namespace(dataset="shrec" if recipe == "shrec" else "modelnet", input_pc_num=N, node_num=M, som_k=K, batch_size=len(idx),
                    classes=40, **flags)
    root = os.path.join(tmp, name)
    dataset = []
    for s, (data, node) in enumerate(cl):
        if recipe == "shapenet":
            file = "%s/shape%03d" % (FOLDERS[labels[s]], s)
            os.makedirs(os.path.join(root, FOLDERS[labels[s]]), exist_ok=True)
            np.savez(os.path.join(root, file + "_%dx%d.npz" % (rows, rows)), pc=data[:, :3], sn=data[:, 3:], part_label=segs[s],
                     som_node=node)
            dataset.append("shape_data/" + file)
        elif recipe == "shrec":
            f = os.path.join(root, "model_%03d.npz" % s)
            os.makedirs(root, exist_ok=True)
            np.savez(f, pc=data[:, :3], sn=data[:, 3:], som_node=node)
            dataset.append((f, int(labels[s])))
        else:
            for sub in ("c", "%dx%d_som_nodes/c" % (rows, rows)):
                os.makedirs(os.path.join(root, sub), exist_ok=True)
            np.save(os.path.join(root, "c", "c_%04d.npy" % s), data)
            np.save(os.path.join(root, "%dx%d_som_nodes" % (rows, rows), "c", "c_%04d.npy" % s), node)
            dataset.append((os.path.join(root, "c", "c_%04d.npy" % s), int(labels[s]),
                            os.path.join(root, "%dx%d_som_nodes" % (rows, rows), "c", "c_%04d.npy" % s)))
    if recipe == "shapenet":
        L = object.__new__(sl.ShapeNetLoader)
        L.root, L.opt, L.mode, L.node_num, L.rows, L.cols = root, opt, mode, M, rows, rows
        L.dataset = dataset
        L.folders = FOLDERS
        L.knn_builder = sl.KNNBuilder(K)
    else:
        L = object.__new__(ms.ModelNet_Shrec_Loader)
        L.root, L.opt, L.mode, L.dataset = root, opt, mode, dataset
        L.knn_builder = ms.KNNBuilder(K)
    out = {k: [] for k in ("pc", "sn", "node", "knn_I", "label", "seg_out", "replay_idx", "replay_draws")}
    train = mode == "train"
    for b, s in enumerate(idx):
        item_seed = seed * 1000 + b
        np.random.seed(item_seed)
        item = L[s]
        chosen, d = record_draws(item_seed, recipe, train, flags, sizes[s], N, M)
        if recipe == "shapenet":
            pc, sn, label, seg, node, knn = item
            out["seg_out"].append(seg.numpy())
            assert np.array_equal(seg.numpy(), segs[s][chosen])
        else:
            pc, sn, label, node, knn = item[:5]
        want = BA.augment_np(cl[s][0], cl[s][1], chosen, d, train, recipe, **flags)
        for got, exp, what in zip((pc.numpy(), sn.numpy(), node.numpy()), want, ("pc", "sn", "node")):
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), exp.view(np.int32)), \
                "%s slot %d: the restatement fed the recorded draws differs from the loader's %s" % (name, b, what)
        out["pc"].append(pc.numpy()); out["sn"].append(sn.numpy()); out["node"].append(node.numpy())
        out["knn_I"].append(knn.numpy()); out["label"].append(label)
        out["replay_idx"].append(chosen); out["replay_draws"].append(d)
    P = sum(sizes)
    src = np.concatenate([c[0] for c in cl], 0).T.copy()
    res = dict(src=src, offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
               nodes_src=np.stack([c[1] for c in cl]), labels=labels, idx=np.asarray(idx, np.int64), N=np.int32(N), M=np.int32(M),
               K=np.int32(K), recipe=np.str_(recipe), mode=np.str_(mode),
               flags=np.int32((ops.BATCH_TRAIN if train else 0) | (ops.BATCH_SHAPENET if recipe == "shapenet" else 0)
                              | (ops.BATCH_ROT_HORIZONTAL if flags["rot_horizontal"] else 0)
                              | (ops.BATCH_ROT_PERTURBATION if flags["rot_perturbation"] else 0)
                              | (ops.BATCH_TRANSLATION if flags["translation_perturbation"] else 0)),
               **{k: np.stack(v) for k, v in out.items() if v and k != "label"})
    res["label"] = np.asarray(out["label"], np.int64)
    if recipe == "shapenet":
        res["seg"] = np.concatenate(segs)
    assert src.shape == (6, P)
    return res


ON = dict(rot_horizontal=True, rot_perturbation=True, translation_perturbation=True)
OFF = dict(rot_horizontal=False, rot_perturbation=False, translation_perturbation=False)
CASES = {   # name: recipe, mode, cloud sizes, idx, N, M, K, flags, seed
    "modelnet_train_all_flags": ("modelnet", "train", [1000, 800, 1200], [0, 2, 1, 0], 500, 64, 9, ON, 1),
    "modelnet_train_no_flags": ("modelnet", "train", [1000, 800, 1200], [2, 1, 0], 500, 64, 9, OFF, 2),
    "modelnet_test": ("modelnet", "test", [1000, 800, 1200], [1, 0, 2], 500, 64, 9, ON, 3),
    "shrec_train_4x4_k1": ("shrec", "train", [700, 600], [1, 0], 256, 16, 1, ON, 4),
    "shapenet_train_ragged": ("shapenet", "train", [600, 512, 400], [0, 1, 2, 2], 512, 64, 9, OFF, 5),
    "modelnet_train_bench_shape": ("modelnet", "train", [10000], [0], 5000, 64, 9, ON, 6),
}


def generate(out_dir):
    ms, sl = import_loaders()
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, spec in CASES.items():
            d = make_case(ms, sl, tmp, name, *spec)
            path = os.path.join(out_dir, name + ".npz")
            np.savez_compressed(path, **d)
            print("%-34s %8.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = args[0] if args else os.path.join(ROOT, "tests", "golden", "batch")
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
