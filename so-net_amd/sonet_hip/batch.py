"""Training / test batches assembled on the device (the reference's DataLoader item + collate, without the host).

The reference builds every step's batch in DataLoader workers: per cloud a random subset of the points, rotations, jitter, scale
and shift in float64 numpy, a faiss self-kNN of the SOM nodes, then collate and a host-to-device copy
(data/modelnet_shrec_loader.py:193-271, data/shapenet_loader.py:131-198, data/augmentation.py).  Here the dataset is loaded to the
device once (``DeviceClouds``) and each batch is one ``sonet_assemble_batch_f32`` launch plus the node kNN (``BatchAssembler``).  The
batch is the tuple the reference's loader collates, same dtypes and layouts, so ``Model.set_input(*batch)`` takes it unchanged.

The module also holds the numpy restatement of the kernel's random-number contract (``philox4x32_10``, ``slot_draws``) and of the
reference's float64 augmentation fed with given draws (``augment_np``): the tests and tools/make_batch_golden.py use them.
"""
import math
import os

import numpy as np
import torch

from . import ops
from ._lib import SonetHipError

RECIPES = ("modelnet", "shrec", "shapenet")


# ---------------------------------------------------------------------------------------------------- numpy restatement of the RNG
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_TWO_M32 = 2.0 ** -32


def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr (..., 4) u32 counter words, key (2,) u32 -> (..., 4) u32."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _blocks(seed, step, b, stream, elements):
    e = np.asarray(elements, dtype=np.uint64)
    ctr = np.stack(np.broadcast_arrays(np.uint64(step & 0xFFFFFFFF), np.uint64(b), np.uint64(stream), e), -1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def unit(w):
    """u32 -> uniform in [0, 1): w * 2^-32."""
    return np.asarray(w, dtype=np.float64) * _TWO_M32


def normals3(w):
    """(..., 4) u32 blocks -> (..., 3) f64 standard normals (Box-Muller, include/sonet_hip.h)."""
    w = np.asarray(w)
    ra = np.sqrt(-2.0 * np.log((w[..., 0].astype(np.float64) + 1.0) * _TWO_M32))
    rb = np.sqrt(-2.0 * np.log((w[..., 2].astype(np.float64) + 1.0) * _TWO_M32))
    ta, tb = 2 * np.pi * unit(w[..., 1]), 2 * np.pi * unit(w[..., 3])
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb)], -1)


def slot_draws(seed, step, b, n_s, N, M, recipe="modelnet"):
    """What the kernel draws for slot b: (chosen local indices [N] i64 in output order, draw record [D] f64)."""
    if recipe == "shapenet" and N >= n_s:
        t = np.arange(N - n_s)
        w = _blocks(seed, step, b, 1, t >> 2)[np.arange(len(t)), t & 3] if len(t) else np.zeros(0, np.uint32)
        chosen = np.concatenate([np.arange(n_s), (w.astype(np.uint64) * np.uint64(n_s)) >> np.uint64(32)]).astype(np.int64)
    else:
        keys = _blocks(seed, step, b, 0, np.arange((n_s + 3) // 4)).reshape(-1)[:n_s]
        chosen = np.sort(np.lexsort((np.arange(n_s), keys))[:N]).astype(np.int64)
    d = np.zeros(ops.batch_draw_size(N, M))
    w0, w2 = _blocks(seed, step, b, 2, 0), _blocks(seed, step, b, 2, 2)
    d[0] = unit(w0[0])
    d[1:4] = normals3(_blocks(seed, step, b, 2, 1))
    d[4] = 0.8 + (1.2 - 0.8) * unit(w0[1])
    d[5:8] = -0.1 + (0.1 - -0.1) * unit(w2[:3])
    o = ops.BATCH_DRAW_SCALARS
    d[o:o + 3 * N] = normals3(_blocks(seed, step, b, 3, np.arange(N))).reshape(-1)
    d[o + 3 * N:o + 6 * N] = normals3(_blocks(seed, step, b, 4, np.arange(N))).reshape(-1)
    d[o + 6 * N:] = normals3(_blocks(seed, step, b, 5, np.arange(M))).reshape(-1)
    return chosen, d


def augment_np(data, som_node, chosen, d, train, recipe="modelnet", rot_horizontal=False, rot_perturbation=False,
               translation_perturbation=False):
    """The reference's __getitem__ arithmetic (float64 numpy, the same calls in the same order) fed with given draws.

    data n_s x 6 (points | normals), som_node M x 3, chosen [N] local indices, d the draw record -> (pc 3xN, sn 3xN, node 3xM) f32."""
    N, M = len(chosen), som_node.shape[0]
    data = data[chosen, :]
    pc_np, sn_np, som_node_np = data[:, 0:3], data[:, 3:6], som_node
    if train:
        if recipe != "shapenet" and rot_horizontal:
            rotation_angle = d[0] * 2 * np.pi
            cosval, sinval = np.cos(rotation_angle), np.sin(rotation_angle)
            R = np.array([[cosval, 0, sinval], [0, 1, 0], [-sinval, 0, cosval]])
            pc_np, sn_np, som_node_np = np.dot(pc_np, R), np.dot(sn_np, R), np.dot(som_node_np, R)
        if recipe != "shapenet" and rot_perturbation:
            angles = np.clip(0.06 * d[1:4], -0.18, 0.18)
            Rx = np.array([[1, 0, 0], [0, np.cos(angles[0]), -np.sin(angles[0])], [0, np.sin(angles[0]), np.cos(angles[0])]])
            Ry = np.array([[np.cos(angles[1]), 0, np.sin(angles[1])], [0, 1, 0], [-np.sin(angles[1]), 0, np.cos(angles[1])]])
            Rz = np.array([[np.cos(angles[2]), -np.sin(angles[2]), 0], [np.sin(angles[2]), np.cos(angles[2]), 0], [0, 0, 1]])
            R = np.dot(Rz, np.dot(Ry, Rx))
            pc_np, sn_np, som_node_np = np.dot(pc_np, R), np.dot(sn_np, R), np.dot(som_node_np, R)
        o = ops.BATCH_DRAW_SCALARS
        jp = d[o:o + 3 * N].reshape(N, 3)
        jn = d[o + 3 * N:o + 6 * N].reshape(N, 3)
        jm = d[o + 6 * N:o + 6 * N + 3 * M].reshape(M, 3)
        t = np.clip(0.01 * jp, -0.05, 0.05)
        t += pc_np
        pc_np = t
        t = np.clip(0.01 * jn, -0.05, 0.05)
        t += sn_np
        sn_np = t
        t = np.clip(0.04 * jm, -0.1, 0.1)
        t += som_node_np
        som_node_np = t
        scale = d[4]
        pc_np, som_node_np, sn_np = pc_np * scale, som_node_np * scale, sn_np * scale
        if recipe != "shapenet" and translation_perturbation:
            shift = d[5:8].reshape(1, 3)
            pc_np += shift
            som_node_np += shift
    return (pc_np.transpose().astype(np.float32), sn_np.transpose().astype(np.float32),
            som_node_np.transpose().astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the dataset on the device
def _clouds(a, name):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(a, np.ndarray):
        if a.ndim != 3 or a.shape[2] != 3:
            raise SonetHipError("%s must be S x n x 3 or a list of n_i x 3, got %s" % (name, a.shape))
        return list(a)
    out = [np.asarray(c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c) for c in a]
    for c in out:
        if c.ndim != 2 or c.shape[1] != 3:
            raise SonetHipError("%s: every cloud must be n_i x 3, got %s" % (name, c.shape))
    return out


class DeviceClouds:
    """A whole split on the device: points and normals packed planar (``src`` 6 x P f32) with CSR ``offsets`` (S+1 i64), ``labels`` S
    i64, ``nodes`` S x M x 3 f32 (the reference's som_nodes file layout), ``seg`` P i64 per-point part labels (optional).

    points / normals: per-cloud n_i x 3 arrays (ragged allowed) or one S x n x 3.  nodes=None builds them once with
    ``util.som.build_nodes`` (8 x 8, the dataset notebook's schedule), which needs clouds of equal size."""

    def __init__(self, points, normals, labels, nodes=None, seg=None, device=None, rows=8, cols=8):
        dev = torch.device(device if device is not None else "cuda")
        pts, nrm = _clouds(points, "points"), _clouds(normals, "normals")
        if len(pts) != len(nrm) or any(p.shape != n.shape for p, n in zip(pts, nrm)):
            raise SonetHipError("points and normals must have the same clouds and sizes")
        S = len(pts)
        if S < 1:
            raise SonetHipError("no clouds")
        sizes = np.array([p.shape[0] for p in pts], dtype=np.int64)
        if sizes.min() < 1 or sizes.max() > 2 ** 31 - 1:
            raise SonetHipError("every cloud needs 1 .. 2^31-1 points")
        self.sizes = sizes
        self.offsets_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        flat = np.concatenate([np.concatenate(pts, 0), np.concatenate(nrm, 0)], 1).astype(np.float32)      # P x 6
        self.src = torch.from_numpy(np.ascontiguousarray(flat.T)).to(dev)
        self.offsets = torch.from_numpy(self.offsets_host).to(dev)
        self.labels = torch.as_tensor(np.asarray(labels, dtype=np.int64)).to(dev)
        if self.labels.shape != (S,):
            raise SonetHipError("labels must hold one class per cloud (%d), got %s" % (S, tuple(self.labels.shape)))
        if nodes is None:
            if sizes.min() != sizes.max():
                raise SonetHipError("ragged clouds without nodes: pass nodes (S x M x 3), build_nodes needs equal sizes")
            from util import som
            pc = self.src[:3].reshape(3, S, int(sizes[0])).permute(1, 0, 2).contiguous()
            nodes = som.build_nodes(pc, rows, cols).transpose(1, 2)
        nodes = torch.as_tensor(nodes.detach() if isinstance(nodes, torch.Tensor) else np.asarray(nodes, dtype=np.float32))
        if nodes.dim() != 3 or nodes.shape[0] != S or nodes.shape[2] != 3:
            raise SonetHipError("nodes must be S x M x 3, got %s" % (tuple(nodes.shape),))
        self.nodes = nodes.to(device=dev, dtype=torch.float32).contiguous()
        self.seg = None
        if seg is not None:
            sg = [np.asarray(s.cpu().numpy() if isinstance(s, torch.Tensor) else s, dtype=np.int64).reshape(-1) for s in
                  (list(seg) if not isinstance(seg, np.ndarray) or seg.ndim != 1 else [seg])]
            flat_seg = np.concatenate(sg)
            if flat_seg.shape[0] != self.offsets_host[-1]:
                raise SonetHipError("seg must hold one label per point (%d), got %d" % (self.offsets_host[-1], flat_seg.shape[0]))
            self.seg = torch.from_numpy(flat_seg).to(dev)

    def __len__(self):
        return len(self.sizes)

    @property
    def device(self):
        return self.src.device

    @property
    def node_num(self):
        return self.nodes.shape[1]

    @classmethod
    def from_modelnet(cls, root, mode, opt, device=None):
        """The reference's on-disk ModelNet layout (make_dataset_modelnet40_10k, data/modelnet_shrec_loader.py:28-64):
        modelnet<classes>_shape_names.txt, modelnet<classes>_<mode>.txt, <class>/<name>.npy (n x 6), <r>x<c>_som_nodes/<class>/<name>.npy."""
        rows = round(math.sqrt(opt.node_num))
        with open(os.path.join(root, "modelnet%d_shape_names.txt" % opt.classes)) as f:
            shape_list = [s.rstrip() for s in f.readlines()]
        if mode not in ("train", "test"):
            raise SonetHipError("Network mode error.")
        with open(os.path.join(root, "modelnet%d_%s.txt" % (opt.classes, mode))) as f:
            lines = [s.rstrip() for s in f.readlines()]
        pts, nrm, labels, nodes = [], [], [], []
        for name in lines:
            folder = name[0:-5]
            data = np.load(os.path.join(root, folder, name + ".npy"))
            pts.append(data[:, 0:3])
            nrm.append(data[:, 3:6])
            labels.append(shape_list.index(folder))
            nodes.append(np.load(os.path.join(root, "%dx%d_som_nodes" % (rows, rows), folder, name + ".npy")))
        return cls(pts, nrm, labels, np.stack(nodes).astype(np.float32), device=device)


# ---------------------------------------------------------------------------------------------------- batches
class BatchAssembler:
    """Batches of ``clouds`` with the reference's recipe.  Reads input_pc_num, node_num, som_k, rot_horizontal, rot_perturbation and
    translation_perturbation from ``opt``; mode 'train' augments, 'test' only subsamples; recipe 'modelnet' / 'shrec' / 'shapenet'.

    ``batch(idx, step)`` -> modelnet (pc, sn, label, node, node_knn_I); shrec appends index; shapenet (pc, sn, label, seg, node,
    node_knn_I).  The draws of a slot depend on (seed, step, slot) only.  Not for graph capture: the step is a kernel argument."""

    def __init__(self, clouds, opt, mode="train", recipe="modelnet", seed=0):
        if recipe not in RECIPES:
            raise SonetHipError("recipe must be one of %s, got %r" % (RECIPES, recipe))
        if mode not in ("train", "test", "val"):
            raise SonetHipError("mode must be train / test / val, got %r" % (mode,))
        if recipe == "shapenet" and clouds.seg is None:
            raise SonetHipError("the shapenet recipe needs per-point part labels (DeviceClouds(seg=...))")
        self.clouds, self.mode, self.recipe, self.seed = clouds, mode, recipe, int(seed)
        self.N, self.M = int(opt.input_pc_num), int(opt.node_num)
        if clouds.node_num != self.M:
            raise SonetHipError("opt.node_num=%d but the clouds carry %d nodes" % (self.M, clouds.node_num))
        self.K = int(opt.som_k) if opt.som_k >= 2 else 1
        f = ops.BATCH_TRAIN if mode == "train" else 0
        if recipe == "shapenet":
            f |= ops.BATCH_SHAPENET
        else:
            f |= ops.BATCH_ROT_HORIZONTAL if getattr(opt, "rot_horizontal", False) else 0
            f |= ops.BATCH_ROT_PERTURBATION if getattr(opt, "rot_perturbation", False) else 0
            f |= ops.BATCH_TRANSLATION if getattr(opt, "translation_perturbation", False) else 0
            if self.N > int(clouds.sizes.min()):
                raise SonetHipError("input_pc_num=%d > %d points of the smallest cloud (sampling without replacement)"
                                    % (self.N, int(clouds.sizes.min())))
        self.flags = f

    def _run(self, idx, step, check, **kw):
        c = self.clouds
        return ops.assemble_batch(c.src, c.offsets, c.nodes, idx, self.N, self.K, self.flags, self.seed, step,
                                  sizes=c.sizes if check else None, **kw)

    def _pack(self, idx, r):
        c = self.clouds
        label = c.labels[idx]
        if self.recipe == "shapenet":
            return r["pc"], r["sn"], label, c.seg[r["chosen"]], r["node"], r["knn_I"]
        if self.recipe == "shrec":
            return r["pc"], r["sn"], label, r["node"], r["knn_I"], idx
        return r["pc"], r["sn"], label, r["node"], r["knn_I"]

    def _idx(self, idx):
        return torch.as_tensor(np.asarray(idx, dtype=np.int64) if not isinstance(idx, torch.Tensor) else idx,
                               dtype=torch.int64).to(self.clouds.device).contiguous()

    def batch(self, idx, step):
        """One batch of the clouds ``idx`` (sequence or tensor of cloud numbers) at ``step``; idx is checked before the launch."""
        idx = self._idx(idx)
        return self._pack(idx, self._run(idx, step, True))

    def batch_with_draws(self, idx, step, replay_idx=None, replay_draws=None):
        """``batch`` plus the raw dict of ops.assemble_batch with the draw record (replay / inspection)."""
        idx = self._idx(idx)
        r = self._run(idx, step, True, replay_idx=replay_idx, replay_draws=replay_draws, want_draws=True)
        return self._pack(idx, r), r

    def batches_per_epoch(self, batch_size):
        return (len(self.clouds) + batch_size - 1) // batch_size

    def epoch(self, epoch, batch_size, shuffle=True):
        """The batches of one epoch (the last one may be short, as DataLoader's default): a device-side permutation seeded from
        (seed, epoch) when shuffling; step = epoch * batches_per_epoch + i, so no two steps of a run share draws."""
        S, dev = len(self.clouds), self.clouds.device
        if shuffle:
            g = torch.Generator(device=dev)
            g.manual_seed((self.seed * 1000003 + int(epoch)) % (2 ** 63))
            order = torch.randperm(S, generator=g, device=dev)
        else:
            order = torch.arange(S, device=dev)
        nb = self.batches_per_epoch(batch_size)
        for i in range(nb):
            idx = order[i * batch_size:(i + 1) * batch_size]
            yield self._pack(idx, self._run(idx, int(epoch) * nb + i, False))
