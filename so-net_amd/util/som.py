"""BatchSOM -- mirror of the reference's util/som.py:175-366 on the MI355X kernels.

Constructor, attributes (``node``, ``node_idx_list``, ``rows/cols/dim/node_num``, ``sigma``,
``learning_rate``, ``max_iteration``) and method signatures follow the reference so that
models/networks.py:104-106,124-144 runs on it unchanged.  What differs is underneath:

* ``query_topk`` / ``query`` call one fused gfx950 kernel (``sonet_som_assign_f32``) instead of
  materialising B x 3 x N x M differences, a B x N x M distance matrix and a B x N x M x k compare;
* the k winners of a point are returned in canonical order -- ascending (distance, node id) -- which
  is one of the orders ``torch.topk(sorted=False)`` (util/som.py:253) is allowed to return;
* ``assign`` exposes the compact result (int32 ids, per-node counts and coordinate sums) that the
  level-2 Encoder consumes directly; the dense one-hot ``mask`` of the reference API is only built
  when ``query_topk`` / ``query`` is called.

The SOM *trainer*: ``optimize`` (util/som.py:355-366) runs the whole schedule in one launch of its own kernel
(csrc/som_train.hip, ``sonet_som_train_f32``); ``batch_update`` (util/som.py:295-352) is restated on top of the
assignment kernel in closed form: for the Gaussian neighbourhood weights w[i, j] the reference's
B x 3 x M x rows x cols broadcast reduces to two M x M products,
    node[:, :, j] += lr * ( sum_i w[i,j] r[b,i] mean[b,:,i]  -  node[b,:,j] * sum_i w[i,j] r[b,i] ).
"""
import math

import numpy as np
import torch

from sonet_hip import ops as _ops
from sonet_hip import overlay as _overlay

# the single-cloud ``SOM`` class (util/som.py:17-172; used by no model, its twin under data/build_som builds the
# node files offline) is served from the reference checkout's own file
__getattr__ = _overlay.delegate(__package__, "som.py", __file__, optional_imports=("torchvision", "faiss"))


class BatchSOM():
    def __init__(self, rows=4, cols=4, dim=3, gpu_id=None, batch_size=10):
        self.rows, self.cols, self.dim = rows, cols, dim
        self.node_num = rows * cols
        self.sigma = 0.4
        self.learning_rate = 0.5
        self.max_iteration = 60
        self.gpu_id = gpu_id
        assert gpu_id >= 0                                              # util/som.py:187
        self.device = torch.device("cuda:%d" % gpu_id if torch.cuda.is_available() else "cpu")
        self.batch_size = batch_size
        self.node = torch.zeros(batch_size, dim, self.node_num, dtype=torch.float32, device=self.device)
        self.node_idx_list = torch.arange(self.node_num, dtype=torch.int64, device=self.device)
        self.init_weighting_matrix = self._gaussian_table(self.sigma).to(self.device)   # M x rows x cols
        self._node_init_value = None
        self.last_assignment = None

    # ------------------------------------------------------------------ neighbourhood weights
    def idx2multi(self, i):
        return (i // self.cols, i % self.cols)

    def gaussian(self, c, sigma):
        d = 2 * np.pi * sigma * sigma
        ax = np.exp(-np.power(np.arange(self.rows) - c[0], 2) / d)
        ay = np.exp(-np.power(np.arange(self.cols) - c[1], 2) / d)
        return torch.from_numpy(np.outer(ax, ay).astype(np.float32))

    def _gaussian_table(self, sigma):
        return torch.stack([self.gaussian(self.idx2multi(i), sigma) for i in range(self.node_num)])

    def get_init_weighting_matrix(self):
        self.init_weighting_matrix = self._gaussian_table(self.sigma).to(self.device)

    def get_weighting_matrix(self, sigma):
        scale = 1.0 / ((sigma / self.sigma) ** 2)
        return torch.exp(torch.log(self.init_weighting_matrix) * scale)

    # ------------------------------------------------------------------ node initialisation
    @property
    def node_init_value(self):
        """dim x M initial node layout from the repulsive potential field (util/potential_field.py, restated in
        ``potential_field_nodes``).  Built lazily -- the models overwrite ``node`` with dataset nodes on every forward
        (models/networks.py:124), so it only runs if ``node_init`` / ``optimize`` is used -- and shared by every instance
        of the same layout."""
        if self._node_init_value is None:
            self._node_init_value = torch.from_numpy(potential_field_nodes(self.node_num, self.dim, self.rows, self.cols)
                                                     .transpose().astype(np.float32))
        return self._node_init_value

    def node_init(self, batch_size):
        self.batch_size = batch_size
        self.node = self.node_init_value.to(self.device).unsqueeze(0).repeat(batch_size, 1, 1).contiguous()

    # ------------------------------------------------------------------ assignment (the hot path)
    def assign(self, x, k, want_i64=False):
        """Compact SOM assignment of x (B x 3 x N) against ``self.node`` (B x 3 x M)."""
        node = self.node
        if node.dtype != torch.float32 or not node.is_contiguous():
            node = node.float().contiguous()
        a = _ops.som_assign(x.contiguous(), node, int(k), want_i64=want_i64)
        self.last_assignment = a
        return a

    def assign_sort(self, x, sn, k, knn=None, deterministic=False):
        """Assignment + node-sorted grouping in two launches (the no-grad pooled path of the level-2 Encoder): -> (assignment,
        grouping dict), or None when the batch is outside what the fused launches take (B > 65535, M > 1024, k > 4) -- the caller
        then uses assign() + som_sort_group."""
        node = self.node
        if node.dtype != torch.float32 or not node.is_contiguous():
            node = node.float().contiguous()
        M = node.shape[2]
        if x.shape[0] > 65535 or M > 1024 or not (1 <= int(k) <= min(4, M)):
            return None
        # (knn = (node_knn_I, K, center_avg): KNNModule's index / coordinate side rides on the second launch -- grouping dict "knn_prep")
        # (deterministic: the order inside a node independent of atomics' arrival -- the training forward's sorted copy)
        a, g = _ops.som_assign_sort(x.contiguous(), sn, node, int(k), knn=knn, deterministic=bool(deterministic) and knn is None)
        self.last_assignment = a
        return a, g

    def query_topk(self, x, k):
        """-> mask B x kN x M int32, mask_row_max B x M int32, min_idx B x kN int64 (k-major)."""
        a = self.assign(x, k, want_i64=True)
        mask = _ops.som_mask(a.min_idx_i32, a.M)
        mask_row_max = (a.count > 0).to(torch.int32)
        return mask, mask_row_max, a.min_idx_i64

    def query(self, x):
        """k = 1 variant with float mask (util/som.py:271-293) -> mask B x N x M f32, mask_row_max B x M f32."""
        a = self.assign(x, 1)
        mask = _ops.som_mask(a.min_idx_i32, a.M).float()
        return mask, (a.count > 0).float()

    # ------------------------------------------------------------------ batch-SOM training
    def batch_update(self, x, learning_rate, sigma):
        assert x.size()[1] == self.dim and x.size()[0] == self.batch_size
        a = self.assign(x, 1)
        g = _ops.som_group(x.contiguous(), None, a)               # mean = sum / (count + 1e-5)
        mean, r = g["som_node"], g["row_max"].float()             # B x 3 x M, B x M
        w = self.get_weighting_matrix(sigma).reshape(self.node_num, self.node_num)      # w[i, j]
        pull = torch.matmul(mean * r.unsqueeze(1), w)                                    # sum_i w[i,j] r_i mean_i
        mass = torch.matmul(r, w).unsqueeze(1)                                           # sum_i w[i,j] r_i
        self.node = self.node + learning_rate * (pull - self.node * mass)

    def train_schedule(self):
        """(lr_t, sigma_t) of optimize at the CURRENT attributes, util/som.py:355-366: int(max_iteration / 3) iterations at
        (learning_rate, sigma), then max_iteration iterations at learning_rate / (1 + 2 it / max_iteration), sigma / (...)."""
        lrs, sigmas = [], []
        for _ in range(int(self.max_iteration / 3)):
            lrs.append(self.learning_rate)
            sigmas.append(self.sigma)
        for it in range(self.max_iteration):
            decay = 1 + 2 * it / self.max_iteration
            lrs.append(self.learning_rate / decay)
            sigmas.append(self.sigma / decay)
        return lrs, sigmas

    def train_tables(self, device=None):
        """-> (lr T, w T x M x M, node_init_value 3 x M), f32 on ``device``, for one som_train launch: w[t] is
        get_weighting_matrix(sigma_t) (exp(log(w0) * scale_t) in f32 on the device, vectorised over t).  The last schedule,
        layout and device are cached."""
        device = torch.device(device) if device is not None else self.init_weighting_matrix.device
        w0 = self.init_weighting_matrix
        key = (self.rows, self.cols, self.sigma, self.learning_rate, self.max_iteration, device, w0.data_ptr(), w0._version)
        cache = self.__dict__.setdefault("_train_tables", {})
        if key not in cache:
            lrs, sigmas = self.train_schedule()
            scales = [1.0 / ((s / self.sigma) ** 2) for s in sigmas]                  # get_weighting_matrix
            lr = torch.tensor(lrs, dtype=torch.float32, device=device)
            sc = torch.tensor(scales, dtype=torch.float32, device=device).view(-1, 1, 1, 1)
            w = torch.exp(torch.log(w0.to(device)).unsqueeze(0) * sc).reshape(len(lrs), self.node_num, self.node_num).contiguous()
            cache.clear()
            cache[key] = (lr, w, self.node_init_value.to(device).contiguous())
        return cache[key]

    def optimize(self, x):
        """util/som.py:355-366: ``node_init`` then the whole schedule -- in ONE som_train launch (csrc/som_train.hip) when the
        kernel takes the shape, else in the batch_update loop.  Afterwards ``node`` is B x 3 x M f32 and ``batch_size`` B."""
        assert x.size()[1] == self.dim
        xs = x.detach()
        if xs.dtype != torch.float32 or not xs.is_contiguous():
            xs = xs.float().contiguous()
        B, _, N = xs.shape
        if not _ops.som_train_supported(N, self.node_num):
            self.node_init(B)
            for lr, sigma in zip(*self.train_schedule()):
                self.batch_update(xs, lr, sigma)
            return
        lr, w, node0 = self.train_tables(xs.device)
        self.batch_size = B
        self.node = _ops.som_train(xs, node0, w, lr)


_PF_NODES = {}


def potential_field_nodes(node_num, dim, rows=None, cols=None):
    """M x dim float64 node layout of the reference's PotentialField (util/potential_field.py), restated:
    a seed-2017 uniform draw in [-1, 1) (a private RandomState: numpy's global generator is left alone), 100 steps of
    node += 0.01 * force with force_j = wall(node_j) + sum_{k = 0..M-1} (node_j - node_k) / n / n^2, n = |node_j - node_k| + 1e-5,
    then the row / column reorder.  The per-node accumulation order is the reference's, and |f| is computed like the
    np.linalg.norm of a 3-vector there (sqrt of BLAS ddot: x0*x0 then fused multiply-adds, emulated exactly below) and n^2 like
    the power of a numpy scalar (libm pow, which is not always n * n), so the result is bit-identical to the reference's.  The reference reorders on a sqrt(M) x sqrt(M) grid only (it fails for other M); for
    such M the grid here is rows x cols."""
    key = (node_num, dim, rows, cols)
    if key in _PF_NODES:
        return _PF_NODES[key].copy()
    M = node_num
    node = np.random.RandomState(2017).rand(M, dim) * 2 - 1
    for _ in range(100):
        force = 0.0 + np.where(np.abs(node) < 0.01, 0.0, -1 * node * M / 1.5)             # wall force first
        for k in range(M):
            f = node - node[k]
            sq = f[:, 0] * f[:, 0]
            for d in range(1, dim):
                sq = _fma(f[:, d], f[:, d], sq)
            fn = np.sqrt(sq) + 0.00001
            fn2 = np.array([math.pow(v, 2) for v in fn.tolist()])                          # f_norm ** 2 of a numpy scalar = libm pow
            force += f / fn[:, None] / fn2[:, None]
        node += force * 0.01
    node = node[node[:, 0].argsort()]
    r = int(math.sqrt(M))
    r, c = (r, r) if r * r == M else (rows, cols)
    node = node.reshape((r, c, dim))
    for i in range(r):
        node[i] = node[i][node[i][:, 1].argsort()]
    node = node.reshape((M, dim))
    _PF_NODES[key] = node
    return node.copy()


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                       # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _fma(a, b, c):
    """Correctly rounded a * b + c in float64 arrays (Boldo & Melquiond's emulation: exact product, exact sum, the low parts
    added with round-to-odd, one final rounding)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    pe = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    th, tl = _two_sum(c, p)
    v, e = _two_sum(tl, pe)
    even = (v.view(np.int64) & 1) == 0
    v = np.where((e != 0) & even, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
    return th + v


_BUILDERS = {}


def build_nodes(pc, rows=8, cols=8, max_iteration=60):
    """SOM nodes of raw clouds: pc B x 3 x N (CUDA) -> B x 3 x (rows * cols) f32.  Every cloud gets the schedule of the
    reference's single-cloud SOM.optimize (util/som.py:150-172, data/build_som), all of them in one launch."""
    dev = pc.device
    key = (rows, cols, dev)
    s = _BUILDERS.get(key)
    if s is None:
        s = _BUILDERS[key] = BatchSOM(rows, cols, 3, dev.index if dev.index is not None else 0, pc.shape[0])
    s.max_iteration = max_iteration
    s.optimize(pc)
    return s.node
