"""SHREC16 retrieval on the device: class-restricted ranked neighbour lists with one host transfer, for the files alone.

The reference's retrieval script (shrec16/test.py:42-99) fills an N x 55 score matrix batch by batch and then runs, per test shape, a
Python iteration of ``torch.eq`` / ``torch.nonzero`` over all predicted labels, ``torch.norm`` of the gathered rows, ``torch.sort``, two
device-to-host copies and one ``np.savetxt``.  Here ``ShapeRetrieval`` accumulates the scores in preallocated device buffers and one
``ops.retrieval_lists`` call (``sonet_retrieval_lists_f32``) ranks every shape against its own predicted class.

In shrec16/test.py lines 42-99 become

    lists = retrieve_shrec(model.encoder, model.classifier, assembler, opt.batch_size)     # a test-mode 'shrec' BatchAssembler
    lists.write(output_folder)

with ``model_ids=`` when the files are to be named by something else than the assembler's cloud index.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import SonetHipError


def write_lists(folder, model_ids, nn_id, nn_dist, count):
    """Host arrays -> one file per query named '%06d' % model_ids[q] with count[q] rows '%06d %f' (id, distance): the files of
    shrec16/test.py:93-99 (np.savetxt with that format).  Returns the number of files."""
    os.makedirs(folder, exist_ok=True)
    nn_dist = np.asarray(nn_dist, dtype=np.float64)
    for q in range(len(model_ids)):
        k = int(count[q])
        with open(os.path.join(folder, "%06d" % model_ids[q]), "w") as f:
            f.write("".join("%06d %f\n" % (i, d) for i, d in zip(nn_id[q, :k].tolist(), nn_dist[q, :k].tolist())))
    return len(model_ids)


class ShapeRetrieval:
    """Scores (or any ``channels``-wide feature) and model ids of up to ``capacity`` shapes, then their ranked lists.  ``update``
    launches two copies and returns (no sync, no ``.item()``); ``lists`` makes the one ``ops.retrieval_lists`` call over what was
    accumulated; ``write`` makes the one device-to-host transfer and writes the reference's files."""

    def __init__(self, capacity, channels, top=1000, device=None):
        if not 1 <= int(capacity) <= ops.RETRIEVAL_MAX_N or not 1 <= int(channels) <= ops.RETRIEVAL_MAX_D:
            raise SonetHipError("ShapeRetrieval: need 1 <= capacity < 2^24 and 1 <= channels <= %d, got %r and %r"
                                % (ops.RETRIEVAL_MAX_D, capacity, channels))
        if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= ops.RETRIEVAL_MAX_TOP:
            raise SonetHipError("top must be an int in [1, %d], got %r" % (ops.RETRIEVAL_MAX_TOP, top))
        self.capacity, self.channels, self.top = int(capacity), int(channels), top
        self.device = torch.device(device) if device is not None else None
        self._feat = self._ids = None
        self.filled = 0
        self._lists = None

    def reset(self):
        self.filled = 0
        self._lists = None

    def update(self, score, model_ids):
        """score B x channels f32, model_ids B i64, both on the device: copied to rows filled .. filled + B."""
        for t, name, dtype, dim in ((score, "score", torch.float32, 2), (model_ids, "model_ids", torch.int64, 1)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise SonetHipError("%s must be a CUDA tensor/variable" % name)
            if t.dtype != dtype or t.dim() != dim:
                raise SonetHipError("%s must be %d-D %s, got %s %s" % (name, dim, dtype, tuple(t.shape), t.dtype))
        B = score.shape[0]
        if score.shape[1] != self.channels or model_ids.shape[0] != B:
            raise SonetHipError("score must be B x %d and model_ids B, got %s and %s" % (self.channels, tuple(score.shape),
                                                                                        tuple(model_ids.shape)))
        if self.filled + B > self.capacity:
            raise SonetHipError("ShapeRetrieval: %d + %d shapes exceed the capacity %d" % (self.filled, B, self.capacity))
        if self._feat is None:
            dev = self.device if self.device is not None else score.device
            self._feat = torch.empty((self.capacity, self.channels), dtype=torch.float32, device=dev)
            self._ids = torch.empty((self.capacity,), dtype=torch.int64, device=dev)
        self._feat[self.filled:self.filled + B].copy_(score)
        self._ids[self.filled:self.filled + B].copy_(model_ids)
        self.filled += B
        self._lists = None

    @property
    def features(self):
        return self._feat[:self.filled]

    @property
    def model_ids(self):
        return self._ids[:self.filled]

    def lists(self, labels=None, n_label=None, want_pos=False):
        """``ops.RetrievalLists`` of every accumulated shape: labels None = the arg-max of the scores, as the reference predicts."""
        if self.filled == 0:
            raise SonetHipError("ShapeRetrieval.lists() before any update()")
        self._lists = ops.retrieval_lists(self.features, labels=labels, ids=self.model_ids, top=self.top, n_label=n_label,
                                          want_pos=want_pos)
        return self._lists

    def write(self, folder):
        """One file per shape named '%06d' % id with rows '%06d %f' (id, distance), nearest first, at most ``top`` rows: what
        shrec16/test.py:93-99 writes.  Returns the number of files."""
        r = self._lists if self._lists is not None else self.lists()
        Q, top = r.nn_id.shape
        packed = torch.cat([r.nn_id.reshape(-1), r.nn_dist.reshape(-1).view(torch.int32).to(torch.int64), r.count.to(torch.int64),
                            self.model_ids, r.bad.to(torch.int64)]).cpu().numpy()              # the one transfer
        nn_id = packed[:Q * top].reshape(Q, top)
        nn_dist = packed[Q * top:2 * Q * top].astype(np.int32).view(np.float32).reshape(Q, top)
        count, ids, bad = packed[2 * Q * top:2 * Q * top + Q], packed[2 * Q * top + Q:2 * Q * top + 2 * Q], int(packed[-1])
        if bad:
            raise SonetHipError("retrieval: %d shape(s) with a label outside [0, n_label)" % bad)
        return write_lists(folder, ids, nn_id, nn_dist, count)


def retrieve_shrec(encoder, classifier, assembler, batch_size, top=1000, model_ids=None):
    """One pass over the split of a test-mode shrec ``BatchAssembler``: forward per batch, ``update`` with the class scores and the
    cloud indices (``model_ids``: a device i64 tensor indexed by cloud index, to name the shapes otherwise), no host sync inside the
    loop; returns the ``ShapeRetrieval`` with its lists computed."""
    if assembler.recipe != "shrec" or assembler.mode == "train":
        raise SonetHipError("retrieve_shrec needs a test-mode shrec BatchAssembler, got recipe %r mode %r"
                            % (assembler.recipe, assembler.mode))
    encoder.eval()
    classifier.eval()
    acc = None
    with torch.no_grad():
        for pc, sn, label, node, node_knn_I, index in assembler.epoch(0, batch_size, shuffle=False):
            score = classifier(encoder(pc, sn, node, node_knn_I)).float().contiguous()
            if acc is None:
                acc = ShapeRetrieval(len(assembler.clouds), score.shape[1], top=top, device=score.device)
            acc.update(score, index if model_ids is None else model_ids[index])
    acc.lists()
    return acc
