"""tests/f64_classifier.py -- TEST INFRASTRUCTURE: one classifier training step of the reference in float64, in plain torch autograd,
with the three arg-max pools either FREE (computed here, as the reference computes them) or FORCED (positions given).

Follows, line by line, what ``models/classifier.py:78-99`` runs with dropout off:
  Encoder.forward           models/networks.py:111-199   (query_topk util/som.py:237-269 with sorted slots, grouping :128-172,
                                                          PointResNet models/layers.py:419-432, index_max + gather :180-185,
                                                          KNNModule models/layers.py:313-367, PointNet :384-387, global max :197)
  Classifier.forward        models/networks.py:218-227   (MyLinear models/layers.py:156-166)
  nn.CrossEntropyLoss       models/classifier.py:47,93
BatchNorm in training mode (batch statistics, biased variance: F.batch_norm(training=True), models/layers.py:60-70).

Why it exists: end-to-end gradients pass three arg-max pools; ANY change of rounding flips a few of the
10^5 winners and one flip moves a first-PointNet weight gradient by ~3e-3 rel-rms, so a free-routing comparison can only be statistical.
With the ROUTING of the implementation under test forced on this float64 run, routing flips cannot explain a difference any more and
every gradient must agree to <= 1e-4 rel-rms.  The restatement itself is pinned to the reference: in free mode it reproduces the
``grad64/`` gradients and the ``route64/`` positions the unmodified reference produced in float64 (oracle/make_golden.py
golden_train_step), see tests/test_oracle_golden.py::test_f64_restatement_reproduces_the_reference_float64_run.

``rounding="bf16"``: the same step with bf16 rounding (round to nearest even, 8 significand bits) exactly where the bf16 training step of this
project rounds (``ops.precision("bf16")``), so that with its routing and ReLU patterns forced the only differences left are f32 summation
order and the rare rounding flip it causes (tests/test_gpu_bf16_forced_routing.py).  Forward sites are straight-through
(t + (bf16(t) - t).detach(): the gradient passes unchanged), backward sites are the identity forward and round the incoming gradient.
Forward (so-net_amd/ paths):
  <layer>.weight   every conv weight as a matrix-core operand: the bf16 pack (models/layers.py:715-731, :844), also in the transposed pack
                   of the input-gradient launches (models/layers.py:101-138) -- one rounded copy serves both
  <first>.input    the first layer's input x_aug, cast to the pack's storage type (models/layers.py:845-849)
  <layer>.raw      every layer output as stored: W x + b in f32, rounded once (models/layers.py:363, :369, :552-557; the pool epilogue's
                   values are those of the stored tensor, :550-555)
  <layer>.act      the normalised activation of every BatchNorm + ReLU layer as stored (models/layers.py:372), or as the normalise-on-load
                   operand path rounds it (models/layers.py:1370-1380; bit-identical: tests/test_gpu_bf16_xaff.py)
  knnlayer.layers.0.input, final_pointnet.layers.0.input
                   the f32 + bf16 concat of the node-level stage (models/layers.py:1193, models/networks.py:430), cast by the layer (:846)
  pool1, pool2, pool3
                   the pooled values (models/layers.py:555-558, :1197, models/networks.py:432): gathers of stored bf16 values (pool1 comes
                   back as f32 holding them)
Backward:
  <bn layer>.g_raw the BatchNorm + ReLU backward's output, bf16 (``pointwise_bwd_apply_bf16`` models/layers.py:460, or ``pointmlp_bf16_bnb``
                   :457); the weight gradient reads it (:468)
  <layer>.g_in     every input gradient the dgrad launches store (models/layers.py:141-149, :479-496: bf16 out; the pooled layer's sparse
                   dgrad, both panels, :642-646)
  first_pointnet.skip.g
                   the sum of the first layer's two consumers' gradients, bf16: autograd adds the two bf16 tensors, or, with the gradient
                   carry, the second layer's input-gradient store adds the first one -- y = bf16(float(bf16(result)) + float(acc))
                   (csrc/pointmlp_bf16.hip, sonet_pointmlp_bf16_acc / _bnb; models/layers.py:454-457, :491-492): the same two roundings
  first_pointnet.layers.3.g_out
                   the pooled layer's output gradient (the pooled values are f32 holding bf16 values, their gradient the knn gather's f32
                   backward, models/operations.py:25-28) as an operand of the matrix-core sparse dgrad, with the bf16 weight pack
                   (models/layers.py:616-624, ``ops.pooled_dgrad``: "g and W rounded to bf16"); its weight and bias gradients read it
                   unrounded (:586, :591-602).  ``pooled_dgrad="f32"``: the f32 sparse dgrad (``ops.POOLED_DGRAD_MFMA`` off) rounds neither
                   the gradient nor the weight (:613, :642-643)
  feature.g        ``feature.float()`` (models/networks.py:436): autograd casts the heads' f32 gradient to bf16
Unrounded: weight gradients (f32 out), BatchNorm's statistics and affine-parameter gradients (f32 / f64 sums), the heads (f32 FC layers).
"""
import torch
import torch.nn.functional as F


def _bn_train(y, sd, prefix):
    with torch.no_grad():
        dims = [0] + list(range(2, y.dim()))
        n = y.numel() // y.shape[1]
        _STATS[prefix] = (y.mean(dim=dims), y.var(dim=dims, unbiased=False), n)
    return F.batch_norm(y, None, None, sd[prefix + ".norm.weight"], sd[prefix + ".norm.bias"], True, 0.1, 1e-5)


_TAKEN = {}          # the ReLU patterns the last free run took: {layer prefix: bool tensor}
_STATS = {}          # the batch statistics of every BatchNorm layer of the last run: {layer prefix: (mean, biased var, n)}


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _snap_stats(stored, exact):
    """How far the run's stored bf16 tensor is from the twin's exact value at a forced site:
    ulps   worst distance in bf16 units in the last place of max(|exact|, the tensor's rms) -- a value that cancels to almost nothing carries
           the absolute rounding error of its terms (and of a neighbour's rounding decision one layer up); 0.5 = correctly rounded;
    rel    ||stored - exact|| / ||exact||: bf16 rounding noise is ~1e-3, a tensor 1 % off is >= 1e-2;
    scale  <stored - exact, exact> / <exact, exact>: the relative scale error (rounding noise averages out to ~1e-6 over a tensor)."""
    e = exact.detach()
    d = stored - e
    mag = torch.maximum(e.abs(), e.pow(2).mean().sqrt())
    ulp = torch.ldexp(torch.ones_like(mag), torch.frexp(mag)[1] - 8)
    ee = float((e * e).sum())
    return dict(ulps=float((d.abs() / ulp.clamp_min(2.0 ** -126)).max()), rel=float(d.norm()) / max(ee, 1e-300) ** 0.5,
                scale=float((d * e).sum()) / max(ee, 1e-300))


class _GradRound(torch.autograd.Function):
    """Identity forward; the incoming gradient rounded to bf16 -- or replaced by the run's own (``R.stored_grads``) -- and recorded under
    ``name`` in ``R.bwd_sites``."""

    @staticmethod
    def forward(ctx, x, name, R):
        ctx.name, ctx.R = name, R
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        s = ctx.R.stored_grads.get(ctx.name)
        if s is None:
            out = _bf16(g)
        else:
            out = s.to(device=g.device, dtype=g.dtype).reshape(g.shape)
            ctx.R.snap[ctx.name] = _snap_stats(out, g)
        ctx.R.bwd_sites[ctx.name] = out.detach()
        return out, None, None


# the rounding sites of rounding="bf16" (pooled_dgrad="mfma"; pooled_dgrad="f32" drops "first_pointnet.layers.3.g_out"): see the module docstring
_BN_LAYERS = ("first_pointnet.layers.0", "first_pointnet.layers.1", "first_pointnet.layers.2", "knnlayer.layers.0", "knnlayer.layers.1",
              "final_pointnet.layers.0")
_CONV_LAYERS = _BN_LAYERS[:3] + ("first_pointnet.layers.3",) + _BN_LAYERS[3:] + ("final_pointnet.layers.1",)
BF16_FORWARD_SITES = tuple(sorted([l + ".weight" for l in _CONV_LAYERS] + [l + ".raw" for l in _CONV_LAYERS] + [l + ".act" for l in _BN_LAYERS]
                                  + ["first_pointnet.layers.0.input", "knnlayer.layers.0.input", "final_pointnet.layers.0.input",
                                     "pool1", "pool2", "pool3"]))
BF16_BACKWARD_SITES = tuple(sorted([l + ".g_raw" for l in _BN_LAYERS] + [l + ".g_in" for l in _CONV_LAYERS if l != "first_pointnet.layers.0"]
                                   + ["first_pointnet.skip.g", "first_pointnet.layers.3.g_out", "feature.g"]))


class _Rounder:
    """rounding=None: identities.  "bf16": ``fwd`` straight-through rounding, ``bwd`` gradient rounding; both record what they saw."""

    def __init__(self, rounding, stored=None, stored_grads=None):
        if rounding not in (None, "bf16"):
            raise ValueError("rounding must be None or 'bf16', got %r" % (rounding,))
        self.on = rounding == "bf16"
        self.fwd_sites, self.bwd_sites = {}, {}
        self.stored, self.stored_grads, self.snap = stored or {}, stored_grads or {}, {}

    def fwd(self, name, t):
        if not self.on:
            return t
        s = self.stored.get(name)
        if s is None:
            s = _bf16(t)
        else:
            # the run's own rounding decision: its stored value, which must be the exact value rounded (to within one bf16 unit in the
            # last place of the exact value: f32 accumulation order may tip a value that sits near a rounding midpoint)
            s = s.to(device=t.device, dtype=t.dtype).reshape(t.shape)
            self.snap[name] = _snap_stats(s, t)
        t = t + (s - t).detach()
        self.fwd_sites[name] = t.detach()
        return t

    def bwd(self, name, t):
        return _GradRound.apply(t, name, self) if self.on else t


def _act(y, relu, mask, key=None):
    """ReLU, free (``mask`` None) or FORCED: a given 0 / 1 pattern instead of the sign test -- the other discrete decision of the step."""
    if not relu:
        return y
    if mask is None:
        if key is not None:
            _TAKEN[key] = (y > 0).detach()
        return F.relu(y)
    return y * mask.reshape(y.shape).to(y.dtype)


def _conv(x, sd, prefix, bn, relu, masks=None, R=None):
    w = sd[prefix + ".conv.weight"]
    if R is not None:
        w = R.fwd(prefix + ".weight", w)
    b = sd[prefix + ".conv.bias"]
    y = (F.conv2d if x.dim() == 4 else F.conv1d)(x, w if w.dim() == x.dim() else w.reshape(w.shape[0], w.shape[1], *([1] * (x.dim() - 2))),
                                                    b if R is None or not bn else b.detach())
    if R is not None:
        y = R.fwd(prefix + ".raw", y)
        if bn:
            # (the bias in front of a BatchNorm: its gradient, the sum of the UNROUNDED g_raw, is 0 -- the step returns exact zeros)
            y = R.bwd(prefix + ".g_raw", y) + (b - b.detach()).view(1, -1, *([1] * (y.dim() - 2)))
    if bn:
        y = _bn_train(y, sd, prefix)
    y = _act(y, relu, None if masks is None else masks[prefix], prefix)
    if R is not None and bn:
        y = R.fwd(prefix + ".act", y)
    return y


def _linear(x, sd, prefix, bn, relu, masks=None):
    y = F.linear(x, sd[prefix + ".linear.weight"], sd[prefix + ".linear.bias"])
    if bn:
        y = _bn_train(y, sd, prefix)
    return _act(y, relu, None if masks is None else masks["cls." + prefix], "cls." + prefix)


def leaf_params(sd, device, dtype=torch.float64):
    """state_dict (reference key names) -> {key: float64 leaf requiring grad} for the floating-point entries."""
    out = {}
    for k, v in sd.items():
        if v.is_floating_point():
            out[k] = v.detach().to(device=device, dtype=dtype).clone().requires_grad_(not k.endswith(("running_mean", "running_var")))
    return out


def som_stage(pc, sn, node, k):
    """util/som.py:237-269 (slots in ascending distance order: the reference under ref_harness.sorted_topk()) + models/networks.py:128-172,
    in the dtype of the inputs.  -> min_idx B x kN (k-major), row_max B x M, som_node B x 3 x M, x_augmented B x 6 x kN."""
    B, _, N = pc.shape
    M = node.shape[2]
    diff = pc.unsqueeze(3) - node.unsqueeze(2)                                   # B x 3 x N x M
    diff_norm = (diff ** 2).sum(dim=1)
    _, idx = torch.topk(diff_norm, k=k, dim=2, largest=False, sorted=True)       # B x N x k
    min_idx = torch.cat([idx[..., i] for i in range(k)], dim=1)                  # B x kN
    mask = F.one_hot(min_idx, M)                                                 # B x kN x M
    row_max = mask.max(dim=1)[0]
    row_sum = mask.sum(dim=1)
    x_stack = torch.cat([pc] * k, dim=2)
    sn_stack = torch.cat([sn] * k, dim=2)
    fm = mask.to(pc.dtype).unsqueeze(1)                                          # B x 1 x kN x M
    som_node = (x_stack.unsqueeze(3) * fm).sum(dim=2) / (row_sum.unsqueeze(1).float() + 1e-5)   # (.float(): networks.py:142, also in a float64 run)
    centers = (fm * som_node.unsqueeze(2)).sum(dim=3)
    x_aug = torch.cat((x_stack - centers, sn_stack), dim=1)
    return min_idx, row_max, som_node, x_aug


def index_max_positions(first, min_idx, M, zero_pos=None):
    """models/index_max_ext/index_max.cpp:97-109 on float32 values (the extension reads float32 only: oracle/make_golden.py casts at the
    shim): running max starts at -1000 / position 0, strict '>', ascending n.  first B x C x L, min_idx B x L -> B x C x M (int64).
    ``zero_pos`` (B,): where the reference's "position 0" -- a bin nothing beat -- sits in THIS column order (node-sorted columns: the
    sorted position of original column 0); default 0."""
    v = first.detach().float()
    B, C, L = v.shape
    out = torch.zeros(B, C, M, dtype=torch.int64, device=v.device)
    ar = torch.arange(L, device=v.device)
    z = torch.zeros(B, 1, dtype=torch.int64, device=v.device) if zero_pos is None else zero_pos.long().view(B, 1)
    for m in range(M):
        sel = (min_idx == m)                                                     # B x L
        vm = torch.where(sel.unsqueeze(1), v, torch.full_like(v, -float("inf")))
        best = vm.max(dim=2, keepdim=True)[0]                                    # B x C x 1
        first_at = torch.where(vm == best, ar.view(1, 1, L), torch.full((1, 1, 1), L, device=v.device)).min(dim=2)[0]
        ok = (best.squeeze(2) > -1000.0) & (first_at < L)
        out[:, :, m] = torch.where(ok, first_at, z.expand(B, C))
    return out


def train_step(enc, cls, label, node_knn_I, som_k=9, pc=None, sn=None, node=None, k=3, stage=None, route=None, masks=None, rounding=None,
               stored=None, stored_grads=None, pooled_dgrad="mfma"):
    """One forward + backward.  ``enc`` / ``cls``: ``leaf_params`` dictionaries.
    Inputs either (pc, sn, node) -- the SOM stage runs here, in their dtype -- or ``stage`` = dict(x_aug B x 6 x kN, min_idx B x kN,
    row_max B x M, som_node B x 3 x M[, pos0 B]) taken from the implementation under test (any column order: a point-wise network and
    BatchNorm's batch sums do not care; pos0 = where original column 0 sits in that order, the reference's gather position of an empty
    node, models/networks.py:185).  ``route`` = None (free) or dict(pool1 B x 384 x M positions ALREADY multiplied by row_max, pool2 B x 512 x M,
    pool3 B x F).  ``masks`` = None (ReLU as usual) or {layer prefix ("first_pointnet.layers.0" .. "cls.fc2"): 0 / 1 tensor with the
    element count of that layer's output, in the column order of the stage}: the ReLU pattern of the run under test, forced.
    ``rounding`` = None (plain float64) or "bf16" (the bf16 training step's rounding sites, module docstring);
    ``pooled_dgrad`` (bf16 only) "mfma" | "f32": which sparse input gradient of the pooled layer ran (module docstring);
    ``stored`` (bf16 only) = {forward site: the bf16 tensor the run under test stored there}: its ROUNDING decisions forced, as ``masks``
    forces its ReLU decisions -- a value a hair from a rounding midpoint rounds either way depending on f32 summation order, and one such
    flip perturbs every output of the next layer in that column: left free, the flips multiply ~100x per layer (measured) and the two
    forwards drift apart by bf16 noise.  Each stored value must be the twin's exact value rounded: ``snap`` reports per site its worst
    distance in ulps, its rel-rms distance and its relative scale error (``_snap_stats``) -- forcing a site hides from the gradients
    downstream whatever error the stored tensor carries, so these numbers ARE the check of what produced it;  ``stored_grads`` (bf16
    only) = {backward site: the bf16 gradient the run stored there}: the same for the backward, where the flips multiply the same way.
    -> dict(loss, feature, score, grads {key: tensor}, route {pool1, pool2, pool3}, masks {layer prefix: the ReLU pattern a free run took},
    bn {layer prefix: (batch mean, biased batch variance, element count)}, sites {site: the forward value / the gradient it rounded}
    (rounding="bf16"; empty otherwise), snap {forced site: dict(ulps, rel, scale), see ``_snap_stats``})."""
    _TAKEN.clear()
    _STATS.clear()
    R = _Rounder(rounding, stored, stored_grads) if rounding is not None else None
    e = encoder_forward(enc, node_knn_I, som_k, pc, sn, node, k, stage, route, masks, R, pooled_dgrad)
    feature = e["feature"]
    s = _linear(_linear(feature, cls, "fc1", True, True, masks), cls, "fc2", True, True, masks)
    score = _linear(s, cls, "fc3", False, False)
    loss = F.cross_entropy(score, label.long())
    leaves = {k_: v for k_, v in list(enc.items()) + [("cls." + k_, v) for k_, v in cls.items()] if v.requires_grad}
    gr = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    sites = {} if R is None else dict(R.fwd_sites, **R.bwd_sites)
    return dict(loss=loss.detach(), feature=feature.detach(), score=score.detach(), grads={k_: g for k_, g in zip(leaves, gr) if g is not None},
                route=dict(pool1=e["pool1"], pool2=e["pool2"], pool3=e["pool3"]), masks=dict(_TAKEN), bn=dict(_STATS), sites=sites,
                snap={} if R is None else dict(R.snap))


def encoder_forward(enc, node_knn_I, som_k, pc, sn, node, k, stage, route, masks, R, pooled_dgrad="mfma", som_k_type="avg"):
    """The encoder part of ``train_step`` (models/networks.py:111-199), arguments as there; ``R``: its ``_Rounder`` or None.
    ``som_k_type``: the KNNModule's neighbourhood centre (models/layers.py:340-343), "avg" (the neighbour mean) or "center" (the node).
    -> dict(min_idx, row_max, som_node, x_aug (the stage, detached), first (first_pn_out, B x 384 x kN), pool1, masked_max, knn_center,
    knn_feature (B x 512 x M), pool2, final (final_pn_out, B x 1024 x M), pool3, feature)."""
    dt = next(iter(enc.values())).dtype
    fw = (lambda name, t: t) if R is None else R.fwd
    bw = (lambda name, t: t) if R is None else R.bwd
    if stage is None:
        min_idx, row_max, som_node, x_aug = som_stage(pc.to(dt), sn.to(dt), node.to(dt), k)
    else:
        min_idx, row_max = stage["min_idx"].long(), stage["row_max"].long()
        som_node, x_aug = stage["som_node"].to(dt), stage["x_aug"].to(dt)
    x_aug, som_node = x_aug.detach(), som_node.detach()
    M = som_node.shape[2]
    p = "first_pointnet.layers."
    l0 = _conv(fw(p + "0.input", x_aug), enc, p + "0", True, True, masks, R)
    s0 = bw("first_pointnet.skip.g", l0)
    t = _conv(bw(p + "1.g_in", s0), enc, p + "1", True, True, masks, R)
    t = _conv(bw(p + "2.g_in", t), enc, p + "2", True, True, masks, R)
    x3 = bw(p + "3.g_in", torch.cat((s0, t), dim=1))
    first = _conv(x3 if R is None else x3.detach(), enc, p + "3", False, False, None, R)                      # B x 384 x kN
    if R is not None:
        # the input gradient of the pooled layer takes its own path: W (bf16 pack or f32) against the output gradient (rounded or not)
        if pooled_dgrad not in ("mfma", "f32"):
            raise ValueError("pooled_dgrad must be 'mfma' or 'f32', got %r" % (pooled_dgrad,))
        w3 = enc[p + "3.conv.weight"].detach()
        w3 = _bf16(w3) if pooled_dgrad == "mfma" else w3
        yx = F.conv1d(x3, w3 if w3.dim() == 3 else w3.unsqueeze(2))
        if pooled_dgrad == "mfma":
            yx = bw(p + "3.g_out", yx)
        first = first + (yx - yx.detach())
    if route is None:
        zero_pos = None if stage is None or stage.get("pos0") is None else stage["pos0"]
        pool1 = index_max_positions(first, min_idx, M, zero_pos)
        zp = torch.zeros(pool1.shape[0], 1, 1, dtype=torch.int64, device=pool1.device) if zero_pos is None else zero_pos.long().view(-1, 1, 1)
        pool1 = torch.where(row_max.unsqueeze(1) > 0, pool1, zp.expand_as(pool1))           # networks.py:185: index * mask_row_max
    else:
        pool1 = route["pool1"].long()
    masked_max = fw("pool1", first.gather(2, pool1))                               # networks.py:185
    knn_I = node_knn_I[:, :, :som_k].long()
    B = som_node.shape[0]

    def knn_gather(x):                                                            # operations.py:19-54
        C = x.shape[1]
        return x.gather(2, knn_I.reshape(B, 1, -1).expand(B, C, M * som_k)).reshape(B, C, M, som_k)
    nb = knn_gather(som_node)
    if som_k_type == "avg":
        center = nb.mean(dim=3, keepdim=True)
    elif som_k_type == "center":
        center = som_node.unsqueeze(3)
    else:
        raise ValueError("som_k_type must be 'avg' or 'center', got %r" % (som_k_type,))
    h = torch.cat(((nb - center).detach(), knn_gather(masked_max)), dim=1)
    h = bw("knnlayer.layers.0.g_in", fw("knnlayer.layers.0.input", h))
    h = _conv(h, enc, "knnlayer.layers.0", True, True, masks, R)
    h = _conv(bw("knnlayer.layers.1.g_in", h), enc, "knnlayer.layers.1", True, True, masks, R)   # B x 512 x M x K'
    pool2 = h.max(dim=3)[1] if route is None else route["pool2"].long()
    knn_feature = fw("pool2", h.gather(3, pool2.unsqueeze(3)).squeeze(3))
    f = torch.cat((center.squeeze(3).detach(), knn_feature), dim=1)
    f = bw("final_pointnet.layers.0.g_in", fw("final_pointnet.layers.0.input", f))
    final = _conv(f, enc, "final_pointnet.layers.0", True, True, masks, R)
    final = _conv(bw("final_pointnet.layers.1.g_in", final), enc, "final_pointnet.layers.1", False, False, None, R)
    pool3 = final.max(dim=2)[1] if route is None else route["pool3"].long()
    feature = bw("feature.g", fw("pool3", final.gather(2, pool3.unsqueeze(2)).squeeze(2)))
    return dict(min_idx=min_idx, row_max=row_max, som_node=som_node, x_aug=x_aug, first=first, pool1=pool1, masked_max=masked_max,
                knn_center=center.squeeze(3).detach(), knn_feature=knn_feature, pool2=pool2, final=final, pool3=pool3, feature=feature)
