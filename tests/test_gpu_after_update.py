"""A lived-in model against a fresh twin, bit for bit.

The lived-in model trains for a few steps (FusedAdam in between): every weight pack has been refreshed by ``sonet_pack_multi``, every tensor
derived from weights and buffers (models/layers.py: ``_packed*``, ``_lead_cols``, ``_eval_affine``, ``_h3_ok``, ``PointResNet._fused_state``,
``MyLinear``'s affine, the up-convolution packs; models/networks.py: ``Segmenter._layer1_split``) has been built and invalidated, running
statistics have been written through raw pointers.  The twin comes from the constructor, receives the lived-in model's ``state_dict()`` and
runs with ``ops.PACK_REGISTRY = False``: its packs come from the single-pack entries and none of its caches has ever been warm.  Both sides
run the same kernels on the same values, so the comparison has no tolerance: a difference is a stale derived tensor or a refresh that
differs from a fresh pack.

Order of events (W = optimizer step; every comparison is against a twin built at that moment):
    train, W, train, W, train, W | train == twin A | W | eval == twin B | train == twin B | W | train == twin C | eval == twin C
    | train | eval == twin D
Twins C catch what an eval forward built at the earlier weights and statistics and a later step or eval forward still uses; twin D what is
folded from running statistics alone (no parameter changed in between: only the hand-placed invalidations can tell)."""
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_STEPS = 3


def _opt(B, N, M, **kw):
    o = dict(gpu_id=0, device=torch.device(DEV), batch_size=B, input_pc_num=N, surface_normal=True, feature_num=1024, activation="relu",
             normalization="batch", dropout=0.0, node_num=M, k=3, som_k=9, som_k_type="avg", bn_momentum=0.1, bn_momentum_decay_step=None,
             bn_momentum_decay=0.6, classes=40)
    o.update(kw)
    return Namespace(**o)


class Setup:
    """kind "classifier" | "segmenter" | "autoencoder": the modules, their inputs, one training step and one eval forward."""

    def __init__(self, kind, B, N, M):
        from sonet_hip import synth
        self.kind, self.B, self.N, self.M = kind, B, N, M
        if kind == "segmenter":
            self.opt = _opt(B, N, M, som_k_type="center", classes=50)
        elif kind == "autoencoder":
            self.opt = _opt(B, N, M, feature_num=256, output_fc_pc_num=256, output_conv_pc_num=1024, decoder_fused=True,
                            decoder_fused_train=(4, 5, 6), chamfer_fused=True)
        else:
            self.opt = _opt(B, N, M)
        inp = synth.make_inputs(B, N, M=M, som_k=9, seed=9, device=torch.device(DEV))
        gen = torch.Generator().manual_seed(5)
        self.inp = dict(inp, part=torch.randint(0, 50, (B, N), generator=gen).to(DEV), cat=torch.randint(0, 16, (B,), generator=gen).to(DEV))

    def modules(self, seeds=None):
        """Fresh modules from the constructor, in training mode on the device; ``seeds``: synthetic weights (the lived-in model's start)."""
        from models import networks as NW
        from sonet_hip import synth
        head = {"classifier": NW.Classifier, "segmenter": NW.Segmenter, "autoencoder": NW.Decoder}[self.kind](self.opt)
        mods = [NW.Encoder(self.opt), head]
        if self.kind == "classifier":
            mods[0].want_first_pn_out = False
        if seeds is not None:
            for m, s in zip(mods, seeds):
                synth.fill_state_dict_(m.state_dict(), s)
        for m in mods:
            m.to(DEV).train()
        return mods

    def twin_of(self, mods):
        twin = self.modules()
        for t, m in zip(twin, mods):
            t.load_state_dict(m.state_dict())
        return twin

    def train_step(self, mods):
        """forward, loss, backward -> (launch names, dict of everything the step leaves behind)."""
        from models import losses as LS, networks as NW
        from sonet_hip import ops
        enc, head = mods
        i = self.inp
        for m in mods:
            m.train()
            m.zero_grad(set_to_none=True)
        with ops.kernel_timing() as rec:
            if self.kind == "segmenter":
                score = NW.segmentation_forward(enc, head, i["pc"], i["sn"], i["cat"], i["node"], i["node_knn_I"], is_train=True, epoch=0)
                loss = LS.CrossEntropyLossSeg()(score, i["part"])
            else:
                feat = enc(i["pc"], i["sn"], i["node"], i["node_knn_I"], is_train=True, epoch=0)
                if self.kind == "classifier":
                    loss = torch.nn.functional.cross_entropy(head(feat, 0), i["label"])
                else:
                    loss = LS.ChamferLoss(self.opt)(head(feat), i["pc"])
            loss.backward()
        torch.cuda.synchronize()
        out = {"loss": loss.detach().clone()}
        for tag, m in zip(("enc.", "head."), mods):
            out.update({"grad " + tag + k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
            out.update({"stat " + tag + k: v.clone() for k, v in m.state_dict().items() if "running" in k})
        return [n for n, _, _ in rec.records], out

    def eval_forward(self, mods):
        from models import networks as NW
        from sonet_hip import ops
        enc, head = mods
        i = self.inp
        for m in mods:
            m.eval()
        out = {}
        with torch.no_grad(), ops.kernel_timing() as rec:
            if self.kind == "segmenter":
                out["score"] = NW.segmentation_forward(enc, head, i["pc"], i["sn"], i["cat"], i["node"], i["node_knn_I"]).clone()
                out["feature"] = enc.feature.detach().clone()
            else:
                feat = enc(i["pc"], i["sn"], i["node"], i["node_knn_I"], False, None)
                out["feature"] = feat.clone()
                if self.kind == "classifier":
                    out["logits"] = head(feat, None).clone()
                else:
                    out["decoded"] = head(feat).clone()
                    out["conv_pc4"] = head.conv_pc4.clone()
        torch.cuda.synchronize()
        return [n for n, _, _ in rec.records], out


def _same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]))]
    assert not bad, "%s: %d of %d tensors differ from the fresh twin's: %s" % (what, len(bad), len(a), bad[:8])


def _no_packs(names):
    return [n for n in names if "pack" not in n]


def _fused_layers(mods):
    from models import layers as L
    return [(name, m) for mod in mods for name, m in mod.named_modules() if isinstance(m, L._FusedPointwise) and m._fusable()]


class _TwinMode:
    """The twin's side of a comparison: no registry (packs from the single-pack entries)."""

    def __enter__(self):
        from sonet_hip import ops
        self.old = ops.PACK_REGISTRY
        ops.PACK_REGISTRY = False

    def __exit__(self, *exc):
        from sonet_hip import ops
        ops.PACK_REGISTRY = self.old
        return False


def _compare(s, lived, what, train=True, twin=None):
    from sonet_hip import ops
    twin = s.twin_of(lived) if twin is None else twin
    if ops.POINTMLP_PRECISION == "h3":
        # the lived-in model reads the weight side of the range guard lazily (layers.H3_CHECK_EVERY): with every layer inside the guard
        # the two sides cannot legitimately take different arithmetic
        for name, m in _fused_layers(twin):
            assert ops.h3_weight_ok(m._weight2d()), (what, name)
    run = s.train_step if train else s.eval_forward
    with _TwinMode():
        t_names, t_out = run(twin)
    l_names, l_out = run(lived)
    assert any("pack_multi" in n for n in l_names) or not train or what.endswith("same weights"), (what, "the lived-in model refreshed nothing")
    assert not any("pack_multi" in n for n in t_names), what
    _same(l_out, t_out, what)
    assert _no_packs(l_names) == _no_packs(t_names), (what, [(a, b) for a, b in zip(_no_packs(l_names), _no_packs(t_names)) if a != b][:4],
                                                      len(l_names), len(t_names))
    return twin


CASES = [("classifier", "h3", 8, 512, 16), ("classifier", "x3", 8, 512, 16), ("classifier", "bf16", 8, 512, 16), ("segmenter", "h3", 8, 512, 16),
         ("autoencoder", "h3", 4, 512, 16),
         # synthetic_b36_n5000's shape: the smallest that takes the normalise-on-load kernels and the gradient carry (deferred state
         # between layers)
         ("classifier", "bf16", 36, 5000, 64), ("classifier", "h3", 36, 5000, 64)]


@pytest.mark.parametrize("kind,mode,B,N,M", CASES, ids=["%s-%s-b%d-n%d" % c[:4] for c in CASES])
def test_lived_in_model_equals_a_fresh_twin(kind, mode, B, N, M):
    from sonet_hip import ops
    from sonet_hip.optim import FusedAdam
    old_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                    # (the decoder's aten convolutions: the same algorithm on both sides)
    try:
        with ops.precision(mode):
            s = Setup(kind, B, N, M)
            lived = s.modules(seeds=(3, 4))
            opts = [FusedAdam(m.parameters(), lr=1e-3) for m in lived]

            def update():
                for o in opts:
                    o.step()

            for _ in range(K_STEPS):
                s.train_step(lived)
                update()
            _compare(s, lived, "step k + 1")
            update()
            twin = _compare(s, lived, "eval after k + 1 steps", train=False)
            _compare(s, lived, "train after eval, same weights", twin=twin)
            update()
            twin = _compare(s, lived, "train after eval and one more update")
            _compare(s, lived, "second eval", train=False, twin=twin)
            # a step WITHOUT an update: the running statistics move (through raw pointers) while no parameter's version does -- what is
            # folded from them is fresh only where the writer said so by hand (``_affine_key = None``, ``increment_version``)
            s.train_step(lived)
            _compare(s, lived, "eval after a step without an update", train=False)
    finally:
        torch.backends.cudnn.deterministic = old_det
