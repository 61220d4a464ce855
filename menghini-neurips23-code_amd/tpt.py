"""Test-time prompt tuning (TPT: Shu et al., NeurIPS 2022 -- the model of include/grip_amd.h, grip_view_entropy, not the paper's code) for the textual
strategies: every test image gets its OWN prompt for the time of its prediction.  An episode takes `views` views of the image (view 0 the image itself,
the others augment.ViewSampler boxes under the item's base name with the epoch fixed at 0: the views of pseudolabels.MultiView), keeps the
keep = max(1, floor(rho views)) views whose prediction has the lowest entropy, takes `steps` AdamW steps on the context from a zero optimizer state
against the entropy of their mean prediction (engine.view_entropy), classifies view 0 with the tuned context and puts the context back, bit for bit.

The image tower of a textual strategy is frozen, so an item's V views are encoded once and an episode is a text-tower step on their features.  An episode
never all-reduces a gradient: ranks hold different items, and different counts of them.  Nothing here touches the strategy's optimizer."""
import math

import torch

from . import engine, pseudolabels as pl, steps as gsteps


def keep_from_rho(views, rho):
    """max(1, floor(rho views)): the number of confident views an episode keeps."""
    return max(1, int(math.floor(float(rho) * int(views))))


class TestTimeTuner:
    """TestTimeTuner(model, clip_model, ...): `model` a models.TextPrefixModel (model.classes names the class list of the episodes), clip_model the CLIP
    whose frozen image tower made the view features.  lr, steps and rho are the paper's; AdamW runs on torch's defaults otherwise (betas 0.9 / 0.999,
    eps 1e-8, weight decay 0.01), as the paper's code does.  Only model.prefix is tuned: the deep prompts of a deep-CoOp model stay frozen.

    graphed: NOT BUILT (the default is False, True raises).  A captured episode step (forward + loss + backward replayed from a HIP graph per item)
    was tried and taken out: with episodes enqueued back to back and no host synchronisation between them its rows went wrong at the ViT-B/16 text-tower shapes and stayed wrong
    (cause not found), and where it was right it saved 0.6 % of an episode that is bound by the GPU, not by launches (tools/tpt_probe.py).

    `episodes` counts the tune() calls."""
    __test__ = False      # (not a test class, whatever its name suggests to a collector)

    def __init__(self, model, clip_model, views=64, rho=0.1, lr=5e-3, steps=1, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=0.5, seed=0, graphed=False):
        from .augment import ViewSampler
        if isinstance(views, bool) or not isinstance(views, int) or not 1 <= views <= engine.VIEW_MODE_MAX_VIEWS:
            raise ValueError(f"TestTimeTuner: views = {views!r} (an integer in 1 .. {engine.VIEW_MODE_MAX_VIEWS})")
        if not 0.0 < float(rho) <= 1.0:
            raise ValueError(f"TestTimeTuner: rho = {rho} (0 < rho <= 1)")
        if not 0.0 <= float(lr) < math.inf:
            raise ValueError(f"TestTimeTuner: lr = {lr} (a finite lr >= 0)")
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
            raise ValueError(f"TestTimeTuner: steps = {steps!r} (an integer >= 0)")
        self.model, self.clip_model = model, clip_model
        self.views, self.rho, self.lr, self.steps = views, float(rho), float(lr), steps
        self.keep = keep_from_rho(views, rho)
        self.sampler = ViewSampler(seed=seed, scale=scale, ratio=ratio, flip=flip)      # (raises on a bad scale / ratio / flip)
        self.targets = gsteps.ViewEntropyTargets(views, self.keep)
        if graphed:
            raise ValueError("TestTimeTuner: graphed = True is not built (the episode step runs eagerly)")
        self.episodes = 0
        self._scale = None
        self._optimizer = None

    # ------------------------------------------------------------------ views
    def boxes(self, names, H, W):
        """int32 [len(names) * views, 5]: pseudolabels.view_boxes of this tuner's sampler -- an item's boxes depend on its name alone."""
        return pl.view_boxes(self.sampler, self.views, names, H, W)

    def make_views(self, images, names):
        """images [B, 3, H, H] f32 on the GPU -> their views [B * views, 3, H, H], image-major (view 0 is a bit-exact copy)."""
        return pl.make_views(self.sampler, self.views, images, names)

    @torch.no_grad()
    def encode_views(self, images, names, chunk=880):
        """[B, views, e] f32: the frozen image tower's features of the batch's views, encoded on THIS rank alone (Tower.encode_chunks: the rows
        encode_pool writes for the same views on one rank, bit for bit, and no cache key -- a view is not the image a PoolFeatureCache knows).
        NOT encode_pool: that is a collective over a pool every rank holds alike, and `predict` hands every rank different items."""
        vw = self.make_views(images.float().contiguous(), list(names))
        tower = self.clip_model.visual.tower
        out = torch.empty(vw.shape[0], tower.embed_dim, dtype=torch.float32, device=tower.device)
        tower.encode_chunks(vw, out, 0, vw.shape[0], chunk)
        return out.view(images.shape[0], self.views, -1)

    # ------------------------------------------------------------------ the episode
    def scale(self):
        if self._scale is None:
            self._scale = self.clip_model.logit_scale.exp().item()
        return self._scale

    def _loss(self, x):
        logits = gsteps.CosineHeadFn.apply(x, self.model(self.model.classes), self.scale())
        return gsteps.step_loss(logits, None, None, soft=self.targets)

    def _backward_eager(self, x):
        self.model.prefix.grad = None
        self._loss(x).backward()

    def tune(self, view_features):
        """view_features f32 [views, e] of ONE item (row 0: the image itself) -> its logits row [C] under the context tuned on them.  model.prefix, its
        .grad and every other parameter are afterwards what they were, bit for bit."""
        x = view_features.detach().float().contiguous()
        if x.dim() != 2 or x.shape[0] != self.views:
            raise ValueError(f"TestTimeTuner.tune: view features [{self.views}, e] of one item were expected, got {tuple(x.shape)}")
        model = self.model
        prefix, deep = model.prefix, getattr(model, "deep_prefix", None)
        saved, saved_grad = prefix.detach().clone(), prefix.grad
        deep_rg = None if deep is None else deep.requires_grad
        self.episodes += 1
        try:
            if deep is not None:
                deep.requires_grad_(False)      # frozen for the episode: no gradient is computed for it, its .grad is not touched
            if self._optimizer is None or self._optimizer.param_groups[0]["params"][0] is not prefix:
                self._optimizer = torch.optim.AdamW([prefix], lr=self.lr)      # the tuner's OWN optimizer
            self._optimizer.state.clear()       # every episode starts from a zero state
            self._optimizer.param_groups[0]["lr"] = self.lr
            with torch.enable_grad():
                for _ in range(self.steps):
                    self._backward_eager(x)
                    self._optimizer.step()
            with torch.no_grad():
                row = engine.cosine_head(x[:1], model(model.classes), self.scale(), want_probs=False)[0][0]
        finally:
            with torch.no_grad():
                prefix.copy_(saved)
            prefix.grad = saved_grad
            if deep is not None:
                deep.requires_grad_(deep_rg)
        return row

    @torch.no_grad()
    def predict_rows(self, view_features):
        """[B, views, e] -> [B, C]: one episode per item, in order."""
        return torch.stack([self.tune(view_features[i]) for i in range(view_features.shape[0])])
