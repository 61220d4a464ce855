"""Prompt-tuning steps on the native engine (forward + input-gradient backward + SGD on the prompt
tensors only), shaped after the reference's `_train_epoch` bodies:
  CoOp  methods/semi_supervised_learning/textual_prompt.py:92-135
  VPT   methods/unsupervised_learning/visual_prompt.py:113-140
  UPT   methods/transductive_zsl/multimodal_prompt.py:98-133
The per-sample `.item()` host syncs of the reference loops are gone: labels stay on the device.
"""
import torch

from . import dist as gdist
from . import engine
from .engine import CandidateCEFn, CosineHeadFn, SoftCEFn, ViewEntropyFn, WeightedCEFn


def fpl_row_weights(is_pseudo, gamma_seen=1.0, gamma_pseudo=1.0):
    """Per-row weights that turn `gamma_a * CE(rows_a) + gamma_b * CE(rows_b)` (each CE a mean over
    its own rows) into one weighted sum: the FPL losses of
    methods/semi_supervised_learning/textual_fpl.py:117-165 (gamma_seen = |unseen|/|seen|, gamma_pseudo = 1),
    methods/transductive_zsl/textual_fpl.py:117-147 (gamma_seen = 1, gamma_pseudo = |seen|/|unseen|) and
    methods/unsupervised_learning/visual_fpl.py:107-122 (all rows one group)."""
    is_pseudo = torch.as_tensor(is_pseudo, dtype=torch.bool)
    n_p = int(is_pseudo.sum())
    n_s = is_pseudo.numel() - n_p
    w = torch.zeros(is_pseudo.numel(), dtype=torch.float32)
    if n_s:
        w[~is_pseudo] = gamma_seen / n_s
    if n_p:
        w[is_pseudo] = gamma_pseudo / n_p
    return w


class SoftTargets:
    """What a prompt step needs to train on soft targets (engine.soft_ce): `matrix` f32 [rows, cz] on the device -- the Z or Q a pseudolabel pass ranked,
    read in place (pseudolabels.SoftTargetStore.matrix) -- `col_map` int32 [cz], the logits column of every matrix column, the sharpening
    `temperature` and the label `smoothing`.  matrix=None: smoothing alone (every row keeps its one-hot).  A step takes it as `soft=` together with a
    per-batch `soft_row` int32 [B] (the matrix row of each batch row, -1: a hard row); tip_step and adapter_step keep hard labels."""

    def __init__(self, matrix=None, col_map=None, temperature=1.0, smoothing=0.0):
        if (matrix is None) != (col_map is None):
            raise ValueError("SoftTargets: matrix and col_map come together")
        if not 0.0 < float(temperature) < float("inf"):
            raise ValueError(f"SoftTargets: temperature = {temperature} (a finite temperature > 0)")
        if not 0.0 <= float(smoothing) < 1.0:
            raise ValueError(f"SoftTargets: smoothing = {smoothing} (0 <= smoothing < 1)")
        self.matrix, self.col_map, self.temperature, self.smoothing = matrix, col_map, float(temperature), float(smoothing)

    def key(self):
        """What a captured graph depends on: the addresses it read the matrix and the map from, their shapes and the two scalars."""
        m, c = self.matrix, self.col_map
        return (None if m is None else (m.data_ptr(), tuple(m.shape), c.data_ptr()), self.temperature, self.smoothing)


class CandidateTargets:
    """What a prompt step needs to train on candidate SETS with the partial-label loss (engine.candidate_ce): `mask` int32 [rows, ceil(cz / 32)] on the
    device -- the sets the last pseudolabel pass selected, read in place (pseudolabels.CandidateStore.mask) -- and `col_map` int32 [cz], the logits
    column of every mask column.  A step takes it as `soft=`, as it takes a SoftTargets, together with a per-batch `soft_row` int32 [B] that then carries
    the MASK row of each batch row (-1: a hard row); step_loss dispatches on the type.  tip_step and adapter_step keep hard labels."""

    def __init__(self, mask, col_map):
        if not torch.is_tensor(mask) or mask.dim() != 2 or mask.dtype != torch.int32 or not torch.is_tensor(col_map) or col_map.dim() != 1:
            raise ValueError(f"CandidateTargets: an int32 [rows, words] mask and a [cz] col_map were expected, got {getattr(mask, 'shape', type(mask))} "
                             f"{getattr(mask, 'dtype', None)} and {getattr(col_map, 'shape', type(col_map))}")
        if mask.shape[1] != (col_map.shape[0] + 31) // 32:
            raise ValueError(f"CandidateTargets: a mask of {mask.shape[1]} words for {col_map.shape[0]} classes (ceil(cz / 32) words)")
        self.mask, self.col_map = mask, col_map

    @property
    def matrix(self):
        """The per-pool-row buffer, under the name the graphed steps ask a SoftTargets for."""
        return self.mask

    def key(self):
        """What a captured graph depends on: the addresses it read the mask and the map from, and their shapes."""
        return ("candidates", self.mask.data_ptr(), tuple(self.mask.shape), self.col_map.data_ptr())


class ViewEntropyTargets:
    """What a test-time episode step (tpt.TestTimeTuner) hands over as `soft=`: no targets at all -- the logits' rows are `views` views per image,
    image-major, and the loss is the entropy of the mean prediction of every image's `keep` most confident views (engine.view_entropy); step_loss
    dispatches on the type.  labels, row_weight and soft_row are not read."""

    matrix = None      # no per-pool-row buffer: a graphed step keeps no soft_row

    def __init__(self, views, keep):
        for name, val in (("views", views), ("keep", keep)):
            if isinstance(val, bool) or not isinstance(val, int):
                raise ValueError(f"ViewEntropyTargets: {name} = {val!r} (an integer)")
        if not 1 <= views <= engine.VIEW_MODE_MAX_VIEWS or not 1 <= keep <= views:
            raise ValueError(f"ViewEntropyTargets: views = {views}, keep = {keep} (1 <= views <= {engine.VIEW_MODE_MAX_VIEWS}, 1 <= keep <= views)")
        self.views, self.keep = views, keep

    def key(self):
        """What a captured graph depends on."""
        return ("view_entropy", self.views, self.keep)


def step_loss(logits, labels, row_weight, soft=None, soft_row=None):
    """The loss of a prompt step: WeightedCEFn, exactly as before, without `soft`; SoftCEFn on the rows of soft.matrix that soft_row names with a
    SoftTargets; CandidateCEFn on the rows of soft.mask that soft_row names with a CandidateTargets; ViewEntropyFn with a ViewEntropyTargets."""
    if soft is None:
        return WeightedCEFn.apply(logits, labels, row_weight)
    if isinstance(soft, CandidateTargets):
        if soft_row is None:
            raise ValueError("a step with candidate sets needs the batch's soft_row (the mask row of every batch row, -1 for a hard row)")
        return CandidateCEFn.apply(logits, labels, row_weight, soft.mask, soft_row, soft.col_map)
    if isinstance(soft, ViewEntropyTargets):
        return ViewEntropyFn.apply(logits, soft.views, soft.keep)
    if soft.matrix is None:
        return SoftCEFn.apply(logits, labels, row_weight, None, None, None, soft.temperature, soft.smoothing)
    if soft_row is None:
        raise ValueError("a step with a soft-target matrix needs the batch's soft_row (the matrix row of every batch row, -1 for a hard row)")
    return SoftCEFn.apply(logits, labels, row_weight, soft.matrix, soft_row, soft.col_map, soft.temperature, soft.smoothing)


_SIDE = {}


def _side_stream(device):
    key = torch.device(device).index or 0
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


def _finish(loss, params, optimizer, logits=None):
    loss.backward()
    gdist.allreduce_mean_([p.grad for p in params if p.grad is not None])
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)       # the next backward adopts its gradient tensors (no fill, no add kernels)
    return loss.detach() if logits is None else (loss.detach(), logits.detach())


def _coop_params(model):
    """The textual model's trainable tensors: the context and, with deep CoOp (model.deep_prefix [D, P, d]), its deep prompts -- their gradient is
    all-reduced with the context's."""
    deep = getattr(model, "deep_prefix", None)
    return [model.prefix] if deep is None else [model.prefix, deep]


def coop_step(model, clip_model, images, labels, row_weight, optimizer, image_features=None, return_logits=False, soft=None, soft_row=None):
    """Textual prompt step: text tower forward+backward over all class prompts, frozen image tower
    forward only (or cached features).  soft / soft_row: SoftTargets and the batch's matrix rows (step_loss); None: hard labels."""
    side = None
    if image_features is None:
        # the frozen image tower does not depend on the prompt: run it on a second stream next to the text
        # tower's forward (both are small-batch launches that leave CUs idle on their own)
        side = _side_stream(images.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            image_features = clip_model.encode_image(images)
    text_features = model(model.classes)
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
        image_features.record_stream(torch.cuda.current_stream())
    logits = CosineHeadFn.apply(image_features, text_features, clip_model.logit_scale.exp().item())
    loss = step_loss(logits, labels, row_weight, soft, soft_row)
    return _finish(loss, _coop_params(model), optimizer, logits if return_logits else None)


def vpt_step(model, text_features, logit_scale, images, labels, row_weight, optimizer, return_logits=False, soft=None, soft_row=None):
    """Visual prompt step: image tower forward+backward; text features fixed for the epoch.  soft / soft_row: as coop_step."""
    image_features = model(images)
    logits = CosineHeadFn.apply(image_features, text_features, logit_scale)
    loss = step_loss(logits, labels, row_weight, soft, soft_row)
    deep = getattr(model, "deep_prefix", None)      # VPT-Deep: its gradient is all-reduced with the prompt's
    return _finish(loss, [model.prefix] if deep is None else [model.prefix, deep], optimizer, logits if return_logits else None)


def upt_step(model, logit_scale, images, labels, row_weight, optimizer, return_logits=False, soft=None, soft_row=None):
    """Multimodal prompt step: mixer + both towers forward and backward.  soft / soft_row: as coop_step."""
    text_features, image_features = model(images, model.classes)
    logits = CosineHeadFn.apply(image_features, text_features, logit_scale)
    loss = step_loss(logits, labels, row_weight, soft, soft_row)
    return _finish(loss, [p for p in model.parameters() if p.requires_grad], optimizer, logits if return_logits else None)


class GraphedStep:
    """A prompt step whose forward + backward is captured ONCE in a HIP graph and replayed per step (shapes are static within an
    epoch: same batch size, same class list).  A CoOp step is ~330 launches of 10-25 us on two streams, a UPT step adds the
    mixer's dozens of tiny torch kernels; replaying them as one graph removes the per-launch host cost, nothing else changes: the
    captured kernels are the ones the eager step launches, the prompt-gradient all-reduce and the optimizer step stay outside
    the graph (eager), so the same object serves one GPU and N.  A batch of another shape falls back to the eager step.

    Static inputs: images [B,3,R,R] / labels [B] / row weights [B] are copied into fixed buffers before each replay; the
    trainable parameters are read in place, their .grad buffers are written in place.  Subclasses give `forward_logits`
    (static inputs -> logits), `params` and the eager fallback.

    soft (a SoftTargets, the prompt steps only): the loss is step_loss on it, and the step is called with a fourth argument soft_row [B] that is copied
    into one more static int32 buffer.  The graph captures the ADDRESSES of soft.matrix and soft.col_map: a pass that writes a new matrix of the same
    shape into the same buffer (pseudolabels.SoftTargetStore.record does) is what the next replay trains on; a SoftTargets whose key() moved --
    another buffer, shape, temperature or smoothing -- is a batch of "another shape" and runs the eager step."""

    def __init__(self, optimizer, soft=None):
        self.optimizer = optimizer
        self.soft = soft
        self.graph = None
        self.key = None
        self._pins = []
        self.r = self._soft_row = None

    def __del__(self):
        try:
            engine.release_pins(self._pins)
        except Exception:
            pass

    # -- subclass interface
    def params(self):
        raise NotImplementedError

    def forward_logits(self):
        raise NotImplementedError

    def eager(self, images, labels, row_weight):
        raise NotImplementedError

    def shape_key(self, images):
        return (tuple(images.shape), images.dtype)

    def _key(self, images):
        key = self.shape_key(images)
        return key if self.soft is None else key + (self.soft.key(),)

    def _wants_rows(self):
        return self.soft is not None and self.soft.matrix is not None

    # -- machinery
    def _body(self):
        logits = self.forward_logits()
        self.logits = logits.detach()      # [B, C] of the step just run (a static buffer of the graph; the eager fallback's own tensor)
        loss = step_loss(logits, self.y, self.w, self.soft, self.r)
        loss.backward()
        return loss.detach()

    def _capture(self, images, labels, row_weight, soft_row=None):
        dev = images.device
        self.x, self.y, self.w = images.clone(), labels.to(torch.int32).clone(), row_weight.to(torch.float32).clone()
        if self._wants_rows():
            self.r = soft_row.to(device=dev, dtype=torch.int32).clone()
        self.key = self._key(images)
        ps = self.params()
        warm = torch.cuda.Stream(device=dev)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):              # warm-up off the default stream: workspaces, lazy kernel attributes, cached token ids
            for _ in range(2):
                for p in ps:
                    p.grad = None
                self._body()
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # the workspaces the captured forwards take are dedicated to this graph (never handed to an eager forward while it lives)
        with engine.pin_workspaces() as self._pins, torch.cuda.graph(self.graph):
            # .grad = None inside the capture: autograd then ADOPTS each gradient tensor the backward produces (memory of the graph's
            # private pool, rewritten in place by every replay) instead of zero-filling a buffer and adding into it -- for the UPT
            # step that was one fill and one add kernel per mixer parameter, 44 launches of ~2 us in a 3.4-ms step (r03)
            for p in ps:
                p.grad = None
            self.loss = self._body()
        self._graph_logits = self.logits           # the graph's static output buffer
        for p in ps:
            if p.grad is None:                     # (a parameter the loss does not reach)
                p.grad = torch.zeros_like(p)
        self.grads = [p.grad for p in ps]

    def __call__(self, images, labels, row_weight, soft_row=None):
        if self._wants_rows() and soft_row is None:
            raise ValueError("a graphed step with a soft-target matrix needs the batch's soft_row")
        self._soft_row = soft_row                  # (what the eager fallback passes on)
        if self.graph is None:
            self._capture(images, labels, row_weight, soft_row)
        if self._key(images) != self.key:
            for p in self.params():
                p.grad = None                      # (the graph's gradient buffers hold the previous replay's values)
            loss, self.logits = self.eager(images, labels, row_weight)
            return loss
        self.x.copy_(images)
        self.y.copy_(labels)
        self.w.copy_(row_weight)
        if self.r is not None:
            self.r.copy_(soft_row)
        for p, g in zip(self.params(), self.grads):
            p.grad = g
        self.graph.replay()
        self.logits = self._graph_logits
        gdist.allreduce_mean_(self.grads)
        self.optimizer.step()
        return self.loss


class GraphedCoopStep(GraphedStep):
    """coop_step (textual prompt: text tower forward + backward, frozen image tower on a side stream) replayed from a HIP graph.  A model with deep
    prompts (deep CoOp, model.deep_prefix) has them captured as one more static parameter."""

    def __init__(self, model, clip_model, optimizer, soft=None):
        super().__init__(optimizer, soft)
        self.model, self.clip_model = model, clip_model
        self.scale = clip_model.logit_scale.exp().item()

    def params(self):
        return _coop_params(self.model)

    def shape_key(self, images):
        return (tuple(images.shape), images.dtype, tuple(self.model.classes))

    def forward_logits(self):
        side = _side_stream(self.x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            image_features = self.clip_model.encode_image(self.x)
        text_features = self.model(self.model.classes)
        torch.cuda.current_stream().wait_stream(side)
        return CosineHeadFn.apply(image_features, text_features, self.scale)

    def eager(self, images, labels, row_weight):
        return coop_step(self.model, self.clip_model, images, labels, row_weight, self.optimizer, return_logits=True, soft=self.soft, soft_row=self._soft_row)


class GraphedCoopFeatureStep(GraphedStep):
    """coop_step on image features that were encoded ahead (lookahead_image_features): the text tower's forward + backward, the
    cosine head and the loss, replayed from a HIP graph; the static input is the feature block [B, embed_dim]."""

    def __init__(self, model, clip_model, optimizer, soft=None):
        super().__init__(optimizer, soft)
        self.model, self.clip_model = model, clip_model
        self.scale = clip_model.logit_scale.exp().item()

    def params(self):
        return _coop_params(self.model)

    def shape_key(self, feats):
        return (tuple(feats.shape), feats.dtype, tuple(self.model.classes))

    def forward_logits(self):
        return CosineHeadFn.apply(self.x, self.model(self.model.classes), self.scale)

    def eager(self, feats, labels, row_weight):
        return coop_step(self.model, self.clip_model, None, labels, row_weight, self.optimizer, image_features=feats, return_logits=True, soft=self.soft,
                         soft_row=self._soft_row)


def lookahead_overlap():
    """Quarters of the chip an overlapped look-ahead encode may use (1-3), 0 = no overlap (the default).  $GRIP_LOOKAHEAD_OVERLAP (developer A/B: measured
    and rejected in r05 -- on this runtime the masked stream's kernels and the graph replays of the steps do not run side by side)."""
    import os
    v = os.environ.get("GRIP_LOOKAHEAD_OVERLAP", "0")
    return int(v) if v in ("0", "1", "2", "3") else 0


def lookahead_image_features(clip_model, batches, group=8, overlap=None):
    """The frozen image tower of a textual-prompt epoch, run `group` batches ahead: the image features of a step do not depend
    on the prompt being trained, so the batches of `group` consecutive steps are encoded in ONE inference forward (group x B x S
    rows feed the persistent 256x256 GEMMs at the pool-encode rate; a 16-image forward leaves them a quarter full) and each
    step receives its slice.  Every image is still encoded every time a step uses it (nothing is cached across steps or epochs),
    and the engine's forward is chunk-independent, so the features are bit-identical to a per-step encode.

    r05 experiment, OFF by default (`overlap` / GRIP_LOOKAHEAD_OVERLAP = 1..3 quarters of the chip): the encode of group g + 1 enqueued on a CU-masked
    side stream (engine.masked_stream; the persistent kernels size their grids to it, grip_set_cu_budget) BEFORE group g's features are yielded, so that
    it could run beside the prompt steps -- a latency-bound chain of ~176 launches of 28 - 60 workgroups each -- on the CUs the mask leaves free.  Same
    features bit for bit (tests/test_gpu_determinism.py), but no overlap happens on this runtime: encode 28.5 ms + 51 steps 56.3 ms take 102 ms
    "together" (88 ms with an ordinary side stream), tools/overlap_probe.py; profiles/HISTORY.md 11.6.

    `batches` yields tuples whose first element is the image batch [B, 3, R, R] (any further elements are passed through);
    yields (features [B, embed_dim], *rest) in the same order."""
    quarters = lookahead_overlap() if overlap is None else int(overlap)

    def groups():
        pending = []
        for b in batches:
            pending.append(b)
            if len(pending) == group:
                yield pending
                pending = []
        if pending:
            yield pending

    def encode(pending, side=None, budget=0):
        x = torch.cat([b[0] for b in pending])
        with torch.no_grad():
            if side is None:
                return clip_model.encode_image(x)
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                engine.set_cu_budget(budget)
                try:
                    feats = clip_model.encode_image(x)
                finally:
                    engine.set_cu_budget(0)
            x.record_stream(side)
            return feats

    def slices(pending, feats):
        at = 0
        for b in pending:
            n = b[0].shape[0]
            yield (feats[at:at + n],) + tuple(b[1:])
            at += n

    it = groups()
    cur = next(it, None)
    if cur is None:
        return
    ms = engine.masked_stream(cur[0][0].device, quarters) if quarters and cur[0][0].is_cuda else None
    if ms is None:
        while cur is not None:
            yield from slices(cur, encode(cur))
            cur = next(it, None)
        return
    side, n_cus = ms
    feats = encode(cur)
    while cur is not None:
        nxt = next(it, None)
        nxt_feats = encode(nxt, side, n_cus) if nxt is not None else None      # enqueued BEFORE this group's steps: runs beside them
        yield from slices(cur, feats)
        if nxt is not None:
            torch.cuda.current_stream().wait_stream(side)
            nxt_feats.record_stream(torch.cuda.current_stream())
        cur, feats = nxt, nxt_feats


class GraphedVptStep(GraphedStep):
    """vpt_step (visual prompt: image tower forward + backward; text features fixed for the epoch) replayed from a HIP graph.  The graph
    captures a shared prompt ([P, d] / [1, P, d]), with its deep prompts (VPT-Deep, model.deep_prefix [D, P, d]) as one more static parameter when
    the model has them; a model whose prompt is per image ([B, P, d]) runs the eager step."""

    def __init__(self, model, text_features, logit_scale, optimizer, soft=None):
        super().__init__(optimizer, soft)
        self.model, self.text_features, self.scale = model, text_features, float(logit_scale)

    def params(self):
        deep = getattr(self.model, "deep_prefix", None)
        return [self.model.prefix] if deep is None else [self.model.prefix, deep]

    def forward_logits(self):
        return CosineHeadFn.apply(self.model(self.x), self.text_features, self.scale)

    def __call__(self, images, labels, row_weight, soft_row=None):
        if engine.is_per_image_prefix(self.model.prefix):
            self._soft_row = soft_row
            loss, self.logits = self.eager(images, labels, row_weight)
            return loss
        return super().__call__(images, labels, row_weight, soft_row)

    def eager(self, images, labels, row_weight):
        return vpt_step(self.model, self.text_features, self.scale, images, labels, row_weight, self.optimizer, return_logits=True, soft=self.soft,
                        soft_row=self._soft_row)


class GraphedUptStep(GraphedStep):
    """upt_step (multimodal prompt: mixer + both towers forward and backward, towers on two streams) replayed from a HIP graph.  Every trainable
    parameter is captured, vpt_embeddings_deep included: with mix_deep (deep UPT) the graph holds the deep mixer and the tower's deep prompts."""

    def __init__(self, model, logit_scale, optimizer, soft=None):
        super().__init__(optimizer, soft)
        self.model, self.scale = model, float(logit_scale)

    def params(self):
        return [p for p in self.model.parameters() if p.requires_grad]

    def shape_key(self, images):
        return (tuple(images.shape), images.dtype, tuple(self.model.classes))

    def forward_logits(self):
        text_features, image_features = self.model(self.x, self.model.classes)
        return CosineHeadFn.apply(image_features, text_features, self.scale)

    def eager(self, images, labels, row_weight):
        return upt_step(self.model, self.scale, images, labels, row_weight, self.optimizer, return_logits=True, soft=self.soft, soft_row=self._soft_row)


def tip_step(model, image_features, clip_logits, labels, row_weight, optimizer, return_logits=False):
    """Tip-Adapter-F step on a models.TipAdapterModel with train_keys: cache head over cached image features and the CLIP logits of the trained
    prompt (both constants of the step) -> weighted CE -> the keys' gradient -> optimizer.  No tower runs.  Hard labels only (no soft targets)."""
    logits = model(image_features, clip_logits)
    loss = WeightedCEFn.apply(logits, labels, row_weight)
    return _finish(loss, [model.keys], optimizer, logits if return_logits else None)


class GraphedTipStep(GraphedStep):
    """tip_step replayed from a HIP graph: the cache head's forward and backward and the loss are four kernels, so a step is launch cost and little
    else.  The static inputs are the feature block [B, embed_dim] (GraphedStep's `x`) and the CLIP logits [B, C] of the same rows; call it as
    step(image_features, labels, row_weight, clip_logits)."""

    def __init__(self, model, optimizer):
        super().__init__(optimizer)
        self.model = model
        self.z = None

    def params(self):
        return [self.model.keys]

    def forward_logits(self):
        return self.model(self.x, self.z)

    def eager(self, feats, labels, row_weight):
        return tip_step(self.model, feats, self._clip_logits, labels, row_weight, self.optimizer, return_logits=True)

    def __call__(self, feats, labels, row_weight, clip_logits):
        self._clip_logits = clip_logits
        if self.z is None or self.z.shape != clip_logits.shape:
            if self.graph is not None:      # another batch shape: the eager step (GraphedStep.__call__ sees the feature block's shape differ too)
                return super().__call__(feats, labels, row_weight)
            self.z = clip_logits.detach().float().clone()
        else:
            self.z.copy_(clip_logits)
        return super().__call__(feats, labels, row_weight)


def adapter_step(model, image_features, text_features, scale, labels, row_weight, optimizer, return_logits=False):
    """CLIP-Adapter step on a models.ClipAdapterModel: feature adapter over cached image features -> cosine head against the fixed text features of
    the trained prompt (constants of the step) -> weighted CE -> the gradients of w1 and w2 -> optimizer.  No tower runs.  Hard labels only (no soft
    targets)."""
    feats = model(image_features)
    logits = CosineHeadFn.apply(feats, text_features, scale)
    loss = WeightedCEFn.apply(logits, labels, row_weight)
    return _finish(loss, [model.w1, model.w2], optimizer, logits if return_logits else None)


class GraphedAdapterStep(GraphedStep):
    """adapter_step replayed from a HIP graph: the adapter's forward and backward, the cosine head's and the loss are a handful of kernels, so a
    step is launch cost and little else.  The static input is the feature block [B, embed_dim] (GraphedStep's `x`); the text features and the scale
    are constants of the object.  A batch of another shape runs the eager step."""

    def __init__(self, model, text_features, scale, optimizer):
        super().__init__(optimizer)
        self.model, self.scale = model, float(scale)
        self.text = text_features.detach().float().contiguous()

    def params(self):
        return [self.model.w1, self.model.w2]

    def forward_logits(self):
        return CosineHeadFn.apply(self.model(self.x), self.text, self.scale)

    def eager(self, feats, labels, row_weight):
        return adapter_step(self.model, feats, self.text, self.scale, labels, row_weight, self.optimizer, return_logits=True)
