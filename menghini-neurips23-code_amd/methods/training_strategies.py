"""Stand-in for the reference's MISSING `methods/*/training_strategies.py` (every strategy file does
`from .training_strategies import TrainingStrategy`, but the file is absent upstream: SURVEY.md 0.2).
The contract is reconstructed from the call sites and from `pseudo_iterative.py:62-125`
(GRIP schedule).  Everything that cannot be pinned from the snapshot is an explicit config knob with a
documented default: prompt-init seed (`OPTIM_SEED`), `MOMENTUM` (0), loader shuffle seed, best-epoch rule
(highest validation accuracy, first wins).  Training trajectories are therefore NOT claimed to match
upstream bit for bit; the per-step numerics are the parity-tested kernels.

One class covers the three prompt modalities (config.MODALITY in {"text", "image", "multi"}) and the three
learning paradigms (config.LEARNING_PARADIGM in {"ssl", "ul", "trzsl"}); the reference's eighteen strategy
classes are thin aliases of it (methods/strategies.py).
"""
import copy
import logging
import math

import numpy as np
import torch

from .. import clip, dist as gdist, pseudolabels as pl, steps
from ..engine import cosine_head, soft_ce
from ..models import ClipAdapterModel, CustomImageEncoder, CustomTextEncoder, GdaHeadModel, ImagePrefixModel, LinearProbeModel, MaPLeModel, TextPrefixModel, TipAdapterModel, UPTModel
from ..utils import pseudolabel_top_k

log = logging.getLogger(__name__)


def multi_view_from_config(config, keep=False):
    """The pl.MultiView of a config's MV_* settings (MV_VIEWS outside 2 .. 64 and bad boxes or parameters raise ValueError); keep: a frozen image tower,
    whose view embeddings may stay across passes up to MV_CACHE_BYTES (default 4 GiB)."""
    g = lambda name, default: getattr(config, name, default)
    return pl.MultiView(views=g("MV_VIEWS", 16), scale=tuple(g("MV_SCALE", (0.5, 1.0))), ratio=tuple(g("MV_RATIO", (3.0 / 4.0, 4.0 / 3.0))),
                        flip=float(g("MV_FLIP", 0.5)), seed=int(g("MV_SEED", 0)), rho=float(g("MV_RHO", 0.3)), lam=float(g("MV_LAMBDA", 4.0)),
                        lam_y=float(g("MV_LAMBDA_Y", 0.2)), outer=int(g("MV_OUTER", 5)), inner=int(g("MV_INNER", 3)),
                        keep_bytes=int(g("MV_CACHE_BYTES", 4 << 30)) if keep else 0)


def tpt_settings_from_config(config):
    """The keyword arguments of tpt.TestTimeTuner of a config's TPT_* settings; a bad value raises ValueError (the tuner's own checks, run here on a
    sampler and a targets object, so that a config fails when the strategy is built and not at the first prediction)."""
    from .. import tpt
    g = lambda name, default: getattr(config, name, default)
    kw = dict(views=g("TPT_VIEWS", 64), rho=float(g("TPT_RHO", 0.1)), lr=float(g("TPT_LR", 5e-3)), steps=g("TPT_STEPS", 1),
              scale=tuple(g("TPT_SCALE", (0.08, 1.0))), ratio=tuple(g("TPT_RATIO", (3.0 / 4.0, 4.0 / 3.0))), flip=float(g("TPT_FLIP", 0.5)),
              seed=int(g("TPT_SEED", 0)))
    tpt.TestTimeTuner(None, None, **kw)      # (validates; holds no device memory)
    return kw


def stream_cache_from_config(config):
    """The tda.StreamCache of a config's TDA_* settings (TDA_POS_CAP 3, TDA_NEG_CAP 2, TDA_POS_ALPHA 2.0, TDA_POS_BETA 5.0, TDA_NEG_ALPHA 0.117,
    TDA_NEG_BETA 1.0, TDA_NEG_ENTROPY (0.2, 0.5), TDA_NEG_MASK (0.03, 1.0): the paper's as recalled, untuned here); a bad value raises ValueError when
    the strategy is built."""
    from .. import tda
    g = lambda name, default: getattr(config, name, default)
    return tda.StreamCache(pos_cap=g("TDA_POS_CAP", 3), neg_cap=g("TDA_NEG_CAP", 2), pos_alpha=g("TDA_POS_ALPHA", 2.0), pos_beta=g("TDA_POS_BETA", 5.0),
                           neg_alpha=g("TDA_NEG_ALPHA", 0.117), neg_beta=g("TDA_NEG_BETA", 1.0), neg_entropy=g("TDA_NEG_ENTROPY", (0.2, 0.5)),
                           neg_mask=g("TDA_NEG_MASK", (0.03, 1.0)))


def make_scheduler(optimizer, config):
    """WarmupCosineSchedule stepped once per EPOCH (utils/schedulers.py:36-65 of the reference)."""
    warm, total = int(getattr(config, "WARMUP_EPOCHS", 0)), int(config.EPOCHS)

    def lr_lambda(step):
        if step < warm:
            return float(step) / float(max(1.0, warm))
        progress = float(step - warm) / float(max(1, total - warm))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda)


class TrainingStrategy:
    def __init__(self, config, label_to_idx, classes, seen_classes, unseen_classes, device, data_folder=None):
        self.config = config
        self.classes, self.seen_classes, self.unseen_classes = classes, seen_classes, unseen_classes
        self.label_to_idx = label_to_idx
        self.device = device
        self.data_folder = data_folder
        self.clip_model, self.transform = clip.load(config.VIS_ENCODER, device=device)
        self.template = config.PROMPT_TEMPLATE
        self.modality = config.MODALITY
        self.paradigm = getattr(config, "LEARNING_PARADIGM", "ssl")
        self.val_unseen_files = self.val_unseen_labs = None
        self.balance_param = 1.0
        self.check_unlabeled = set()
        # Textual strategies: the image tower carries no prompt and never changes, so the pool's screen embeddings and every row a refinement tower
        # re-encoded are the same bits in every pseudolabel pass (GRIP: 10 passes over one pool): kept for the strategy's lifetime
        # (`CACHE_POOL_FEATURES: False` restores the re-encode; POOL_CACHE_MAX_MB: the budget).  Visual and multimodal strategies encode the pool
        # with trained prompts: they have no cache.
        self.pool_cache = None
        if self.modality == "text" and getattr(config, "CACHE_POOL_FEATURES", True):
            self.pool_cache = pl.PoolFeatureCache(int(float(getattr(config, "POOL_CACHE_MAX_MB", pl.POOL_CACHE_MAX_BYTES >> 20)) * 2 ** 20))
        # TIP_ADAPTER (textual strategies): the key/value cache built from the training set after each prompt training (build_tip_cache); None = off
        self.tip, self.tip_classes, self.tip_losses, self.tip_search = None, None, [], None
        if bool(getattr(config, "TIP_ADAPTER", False)) and self.modality != "text":
            log.info(f"TIP_ADAPTER is ignored by the {self.modality} strategies: their pool features move with the prompt (textual strategies only)")
        # CLIP_ADAPTER (textual strategies): the feature adapter trained on the cached training features after each prompt training
        # (build_feature_adapter); None = off
        self.adapter, self.adapter_losses = None, []
        if bool(getattr(config, "CLIP_ADAPTER", False)) and self.modality != "text":
            log.info(f"CLIP_ADAPTER is ignored by the {self.modality} strategies: their image features move with the prompt (textual strategies only)")
        self.clip_adapter()      # (raises when CLIP_ADAPTER and TIP_ADAPTER are both set)
        # GDA_HEAD (textual strategies): the Gaussian discriminant head fitted to the cached training features after each prompt training
        # (build_gda_head); None = off
        self.gda, self.gda_classes, self.gda_search = None, None, None
        if bool(getattr(config, "GDA_HEAD", False)) and self.modality != "text":
            log.info(f"GDA_HEAD is ignored by the {self.modality} strategies: their image features move with the prompt (textual strategies only)")
        self.gda_head()          # (raises when GDA_HEAD is set together with TIP_ADAPTER or CLIP_ADAPTER)
        # LINEAR_PROBE (textual strategies): the linear classifier trained on the cached training features after each prompt training
        # (build_linear_probe); None = off
        self.probe, self.probe_classes, self.probe_search, self.probe_targets = None, None, None, None
        if bool(getattr(config, "LINEAR_PROBE", False)) and self.modality != "text":
            log.info(f"LINEAR_PROBE is ignored by the {self.modality} strategies: their image features move with the prompt (textual strategies only)")
        self.linear_probe()      # (raises when LINEAR_PROBE is set together with TIP_ADAPTER, CLIP_ADAPTER or GDA_HEAD)
        # LABEL_PROPAGATION (all modalities, default False): every pseudolabel pass propagates the head's probabilities over the pool's kNN graph
        # (LP_K 16, LP_ALPHA 0.8, LP_GAMMA 10, LP_ITERS 10: untuned).  Textual strategies keep the graph per pool -- their image tower is frozen, the graph
        # is an invariant of the run; visual and multimodal strategies rebuild it every pass: their features move with the prompt.
        self.label_prop = None
        if bool(getattr(config, "LABEL_PROPAGATION", False)):
            self.label_prop = pl.LabelPropagation(k=int(getattr(config, "LP_K", 16)), alpha=float(getattr(config, "LP_ALPHA", 0.8)),
                                                  gamma=float(getattr(config, "LP_GAMMA", 10.0)), iters=int(getattr(config, "LP_ITERS", 10)),
                                                  keep_graphs=self.modality == "text")
        # TRANSDUCTIVE_GMM (all modalities, default False): every pseudolabel pass fits one Gaussian per class to the pool's embeddings and scans the
        # graph-regularised assignments (pl.TransductiveGMM, after TransCLIP-ZS; GMM_K 3, GMM_LAMBDA 1.0, GMM_ITERS 10, GMM_Z_ITERS 5: untuned).  The graph is
        # kept or rebuilt as for LABEL_PROPAGATION.  `predict`, validation, the Tip cache and the adapter do not see it.
        self.gmm = None
        if bool(getattr(config, "TRANSDUCTIVE_GMM", False)):
            if self.label_prop is not None:
                raise ValueError("TRANSDUCTIVE_GMM and LABEL_PROPAGATION are two different transductions of the same pool: set one of them")
            self.gmm = pl.TransductiveGMM(k=int(getattr(config, "GMM_K", 3)), lam=float(getattr(config, "GMM_LAMBDA", 1.0)),
                                          iters=int(getattr(config, "GMM_ITERS", 10)), z_iters=int(getattr(config, "GMM_Z_ITERS", 5)),
                                          keep_graphs=self.modality == "text")
        # BALANCED_PSEUDOLABELS (all modalities, default False): every pseudolabel pass balances its [n, c] matrix -- the head's probabilities, or the Z
        # of LABEL_PROPAGATION / TRANSDUCTIVE_GMM when one of them is on -- towards a class prior with Sinkhorn-Knopp before the leaderboard scan
        # (pl.BalancedAssignment; OT_TAU 1.0, OT_ITERS 3, OT_PRIOR None = uniform, else a list of c weights: untuned).  `predict`, validation, the Tip
        # cache and the adapter do not see it.
        self.balanced = None
        if bool(getattr(config, "BALANCED_PSEUDOLABELS", False)):
            self.balanced = pl.BalancedAssignment(tau=float(getattr(config, "OT_TAU", 1.0)), iters=int(getattr(config, "OT_ITERS", 3)),
                                                  prior=getattr(config, "OT_PRIOR", None), inner=self.label_prop if self.label_prop is not None else self.gmm)
        # SOFT_PSEUDOLABELS (all modalities, default False; SOFT_TEMPERATURE 1.0: untuned): every pseudolabelled row of a prompt step trains on its
        # sharpened row of the matrix the pass ranked (Z or Q; pl.SoftTargetStore -> engine.soft_ce) instead of the one-hot of its pseudolabel; labelled
        # rows keep their one-hot.  It needs one of the three transductions above: the per-image pass has no device matrix to offer.  LABEL_SMOOTHING
        # (default 0.0) smooths every row's target and works on its own.  row_weights, the epoch accuracy, the held-out pseudolabel validation, `predict`,
        # the Tip cache and the adapter (hard labels) do not see either.
        self.soft_store, self.soft_temperature = None, float(getattr(config, "SOFT_TEMPERATURE", 1.0))
        self.label_smoothing = float(getattr(config, "LABEL_SMOOTHING", 0.0))
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"LABEL_SMOOTHING: {self.label_smoothing} (0 <= LABEL_SMOOTHING < 1)")
        if bool(getattr(config, "SOFT_PSEUDOLABELS", False)):
            if self.transduction() is None:
                raise ValueError("SOFT_PSEUDOLABELS needs LABEL_PROPAGATION, TRANSDUCTIVE_GMM or BALANCED_PSEUDOLABELS: only a transduced pass keeps the "
                                 "matrix it ranked on the device")
            if not 0.0 < self.soft_temperature < float("inf"):
                raise ValueError(f"SOFT_TEMPERATURE: {self.soft_temperature} (a finite temperature > 0)")
            self.soft_store = pl.SoftTargetStore()
        # CANDIDATE_PSEUDOLABELS (all modalities and paradigms, default False; CPL_TAU 0.99, CPL_SLOTS 2, CPL_COMBINE "intersection": untuned): every
        # pseudolabel pass keeps a SET of classes per pool image instead of one label (pl.CandidateSelection -> engine.candidate_select, on the matrix
        # the pass would have ranked: Z / Q of the transductions above, else the head's probabilities; each class claims CPL_SLOTS x N_PSEUDOSHOTS rows)
        # and every pseudolabelled row of a prompt step trains on -log sum_{c in S} p_c (pl.CandidateStore -> engine.candidate_ce); labelled rows keep
        # their one-hot.  The training list is every pool row with a non-empty set, once, labelled with the set's first member: row_weights, the epoch
        # accuracy, the held-out pseudolabel validation, `predict`, the Tip cache, the adapter, GDA and the probe see that hard label.  Fixed soft rows
        # and smoothing are other targets for the same rows: not composed.
        self.candidate_selection = self.candidate_store = None
        if bool(getattr(config, "CANDIDATE_PSEUDOLABELS", False)):
            if bool(getattr(config, "SOFT_PSEUDOLABELS", False)) or self.label_smoothing > 0.0:
                raise ValueError("CANDIDATE_PSEUDOLABELS trains the pseudolabelled rows on candidate sets: SOFT_PSEUDOLABELS and LABEL_SMOOTHING > 0 give "
                                 "the same rows other targets (these compositions are not built): set one of them")
            self.candidate_selection = pl.CandidateSelection(tau=float(getattr(config, "CPL_TAU", 0.99)), slots=getattr(config, "CPL_SLOTS", 2),
                                                             combine=getattr(config, "CPL_COMBINE", "intersection"))
            self.candidate_store = pl.CandidateStore()
        # MULTIVIEW_PSEUDOLABELS (all modalities and paradigms, default False; MV_VIEWS 16, MV_SCALE (0.5, 1.0), MV_RATIO (3/4, 4/3), MV_FLIP 0.5,
        # MV_SEED 0, MV_RHO 0.3, MV_LAMBDA 4, MV_LAMBDA_Y 0.2: the paper's; MV_OUTER 5, MV_INNER 3: untuned): every pseudolabel pass encodes MV_VIEWS views
        # of every pool image under the current prompts and hands the mean-shift mode of their embeddings (pl.MultiView -> engine.view_mode) to the head,
        # the transductions, the balance, the soft rows and the candidate sets in place of the single embedding.  V tower forwards per image.  A textual
        # strategy (frozen tower) keeps a pool's view embeddings across iterations when they fit MV_CACHE_BYTES (default 4 GiB); the others encode every
        # pass.  MV_PREDICT (default False): `predict`, and so validation and test, classify the mode of each item's views; adapter, Tip, GDA and probe
        # terms then apply to the mode.  The training sets of those heads stay single-view.
        self.multi_view, self.mv_predict = None, bool(getattr(config, "MV_PREDICT", False))
        if bool(getattr(config, "MULTIVIEW_PSEUDOLABELS", False)) or self.mv_predict:
            self.multi_view = multi_view_from_config(config, keep=self.modality == "text")
        self.mv_passes = self.multi_view if bool(getattr(config, "MULTIVIEW_PSEUDOLABELS", False)) else None      # what the passes install
        # TPT (textual strategies, default False; TPT_VIEWS 64, TPT_RHO 0.1, TPT_LR 5e-3, TPT_STEPS 1, TPT_SCALE (0.08, 1), TPT_RATIO (3/4, 4/3), TPT_FLIP 0.5:
        # the paper's; TPT_SEED 0, TPT_VALIDATION False: untuned): `predict` -- and so test_predictions and evaluation -- classifies every item with a
        # context tuned to it for the time of its prediction (tpt.TestTimeTuner: TPT_VIEWS views of the item through the frozen image tower, one
        # episode of TPT_STEPS AdamW steps on the entropy of the mean prediction of its confident views, the row of view 0 under the tuned context);
        # Tip, GDA and probe terms are added to that row from view 0's features as today.  The validation inside `train` runs every epoch and keeps
        # the plain path unless TPT_VALIDATION is set.  The pseudolabel passes are untouched.  Visual and multimodal strategies ignore the switch:
        # their image features move with the prompt, and an episode would be TPT_VIEWS tower backward passes.
        self.tpt_settings, self._tpt, self._tpt_plain = None, None, False
        if bool(getattr(config, "TPT", False)):
            if self.modality != "text":
                log.info(f"TPT is ignored by the {self.modality} strategies: their image features move with the prompt (textual strategies only)")
            else:
                if self.mv_predict:
                    raise ValueError("TPT and MV_PREDICT are two answers to the same question (how to classify an item from its views): set one of them")
                if bool(getattr(config, "CLIP_ADAPTER", False)):
                    raise ValueError("TPT and CLIP_ADAPTER: an episode would have to adapt the view features (this composition is not built): set one of them")
                self.tpt_settings = tpt_settings_from_config(config)
        # TDA (all modalities and paradigms, default False; the TDA_* settings of stream_cache_from_config; TDA_VALIDATION False): `predict` -- and so
        # test_predictions and evaluation -- runs the items' logits and image features, gathered in dataset order, through a test-time streaming cache
        # (tda.StreamCache: per-class queues of the lowest-entropy items seen so far, every item scored against the queues of its moment).  No tower
        # pass: it sees only what the heads produced, so it composes with Tip, GDA, probe, adapter, MV_PREDICT and TPT.  Every rank runs the same
        # stream over the whole gathered set.  The validation inside `train` keeps the plain path unless TDA_VALIDATION is set.  The pseudolabel
        # passes are untouched.
        self.tda, self._tda_plain = None, False
        if bool(getattr(config, "TDA", False)):
            self.tda = stream_cache_from_config(config)
        self.declare_custom_encoder()
        self.initialize_prompts_parameters()

    def transduction(self):
        """What the pseudolabel passes install with pl.label_propagation(): the BalancedAssignment (which wraps the LabelPropagation or the
        TransductiveGMM when one is on), else the LabelPropagation, the TransductiveGMM, or None."""
        if self.balanced is not None:
            return self.balanced
        return self.label_prop if self.label_prop is not None else self.gmm

    @property
    def gmm_state(self):
        """(mean [c, e], var [e]) of the most recent TRANSDUCTIVE_GMM pass (None before the first, or with the switch off): the class Gaussians of
        the pool, which can score images that were not in it."""
        return None if self.gmm is None else self.gmm.state

    # ------------------------------------------------------------------ encoders / prompts / model
    def declare_custom_encoder(self):
        self.image_encoder = CustomImageEncoder(self.clip_model.visual) if self.modality in ("image", "multi") else None
        self.text_encoder = CustomTextEncoder(self.clip_model, self.device, torch.float32) if self.modality in ("text", "multi") else None

    def initialize_prompts_parameters(self):
        c = self.config
        g = torch.Generator().manual_seed(int(getattr(c, "OPTIM_SEED", 0)))
        mean, std = float(getattr(c, "MEAN_INIT", 0.0)), float(getattr(c, "VAR_INIT", 0.02))
        d = self.clip_model.dims

        def init(*shape):
            if getattr(c, "VIS_PREFIX_INIT", "normal") == "uniform":
                return (torch.rand(*shape, generator=g) * 2 - 1) * std + mean
            return torch.randn(*shape, generator=g) * std + mean
        if self.modality == "text":
            self.initial_prefix = init(1, int(c.PREFIX_SIZE), d.transformer_width)
            # COOP_DEEP: deep contexts for blocks 1 .. layers - 1, drawn after the shallow context (which stays bit-identical with and without them)
            self.initial_deep_prefix = init(d.transformer_layers - 1, int(c.PREFIX_SIZE), d.transformer_width) if self.coop_deep() else None
        elif self.modality == "image":
            self.initial_prefix = init(int(c.PREFIX_SIZE), d.vision_width)
            # VPT_DEEP: deep prompts for blocks 1 .. layers - 1, drawn after the shallow prompt (which stays bit-identical with and without them)
            self.initial_deep_prefix = init(d.vision_layers - 1, int(c.PREFIX_SIZE), d.vision_width) if self.vpt_deep() else None
        else:
            self.coop_init = init(1, int(c.TEXT_PREFIX_SIZE), d.transformer_width)
            self.vpt_init = init(1, int(c.VISION_PREFIX_SIZE), d.vision_width)
            # UPT_DEEP: vpt_embeddings_deep for blocks 1 .. layers - 1, drawn after the two prompts (which stay bit-identical with and without it)
            self.vpt_deep_init = init(d.vision_layers - 1, int(c.VISION_PREFIX_SIZE), d.vision_width) if self.upt_deep() else None
            # MAPLE: the deep text prompts of blocks 1 .. MAPLE_DEPTH, drawn after the two prompts (which stay bit-identical with and without it);
            # the visual side is coupled to them (MaPLeModel), so vpt_init is drawn but not trained
            self.maple_deep_init = None
            if self.maple():
                if self.upt_deep():
                    raise ValueError("MAPLE and UPT_DEEP are two different deep multimodal models: set one of them")
                if int(c.TEXT_PREFIX_SIZE) != int(c.VISION_PREFIX_SIZE):
                    raise ValueError(f"MAPLE couples the visual prompt to the text prompt token by token: TEXT_PREFIX_SIZE ({c.TEXT_PREFIX_SIZE}) must "
                                     f"equal VISION_PREFIX_SIZE ({c.VISION_PREFIX_SIZE})")
                most = min(d.transformer_layers, d.vision_layers) - 1
                depth = int(getattr(c, "MAPLE_DEPTH", most))
                if not 0 <= depth <= most:
                    raise ValueError(f"MAPLE_DEPTH = {depth}: 0 .. {most} deep prompts (min(text layers, vision layers) - 1)")
                self.maple_deep_init = init(depth, int(c.TEXT_PREFIX_SIZE), d.transformer_width) if depth else None

    def vpt_deep(self):
        """Deep visual prompts (VPT-Deep) for the visual strategies: config VPT_DEEP, default False.  The multimodal strategies ignore it, as the
        reference does (its UPT computes vpt_embeddings_deep and discards it); they have UPT_DEEP."""
        return self.modality == "image" and bool(getattr(self.config, "VPT_DEEP", False))

    def coop_deep(self):
        """Deep text prompts (deep CoOp) for the textual strategies: config COOP_DEEP, default False.  The visual strategies have no trainable text
        side and the multimodal ones keep UPT's single mixed context: both ignore it."""
        return self.modality == "text" and bool(getattr(self.config, "COOP_DEEP", False))

    def upt_deep(self):
        """Deep UPT for the multimodal strategies: config UPT_DEEP, default False.  UPTModel(mix_deep=True) mixes vpt_embeddings_deep with the
        prompts and feeds its outputs to the image tower as deep prompts."""
        return self.modality == "multi" and bool(getattr(self.config, "UPT_DEEP", False))

    def maple(self):
        """Coupled deep multimodal prompts (MaPLe) for the multimodal strategies: config MAPLE, default False (optional MAPLE_DEPTH, default
        min(text layers, vision layers) - 1).  MaPLeModel replaces UPTModel: deep text prompts, each visual prompt a trainable Linear of the text
        prompt of its depth.  Textual and visual strategies ignore it."""
        return self.modality == "multi" and bool(getattr(self.config, "MAPLE", False))

    def tip_adapter(self):
        """Tip-Adapter cache head for the textual strategies: config TIP_ADAPTER, default False (TIP_ALPHA 1.0, TIP_BETA 5.5, TIP_PSEUDO_WEIGHT 1.0,
        TIP_FINETUNE_EPOCHS 0 = training-free, TIP_LR 1e-3, TIP_SEARCH False).  Their image tower is frozen and their training features are cached, so
        the cache costs no tower pass.  Visual and multimodal strategies ignore it, as they ignore COOP_DEEP."""
        return self.modality == "text" and bool(getattr(self.config, "TIP_ADAPTER", False))

    def clip_adapter(self):
        """CLIP-Adapter feature head for the textual strategies: config CLIP_ADAPTER, default False (ADAPTER_RATIO 0.2, ADAPTER_REDUCTION 4,
        ADAPTER_EPOCHS 20, ADAPTER_LR 1e-3).  Their image tower is frozen and their training features are cached, so the adapter trains without a
        tower pass.  Visual and multimodal strategies ignore it, as they ignore TIP_ADAPTER.  Together with TIP_ADAPTER it is refused: they are two
        different heads on the same features, and stacking them is not defined here."""
        on = self.modality == "text" and bool(getattr(self.config, "CLIP_ADAPTER", False))
        if on and bool(getattr(self.config, "TIP_ADAPTER", False)):
            raise ValueError("CLIP_ADAPTER and TIP_ADAPTER are two different heads on the same image features: set one of them")
        return on

    def gda_head(self):
        """Gaussian discriminant head for the textual strategies: config GDA_HEAD, default False (GDA_ALPHA 1.0, GDA_SHRINK 1.0, GDA_PSEUDO_WEIGHT 1.0,
        GDA_SEARCH False, GDA_ALPHA_GRID (0.1, 0.3, 1, 3, 10): untuned).  Their image tower is frozen and their training features are cached, so the
        head costs no tower pass and no training.  Visual and multimodal strategies ignore it, as they ignore TIP_ADAPTER.  Together with
        TIP_ADAPTER or CLIP_ADAPTER it is refused: they are different heads on the same features, and stacking them is not defined here."""
        on = self.modality == "text" and bool(getattr(self.config, "GDA_HEAD", False))
        if on and (bool(getattr(self.config, "TIP_ADAPTER", False)) or bool(getattr(self.config, "CLIP_ADAPTER", False))):
            raise ValueError("GDA_HEAD, TIP_ADAPTER and CLIP_ADAPTER are different heads on the same image features: set one of them")
        return on

    def linear_probe(self):
        """Trained linear probe for the textual strategies: config LINEAR_PROBE, default False (PROBE_ITERS 300, PROBE_MOMENTUM 0.9, PROBE_L2 0.1,
        PROBE_ALPHA 1.0, PROBE_PSEUDO_WEIGHT 1.0, PROBE_SEARCH False, PROBE_ALPHA_GRID (0.1, 0.3, 1, 3, 10), PROBE_INIT "zero" or "gda" -- which reads
        GDA_SHRINK: untuned).  Their image tower is frozen and their training features are cached, so the probe trains without a tower pass.  Visual
        and multimodal strategies ignore it, as they ignore GDA_HEAD.  Together with TIP_ADAPTER, CLIP_ADAPTER or GDA_HEAD it is refused: they are
        different heads on the same features, and stacking them is not defined here."""
        on = self.modality == "text" and bool(getattr(self.config, "LINEAR_PROBE", False))
        others = [k for k in ("TIP_ADAPTER", "CLIP_ADAPTER", "GDA_HEAD") if bool(getattr(self.config, k, False))]
        if on and others:
            raise ValueError(f"LINEAR_PROBE and {' and '.join(others)} are different heads on the same image features: set one of them")
        if on and str(getattr(self.config, "PROBE_INIT", "zero")) not in ("zero", "gda"):
            raise ValueError(f"PROBE_INIT: {getattr(self.config, 'PROBE_INIT')!r} (\"zero\" or \"gda\")")
        return on

    def define_model(self, classes=None):
        c, dev = self.config, self.device
        self.tip = None      # a cache belongs to the prompt it was built after: validation during the next training sees CLIP logits alone
        self.adapter = None  # and so does a feature adapter
        self.gda = None      # and a discriminant head
        self.probe = None    # and a trained linear probe
        classes = classes if classes is not None else self.classes
        if self.modality == "text":
            deep = getattr(self, "initial_deep_prefix", None)
            self.model = TextPrefixModel(self.initial_prefix.clone().to(dev), self.text_encoder, classes, device=dev,
                                         deep_prefix=None if deep is None else deep.clone().to(dev))
        elif self.modality == "image":
            deep = getattr(self, "initial_deep_prefix", None)
            self.model = ImagePrefixModel(self.initial_prefix.clone().to(dev), self.image_encoder, device=dev,
                                          deep_prefix=None if deep is None else deep.clone().to(dev))
        elif self.maple():
            torch.manual_seed(int(getattr(c, "OPTIM_SEED", 0)))      # the coupling Linears' initialisation
            deep = self.maple_deep_init
            self.model = MaPLeModel(self.coop_init.clone().to(dev), None if deep is None else deep.clone().to(dev), self.image_encoder, self.text_encoder,
                                    classes, device=dev, dtype=torch.float32)
        else:
            torch.manual_seed(int(getattr(c, "OPTIM_SEED", 0)))
            deep = getattr(self, "vpt_deep_init", None)
            self.model = UPTModel(self.coop_init.clone().to(dev), self.vpt_init.clone().to(dev), None if deep is None else deep.clone().to(dev),
                                  self.image_encoder, self.text_encoder, classes, int(getattr(c, "TRANSFORMER_DIM", 128)), device=dev,
                                  dtype=torch.float32, mix_deep=deep is not None)
        params = [p for p in self.model.parameters() if p.requires_grad]
        self.optimizer = torch.optim.SGD(params, lr=float(c.LR), weight_decay=float(c.DECAY), momentum=float(getattr(c, "MOMENTUM", 0.0)))
        self.scheduler = make_scheduler(self.optimizer, c)
        self.loss_func = torch.nn.CrossEntropyLoss()
        self._model_gen = getattr(self, "_model_gen", 0) + 1       # a new model / optimizer: captured step graphs of the old one are stale

    def unwrap_model(self):
        return self.model

    def training_model(self, img):
        return self.model(img)

    def backpropagate(self):
        self.optimizer.step()
        self.optimizer.zero_grad()

    def update_scheduler(self):
        self.scheduler.step()

    def prompt_snapshot(self):
        m = self.unwrap_model()
        if self.modality in ("text", "image") and getattr(m, "deep_prefix", None) is not None:      # VPT-Deep / deep CoOp
            return [m.prefix.detach().cpu().numpy(), m.deep_prefix.detach().cpu().numpy()]
        if self.modality in ("text", "image"):
            return [m.prefix.detach().cpu().numpy()]
        if self.maple():      # [ctx, compound_prompts_text (None for depth 0), proj_weight, proj_bias]
            return [None if p is None else p.detach().cpu().numpy() for p in (m.ctx, m.compound_prompts_text, m.proj_weight, m.proj_bias)]
        # multimodal_prompt.py:149-158 of the reference: the eight trainable pieces, positionally -- NOT the whole UPTModel
        # state_dict, which would drag ~1 GB of frozen CLIP weights (registered sub-modules) to the host every epoch.
        sd = lambda mod: copy.deepcopy({k: v.detach().cpu() for k, v in mod.state_dict().items()})   # noqa: E731
        return [sd(m.transformer), sd(m.proj_coop_pre), sd(m.proj_coop_post), sd(m.proj_vpt_pre), sd(m.proj_vpt_post),
                m.coop_embeddings.detach().cpu().numpy(),
                None if m.vpt_embeddings_deep is None else m.vpt_embeddings_deep.detach().cpu().numpy(),
                m.vpt_embeddings.detach().cpu().numpy()]

    # ------------------------------------------------------------------ features
    def text_prompts(self, classes):
        return [self.template.format(" ".join(i.split("_"))) for i in classes]

    @torch.no_grad()
    def fixed_text_features(self, classes):
        return self.clip_model.encode_text(clip.tokenize(self.text_prompts(classes)).to(self.device))

    def scale(self):
        return self.clip_model.logit_scale.exp().item()

    def frozen_image_features(self, images, names=None):
        """Features of the FROZEN image tower.  Textual strategies re-encode the same images every epoch upstream
        (e.g. textual_prompt.py:100: 150 epochs x the same shots); the tower is deterministic and row-independent, so the
        features are cached per file name (`CACHE_FROZEN_FEATURES: False` restores the re-encode)."""
        if names is None or not getattr(self.config, "CACHE_FROZEN_FEATURES", True):
            with torch.no_grad():
                return self.clip_model.encode_image(images)
        cache = self.__dict__.setdefault("_frozen_cache", {})
        miss = [i for i, n in enumerate(names) if n not in cache]
        if miss:
            with torch.no_grad():
                f = self.clip_model.encode_image(images[miss])
            for j, i in enumerate(miss):
                cache[names[i]] = f[j]
        return torch.stack([cache[n] for n in names])

    def features(self, images, classes, names=None):
        """(image_features, text_features) of the CURRENT model, autograd-ready where prompts are involved."""
        if self.modality == "text":
            self.model.classes = classes
            return self.frozen_image_features(images, names), self.model(classes)
        if self.modality == "image":
            return self.model(images), self.fixed_text_features(classes)
        self.model.classes = classes
        txt, img = self.model(images, classes)
        return img, txt

    # ------------------------------------------------------------------ datasets
    def create_training_dataset(self, train_data, unlabeled_data=None):
        """Plain strategies train on the labeled seen data as is; FPL strategies (subclass hook `fpl`)
        add CLIP pseudolabels for the unlabeled pool (e.g. textual_fpl.py:51-121 of each paradigm)."""
        if not getattr(self, "fpl", False) or unlabeled_data is None:
            return train_data
        c = self.config
        pseudo_classes = self.classes if self.paradigm in ("ssl", "ul") else self.unseen_classes
        # the frozen-CLIP pass runs the same towers over the same pool as the trained-prompt passes after it
        with pl.pool_cache(self.pool_cache), pl.label_propagation(self.transduction()), pl.soft_targets(self.soft_store), \
                pl.candidate_sets(self.candidate_selection, self.candidate_store), pl.multi_view(self.mv_passes):
            pseudolabel_top_k(c, c.DATASET_NAME, int(c.N_PSEUDOSHOTS), self.template, unlabeled_data, pseudo_classes, self.transform,
                              self.clip_model, self.label_to_idx, self.device, c.VIS_ENCODER, getattr(c, "SPLIT_SEED", 0))
        return self.merge_pseudolabels(train_data, unlabeled_data)

    def merge_pseudolabels(self, train_data, unlabeled_data):
        c = self.config
        unseen_imgs, unseen_labs = list(unlabeled_data.filepaths), [int(l) for l in unlabeled_data.labels]
        if int(c.N_PSEUDOSHOTS) >= 10:     # hold out part of the pseudolabels for validation (textual_fpl.py:84-103)
            np.random.seed(int(getattr(c, "validation_seed", 0)))
            tr = np.random.choice(range(len(unseen_imgs)), size=int(len(unseen_imgs) * float(c.ratio_train_val)), replace=False)
            va = sorted(set(range(len(unseen_imgs))).difference(set(tr.tolist())))
            self.val_unseen_files = [unseen_imgs[i] for i in va]
            self.val_unseen_labs = [unseen_labs[i] for i in va]
            unseen_imgs, unseen_labs = [unseen_imgs[i] for i in tr], [unseen_labs[i] for i in tr]
        else:
            self.val_unseen_files = self.val_unseen_labs = None
        self.check_unlabeled = set(p.split("/")[-1] for p in unseen_imgs)
        if self.paradigm == "ul":
            train_data.filepaths, train_data.labels = unseen_imgs, unseen_labs
            self.balance_param = 1.0
        else:
            seen_imgs = list(train_data.filepaths)
            seen_labs = [l if train_data.label_id else self.label_to_idx[l] for l in train_data.labels]
            n_u, n_s = max(len(unseen_imgs), 1), max(len(seen_imgs), 1)
            # ssl: |unseen| / |seen| (semi_supervised_learning/textual_fpl.py:115, visual_fpl.py:110), trzsl: |seen| / |unseen|
            # (transductive_zsl/textual_fpl.py:109, visual_fpl.py:105); the multimodal strategies take the square root in both
            # paradigms (semi_supervised_learning/multimodal_fpl.py:107, transductive_zsl/multimodal_fpl.py:104)
            ratio = n_u / n_s if self.paradigm == "ssl" else n_s / n_u
            self.balance_param = math.sqrt(ratio) if self.modality == "multi" else ratio
            train_data.filepaths, train_data.labels = unseen_imgs + seen_imgs, unseen_labs + seen_labs
        train_data.label_id = True
        return train_data

    def row_weights(self, labels, names):
        """FPL loss as per-row weights (steps.fpl_row_weights); plain strategies use the mean CE."""
        if not getattr(self, "fpl", False) or self.paradigm == "ul":
            return steps.fpl_row_weights([False] * len(labels))
        if self.paradigm == "ssl":     # membership by file name (textual_fpl.py:123-165)
            return steps.fpl_row_weights([n in self.check_unlabeled for n in names], gamma_seen=self.balance_param, gamma_pseudo=1.0)
        unseen_ids = {self.label_to_idx[c] for c in self.unseen_classes}   # membership by label id (transductive_zsl/textual_fpl.py:117-147)
        return steps.fpl_row_weights([int(l) in unseen_ids for l in labels], gamma_seen=1.0, gamma_pseudo=self.balance_param)

    def soft_targets(self, classes, only_seen=False):
        """The steps.SoftTargets (or, with CANDIDATE_PSEUDOLABELS, the steps.CandidateTargets) of an epoch over `classes`, or None (every switch absent:
        the steps call WeightedCEFn exactly as before).  The matrix
        is the one the last pseudolabel pass recorded (SOFT_PSEUDOLABELS; none for only_seen training, which has no pseudolabelled rows, and before a
        pass has recorded one); LABEL_SMOOTHING alone gives a SoftTargets without a matrix."""
        cand = None if only_seen else self.candidate_store
        if cand is not None and cand.mask is not None:      # (CANDIDATE_PSEUDOLABELS: the sets of the last pass; excludes the two switches below)
            return steps.CandidateTargets(cand.mask, cand.col_map([self.label_to_idx[c] for c in classes]))
        store = None if only_seen else self.soft_store
        if store is not None and store.matrix is not None:
            ids = [self.label_to_idx[c] for c in classes]
            return steps.SoftTargets(store.matrix, store.col_map(ids), self.soft_temperature, self.label_smoothing)
        return steps.SoftTargets(smoothing=self.label_smoothing) if self.label_smoothing > 0.0 else None

    def soft_rows(self, soft, labels, names):
        """int32 [B] on the device: the matrix row of every PSEUDOLABELLED row of the batch -- membership as row_weights decides it: by file name in
        check_unlabeled (ssl, ul), by an unseen label id (trzsl) -- and -1 for the labelled rows, which keep their one-hot.  None without a matrix."""
        if soft is None or soft.matrix is None:
            return None
        if self.paradigm == "trzsl":
            unseen_ids = {self.label_to_idx[c] for c in self.unseen_classes}
            pseudo = [int(l) in unseen_ids for l in labels]
        else:
            pseudo = [n in self.check_unlabeled for n in names]
        store = self.candidate_store if isinstance(soft, steps.CandidateTargets) else self.soft_store
        return store.rows(list(names), hard=[not p for p in pseudo])      # (built on the host, one upload: no synchronisation)

    # ------------------------------------------------------------------ loops
    def _loader(self, data, shuffle):
        """Data-parallel like the reference under `accelerate launch` (methods_config/accelerate_config.yml: MULTI_GPU): every rank gets its OWN
        batches of BATCH_SIZE -- batch j of the epoch's order goes to rank j % world_size, the tail is padded with samples from the start
        (dist.rank_batches = accelerate's BatchSamplerShard; `accelerator.prepare(loader)`, e.g. textual_prompt.py:239) -- so N ranks take one
        optimizer step on N x BATCH_SIZE samples with the gradients averaged (DDP behind accelerator.backward, :131).  The shuffle seed is the same
        on every rank (`LOADER_SEED`, default 0: unpinnable upstream)."""
        seed = int(getattr(self.config, "LOADER_SEED", 0))
        sampler = gdist.RankBatchSampler(len(data), int(self.config.BATCH_SIZE), shuffle, seed=seed)
        # (the loader gets its own generator: without one every iter(loader) draws a base seed from the GLOBAL torch RNG, which would shift the stream
        # the prompt re-initialisations of the GRIP iterations read -- ADVICE r5)
        return torch.utils.data.DataLoader(data, batch_sampler=sampler, generator=torch.Generator().manual_seed(seed + 1))

    def _class_space(self, only_seen):
        classes = self.seen_classes if only_seen else self.classes
        idx = torch.tensor([self.label_to_idx[c] for c in classes], device=self.device)
        lut = torch.full((int(idx.max()) + 1,), -1, dtype=torch.long, device=self.device)
        lut[idx] = torch.arange(len(classes), device=self.device)
        return classes, idx, lut

    def _graphed_step(self, classes, soft=None):
        """The HIP-graph replay of this strategy's prompt step (steps.Graphed*Step) for the current model and class list; rebuilt
        whenever define_model made a new model / optimizer, or the soft targets' key moved (another matrix buffer, temperature or smoothing)."""
        key = (self._model_gen, tuple(classes)) if soft is None else (self._model_gen, tuple(classes), soft.key())
        if getattr(self, "_gkey", None) != key:
            kw = {} if soft is None else {"soft": soft}
            if self.modality == "text":
                self.model.classes = classes
                g = steps.GraphedCoopFeatureStep(self.model, self.clip_model, self.optimizer, **kw)
            elif self.modality == "image":
                g = steps.GraphedVptStep(self.model, self.fixed_text_features(classes), self.scale(), self.optimizer, **kw)
            else:
                self.model.classes = classes
                g = steps.GraphedUptStep(self.model, self.scale(), self.optimizer, **kw)
            self._gkey, self._gstep = key, g
        return self._gstep

    def view_sampler(self):
        """The train-time augmentation of the prompt steps (config AUGMENT, default False; "rrc_flip" = RandomResizedCrop + RandomHorizontalFlip, the
        training transform CoOp, VPT, MaPLe and Tip-Adapter-F are published with): a grip_amd.augment.ViewSampler with AUG_SCALE (0.08, 1.0),
        AUG_RATIO (3/4, 4/3), AUG_FLIP 0.5 and AUG_SEED 0, or None.  Only the batches of `_train_epoch` are augmented: validation, predict, evaluation,
        the Tip-Adapter cache build and every pseudolabel pass read the pool as it is."""
        c = self.config
        mode = getattr(c, "AUGMENT", False)
        if not mode:
            return None
        if mode != "rrc_flip":
            raise ValueError(f"AUGMENT: {mode!r} is not a known augmentation (False or 'rrc_flip')")
        from ..augment import ViewSampler
        return ViewSampler(seed=int(getattr(c, "AUG_SEED", 0)), scale=tuple(getattr(c, "AUG_SCALE", (0.08, 1.0))),
                           ratio=tuple(getattr(c, "AUG_RATIO", (3.0 / 4.0, 4.0 / 3.0))), flip=float(getattr(c, "AUG_FLIP", 0.5)))

    def _train_epoch(self, train_loader, only_seen=False, epoch=0):
        """One epoch of the strategy's prompt step (the `_train_epoch` bodies of the reference, e.g. textual_prompt.py:63-159).
        Default: every full-sized batch replays the step's forward + backward from a HIP graph (steps.Graphed*Step; a batch of
        another shape -- the ragged last one -- runs the same kernels eagerly), the textual modality encodes the frozen image
        tower `IMAGE_LOOKAHEAD` (51) batches at a time when its features are not cached, and loss / accuracy accumulate on the
        device: one host synchronisation per epoch instead of three per batch.  `GRAPH_STEPS: False` or gradient accumulation
        (ACCUMULATION_ITER > 1) take the eager per-batch path.

        With AUGMENT on, every batch's `img` (what the reference trains on) is replaced on the device by its view of `epoch` (view_sampler: one
        launch per batch, outside the graph -- the graphed steps copy their batch into a static buffer).  The frozen features of a textual
        strategy then change every epoch: the name-keyed cache is neither read nor filled, the look-ahead encode runs instead."""
        classes, ids, lut = self._class_space(only_seen)
        if self.modality in ("text", "multi"):
            # features() / predict() / trained_features() re-point model.classes at their own class list between epochs; the eager fallback of a
            # graphed step (ragged last batch) reads it at call time, so it is re-set here every epoch, not only when the graph is (re)built
            self.model.classes = classes
        accum = int(getattr(self.config, "ACCUMULATION_ITER", 1))
        aug = self.view_sampler()
        soft = self.soft_targets(classes, only_seen)
        if accum != 1 or not getattr(self.config, "GRAPH_STEPS", True):
            return self._train_epoch_eager(train_loader, classes, ids, lut, accum, aug, epoch, soft)
        g = self._graphed_step(classes, soft)
        total = torch.zeros((), dtype=torch.float64, device=self.device)      # the sum the eager loop forms in Python doubles
        correct = torch.zeros((), dtype=torch.int64, device=self.device)
        count = 0

        def batches():
            for img, _, _, label, names in train_loader:
                w = self.row_weights(label.tolist(), names)          # labels are still on the host here: no synchronisation
                img = img.to(self.device, non_blocking=True)
                if aug is not None:
                    img = aug.batch(img.contiguous(), names, epoch)
                rows = self.soft_rows(soft, label.tolist(), names)   # (None without a soft-target matrix)
                yield img, label.to(self.device, non_blocking=True), w.to(self.device, non_blocking=True), list(names), rows

        if self.modality == "text":
            if aug is None and getattr(self.config, "CACHE_FROZEN_FEATURES", True):
                stream = ((self.frozen_image_features(img, names), label, w, rows) for img, label, w, names, rows in batches())
            else:           # every image is encoded every time it is used, a group of batches per frozen-tower forward
                stream = steps.lookahead_image_features(self.clip_model, ((img, label, w, rows) for img, label, w, _, rows in batches()),
                                                        int(getattr(self.config, "IMAGE_LOOKAHEAD", 51)))
        else:
            stream = ((img, label, w, rows) for img, label, w, _, rows in batches())
        for x, label, w, rows in stream:
            total += g(x, lut[label], w) if rows is None else g(x, lut[label], w, rows)
            correct += (ids[g.logits.argmax(1)] == label).sum()
            count += len(label)
        self.update_scheduler()
        return self._epoch_stats(total, correct, count, len(train_loader))

    def _epoch_stats(self, total, correct, count, n_batches):
        """(mean loss per batch, accuracy) over ALL ranks' batches: the reference gathers predictions and labels of every rank, padded duplicates
        included, for the accuracy (textual_prompt.py:146-150); its loss stays per rank -- here it is the mean over the ranks."""
        t = torch.tensor([float(total), float(correct), float(count), float(n_batches)], dtype=torch.float64, device=self.device)
        gdist.allreduce_sum_(t)
        total, correct, count, n_batches = t.tolist()
        return total / max(n_batches, 1.0), correct / max(count, 1.0)

    def _train_epoch_eager(self, train_loader, classes, ids, lut, accum, aug=None, epoch=0, soft=None):
        total, correct, count = 0.0, 0, 0
        for i, (img, _, _, label, names) in enumerate(train_loader):
            img, label = img.to(self.device), label.to(self.device)
            if aug is not None:
                img = aug.batch(img.contiguous(), names, epoch)
            image_features, text_features = self.features(img, classes, None if aug is not None else list(names))      # views are never cached by name
            logits = steps.CosineHeadFn.apply(image_features, text_features, self.scale())
            w = self.row_weights(label.tolist(), names).to(self.device)
            loss = steps.step_loss(logits, lut[label], w, soft, self.soft_rows(soft, label.tolist(), names)) / accum
            loss.backward()
            total += float(loss.detach()) * accum
            if (i + 1) % accum == 0 or i + 1 == len(train_loader):
                gdist.allreduce_mean_([p.grad for p in self.model.parameters() if p.grad is not None])
                self.backpropagate()
            correct += int((ids[logits.argmax(1)] == label).sum())
            count += len(label)
        self.update_scheduler()
        return self._epoch_stats(total, correct, count, len(train_loader))

    @torch.no_grad()
    def predict(self, data, classes):
        """Global label ids predicted for every item of `data`, logits [N, len(classes)] on the CPU, in dataset order on every rank.  Sharded like the
        reference's evaluation loops under accelerate (`accelerator.prepare(test_loader)`, textual_prompt.py:239): each rank runs its own batches
        (dist.rank_batches over the dataset order), the per-rank logits are all-gathered and the samples accelerate's even sharding duplicated
        are dropped again (:285-294)."""
        ids = torch.tensor([self.label_to_idx[c] for c in classes], device=self.device)
        outs = []
        tuner = self.test_time_tuner(classes)      # None unless TPT is on (and this is not the plain validation of `train`)
        cache, feats = (None if self._tda_plain else self.tda), []      # TDA: the features of every batch are kept for the stream below
        for batch in self._loader(data, False):
            img = batch[0].to(self.device)
            if tuner is not None:     # TPT: every item's row comes from a context tuned on its own views; view 0's features feed the heads below
                view_features = tuner.encode_views(img, list(batch[-1]))      # (the item names: last in a batch, with or without labels)
                image_features = view_features[:, 0].contiguous()
                logits = tuner.predict_rows(view_features)
                text_features = None
            elif self.mv_predict:     # MV_PREDICT: the mode of each item's views under the current model stands in for its single embedding
                views = self.multi_view.make_views(img.float().contiguous(), list(batch[-1]))      # (the item names: last in a batch, with or without labels)
                view_features, text_features = self.features(views, classes)
                image_features = self.multi_view.aggregate(view_features.detach().float().view(img.shape[0], self.multi_view.views, -1), text_features.detach(),
                                                           self.scale())
            else:
                image_features, text_features = self.features(img, classes)
            if self.adapter is not None:      # CLIP_ADAPTER: the features are adapted before the head (row by row: the batching changes no bit)
                image_features = self.adapter(image_features)
            if tuner is None:
                logits, _, am, _ = cosine_head(image_features, text_features, self.scale(), want_probs=False)
            if self.tip is not None:      # TIP_ADAPTER: the cache term of the iteration's training set
                logits = self._add_cache_term(image_features, logits, classes)
            if self.gda is not None:      # GDA_HEAD: the discriminant term of the iteration's training set
                logits = self._add_gda_term(image_features, logits, classes)
            if self.probe is not None:    # LINEAR_PROBE: the trained residual of the iteration's training set
                logits = self._add_probe_term(image_features, logits, classes)
            outs.append(logits)
            if cache is not None:
                feats.append(image_features.detach().float())      # what the head terms saw
        logits = torch.cat(outs) if outs else torch.empty(0, len(classes), device=self.device)
        logits = gdist.gather_in_dataset_order(logits, len(data), int(self.config.BATCH_SIZE))
        if cache is not None and feats:     # TDA: one stream over the whole set, in dataset order, the same on every rank
            emb = gdist.gather_in_dataset_order(torch.cat(feats), len(data), int(self.config.BATCH_SIZE))
            logits = cache(logits, emb)
        return ids[logits.argmax(1)].cpu(), logits.cpu()

    def test_time_tuner(self, classes):
        """The tpt.TestTimeTuner of the current model over `classes`, or None: TPT off, or the plain validation of `train`.  One tuner per model
        (define_model makes a new one stale); it owns its optimizer."""
        if self.tpt_settings is None or self._tpt_plain:
            return None
        from ..tpt import TestTimeTuner
        if self._tpt is None or self._tpt.model is not self.model:
            self._tpt = TestTimeTuner(self.model, self.clip_model, **self.tpt_settings)
        self.model.classes = classes
        return self._tpt

    def _run_validation(self, val_data, only_seen=False):
        classes = self.seen_classes if only_seen and self.val_unseen_files is None else self.classes
        pred, _ = self.predict(val_data, classes)
        labels = torch.tensor([l if val_data.label_id else self.label_to_idx[l] for l in val_data.labels])
        return float((pred == labels).float().mean())

    def train(self, train_data, val_data, unlabeled_data=None, only_seen=False, iter_train=False):
        train_data = self.create_training_dataset(train_data, unlabeled_data) if not iter_train else train_data
        self.define_model(self.seen_classes if only_seen else self.classes)
        loader = self._loader(train_data, True)
        best_acc, best_prompt = -1.0, None
        for epoch in range(int(self.config.EPOCHS)):
            loss, acc = self._train_epoch(loader, only_seen=only_seen, epoch=epoch)
            self._tpt_plain = not bool(getattr(self.config, "TPT_VALIDATION", False))      # (an episode per validation item every epoch: only on request)
            self._tda_plain = not bool(getattr(self.config, "TDA_VALIDATION", False))
            try:
                val_acc = self._run_validation(val_data, only_seen=only_seen) if val_data is not None and len(val_data) else acc
            finally:
                self._tpt_plain = self._tda_plain = False
            log.info(f"epoch {epoch}: loss {loss:.4f} train acc {acc:.3f} val acc {val_acc:.3f}")
            if val_acc > best_acc:
                best_acc, best_prompt = val_acc, self.prompt_snapshot()
        if self.tip_adapter():
            self.build_tip_cache(train_data, val_data, only_seen=only_seen)
        if self.clip_adapter():
            self.build_feature_adapter(train_data, val_data, only_seen=only_seen)
        if self.gda_head():
            self.build_gda_head(train_data, val_data, only_seen=only_seen)
        if self.linear_probe():
            self.build_linear_probe(train_data, val_data, only_seen=only_seen)
        return best_acc, best_prompt

    # ------------------------------------------------------------------ Tip-Adapter cache (TIP_ADAPTER, textual strategies)
    @torch.no_grad()
    def _tip_inputs(self, data, classes, lut):
        """(frozen image features [N, E], CLIP logits [N, C] of the current prompt, class positions [N], names) of a labelled dataset, in dataset
        order; items whose label is outside `classes` are dropped."""
        feats, labs, names = [], [], []
        for img, _, _, label, nm in torch.utils.data.DataLoader(data, batch_size=int(self.config.BATCH_SIZE), shuffle=False):
            feats.append(self.frozen_image_features(img.to(self.device), list(nm)))
            label = label.to(self.device)
            labs.append(torch.where(label < len(lut), lut[label.clamp(max=len(lut) - 1)], torch.full_like(label, -1)))
            names += list(nm)
        feats, labs = torch.cat(feats), torch.cat(labs)
        keep = labs >= 0
        self.model.classes = classes
        logits = cosine_head(feats[keep], self.model(classes), self.scale(), want_probs=False)[0]
        return feats[keep], logits, labs[keep], [n for n, k in zip(names, keep.tolist()) if k]

    def build_tip_cache(self, train_data, val_data=None, only_seen=False):
        """The Tip-Adapter cache of the iteration just trained: keys = the unit-normalised frozen features of the training set (labelled shots and
        pseudolabelled pool rows: the same cached embeddings the prompt steps read), values = their labels, key weight TIP_PSEUDO_WEIGHT for the
        pseudolabelled rows.  TIP_FINETUNE_EPOCHS > 0 trains the keys alone (Tip-Adapter-F: steps.GraphedTipStep on the training set, AdamW at TIP_LR);
        TIP_SEARCH picks (alpha, beta) on the validation set.  From here on predict() -- hence _run_validation, test_predictions and evaluation -- adds
        the cache term to the logits it computes.

        The pseudolabel pass is NOT touched: assign_pseudo_labels and the frozen-CLIP pass keep ranking the pool by the CLIP logits of the prompts
        alone, so their lists stay the certified lists of the reference function."""
        c = self.config
        classes, ids, lut = self._class_space(only_seen)
        feats, clip_logits, labs, names = self._tip_inputs(train_data, classes, lut)
        pseudo = [getattr(self, "fpl", False) and (self.paradigm == "ul" or n in self.check_unlabeled) for n in names]
        epochs = int(getattr(c, "TIP_FINETUNE_EPOCHS", 0))
        self.tip = TipAdapterModel.from_lists(feats, labs, pseudo, len(classes), pseudo_weight=float(getattr(c, "TIP_PSEUDO_WEIGHT", 1.0)),
                                              alpha=float(getattr(c, "TIP_ALPHA", 1.0)), beta=float(getattr(c, "TIP_BETA", 5.5)), train_keys=epochs > 0)
        self.tip_classes, self.tip_losses, self.tip_search = list(classes), [], None
        if epochs > 0:
            B = int(c.BATCH_SIZE)
            opt = torch.optim.AdamW([self.tip.keys], lr=float(getattr(c, "TIP_LR", 1e-3)), eps=1e-4)
            step = steps.GraphedTipStep(self.tip, opt) if getattr(c, "GRAPH_STEPS", True) else None
            g = torch.Generator().manual_seed(int(getattr(c, "LOADER_SEED", 0)))
            gid = ids[labs].tolist()      # global label ids, as row_weights reads them
            for _ in range(epochs):
                order = torch.randperm(len(names), generator=g).tolist()
                total, nb = torch.zeros((), dtype=torch.float64, device=self.device), 0
                for lo in range(0, len(order), B):
                    rows = order[lo:lo + B]
                    idx = torch.tensor(rows, device=self.device)
                    w = self.row_weights([gid[r] for r in rows], [names[r] for r in rows]).to(self.device)
                    if step is not None:
                        total += step(feats[idx], labs[idx], w, clip_logits[idx])
                    else:
                        total += steps.tip_step(self.tip, feats[idx], clip_logits[idx], labs[idx].to(torch.int32), w, opt)
                    nb += 1
                self.tip_losses.append(float(total) / max(nb, 1))
            log.info(f"Tip-Adapter-F: {epochs} epochs over {len(names)} keys, loss {self.tip_losses[0]:.4f} -> {self.tip_losses[-1]:.4f}")
        if bool(getattr(c, "TIP_SEARCH", False)) and val_data is not None and len(val_data):
            vf, vl, vy, _ = self._tip_inputs(val_data, classes, lut)
            if len(vy):
                self.tip_search = self.tip.search(list(getattr(c, "TIP_ALPHA_GRID", (0.5, 1.0, 2.0, 3.0, 5.0))),
                                                  list(getattr(c, "TIP_BETA_GRID", (1.0, 3.0, 5.5, 8.0))), vf, vl, vy)
                log.info(f"Tip-Adapter search: alpha {self.tip_search[0]:g} beta {self.tip_search[1]:g} (validation accuracy {self.tip_search[2]:.3f})")
        return self.tip

    def load_tip_cache(self, path, classes=None):
        """Install a cache file written by utils.save_parameters(..., cache=strategy.tip); `classes`: its class list (default: all classes)."""
        self.tip = TipAdapterModel.load(path, device=self.device)
        self.tip_classes = list(classes if classes is not None else self.classes)
        return self.tip

    @torch.no_grad()
    def _add_cache_term(self, image_features, logits, classes):
        """logits [N, len(classes)] + the cache term of the columns the cache knows (all of them when `classes` is the cache's own list: then the
        kernel adds in place of a clone; otherwise the term is computed against zeros and its columns are gathered)."""
        if list(classes) == self.tip_classes:
            return self.tip(image_features, logits)
        term = self.tip(image_features, torch.zeros(logits.shape[0], len(self.tip_classes), device=logits.device))
        pos = {c: i for i, c in enumerate(self.tip_classes)}
        cols = [(j, pos[c]) for j, c in enumerate(classes) if c in pos]
        if cols:
            dst, src = (torch.tensor(x, device=logits.device) for x in zip(*cols))
            logits[:, dst] += term[:, src]
        return logits

    # ------------------------------------------------------------------ CLIP-Adapter feature head (CLIP_ADAPTER, textual strategies)
    def build_feature_adapter(self, train_data, val_data=None, only_seen=False):
        """The CLIP-Adapter of the iteration just trained: a fresh models.ClipAdapterModel (seeded with OPTIM_SEED from a generator of its own)
        trained for ADAPTER_EPOCHS on the training set's cached frozen features (labelled shots and pseudolabelled pool rows: the rows the prompt
        steps read) against the fixed text features of the prompt just trained, with the strategy's row weights, a LOADER_SEED permutation per
        epoch and batches of BATCH_SIZE (steps.GraphedAdapterStep, or steps.adapter_step with GRAPH_STEPS: False; AdamW at ADAPTER_LR).  From here
        on predict() -- hence _run_validation, test_predictions and evaluation -- adapts the image features before the cosine head.

        The pseudolabel pass is NOT touched: assign_pseudo_labels and the frozen-CLIP pass keep ranking the pool by the CLIP logits of the prompts
        alone, so pseudolabel lists and prompt files are the same with the switch on or off."""
        c = self.config
        classes, ids, lut = self._class_space(only_seen)
        with torch.random.fork_rng(devices=[]):      # (a DataLoader without a generator of its own draws its base seed from the GLOBAL stream, which
            feats, _, labs, names = self._tip_inputs(train_data, classes, lut)      # the GRIP prompt re-initialisations read: ADVICE r5 -- left as found)
        with torch.no_grad():
            text = self.model(classes).detach().float().contiguous()
        model = ClipAdapterModel(feats.shape[1], reduction=int(getattr(c, "ADAPTER_REDUCTION", 4)), ratio=float(getattr(c, "ADAPTER_RATIO", 0.2)),
                                 seed=int(getattr(c, "OPTIM_SEED", 0)), device=self.device)
        epochs, B, scale = int(getattr(c, "ADAPTER_EPOCHS", 20)), int(c.BATCH_SIZE), self.scale()
        opt = torch.optim.AdamW([model.w1, model.w2], lr=float(getattr(c, "ADAPTER_LR", 1e-3)), eps=1e-4)
        step = steps.GraphedAdapterStep(model, text, scale, opt) if getattr(c, "GRAPH_STEPS", True) else None
        g = torch.Generator().manual_seed(int(getattr(c, "LOADER_SEED", 0)))
        gid = ids[labs].tolist()      # global label ids, as row_weights reads them
        self.adapter_losses = []
        for _ in range(epochs):
            order = torch.randperm(len(names), generator=g).tolist()
            total, nb = torch.zeros((), dtype=torch.float64, device=self.device), 0
            for lo in range(0, len(order), B):
                rows = order[lo:lo + B]
                idx = torch.tensor(rows, device=self.device)
                w = self.row_weights([gid[r] for r in rows], [names[r] for r in rows]).to(self.device)
                if step is not None:
                    total += step(feats[idx], labs[idx], w)
                else:
                    total += steps.adapter_step(model, feats[idx], text, scale, labs[idx].to(torch.int32), w, opt)
                nb += 1
            self.adapter_losses.append(float(total) / max(nb, 1))
        if epochs > 0:
            log.info(f"CLIP-Adapter: {epochs} epochs over {len(names)} rows, loss {self.adapter_losses[0]:.4f} -> {self.adapter_losses[-1]:.4f}")
        self.adapter = model
        return model

    def load_feature_adapter(self, path):
        """Install an adapter file written by utils.save_parameters(..., adapter=strategy.adapter)."""
        self.adapter = ClipAdapterModel.load(path, device=self.device)
        return self.adapter

    # ------------------------------------------------------------------ Gaussian discriminant head (GDA_HEAD, textual strategies)
    def build_gda_head(self, train_data, val_data=None, only_seen=False):
        """The discriminant head of the iteration just trained: models.GdaHeadModel.fit on the training set's cached frozen features (labelled shots
        and pseudolabelled pool rows: the rows the prompt steps read; a pseudolabelled row weighs GDA_PSEUDO_WEIGHT), ridge GDA_SHRINK, no training.
        GDA_SEARCH picks alpha from GDA_ALPHA_GRID on the validation set.  From here on predict() -- hence _run_validation, test_predictions and
        evaluation -- adds alpha * (normalize(f) . w_c - bias_c) to the logits it computes.

        The pseudolabel pass is NOT touched: assign_pseudo_labels and the frozen-CLIP pass keep ranking the pool by the CLIP logits of the prompts
        alone, so pseudolabel lists and prompt files are the same with the switch on or off."""
        c = self.config
        classes, ids, lut = self._class_space(only_seen)
        with torch.random.fork_rng(devices=[]):      # (_tip_inputs' DataLoader draws its base seed from the global stream: see build_feature_adapter)
            feats, _, labs, names = self._tip_inputs(train_data, classes, lut)
        pseudo = [getattr(self, "fpl", False) and (self.paradigm == "ul" or n in self.check_unlabeled) for n in names]
        self.gda = GdaHeadModel.fit(feats, labs, pseudo, len(classes), pseudo_weight=float(getattr(c, "GDA_PSEUDO_WEIGHT", 1.0)),
                                    shrink=float(getattr(c, "GDA_SHRINK", 1.0)), alpha=float(getattr(c, "GDA_ALPHA", 1.0)))
        self.gda_classes, self.gda_search = list(classes), None
        if bool(getattr(c, "GDA_SEARCH", False)) and val_data is not None and len(val_data):
            with torch.random.fork_rng(devices=[]):
                vf, vl, vy, _ = self._tip_inputs(val_data, classes, lut)
            if len(vy):
                self.gda_search = self.gda.search(list(getattr(c, "GDA_ALPHA_GRID", (0.1, 0.3, 1.0, 3.0, 10.0))), vf, vl, vy)
                log.info(f"GDA head search: alpha {self.gda_search[0]:g} (validation accuracy {self.gda_search[1]:.3f})")
        return self.gda

    def load_gda_head(self, path, classes=None):
        """Install a head file written by utils.save_parameters(..., gda=strategy.gda); `classes`: its class list (default: all classes)."""
        self.gda = GdaHeadModel.load(path, device=self.device)
        self.gda_classes = list(classes if classes is not None else self.classes)
        return self.gda

    @torch.no_grad()
    def _add_gda_term(self, image_features, logits, classes):
        """logits [N, len(classes)] + the discriminant term of the columns the head knows (all of them when `classes` is the head's own list: one
        launch; otherwise the term is computed against no base and its columns are gathered), as _add_cache_term does for the Tip cache."""
        if list(classes) == self.gda_classes:
            return self.gda(image_features, logits)
        term = self.gda(image_features, torch.zeros(logits.shape[0], len(self.gda_classes), device=logits.device))
        pos = {c: i for i, c in enumerate(self.gda_classes)}
        cols = [(j, pos[c]) for j, c in enumerate(classes) if c in pos]
        if cols:
            dst, src = (torch.tensor(x, device=logits.device) for x in zip(*cols))
            logits[:, dst] += term[:, src]
        return logits

    # ------------------------------------------------------------------ trained linear probe (LINEAR_PROBE, textual strategies)
    def build_linear_probe(self, train_data, val_data=None, only_seen=False):
        """The linear probe of the iteration just trained: models.LinearProbeModel.fit on the training set's cached frozen features (labelled shots and
        pseudolabelled pool rows: the rows the prompt steps read; a pseudolabelled row weighs PROBE_PSEUDO_WEIGHT) against the CLIP logits of the prompt
        just trained -- a residual on them that starts at zero (PROBE_INIT "gda": at the Gaussian discriminant head of the same rows, ridge GDA_SHRINK) --
        for PROBE_ITERS full-batch heavy-ball iterations (PROBE_MOMENTUM, ridge PROBE_L2, the step from the Lipschitz bound).  With SOFT_PSEUDOLABELS
        the pseudolabelled rows train on the targets engine.soft_ce builds for them from the last pass's matrix (the sharpening is that kernel's, not
        restated here); every other row is hard.  PROBE_SEARCH picks alpha from PROBE_ALPHA_GRID on the validation set.  From here on predict() --
        hence _run_validation, test_predictions and evaluation -- adds alpha * (scale * normalize(f) . W_c + b_c) to the logits it computes.

        The pseudolabel pass is NOT touched: assign_pseudo_labels and the frozen-CLIP pass keep ranking the pool by the CLIP logits of the prompts
        alone, so pseudolabel lists and prompt files are the same with the switch on or off."""
        c = self.config
        classes, ids, lut = self._class_space(only_seen)
        with torch.random.fork_rng(devices=[]):      # (_tip_inputs' DataLoader draws its base seed from the global stream: see build_feature_adapter)
            feats, clip_logits, labs, names = self._tip_inputs(train_data, classes, lut)
        pseudo = [getattr(self, "fpl", False) and (self.paradigm == "ul" or n in self.check_unlabeled) for n in names]
        labels, targets = labs, None
        soft = self.soft_targets(classes, only_seen)
        if isinstance(soft, steps.CandidateTargets):
            soft = None         # (CANDIDATE_PSEUDOLABELS: the probe keeps the hard label of every set)
        rows = self.soft_rows(soft, ids[labs].tolist(), names) if soft is not None else None
        if rows is not None:
            _, _, targets = soft_ce(clip_logits, labs, torch.ones(len(names), device=self.device), soft.matrix, rows, soft.col_map, soft.temperature,
                                    soft.smoothing, want_target=True)
            labels = torch.where(rows.to(labs.device) >= 0, torch.full_like(labs, -1), labs)
        self.probe_targets = (labels, targets)      # (what the fit was given: the rows with label -1 train on their row of targets)
        init = None
        scale = float(self.scale())
        if str(getattr(c, "PROBE_INIT", "zero")) == "gda":
            g = GdaHeadModel.fit(feats, labs, pseudo, len(classes), pseudo_weight=float(getattr(c, "PROBE_PSEUDO_WEIGHT", 1.0)),
                                 shrink=float(getattr(c, "GDA_SHRINK", 1.0)))
            init = (g.w / scale, -g.bias)
        self.probe = LinearProbeModel.fit(feats, clip_logits, labels, pseudo, len(classes), soft=targets,
                                          pseudo_weight=float(getattr(c, "PROBE_PSEUDO_WEIGHT", 1.0)), scale=scale, l2=float(getattr(c, "PROBE_L2", 0.1)),
                                          iters=int(getattr(c, "PROBE_ITERS", 300)), momentum=float(getattr(c, "PROBE_MOMENTUM", 0.9)),
                                          alpha=float(getattr(c, "PROBE_ALPHA", 1.0)), init=init)
        self.probe_classes, self.probe_search = list(classes), None
        trace = self.probe.loss_trace
        log.info(f"linear probe: {trace.numel()} iterations over {len(names)} rows, loss {float(trace[0]):.4f} -> {float(trace[-1]):.4f} (at the start of the last)")
        if bool(getattr(c, "PROBE_SEARCH", False)) and val_data is not None and len(val_data):
            with torch.random.fork_rng(devices=[]):
                vf, vl, vy, _ = self._tip_inputs(val_data, classes, lut)
            if len(vy):
                self.probe_search = self.probe.search(list(getattr(c, "PROBE_ALPHA_GRID", (0.1, 0.3, 1.0, 3.0, 10.0))), vf, vl, vy)
                log.info(f"linear probe search: alpha {self.probe_search[0]:g} (validation accuracy {self.probe_search[1]:.3f})")
        return self.probe

    def load_linear_probe(self, path, classes=None):
        """Install a head file written by utils.save_parameters(..., probe=strategy.probe); `classes`: its class list (default: all classes)."""
        self.probe = LinearProbeModel.load(path, device=self.device)
        self.probe_classes = list(classes if classes is not None else self.classes)
        return self.probe

    @torch.no_grad()
    def _add_probe_term(self, image_features, logits, classes):
        """logits [N, len(classes)] + the probe's term of the columns it knows (all of them when `classes` is the probe's own list: one launch;
        otherwise the term is computed against no base and its columns are gathered), as _add_gda_term does for the discriminant head."""
        if list(classes) == self.probe_classes:
            return self.probe(image_features, logits)
        term = self.probe(image_features, torch.zeros(logits.shape[0], len(self.probe_classes), device=logits.device))
        pos = {c: i for i, c in enumerate(self.probe_classes)}
        cols = [(j, pos[c]) for j, c in enumerate(classes) if c in pos]
        if cols:
            dst, src = (torch.tensor(x, device=logits.device) for x in zip(*cols))
            logits[:, dst] += term[:, src]
        return logits

    # ------------------------------------------------------------------ evaluation
    def test_predictions(self, data, standard_zsl=False):
        import pandas as pd
        classes = self.unseen_classes if standard_zsl else self.classes
        pred, _ = self.predict(data, classes)
        idx_to_class = {v: k for k, v in self.label_to_idx.items()}
        df = pd.DataFrame({"id": [f.split("/")[-1] for f in data.filepaths], "class": [idx_to_class[int(p)] for p in pred]})
        df.drop_duplicates(subset=["id", "class"], inplace=True)
        return df

    def evaluation(self, data):
        pred, logits = self.predict(data, self.classes)
        idx_to_class = {v: k for k, v in self.label_to_idx.items()}
        return [f.split("/")[-1] for f in data.filepaths], [idx_to_class[int(p)] for p in pred], logits

    # ------------------------------------------------------------------ pseudolabels from the trained model
    @torch.no_grad()
    def trained_text_features(self, classes, clip_model):
        """Text features [C, E] of the CURRENT prompts through `clip_model`'s text tower (the f16 model or its exact twin),
        and the visual prompt (or None) the image side has to be encoded with."""
        from ..engine import text_prefix_forward
        if self.modality == "text":
            ids = self.text_encoder._token_ids(self.model.prefix.shape[1], classes)
            deep = getattr(self.model, "deep_prefix", None)      # deep CoOp: the twin's text tower reads the same deep prompts
            return text_prefix_forward(clip_model.text_tower, ids, self.model.prefix.detach(), deep=None if deep is None else deep.detach()), None
        if self.modality == "image":
            return clip_model.encode_text(clip.tokenize(self.text_prompts(classes)).to(self.device)), self.model.prefix.detach()
        if self.maple():      # the twin's text tower reads the same deep text prompts; the image side takes vis_prefix (+ deep_prompts())
            ctx, deep_text, vis_prefix, _ = self.model.couple()
            ids = self.text_encoder._token_ids(ctx.shape[1], classes)
            return text_prefix_forward(clip_model.text_tower, ids, ctx.detach(), deep=None if deep_text is None else deep_text.detach()), vis_prefix.detach()
        coop_embs, vpt_embs = self.model.mix()[:2]
        ids = self.text_encoder._token_ids(coop_embs.shape[1], classes)
        return text_prefix_forward(clip_model.text_tower, ids, coop_embs.detach()), vpt_embs.detach()

    @torch.no_grad()
    def deep_prompts(self):
        """The trained deep prompts [D, P, d] the image tower reads (detached), or None: the visual model's deep_prefix, or the deep rows of
        the UPT mixer's output (deep UPT; the mixer is deterministic, so this is the tensor the model's own forward feeds the tower)."""
        if self.modality == "image":
            deep = getattr(self.model, "deep_prefix", None)
        elif self.modality == "multi" and self.maple():
            deep = self.model.couple()[3]      # the coupled deep visual prompts
        else:
            deep = self.model.mix()[2] if self.modality == "multi" and getattr(self.model, "mix_deep", False) else None
        return None if deep is None else deep.detach()

    @torch.no_grad()
    def trained_features(self, images, classes, chunk=440, paths=None):
        """(image features [N, E] of the whole ordered pool, text features [C, E]) of the CURRENT model for the pseudolabel pass.
        The image side goes through pseudolabels.encode_pool: chunked, sharded contiguously over the ranks of one node, one
        all-gather of the embeddings -- with the trained visual prompt where the modality has one.  The text
        side is computed once per call on every rank (C x 6 GF, cheaper than a broadcast); the UPT mixer runs once.  The
        reference does all of this per image at batch 1 (textual_fpl.py:203-205 + :225; visual_fpl.py:250 + :264;
        multimodal_fpl.py:223 runs BOTH towers and the mixer for every image).  paths: the pool's ordered paths, the key under which a textual
        strategy's pool cache (installed by the caller) holds the prompt-free embeddings."""
        tower = self.clip_model.visual.tower
        mv = pl.multiview()

        def pool(txt, prefix=None, deep=None):
            """With a MultiView installed: the modes of every image's views under the current visual prompts in place of encode_pool's rows (they depend
            on txt: the pool cache is neither read nor written)."""
            if paths is None:
                raise ValueError("trained_features: a MultiView is installed and needs the pool's ordered paths (they name the views' boxes)")
            return mv.features(tower, images, paths, txt, self.scale(), chunk=chunk, prefix=prefix, deep=deep), txt
        if self.modality == "text":
            self.model.classes = classes
            if mv is not None:
                return pool(self.model(classes))
            return pl.encode_pool(tower, images, chunk=chunk, paths=paths), self.model(classes)
        if self.modality == "image":
            if mv is not None:
                return pool(self.fixed_text_features(classes), self.model.prefix.detach(), self.deep_prompts())
            return pl.encode_pool(tower, images, chunk=chunk, prefix=self.model.prefix.detach(), deep=self.deep_prompts()), self.fixed_text_features(classes)
        self.model.classes = classes
        if self.maple():
            ctx, deep_text, vis_prefix, vis_deep = self.model.couple()
            txt = self.model.text_encoder(ctx, classes, **({} if deep_text is None else {"deep_prompts": deep_text}))
            if mv is not None:
                return pool(txt, vis_prefix.detach(), None if vis_deep is None else vis_deep.detach())
            return pl.encode_pool(tower, images, chunk=chunk, prefix=vis_prefix.detach(), deep=None if vis_deep is None else vis_deep.detach()), txt
        coop_embs, vpt_embs, *deep = self.model.mix()
        txt = self.model.text_encoder(coop_embs, classes)
        if mv is not None:
            return pool(txt, vpt_embs.detach(), deep[0].detach() if deep else None)
        return pl.encode_pool(tower, images, chunk=chunk, prefix=vpt_embs.detach(), deep=deep[0].detach() if deep else None), txt

    @torch.no_grad()
    def assign_pseudo_labels(self, k, unlabeled_data):
        """The nine `assign_pseudo_labels` of the reference (e.g. transductive_zsl/multimodal_fpl.py:194-285):
        leaderboard over the TRAINED model's logits on the unseen classes (arg-max on the logits, :222)."""
        from ..utils.clip_pseudolabels import _pool_images
        classes = self.unseen_classes if self.paradigm == "trzsl" else self.classes
        images = _pool_images(unlabeled_data, self.transform, self.device)
        labels = [self.label_to_idx[c] for c in classes]
        paths = list(unlabeled_data.filepaths)      # the pool as passed to the pass (grip_train resets it to the original list every iteration): the cache's key
        with pl.pool_cache(self.pool_cache), pl.label_propagation(self.transduction()), pl.soft_targets(self.soft_store), \
                pl.candidate_sets(self.candidate_selection, self.candidate_store), pl.multi_view(self.mv_passes):       # (None: nothing is installed)
            if pl.propagation() is not None:
                log.info(f"{pl.propagation()} is installed: the pass propagates over the pool and takes the plain branch (no reference list to be identical to)")
            if pl.candidates() is not None:
                log.info(f"{pl.candidates()[0]} is installed: the pass selects candidate sets and takes the plain branch (no reference list to be identical to)")
            if pl.multiview() is not None:
                log.info(f"{pl.multiview()} is installed: the pass encodes every image's views and takes the plain branch (no reference list to be identical to)")
            if pl.mode() == "identical" and pl.propagation() is None and pl.candidates() is None and pl.multiview() is None and not self.clip_model.exact:
                # the lists the reference's fp32 pass would produce with these prompts: f16 screen + exact refinement
                twin = self.clip_model.exact_twin()
                txt, vprompt = self.trained_text_features(classes, twin)
                fp, lab = pl.identical_lists(self.clip_model.visual.tower, twin.visual.tower, images, txt, self.scale(),
                                             paths, labels, k, chunk=440, prefix=vprompt, argmax_on="logits",
                                             visual_mid=pl.mid_tower(self.clip_model, len(paths)), deep=self.deep_prompts())
            else:
                img, txt = self.trained_features(images, classes, paths=paths)
                fp, lab = pl.pseudolabel_from_features(img, txt, self.scale(), paths, labels, k, argmax_on="logits")
        unlabeled_data.filepaths, unlabeled_data.labels, unlabeled_data.label_id = fp, lab, True
        return unlabeled_data

    def get_pseudo_labels(self, unlabeled_examples):
        return self.assign_pseudo_labels(int(self.config.N_PSEUDOSHOTS), unlabeled_examples)

    # ------------------------------------------------------------------ iterative schedules
    def _n_pseudoshots(self, niter, num_samples, n_unlabeled, n_classes):
        n = int(niter * num_samples / n_classes)            # pseudo_iterative.py:62-75, 113-125
        return n if n * n_classes <= n_unlabeled else math.floor(n_unlabeled / n_classes)

    def grip_train(self, train_data, val_data, unlabeled_data, only_seen=False):
        """GRIP: grow the number of pseudolabels per class by one STEP_QUANTILE of the pool per iteration,
        re-initialising the prompts each time; iteration 1 labels with frozen CLIP, later ones with the
        previously trained prompts."""
        c = self.config
        num_iter = int(100 / int(c.STEP_QUANTILE))
        n_cls = len(self.unseen_classes if self.paradigm == "trzsl" else self.classes)
        num_samples = int(len(unlabeled_data) / num_iter)
        original_train, original_unlabeled = copy.copy(train_data.filepaths), copy.copy(unlabeled_data.filepaths)
        original_labels, original_label_id = copy.copy(train_data.labels), train_data.label_id
        out = None
        for niter in range(1, num_iter + 1):
            c.N_PSEUDOSHOTS = max(1, self._n_pseudoshots(niter, num_samples, len(original_unlabeled), n_cls))
            train_data.filepaths, train_data.labels, train_data.label_id = list(original_train), list(original_labels), original_label_id
            unlabeled_data.filepaths, unlabeled_data.labels = list(original_unlabeled), None
            if niter == 1:
                data = self.create_training_dataset(train_data, unlabeled_data)
            else:
                data = self.merge_pseudolabels(train_data, self.get_pseudo_labels(unlabeled_data))
            out = self.train(data, val_data, only_seen=only_seen, iter_train=True)
            from ..utils import save_parameters, save_pseudo_labels
            save_pseudo_labels(list(data.filepaths), list(data.labels), c, niter)     # compute_metrics.py:150-154
            save_parameters(out[1], c, iteration=niter, cache=self.tip, adapter=self.adapter, gda=self.gda, probe=self.probe)
            log.info(f"GRIP iteration {niter}/{num_iter}: {c.N_PSEUDOSHOTS} pseudo-shots per class, val acc {out[0]:.3f}")
        return out

    def fixed_iterative_train(self, train_data, val_data, unlabeled_data, only_seen=False):
        """Iterative FPL: same loop with a FIXED number of pseudo-shots per class."""
        c = self.config
        k = int(c.N_PSEUDOSHOTS)
        original_train, original_unlabeled = copy.copy(train_data.filepaths), copy.copy(unlabeled_data.filepaths)
        original_labels, original_label_id = copy.copy(train_data.labels), train_data.label_id
        out = None
        for niter in range(1, int(100 / int(c.STEP_QUANTILE)) + 1):
            c.N_PSEUDOSHOTS = k
            train_data.filepaths, train_data.labels, train_data.label_id = list(original_train), list(original_labels), original_label_id
            unlabeled_data.filepaths, unlabeled_data.labels = list(original_unlabeled), None
            data = self.create_training_dataset(train_data, unlabeled_data) if niter == 1 else \
                self.merge_pseudolabels(train_data, self.get_pseudo_labels(unlabeled_data))
            out = self.train(data, val_data, only_seen=only_seen, iter_train=True)
        return out
