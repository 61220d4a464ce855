"""Test-time streaming cache (TDA: Karmanov et al., CVPR 2024 -- the model of include/grip_amd.h, grip_stream_cache_plan / grip_stream_cache_head, not the
paper's code) for every strategy: as the items of a `predict` call stream by in dataset order, the lowest-entropy items seen so far sit in small
per-class queues, a positive and a negative one, and every item is scored against the queue contents of its moment with the Tip-Adapter affinity.  No
tower pass, no backward: the adapter only post-processes the logits and the image features `predict` already has, so it composes with every head.

The published form is a host loop per item.  Here the queue history comes from one scan of the base logits (engine.stream_cache_plan) and the scores
from one interval-masked cache head over all items (engine.stream_cache_head); the rows are the loop's, item for item.  A stream is one call: nothing
survives it."""
from . import engine, native


class StreamCache:
    """StreamCache(...)(base_logits [n, c], img_emb [n, e]) -> adapted logits [n, c], both f32 on the GPU and in stream (dataset) order.

    The defaults are the paper's ImageNet settings AS RECALLED (queue sizes 3 / 2, alpha 2.0 / 0.117, beta 5.0 / 1.0, the negative queue's entropy window
    (0.2, 0.5) on H / log c and its mask window (0.03, 1.0) on the probabilities): recalled, untuned here.  neg_cap = 0 turns the negative queue off.
    A bad value raises ValueError.  `streams` counts the calls; `plan` is the last call's queue history (engine.stream_cache_plan's dict)."""

    def __init__(self, pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, neg_entropy=(0.2, 0.5), neg_mask=(0.03, 1.0)):
        try:
            s = engine.check_stream_cache_settings("StreamCache", pos_cap=pos_cap, neg_cap=neg_cap, pos_alpha=pos_alpha, pos_beta=pos_beta,
                                                   neg_alpha=neg_alpha, neg_beta=neg_beta, neg_entropy=neg_entropy, neg_mask=neg_mask)
        except native.GripError as err:
            raise ValueError(str(err)) from None
        self.settings = dict(zip(("pos_cap", "neg_cap", "pos_alpha", "pos_beta", "neg_alpha", "neg_beta", "neg_entropy", "neg_mask"), s))
        self.streams = 0
        self.plan = None

    def __call__(self, base_logits, img_emb):
        logits, self.plan = engine.stream_cache(base_logits.detach().float().contiguous(), img_emb.detach().float().contiguous(), **self.settings)
        self.streams += 1
        return logits
