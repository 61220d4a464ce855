"""Encoder wrappers with the reference's names and signatures (models/clip_encoders.py), running
on the native towers.  Backbone parameters stay frozen; autograd delivers a gradient only to the
prompt tensors."""
import logging

import torch
import torch.nn as nn

from .. import clip
from ..engine import text_prefix_forward, vit_prefix_forward

log = logging.getLogger(__name__)


class TextEncoder(nn.Module):
    """CLIP text encoder (reference :13-22)."""

    def __init__(self, clip_model):
        super().__init__()
        self.clip_model = clip_model

    def forward(self, text):
        return self.clip_model.encode_text(text)


class CustomTextEncoder(nn.Module):
    """Reference :25-90: splice a learnable prefix over token positions 1..P of 'X .. X <class>'."""

    def __init__(self, clip_model, device, dtype):
        super().__init__()
        self.dtype = dtype
        self.clip_model = clip_model
        self.transformer = clip_model.transformer
        self.positional_embedding = clip_model.positional_embedding
        self.ln_final = clip_model.ln_final
        self.text_projection = clip_model.text_projection
        self.token_embedding = clip_model.token_embedding
        self.device = device
        self._tok_cache = {}

    def tokenize(self, text):
        return torch.cat([clip.tokenize(tok) for tok in text])

    def _token_ids(self, n_prefix, classes):
        key = (n_prefix, tuple(classes))
        ids = self._tok_cache.get(key)
        if ids is None:
            prompts = [" ".join([" ".join(["X"] * n_prefix).strip(), c]) for c in classes]   # reference :54-57
            ids = clip.tokenize(prompts).to(self.device)
            if len(self._tok_cache) > 64:
                self._tok_cache.clear()
            self._tok_cache[key] = ids
        return ids

    def forward(self, class_embeddings, classes, enable_pos_emb=True, deep_prompts=None):
        """deep_prompts: None or the context's deep prompts (deep CoOp): [D, P, d] (or [D, 1, P, d]) with a shared context, [D, C, P, d] with one
        context per class, 1 <= D <= layers - 1.  Before block l (1 <= l <= D) positions 1 .. P of every class's stream are replaced by
        deep_prompts[l - 1], no LayerNorm and no positional embedding -- the text-tower mirror of CustomVisionTransformer's deep_prompts.
        Differentiable, as class_embeddings is."""
        token_ids = self._token_ids(class_embeddings.size()[1], classes)
        return text_prefix_forward(self.clip_model.text_tower, token_ids, class_embeddings, pos_emb=bool(enable_pos_emb), deep=deep_prompts)   # :70-74


class ImageEncoder(nn.Module):
    """CLIP image encoder (reference :93-102)."""

    def __init__(self, clip_model):
        super().__init__()
        self.clip_model = clip_model

    def forward(self, text):
        return self.clip_model.encode_image(text)


class CustomVisionTransformer(nn.Module):
    """Reference :105-194: ViT with a visual prompt inserted between CLS and the patches.  image_prefix follows the reference's
    image_prefix.expand(B, -1, -1) (:148): [P, d] or [1, P, d] is one prompt shared by the batch, [B, P, d] one prompt per image
    (instance-conditioned prompts, or several prompt sets in one batch); autograd returns the gradient in the prompt's own shape --
    [B, P, d] per image.  Any other leading size raises, as expand does."""

    def __init__(self, vision_transformer):
        super().__init__()
        self.input_resolution = vision_transformer.input_resolution
        self.output_dim = vision_transformer.output_dim
        self.conv1 = vision_transformer.conv1
        self.class_embedding = vision_transformer.class_embedding
        self.positional_embedding = vision_transformer.positional_embedding
        self.ln_pre = vision_transformer.ln_pre
        self.transformer = vision_transformer.transformer
        self.ln_post = vision_transformer.ln_post
        self.proj = vision_transformer.proj
        self._vt = [vision_transformer]

    def forward(self, x, image_prefix, pos_emb=True, deep_embs=None, deep_prompts=None):
        """deep_prompts: None or [D, P, d] (1 <= D <= layers - 1) deep visual prompts: before block l (1 <= l <= D) the stream's prompt rows are
        replaced by deep_prompts[l - 1], no LayerNorm and no positional embedding -- the reference's deep branch (:158-174) with its vpt_proj and
        vpt_dropout as identity (a projection, if wanted, is applied by the caller before the call).  Differentiable, as image_prefix is."""
        if deep_embs is not None:
            # reference :158-174 reads self.visual / self.mvlpt_model, attributes this class never has: the branch raises
            # AttributeError upstream as well (VPT_DEEP is False in every config).  The native form of deep prompts is `deep_prompts`.
            raise NotImplementedError("deep prompts are unreachable in the reference (VPT_DEEP: False; :158-174 reads attributes that do not exist); "
                                      "pass deep_prompts= for the engine's deep visual prompts")
        return vit_prefix_forward(self._vt[0].tower, x, image_prefix, pos_emb=bool(pos_emb), deep=deep_prompts)   # :141


class CustomImageEncoder(nn.Module):
    """Reference :198-208.  prefix: [P, d] / [1, P, d] shared, or [B, P, d] one prompt per image (CustomVisionTransformer)."""

    def __init__(self, visual):
        super().__init__()
        self.visual = CustomVisionTransformer(visual)
        self.dtype = self.visual.conv1.weight.dtype

    def forward(self, image, prefix, deep_embds=None, deep_prompts=None):
        return self.visual(image, prefix, deep_embs=deep_embds, deep_prompts=deep_prompts)
