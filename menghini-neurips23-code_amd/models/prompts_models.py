"""Prompt models with the reference's names, constructor/forward signatures and parameter names
(models/prompts_models.py): they own the only trainable tensors."""
import logging

import torch
from torch import nn

from .. import clip

log = logging.getLogger(__name__)


_SIDE = {}


def _side_stream(device):
    key = torch.device(device).index or 0
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


class _ModuleShim:
    """Reference callers reach `.module.classes` whenever torch.cuda.is_available() (DDP-wrapped
    model, e.g. methods/semi_supervised_learning/textual_prompt.py:94-97); PyTorch-ROCm reports
    cuda available, so an un-wrapped model must answer to `.module` too."""

    @property
    def module(self):
        return self


class TextPrefixModel(_ModuleShim, nn.Module):
    def __init__(self, initial_prefix, text_encoder, classes, temperature=0.07, device="cpu", deep_prefix=None):
        super().__init__()
        self.device = device
        self.initialized_prefix = initial_prefix
        self.classes = classes
        self.prefix = nn.Parameter(initial_prefix)
        self.text_encoder = text_encoder
        # deep CoOp: [D, P, d] prompts replacing the context rows entering blocks 1 .. D (CustomTextEncoder.forward(deep_prompts=))
        self.deep_prefix = nn.Parameter(deep_prefix) if deep_prefix is not None else None

    def forward(self, classes):
        if self.deep_prefix is None:
            return self.text_encoder(self.prefix, classes)     # un-normalised, as reference :31-36
        return self.text_encoder(self.prefix, classes, deep_prompts=self.deep_prefix)


class ImagePrefixModel(_ModuleShim, nn.Module):
    def __init__(self, initial_prefix, image_encoder, temperature=0.07, device="cpu", deep_prefix=None):
        super().__init__()
        self.device = device
        self.initialized_prefix = initial_prefix
        self.prefix = nn.Parameter(initial_prefix)
        self.image_encoder = image_encoder
        # VPT-Deep: [D, P, d] prompts replacing the prompt rows entering blocks 1 .. D (CustomVisionTransformer.forward(deep_prompts=))
        self.deep_prefix = nn.Parameter(deep_prefix) if deep_prefix is not None else None

    def forward(self, x):
        if self.deep_prefix is None:
            return self.image_encoder(x, self.prefix)          # un-normalised, as reference :55-61
        return self.image_encoder(x, self.prefix, deep_prompts=self.deep_prefix)


class UPTModel(_ModuleShim, nn.Module):
    def __init__(self, coop_embeddings, vpt_embeddings, vpt_embeddings_deep, image_encoder, text_encoder, classes,
                 dim_transformer, temperature=0.07, device="cpu", dtype=torch.float32, mix_deep=False):
        super().__init__()
        self.device = device
        self.classes = classes
        self.temperature = temperature
        self.dtype = dtype
        self.coop_embeddings = nn.Parameter(coop_embeddings)
        self.vpt_embeddings = nn.Parameter(vpt_embeddings)
        self.coop_length, self.coop_dim = self.coop_embeddings.size()[1], self.coop_embeddings.size()[2]
        self.vpt_length, self.vpt_dim = self.vpt_embeddings.size()[1], self.vpt_embeddings.size()[2]
        self.vpt_embeddings_deep = nn.Parameter(vpt_embeddings_deep) if vpt_embeddings_deep is not None else None
        # deep UPT: vpt_embeddings_deep [D, P, dv] joins the mixer's sequence and its outputs become the image tower's deep prompts (what :133-134
        # and :146 intend; upstream :135 and :150 discard them).  Off (the default), a given vpt_embeddings_deep is ignored, as upstream.
        if mix_deep and self.vpt_embeddings_deep is None:
            raise ValueError("UPTModel(mix_deep=True) needs vpt_embeddings_deep [D, P, vision_width]")
        self.mix_deep = bool(mix_deep)
        self.proj_coop_pre = nn.Linear(self.coop_dim, dim_transformer, dtype=self.dtype).to(self.device)
        self.proj_coop_post = nn.Linear(dim_transformer, self.coop_dim, dtype=self.dtype).to(self.device)
        self.proj_vpt_pre = nn.Linear(self.vpt_dim, dim_transformer, dtype=self.dtype).to(self.device)
        self.proj_vpt_post = nn.Linear(dim_transformer, self.vpt_dim, dtype=self.dtype).to(self.device)
        self.transformer = clip.model.Transformer(width=dim_transformer, layers=1, heads=1).to(self.device)
        self.image_encoder = image_encoder
        self.text_encoder = text_encoder

    def _native_mixer_ok(self):
        """The native mixer covers what the reference builds (:99-119): one block, one head, on the GPU, float32 -- or the float16 branch
        of multimodal_prompt.py:46 (fp16 prompt embeddings and projection Linears around the fp32 block: the same kernels with fp16 rounding
        points, grip_upt_mixer.half_linears) -- with up to 31 deep prompts [D, P, dv] when mix_deep is on.  Any other shape runs the same
        arithmetic through the framework's kernels."""
        import os
        t = self.transformer
        dtypes_ok = all(p.dtype == self.dtype for p in (self.coop_embeddings, self.vpt_embeddings, self.proj_coop_pre.weight, self.proj_vpt_post.weight)) \
            and t.resblocks[0].ln_1.weight.dtype == torch.float32
        if self.mix_deep:
            d = self.vpt_embeddings_deep
            dtypes_ok = dtypes_ok and d.dtype == self.dtype and d.is_cuda and d.dim() == 3 and 1 <= d.shape[0] <= 31 \
                and tuple(d.shape[1:]) == (self.vpt_length, self.vpt_dim)
        return (self.dtype in (torch.float32, torch.float16) and dtypes_ok and self.coop_embeddings.is_cuda and os.environ.get("GRIP_NATIVE_MIXER", "1") != "0"
                and getattr(t, "layers", 0) == 1 and t.resblocks[0].attn.num_heads == 1 and len(self.coop_embeddings) == 1
                and self.coop_length == self.vpt_length and self.coop_length <= 16 and t.width % 64 == 0 and t.width <= 256)

    def mix(self):
        """Reference :129-146 (incl. the fp32 -> fp16 -> dtype round trip of :138-145): (coop_embs, vpt_embs), and with mix_deep
        (coop_embs, vpt_embs, deep_embs [D, P, dv]) -- the visual rows of the mixer's output split into the shallow prompt and the deep ones."""
        deep = self.vpt_embeddings_deep if self.mix_deep else None
        if self._native_mixer_ok():
            from ..engine import UptMixerFn
            b = self.transformer.resblocks[0]
            outs = UptMixerFn.apply(
                self.coop_embeddings, self.vpt_embeddings, self.proj_coop_pre.weight, self.proj_coop_pre.bias, self.proj_vpt_pre.weight,
                self.proj_vpt_pre.bias, b.ln_1.weight, b.ln_1.bias, b.attn.in_proj_weight, b.attn.in_proj_bias, b.attn.out_proj.weight,
                b.attn.out_proj.bias, b.ln_2.weight, b.ln_2.bias, b.mlp.c_fc.weight, b.mlp.c_fc.bias, b.mlp.c_proj.weight, b.mlp.c_proj.bias,
                self.proj_coop_post.weight, self.proj_coop_post.bias, self.proj_vpt_post.weight, self.proj_vpt_post.bias, *([] if deep is None else [deep]))
            return tuple(o.reshape(-1, n, d).to(self.dtype) for o, n, d in zip(outs, (self.coop_length, self.vpt_length, self.vpt_length),
                                                                               (self.coop_dim, self.vpt_dim, self.vpt_dim)))
        coop = self.proj_coop_pre(self.coop_embeddings)
        vpt = self.proj_vpt_pre(self.vpt_embeddings if deep is None else torch.cat((self.vpt_embeddings, deep), dim=0))
        seq = torch.cat((coop, vpt), dim=0).to(torch.float32)
        out = self.transformer(seq).to(torch.float16)
        n = len(self.coop_embeddings)
        coop_embs = self.proj_coop_post(out[:n].to(self.dtype)).reshape(-1, self.coop_length, self.coop_dim)
        vpt_embs = self.proj_vpt_post(out[n:].to(self.dtype)).reshape(-1, self.vpt_length, self.vpt_dim)
        if deep is None:
            return coop_embs, vpt_embs
        nv = len(self.vpt_embeddings)
        return coop_embs, vpt_embs[:nv], vpt_embs[nv:]

    def forward(self, x, classes):
        coop_embs, vpt_embs, *deep = self.mix()
        kw = {"deep_prompts": deep[0]} if deep else {}
        if x.is_cuda:
            # the two towers are independent until the head: the image tower (forward and, through autograd's
            # stream tracking, its backward) runs on a side stream next to the text tower
            main = torch.cuda.current_stream()
            side = _side_stream(x.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                visual_out = self.image_encoder(x, vpt_embs, **kw)
            vpt_embs.record_stream(side)
            if deep:
                deep[0].record_stream(side)
            text_out = self.text_encoder(coop_embs, classes)
            main.wait_stream(side)
            visual_out.record_stream(main)
            return text_out, visual_out
        text_out = self.text_encoder(coop_embs, classes)
        visual_out = self.image_encoder(x, vpt_embs, **kw)
        return text_out, visual_out


class MaPLeModel(_ModuleShim, nn.Module):
    """Coupled deep multimodal prompts (MaPLe, Khattak et al., CVPR 2023): the text tower owns the prompts -- a shallow context ctx [1, P, dt] and
    one deep context per block, compound_prompts_text [D, P, dt] -- and every visual prompt is a trainable Linear(dt -> dv) of the text prompt of
    the same depth, with its own weights per depth: proj_weight [1 + D, dv, dt], proj_bias [1 + D, dv] (slice 0 couples ctx, slice l block l's
    deep prompt; each initialised as nn.Linear initialises its own).  Both towers read them through the existing deep calls.  MaPLe appends its
    visual prompts after the patch tokens, this engine inserts prompts after CLS: prompt rows carry no positional embedding and the ViT's
    attention has no mask, so it is the same function up to f32 summation order.  Parameters and coupling arithmetic are f32 (MaPLe runs fp16;
    its rounding points are not modelled).  compound_prompts_text None (D = 0): only the shallow pair, through the shallow tower calls.
    forward(x, classes) -> (text_out, visual_out), un-normalised: UPTModel's contract, so steps.upt_step / GraphedUptStep serve it as they are."""

    def __init__(self, ctx, compound_prompts_text, image_encoder, text_encoder, classes, temperature=0.07, device="cpu", dtype=torch.float32,
                 vision_width=None):
        super().__init__()
        self.device = device
        self.classes = classes
        self.temperature = temperature
        self.dtype = dtype
        if ctx.dim() != 3 or ctx.shape[0] != 1:
            raise ValueError(f"MaPLeModel: ctx has shape {tuple(ctx.shape)}, expected [1, P, text_width] (one shared context)")
        self.ctx = nn.Parameter(ctx)
        P, dt = ctx.shape[1], ctx.shape[2]
        if compound_prompts_text is not None and (compound_prompts_text.dim() != 3 or tuple(compound_prompts_text.shape[1:]) != (P, dt)):
            raise ValueError(f"MaPLeModel: compound_prompts_text has shape {tuple(compound_prompts_text.shape)}, expected [D, {P}, {dt}]")
        self.compound_prompts_text = nn.Parameter(compound_prompts_text) if compound_prompts_text is not None else None
        self.n_deep = 0 if compound_prompts_text is None else compound_prompts_text.shape[0]
        if vision_width is None:
            vision_width = image_encoder.visual.conv1.weight.shape[0]
        lin = [nn.Linear(dt, int(vision_width), dtype=dtype) for _ in range(1 + self.n_deep)]      # nn.Linear's own initialisation, depth by depth
        self.proj_weight = nn.Parameter(torch.stack([l.weight.detach() for l in lin]).to(device))
        self.proj_bias = nn.Parameter(torch.stack([l.bias.detach() for l in lin]).to(device))
        self.image_encoder = image_encoder
        self.text_encoder = text_encoder

    def _native_couple_ok(self):
        """The native coupling kernel (csrc/couple.hip) covers f32 on the GPU, up to 16 prompt tokens and 31 deep sets, widths that are multiples
        of 64 up to 1024.  Any other shape -- and GRIP_NATIVE_COUPLE=0 -- runs the same products through the framework's linear."""
        import os
        ts = [self.ctx, self.proj_weight, self.proj_bias] + ([] if self.compound_prompts_text is None else [self.compound_prompts_text])
        dv, dt = self.proj_weight.shape[1], self.proj_weight.shape[2]
        return (os.environ.get("GRIP_NATIVE_COUPLE", "1") != "0" and all(t.is_cuda and t.dtype == torch.float32 for t in ts)
                and self.ctx.shape[1] <= 16 and self.n_deep <= 31 and dt % 64 == 0 and dv % 64 == 0 and dt <= 1024 and dv <= 1024)

    def couple(self):
        """(ctx [1, P, dt], deep_text [D, P, dt] or None, vis_prefix [P, dv], vis_deep [D, P, dv] or None): what the two towers read."""
        deep = self.compound_prompts_text
        if self._native_couple_ok():
            from ..engine import PromptCoupleFn
            out = PromptCoupleFn.apply(self.ctx, deep, self.proj_weight, self.proj_bias)
            vis_prefix, vis_deep = (out, None) if deep is None else out
            return self.ctx, deep, vis_prefix, vis_deep
        linear = torch.nn.functional.linear
        vis_prefix = linear(self.ctx[0], self.proj_weight[0], self.proj_bias[0])
        vis_deep = None if deep is None else torch.stack([linear(deep[l], self.proj_weight[l + 1], self.proj_bias[l + 1]) for l in range(self.n_deep)])
        return self.ctx, deep, vis_prefix, vis_deep

    def forward(self, x, classes):
        ctx, deep_text, vis_prefix, vis_deep = self.couple()
        tkw = {} if deep_text is None else {"deep_prompts": deep_text}
        vkw = {} if vis_deep is None else {"deep_prompts": vis_deep}
        if x.is_cuda:
            # the towers on two streams, as UPTModel.forward
            main = torch.cuda.current_stream()
            side = _side_stream(x.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                visual_out = self.image_encoder(x, vis_prefix, **vkw)
            vis_prefix.record_stream(side)
            if vis_deep is not None:
                vis_deep.record_stream(side)
            text_out = self.text_encoder(ctx, classes, **tkw)
            main.wait_stream(side)
            visual_out.record_stream(main)
            return text_out, visual_out
        text_out = self.text_encoder(ctx, classes, **tkw)
        visual_out = self.image_encoder(x, vis_prefix, **vkw)
        return text_out, visual_out
