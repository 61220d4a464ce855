"""Host side of the native towers: weight blobs, handles, workspaces, autograd glue.

torch is used for device memory, streams and autograd bookkeeping only; every FLOP of the
encoders, the head and the losses runs in libgrip_amd.so (csrc/*.hip).
"""
import ctypes
import math
import os
import weakref
from ctypes import byref, c_int64, c_size_t, c_uint64, c_void_p

import torch

from . import native
from .config import ClipDims


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(device):
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise native.GripError(
            "grip_amd runs only on an AMD GPU (device 'cuda' under PyTorch-ROCm); there is no CPU path. "
            f"Requested device: {device}")
    return device


_PINNING = []      # stack of lists: workspaces handed out while a HIP graph is being captured (see pin_workspaces)


class pin_workspaces:
    """Context manager around a HIP-graph capture (steps.GraphedStep): every workspace a tower hands out inside it is DEDICATED to
    that graph -- a train-mode one is never handed to another forward again (a replay would overwrite the activations an eager
    forward on the same workspace is still holding for its backward), an inference one is a private allocation (the shared
    inference workspace may be replaced by a larger one and freed under the graph).  The list it yields keeps them alive; the
    owner un-pins with release_pins when the graph dies."""

    def __enter__(self):
        self.pins = []
        _PINNING.append(self.pins)
        return self.pins

    def __exit__(self, *exc):
        _PINNING.pop()
        return False


def release_pins(pins):
    for tower, ws in pins:
        tower._pinned.pop(ws.data_ptr(), None)
    pins.clear()


class Tower:
    """One frozen CLIP tower (vision or text) living in two HBM blobs behind a native handle."""

    def __init__(self, kind, width, layers, heads, embed_dim, seq0, patch=0, resolution=0, vocab=0,
                 max_prefix=64, device="cuda", exact=False):
        self.device = require_gpu(device)
        self.lib = native.lib()
        self.precision = int(exact)  # grip_dims.precision: 0 f16 towers, 1 f32 (exact comparison mode), 2 split-f16 (the middle tier of screen-and-refine)
        self.exact = self.precision != 0     # f32 weights / activations / attention: inference only
        self.dims = native.Dims(kind, width, layers, heads, embed_dim, seq0, patch, resolution, vocab, max_prefix, self.precision)
        self.kind, self.width, self.embed_dim, self.seq0 = kind, width, embed_dim, seq0
        n16, n32 = c_int64(), c_int64()
        native.check(self.lib.grip_layout_size(byref(self.dims), byref(n16), byref(n32)))
        # the GEMM-operand blob: f16, or f32 elements in exact mode (same element offsets)
        self.blob16 = torch.zeros(n16.value, dtype=torch.float32 if self.exact else torch.float16, device=self.device)
        self.blob32 = torch.zeros(n32.value, dtype=torch.float32, device=self.device)
        self.slots = {}
        s, i = native.Slot(), 0
        while self.lib.grip_layout_slot(byref(self.dims), i, byref(s)) == 0:
            self.slots[s.name.decode()] = (s.dtype, s.derived, s.offset, s.rows, s.cols, s.ld)
            i += 1
        h = c_void_p()
        native.check(self.lib.grip_tower_create(byref(self.dims), _ptr(self.blob16), _ptr(self.blob32), byref(h)))
        self.handle = h
        self._ws = {}
        self._owners = {}
        self._pinned = {}        # data_ptr -> workspace dedicated to a captured HIP graph
        self._finalized = False

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.grip_tower_destroy(self.handle)
        except Exception:
            pass

    # ---- weights
    def primary_names(self):
        return [n for n, v in self.slots.items() if not v[1]]

    def view(self, name):
        """Tensor view (rows x cols, row stride ld) of a slot inside its blob."""
        dtype, _, off, rows, cols, ld = self.slots[name]
        blob = self.blob16 if dtype == 0 else self.blob32
        return blob.as_strided((rows, cols), (ld, 1), off)

    def load(self, name, tensor):
        v = self.view(name)
        v.copy_(tensor.reshape(v.shape).to(device=self.device, dtype=v.dtype))
        self._finalized = False

    def finalize(self):
        native.check(self.lib.grip_tower_finalize(self.handle, _stream()))
        self._finalized = True

    # ---- workspaces
    def workspace(self, batch, n_prefix, train, seq_len=0):
        """Inference workspaces are interchangeable (the largest is kept).  Train-mode workspaces hold the activations a
        backward still needs: each shape keeps a small pool, and a workspace whose forward is still waiting for its
        backward (its autograd ctx is alive and has not run) is never handed out again -- model(aug_1) and model(aug_2)
        before one loss.backward() get two workspaces instead of overwriting each other."""
        key = (batch, n_prefix, bool(train), seq_len)
        if train:
            pool = self._ws.setdefault(key, [])
            ws = next((w for w in pool if not self._busy(w)), None)
            if ws is None:
                nbytes = c_size_t()
                native.check(self.lib.grip_workspace_bytes(self.handle, batch, n_prefix, seq_len, 1, byref(nbytes)))
                ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=self.device)
                pool.append(ws)
            if _PINNING:
                self._pinned[ws.data_ptr()] = ws
                _PINNING[-1].append((self, ws))
            return ws
        if _PINNING:      # inside a graph capture: a private inference workspace (kept alive by the graph's owner)
            nbytes = c_size_t()
            native.check(self.lib.grip_workspace_bytes(self.handle, batch, n_prefix, seq_len, 0, byref(nbytes)))
            ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=self.device)
            _PINNING[-1].append((self, ws))
            return ws
        ws = self._ws.get(key)
        if ws is None:
            nbytes = c_size_t()
            native.check(self.lib.grip_workspace_bytes(self.handle, batch, n_prefix, seq_len, 0, byref(nbytes)))
            for k in [k for k in self._ws if not k[2]]:
                if self._ws[k].numel() >= nbytes.value:
                    return self._ws[k]
                del self._ws[k]
            ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _busy(self, ws):
        if ws.data_ptr() in self._pinned:
            return True
        owner = self._owners.get(ws.data_ptr())
        return owner is not None and owner() is not None

    def hold(self, ws, ctx):
        """Mark a train-mode workspace as owned by the autograd ctx of its forward until that ctx's backward ran
        (release) or the graph was dropped (the weak reference dies)."""
        self._owners[ws.data_ptr()] = weakref.ref(ctx)

    def release(self, ws):
        self._owners.pop(ws.data_ptr(), None)

    @staticmethod
    def _aligned(ws):
        off = (-ws.data_ptr()) % 256
        return c_void_p(ws.data_ptr() + off), ws.numel() - off

    # ---- forward / backward
    def vit_prefix(self, prefix, B):
        """The visual prompt as the native call takes it, following `image_prefix.expand(B, -1, -1)` of the reference
        (models/clip_encoders.py:148): (prefix f32 contiguous or None, n_prefix, per_image).  [P, d] and [1, P, d] are one prompt shared by the
        batch (passed as [P, d]); [B, P, d] is one prompt per image (GRIP_FWD_PER_IMAGE_PREFIX); any other leading size raises, as expand does."""
        if prefix is None:
            return None, 0, False
        P = prefix.shape[-2]
        if prefix.dim() == 3 and prefix.shape[0] != 1:
            if prefix.shape[0] != B or prefix.shape[2] != self.width:
                raise native.GripError(f"visual prompt of shape {tuple(prefix.shape)} for a batch of {B} images: expected [P, {self.width}], "
                                       f"[1, P, {self.width}] (shared) or [{B}, P, {self.width}] (one prompt per image)")
            return prefix.contiguous().float(), P, True
        return prefix.reshape(P, self.width).contiguous().float(), P, False

    def vit_deep(self, deep, P):
        """Deep visual prompts as the native call takes them: (deep f32 contiguous [D, P, d] or None, D).  deep[l - 1] replaces the prompt
        rows of the stream entering block l, 1 <= l <= D <= layers - 1 (grip_vit_forward_deep, include/grip_amd.h)."""
        if deep is None:
            return None, 0
        check_deep_prompts(deep, P, self.width, self.dims.layers)
        return deep.contiguous().float(), deep.shape[0]

    def vit_forward(self, images, prefix=None, train=False, pos_emb=True, deep=None):
        """CustomVisionTransformer.forward: images [B, 3, R, R]; prefix None, [P, d] / [1, P, d] (shared) or [B, P, d] (one prompt per image);
        deep None or [D, P, d] deep prompts (shared prompt only)."""
        if not self._finalized:
            self.finalize()
        assert self.kind == 0
        images = images.contiguous()
        if images.dtype not in (torch.float32, torch.float16):
            images = images.float()
        B = images.shape[0]
        prefix, P, per_image = self.vit_prefix(prefix, B)
        deep, D = self.vit_deep(deep, P)
        out = torch.empty(B, self.embed_dim, dtype=torch.float32, device=self.device)
        ws = self.workspace(B, P, train)
        p, n = self._aligned(ws)
        gen = c_uint64(0)
        flags = (native.FWD_TRAIN if train else 0) | (0 if pos_emb else native.FWD_NO_POS_EMB) | (native.FWD_PER_IMAGE_PREFIX if per_image else 0)
        if D:
            native.check(self.lib.grip_vit_forward_deep(self.handle, _ptr(images), int(images.dtype == torch.float16), _ptr(prefix), P, _ptr(deep), D, B,
                                                        _ptr(out), p, n, flags, byref(gen), _stream()))
        else:
            native.check(self.lib.grip_vit_forward(self.handle, _ptr(images), int(images.dtype == torch.float16), _ptr(prefix), P, B,
                                                   _ptr(out), p, n, flags, byref(gen), _stream()))
        ws.generation = gen.value
        ws.per_image = B if per_image else 0      # the backward's grad_prefix is [B, P, d] then (vit_backward checks it is given that shape)
        ws.n_deep = D                             # ... and grad_deep [D, P, d]
        return out, ws

    @torch.no_grad()
    def encode_chunks(self, images, out, lo, hi, chunk, prefix=None, streams=2, hilo=False, deep=None):
        """Inference encode of images[lo:hi] into out[0:hi-lo] in chunks, alternating between two HIP streams (each
        with its own workspace): the HBM-bound kernels of one chunk (LayerNorm, attention, patch gather) run next to
        the power-bound GEMMs of the other.  Rows are independent of the chunking, so the result is bit-identical to
        a single-stream pass (+6 % on the 50k-image pass).  streams=1 keeps everything on the current stream (per-kernel
        timings are only meaningful that way).  `images` is a tensor or a callable (a, b) -> tensor.
        hilo=True (f16 towers): the residual stream as a compensated f16 pair (GRIP_FWD_STREAM_HILO, include/grip_amd.h): the screen
        of the pseudolabel pass -- a different (more accurate) function of the image than the plain f16 stream's, equally chunk-independent.
        prefix: None, one prompt for every image ([P, d] / [1, P, d]), or one prompt per image aligned with `images`: [N, P, d] on any
        device, N >= hi; rows lo .. hi are read chunk by chunk with their images.
        deep: None or [D, P, d] deep prompts of a shared prompt (every image alike, so still chunk-independent)."""
        if not self._finalized:
            self.finalize()
        per_image = is_per_image_prefix(prefix)
        P = 0 if prefix is None else prefix.shape[-2]
        if per_image:
            if prefix.shape[0] < hi or prefix.shape[2] != self.width:
                raise native.GripError(f"per-image visual prompts of shape {tuple(prefix.shape)} do not cover images {lo} .. {hi} (width {self.width})")
        elif prefix is not None:
            prefix = prefix.reshape(P, self.width).contiguous().float()
        if deep is not None:
            if per_image:
                raise native.GripError("deep visual prompts need one prompt shared by every image, not per-image prompts")
            deep = deep.to(self.device)
        deep, D = self.vit_deep(deep, P)
        if not hasattr(self, "_enc_streams"):
            self._enc_streams = [torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)]
            self._enc_ws = {}
        nbytes = c_size_t()
        native.check(self.lib.grip_workspace_bytes(self.handle, min(chunk, max(hi - lo, 1)), P, 0, 0, byref(nbytes)))
        for k in (0, 1):
            if k not in self._enc_ws or self._enc_ws[k].numel() < nbytes.value + 256:
                self._enc_ws[k] = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=self.device)
        main = torch.cuda.current_stream()
        for st in self._enc_streams:
            st.wait_stream(main)
        if hasattr(images, "plan"):
            images.plan(lo, hi, chunk)      # lazy file pools decode one chunk ahead, never past the shard
        for i, s in enumerate(range(lo, hi, chunk)):
            e = min(s + chunk, hi)
            k = (i & 1) if streams == 2 else 0
            with torch.cuda.stream(self._enc_streams[k] if streams == 2 else main):
                x = images[s:e] if torch.is_tensor(images) else images(s, e)
                x = x.to(self.device, non_blocking=True).contiguous()
                if x.dtype not in (torch.float32, torch.float16):
                    x = x.float()
                if streams == 2:
                    x.record_stream(self._enc_streams[k])
                pre = prefix
                if per_image:       # this chunk's prompts, moved and cast on the chunk's stream like its images
                    pre = prefix[s:e].to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
                    if streams == 2:
                        pre.record_stream(self._enc_streams[k])
                o = out[s - lo: e - lo]
                p, n = self._aligned(self._enc_ws[k])
                flags = (native.FWD_STREAM_HILO if (hilo and self.precision == 0) else 0) | (native.FWD_PER_IMAGE_PREFIX if per_image else 0)
                st = c_void_p((self._enc_streams[k] if streams == 2 else main).cuda_stream)
                if D:
                    native.check(self.lib.grip_vit_forward_deep(self.handle, _ptr(x), int(x.dtype == torch.float16), _ptr(pre), P, _ptr(deep), D, e - s, _ptr(o),
                                                                p, n, flags, None, st))
                else:
                    native.check(self.lib.grip_vit_forward(self.handle, _ptr(x), int(x.dtype == torch.float16), _ptr(pre), P, e - s, _ptr(o), p, n,
                                                           flags, None, st))
        for st in self._enc_streams:
            main.wait_stream(st)
        return out

    def vit_backward(self, grad_emb, prefix, ws, generation=0):
        """Prompt gradient of the train-mode forward on `ws`: [P, d] for a shared prompt (summed over the batch), [B, P, d] for per-image prompts.
        After a forward with deep prompts: (prompt gradient, deep-prompt gradient [D, P, d] summed over the batch)."""
        grad_emb = grad_emb.contiguous().float()
        prefix, P, per_image = self.vit_prefix(prefix, grad_emb.shape[0])
        if getattr(ws, "per_image", 0) != (grad_emb.shape[0] if per_image else 0):
            raise native.GripError(f"vit_backward: the prompt of shape {tuple(prefix.shape)} is not the one the forward on this workspace read "
                                   f"({'per image, batch ' + str(ws.per_image) if getattr(ws, 'per_image', 0) else 'shared'})")
        g = torch.empty(prefix.shape, dtype=torch.float32, device=self.device)
        p, n = self._aligned(ws)
        D = getattr(ws, "n_deep", 0)
        if D:
            gd = torch.empty(D, P, self.width, dtype=torch.float32, device=self.device)
            native.check(self.lib.grip_vit_backward_deep(self.handle, _ptr(grad_emb), _ptr(prefix), _ptr(g), _ptr(gd), p, n, generation, _stream()))
            return g, gd
        native.check(self.lib.grip_vit_backward_prefix(self.handle, _ptr(grad_emb), _ptr(prefix), _ptr(g), p, n, generation, _stream()))
        return g

    # Encode only the positions up to the longest prompt's EOT: the text transformer is causal and only the EOT row is
    # read, so later positions cannot influence any output (exact; the reference encodes all 77).
    truncate_text_at_eot = True

    def text_deep(self, deep, pc, P):
        """Deep text prompts as the native call takes them: (deep f32 contiguous [D, pc, P, d] or None, D).  deep[l - 1] replaces the context rows of the
        stream entering block l, 1 <= l <= D <= layers - 1 (grip_text_forward_deep, include/grip_amd.h).  A shared context (pc == 1) takes [D, P, d] or
        [D, 1, P, d], a class-specific one [D, C, P, d]."""
        if deep is None:
            return None, 0
        check_text_deep_prompts(deep, pc, P, self.width, self.dims.layers)
        return deep.reshape(deep.shape[0], pc, P, self.width).contiguous().float(), deep.shape[0]

    def text_forward(self, token_ids, prefix=None, train=False, seq_len=None, pos_emb=True, deep=None):
        """CustomTextEncoder.forward: prefix None or [pc, P, d] (pc = 1: one context for every class, or one per class); deep None or the deep
        prompts of that context (text_deep)."""
        if not self._finalized:
            self.finalize()
        assert self.kind == 1
        # int32 ids and EOT row indices are kept on the token tensor (keyed by its version counter: an in-place edit recomputes
        # them) -- a prompt step would otherwise spend three tiny launches per forward re-deriving the same indices
        memo = getattr(token_ids, "_grip_ids", None)
        if memo is not None and memo[0] == token_ids._version and memo[1].device == self.device:
            ids, eot = memo[1], memo[2]
        else:
            ids = token_ids.to(device=self.device, dtype=torch.int32).contiguous()
            eot = ids.argmax(dim=-1).to(torch.int32).contiguous()
            token_ids._grip_ids = (token_ids._version, ids, eot)
        C = ids.shape[0]
        if seq_len is None:
            seq_len = min(int(eot.max().item()) + 1, self.seq0) if self.truncate_text_at_eot else 0
        P, pc = 0, 1
        if prefix is not None:
            pc, P = prefix.shape[0], prefix.shape[1]
            prefix = prefix.contiguous().float()
        deep, D = self.text_deep(deep, pc, P)
        flags = (native.FWD_TRAIN if train else 0) | (0 if pos_emb else native.FWD_NO_POS_EMB)
        if P and pc == 1 and not self.exact and self.share_text_prefix and self._shares_prefix(token_ids, ids, eot, P):
            flags |= native.FWD_SHARED_PREFIX
        self.last_text_flags = flags
        out = torch.empty(C, self.embed_dim, dtype=torch.float32, device=self.device)
        ws = self.workspace(C, P, train, seq_len)
        p, n = self._aligned(ws)
        gen = c_uint64(0)
        if D:
            native.check(self.lib.grip_text_forward_deep(self.handle, _ptr(ids), _ptr(eot), _ptr(prefix), P, pc, _ptr(deep), D, C, seq_len, _ptr(out), p, n,
                                                         flags, byref(gen), _stream()))
        else:
            native.check(self.lib.grip_text_forward(self.handle, _ptr(ids), _ptr(eot), _ptr(prefix), P, pc, C, seq_len, _ptr(out), p, n,
                                                    flags, byref(gen), _stream()))
        ws.generation = gen.value
        ws.n_deep = D         # the backward then returns grad_deep [D, pc, P, d] as well
        return out, ws, (ids, eot, seq_len)

    # One shared context (CoOp / UPT text side): positions 0 .. P hold the same tokens for every class and the mask is causal, so
    # the engine encodes them once (include/grip_amd.h, GRIP_FWD_SHARED_PREFIX).  GRIP_TEXT_SHARED_PREFIX=0 keeps the plain
    # n_class x seq_len layout (developer A/B; the tests hold the two equal).
    share_text_prefix = os.environ.get("GRIP_TEXT_SHARED_PREFIX", "1") != "0"

    @staticmethod
    def _shares_prefix(token_ids, ids, eot, P):
        """True when every class has the same tokens at positions 0 .. P and its EOT after them (checked once per token tensor
        and context length, remembered with the tensor's version counter)."""
        memo = getattr(token_ids, "_grip_shared", None)
        if memo is not None and memo[0] == token_ids._version and memo[1] == P:
            return memo[2]
        ok = bool(ids.shape[0] >= 2 and ids.shape[1] > P + 1 and (ids[:, :P + 1] == ids[:1, :P + 1]).all().item() and int(eot.min().item()) > P)
        token_ids._grip_shared = (token_ids._version, P, ok)
        return ok

    def text_backward(self, grad_emb, prefix_shape, ws, generation=0):
        """Context gradient [pc, P, d] of the train-mode forward on `ws` (summed over the classes when pc == 1).  After a forward with deep prompts:
        (context gradient, deep-prompt gradient [D, pc, P, d])."""
        grad_emb = grad_emb.contiguous().float()
        g = torch.empty(prefix_shape, dtype=torch.float32, device=self.device)
        p, n = self._aligned(ws)
        D = getattr(ws, "n_deep", 0)
        if D:
            gd = torch.empty((D,) + tuple(prefix_shape), dtype=torch.float32, device=self.device)
            native.check(self.lib.grip_text_backward_deep(self.handle, _ptr(grad_emb), _ptr(g), _ptr(gd), p, n, generation, _stream()))
            return g, gd
        native.check(self.lib.grip_text_backward_prefix(self.handle, _ptr(grad_emb), _ptr(g), p, n, generation, _stream()))
        return g


def check_deep_prompts(deep, P, width, layers):
    """Deep visual prompts must be [D, P, width] with 1 <= D <= layers - 1: the shallow prompt's token count P (they replace its rows) and one
    prompt per block after the first.  Raises GripError otherwise."""
    if deep.dim() != 3 or deep.shape[1] != P or deep.shape[2] != width or not 1 <= deep.shape[0] <= layers - 1:
        raise native.GripError(f"deep visual prompts of shape {tuple(deep.shape)}: expected [D, {P}, {width}] with 1 <= D <= {layers - 1} "
                               f"(the shallow prompt's P = {P} and width; one prompt per block after the first)")


def check_text_deep_prompts(deep, pc, P, width, layers):
    """Deep text prompts must be [D, P, width] or [D, 1, P, width] for one shared context (pc == 1), [D, C, P, width] for a class-specific one (pc == C),
    with 1 <= D <= layers - 1 and the shallow context's token count P (they replace its rows).  Raises GripError otherwise."""
    ok = torch.is_tensor(deep) and deep.dim() in (3, 4) and P > 0 and 1 <= deep.shape[0] <= layers - 1 and (
        tuple(deep.shape[1:]) == (pc, P, width) or (pc == 1 and tuple(deep.shape[1:]) == (P, width)))
    if not ok:
        want = f"[D, {P}, {width}] (or [D, 1, {P}, {width}])" if pc == 1 else f"[D, {pc}, {P}, {width}]"
        raise native.GripError(f"deep text prompts of shape {tuple(deep.shape) if torch.is_tensor(deep) else type(deep).__name__}: expected {want} with "
                               f"1 <= D <= {layers - 1} (the shallow context's {'one shared set' if pc == 1 else 'C = ' + str(pc) + ' per-class sets'} of "
                               f"P = {P} tokens and width; one prompt per block after the first)")


def is_per_image_prefix(prefix):
    """True for a visual prompt tensor that holds one prompt per image ([B, P, d] with B != 1); [P, d] and [1, P, d] are shared."""
    return torch.is_tensor(prefix) and prefix.dim() == 3 and prefix.shape[0] != 1


def vision_tower(d: ClipDims, device="cuda", max_prefix=64, exact=False):
    return Tower(0, d.vision_width, d.vision_layers, d.vision_heads, d.embed_dim, d.vision_seq, d.vision_patch_size,
                 d.image_resolution, 0, max_prefix, device, exact)


def text_tower(d: ClipDims, device="cuda", max_prefix=64, exact=False):
    return Tower(1, d.transformer_width, d.transformer_layers, d.transformer_heads, d.embed_dim, d.context_length, 0, 0,
                 d.vocab_size, max_prefix, device, exact)


# ------------------------------------------------------------------------------------------ autograd
class VitPrefixFn(torch.autograd.Function):
    """CustomVisionTransformer.forward with autograd to the visual prompt only (frozen backbone).  The prompt follows the reference's
    image_prefix.expand(B, -1, -1): [P, d] / [1, P, d] shared by the batch, or [B, P, d] one prompt per image; the gradient comes back in
    the prompt's own shape and dtype ([B, P, d]: each image's own gradient, no sum over the batch).  The HIP-graph training steps
    (steps.GraphedVptStep) capture shared prompts only: a per-image prompt runs this function eagerly."""

    @staticmethod
    def forward(ctx, tower, images, prefix, pos_emb=True, deep=None):
        need = ctx.needs_input_grad[2] or (deep is not None and ctx.needs_input_grad[4])   # grad mode is off inside Function.forward
        if need and tower.exact:
            raise native.GripError("exact (f32) towers are inference-only: prompt gradients need a default-precision tower")
        out, ws = tower.vit_forward(images, prefix.detach(), train=need, pos_emb=pos_emb, deep=None if deep is None else deep.detach())
        ctx.tower, ctx.ws, ctx.generation = tower, ws, ws.generation
        if need:
            tower.hold(ws, ctx)
        ctx.save_for_backward(prefix.detach())
        ctx.pshape, ctx.pdtype = prefix.shape, prefix.dtype
        ctx.dshape, ctx.ddtype = (None, None) if deep is None else (deep.shape, deep.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (prefix,) = ctx.saved_tensors
        g = ctx.tower.vit_backward(grad_out, prefix, ctx.ws, ctx.generation)
        ctx.tower.release(ctx.ws)
        if ctx.dshape is None:
            return None, None, g.reshape(ctx.pshape).to(ctx.pdtype), None
        g, gd = g
        return None, None, g.reshape(ctx.pshape).to(ctx.pdtype), None, gd.reshape(ctx.dshape).to(ctx.ddtype)


class TextPrefixFn(torch.autograd.Function):
    """CustomTextEncoder.forward with autograd to the textual prompt only -- and, when given, to its deep prompts (the gradient in deep's own
    shape and dtype)."""

    @staticmethod
    def forward(ctx, tower, token_ids, prefix, pos_emb=True, deep=None):
        need = ctx.needs_input_grad[2] or (deep is not None and ctx.needs_input_grad[4])
        if need and tower.exact:
            raise native.GripError("exact (f32) towers are inference-only: prompt gradients need a default-precision tower")
        cached = getattr(token_ids, "_grip_seq_len", None)
        out, ws, keep = tower.text_forward(token_ids, prefix.detach(), train=need, seq_len=cached, pos_emb=pos_emb, deep=None if deep is None else deep.detach())
        token_ids._grip_seq_len = keep[2]
        ctx.tower, ctx.ws, ctx.generation = tower, ws, ws.generation
        if need:
            tower.hold(ws, ctx)
        ctx.keep = keep   # the native handle remembers the EOT-index pointer until backward
        ctx.pshape, ctx.pdtype = prefix.shape, prefix.dtype
        ctx.dshape, ctx.ddtype = (None, None) if deep is None else (deep.shape, deep.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.tower.text_backward(grad_out, tuple(ctx.pshape), ctx.ws, ctx.generation)
        ctx.tower.release(ctx.ws)
        if ctx.dshape is None:
            return None, None, g.to(ctx.pdtype), None
        g, gd = g
        return None, None, g.to(ctx.pdtype), None, gd.reshape(ctx.dshape).to(ctx.ddtype)


def vit_prefix_forward(tower, images, prefix, pos_emb=True, deep=None):
    """CustomVisionTransformer.forward on the native tower.  The train-mode forward (activations saved for the prompt
    gradient) runs only when a gradient can actually be asked for: grad mode on AND the prompt requires grad.  Under
    torch.no_grad() -- validation, test predictions, the pseudolabel passes -- it is the plain inference forward, the same
    arithmetic as the pool encode (autograd's needs_input_grad alone does not see the surrounding no_grad).
    deep: None or [D, P, d] deep prompts (VPT-Deep); differentiable as well, the gradient in deep's shape and dtype."""
    if deep is None:
        if torch.is_grad_enabled() and prefix.requires_grad:
            return VitPrefixFn.apply(tower, images, prefix, pos_emb)
        return tower.vit_forward(images, prefix.detach(), train=False, pos_emb=pos_emb)[0]
    if torch.is_grad_enabled() and (prefix.requires_grad or deep.requires_grad):
        return VitPrefixFn.apply(tower, images, prefix, pos_emb, deep)
    return tower.vit_forward(images, prefix.detach(), train=False, pos_emb=pos_emb, deep=deep.detach())[0]


def text_prefix_forward(tower, token_ids, prefix, pos_emb=True, deep=None):
    """CustomTextEncoder.forward on the native tower; see vit_prefix_forward.  pos_emb=False is the reference's enable_pos_emb=False
    branch (models/clip_encoders.py:70-74): the positional embedding is not added (the positions' gradient path is untouched: it is additive).
    deep: None or the context's deep prompts ([D, P, d] / [D, 1, P, d] shared, [D, C, P, d] per class; Tower.text_deep); differentiable as well."""
    if deep is None:
        if torch.is_grad_enabled() and prefix.requires_grad:
            return TextPrefixFn.apply(tower, token_ids, prefix, pos_emb)
    elif torch.is_grad_enabled() and (prefix.requires_grad or deep.requires_grad):
        return TextPrefixFn.apply(tower, token_ids, prefix, pos_emb, deep)
    cached = getattr(token_ids, "_grip_seq_len", None)
    out, _, keep = tower.text_forward(token_ids, prefix.detach(), train=False, seq_len=cached, pos_emb=pos_emb, deep=None if deep is None else deep.detach())
    token_ids._grip_seq_len = keep[2]
    return out


def cosine_head(img_emb, txt_emb, scale, want_probs=True):
    """normalize -> scale * img @ txt.T -> softmax / argmax, fused (no autograd)."""
    lib = native.lib()
    img = img_emb.detach().contiguous().float()
    txt = txt_emb.detach().contiguous().float()
    n, e = img.shape
    c = txt.shape[0]
    dev = img.device
    logits = torch.empty(n, c, dtype=torch.float32, device=dev)
    probs = torch.empty(n, c, dtype=torch.float32, device=dev) if want_probs else None
    am_l = torch.empty(n, dtype=torch.int32, device=dev)
    am_p = torch.empty(n, dtype=torch.int32, device=dev) if want_probs else None
    scratch = torch.empty(c, e, dtype=torch.float32, device=dev)
    native.check(lib.grip_cosine_head(_ptr(img), _ptr(txt), float(scale), n, c, e, _ptr(logits), _ptr(probs), _ptr(am_l), _ptr(am_p),
                                      _ptr(scratch), _stream()))
    return logits, probs, am_l, am_p


class CosineHeadFn(torch.autograd.Function):
    """logits = scale * normalize(img) @ normalize(txt).T with native forward and backward."""

    @staticmethod
    def forward(ctx, img_emb, txt_emb, scale):
        logits, _, _, _ = cosine_head(img_emb, txt_emb, scale, want_probs=False)
        ctx.save_for_backward(img_emb.detach(), txt_emb.detach())
        ctx.scale = float(scale)
        ctx.need = (img_emb.requires_grad, txt_emb.requires_grad)
        return logits

    @staticmethod
    def backward(ctx, grad_logits):
        img, txt = ctx.saved_tensors
        lib = native.lib()
        img = img.contiguous().float()
        txt = txt.contiguous().float()
        n, e = img.shape
        c = txt.shape[0]
        g = grad_logits.contiguous().float()
        gi = torch.empty_like(img) if ctx.need[0] else None
        gt = torch.empty_like(txt) if ctx.need[1] else None
        native.check(lib.grip_cosine_head_backward(_ptr(img), _ptr(txt), ctx.scale, n, c, e, _ptr(g), _ptr(gi), _ptr(gt), _stream()))
        return gi, gt, None


class WeightedCEFn(torch.autograd.Function):
    """sum_i w_i * CE(logits_i, label_i), native forward+backward (one kernel produces both)."""

    @staticmethod
    def forward(ctx, logits, labels, row_weight):
        lib = native.lib()
        lg = logits.contiguous().float()
        n, c = lg.shape
        lab = labels.to(device=lg.device, dtype=torch.int32).contiguous()
        w = row_weight.to(device=lg.device, dtype=torch.float32).contiguous()
        loss = torch.zeros(1, dtype=torch.float32, device=lg.device)
        grad = torch.empty_like(lg)
        native.check(lib.grip_weighted_ce(_ptr(lg), _ptr(lab), _ptr(w), n, c, _ptr(loss), _ptr(grad), _stream()))
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


_COL_MAPS_OK = []       # [(weakref of a col_map tensor, its version counter, c)] that passed the host check of soft_ce, most recent first


def _check_col_map(col_map, c, who="soft_ce"):
    """col_map (int32 [cz] on the device) is injective into [0, c): checked on the host ONCE per tensor (and per version of it) -- a later call with the
    same tensor costs no device read, so a step may run under graph capture once its warm-up has passed here."""
    import weakref
    for ref, version, cc in _COL_MAPS_OK:
        held = ref()        # (alive: its memory has not been handed to another tensor since the check)
        if held is not None and held.data_ptr() == col_map.data_ptr() and held.numel() == col_map.numel() and version == col_map._version and cc == c:
            return
    host = col_map.cpu()
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= c or torch.unique(host).numel() != host.numel()):
        raise native.GripError(f"{who}: col_map must hold distinct logits columns in [0, {c}), got {host.tolist()}")
    _COL_MAPS_OK.insert(0, (weakref.ref(col_map), col_map._version, c))
    del _COL_MAPS_OK[8:]


def soft_ce(logits, labels, row_weight, soft=None, soft_row=None, col_map=None, temperature=1.0, smoothing=0.0, want_target=False):
    """(loss, grad[, target]) of the weighted cross-entropy against soft targets (csrc/soft_ce.hip, grip_soft_ce): batch row i with
    0 <= soft_row[i] < soft.shape[0] trains on softmax((1 / temperature) log max(soft[soft_row[i]], 2^-126)) scattered to the logits columns
    col_map[j], every other row on onehot(labels[i]); every target is smoothed, t = (1 - smoothing) s + smoothing / c.  loss: 0-d f32,
    sum_i w_i (T_i lse_i - <t_i, x_i>); grad [n, c] = w_i (T_i softmax(x_i) - t_i); target [n, c] = t with want_target.  `soft` (f32 [rows, cz]) is read in
    place: no [n, c] target block is built on the host.  soft=None with smoothing 0 gives grip_weighted_ce's bits.  No autograd (SoftCEFn)."""
    lib = native.lib()
    if not torch.is_tensor(logits) or logits.dim() != 2 or not logits.is_cuda:
        raise native.GripError(f"soft_ce: logits must be a [n, c] tensor on the GPU, got {getattr(logits, 'shape', type(logits))}")
    lg = logits.detach().contiguous().float()
    n, c = lg.shape
    dev = lg.device
    if not torch.is_tensor(labels) or tuple(labels.shape) != (n,) or labels.dtype.is_floating_point:
        raise native.GripError(f"soft_ce: labels must be an integer [{n}] tensor, got {getattr(labels, 'shape', type(labels))} {getattr(labels, 'dtype', None)}")
    if not torch.is_tensor(row_weight) or tuple(row_weight.shape) != (n,) or not row_weight.dtype.is_floating_point:
        raise native.GripError(f"soft_ce: row_weight must be a floating-point [{n}] tensor, got {getattr(row_weight, 'shape', type(row_weight))}")
    lab = labels.to(device=dev, dtype=torch.int32).contiguous()
    w = row_weight.to(device=dev, dtype=torch.float32).contiguous()
    rows = cz = 0
    if soft is not None:
        if not torch.is_tensor(soft) or soft.dim() != 2 or soft.dtype != torch.float32 or soft.device != dev or not soft.is_contiguous():
            raise native.GripError(f"soft_ce: soft must be a contiguous float32 [rows, cz] tensor on {dev} (it is read in place), got "
                                   f"{getattr(soft, 'shape', type(soft))} {getattr(soft, 'dtype', None)} on {getattr(soft, 'device', None)}")
        rows, cz = soft.shape
        soft_row = _gmm_operand("soft_ce", "soft_row", soft_row, (n,), lg, torch.int32)
        if not torch.is_tensor(col_map) or tuple(col_map.shape) != (cz,) or col_map.dtype != torch.int32 or col_map.device != dev or not col_map.is_contiguous():
            raise native.GripError(f"soft_ce: col_map must be a contiguous int32 [{cz}] tensor on {dev}, got {getattr(col_map, 'shape', type(col_map))} "
                                   f"{getattr(col_map, 'dtype', None)}")
        if not 1 <= cz <= c:
            raise native.GripError(f"soft_ce: soft has {cz} columns for {c} logits columns (1 .. c)")
        _check_col_map(col_map, c)
    else:
        soft_row = col_map = None
    if not 0.0 < float(temperature) < float("inf"):
        raise native.GripError(f"soft_ce: temperature = {temperature} (a finite temperature > 0)")
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    grad = torch.empty_like(lg)
    target = torch.empty_like(lg) if want_target else None
    native.check(lib.grip_soft_ce(_ptr(lg), _ptr(lab), _ptr(w), n, c, _ptr(soft), rows, cz, _ptr(soft_row), _ptr(col_map), 1.0 / float(temperature),
                                  float(smoothing), _ptr(loss), _ptr(grad), _ptr(target), _stream()))
    return (loss[0], grad, target) if want_target else (loss[0], grad)


class SoftCEFn(torch.autograd.Function):
    """WeightedCEFn's twin on soft targets: sum_i w_i CE(logits_i, t_i) with t of engine.soft_ce, native forward + backward (one kernel produces both).
    apply(logits, labels, row_weight, soft, soft_row, col_map, temperature, smoothing)."""

    @staticmethod
    def forward(ctx, logits, labels, row_weight, soft, soft_row, col_map, temperature, smoothing):
        loss, grad = soft_ce(logits, labels, row_weight, soft, soft_row, col_map, temperature, smoothing)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g,) + (None,) * 7


CANDIDATE_COMBINE = {"intersection": 0, "union": 1, "intra": 2, "inter": 3}      # grip_candidate_select's combine


def candidate_select(probs, claim, tau=0.99, combine="intersection"):
    """(mask int32 [n, ceil(c / 32)], count int32 [n], label int32 [n], threshold f32 [c]): the candidate pseudolabel sets of include/grip_amd.h on the
    native kernels (csrc/candidate.hip).  threshold[c] is the claim-th largest value of column c, exact; the INTER set of a row holds the classes whose
    threshold the row reaches, the INTRA set the smallest prefix of its classes (probability descending, index ascending) whose f32 running sum reaches
    tau; `combine` ("intersection", "union", "intra", "inter") joins them.  Class j is bit j % 32 of mask word j // 32; label is the member of highest
    rank, -1 for an empty set.  probs must be finite and >= 0.  Bit-identical from call to call."""
    if not torch.is_tensor(probs) or probs.dim() != 2 or not probs.is_floating_point():
        raise native.GripError(f"candidate_select: probs must be a floating-point [n, c] tensor, got {getattr(probs, 'shape', type(probs))}")
    n, c = probs.shape
    require_gpu(probs.device)
    if combine not in CANDIDATE_COMBINE:
        raise native.GripError(f"candidate_select: combine = {combine!r} (one of {sorted(CANDIDATE_COMBINE)})")
    if isinstance(claim, bool) or not isinstance(claim, int) or not 1 <= claim <= max(n, 1):
        raise native.GripError(f"candidate_select: claim = {claim!r} (an integer in [1, n = {n}])")
    if not 0.0 < float(tau) <= 1.0:
        raise native.GripError(f"candidate_select: tau = {tau} (in (0, 1])")
    p = probs.detach().contiguous().float()
    lib = native.lib()
    nbytes = c_size_t()
    native.check(lib.grip_candidate_select_workspace(n, c, byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=p.device)
    mask = torch.empty(n, (c + 31) // 32, dtype=torch.int32, device=p.device)
    count = torch.empty(n, dtype=torch.int32, device=p.device)
    label = torch.empty(n, dtype=torch.int32, device=p.device)
    threshold = torch.empty(c, dtype=torch.float32, device=p.device)
    native.check(lib.grip_candidate_select(_ptr(p), n, c, int(claim), float(tau), CANDIDATE_COMBINE[combine], _ptr(threshold), _ptr(mask), _ptr(count),
                                           _ptr(label), _ptr(ws), ws.numel(), _stream()))
    return mask, count, label, threshold


def candidate_ce(logits, labels, row_weight, cand=None, cand_row=None, col_map=None):
    """(loss, grad) of the weighted partial-label cross-entropy (csrc/candidate.hip, grip_candidate_ce): batch row i with 0 <= cand_row[i] < cand.shape[0]
    trains on the candidate SET in that row of the mask matrix `cand` (int32 [rows, ceil(cz / 32)], candidate_select's layout; mask column j is logits
    column col_map[j]): loss_i = w_i (lse(x_i) - lse_S(x_i)), grad_i = w_i (softmax(x_i) - softmax_S(x_i)); an empty set contributes nothing.  Every other
    row trains on labels[i] as grip_weighted_ce does.  loss: 0-d f32; grad [n, c].  `cand` is read in place.  cand=None gives grip_weighted_ce's bits.
    No autograd (CandidateCEFn)."""
    lib = native.lib()
    if not torch.is_tensor(logits) or logits.dim() != 2 or not logits.is_cuda:
        raise native.GripError(f"candidate_ce: logits must be a [n, c] tensor on the GPU, got {getattr(logits, 'shape', type(logits))}")
    lg = logits.detach().contiguous().float()
    n, c = lg.shape
    dev = lg.device
    if not torch.is_tensor(labels) or tuple(labels.shape) != (n,) or labels.dtype.is_floating_point:
        raise native.GripError(f"candidate_ce: labels must be an integer [{n}] tensor, got {getattr(labels, 'shape', type(labels))} "
                               f"{getattr(labels, 'dtype', None)}")
    if not torch.is_tensor(row_weight) or tuple(row_weight.shape) != (n,) or not row_weight.dtype.is_floating_point:
        raise native.GripError(f"candidate_ce: row_weight must be a floating-point [{n}] tensor, got {getattr(row_weight, 'shape', type(row_weight))}")
    lab = labels.to(device=dev, dtype=torch.int32).contiguous()
    w = row_weight.to(device=dev, dtype=torch.float32).contiguous()
    rows = cz = 0
    if cand is not None:
        if not torch.is_tensor(col_map) or col_map.dim() != 1 or col_map.dtype != torch.int32 or col_map.device != dev or not col_map.is_contiguous():
            raise native.GripError(f"candidate_ce: col_map must be a contiguous int32 [cz] tensor on {dev}, got {getattr(col_map, 'shape', type(col_map))} "
                                   f"{getattr(col_map, 'dtype', None)}")
        cz = col_map.shape[0]
        if not 1 <= cz <= c:
            raise native.GripError(f"candidate_ce: col_map names {cz} mask columns for {c} logits columns (1 .. c)")
        words = (cz + 31) // 32
        if not torch.is_tensor(cand) or cand.dim() != 2 or cand.shape[1] != words or cand.dtype != torch.int32 or cand.device != dev or not cand.is_contiguous():
            raise native.GripError(f"candidate_ce: cand must be a contiguous int32 [rows, {words}] tensor on {dev} (it is read in place), got "
                                   f"{getattr(cand, 'shape', type(cand))} {getattr(cand, 'dtype', None)} on {getattr(cand, 'device', None)}")
        rows = cand.shape[0]
        cand_row = _gmm_operand("candidate_ce", "cand_row", cand_row, (n,), lg, torch.int32)
        _check_col_map(col_map, c, "candidate_ce")
    else:
        cand_row = col_map = None
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    grad = torch.empty_like(lg)
    native.check(lib.grip_candidate_ce(_ptr(lg), _ptr(lab), _ptr(w), n, c, _ptr(cand), rows, cz, _ptr(cand_row), _ptr(col_map), _ptr(loss), _ptr(grad),
                                       _stream()))
    return loss[0], grad


class CandidateCEFn(torch.autograd.Function):
    """SoftCEFn's twin on candidate sets: sum_i w_i (lse(x_i) - lse_S(x_i)) of engine.candidate_ce, native forward + backward (one kernel produces both).
    apply(logits, labels, row_weight, cand, cand_row, col_map)."""

    @staticmethod
    def forward(ctx, logits, labels, row_weight, cand, cand_row, col_map):
        loss, grad = candidate_ce(logits, labels, row_weight, cand, cand_row, col_map)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g,) + (None,) * 5


class UptMixerFn(torch.autograd.Function):
    """UPTModel's prompt mixer (models/prompts_models.py:129-146) on the native kernels (csrc/mixer.hip): forward and the
    gradients of all 22 tensors -- the two prompt embeddings, the four projections and the one-block transformer.  A 23rd tensor,
    vpt_embeddings_deep [D, P, dv], makes it the deep mixer (grip_upt_mixer_*_deep: the sequence grows to 2 + D tokens); it then
    returns (coop, vpt, vpt_deep) and that tensor's gradient too."""

    @staticmethod
    def forward(ctx, *tensors):
        lib = native.lib()
        ts = [t.detach().contiguous().float() for t in tensors]
        coop, vpt = ts[0].reshape(-1, ts[0].shape[-1]), ts[1].reshape(-1, ts[1].shape[-1])
        P, dt, dv, D = coop.shape[0], coop.shape[1], vpt.shape[1], ts[2].shape[0]
        if vpt.shape[0] != P:
            raise native.GripError(f"UPT mixer: {P} text prompt tokens but {vpt.shape[0]} visual ones (the reference concatenates them along dim 0)")
        deep = ts[22] if len(ts) > 22 else None
        if deep is not None and (deep.dim() != 3 or tuple(deep.shape[1:]) != (P, dv)):
            raise native.GripError(f"UPT mixer: vpt_embeddings_deep has shape {tuple(deep.shape)}, expected [D, {P}, {dv}]")
        nd = 0 if deep is None else deep.shape[0]
        dev = coop.device
        nbytes = c_size_t()
        if deep is None:
            native.check(lib.grip_upt_mixer_workspace(P, dt, dv, D, byref(nbytes)))
        else:
            native.check(lib.grip_upt_mixer_deep_workspace(P, nd, dt, dv, D, byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        coop_out = torch.empty(P, dt, dtype=torch.float32, device=dev)
        vpt_out = torch.empty(P, dv, dtype=torch.float32, device=dev)
        # the reference's float16 branch (multimodal_prompt.py:46): fp16 projection Linears / prompt embeddings around the fp32 block
        half = int(tensors[2].dtype == torch.float16)
        m = native.UptMixer(P, dt, dv, D, half, 0, *[t.data_ptr() for t in ts[:22]])
        if deep is None:
            native.check(lib.grip_upt_mixer_forward(byref(m), _ptr(coop_out), _ptr(vpt_out), _ptr(ws), ws.numel(), _stream()))
            outs = (coop_out, vpt_out)
        else:
            deep_out = torch.empty(nd, P, dv, dtype=torch.float32, device=dev)
            native.check(lib.grip_upt_mixer_forward_deep(byref(m), _ptr(deep), nd, _ptr(coop_out), _ptr(vpt_out), _ptr(deep_out), _ptr(ws), ws.numel(),
                                                         _stream()))
            outs = (coop_out, vpt_out, deep_out)
        ctx.save_for_backward(*ts)
        ctx.ws, ctx.dims, ctx.half = ws, (P, dt, dv, D, nd), half
        ctx.shapes = [t.shape for t in tensors]
        ctx.dtypes = [t.dtype for t in tensors]
        return outs

    @staticmethod
    def backward(ctx, d_coop, d_vpt, d_deep=None):
        lib = native.lib()
        ts = ctx.saved_tensors
        P, dt, dv, D, nd = ctx.dims
        dev = ts[0].device
        d_coop = torch.zeros(P, dt, device=dev) if d_coop is None else d_coop.contiguous().float()
        d_vpt = torch.zeros(P, dv, device=dev) if d_vpt is None else d_vpt.contiguous().float()
        grads = [torch.empty_like(t) for t in ts]
        m = native.UptMixer(P, dt, dv, D, ctx.half, 0, *[t.data_ptr() for t in ts[:22]])
        g = native.UptMixer(P, dt, dv, D, ctx.half, 0, *[t.data_ptr() for t in grads[:22]])
        if nd == 0:
            native.check(lib.grip_upt_mixer_backward(byref(m), _ptr(d_coop), _ptr(d_vpt), byref(g), _ptr(ctx.ws), ctx.ws.numel(), _stream()))
        else:
            d_deep = torch.zeros(nd, P, dv, device=dev) if d_deep is None else d_deep.contiguous().float()
            native.check(lib.grip_upt_mixer_backward_deep(byref(m), _ptr(ts[22]), nd, _ptr(d_coop), _ptr(d_vpt), _ptr(d_deep), byref(g), _ptr(grads[22]),
                                                          _ptr(ctx.ws), ctx.ws.numel(), _stream()))
        return tuple(gr.reshape(sh).to(dtp) for gr, sh, dtp in zip(grads, ctx.shapes, ctx.dtypes))


def _couple_dims(ctx, deep, w, b):
    """(P, D, dt, dv) of a coupling call; ctx [P, dt] or [1, P, dt], deep None or [D, P, dt], w [1 + D, dv, dt], b [1 + D, dv]."""
    P, dt = ctx.shape[-2], ctx.shape[-1]
    D = 0 if deep is None else deep.shape[0]
    if ctx.numel() != P * dt or w.dim() != 3 or w.shape[0] != 1 + D or w.shape[2] != dt or tuple(b.shape) != (1 + D, w.shape[1]) \
            or (deep is not None and tuple(deep.shape) != (D, P, dt)):
        raise native.GripError(f"prompt coupling: ctx {tuple(ctx.shape)}, deep_text {None if deep is None else tuple(deep.shape)}, w {tuple(w.shape)}, "
                               f"b {tuple(b.shape)}: expected [P, dt], [D, P, dt], [1 + D, dv, dt], [1 + D, dv]")
    return P, D, dt, w.shape[1]


def prompt_couple_forward(ctx, deep_text, w, b):
    """MaPLe's coupling function on the native kernel (csrc/couple.hip), no autograd: (vis_prefix [P, dv], vis_deep [D, P, dv] or None)."""
    lib = native.lib()
    ctx, w, b = (t.detach().contiguous().float() for t in (ctx, w, b))
    deep = None if deep_text is None else deep_text.detach().contiguous().float()
    P, D, dt, dv = _couple_dims(ctx, deep, w, b)
    vis_prefix = torch.empty(P, dv, dtype=torch.float32, device=ctx.device)
    vis_deep = torch.empty(D, P, dv, dtype=torch.float32, device=ctx.device) if D else None
    native.check(lib.grip_prompt_couple_forward(_ptr(ctx), _ptr(deep), P, D, dt, dv, _ptr(w), _ptr(b), _ptr(vis_prefix), _ptr(vis_deep), _stream()))
    return vis_prefix, vis_deep


class PromptCoupleFn(torch.autograd.Function):
    """MaPLe's coupling function with native forward and backward: (ctx, deep_text or None, w, b) -> (vis_prefix, vis_deep) -- vis_prefix alone
    when deep_text is None -- and the gradients of all four.  The gradient of ctx / deep_text is the coupling's share; autograd adds the text
    tower's (TextPrefixFn) on the same leaves."""

    @staticmethod
    def forward(ctx_, ctx, deep_text, w, b):
        ts = [None if t is None else t.detach().contiguous().float() for t in (ctx, deep_text, w, b)]
        ctx_.dims = _couple_dims(ts[0], ts[1], ts[2], ts[3])
        ctx_.meta = [None if t is None else (t.shape, t.dtype) for t in (ctx, deep_text, w, b)]
        ctx_.save_for_backward(*[t for t in ts[:3] if t is not None])
        vis_prefix, vis_deep = prompt_couple_forward(*ts)
        return vis_prefix if vis_deep is None else (vis_prefix, vis_deep)

    @staticmethod
    def backward(ctx_, d_prefix, d_deep=None):
        lib = native.lib()
        P, D, dt, dv = ctx_.dims
        saved = ctx_.saved_tensors
        x, deep, w = (saved[0], saved[1], saved[2]) if D else (saved[0], None, saved[1])
        dev = x.device
        d_prefix = torch.zeros(P, dv, device=dev) if d_prefix is None else d_prefix.contiguous().float()
        if D:
            d_deep = torch.zeros(D, P, dv, device=dev) if d_deep is None else d_deep.contiguous().float()
        g_x, g_w = torch.empty_like(x), torch.empty_like(w)
        g_deep = torch.empty_like(deep) if D else None
        g_b = torch.empty(1 + D, dv, dtype=torch.float32, device=dev)
        nbytes = c_size_t()
        native.check(lib.grip_prompt_couple_workspace(P, D, dt, dv, byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        native.check(lib.grip_prompt_couple_backward(_ptr(x), _ptr(deep), P, D, dt, dv, _ptr(w), _ptr(d_prefix), _ptr(d_deep if D else None), _ptr(g_x),
                                                     _ptr(g_deep), _ptr(g_w), _ptr(g_b), _ptr(ws), ws.numel(), _stream()))
        return tuple(None if m is None else g.reshape(m[0]).to(m[1]) for g, m in zip((g_x, g_deep, g_w, g_b), ctx_.meta))


def _cache_head_args(img_emb, keys, class_start, key_weight, logits):
    """Contiguous f32 / int32 operands and (n, m, c, e) of a cache-head call, shapes checked (the values of class_start are the caller's:
    models.cache_models.TipAdapterModel builds and validates them on the host)."""
    img, k = img_emb.detach().contiguous().float(), keys.detach().contiguous().float()
    cs = class_start.to(device=img.device, dtype=torch.int32).contiguous()
    v = None if key_weight is None else key_weight.detach().to(device=img.device, dtype=torch.float32).contiguous()
    if img.dim() != 2 or k.dim() != 2 or logits.dim() != 2 or k.shape[1] != img.shape[1] or logits.shape[0] != img.shape[0] \
            or cs.dim() != 1 or cs.numel() != logits.shape[1] + 1 or (v is not None and tuple(v.shape) != (k.shape[0],)):
        raise native.GripError(f"cache head: img_emb {tuple(img_emb.shape)}, keys {tuple(keys.shape)}, class_start {tuple(class_start.shape)}, key_weight "
                               f"{None if key_weight is None else tuple(key_weight.shape)}, logits {tuple(logits.shape)}: expected [n, e], [m, e], [c + 1], "
                               "[m], [n, c]")
    return img, k, cs, v, (img.shape[0], k.shape[0], logits.shape[1], img.shape[1])


def _cache_head_workspace(dims, device):
    nbytes = c_size_t()
    native.check(native.lib().grip_cache_head_workspace(*dims, byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


def cache_head(img_emb, keys, class_start, key_weight, alpha, beta, clip_logits):
    """Tip-Adapter's cache term added to a CLONE of clip_logits [n, c] on the native kernel (csrc/cache_head.hip), no autograd:
    out[i, y] = clip_logits[i, y] + alpha * sum_{j in class y} key_weight[j] * exp(-beta * (1 - normalize(img_emb)[i] . keys[j]))."""
    out = clip_logits.detach().float().clone(memory_format=torch.contiguous_format)
    img, k, cs, v, dims = _cache_head_args(img_emb, keys, class_start, key_weight, out)
    ws = _cache_head_workspace(dims, img.device)
    native.check(native.lib().grip_cache_head_forward(_ptr(img), _ptr(k), _ptr(cs), _ptr(v), float(alpha), float(beta), *dims, _ptr(out), _ptr(ws), ws.numel(),
                                                      _stream()))
    return out


class CacheHeadFn(torch.autograd.Function):
    """(img_emb, keys, class_start, key_weight or None, alpha, beta, clip_logits) -> adapted logits, native forward and backward.  The gradient goes to
    the keys (Tip-Adapter-F trains them alone) and, unchanged, to clip_logits; the image embeddings come from a frozen tower and get none --
    marking them as requiring grad is an error, not a silent zero."""

    @staticmethod
    def forward(ctx, img_emb, keys, class_start, key_weight, alpha, beta, clip_logits):
        if img_emb.requires_grad:
            raise native.GripError("cache head: img_emb requires grad, but the head has no gradient for the image embeddings (its image tower is frozen); "
                                   "detach them")
        out = cache_head(img_emb, keys, class_start, key_weight, alpha, beta, clip_logits)
        ctx.save_for_backward(img_emb.detach(), keys.detach(), class_start, *([] if key_weight is None else [key_weight.detach()]))
        ctx.hyper = (float(alpha), float(beta))
        ctx.meta = (keys.shape, keys.dtype, clip_logits.dtype, keys.requires_grad, clip_logits.requires_grad)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        img, keys, cs, *rest = ctx.saved_tensors
        shape, dtype, ldtype, need_k, need_l = ctx.meta
        g = grad_out.contiguous().float()
        gk = None
        if need_k:
            img, k, cs, v, dims = _cache_head_args(img, keys, cs, rest[0] if rest else None, g)
            gk = torch.empty_like(k)
            ws = _cache_head_workspace(dims, img.device)
            native.check(native.lib().grip_cache_head_backward(_ptr(img), _ptr(k), _ptr(cs), _ptr(v), *ctx.hyper, *dims, _ptr(g), _ptr(gk), _ptr(ws),
                                                               ws.numel(), _stream()))
            gk = gk.reshape(shape).to(dtype)
        return None, gk, None, None, None, None, (grad_out.to(ldtype) if need_l else None)


def _feature_adapter_args(img_emb, w1, w2):
    """Contiguous f32 operands and (n, e, h) of a feature-adapter call, shapes checked (the kernel checks the values of e and h)."""
    img, a, b = img_emb.detach().contiguous().float(), w1.detach().contiguous().float(), w2.detach().contiguous().float()
    if img.dim() != 2 or a.dim() != 2 or b.dim() != 2 or a.shape[1] != img.shape[1] or tuple(b.shape) != (a.shape[1], a.shape[0]):
        raise native.GripError(f"feature adapter: img_emb {tuple(img_emb.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}: expected [n, e], [h, e], [e, h]")
    return img, a, b, (img.shape[0], img.shape[1], a.shape[0])


def _feature_adapter_workspace(dims, device):
    nbytes = c_size_t()
    native.check(native.lib().grip_feature_adapter_workspace(*dims, byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


def _feature_adapter_forward(img_emb, w1, w2, ratio, train):
    img, a, b, dims = _feature_adapter_args(img_emb, w1, w2)
    out = torch.empty_like(img)
    hidden = torch.empty(dims[0], dims[2], dtype=torch.float32, device=img.device) if train else None
    act = torch.empty_like(img) if train else None
    native.check(native.lib().grip_feature_adapter_forward(_ptr(img), _ptr(a), _ptr(b), float(ratio), *dims, _ptr(out), _ptr(hidden), _ptr(act), _stream()))
    return out, hidden, act, img, a, b, dims


def feature_adapter(img_emb, w1, w2, ratio):
    """CLIP-Adapter's feature head on the native kernel (csrc/feature_adapter.hip), no autograd, one launch:
    out [n, e] = ratio * relu(relu(img_emb @ w1.T) @ w2.T) + (1 - ratio) * img_emb, f32.  A row's bits depend on that row and the weights only."""
    return _feature_adapter_forward(img_emb, w1, w2, ratio, False)[0]


class FeatureAdapterFn(torch.autograd.Function):
    """(img_emb, w1, w2, ratio) -> adapted features, native forward and backward.  The gradient goes to w1 and w2; the image embeddings come from a
    frozen tower and get none -- marking them as requiring grad is an error, not a silent zero.  When neither weight requires grad the forward is the
    inference call (the hidden activations never reach memory); otherwise it keeps the two post-ReLU tensors for the backward."""

    @staticmethod
    def forward(ctx, img_emb, w1, w2, ratio):
        if img_emb.requires_grad:
            raise native.GripError("feature adapter: img_emb requires grad, but the head has no gradient for the image embeddings (its image tower is "
                                   "frozen); detach them")
        train = w1.requires_grad or w2.requires_grad
        out, hidden, act, img, a, b, dims = _feature_adapter_forward(img_emb, w1, w2, ratio, train)
        if train:
            ctx.save_for_backward(img, b, hidden, act)
        ctx.ratio, ctx.dims = float(ratio), dims
        ctx.meta = ((w1.shape, w1.dtype, w1.requires_grad), (w2.shape, w2.dtype, w2.requires_grad))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        img, b, hidden, act = ctx.saved_tensors
        n, e, h = ctx.dims
        g = grad_out.contiguous().float()
        g1, g2 = torch.empty(h, e, dtype=torch.float32, device=img.device), torch.empty(e, h, dtype=torch.float32, device=img.device)
        ws = _feature_adapter_workspace(ctx.dims, img.device)
        native.check(native.lib().grip_feature_adapter_backward(_ptr(img), _ptr(b), _ptr(hidden), _ptr(act), _ptr(g), ctx.ratio, n, e, h, _ptr(g1), _ptr(g2),
                                                                _ptr(ws), ws.numel(), _stream()))
        (s1, d1, need1), (s2, d2, need2) = ctx.meta
        return None, (g1.reshape(s1).to(d1) if need1 else None), (g2.reshape(s2).to(d2) if need2 else None), None


KNN_MAX_K = 32      # csrc/knn_graph.hip: KG_MAX_K


def knn_graph(queries, base=None, k=16, self_offset=None):
    """(idx int32 [n, k], sim f32 [n, k]): per row of `queries` [n, e] the k rows of `base` [m, e] of largest cosine, ordered (sim descending, index
    ascending), on the native kernel (csrc/knn_graph.hip); the [n, m] similarities never reach memory.  base=None: pool on pool (a row is not its
    own neighbour).  self_offset: query i is base row self_offset + i and is excluded for it (default: 0 when base is None, else nothing excluded).
    Embeddings are taken un-normalised; finite rows of non-zero norm are the caller's duty."""
    if not torch.is_tensor(queries) or queries.dim() != 2 or not queries.is_floating_point():
        raise native.GripError(f"knn_graph: queries must be a floating-point [n, e] tensor, got {getattr(queries, 'shape', type(queries))}")
    q = queries.detach().contiguous().float()
    if base is None:
        b = q
        off = 0 if self_offset is None else int(self_offset)
    else:
        if not torch.is_tensor(base) or base.dim() != 2 or not base.is_floating_point() or base.shape[1] != q.shape[1] or base.device != q.device:
            raise native.GripError(f"knn_graph: base must be a floating-point [m, {q.shape[1]}] tensor on {q.device}, got "
                                   f"{getattr(base, 'shape', type(base))}")
        b = base.detach().contiguous().float()
        off = -1 if self_offset is None else int(self_offset)
    require_gpu(q.device)
    (n, e), m, k = q.shape, b.shape[0], int(k)
    lib = native.lib()
    nbytes = c_size_t()
    native.check(lib.grip_knn_graph_workspace(n, m, e, k, byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=q.device)
    idx = torch.empty(n, k, dtype=torch.int32, device=q.device)
    sim = torch.empty(n, k, dtype=torch.float32, device=q.device)
    native.check(lib.grip_knn_graph(_ptr(q), _ptr(b), n, m, e, k, off, _ptr(idx), _ptr(sim), _ptr(ws), ws.numel(), _stream()))
    return idx, sim


def label_propagate(probs, idx, sim, alpha, gamma, iters):
    """(Z f32 [n, c], pred int32 [n]): `iters` steps of Z <- (1 - alpha) probs + alpha W Z on the directed kNN graph (idx, sim) of engine.knn_graph,
    W = softmax(gamma sim) over each row's neighbours; pred is the first arg-max of Z's rows (csrc/knn_graph.hip)."""
    if not torch.is_tensor(probs) or probs.dim() != 2 or not probs.is_floating_point():
        raise native.GripError(f"label_propagate: probs must be a floating-point [n, c] tensor, got {getattr(probs, 'shape', type(probs))}")
    n, c = probs.shape
    if not torch.is_tensor(idx) or not torch.is_tensor(sim) or idx.dim() != 2 or idx.shape[0] != n or tuple(sim.shape) != tuple(idx.shape) \
            or idx.dtype != torch.int32 or sim.dtype != torch.float32 or idx.device != probs.device or sim.device != probs.device:
        raise native.GripError(f"label_propagate: idx (int32) and sim (f32) must both be [{n}, k] on {probs.device}, got "
                               f"{getattr(idx, 'shape', None)} {getattr(idx, 'dtype', None)} and {getattr(sim, 'shape', None)} {getattr(sim, 'dtype', None)}")
    require_gpu(probs.device)
    p = probs.detach().contiguous().float()
    ix, sm = idx.contiguous(), sim.contiguous()
    k = ix.shape[1]
    lib = native.lib()
    nbytes = c_size_t()
    native.check(lib.grip_label_propagate_workspace(n, c, k, byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=p.device)
    out = torch.empty_like(p)
    pred = torch.empty(n, dtype=torch.int32, device=p.device)
    native.check(lib.grip_label_propagate(_ptr(p), _ptr(ix), _ptr(sm), float(alpha), float(gamma), int(iters), n, c, k, _ptr(out), _ptr(pred), _ptr(ws),
                                          ws.numel(), _stream()))
    return out, pred


GMM_MSTEP_ROWS = 256    # csrc/gmm_transduce.hip: GM_ROWS, the fixed row partition of the M-step's sums


def _gmm_operand(who, name, t, shape, like=None, dtype=torch.float32):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or (like is not None and t.device != like.device):
        raise native.GripError(f"{who}: {name} must be a {str(dtype).replace('torch.', '')} {list(shape)} tensor" +
                               (f" on {like.device}" if like is not None else "") +
                               f", got {getattr(t, 'shape', type(t))} {getattr(t, 'dtype', None)}")
    return t.detach().contiguous()


def gmm_mstep(z, feats, var_floor=1e-8):
    """(count f32 [c], mean f32 [c, e], var f32 [e]) of the weighted class Gaussians with a shared diagonal covariance: count_c = sum_i z_ic,
    mean_c = sum_i z_ic feats_i / count_c (zero where the count is 0), var_d = max(var_floor, mean_i sum_c z_ic (feats_id - mean_cd)^2), on the
    native kernels (csrc/gmm_transduce.hip): no atomics, a fixed row partition, bit-identical from call to call.  feats is taken as given."""
    if not torch.is_tensor(z) or z.dim() != 2 or not torch.is_tensor(feats) or feats.dim() != 2 or feats.shape[0] != z.shape[0]:
        raise native.GripError(f"gmm_mstep: z [n, c] and feats [n, e] expected, got {getattr(z, 'shape', type(z))} and {getattr(feats, 'shape', type(feats))}")
    (n, c), e = z.shape, feats.shape[1]
    zz = _gmm_operand("gmm_mstep", "z", z, (n, c))
    f = _gmm_operand("gmm_mstep", "feats", feats, (n, e), zz)
    require_gpu(zz.device)
    lib = native.lib()
    nbytes = c_size_t()
    native.check(lib.grip_gmm_mstep_workspace(n, c, e, byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=zz.device)
    count = torch.empty(c, dtype=torch.float32, device=zz.device)
    mean = torch.empty(c, e, dtype=torch.float32, device=zz.device)
    var = torch.empty(e, dtype=torch.float32, device=zz.device)
    native.check(lib.grip_gmm_mstep(_ptr(zz), _ptr(f), n, c, e, float(var_floor), _ptr(count), _ptr(mean), _ptr(var), _ptr(ws), ws.numel(), _stream()))
    return count, mean, var


def gmm_estep(feats, mean, var, probs, idx, sim, z, lam=1.0, z_iters=5):
    """(Z f32 [n, c], pred int32 [n]): the scores G_ic = feats_i . (mean_c / var) - 1/2 sum_d mean_cd^2 / var_d once on the f32 MFMA, then `z_iters`
    Jacobi sweeps Z_i <- softmax_c(G_ic + lam log max(probs_ic, 2^-126) + sum_j max(0, sim_ij) Z_{idx_ij, c}) from Z = z over the directed graph
    (idx, sim) of engine.knn_graph; pred is the first arg-max of Z's rows (csrc/gmm_transduce.hip).  feats is taken as given."""
    if not torch.is_tensor(feats) or feats.dim() != 2 or not torch.is_tensor(probs) or probs.dim() != 2 or probs.shape[0] != feats.shape[0] \
            or not torch.is_tensor(idx) or idx.dim() != 2:
        raise native.GripError(f"gmm_estep: feats [n, e], probs [n, c] and idx [n, k] expected, got {getattr(feats, 'shape', type(feats))}, "
                               f"{getattr(probs, 'shape', type(probs))} and {getattr(idx, 'shape', type(idx))}")
    (n, e), c, k = feats.shape, probs.shape[1], idx.shape[1]
    f = _gmm_operand("gmm_estep", "feats", feats, (n, e))
    mu = _gmm_operand("gmm_estep", "mean", mean, (c, e), f)
    v = _gmm_operand("gmm_estep", "var", var, (e,), f)
    p = _gmm_operand("gmm_estep", "probs", probs, (n, c), f)
    ix = _gmm_operand("gmm_estep", "idx", idx, (n, k), f, torch.int32)
    sm = _gmm_operand("gmm_estep", "sim", sim, (n, k), f)
    zz = _gmm_operand("gmm_estep", "z", z, (n, c), f)
    require_gpu(f.device)
    lib = native.lib()
    nbytes = c_size_t()
    native.check(lib.grip_gmm_estep_workspace(n, c, e, k, byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=f.device)
    out = torch.empty(n, c, dtype=torch.float32, device=f.device)
    pred = torch.empty(n, dtype=torch.int32, device=f.device)
    native.check(lib.grip_gmm_estep(_ptr(f), _ptr(mu), _ptr(v), _ptr(p), _ptr(ix), _ptr(sm), _ptr(zz), float(lam), int(z_iters), n, c, e, k, _ptr(out),
                                    _ptr(pred), _ptr(ws), ws.numel(), _stream()))
    return out, pred


def gmm_transduce(feats, probs, idx, sim, lam=1.0, iters=10, z_iters=5, var_floor=1e-8):
    """(Z [n, c], pred int32 [n], mean [c, e], var [e], count [c]): the transductive GMM recursion of include/grip_amd.h (after TransCLIP-ZS, not that
    code) from Z = probs: `iters` times an M-step on (Z, feats) and an E-step of `z_iters` sweeps.  feats are normalised to unit rows here (torch);
    mean / var / count are the last M-step's, which can score images that were not in the pool."""
    if int(iters) < 1:
        raise native.GripError(f"gmm_transduce: iters = {iters} (at least 1)")
    if not torch.is_tensor(feats) or feats.dim() != 2 or not feats.is_floating_point() or not torch.is_tensor(probs) or not probs.is_floating_point():
        raise native.GripError(f"gmm_transduce: floating-point feats [n, e] and probs [n, c] expected, got {getattr(feats, 'shape', type(feats))} and "
                               f"{getattr(probs, 'shape', type(probs))}")
    f = torch.nn.functional.normalize(feats.detach().float(), dim=1).contiguous()
    p = probs.detach().float().contiguous()
    z, pred = p, None
    for _ in range(int(iters)):
        count, mean, var = gmm_mstep(z, f, var_floor)
        z, pred = gmm_estep(f, mean, var, p, idx, sim, z, lam, z_iters)
    return z, pred, mean, var, count


GDA_SCATTER_ROWS = 256      # csrc/gda_head.hip: GD_ROWS, the fixed row chunk of the scatter
GDA_SCATTER_SLICES = 16     # csrc/gda_head.hip: GD_SLICES, the K-slices the chunks are grouped into at most
GDA_MAX_E = 1024            # csrc/gda_head.hip: GD_MAX_E


def _gda_workspace(query, dims, device):
    nbytes = c_size_t()
    native.check(query(*dims, byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


def class_scatter(feats, labels, row_weight, mean):
    """S f32 [e, e] = sum_i r_i (feats_i - mean[labels_i]) (feats_i - mean[labels_i])^T, the within-class scatter in its direct form on the native
    SYRK (csrc/gda_head.hip): feats [n, e] taken as given, labels int32 [n], row_weight f32 [n] or None (1), mean [c, e].  No atomics, a fixed row
    partition, bit-symmetric and bit-identical from call to call.  A row with a label outside 0 .. c - 1 or a weight of 0 contributes nothing (the
    values of labels are the caller's: models.gda_models.GdaHeadModel validates them on the host)."""
    if not torch.is_tensor(feats) or feats.dim() != 2 or not torch.is_tensor(mean) or mean.dim() != 2 or mean.shape[1] != feats.shape[1]:
        raise native.GripError(f"class_scatter: feats [n, e] and mean [c, e] expected, got {getattr(feats, 'shape', type(feats))} and "
                               f"{getattr(mean, 'shape', type(mean))}")
    (n, e), c = feats.shape, mean.shape[0]
    f = _gmm_operand("class_scatter", "feats", feats, (n, e))
    y = _gmm_operand("class_scatter", "labels", labels, (n,), f, torch.int32)
    r = None if row_weight is None else _gmm_operand("class_scatter", "row_weight", row_weight, (n,), f)
    mu = _gmm_operand("class_scatter", "mean", mean, (c, e), f)
    require_gpu(f.device)
    lib = native.lib()
    ws = _gda_workspace(lib.grip_class_scatter_workspace, (n, c, e), f.device)
    out = torch.empty(e, e, dtype=torch.float32, device=f.device)
    native.check(lib.grip_class_scatter(_ptr(f), _ptr(y), _ptr(r), _ptr(mu), n, c, e, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def spd_solve(a, rhs, a_scale=1.0, ridge_rel=0.0, want_factor=False):
    """x f32 [c, e] with M x_c = rhs_c, M = a_scale a + ridge_rel a_scale (tr(a) / e) I, by the native blocked Cholesky (csrc/gda_head.hip); a [e, e] is
    read from its lower triangle only.  want_factor: (x, L) with M = L L^T, L lower triangular.  Reads the kernel's info word (one synchronisation) and
    raises GripError naming the pivot when M is not positive definite in f32."""
    if not torch.is_tensor(a) or a.dim() != 2 or a.shape[0] != a.shape[1] or not torch.is_tensor(rhs) or rhs.dim() != 2 or rhs.shape[1] != a.shape[0]:
        raise native.GripError(f"spd_solve: a [e, e] and rhs [c, e] expected, got {getattr(a, 'shape', type(a))} and {getattr(rhs, 'shape', type(rhs))}")
    e, c = a.shape[0], rhs.shape[0]
    aa = _gmm_operand("spd_solve", "a", a, (e, e))
    b = _gmm_operand("spd_solve", "rhs", rhs, (c, e), aa)
    require_gpu(aa.device)
    lib = native.lib()
    ws = _gda_workspace(lib.grip_spd_solve_workspace, (e, c), aa.device)
    x = torch.empty(c, e, dtype=torch.float32, device=aa.device)
    fac = torch.empty(e, e, dtype=torch.float32, device=aa.device) if want_factor else None
    info = torch.empty(1, dtype=torch.int32, device=aa.device)
    native.check(lib.grip_spd_solve(_ptr(aa), float(a_scale), float(ridge_rel), _ptr(b), e, c, _ptr(x), _ptr(fac), _ptr(info), _ptr(ws), ws.numel(),
                                    _stream()))
    bad = int(info.item())
    if bad:
        raise native.GripError(f"spd_solve: the matrix is not positive definite in f32: pivot {bad - 1} of {e} is not > 0 "
                               f"(a_scale = {float(a_scale):g}, ridge_rel = {float(ridge_rel):g})")
    return (x, fac) if want_factor else x


def linear_head(img_emb, w, bias, alpha, base_logits=None, want_argmax=False):
    """logits f32 [n, c] = base_logits + alpha * ((img_emb @ w.T) / |img_emb| - bias) in ONE launch of the native head (csrc/gda_head.hip), no autograd;
    img_emb [n, e] NOT normalised, w [c, e], bias [c], base_logits [n, c] or None (0).  The result is a new tensor (the C entry point also works in
    place).  want_argmax: (logits, pred int32 [n]), the first arg-max of every row."""
    if not torch.is_tensor(img_emb) or img_emb.dim() != 2 or not torch.is_tensor(w) or w.dim() != 2 or w.shape[1] != img_emb.shape[1]:
        raise native.GripError(f"linear_head: img_emb [n, e] and w [c, e] expected, got {getattr(img_emb, 'shape', type(img_emb))} and "
                               f"{getattr(w, 'shape', type(w))}")
    (n, e), c = img_emb.shape, w.shape[0]
    f = _gmm_operand("linear_head", "img_emb", img_emb, (n, e))
    ww = _gmm_operand("linear_head", "w", w, (c, e), f)
    b = _gmm_operand("linear_head", "bias", bias, (c,), f)
    if base_logits is None:
        out, base = torch.empty(n, c, dtype=torch.float32, device=f.device), None
    else:
        out = _gmm_operand("linear_head", "base_logits", base_logits, (n, c), f).clone(memory_format=torch.contiguous_format)
        base = out
    require_gpu(f.device)
    lib = native.lib()
    ws = _gda_workspace(lib.grip_linear_head_workspace, (n, c, e), f.device)
    pred = torch.empty(n, dtype=torch.int32, device=f.device) if want_argmax else None
    native.check(lib.grip_linear_head(_ptr(f), _ptr(ww), _ptr(b), float(alpha), _ptr(base), n, c, e, _ptr(out), _ptr(pred), _ptr(ws), ws.numel(), _stream()))
    return (out, pred) if want_argmax else out


PROBE_SCORE_ROWS = 32       # csrc/linear_probe.hip: PB_BM, the rows whose losses one workgroup of the score kernel adds
PROBE_ROWS = 64             # csrc/linear_probe.hip: PB_ROWS, the fixed row chunk of the contraction
PROBE_MAX_C = 1024          # csrc/linear_probe.hip: PB_MAX_C


def probe_slice_cap(c, e):
    """The most K-slices the contraction of grip_probe_objective cuts n rows into (csrc/linear_probe.hip, probe_plan): a function of (c, e) alone."""
    return min(64, max(4, 1024 // (((c + 127) // 128) * ((e + 63) // 64))))


def probe_slices(n, c, e):
    """(chunks per slice, slices) of the contraction's fixed row partition."""
    nch = (n + PROBE_ROWS - 1) // PROBE_ROWS
    per = (nch + probe_slice_cap(c, e) - 1) // probe_slice_cap(c, e)
    return per, (nch + per - 1) // per


def _probe_operands(who, feats, base, labels, soft, row_weight, c):
    if not torch.is_tensor(feats) or feats.dim() != 2:
        raise native.GripError(f"{who}: feats [n, e] expected, got {getattr(feats, 'shape', type(feats))}")
    n, e = feats.shape
    f = _gmm_operand(who, "feats", feats, (n, e))
    bs = None if base is None else _gmm_operand(who, "base", base, (n, c), f)
    y = _gmm_operand(who, "labels", labels, (n,), f, torch.int32)
    sf = None if soft is None else _gmm_operand(who, "soft", soft, (n, c), f)
    r = None if row_weight is None else _gmm_operand(who, "row_weight", row_weight, (n,), f)
    require_gpu(f.device)
    return f, bs, y, sf, r, n, e


def _probe_scalar(who, name, v, positive=True):
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")) or (v <= 0 if positive else v < 0):
        raise native.GripError(f"{who}: {name} = {v:g} (must be finite and {'> 0' if positive else '>= 0'})")
    return v


def probe_norm(labels, soft, row_weight, c):
    """nu = 1 / sum_i r_i over the rows that contribute to grip_probe_objective (a label in 0 .. c - 1, or -1 with soft given; a weight that is not 0),
    as a Python float: the sum runs on the device in float64, reading it back is ONE synchronisation."""
    ok = ((labels >= 0) & (labels < c)) | ((labels == -1) if soft is not None else torch.zeros_like(labels, dtype=torch.bool))
    r = torch.ones(labels.shape[0], dtype=torch.float64, device=labels.device) if row_weight is None else row_weight.double()
    total = float(torch.where(ok & (r != 0), r, torch.zeros_like(r)).sum().item())
    if not total > 0:
        raise native.GripError(f"probe_norm: the weights of the contributing rows add up to {total:g} (no row contributes)")
    return 1.0 / total


def probe_objective(feats, w, b, base, labels, soft, row_weight, scale, norm):
    """(loss 0-d, grad_w [c, e], grad_b [c]), the DATA term of the linear probe of include/grip_amd.h and its gradient on the native kernels
    (csrc/linear_probe.hip): x = base + scale feats @ w.T + b, loss = norm sum_i r_i (T_i lse(x_i) - t_i . x_i) with t = onehot(labels) or, for labels == -1,
    the row of soft.  feats [n, e] taken as given; b, base, soft, row_weight may be None.  Three launches, no atomics, bit-identical from call to call."""
    if not torch.is_tensor(w) or w.dim() != 2:
        raise native.GripError(f"probe_objective: w [c, e] expected, got {getattr(w, 'shape', type(w))}")
    c = w.shape[0]
    f, bs, y, sf, r, n, e = _probe_operands("probe_objective", feats, base, labels, soft, row_weight, c)
    ww = _gmm_operand("probe_objective", "w", w, (c, e), f)
    bb = None if b is None else _gmm_operand("probe_objective", "b", b, (c,), f)
    scale, norm = _probe_scalar("probe_objective", "scale", scale), _probe_scalar("probe_objective", "norm", norm)
    lib = native.lib()
    ws = _gda_workspace(lib.grip_probe_objective_workspace, (n, c, e), f.device)
    loss = torch.empty(1, dtype=torch.float32, device=f.device)
    gw = torch.empty(c, e, dtype=torch.float32, device=f.device)
    gb = torch.empty(c, dtype=torch.float32, device=f.device)
    native.check(lib.grip_probe_objective(_ptr(f), _ptr(ww), _ptr(bb), _ptr(bs), _ptr(y), _ptr(sf), _ptr(r), scale, norm, n, c, e, _ptr(loss), _ptr(gw),
                                          _ptr(gb), _ptr(ws), ws.numel(), _stream()))
    return loss[0], gw, gb


def probe_fit(feats, base, labels, soft, row_weight, scale, l2, lr, momentum, iters, w, b, state=None, want_trace=False, norm=None):
    """(w, b, state[, trace]): `iters` full-batch heavy-ball iterations of the linear probe (grip_probe_fit: torch.optim.SGD(momentum) semantics on
    norm sum_i r_i CE_i + (l2 / 2) |w|^2, three launches an iteration, no host synchronisation, capturable in a graph).  w [c, e] and b [c] are the start
    and are NOT modified: the result is new tensors.  state = (mom_w, mom_b, norm, workspace) as an earlier call returned it (None: zero momentum):
    probe_fit(k1) and then probe_fit(k2, state=...) give the bits of probe_fit(k1 + k2).  norm = 1 / sum of the contributing rows' weights comes from
    `norm`, else from `state`, else from probe_norm -- the only synchronisation, and only when the caller gave neither.  trace f32 [iters]: the data
    term at the start of every iteration (stays on the device)."""
    if not torch.is_tensor(w) or w.dim() != 2:
        raise native.GripError(f"probe_fit: w [c, e] expected, got {getattr(w, 'shape', type(w))}")
    c = w.shape[0]
    f, bs, y, sf, r, n, e = _probe_operands("probe_fit", feats, base, labels, soft, row_weight, c)
    ww = _gmm_operand("probe_fit", "w", w, (c, e), f).clone(memory_format=torch.contiguous_format)
    bb = _gmm_operand("probe_fit", "b", b, (c,), f).clone(memory_format=torch.contiguous_format)
    scale, lr = _probe_scalar("probe_fit", "scale", scale), _probe_scalar("probe_fit", "lr", lr)
    l2, momentum = _probe_scalar("probe_fit", "l2", l2, positive=False), _probe_scalar("probe_fit", "momentum", momentum, positive=False)
    if momentum >= 1 or int(iters) < 1:
        raise native.GripError(f"probe_fit: momentum = {momentum:g}, iters = {iters} (0 <= momentum < 1, iters >= 1)")
    lib = native.lib()
    if state is None:
        mw, mb, ws = torch.zeros_like(ww), torch.zeros_like(bb), _gda_workspace(lib.grip_probe_fit_workspace, (n, c, e), f.device)
    else:
        mw = _gmm_operand("probe_fit", "state[0]", state[0], (c, e), f).clone(memory_format=torch.contiguous_format)
        mb = _gmm_operand("probe_fit", "state[1]", state[1], (c,), f).clone(memory_format=torch.contiguous_format)
        ws = state[3]
        norm = state[2] if norm is None else norm
    norm = _probe_scalar("probe_fit", "norm", probe_norm(y, sf, r, c) if norm is None else norm)
    trace = torch.empty(int(iters), dtype=torch.float32, device=f.device) if want_trace else None
    native.check(lib.grip_probe_fit(_ptr(f), _ptr(bs), _ptr(y), _ptr(sf), _ptr(r), scale, norm, l2, lr, momentum, int(iters), n, c, e, _ptr(ww), _ptr(bb),
                                    _ptr(mw), _ptr(mb), _ptr(trace), _ptr(ws), ws.numel(), _stream()))
    state = (mw, mb, norm, ws)
    return (ww, bb, state, trace) if want_trace else (ww, bb, state)


SINKHORN_ROWS = 16      # csrc/sinkhorn.hip: SK_ROWS, the fixed row partition of the column sums


def sinkhorn_balance(probs, tau=1.0, iters=3, prior=None, log_scale=None):
    """(Q f32 [n, c], pred int32 [n], mass f32 [c], log_scale f32 [c]): the balanced assignment of include/grip_amd.h on the native kernels
    (csrc/sinkhorn.hip) -- `iters` Sinkhorn-Knopp iterations on probs ** tau from the column scaling exp(log_scale) (None: ones), then
    Q_i = softmax_c(tau log probs_i + log_scale), its first arg-max and the column sums mass.  prior: None (uniform) or [c] finite positive weights,
    normalised in float64 on the host; the columns are pressed towards n * prior.  iters = 0 is one bare step under the given log_scale.  The returned
    log_scale continues the recursion in a later call.  No atomics, a fixed row partition, bit-identical from call to call."""
    if not torch.is_tensor(probs) or probs.dim() != 2 or not probs.is_floating_point():
        raise native.GripError(f"sinkhorn_balance: probs must be a floating-point [n, c] tensor, got {getattr(probs, 'shape', type(probs))}")
    n, c = probs.shape
    require_gpu(probs.device)
    p = probs.detach().contiguous().float()
    if prior is None:
        log_target = torch.full((c,), math.log(1.0 / max(c, 1)), dtype=torch.float32, device=p.device)      # (filled on the device: no host copy per pass)
    else:
        if not torch.is_tensor(prior) or tuple(prior.shape) != (c,) or prior.is_complex():
            raise native.GripError(f"sinkhorn_balance: prior must be a real [{c}] tensor, got {getattr(prior, 'shape', type(prior))}")
        target = prior.detach().to("cpu", torch.float64)
        if not bool((torch.isfinite(target) & (target > 0)).all()):
            raise native.GripError("sinkhorn_balance: prior must hold finite positive weights")
        log_target = torch.log(target / target.sum()).to(torch.float32).to(p.device)
    b_in = None if log_scale is None else _gmm_operand("sinkhorn_balance", "log_scale", log_scale, (c,), p)
    lib = native.lib()
    nbytes = c_size_t()
    native.check(lib.grip_sinkhorn_workspace(n, c, byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=p.device)
    q = torch.empty_like(p)
    pred = torch.empty(n, dtype=torch.int32, device=p.device)
    mass = torch.empty(c, dtype=torch.float32, device=p.device)
    b_out = torch.empty(c, dtype=torch.float32, device=p.device)
    native.check(lib.grip_sinkhorn_balance(_ptr(p), _ptr(log_target), _ptr(b_in), float(tau), int(iters), n, c, _ptr(q),
                                           _ptr(pred), _ptr(mass), _ptr(b_out), _ptr(ws), ws.numel(), _stream()))
    return q, pred, mass, b_out


VIEW_MODE_MAX_VIEWS = 64        # csrc/view_mode.hip: VM_MAXV
VIEW_MODE_MAX_E = 1024          # csrc/view_mode.hip: VM_MAXE
VIEW_MODE_DEFAULTS = dict(rho=0.3, lam=4.0, lam_y=0.2, h2_floor=2.0 ** -20, outer=5, inner=3)      # rho, lam, lam_y: the paper's; the counts are untuned


def view_mode(view_emb, view_probs=None, rho=0.3, lam=4.0, lam_y=0.2, h2_floor=2.0 ** -20, outer=5, inner=3, mode_in=None, y_in=None, want_h2=False):
    """(mode f32 [n, e], y f32 [n, v][, h2 f32 [n, v]]): the multi-view mode of include/grip_amd.h on the native kernel (csrc/view_mode.hip) -- view_emb
    [n, v, e] f32 (view 0 the un-augmented image), view_probs [n, v, c] f32 or None (no affinity term), mode_in [n, e] / y_in [n, v] or None (u_0 and
    1 / v).  mode is not normalised.  Everything is validated here, on the host, before the one launch; bit-identical from call to call, and an image's
    bits do not depend on n or on its place."""
    if not torch.is_tensor(view_emb) or view_emb.dim() != 3 or view_emb.dtype != torch.float32:
        raise native.GripError(f"view_mode: view_emb must be a float32 [n, v, e] tensor, got {getattr(view_emb, 'shape', type(view_emb))} "
                               f"{getattr(view_emb, 'dtype', None)}")
    n, v, e = view_emb.shape
    require_gpu(view_emb.device)
    if n < 1 or not 2 <= v <= VIEW_MODE_MAX_VIEWS or e < 64 or e > VIEW_MODE_MAX_E or e % 64:
        raise native.GripError(f"view_mode: n = {n}, v = {v}, e = {e} (n >= 1, 2 <= v <= {VIEW_MODE_MAX_VIEWS}, e a multiple of 64 up to {VIEW_MODE_MAX_E})")
    f = view_emb.detach().contiguous()
    c, s = 1, None
    if view_probs is not None:
        if not torch.is_tensor(view_probs) or view_probs.dim() != 3 or tuple(view_probs.shape[:2]) != (n, v) or view_probs.shape[2] < 1:
            raise native.GripError(f"view_mode: view_probs must be a float32 [{n}, {v}, c] tensor, got {getattr(view_probs, 'shape', type(view_probs))}")
        c = view_probs.shape[2]
        s = _gmm_operand("view_mode", "view_probs", view_probs, (n, v, c), f)
    m0 = None if mode_in is None else _gmm_operand("view_mode", "mode_in", mode_in, (n, e), f)
    y0 = None if y_in is None else _gmm_operand("view_mode", "y_in", y_in, (n, v), f)
    for name, val, ok in (("rho", rho, lambda x: 0 < x <= 1), ("lam", lam, lambda x: x >= 0), ("lam_y", lam_y, lambda x: x > 0),
                          ("h2_floor", h2_floor, lambda x: x > 0)):
        x = float(val)
        if not (math.isfinite(x) and ok(x)):
            raise native.GripError(f"view_mode: {name} = {x:g} is out of range (0 < rho <= 1, lam >= 0, lam_y > 0, h2_floor > 0, all finite)")
    for name, val in (("outer", outer), ("inner", inner)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 0:
            raise native.GripError(f"view_mode: {name} = {val!r} (an integer >= 0)")
    lib = native.lib()
    ws = _gda_workspace(lib.grip_view_mode_workspace, (n, v, c, e), f.device)      # (0 bytes today: the kernel keeps its state in the LDS)
    mode = torch.empty(n, e, dtype=torch.float32, device=f.device)
    y = torch.empty(n, v, dtype=torch.float32, device=f.device)
    h2 = torch.empty(n, v, dtype=torch.float32, device=f.device) if want_h2 else None
    native.check(lib.grip_view_mode(_ptr(f), _ptr(s), n, v, c, e, float(rho), float(lam), float(lam_y), float(h2_floor), outer, inner, _ptr(m0), _ptr(y0),
                                    _ptr(mode), _ptr(y), _ptr(h2), _ptr(ws) if ws.numel() else c_void_p(0), ws.numel(), _stream()))
    return (mode, y, h2) if want_h2 else (mode, y)


VIEW_ENTROPY_MAX_C = 16000      # csrc/view_entropy.hip: VE_MAXC (g lives in the LDS)


def view_entropy(logits, views, keep, want_grad=True, want_entropy=False, want_selected=False, want_mean=False):
    """(loss[, grad][, entropy][, selected][, mean]): the marginal entropy of every image's `keep` most confident views of include/grip_amd.h on the native
    kernel (csrc/view_entropy.hip) -- logits f32 [n views, c], contiguous, on the GPU, image-major; loss 0-d f32, the mean over the n images; grad
    [n views, c] (exactly +0.0 on the views that were not selected), entropy [n, views] (H_p), selected int32 [n, views] (0 / 1), mean [n, c] (pbar).
    Everything is validated here, on the host, before the launch; bit-identical from call to call, and an image's entropies, selection and marginal do
    not depend on n or on its place.  Meant for n = 1 (an episode) up to some hundreds of images (a chunk of views): the per-image work is one workgroup
    per image, but the mean over n > 1 images is ONE workgroup that re-adds n c logarithms serially (27 us at 55 x 16 x 102) -- a pool-sized n would be one
    CU's work; call it in chunks and average the losses on the host side of the graph instead.  No autograd (ViewEntropyFn)."""
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise native.GripError(f"view_entropy: logits must be a contiguous float32 [n views, c] tensor, got {getattr(logits, 'shape', type(logits))} "
                               f"{getattr(logits, 'dtype', None)}")
    require_gpu(logits.device)
    for name, val in (("views", views), ("keep", keep)):
        if isinstance(val, bool) or not isinstance(val, int):
            raise native.GripError(f"view_entropy: {name} = {val!r} (an integer)")
    rows, c = logits.shape
    if not 1 <= views <= VIEW_MODE_MAX_VIEWS or not 1 <= keep <= views:
        raise native.GripError(f"view_entropy: views = {views}, keep = {keep} (1 <= views <= {VIEW_MODE_MAX_VIEWS}, 1 <= keep <= views)")
    if rows < 1 or rows % views or not 1 <= c <= VIEW_ENTROPY_MAX_C:
        raise native.GripError(f"view_entropy: logits [{rows}, {c}] with {views} views (a positive multiple of views rows, 1 <= c <= {VIEW_ENTROPY_MAX_C})")
    lg = logits.detach()
    n, dev = rows // views, lg.device
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    grad = torch.empty_like(lg) if want_grad else None
    ent = torch.empty(n, views, dtype=torch.float32, device=dev) if want_entropy else None
    sel = torch.empty(n, views, dtype=torch.int32, device=dev) if want_selected else None
    mean = torch.empty(n, c, dtype=torch.float32, device=dev) if want_mean or n > 1 else None      # (n > 1: the mean over images re-adds from it)
    native.check(native.lib().grip_view_entropy(_ptr(lg), n, views, c, keep, _ptr(loss), _ptr(grad), _ptr(ent), _ptr(sel), _ptr(mean), _stream()))
    out = (loss[0],) + tuple(t for t, want in ((grad, want_grad), (ent, want_entropy), (sel, want_selected), (mean, want_mean)) if want)
    return out if len(out) > 1 else out[0]


class ViewEntropyFn(torch.autograd.Function):
    """logits -> the marginal-entropy loss of engine.view_entropy, native forward + backward (one kernel produces both; the gradient is scaled by the
    incoming scalar in the backward, as WeightedCEFn's is).  apply(logits, views, keep)."""

    @staticmethod
    def forward(ctx, logits, views, keep):
        loss, grad = view_entropy(logits.contiguous().float(), views, keep)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


STREAM_CACHE_MAX_CAP = 16       # csrc/stream_cache.hip: SC_MAX_CAP (a queue lives in 16 lanes)
STREAM_CACHE_MAX_E = 1024       # csrc/stream_cache.hip: SC_MAX_E
STREAM_CACHE_MAX_N = 1 << 30    # csrc/stream_cache.hip: SC_MAX_N
# the paper's ImageNet settings AS RECALLED, untuned here (tda.StreamCache documents them)
STREAM_CACHE_DEFAULTS = dict(pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, neg_entropy=(0.2, 0.5), neg_mask=(0.03, 1.0))
STREAM_CACHE_PLAN_FIELDS = ("entropy", "pred", "negbits", "pos_leave", "neg_leave", "pos_key", "neg_key", "counts")


def check_stream_cache_settings(who, pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, neg_entropy=(0.2, 0.5),
                                neg_mask=(0.03, 1.0)):
    """The settings of a streaming cache as (pos_cap, neg_cap, pos_alpha, pos_beta, neg_alpha, neg_beta, (ent_lo, ent_hi), (mask_lo, mask_hi)), validated
    on the host (no device needed); a bad value raises GripError."""
    for name, val, lo in (("pos_cap", pos_cap, 1), ("neg_cap", neg_cap, 0)):
        if isinstance(val, bool) or not isinstance(val, int) or not lo <= val <= STREAM_CACHE_MAX_CAP:
            raise native.GripError(f"{who}: {name} = {val!r} (an integer in {lo} .. {STREAM_CACHE_MAX_CAP})")
    scal = [_probe_scalar(who, name, val, positive=False)
            for name, val in (("pos_alpha", pos_alpha), ("pos_beta", pos_beta), ("neg_alpha", neg_alpha), ("neg_beta", neg_beta))]
    wins = []
    for name, val in (("neg_entropy", neg_entropy), ("neg_mask", neg_mask)):
        try:
            lo, hi = (float(v) for v in val)
        except (TypeError, ValueError):
            raise native.GripError(f"{who}: {name} = {val!r} (a pair (lo, hi))") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise native.GripError(f"{who}: {name} = ({lo:g}, {hi:g}) (finite, lo <= hi)")
        wins.append((lo, hi))
    return (pos_cap, neg_cap, *scal, *wins)


def _stream_cache_logits(who, base_logits):
    if not torch.is_tensor(base_logits) or base_logits.dim() != 2 or base_logits.dtype != torch.float32 or not base_logits.is_contiguous():
        raise native.GripError(f"{who}: base_logits must be a contiguous float32 [n, c] tensor, got {getattr(base_logits, 'shape', type(base_logits))} "
                               f"{getattr(base_logits, 'dtype', None)}")
    require_gpu(base_logits.device)
    n, c = base_logits.shape
    if not 1 <= n <= STREAM_CACHE_MAX_N or c < 1:
        raise native.GripError(f"{who}: base_logits [{n}, {c}] (1 <= n <= 2^30, c >= 1)")
    return base_logits.detach(), n, c


def stream_cache_plan(base_logits, pos_cap=3, neg_cap=2, neg_entropy=(0.2, 0.5), neg_mask=(0.03, 1.0)):
    """The queue history of a stream of base logits f32 [n, c] (dataset order) under the model of include/grip_amd.h, on the native kernels
    (csrc/stream_cache.hip: a row launch, a scan launch with a wave per (class, polarity), a compaction) -- a dict of device tensors: entropy f32 [n] (H),
    pred int32 [n], negbits int32 [n, ceil(c / 32)], pos_leave / neg_leave int32 [n] (item j sat in its queue during [j, leave_j); leave_j == j: never
    admitted, INT32_MAX: resident at the end), pos_key / neg_key int32 [n] (the ever-admitted items, ascending; only the first counts[0] / counts[1]
    entries are written) and counts int32 [2].  Nothing is read back to the host.  Validated here before the launches; bit-identical from call to call."""
    x, n, c = _stream_cache_logits("stream_cache_plan", base_logits)
    pos_cap, neg_cap, _, _, _, _, (ent_lo, ent_hi), (mask_lo, mask_hi) = check_stream_cache_settings("stream_cache_plan", pos_cap=pos_cap, neg_cap=neg_cap,
                                                                                                  neg_entropy=neg_entropy, neg_mask=neg_mask)
    dev = x.device
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    plan = dict(entropy=torch.empty(n, dtype=torch.float32, device=dev), pred=i32(n), negbits=i32(n, (c + 31) // 32), pos_leave=i32(n), neg_leave=i32(n),
                pos_key=i32(n), neg_key=i32(n), counts=i32(2))
    lib = native.lib()
    ws = _gda_workspace(lib.grip_stream_cache_plan_workspace, (n, c), dev)      # (0 bytes today)
    native.check(lib.grip_stream_cache_plan(_ptr(x), n, c, pos_cap, neg_cap, ent_lo, ent_hi, mask_lo, mask_hi, _ptr(plan["entropy"]), _ptr(plan["pred"]),
                                            _ptr(plan["pos_leave"]), _ptr(plan["neg_leave"]), _ptr(plan["negbits"]), _ptr(plan["pos_key"]),
                                            _ptr(plan["neg_key"]), _ptr(plan["counts"]), _ptr(ws) if ws.numel() else c_void_p(0), ws.numel(), _stream()))
    return plan


def stream_cache_head(base_logits, img_emb, plan, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, negative=True):
    """The adapted logits f32 [n, c] of a stream: base_logits plus the positive and minus the negative cache term of include/grip_amd.h, every item
    against exactly the keys that sat in a queue when it was scored (plan: stream_cache_plan's dict for the SAME base_logits), on the native f32-MFMA kernel
    (csrc/stream_cache.hip).  img_emb f32 [n, e], not normalised.  negative = False leaves the negative term out (the plan of neg_cap = 0 holds none
    anyway).  No host read: the key counts are read on the device."""
    x, n, c = _stream_cache_logits("stream_cache_head", base_logits)
    if not torch.is_tensor(img_emb) or img_emb.dim() != 2 or img_emb.dtype != torch.float32 or img_emb.shape[0] != n or img_emb.device != x.device:
        raise native.GripError(f"stream_cache_head: img_emb must be a float32 [{n}, e] tensor on {x.device}, got {getattr(img_emb, 'shape', type(img_emb))} "
                               f"{getattr(img_emb, 'dtype', None)}")
    e = img_emb.shape[1]
    if e < 4 or e % 4 or e > STREAM_CACHE_MAX_E:
        raise native.GripError(f"stream_cache_head: e = {e} (a multiple of 4 up to {STREAM_CACHE_MAX_E})")
    f = img_emb.detach().contiguous()
    _, _, pos_alpha, pos_beta, neg_alpha, neg_beta, _, _ = check_stream_cache_settings("stream_cache_head", pos_alpha=pos_alpha, pos_beta=pos_beta,
                                                                                       neg_alpha=neg_alpha, neg_beta=neg_beta)
    shapes = dict(pred=(n,), negbits=(n, (c + 31) // 32), pos_leave=(n,), neg_leave=(n,), pos_key=(n,), neg_key=(n,), counts=(2,))
    if not isinstance(plan, dict):
        raise native.GripError(f"stream_cache_head: plan must be the dict of stream_cache_plan, got {type(plan)}")
    for name, shape in shapes.items():
        t = plan.get(name)
        if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != x.device or not t.is_contiguous():
            raise native.GripError(f"stream_cache_head: plan[{name!r}] must be a contiguous int32 {list(shape)} tensor on {x.device}, got "
                                   f"{getattr(t, 'shape', type(t))} {getattr(t, 'dtype', None)}")
    lib = native.lib()
    ws = _gda_workspace(lib.grip_stream_cache_head_workspace, (n, c, e), x.device)
    out = torch.empty_like(x)
    neg = (lambda name: _ptr(plan[name])) if negative else (lambda name: c_void_p(0))
    native.check(lib.grip_stream_cache_head(_ptr(x), _ptr(f), _ptr(plan["pred"]), neg("negbits"), _ptr(plan["pos_leave"]), neg("neg_leave"),
                                            _ptr(plan["pos_key"]), neg("neg_key"), _ptr(plan["counts"]), pos_alpha, pos_beta, neg_alpha, neg_beta, n, c, e,
                                            _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def stream_cache(base_logits, img_emb, pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, neg_entropy=(0.2, 0.5),
                 neg_mask=(0.03, 1.0)):
    """(logits, plan): the whole stream -- stream_cache_plan, then stream_cache_head on its plan (the negative term off when neg_cap = 0).  The rows are
    the sequential item-by-item algorithm's; rows 0 .. k-1 do not depend on the items from k on."""
    plan = stream_cache_plan(base_logits, pos_cap=pos_cap, neg_cap=neg_cap, neg_entropy=neg_entropy, neg_mask=neg_mask)
    return stream_cache_head(base_logits, img_emb, plan, pos_alpha=pos_alpha, pos_beta=pos_beta, neg_alpha=neg_alpha, neg_beta=neg_beta,
                             negative=neg_cap > 0), plan


def leaderboard_scan(probs, pred, path_rank, k):
    """Host scan (exact, sequential).  probs [n,c] f32 CPU, pred [n] int32 CPU, path_rank [n] int64 CPU."""
    import numpy as np
    lib = native.lib()
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    pred = np.ascontiguousarray(pred, dtype=np.int32)
    rank = np.ascontiguousarray(path_rank, dtype=np.int64)
    n, c = probs.shape
    cap = c * max(1, min(int(k), n))
    out_img = np.empty(cap, dtype=np.int32)
    out_cls = np.empty(cap, dtype=np.int32)
    m = c_int64()
    native.check(lib.grip_leaderboard_scan(c_void_p(probs.ctypes.data), c_void_p(pred.ctypes.data), c_void_p(rank.ctypes.data),
                                           n, c, int(k), c_void_p(out_img.ctypes.data), c_void_p(out_cls.ctypes.data), byref(m)))
    return out_img[: m.value].copy(), out_cls[: m.value].copy()


BOUND_FORMS = {"relative": 0, "odds": 1}


def leaderboard_scan_bounded(probs, pred, path_rank, rel_eps, k, abs_eps=0.0, form="relative", threads=0):
    """grip_leaderboard_scan_bounded: (img, cls, ambiguous) with ambiguous a bool [n] array of the rows the caller has to
    re-encode more accurately before the lists can be trusted (include/grip_amd.h).  rel_eps [n]: per-row bound (0 = final) -- a relative
    bound on every probability (form "relative") or a bound on the spread of the row's logit errors (form "odds": every entry's odds
    p / (1 - p) are known to a factor e^{+-delta});  abs_eps: absolute slack of every non-final row;  threads: worker threads of the scan's
    pre-filter (0 = the library's default)."""
    import numpy as np
    lib = native.lib()
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    pred = np.ascontiguousarray(pred, dtype=np.int32)
    rank = np.ascontiguousarray(path_rank, dtype=np.int64)
    eps = np.ascontiguousarray(rel_eps, dtype=np.float32)
    n, c = probs.shape
    cap = n if int(k) == 10000000 else c * max(1, min(int(k), n))
    out_img = np.empty(max(cap, 1), dtype=np.int32)
    out_cls = np.empty(max(cap, 1), dtype=np.int32)
    amb = np.zeros(max(n, 1), dtype=np.uint8)
    m, na = c_int64(), c_int64()
    native.check(lib.grip_leaderboard_scan_bounded(c_void_p(probs.ctypes.data), c_void_p(pred.ctypes.data), c_void_p(rank.ctypes.data),
                                                   c_void_p(eps.ctypes.data), float(abs_eps), BOUND_FORMS[form], int(threads), n, c, int(k),
                                                   c_void_p(out_img.ctypes.data), c_void_p(out_cls.ctypes.data), byref(m), c_void_p(amb.ctypes.data), byref(na)))
    return out_img[: m.value].copy(), out_cls[: m.value].copy(), amb[:n].astype(bool)


# ------------------------------------------------------------------------------------------ CU-masked side stream (look-ahead encodes)
_MASKED_STREAMS = {}


def set_cu_budget(n_cus):
    """grip_set_cu_budget: CUs the persistent kernels may size their grids to for the launches that follow (0 = the whole chip)."""
    native.check(native.lib().grip_set_cu_budget(int(n_cus)))


def masked_stream(device, quarters=3):
    """(torch stream, n_cus) whose kernels may only run on `quarters` / 4 of the chip's CUs (hipExtStreamCreateWithCUMask), or None when the runtime
    refuses.  Every 32-CU XCD and every 8-CU slice of the CU numbering loses the same share whichever way the driver numbers the CUs (CU i is dropped
    when (i / 8 + i) % 4 >= quarters), so the XCD-aware tile walks of the GEMMs stay balanced.  What it is for: a throughput-bound encode on most of
    the chip next to a latency-bound chain of small kernels on the rest (steps.lookahead_image_features)."""
    import ctypes
    import os
    dev = torch.device(device)
    if dev.index is None:           # "cuda": the CURRENT device, not device 0
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev.index, quarters)
    if key in _MASKED_STREAMS:
        return _MASKED_STREAMS[key]
    out = None
    try:
        total = torch.cuda.get_device_properties(dev).multi_processor_count
        words = (total + 31) // 32
        mask = (ctypes.c_uint32 * words)()
        kept = 0
        for i in range(total):
            if (i // 8 + i) % 4 < quarters:
                mask[i // 32] |= 1 << (i % 32)
                kept += 1
        hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        st = ctypes.c_void_p()
        with torch.cuda.device(dev):
            rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), ctypes.c_uint32(words), mask)
        if rc == 0 and st.value:
            out = (torch.cuda.ExternalStream(st.value, device=dev), kept)
    except Exception:
        out = None
    _MASKED_STREAMS[key] = out
    return out
