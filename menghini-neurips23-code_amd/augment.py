"""Train-time augmentation on the GPU: RandomResizedCrop + RandomHorizontalFlip views of the normalised f32 pool (csrc/augment.hip).

The reference's dataset classes take `augmentations=(aug1, aug2)` ("strong and weak", data/dataset.py:18-79) and apply them on the host with
PIL, per item.  Here a view is a box of a pool image resampled to n_px x n_px with Pillow's antialiased bicubic and optionally mirrored, one
launch for a whole batch, and the boxes come from a counter-based sampler: the box of an image in an epoch is a function of
(seed, file name, epoch, view) alone -- not of the batch it is in, of the order of the batch, of the number of ranks or of anything drawn before.
There is no host fall-back: without the library every call raises."""
import math
from ctypes import c_void_p

import numpy as np
import torch

from . import native, rng

# grip_view (include/grip_amd.h), as a numpy record so a batch's descriptors are filled column-wise
_VIEW = np.dtype([("row", "<i8"), ("top", "<i4"), ("left", "<i4"), ("height", "<i4"), ("width", "<i4"), ("flip", "<i4"), ("pad", "<i4")])


def _launch(images, desc, n_views, n_px, out):
    """The one native call of this module (tests replace it to prove that refused arguments never reach it)."""
    N, _, H, W = images.shape
    native.check(native.lib().grip_augment_views(c_void_p(images.data_ptr()), N, H, W, c_void_p(desc.data_ptr()), n_views, n_px,
                                                 c_void_p(out.data_ptr()), c_void_p(torch.cuda.current_stream(images.device).cuda_stream)))


def views(images, boxes, rows=None, n_px=None, out=None):
    """images [N, 3, H, W] f32 (contiguous, on the GPU), boxes int [V, 5] = (top, left, height, width, flip) -> [V, 3, n_px, n_px] f32:
    view v is box v of image rows[v] (default: image v), resampled to n_px x n_px (default H) as PIL's crop(box).resize((n_px, n_px), BICUBIC)
    would, mirrored left-right where flip != 0.  Everything is validated here, on the host, before anything is uploaded or launched."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"views: expected an image tensor [N, 3, H, W], got {tuple(getattr(images, 'shape', ()))}")
    if images.dtype != torch.float32 or not images.is_cuda or not images.is_contiguous():
        raise ValueError(f"views: the source must be a contiguous float32 tensor on the GPU, got {images.dtype} on {images.device}"
                         f"{'' if images.is_contiguous() else ', not contiguous'}")
    N, _, H, W = (int(s) for s in images.shape)
    n_px = H if n_px is None else int(n_px)
    if n_px < 1:
        raise ValueError(f"views: n_px must be at least 1, got {n_px}")
    b = np.asarray(boxes.cpu() if torch.is_tensor(boxes) else boxes)
    if b.size == 0:
        b = b.reshape(0, 5)
    if b.ndim != 2 or b.shape[1] != 5 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"views: boxes must be an integer array [V, 5] of (top, left, height, width, flip), got {b.dtype} {b.shape}")
    b = b.astype(np.int64)
    V = b.shape[0]
    r = np.arange(V, dtype=np.int64) if rows is None else np.asarray(rows.cpu() if torch.is_tensor(rows) else rows).astype(np.int64).reshape(-1)
    if r.shape[0] != V:
        raise ValueError(f"views: {r.shape[0]} rows for {V} boxes")
    top, left, h, w = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    if V and (h.min() < 1 or w.min() < 1):
        raise ValueError("views: a box needs height >= 1 and width >= 1")
    if V and (top.min() < 0 or left.min() < 0 or (top + h).max() > H or (left + w).max() > W):
        raise ValueError(f"views: a box lies outside the {H} x {W} image")
    if V and (r.min() < 0 or r.max() >= N):
        raise ValueError(f"views: a row lies outside 0 .. {N - 1}")
    if out is None:
        out = torch.empty(V, 3, n_px, n_px, dtype=torch.float32, device=images.device)
    elif (tuple(out.shape) != (V, 3, n_px, n_px) or out.dtype != torch.float32 or out.device != images.device or not out.is_contiguous()):
        raise ValueError(f"views: out must be a contiguous float32 [{V}, 3, {n_px}, {n_px}] tensor on {images.device}")
    if V == 0:
        return out
    d = np.zeros(V, dtype=_VIEW)
    d["row"], d["top"], d["left"], d["height"], d["width"], d["flip"] = r, top, left, h, w, b[:, 4] != 0
    desc = torch.from_numpy(d.view(np.uint8)).to(images.device)
    _launch(images, desc, V, n_px, out)
    desc.record_stream(torch.cuda.current_stream(images.device))
    return out


class ViewSampler:
    """torchvision's RandomResizedCrop.get_params + RandomHorizontalFlip as a pure function of (seed, name, epoch, view).

    Per image: up to 10 attempts of area = H W U(scale), aspect = exp(U(log ratio)), w = round(sqrt(area aspect)), h = round(sqrt(area / aspect)),
    accepted when 0 < w <= W and 0 < h <= H, then top uniform in 0 .. H - h and left uniform in 0 .. W - w; when all ten fail, the central box
    of the nearest allowed aspect ratio (the whole image when its own ratio is allowed).  flip = (u <= p) with u in (0, 1]: p = 0 never flips,
    p = 1 always does.

    Key layout.  The draws of one (name, epoch, view) are 41 uniforms of rng.uniform_at's Philox-4x64 stream with
        key     = (seed, rng.stream_id("augment.view/" + name))
        counter = (0, epoch, view, 0)   (lowest word first: it counts the blocks drawn, the sampler never reaches the next word)
    read as u[4 a + 0 .. 3] = (area, aspect, top, left) of attempt a = 0 .. 9 and u[40] = flip.  Every attempt owns its four slots whether or not
    an earlier one was accepted, so nothing depends on how many draws came before."""

    def __init__(self, seed=0, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=0.5):
        self.seed = int(seed)
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.flip = float(flip)
        if not (0.0 < self.scale[0] <= self.scale[1] and 0.0 < self.ratio[0] <= self.ratio[1] and 0.0 <= self.flip <= 1.0):
            raise ValueError(f"ViewSampler: bad scale {scale}, ratio {ratio} or flip {flip}")

    def box(self, name, epoch, H, W, view=0):
        u = rng.uniform_at(self.seed, rng.stream_id("augment.view/" + str(name)), (int(epoch), int(view), 0), 41)
        flip = int(u[40] <= self.flip)
        log_lo, log_hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        for a in range(10):
            ua, ur, ut, ul = u[4 * a:4 * a + 4]
            area = H * W * (self.scale[0] + (self.scale[1] - self.scale[0]) * ua)
            aspect = math.exp(log_lo + (log_hi - log_lo) * ur)
            w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                top = min(int((H - h + 1) * (1.0 - ut)), H - h)
                left = min(int((W - w + 1) * (1.0 - ul)), W - w)
                return top, left, h, w, flip
        r = W / H
        if r < self.ratio[0]:
            w, h = W, int(round(W / self.ratio[0]))
        elif r > self.ratio[1]:
            h, w = H, int(round(H * self.ratio[1]))
        else:
            w, h = W, H
        h, w = min(h, H), min(w, W)
        return (H - h) // 2, (W - w) // 2, h, w, flip

    def boxes(self, names, epoch, H, W, view=0):
        """int32 [len(names), 5] of (top, left, height, width, flip)."""
        return np.array([self.box(n, epoch, H, W, view) for n in names], dtype=np.int32).reshape(len(names), 5)

    def batch(self, images, names, epoch, n_px=None, view=0):
        """images [B, 3, H, W] (row i is the image called names[i]) -> its views [B, 3, n_px, n_px], one launch."""
        return views(images, self.boxes(list(names), epoch, int(images.shape[2]), int(images.shape[3]), view), n_px=n_px)
