"""Feature adapter (CLIP-Adapter, Gao et al., 2021) on the native kernel (csrc/feature_adapter.hip).

A bias-free bottleneck MLP on the image embedding, blended back into it:
    x  = relu(relu(f @ w1.T) @ w2.T)        w1 [h, e], w2 [e, h], h = e / reduction
    f* = ratio * x + (1 - ratio) * f        f: the un-normalised output of the (frozen) image tower
and the cosine head normalises f* as it normalises f.  One launch; a row's bits depend on that row and the weights only, so any batching of the rows
returns the same features.
"""
import math
import pickle

import torch
from torch import nn

from ..engine import FeatureAdapterFn, feature_adapter

# the kernel's domain (include/grip_amd.h, grip_feature_adapter_forward)
_E_STEP, _E_MAX, _H_STEP, _H_MIN, _H_MAX = 64, 1024, 16, 16, 256


class ClipAdapterModel(nn.Module):
    """Parameters w1 [h, e] and w2 [e, h], initialised as nn.Linear(bias=False) initialises them (U(+-1 / sqrt(fan_in))) from a generator of the
    model's own seeded with `seed`: the global torch RNG is neither read nor advanced, so switching the adapter on moves no other random draw of a
    run.  forward(image_features [n, e]) -> adapted features [n, e] f32."""

    def __init__(self, embed_dim, reduction=4, ratio=0.2, seed=0, device="cpu"):
        super().__init__()
        e, red = int(embed_dim), int(reduction)
        if red < 1 or e < 1 or e % red != 0:
            raise ValueError(f"embed_dim = {e} is not a multiple of reduction = {red}")
        h = e // red
        if e % _E_STEP != 0 or e > _E_MAX or h % _H_STEP != 0 or not _H_MIN <= h <= _H_MAX:
            raise ValueError(f"embed_dim = {e} with reduction = {red} gives a hidden width of {h}: the adapter kernel takes embed_dim a multiple of "
                             f"{_E_STEP} up to {_E_MAX} and a hidden width that is a multiple of {_H_STEP}, {_H_MIN} .. {_H_MAX}")
        self.embed_dim, self.hidden_dim, self.reduction, self.ratio, self.seed = e, h, red, float(ratio), int(seed)
        g = torch.Generator().manual_seed(int(seed))
        b1, b2 = 1.0 / math.sqrt(e), 1.0 / math.sqrt(h)
        self.w1 = nn.Parameter(((torch.rand(h, e, generator=g) * 2 - 1) * b1).to(device))
        self.w2 = nn.Parameter(((torch.rand(e, h, generator=g) * 2 - 1) * b2).to(device))

    def forward(self, image_features):
        if torch.is_grad_enabled() and (self.w1.requires_grad or self.w2.requires_grad):
            return FeatureAdapterFn.apply(image_features, self.w1, self.w2, self.ratio)
        return feature_adapter(image_features, self.w1, self.w2, self.ratio)      # inference: the hidden activations stay on chip

    # ------------------------------------------------------------------ persistence (a file of its own beside the prompt file)
    def state(self):
        return {"w1": self.w1.detach().cpu().numpy(), "w2": self.w2.detach().cpu().numpy(), "ratio": self.ratio, "reduction": self.reduction,
                "seed": self.seed}

    def save(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.state(), f)
        return path

    @classmethod
    def load(cls, path, device="cpu"):
        with open(path, "rb") as f:
            s = pickle.load(f)
        m = cls(s["w1"].shape[1], reduction=s["reduction"], ratio=s["ratio"], seed=s["seed"], device=device)
        with torch.no_grad():
            m.w1.copy_(torch.from_numpy(s["w1"]))
            m.w2.copy_(torch.from_numpy(s["w2"]))
        return m
