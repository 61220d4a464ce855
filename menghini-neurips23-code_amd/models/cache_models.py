"""Key/value cache adapter (Tip-Adapter, Zhang et al., ECCV 2022) on the native cache head (csrc/cache_head.hip).

The keys are image embeddings of a training set, their values the (pseudo)labels; the classifier adds
    alpha * sum_{j in class y} key_weight[j] * exp(-beta * (1 - normalize(f) . key_j))
to the CLIP logit of class y.  With one-hot values the paper's `exp(...) @ cache_values` IS this per-class sum, so the values are stored as a
class id per key and the keys are grouped by class (class_start [c + 1]): the kernel forms the sums on chip and never builds the [n, m] affinity.
Tip-Adapter-F (`train_keys=True`) fine-tunes the keys alone.
"""
import pickle

import torch
from torch import nn

from ..engine import CacheHeadFn, cache_head
from ..native import GripError


def group_keys_by_class(key_class, n_class):
    """(order [m] int64, class_start [n_class + 1] int32) on the CPU: `order` sorts the keys by class and keeps the given order within a class
    (stable), class y owns the sorted rows class_start[y] .. class_start[y + 1] - 1.  Labels outside 0 .. n_class - 1 raise."""
    kc = torch.as_tensor(key_class).detach().cpu().reshape(-1)
    n_class = int(n_class)
    if n_class < 1 or kc.numel() < 1:
        raise ValueError(f"a cache needs at least one class and one key (n_class = {n_class}, {kc.numel()} keys)")
    if kc.dtype.is_floating_point or kc.dtype == torch.bool:
        raise ValueError(f"key_class must hold integer class ids, got {kc.dtype}")
    kc = kc.to(torch.int64)
    if int(kc.min()) < 0 or int(kc.max()) >= n_class:
        raise ValueError(f"key_class holds labels {int(kc.min())} .. {int(kc.max())}: outside 0 .. {n_class - 1}")
    order = torch.sort(kc, stable=True).indices
    start = torch.zeros(n_class + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(torch.bincount(kc, minlength=n_class), 0)
    return order, start.to(torch.int32)


class TipAdapterModel(nn.Module):
    """keys [m, e] (used as stored: Tip-Adapter initialises them unit-norm, Tip-Adapter-F trains them freely), key_class [m] class ids in
    0 .. n_class - 1, key_weight [m] or None (1).  The rows are regrouped by class with a stable sort; `order` maps a stored row to the row it was given
    as.  forward(image_features, clip_logits) -> clip_logits + cache term, [n, n_class] f32."""

    def __init__(self, keys, key_class, n_class, key_weight=None, alpha=1.0, beta=5.5, train_keys=False):
        super().__init__()
        keys = torch.as_tensor(keys)
        if keys.dim() != 2 or keys.shape[0] != torch.as_tensor(key_class).numel():
            raise ValueError(f"keys {tuple(keys.shape)} and key_class ({torch.as_tensor(key_class).numel()} labels): expected [m, e] and [m]")
        order, start = group_keys_by_class(key_class, n_class)
        dev = keys.device
        keys = keys.detach().float()[order.to(dev)].contiguous()
        self.n_class, self.alpha, self.beta = int(n_class), float(alpha), float(beta)
        self.keys = nn.Parameter(keys, requires_grad=True) if train_keys else keys
        self.register_buffer("order", order.to(dev))
        self.register_buffer("key_class", torch.as_tensor(key_class).detach().cpu().reshape(-1).to(torch.int64)[order].to(dev))
        self.register_buffer("class_start", start.to(dev))
        if key_weight is not None:
            key_weight = torch.as_tensor(key_weight, dtype=torch.float32).detach().reshape(-1)
            if key_weight.numel() != keys.shape[0]:
                raise ValueError(f"key_weight has {key_weight.numel()} entries for {keys.shape[0]} keys")
            key_weight = key_weight.to(dev)[order.to(dev)].contiguous()
        self.register_buffer("key_weight", key_weight)

    @classmethod
    def from_lists(cls, features, labels, is_pseudo, n_class, pseudo_weight=1.0, **kw):
        """The cache of a strategy's training set: features [m, e] (the frozen image tower's embeddings, any norm), labels [m] class positions,
        is_pseudo [m] bools (which rows carry a pseudolabel).  Keys are the unit-normalised features; a labelled key weighs 1, a pseudolabelled one
        `pseudo_weight`."""
        f = torch.as_tensor(features).detach().float()
        keys = f / f.norm(dim=-1, keepdim=True)
        pseudo = torch.as_tensor(list(is_pseudo), dtype=torch.bool)
        weight = None
        if float(pseudo_weight) != 1.0 and bool(pseudo.any()):
            weight = torch.where(pseudo, torch.tensor(float(pseudo_weight)), torch.tensor(1.0))
        return cls(keys, torch.as_tensor(list(labels) if not torch.is_tensor(labels) else labels), n_class, key_weight=weight, **kw)

    def forward(self, image_features, clip_logits):
        if clip_logits.dim() != 2 or clip_logits.shape[1] != self.n_class:
            raise GripError(f"cache of {self.n_class} classes applied to logits {tuple(clip_logits.shape)}")
        return CacheHeadFn.apply(image_features, self.keys, self.class_start, self.key_weight, self.alpha, self.beta, clip_logits)

    @torch.no_grad()
    def search(self, alpha_grid, beta_grid, val_features, val_clip_logits, val_labels):
        """The paper's validation grid search: the (alpha, beta) of the grids with the highest validation accuracy (the first such pair in
        alpha-major order).  Sets self.alpha / self.beta to it and returns (alpha, beta, accuracy)."""
        labels = torch.as_tensor(val_labels).to(val_clip_logits.device)
        best = None
        for a in alpha_grid:
            for b in beta_grid:
                out = cache_head(val_features, self.keys, self.class_start, self.key_weight, float(a), float(b), val_clip_logits)
                acc = float((out.argmax(1) == labels).float().mean())
                if best is None or acc > best[2]:
                    best = (float(a), float(b), acc)
        self.alpha, self.beta = best[0], best[1]
        return best

    # ------------------------------------------------------------------ persistence (a file of its own beside the prompt file)
    def state(self):
        return {"keys": self.keys.detach().cpu().numpy(), "key_class": self.key_class.cpu().numpy(),
                "key_weight": None if self.key_weight is None else self.key_weight.cpu().numpy(), "n_class": self.n_class, "alpha": self.alpha,
                "beta": self.beta}

    def save(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.state(), f)
        return path

    @classmethod
    def load(cls, path, device="cpu", train_keys=False):
        with open(path, "rb") as f:
            s = pickle.load(f)
        kw = None if s["key_weight"] is None else torch.from_numpy(s["key_weight"])
        return cls(torch.from_numpy(s["keys"]).to(device), torch.from_numpy(s["key_class"]), s["n_class"], key_weight=kw, alpha=s["alpha"], beta=s["beta"],
                   train_keys=train_keys)
