"""Gaussian discriminant head (after "A Hard-to-Beat Baseline for Training-free CLIP-based Adaptation", Wang et al., ICLR 2024) on the native
scatter / solve / head kernels (csrc/gda_head.hip).

One Gaussian per class with ONE shared full covariance on the unit image embeddings of a training set is a linear classifier:
    N_c = sum_{y_i = c} r_i,   mu_c = sum_{y_i = c} r_i F_i / N_c   (the zero vector for a class without rows)
    S = sum_i r_i (F_i - mu_{y_i}) (F_i - mu_{y_i})^T,   W = sum_i r_i,   A = S / W + shrink * (tr(S) / (W e)) * I
    w_c = A^-1 mu_c,   bias_c = 1/2 mu_c . w_c - log pi_c,   logits = clip_logits + alpha * (normalize(f) . w_c - bias_c)
It needs no training.  This is NOT the paper's code: the ridge above replaces its empirical-Bayes covariance estimate, pseudolabelled rows may weigh
less than labelled ones (r_i = pseudo_weight), the prior is uniform with log pi_c = 0 unless one is given, and a class without rows has w_c = 0 and
bias_c = 0: it contributes nothing to its logit.
"""
import pickle

import torch
from torch import nn

from ..engine import class_scatter, gmm_mstep, linear_head, spd_solve
from ..native import GripError


def gda_labels(labels, n_class):
    """labels as an int64 CPU vector, validated on the host: integer class positions in 0 .. n_class - 1."""
    y = torch.as_tensor(list(labels) if not torch.is_tensor(labels) else labels).detach().cpu().reshape(-1)
    n_class = int(n_class)
    if n_class < 1 or y.numel() < 1:
        raise ValueError(f"a discriminant head needs at least one class and one row (n_class = {n_class}, {y.numel()} rows)")
    if y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError(f"labels must hold integer class ids, got {y.dtype}")
    y = y.to(torch.int64)
    if int(y.min()) < 0 or int(y.max()) >= n_class:
        raise ValueError(f"labels hold {int(y.min())} .. {int(y.max())}: outside 0 .. {n_class - 1}")
    return y


class GdaHeadModel(nn.Module):
    """mean [C, e] (the class centres, kept for inspection), w [C, e], bias [C].  forward(image_features, clip_logits) -> clip_logits +
    alpha * (normalize(image_features) @ w.T - bias), [n, C] f32, one launch of the native linear head."""

    def __init__(self, mean, w, bias, n_class, alpha=1.0):
        super().__init__()
        mean, w, bias = (torch.as_tensor(t).detach().float().contiguous() for t in (mean, w, bias))
        self.n_class, self.alpha = int(n_class), float(alpha)
        if w.dim() != 2 or w.shape[0] != self.n_class or tuple(mean.shape) != tuple(w.shape) or tuple(bias.shape) != (self.n_class,):
            raise ValueError(f"mean {tuple(mean.shape)}, w {tuple(w.shape)}, bias {tuple(bias.shape)}: expected [C, e], [C, e], [C] with C = {self.n_class}")
        self.register_buffer("mean", mean)
        self.register_buffer("w", w.to(mean.device))
        self.register_buffer("bias", bias.to(mean.device))

    @classmethod
    def fit(cls, features, labels, is_pseudo, n_class, pseudo_weight=1.0, shrink=1.0, alpha=1.0, prior=None):
        """The head of a strategy's training set: features [m, e] (the frozen image tower's embeddings, any norm, on the GPU), labels [m] class
        positions, is_pseudo [m] bools (which rows carry a pseudolabel: they weigh `pseudo_weight`, the others 1), prior [n_class] positive or None
        (uniform, log pi = 0).  Four native calls: gmm_mstep (counts and means), class_scatter, spd_solve; the rows are normalised in torch."""
        f = torch.as_tensor(features).detach().float()
        if f.dim() != 2 or f.shape[0] < 1:
            raise ValueError(f"features {tuple(f.shape)}: expected [m, e]")
        y = gda_labels(labels, n_class)
        pseudo = torch.as_tensor(list(is_pseudo), dtype=torch.bool).reshape(-1)
        if y.numel() != f.shape[0] or pseudo.numel() != f.shape[0]:
            raise ValueError(f"features {tuple(f.shape)}, {y.numel()} labels, {pseudo.numel()} pseudo flags: expected one of each per row")
        if not float(pseudo_weight) >= 0.0 or not float(shrink) >= 0.0:
            raise ValueError(f"pseudo_weight = {pseudo_weight}, shrink = {shrink}: each must be >= 0")
        dev, C = f.device, int(n_class)
        unit = (f / f.norm(dim=-1, keepdim=True)).contiguous()
        r = None
        if float(pseudo_weight) != 1.0 and bool(pseudo.any()):
            r = torch.where(pseudo, torch.tensor(float(pseudo_weight)), torch.tensor(1.0))
        total = float(y.numel()) if r is None else float(r.double().sum())      # W, on the host in float64
        if not total > 0.0:
            raise ValueError("every row has weight 0: nothing to fit")
        yd = y.to(dev)
        z = torch.zeros(f.shape[0], C, dtype=torch.float32, device=dev)
        z.scatter_(1, yd[:, None], (torch.ones(f.shape[0]) if r is None else r).to(dev)[:, None])      # Z_ic = r_i [y_i = c]: one writer per row
        count, mean, _ = gmm_mstep(z, unit)
        S = class_scatter(unit, yd.to(torch.int32), None if r is None else r.to(dev), mean)
        w = spd_solve(S, mean, a_scale=1.0 / total, ridge_rel=float(shrink))
        bias = 0.5 * (mean * w).sum(1)
        if prior is not None:
            p = torch.as_tensor(prior, dtype=torch.float32).detach().reshape(-1)
            if p.numel() != C or not bool((p > 0).all()):
                raise ValueError(f"prior must hold {C} positive entries")
            bias = bias - torch.log(p.to(dev))
        empty = count == 0
        w = torch.where(empty[:, None], torch.zeros_like(w), w)
        bias = torch.where(empty, torch.zeros_like(bias), bias)
        return cls(mean, w, bias, C, alpha=alpha)

    @torch.no_grad()
    def forward(self, image_features, clip_logits):
        if clip_logits.dim() != 2 or clip_logits.shape[1] != self.n_class:
            raise GripError(f"discriminant head of {self.n_class} classes applied to logits {tuple(clip_logits.shape)}")
        return linear_head(image_features.detach().float(), self.w, self.bias, self.alpha, clip_logits.detach().float())

    @torch.no_grad()
    def search(self, alpha_grid, val_features, val_clip_logits, val_labels):
        """The alpha of the grid with the highest validation accuracy (the first such one).  Sets self.alpha to it and returns (alpha, accuracy)."""
        labels = torch.as_tensor(val_labels).to(val_clip_logits.device)
        f, base = val_features.detach().float(), val_clip_logits.detach().float()
        best = None
        for a in alpha_grid:
            _, pred = linear_head(f, self.w, self.bias, float(a), base, want_argmax=True)
            acc = float((pred == labels).float().mean())
            if best is None or acc > best[1]:
                best = (float(a), acc)
        self.alpha = best[0]
        return best

    # ------------------------------------------------------------------ persistence (a file of its own beside the prompt file)
    def state(self):
        return {"mean": self.mean.cpu().numpy(), "w": self.w.cpu().numpy(), "bias": self.bias.cpu().numpy(), "n_class": self.n_class,
                "alpha": self.alpha}

    def save(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.state(), f)
        return path

    @classmethod
    def load(cls, path, device="cpu"):
        with open(path, "rb") as f:
            s = pickle.load(f)
        return cls(torch.from_numpy(s["mean"]).to(device), torch.from_numpy(s["w"]).to(device), torch.from_numpy(s["bias"]).to(device), s["n_class"],
                   alpha=s["alpha"])
