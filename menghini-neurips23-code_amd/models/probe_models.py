"""Trained linear probe (the "linear probe" of the CLIP and CoOp papers; text-initialised as in LP++, Huang et al., CVPR 2024) on the native loss-and-
gradient kernels (csrc/linear_probe.hip).

A residual on the CLIP logits that starts at zero, trained by cross-entropy on the unit image embeddings of a training set:
    x_ic = clip_logits_ic + scale * (u_i . W_c) + b_c
    J(W, b) = nu sum_i r_i (T_i lse(x_i) - t_i . x_i) + (l2 / 2) |W|^2,      nu = 1 / sum_i r_i,   t = onehot(label) or a given soft row,   T_i = sum_c t_ic
    full-batch heavy-ball descent (torch.optim.SGD(momentum) semantics), `iters` iterations, three launches each, from zeros or from `init`
    logits = clip_logits + alpha * (scale * normalize(f) . W_c + b_c)        (one launch of the native linear head with w = scale W, bias = -b)
This is NOT LP++'s or CLIP's code: there is no learned per-class blending and no line search; the step defaults to the reciprocal of a Lipschitz
bound of the gradient (a bound, not a tuned value), the regulariser pulls W back to the zero-shot (or prompt-tuned) classifier the residual starts at.
"""
import pickle

import torch
from torch import nn

from ..engine import linear_head, probe_fit
from ..native import GripError
from .gda_models import gda_labels


def probe_default_lr(scale, l2):
    """1 / (1/2 (scale^2 + 1) + l2): the reciprocal of a Lipschitz bound on the gradient of J -- the cross-entropy's Hessian in the logits is below I / 2,
    the rows are unit vectors (the scale^2 for W, the 1 for b), nu normalises the weights, the ridge adds l2.  A bound, not a tuned value."""
    return 1.0 / (0.5 * (float(scale) ** 2 + 1.0) + float(l2))


class LinearProbeModel(nn.Module):
    """w [C, e], b [C].  forward(image_features, clip_logits) -> clip_logits + alpha * (scale * normalize(image_features) @ w.T + b), [n, C] f32, one
    launch of the native linear head.  loss_trace (after fit): the data term at the start of every iteration, f32 [iters] on the device."""

    def __init__(self, w, b, n_class, scale=100.0, alpha=1.0):
        super().__init__()
        w, b = (torch.as_tensor(t).detach().float().contiguous() for t in (w, b))
        self.n_class, self.scale, self.alpha = int(n_class), float(scale), float(alpha)
        if w.dim() != 2 or w.shape[0] != self.n_class or tuple(b.shape) != (self.n_class,) or not self.scale > 0:
            raise ValueError(f"w {tuple(w.shape)}, b {tuple(b.shape)}, scale {self.scale:g}: expected [C, e], [C] with C = {self.n_class} and scale > 0")
        self.register_buffer("w", w)
        self.register_buffer("b", b.to(w.device))
        self.loss_trace = None

    @classmethod
    def fit(cls, features, clip_logits, labels, is_pseudo, n_class, soft=None, pseudo_weight=1.0, scale=100.0, l2=0.1, iters=300, momentum=0.9, lr=None,
            alpha=1.0, init=None):
        """The probe of a strategy's training set: features [m, e] (the frozen image tower's embeddings, any norm, on the GPU), clip_logits [m, C] (the
        logits of the trained prompts on the same rows: the classifier the residual starts at) or None (0), labels [m] class positions -- or -1 on the
        rows that have a soft target --, is_pseudo [m] bools (those rows weigh `pseudo_weight`, the others 1), soft [m, C] non-negative or None: the target of
        every row whose label is -1 (the other rows of it are not read).  lr = None: probe_default_lr(scale, l2), the reciprocal of a Lipschitz bound of
        the gradient -- a bound, not a tuned value.  init = (w [C, e], b [C]) or None (zeros): e.g. a GdaHeadModel's (w / scale, -bias).  The rows
        are normalised in torch; everything else is engine.probe_fit."""
        f = torch.as_tensor(features).detach().float()
        if f.dim() != 2 or f.shape[0] < 1:
            raise ValueError(f"features {tuple(f.shape)}: expected [m, e]")
        C, dev = int(n_class), f.device
        y = torch.as_tensor(list(labels) if not torch.is_tensor(labels) else labels).detach().cpu().reshape(-1)
        soft_rows = (y == -1) if not (y.dtype.is_floating_point or y.dtype == torch.bool) else torch.zeros(y.numel(), dtype=torch.bool)
        if bool(soft_rows.any()) and soft is None:
            raise ValueError("a label of -1 marks a row with a soft target, and no soft matrix was given")
        y = torch.where(soft_rows, torch.full_like(y, -1), gda_labels(torch.where(soft_rows, torch.zeros_like(y), y), C))      # (gda_labels' rules for the rest)
        pseudo = torch.as_tensor(list(is_pseudo), dtype=torch.bool).reshape(-1)
        if y.numel() != f.shape[0] or pseudo.numel() != f.shape[0]:
            raise ValueError(f"features {tuple(f.shape)}, {y.numel()} labels, {pseudo.numel()} pseudo flags: expected one of each per row")
        if not float(pseudo_weight) >= 0.0 or not float(l2) >= 0.0 or not float(scale) > 0.0 or int(iters) < 1:
            raise ValueError(f"pseudo_weight = {pseudo_weight}, l2 = {l2}, scale = {scale}, iters = {iters}: >= 0, >= 0, > 0, >= 1")
        sf = None
        if soft is not None:
            sf = torch.as_tensor(soft).detach().float().to(dev).contiguous()
            if tuple(sf.shape) != (f.shape[0], C) or bool((sf[soft_rows.to(dev)] < 0).any()):
                raise ValueError(f"soft {tuple(sf.shape)}: expected non-negative [{f.shape[0]}, {C}]")
        base = None
        if clip_logits is not None:
            base = torch.as_tensor(clip_logits).detach().float().to(dev).contiguous()
            if tuple(base.shape) != (f.shape[0], C):
                raise ValueError(f"clip_logits {tuple(base.shape)}: expected [{f.shape[0]}, {C}]")
        unit = (f / f.norm(dim=-1, keepdim=True)).contiguous()
        r = None
        if float(pseudo_weight) != 1.0 and bool(pseudo.any()):
            r = torch.where(pseudo, torch.tensor(float(pseudo_weight)), torch.tensor(1.0))
        total = float(y.numel()) if r is None else float(r.double().sum())      # 1 / nu, on the host in float64: every row contributes unless its weight is 0
        if not total > 0.0:
            raise ValueError("every row has weight 0: nothing to fit")
        if init is None:
            w0, b0 = torch.zeros(C, f.shape[1], device=dev), torch.zeros(C, device=dev)
        else:
            w0, b0 = (torch.as_tensor(t).detach().float().to(dev).contiguous() for t in init)
            if tuple(w0.shape) != (C, f.shape[1]) or tuple(b0.shape) != (C,):
                raise ValueError(f"init {tuple(w0.shape)}, {tuple(b0.shape)}: expected [{C}, {f.shape[1]}], [{C}]")
        lr = probe_default_lr(scale, l2) if lr is None else float(lr)
        w, b, _, trace = probe_fit(unit, base, y.to(device=dev, dtype=torch.int32), sf, None if r is None else r.to(dev), float(scale), float(l2), lr,
                                   float(momentum), int(iters), w0, b0, want_trace=True, norm=1.0 / total)
        model = cls(w, b, C, scale=scale, alpha=alpha)
        model.loss_trace = trace
        return model

    @torch.no_grad()
    def forward(self, image_features, clip_logits):
        if clip_logits.dim() != 2 or clip_logits.shape[1] != self.n_class:
            raise GripError(f"linear probe of {self.n_class} classes applied to logits {tuple(clip_logits.shape)}")
        return linear_head(image_features.detach().float(), self.w * self.scale, -self.b, self.alpha, clip_logits.detach().float())

    @torch.no_grad()
    def search(self, alpha_grid, val_features, val_clip_logits, val_labels):
        """The alpha of the grid with the highest validation accuracy (the first such one).  Sets self.alpha to it and returns (alpha, accuracy)."""
        labels = torch.as_tensor(val_labels).to(val_clip_logits.device)
        f, base = val_features.detach().float(), val_clip_logits.detach().float()
        w, bias = self.w * self.scale, -self.b
        best = None
        for a in alpha_grid:
            _, pred = linear_head(f, w, bias, float(a), base, want_argmax=True)
            acc = float((pred == labels).float().mean())
            if best is None or acc > best[1]:
                best = (float(a), acc)
        self.alpha = best[0]
        return best

    # ------------------------------------------------------------------ persistence (a file of its own beside the prompt file)
    def state(self):
        return {"w": self.w.cpu().numpy(), "b": self.b.cpu().numpy(), "n_class": self.n_class, "scale": self.scale, "alpha": self.alpha}

    def save(self, path):
        with open(path, "wb") as f:
            pickle.dump(self.state(), f)
        return path

    @classmethod
    def load(cls, path, device="cpu"):
        with open(path, "rb") as f:
            s = pickle.load(f)
        return cls(torch.from_numpy(s["w"]).to(device), torch.from_numpy(s["b"]).to(device), s["n_class"], scale=s["scale"], alpha=s["alpha"])
