"""float64 statement of the feature adapter (csrc/feature_adapter.hip) with the error bounds of its f32 kernels; torch, any device.

    u_pre = F W1^T,  H = relu(u_pre),  z = H W2^T,  x = relu(z),  out = r x + (1 - r) F            W1 [h, e], W2 [e, h]

Bounds (u = 2^-24; nothing in them comes from a measurement -- an f32 fmaf chain of k terms in any order is within (k + 8) u sum |terms|):
    a_ik  = sum_d |F_id W1_kd|              du_ik = (e + 8) u a_ik                        (hidden pre-activation; ReLU is 1-Lipschitz, so dH = du)
    dz_ij = sum_k du_ik |W2_jk| + (h + 8) u sum_k H_ik |W2_jk|                            (the pre-activation of x, and x itself)
    forward   |err_ij| <= r dz_ij + 4 u (|r x_ij| + |(1 - r) F_ij|) + 2^-126
    backward  (hidden and act are INPUTS of the backward: the float64 reference reads the very values the kernel reads, so no mask is in doubt)
              dX = r G o [act > 0]
              |err grad_w2_jk| <= (n + 8) u sum_i |dX_ij| |H_ik|
              ddH_ik = (e + 8) u sum_j |dX_ij W2_jk|
              |err grad_w1_kd| <= sum_i [H_ik > 0] (ddH_ik + (n + 8) u |dH_ik|) |F_id| + 2^-126
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126

# (n, e, h) of the kernel tests: one row, one fragment, a ragged second 64-row tile, every accumulator count the forward is compiled for
# (h / 16 <= 2, 4, 8, 12, 16), a hidden width that is no power of two (192), the largest e and h
CASES = [(1, 64, 16), (16, 64, 16), (70, 64, 16), (64, 128, 32), (130, 256, 64), (64, 512, 128), (67, 768, 192), (33, 1024, 256)]


def inputs(n, e, h, seed, zero_row=None):
    """(F [n, e] = randn times a per-row scale in 0.1 .. 30, W1, W2 = U(+-1 / sqrt(fan_in)), G [n, e] = randn), f32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, e, generator=g) * (0.1 + 29.9 * torch.rand(n, 1, generator=g))
    w1 = (torch.rand(h, e, generator=g) * 2 - 1) / math.sqrt(e)
    w2 = (torch.rand(e, h, generator=g) * 2 - 1) / math.sqrt(h)
    G = torch.randn(n, e, generator=g)
    if zero_row is not None:
        f[zero_row] = 0
    return f, w1, w2, G


def forward(f, w1, w2, r):
    """dict of float64 tensors: u_pre, H, z, x, out and the bounds du (for H), dz (for x), b_out."""
    F, A, B = f.double(), w1.double(), w2.double()
    e, h = A.shape[1], A.shape[0]
    u_pre = F @ A.T
    H = u_pre.clamp(min=0)
    z = H @ B.T
    x = z.clamp(min=0)
    out = r * x + (1 - r) * F
    du = (e + 8) * U * (F.abs() @ A.abs().T)
    dz = du @ B.abs().T + (h + 8) * U * (H @ B.abs().T)
    b_out = r * dz + 4 * U * ((r * x).abs() + ((1 - r) * F).abs()) + TINY
    return dict(u_pre=u_pre, H=H, z=z, x=x, out=out, du=du, dz=dz, b_out=b_out)


def doubtful(fwd):
    """Number of pre-activations that lie within their forward bound of zero: there an f32 forward may clip what float64 keeps (or the reverse),
    and a gradient computed from its masks is not comparable with float64 autograd."""
    return int((fwd["u_pre"].abs() <= fwd["du"]).sum() + (fwd["z"].abs() <= fwd["dz"]).sum())


def backward(f, w2, hidden, act, G, r, hidden_err=None):
    """dict of float64 tensors: grad_w1 [h, e], grad_w2 [e, h], dH and the bounds b_w1, b_w2.  hidden / act: the post-ReLU tensors the kernel is
    given (any dtype; read as they are).  hidden_err [n, h] (optional): when the backward under test reads a hidden tensor that is NOT the one given
    here but within hidden_err of it element-wise (an f32 forward's, du of the forward bounds) with the same masks, grad_w2 = dX^T hidden inherits
    sum_i |dX_ij| hidden_err_ik, which is added to b_w2; grad_w1 reads hidden through its mask only."""
    F, B, H, X, Gd = f.double(), w2.double(), hidden.double(), act.double(), G.double()
    n, e = F.shape
    dX = r * Gd * (X > 0)
    gw2 = dX.T @ H
    b_w2 = (n + 8) * U * (dX.abs().T @ H.abs())
    if hidden_err is not None:
        b_w2 = b_w2 + dX.abs().T @ hidden_err.double()
    live = (H > 0).double()
    dH = (dX @ B) * live
    ddH = (e + 8) * U * (dX.abs() @ B.abs())
    gw1 = dH.T @ F
    b_w1 = (live * (ddH + (n + 8) * U * dH.abs())).T @ F.abs() + TINY
    return dict(grad_w1=gw1, grad_w2=gw2, dH=dH, b_w1=b_w1, b_w2=b_w2)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0: an exact zero under a zero bound)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
