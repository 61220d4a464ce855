"""float64 reference, bound and inputs for the balanced-assignment kernels (csrc/sinkhorn.hip), shared by the GPU tests and shown to hold for an f32
emulation on the host (tests/test_host_sinkhorn_ref.py).  Everything works on torch tensors of any device.  u = 2^-24 (the unit roundoff of f32; one ulp
is 2 u).  Every term below follows from the inputs, u and the documented 2-ulp accuracy of expf / logf alone; nothing in it is measured.  The reference
runs in float64 on the SAME f32 inputs (P, tau, log_target, the start vector), so only the arithmetic differs.

THE RECURSION (include/grip_amd.h).  L_ic = tau log max(P_ic, 2^-126);  `iters` times  q_i = softmax_c(L_i + b),  s_c = sum_i q_ic,
b_c += log_target_c + log n - log max(s_c, 2^-126);  then Q_i = softmax_c(L_i + b), mass_c = sum_i Q_ic.

THE BOUND, first order in u, carried from step to step.  beta_c bounds |b_c - b64_c|; beta = 0 at the start (both sides take the same f32 vector).
    L           logf within 2 ulp = 4 u relative, the product (or the fused multiply-add it ends in) u, one u of room:      6 u tau |log max(P, 2^-126)|
    argument    a_ic = L_ic + b_c:    ba_ic = 6 u tau |log| + beta_c + u |a_ic|                                (the addition rounds once)
    softmax     the row's maximum is subtracted first (neutral but for the rounding of the difference, u (max_i - a_ic), and 2 u max_c ba_ic for the
                kernel's own maximum and argument):    ba'_ic = ba_ic + u (max_i - a_ic) + 2 u max_c ba_ic
                a softmax whose arguments move by at most ba'_c moves EXACTLY within the monotone interval of tests/gmm_ref.py (no linearisation)
                    lo_c = q_c e^{-ba'_c} / (q_c e^{-ba'_c} + sum_{j != c} q_j e^{+ba'_j}),   hi_c = q_c e^{+ba'_c} / (q_c e^{+ba'_c} + sum_{j != c} q_j e^{-ba'_j})
                its own arithmetic (expf 4 u, the sum of c terms c u, the division u; with room):    bq_ic = max(hi - q, q - lo) + (c + 8) u q_ic + 2^-126
    column sum  n non-negative terms in any order:    bs_c = sum_i bq_ic + n u s_c + 2^-126        (the clamp at 2^-126 moves nothing apart)
    b           with rho_c = bs_c / max(s_c, 2^-126) (the checker asserts rho_c < 1/2 on its inputs) the logarithm of the kernel's sum is off by at most
                -log(1 - rho_c), logf adds 4 u |log| (one u of room: 5 u), float(log n) u log n, the sum log_target + log n u |log_target_c + log n|, the
                difference d_c u |d_c| and the addition u |b_c|:
                    beta_c <- beta_c - log(1 - rho_c) + 5 u |log max(s_c, 2^-126)| + u log n + u |log_target_c + log n| + u |d_c| + u |b_c (new)| + 2^-126
Q is checked under bq, mass under bs, log_scale under beta; pred is the FIRST maximum of the kernel's own row, exactly.  The bound loosens by roughly
3 x per iteration (beta feeds every argument of the next one): the tight checks are the single steps (iters = 0, and iters = 1 from a given b); the
multi-iteration check guards against gross errors and claims no precision."""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
ROWS = 16       # the fixed row partition of the column sums (engine.SINKHORN_ROWS; csrc/sinkhorn.hip SK_ROWS)


def log_target_of(c, prior=None, device="cpu"):
    """The f32 log_target engine.sinkhorn_balance passes on: the prior normalised in float64 (None: uniform), its log rounded to f32."""
    if prior is None:
        return torch.full((c,), math.log(1.0 / c), dtype=torch.float32, device=device)
    t = torch.as_tensor(prior, dtype=torch.float64).cpu()
    return torch.log(t / t.sum()).float().to(device)


def _step64(L, b, beta, tau_abs_log):
    """(q, bq, s, bs) of one softmax step in float64 under the argument error bound beta [c]."""
    n, c = L.shape
    a = L + b
    ba = 6 * U * tau_abs_log + beta + U * a.abs()
    mx = a.max(dim=1, keepdim=True).values
    ba = ba + U * (mx - a) + 2 * U * ba.max(dim=1, keepdim=True).values
    q = torch.softmax(a, dim=1)
    up, dn = q * torch.exp(ba), q * torch.exp(-ba)
    hi = up / (up + (dn.sum(1, keepdim=True) - dn).clamp_min(0.0)).clamp_min(TINY)
    lo = dn / (dn + (up.sum(1, keepdim=True) - up).clamp_min(0.0)).clamp_min(TINY)
    bq = torch.maximum(hi - q, q - lo).clamp_min(0.0) + (c + 8) * U * q + TINY
    s = q.sum(0)
    return q, bq, s, bq.sum(0) + n * U * s + TINY


def balance64(p, log_target, tau, iters, b0=None, bounds=False):
    """(Q64 [n, c], mass64 [c], b64 [c]) of the recursion in float64 on the f32 inputs; with bounds=True also (bq, bs, beta, worst rho) of the module
    docstring."""
    n, c = p.shape
    tau = float(np.float32(tau))
    logp = torch.log(p.double().clamp_min(TINY))
    L, tal = tau * logp, tau * logp.abs()
    lt = log_target.double()
    b = torch.zeros(c, dtype=torch.float64, device=p.device) if b0 is None else b0.double().clone()
    beta = torch.zeros_like(b)
    rho_max = 0.0
    for _ in range(iters):
        _, _, s, bs = _step64(L, b, beta, tal)
        sc = s.clamp_min(TINY)
        rho = bs / sc
        rho_max = max(rho_max, float(rho.max()))
        logs = torch.log(sc)
        d = lt + math.log(n) - logs
        b = b + d
        beta = beta - torch.log1p(-rho.clamp_max(0.999)) + 5 * U * logs.abs() + U * math.log(n) + U * (lt + math.log(n)).abs() + U * d.abs() + U * b.abs() + TINY
    q, bq, s, bs = _step64(L, b, beta, tal)
    return (q, s, b, bq, bs, beta + TINY, rho_max) if bounds else (q, s, b)


def check_balance(p, log_target, tau, iters, b0, q, pred, mass, log_scale):
    """Assert every element of Q, mass and log_scale against float64 and pred (the first maximum of Q's own row); returns the worst |err| / bound."""
    q64, s64, b64, bq, bs, beta, rho = balance64(p, log_target, tau, iters, b0, bounds=True)
    assert rho < 0.5, f"balance: rho = {rho:.3g} on these inputs: the bound of the logarithm does not apply"
    worst = 0.0
    for name, got, want, b in (("Q", q, q64, bq), ("mass", mass, s64, bs), ("log_scale", log_scale, b64, beta)):
        err = (got.double() - want).abs()
        ratio = float((err / b).max())
        assert torch.isfinite(got).all() and (err <= b).all(), f"balance: |{name} - {name}64| is {ratio:.2f} x its bound"
        worst = max(worst, ratio)
    if pred is not None:
        first = np.argmax(q.cpu().numpy(), axis=1)
        assert np.array_equal(pred.cpu().numpy().astype(np.int64), first), "balance: pred is not the first maximum of the row"
    return worst


def balance_f32(p, log_target, tau, iters, b0=None):
    """An f32 emulation of the kernels in torch (no fused multiply-add, torch's own summation order): what the checker must accept."""
    n, c = p.shape
    L = torch.tensor(tau, dtype=torch.float32) * torch.log(p.clamp_min(TINY))
    b = torch.zeros(c, dtype=torch.float32) if b0 is None else b0.clone()
    logn = torch.tensor(math.log(n), dtype=torch.float32)

    def step(b):
        a = L + b
        x = torch.exp(a - a.max(dim=1, keepdim=True).values)
        return x / x.sum(1, keepdim=True)
    for _ in range(iters):
        s = step(b).sum(0)
        b = b + ((log_target + logn) - torch.log(s.clamp_min(TINY)))
    q = step(b)
    return q, torch.from_numpy(np.argmax(q.numpy(), axis=1).astype(np.int32)), q.sum(0), b


# ------------------------------------------------------------------------------------------ inputs and cases
def inputs(n, c, kind, seed):
    """P [n, c] f32: softmax rows of randn logits plus a per-class bias N(0, 1) (an imbalanced marginal).  kind "peaked": the logits x 30 (saturated rows:
    most entries underflow towards 0); "zeros": scattered exact zeros (the 2^-126 clamp), never a whole column."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, c, generator=g) + torch.randn(c, generator=g)
    if kind == "peaked":
        logits = logits * 30
    p = torch.softmax(logits, dim=1)
    if kind == "zeros":
        p[torch.rand(n, c, generator=g) < 0.3] = 0.0
        p[0, :] = 0.0
        keep = torch.randint(0, n, (c,), generator=g)
        p[keep, torch.arange(c)] = p[keep, torch.arange(c)].clamp_min(1e-3)       # every column keeps a non-zero entry
    return p


def advanced_start(p, log_target, tau, iters=5):
    """b after `iters` float64 iterations, rounded to f32: a start vector at which the balance already holds roughly."""
    return balance64(p, log_target, tau, iters)[2].float()


def planted_pool(n, c, seed, shift=2.5, bias_sd=1.5):
    """(P f32 [n, c], labels [n]): n / c rows per class, logits = N(0, 1) noise + `shift` on the true class + a per-class bias N(0, bias_sd^2) -- a head
    that is right about the images and wrong about the marginal."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.arange(n) % c
    logits = torch.randn(n, c, generator=g, dtype=torch.float64) + bias_sd * torch.randn(c, generator=g, dtype=torch.float64)
    logits[torch.arange(n), labels] += shift
    return torch.softmax(logits, dim=1).float(), labels


NS = (1, 63, ROWS, ROWS + 1, 2 * ROWS + 1, 8 * ROWS + 5)       # the last: more than one workgroup (four chunks each)
CS = (1, 2, 64, 65, 102, 128, 129, 1000)
SHAPES = [(n, 102) for n in NS] + [(ROWS + 1, c) for c in CS if c != 102] + [(8 * ROWS + 5, 129)]
KINDS = ("plain", "peaked", "zeros")
# (iters, start, tau, prior): start "zeros" or "advanced" (advanced_start); prior None or "ramp" (weights 1 .. c)
STEPS = [(0, "zeros", 1.0, None), (0, "advanced", 1.0, None), (1, "advanced", 1.0, None), (3, "zeros", 1.0, None), (1, "advanced", 1.0, "ramp"),
         (3, "zeros", 1.0, "ramp"), (0, "advanced", 0.5, None), (1, "advanced", 2.0, None), (3, "zeros", 0.5, None)]
# "peaked" pools leave columns whose first sum lies in the subnormal range at tau = 1 (logits x 30: whole columns near e^-100): rho >= 1/2 there, an f32
# sum of such terms has no relative accuracy and nothing bounds its logarithm, so three iterations from zeros are checked on them at tau = 0.5 only
# (where rho < 1/2 holds); their single steps, from zeros and from an advanced b, are checked at every tau.
CASES = [(n, c, kind, *step) for (n, c) in SHAPES for kind in KINDS for step in STEPS if not (kind == "peaked" and step[:3] == (3, "zeros", 1.0))]


def case_operands(case):
    """(P, log_target, tau, iters, b0 or None) of a case, on the CPU."""
    n, c, kind, iters, start, tau, prior = case
    p = inputs(n, c, kind, seed=n * 1000 + c)
    lt = log_target_of(c, None if prior is None else torch.arange(1, c + 1, dtype=torch.float64))
    b0 = advanced_start(p, lt, tau) if start == "advanced" else None
    return p, lt, tau, iters, b0


def case_id(case):
    return "-".join(f"{v:g}" if isinstance(v, float) else str(v) for v in case)
