"""Developer probe: times the trained linear probe (csrc/linear_probe.hip; engine.probe_fit) against the same recursion composed from torch ops in ONE
process, after warm-up, with device events; native and torch windows ALTERNATE inside the run, and every figure is the median and min .. max over
`--repeats` (default 7, >= 5) windows.

  fit-train  engine.probe_fit, 300 iterations at 1 632 x 512, C = 102 (16 shots of 102 classes: a strategy's training set)
  fit-pool   the same at 50 000 x 512, C = 102 (a whole pool with pseudolabels)
  step       ONE iteration's kernels on their own at both sizes (engine.probe_objective: the score + CE-gradient kernel, the contraction, the finaliser)
The torch recursion is the same heavy-ball descent on unit rows without autograd: x = base + scale u W^T + b, p = softmax(x), g = (p - onehot) / n,
grad_w = scale g^T u + l2 W, grad_b = sum g, m = mu m + grad, (W, b) -= lr m; the loss of every iteration stays on the device (no synchronisation on
either side).  Both sides start from the same unit rows, labels and base.  A line on which the native form is slower says so (`native_over_torch` > 1).
`--out FILE` also writes the JSON there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine  # noqa: E402
from grip_amd.models.probe_models import probe_default_lr  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, pool, summary  # noqa: E402

SCALE, L2, MU = 100.0, 1.0, 0.9


def torch_fit(u, base, y, iters, lr):
    n, (C, e) = u.shape[0], (base.shape[1], u.shape[1])
    W, b = torch.zeros(C, e, device=u.device), torch.zeros(C, device=u.device)
    mw, mb = torch.zeros_like(W), torch.zeros_like(b)
    onehot = torch.nn.functional.one_hot(y, C).float()
    trace = torch.empty(iters, device=u.device)
    rows = torch.arange(n, device=u.device)
    for it in range(iters):
        x = torch.addmm(base + b, u, W.T, alpha=SCALE)
        lp = torch.log_softmax(x, dim=1)
        trace[it] = -lp[rows, y].mean()
        g = (lp.exp() - onehot) / n
        mw = MU * mw + (SCALE * (g.T @ u) + L2 * W)
        mb = MU * mb + g.sum(0)
        W = W - lr * mw
        b = b - lr * mb
    return W, b, trace


def inputs(n, e, C, seed):
    x, centres = pool(n, e, C, seed=seed)
    u = torch.nn.functional.normalize(x, dim=1).contiguous()
    y = torch.arange(n, device="cuda") % C
    base = (SCALE * u @ torch.nn.functional.normalize(centres + 0.05 * torch.randn_like(centres), dim=1).T).contiguous()
    return u, base, y


def fit_case(repeats, n, e=512, C=102, iters=300, windows_iters=2):
    u, base, y = inputs(n, e, C, seed=4)
    y32, lr = y.to(torch.int32), probe_default_lr(SCALE, L2)
    w0, b0 = torch.zeros(C, e, device="cuda"), torch.zeros(C, device="cuda")
    case = f"fit n={n} e={e} C={C} iters={iters}"
    with torch.no_grad():
        native = lambda i: engine.probe_fit(u, base, y32, None, None, SCALE, L2, lr, MU, iters, w0, b0, want_trace=True, norm=1.0 / n)      # noqa: E731
        ts = alternate({"native": native, "torch": lambda i: torch_fit(u, base, y, iters, lr)}, windows_iters, repeats)
        res = [summary(case, who, t, us_per_iteration=round(sorted(t)[len(t) // 2] / iters, 2)) for who, t in ts.items()]
        res.append({"case": case, "who": "verdict", "native_over_torch": round(res[0]["us_median"] / res[1]["us_median"], 3)})
        W, b, _, tr = native(0)
        Wt, bt, trt = torch_fit(u, base, y, iters, lr)
        res.append({"case": case, "who": "agreement", "max_rel_difference_w": float((W - Wt).abs().max() / Wt.abs().max()),
                    "max_abs_difference_b": float((b - bt).abs().max()), "loss_first": [float(tr[0]), float(trt[0])], "loss_last": [float(tr[-1]), float(trt[-1])]})
    return res


def step_case(repeats, iters=20):
    res = []
    for n in (1632, 50000):
        e, C = 512, 102
        u, base, y = inputs(n, e, C, seed=5)
        y32 = y.to(torch.int32)
        g = torch.Generator(device="cuda").manual_seed(6)
        W, b = torch.randn(C, e, device="cuda", generator=g) * 0.01, torch.randn(C, device="cuda", generator=g) * 0.1
        case = f"step n={n} e={e} C={C}"
        per, slices = engine.probe_slices(n, C, e)
        moved = 4.0 * (2 * n * e + n * C + 2 * n * C + 2 * slices * C * e + 2 * C * e)      # feats twice, base, g written and read, partials written and read, W and grad_w
        with torch.no_grad():
            ts = alternate({"native": lambda i: engine.probe_objective(u, W, b, base, y32, None, None, SCALE, 1.0 / n)}, iters, repeats)
        res.append(summary(case, "native", ts["native"], flop=4.0 * n * C * e, bytes=moved, slices=slices, rows_per_slice=per * engine.PROBE_ROWS))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("fit-train", "fit-pool", "step"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("linear_probe_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("linear_probe_probe: needs the GPU (nothing is measured without one)")
    cases = {"fit-train": lambda r: fit_case(r, 1632), "fit-pool": lambda r: fit_case(r, 50000), "step": step_case}
    res = []
    for k, fn in cases.items():
        if a.only in (None, k):
            res += fn(a.repeats)
            torch.cuda.empty_cache()
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
