"""Developer probe: times the Gaussian discriminant head (csrc/gda_head.hip; models.GdaHeadModel) against the same model composed from torch library
ops in ONE process, after warm-up, with device events; native and torch windows ALTERNATE inside the run, and every figure is the median and
min .. max over `--repeats` (default 7, >= 5) windows.

  fit-train  GdaHeadModel.fit at 1 632 x 512, C = 102 (16 shots of 102 classes: a strategy's training set)
  fit-pool   the same at 50 000 x 512, C = 102 (a whole pool with pseudolabels)
  head       the pool-sized head at 50 000 x 512 x 102: engine.linear_head against normalize + matmul + the epilogue in torch
The torch fit is one-hot matmul means, d^T (r d) as a library matmul, torch.linalg.cholesky + torch.cholesky_solve; both sides include the row
normalisation and the host's label handling.  The native fit's time includes spd_solve's read of its info word (one synchronisation).  A line on
which the native form is slower says so (`native_over_torch` > 1).  `--out FILE` also writes the JSON there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine  # noqa: E402
from grip_amd.models import GdaHeadModel  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, pool, summary  # noqa: E402


def torch_fit(feats, y, C, shrink=1.0):
    f = feats / feats.norm(dim=-1, keepdim=True)
    z = torch.zeros(f.shape[0], C, device=f.device)
    z.scatter_(1, y[:, None], 1.0)
    cnt = z.sum(0)
    mean = torch.where(cnt[:, None] == 0, torch.zeros(C, f.shape[1], device=f.device), (z.T @ f) / cnt.clamp_min(1)[:, None])
    d = f - mean[y]
    S = d.T @ d
    W, e = float(f.shape[0]), f.shape[1]
    A = S / W + shrink * torch.trace(S) / (W * e) * torch.eye(e, device=f.device)
    w = torch.cholesky_solve(mean.T.contiguous(), torch.linalg.cholesky(A)).T.contiguous()
    return mean, w, 0.5 * (mean * w).sum(1)


def torch_head(f, w, bias, alpha, base):
    return base + alpha * (torch.nn.functional.normalize(f, dim=1) @ w.T - bias)


def fit_case(repeats, n, e=512, C=102, iters=3):
    x, _ = pool(n, e, C, seed=2)
    y = torch.arange(n, device="cuda") % C
    yl, pseudo = y.cpu(), [False] * n
    case = f"fit n={n} e={e} C={C}"
    with torch.no_grad():
        ts = alternate({"native": lambda i: GdaHeadModel.fit(x, yl, pseudo, C), "torch": lambda i: torch_fit(x, y, C)}, iters, repeats)
        res = [summary(case, who, t) for who, t in ts.items()]
        res.append({"case": case, "who": "verdict", "native_over_torch": round(res[0]["us_median"] / res[1]["us_median"], 3)})
        m = GdaHeadModel.fit(x, yl, pseudo, C)
        _, wt, bt = torch_fit(x, y, C)
        res.append({"case": case, "who": "agreement", "max_rel_difference_w": float((m.w - wt).abs().max() / wt.abs().max()),
                    "max_abs_difference_bias": float((m.bias - bt).abs().max())})
    return res


def head_case(repeats, n=50000, e=512, C=102, iters=10):
    x, centres = pool(n, e, C, seed=3)
    w, bias = (centres * 40).contiguous(), torch.linspace(0, 5, C, device="cuda")
    base = engine.cosine_head(x, centres, 100.0, want_probs=False)[0]
    case = f"head n={n} e={e} C={C}"
    with torch.no_grad():
        ts = alternate({"native": lambda i: engine.linear_head(x, w, bias, 1.0, base, want_argmax=True),
                        "torch": lambda i: torch_head(x, w, bias, 1.0, base).argmax(1)}, iters, repeats)
        res = [summary(case, who, t, flop=2.0 * n * C * e) for who, t in ts.items()]
        res.append({"case": case, "who": "verdict", "native_over_torch": round(res[0]["us_median"] / res[1]["us_median"], 3)})
        a, b = engine.linear_head(x, w, bias, 1.0, base), torch_head(x, w, bias, 1.0, base)
        res.append({"case": case, "who": "agreement", "max_abs_difference": float((a - b).abs().max()),
                    "rows_with_the_same_argmax": float((a.argmax(1) == b.argmax(1)).float().mean())})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("fit-train", "fit-pool", "head"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("gda_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("gda_probe: needs the GPU (nothing is measured without one)")
    cases = {"fit-train": lambda r: fit_case(r, 1632), "fit-pool": lambda r: fit_case(r, 50000), "head": head_case}
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
