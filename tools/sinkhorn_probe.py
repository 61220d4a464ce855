"""Developer probe: times the balanced-assignment kernels (csrc/sinkhorn.hip) against the same recursion written in torch ops in ONE process, after
warm-up, with device events; native and torch windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5,
default 7) windows.

  balance    the pool-sized balance at (n, c) = (50 000, 102), iters 3 and 10: engine.sinkhorn_balance (the host-side prior and the allocations of the
             call included) against torch_balance -- L = tau log(clamp(P)) once, then per iteration  softmax(L + b, 1), sum(0), log  -- an [n, c]
             temporary per iteration; the same final softmax, arg-max and column sum.
  pass       pseudolabels.pseudolabel_from_features at the shapes of BASELINE.json configs[1] (n = 50 000, c = 102, 16 pseudo-shots per class): switch
             off and switch on; wall clock, host scan included

Bytes are computed here from the shapes (a pass reads n c 4 bytes, the final one writes as many); the figures are call times (launches included).
`--out FILE` also writes the JSON there."""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine, pseudolabels as pl  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, pool, summary  # noqa: E402

TINY = 2.0 ** -126
STREAM_TBS = 6.3        # the streaming rate the floor is stated against


def torch_balance(p, log_target, tau, iters):
    L = tau * torch.log(p.clamp_min(TINY))
    b = torch.zeros_like(log_target)
    logn = math.log(p.shape[0])
    for _ in range(iters):
        s = torch.softmax(L + b, dim=1).sum(0)
        b = b + ((log_target + logn) - torch.log(s.clamp_min(TINY)))
    q = torch.softmax(L + b, dim=1)
    return q, q.argmax(dim=1), q.sum(0), b


def balance_case(repeats, n=50000, e=512, c=102, tau=1.0):
    x, centres = pool(n, e, c)
    res = []
    with torch.no_grad():
        probs = engine.cosine_head(x, centres, 100.0)[1]
        lt = torch.full((c,), -math.log(c), device="cuda")
        for iters in (3, 10):
            case = f"balance n={n} c={c} iters={iters}"
            nbytes = (iters + 2) * n * c * 4.0
            res.append({"case": case, "who": "floor (an estimate from the shapes, not a result)", "bytes": nbytes,
                        "stream_floor_us": round(nbytes / (STREAM_TBS * 1e12) * 1e6, 1), "launches": 2 * (iters + 1)})
            ts = alternate({"native": lambda i: engine.sinkhorn_balance(probs, tau, iters), "torch": lambda i: torch_balance(probs, lt, tau, iters)}, 10, repeats)
            for who, t in ts.items():
                res.append(summary(case, who, t))
            res.append({"case": case, "who": "verdict", "native_over_torch": round(res[-2]["us_median"] / res[-1]["us_median"], 3)})
            qn, pn, mn, bn = engine.sinkhorn_balance(probs, tau, iters)
            qt, pt, mt, bt = torch_balance(probs, lt, tau, iters)
            res.append({"case": case, "who": "agreement", "max_abs_difference_q": float((qn - qt).abs().max()), "rows_with_the_same_argmax": float((pn.long() == pt).float().mean()),
                        "max_abs_difference_log_scale": float((bn - bt).abs().max()), "max_column_residual": float((mn / (n / c) - 1).abs().max()),
                        "smallest_argmax_class_before": int(torch.bincount(probs.argmax(1), minlength=c).min()),
                        "smallest_argmax_class_after": int(torch.bincount(pn.long(), minlength=c).min())})
    return res


def pass_case(repeats, n=50000, e=512, c=102, shots=16):
    x, centres = pool(n, e, c)
    paths = [f"/data/pool/img_{i:06d}.jpg" for i in range(n)]
    labels = list(range(c))

    def run(ot):
        ts = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with pl.label_propagation(ot):
                pl.pseudolabel_from_features(x, centres, 100.0, paths, labels, shots)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts[1:]       # (the first pass warms up: path ranks, allocations)
    case = f"pseudolabel pass n={n} c={c} shots={shots} (wall clock, host scan included)"
    return [summary(case, "switch off", run(None)), summary(case, "switch on", run(pl.BalancedAssignment()))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("balance", "pass"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("sinkhorn_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("sinkhorn_probe: needs the GPU (nothing is measured without one)")
    cases = {"balance": balance_case, "pass": pass_case}
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
