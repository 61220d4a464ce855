"""Developer probe: times the transductive GMM kernels (csrc/gmm_transduce.hip) against the same recursion written in torch ops in ONE process, after
warm-up, with device events; native and torch windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5)
windows.

  transduce  the pool-sized transduction at (n, e, c, k) = (50 000, 512, 102, 3), 10 rounds of 5 sweeps, the graph excluded (built once, outside the
             windows): engine.gmm_transduce against torch_transduce -- per round  Z^T F  and the counts as library matmuls / sums, the variance in its
             EXPANDED form (sum_i r_i F_i^2 - 2 sum_c mu_c S_c + sum_c N_c mu_c^2: three reductions instead of the [n, c, e] differences of the direct
             form the kernels compute, which torch could only do class by class), F (mu / var)^T as a library matmul, and per sweep
             softmax(static + (w[:, :, None] * Z[idx]).sum(1))  -- a [n, k, c] temporary per sweep.  Also the two steps on their own.
  pass       pseudolabels.pseudolabel_from_features at the shapes of BASELINE.json configs[1] (n = 50 000, c = 102, 16 pseudo-shots per class): switch
             off, switch on with the graph rebuilt every pass (visual / multimodal strategies), switch on with the graph kept (textual strategies);
             wall clock, host scan included

FLOPs are computed here from the shapes (per round 2 n c e for the sums, 3 n c e for the direct variance, 2 n c e for the scores); the figures are call
times (launches included).  `--out FILE` also writes the JSON there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine, pseudolabels as pl  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, pool, summary  # noqa: E402

TINY = 2.0 ** -126


def torch_mstep(z, f, var_floor):
    cnt = z.sum(0)
    s = z.T @ f
    mean = torch.where(cnt[:, None] == 0, torch.zeros_like(s), s / cnt[:, None])
    v = (z.sum(1, keepdim=True) * f * f).sum(0) - 2 * (mean * s).sum(0) + (cnt[:, None] * mean * mean).sum(0)        # the expanded form
    return cnt, mean, (v / z.shape[0]).clamp_min(var_floor)


def torch_estep(f, mean, var, logp, ix, w, z, z_iters):
    wm = mean / var
    static = f @ wm.T - 0.5 * (mean * wm).sum(1) + logp
    for _ in range(z_iters):
        z = torch.softmax(static + (w[:, :, None] * z[ix]).sum(1), dim=1)
    return z


def torch_transduce(f, probs, idx, sim, lam, iters, z_iters, var_floor):
    ix, w = idx.long(), sim.clamp_min(0)
    logp = lam * torch.log(probs.clamp_min(TINY))
    z = probs
    for _ in range(iters):
        cnt, mean, var = torch_mstep(z, f, var_floor)
        z = torch_estep(f, mean, var, logp, ix, w, z, z_iters)
    return z, z.argmax(dim=1), mean, var, cnt


def transduce_case(repeats, n=50000, e=512, c=102, k=3, lam=1.0, iters=10, z_iters=5, var_floor=1e-8):
    x, centres = pool(n, e, c)
    case = f"transduction n={n} e={e} c={c} k={k}, {iters} x {z_iters} sweeps (graph excluded)"
    res = []
    with torch.no_grad():
        idx, sim = engine.knn_graph(x, k=k)
        probs = engine.cosine_head(x, centres, 100.0)[1]
        f = torch.nn.functional.normalize(x, dim=1).contiguous()
        flop = iters * 7.0 * n * c * e
        ts = alternate({"native": lambda i: engine.gmm_transduce(f, probs, idx, sim, lam, iters, z_iters, var_floor),
                        "torch": lambda i: torch_transduce(f, probs, idx, sim, lam, iters, z_iters, var_floor)}, 2, repeats)
        for who, t in ts.items():
            res.append(summary(case, who, t, flop_direct_form=flop, launches=iters * (6 + z_iters) if who == "native" else None))
        res.append({"case": case, "who": "verdict", "native_over_torch": round(res[0]["us_median"] / res[1]["us_median"], 3)})
        zn, pn, mn, vn, _ = engine.gmm_transduce(f, probs, idx, sim, lam, iters, z_iters, var_floor)
        zt, pt, mt, vt, _ = torch_transduce(f, probs, idx, sim, lam, iters, z_iters, var_floor)
        res.append({"case": case, "who": "agreement", "max_abs_difference_z": float((zn - zt).abs().max()), "rows_with_the_same_argmax": float((pn.long() == pt).float().mean()),
                    "max_rel_difference_var": float(((vn - vt).abs() / vt).max()), "max_abs_difference_mean": float((mn - mt).abs().max())})
        # the two steps on their own, from the operands of the last round
        ix, w, logp = idx.long(), sim.clamp_min(0), lam * torch.log(probs.clamp_min(TINY))
        ts = alternate({"native": lambda i: engine.gmm_mstep(zn, f, var_floor), "torch": lambda i: torch_mstep(zn, f, var_floor)}, 10, repeats)
        for who, t in ts.items():
            res.append(summary(f"M-step n={n} e={e} c={c}", who, t))
        ts = alternate({"native": lambda i: engine.gmm_estep(f, mn, vn, probs, idx, sim, zn, lam, z_iters),
                        "torch": lambda i: torch_estep(f, mn, vn, logp, ix, w, zn, z_iters)}, 10, repeats)
        for who, t in ts.items():
            res.append(summary(f"E-step n={n} e={e} c={c} k={k}, {z_iters} sweeps", who, t))
    return res


def pass_case(repeats, n=50000, e=512, c=102, shots=16):
    x, centres = pool(n, e, c)
    paths = [f"/data/pool/img_{i:06d}.jpg" for i in range(n)]
    labels = list(range(c))

    def run(gmm):
        ts = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with pl.label_propagation(gmm):
                pl.pseudolabel_from_features(x, centres, 100.0, paths, labels, shots)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts[1:]       # (the first pass warms up: path ranks, allocations, the kept graph)
    case = f"pseudolabel pass n={n} c={c} shots={shots} (wall clock, host scan included)"
    return [summary(case, "switch off", run(None)), summary(case, "switch on, graph rebuilt", run(pl.TransductiveGMM())),
            summary(case, "switch on, graph kept", run(pl.TransductiveGMM(keep_graphs=True)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("transduce", "pass"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("gmm_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("gmm_probe: needs the GPU (nothing is measured without one)")
    cases = {"transduce": transduce_case, "pass": pass_case}
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
