"""Developer probe: times the label-propagation kernels (csrc/knn_graph.hip) against their torch compositions in ONE process, after warm-up, with
device events; native and torch windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5) windows.

  graph   the pool graph at (n, e, k) = (50 000, 512, 16): engine.knn_graph (pool on pool) against chunked torch -- F.normalize once, then per
          4 096-row chunk a library f32 matmul against the whole pool, the self column masked, topk (the [chunk, n] scores round-trip through HBM)
  walk    10 propagation iterations at c = 102 on that graph: engine.label_propagate against the torch gather form
          (softmax weights once, then per iteration  (1 - a) P + a (W[:, :, None] * Z[idx]).sum(1)  -- a [n, k, c] temporary per iteration)
  pass    pseudolabels.pseudolabel_from_features at the shapes of BASELINE.json configs[1] (n = 50 000, c = 102, 16 pseudo-shots per class): switch
          off, switch on with the graph rebuilt every pass (visual / multimodal strategies), switch on with the graph kept (textual strategies);
          wall clock, host scan included

FLOPs and bytes are computed here from the shapes: graph 2 n^2 e FLOP; walk per iteration n k c * 4 bytes gathered.  The floor printed with the
graph case is that count over the f32 MFMA peak; the figures are call times (launch included).  `--out FILE` also writes the JSON there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine, pseudolabels as pl  # noqa: E402

PEAK_TF = 157.0      # f32 matrix peak the floor is stated against


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, iters, repeats, warm=1):
    """{name: [us per call of each window]}: per repeat one window of every contender, in turn."""
    for fn in fns.values():
        for i in range(warm):
            fn(i)
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def summary(case, name, ts, **extra):
    r = {"case": case, "who": name, "us_median": round(statistics.median(ts), 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1), "windows": len(ts)}
    r.update(extra)
    return r


def pool(n, e, classes=102, seed=1):
    """A class-structured pool: unit centres + noise, row scales 0.1 .. 30 (embeddings come un-normalised)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = F.normalize(torch.randn(classes, e, device="cuda", generator=g), dim=1)
    y = torch.randint(0, classes, (n,), device="cuda", generator=g)
    x = centres[y] + 0.5 / e ** 0.5 * torch.randn(n, e, device="cuda", generator=g)
    return x * (0.1 + 29.9 * torch.rand(n, 1, device="cuda", generator=g)), centres


def torch_knn(x, k, chunk=4096):
    xn = F.normalize(x, dim=1)
    idx, sim = [], []
    for lo in range(0, x.shape[0], chunk):
        s = xn[lo:lo + chunk] @ xn.T
        r = torch.arange(s.shape[0], device=x.device)
        s[r, lo + r] = -float("inf")
        v, i = s.topk(k, dim=1)
        idx.append(i)
        sim.append(v)
    return torch.cat(idx).to(torch.int32), torch.cat(sim)


def torch_walk(probs, idx, sim, alpha, gamma, iters):
    w = torch.softmax(gamma * sim, dim=1)
    ix, z = idx.long(), probs
    for _ in range(iters):
        z = (1 - alpha) * probs + alpha * (w[:, :, None] * z[ix]).sum(1)
    return z, z.argmax(dim=1)


def graph_case(repeats, n=50000, e=512, k=16):
    x, _ = pool(n, e)
    flop = 2.0 * n * n * e
    case = f"pool graph n={n} e={e} k={k}"
    res = [{"case": "graph floor (an estimate from the shapes, not a result)", "flop": flop, "mfma_floor_us": round(flop / (PEAK_TF * 1e12) * 1e6, 1)}]
    with torch.no_grad():
        ts = alternate({"native": lambda i: engine.knn_graph(x, k=k), "torch": lambda i: torch_knn(x, k)}, 1, repeats)
        for who, t in ts.items():
            res.append(summary(case, who, t, tflops_of_call_time=round(flop / (statistics.median(t) * 1e-6) / 1e12, 1)))
        (ni, ns), (ti, tsim) = engine.knn_graph(x, k=k), torch_knn(x, k)
        same = (torch.sort(ni, dim=1).values == torch.sort(ti, dim=1).values).all(dim=1).float().mean().item()
        res.append({"case": case, "who": "agreement", "rows_with_the_same_neighbour_set": round(same, 5), "max_abs_sim_difference": float((ns - tsim).abs().max())})
    nat, tor = res[1], res[2]
    res.append({"case": case, "who": "verdict", "native_over_torch": round(nat["us_median"] / tor["us_median"], 3)})
    return res


def walk_case(repeats, n=50000, e=512, c=102, k=16, alpha=0.8, gamma=10.0, iters=10):
    x, centres = pool(n, e)
    with torch.no_grad():
        idx, sim = engine.knn_graph(x, k=k)
        probs = engine.cosine_head(x, centres, 100.0)[1]
        ts = alternate({"native": lambda i: engine.label_propagate(probs, idx, sim, alpha, gamma, iters),
                        "torch": lambda i: torch_walk(probs, idx, sim, alpha, gamma, iters)}, 3, repeats)
        case = f"{iters} propagation iterations n={n} c={c} k={k}"
        gathered = 4.0 * n * k * c * iters
        res = [summary(case, who, t, gathered_bytes=gathered, tbytes_per_s_gathered_of_call_time=round(gathered / (statistics.median(t) * 1e-6) / 1e12, 2))
               for who, t in ts.items()]
        zn, zt = engine.label_propagate(probs, idx, sim, alpha, gamma, iters)[0], torch_walk(probs, idx, sim, alpha, gamma, iters)[0]
        res.append({"case": case, "who": "agreement", "max_abs_difference": float((zn - zt).abs().max())})
    res.append({"case": case, "who": "verdict", "native_over_torch": round(res[0]["us_median"] / res[1]["us_median"], 3)})
    return res


def pass_case(repeats, n=50000, e=512, c=102, shots=16):
    x, centres = pool(n, e)
    paths = [f"/data/pool/img_{i:06d}.jpg" for i in range(n)]
    labels = list(range(c))

    def run(lp):
        ts = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with pl.label_propagation(lp):
                pl.pseudolabel_from_features(x, centres, 100.0, paths, labels, shots)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts[1:]       # (the first pass warms up: path ranks, allocations, the kept graph)
    case = f"pseudolabel pass n={n} c={c} shots={shots} (wall clock, host scan included)"
    return [summary(case, "switch off", run(None)), summary(case, "switch on, graph rebuilt", run(pl.LabelPropagation())),
            summary(case, "switch on, graph kept", run(pl.LabelPropagation(keep_graphs=True)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("graph", "walk", "pass"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("label_prop_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("label_prop_probe: needs the GPU (nothing is measured without one)")
    cases = {"graph": graph_case, "walk": walk_case, "pass": pass_case}
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
