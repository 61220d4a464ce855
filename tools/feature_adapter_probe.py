"""Developer probe: times the CLIP-Adapter feature head (csrc/feature_adapter.hip) against its torch composition in ONE process, after warm-up,
with device events; native and torch windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5) windows.

  pool    forward at (n, e, h) = (50 000, 512, 128): engine.feature_adapter against  r * relu(relu(f @ W1.T) @ W2.T) + (1 - r) * f  in torch
          (two library f32 GEMMs and the elementwise kernels), `hot` (the same operands every call) and `cold` (four feature sets of 102 MB in
          rotation: more than the 256 MiB Infinity Cache holds; the outputs rotate with them)
  train   forward + backward at 64 rows: engine.FeatureAdapterFn against torch autograd of the composition
  step    steps.GraphedAdapterStep replay and steps.adapter_step eager at 64 rows, 102 classes (adapter + cosine head + weighted CE + AdamW)

FLOPs and bytes are computed here from the shapes: forward 4 n e h FLOP, n e * 4 bytes read + n e * 4 written (+ the weights).  The floors printed
with the pool case are those counts over the f32 MFMA peak and the HBM peak; the figures are call times (launch included), so a share of a peak is
NOT derived from them -- that needs kernel time (rocprofv3 --kernel-trace --stats -- python tools/feature_adapter_probe.py --only pool).
`--out FILE` also writes the JSON there."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine, steps  # noqa: E402
from grip_amd.models import ClipAdapterModel  # noqa: E402

PEAK_TF, PEAK_TBS = 155.0, 6.3      # measured f32 matrix peak and HBM bandwidth the floors are stated against


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(fns, iters, repeats, warm=3):
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


def torch_adapter(f, w1, w2, r):
    return r * torch.relu(torch.relu(f @ w1.T) @ w2.T) + (1 - r) * f


def verdict(case, res):
    """The acceptance statement of the case: native median <= torch median + the two spreads."""
    nat, tor = (next(x for x in res if x["case"] == case and x["who"] == w) for w in ("native", "torch"))
    slack = (nat["us_max"] - nat["us_min"]) + (tor["us_max"] - tor["us_min"])
    return {"case": case, "who": "verdict", "native_not_slower_than_torch_beyond_the_spreads": nat["us_median"] <= tor["us_median"] + slack,
            "native_over_torch": round(nat["us_median"] / tor["us_median"], 3)}


def pool_case(repeats, n=50000, e=512, h=128, r=0.2):
    model = ClipAdapterModel(e, seed=1, device="cuda")
    w1, w2 = model.w1.detach(), model.w2.detach()
    g = torch.Generator(device="cuda").manual_seed(1)
    flop, nbytes = 4.0 * n * e * h, 2.0 * n * e * 4 + 2.0 * e * h * 4
    res = [{"case": "pool floors (estimates from the shapes, not results)", "flop": flop, "bytes": nbytes,
            "mfma_floor_us": round(flop / (PEAK_TF * 1e12) * 1e6, 1), "hbm_floor_us": round(nbytes / (PEAK_TBS * 1e12) * 1e6, 1)}]
    for sets, tag in ((1, "hot"), (4, "cold")):
        fs = [torch.randn(n, e, device="cuda", generator=g) * 3 for _ in range(sets)]
        with torch.no_grad():
            ts = alternate({"native": lambda i: engine.feature_adapter(fs[i % sets], w1, w2, r), "torch": lambda i: torch_adapter(fs[i % sets], w1, w2, r)},
                           8 * sets, repeats)
            case = f"pool forward n={n} e={e} h={h} {tag}"
            for who, t in ts.items():
                med = statistics.median(t)
                res.append(summary(case, who, t, tflops_of_call_time=round(flop / (med * 1e-6) / 1e12, 1), tbytes_per_s_of_call_time=round(nbytes / (med * 1e-6) / 1e12, 2)))
            res.append(verdict(case, res))
            if sets == 1:
                res.append({"case": "max |native - torch| / max |torch|, pool",
                            "value": float((engine.feature_adapter(fs[0], w1, w2, r) - torch_adapter(fs[0], w1, w2, r)).abs().max() / torch_adapter(fs[0], w1, w2, r).abs().max())})
        del fs
    return res


def train_case(repeats, n=64, e=512, h=128, r=0.2):
    model = ClipAdapterModel(e, seed=2, device="cuda")
    f = torch.randn(n, e, device="cuda") * 3
    G = torch.randn(n, e, device="cuda")

    def native(i):
        model.w1.grad = model.w2.grad = None
        model(f).backward(G)

    def composed(i):
        model.w1.grad = model.w2.grad = None
        torch_adapter(f, model.w1, model.w2, r).backward(G)

    ts = alternate({"native": native, "torch": composed}, 200, repeats, warm=20)
    case = f"train forward + backward n={n} e={e} h={h}"
    res = [summary(case, who, t, flop=12.0 * n * e * h) for who, t in ts.items()]
    return res + [verdict(case, res)]


def step_case(repeats, n=64, c=102, e=512):
    g = torch.Generator(device="cuda").manual_seed(3)
    text = torch.randn(c, e, device="cuda", generator=g)
    f = torch.randn(n, e, device="cuda", generator=g) * 3
    y = torch.randint(0, c, (n,), device="cuda", dtype=torch.int32)
    w = torch.full((n,), 1.0 / n, device="cuda")
    fns = {}
    for name in ("GraphedAdapterStep replay", "adapter_step eager"):
        model = ClipAdapterModel(e, seed=3, device="cuda")
        opt = torch.optim.AdamW([model.w1, model.w2], lr=1e-3, eps=1e-4)
        if name.startswith("Graphed"):
            step = steps.GraphedAdapterStep(model, text, 100.0, opt)
            fns[name] = lambda i, step=step: step(f, y, w)
        else:
            fns[name] = lambda i, model=model, opt=opt: steps.adapter_step(model, f, text, 100.0, y, w, opt)
    ts = alternate(fns, 100, repeats, warm=10)
    return [summary(f"training step n={n} c={c} e={e}", who, t) for who, t in ts.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("pool", "train", "step"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("feature_adapter_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("feature_adapter_probe: needs the GPU (nothing is measured without one)")
    cases = {"pool": pool_case, "train": train_case, "step": step_case}
    res = []
    for k, fn in cases.items():
        if a.only in (None, k):
            res += fn(a.repeats)
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
