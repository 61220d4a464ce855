"""Developer probe: times the Tip-Adapter cache head (csrc/cache_head.hip) in one process, after warm-up, min .. max over five repeats of device-event
windows.

  pool    forward at (n, m, c, e) = (50 000, 1 632, 102, 512): us per call and TF/s of 2 n m e against the 157 TF/s f32 MFMA peak -- `hot` (the same
          operands every call) and `cold` (four operand sets of 102 MB + 20 MB in rotation: more than the 256 MiB Infinity Cache holds);
          at m = 1 024, the largest the cosine head takes, against what could be done before: grip_cosine_head with the keys as classes, then torch
          exp and index_add (which writes the [n, m] affinity to memory)
  train   forward + backward at (64, 1 632, 102, 512) through engine.CacheHeadFn
  step    steps.GraphedTipStep replay at the same shape (cache head forward + weighted CE + cache head backward + SGD)

`--only pool|train|step` runs one case (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/cache_head_probe.py --only pool);
`--out FILE` also writes the JSON there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import engine, steps  # noqa: E402
from grip_amd.models import TipAdapterModel  # noqa: E402

PEAK_TF = 157.3


def timed(fn, iters, repeats=5):
    """us per call: (min, max) over `repeats` event-timed windows of `iters` calls."""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return min(out), max(out)


def operands(n, m, c, e, seed, sets=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    keys = torch.randn(m, e, device="cuda", generator=g)
    keys = keys / keys.norm(dim=1, keepdim=True)
    key_class = torch.arange(m, device="cuda") * c // m      # m / c keys per class, grouped
    fs = [torch.randn(n, e, device="cuda", generator=g) for _ in range(sets)]
    ls = [torch.randn(n, c, device="cuda", generator=g) for _ in range(sets)]
    return keys, key_class, fs, ls


def report(name, n, m, e, t):
    flop = 2.0 * n * m * e
    tf = [flop / (x * 1e-6) / 1e12 for x in (t[1], t[0])]
    return {"case": name, "us_min": round(t[0], 1), "us_max": round(t[1], 1), "tflops_min": round(tf[0], 2), "tflops_max": round(tf[1], 2),
            "share_of_f32_mfma_peak": round(tf[1] / PEAK_TF, 3)}


def pool_case(n=50000, c=102, e=512):
    res = []
    for m, sets, tag in ((1632, 1, "hot"), (1632, 4, "cold"), (1024, 1, "hot")):
        keys, key_class, fs, ls = operands(n, m, c, e, 1, sets)
        model = TipAdapterModel(keys, key_class.cpu(), c, alpha=1.0, beta=5.5)
        with torch.no_grad():
            fn = lambda i: model(fs[i % sets], ls[i % sets])      # noqa: E731  (includes the clone of the logits the head adds into)
            for i in range(3 * sets):
                fn(i)
            res.append(report(f"pool forward m={m} {tag}", n, m, e, timed(fn, 4 * sets)))
    # what a user could do before: the cosine head with the keys as its classes (<= 1 024), exp and a per-class index_add in torch
    keys, key_class, fs, ls = operands(n, 1024, c, e, 1)

    def before(i):
        s = engine.cosine_head(fs[0], keys, 1.0, want_probs=False)[0]
        return ls[0].clone().index_add_(1, key_class, torch.exp(-5.5 * (1.0 - s)))

    with torch.no_grad():
        for i in range(3):
            before(i)
        res.append(report("before: cosine head + torch exp + index_add, m=1024 hot", n, 1024, e, timed(before, 4)))
        model = TipAdapterModel(keys, key_class.cpu(), c, alpha=1.0, beta=5.5)
        res.append({"case": "max |cache head - before| at m=1024", "value": float((model(fs[0], ls[0]) - before(0)).abs().max())})
    return res


def train_case(n=64, m=1632, c=102, e=512):
    keys, key_class, fs, ls = operands(n, m, c, e, 2)
    model = TipAdapterModel(keys, key_class.cpu(), c, alpha=1.0, beta=5.5, train_keys=True)
    G = torch.randn(n, c, device="cuda")

    def fwd_bwd(i):
        model.keys.grad = None
        model(fs[0], ls[0]).backward(G)

    for i in range(10):
        fwd_bwd(i)
    r = report("train forward + backward (CacheHeadFn, eager)", n, m, e, timed(fwd_bwd, 50))
    r["flop_counted"] = "2 n m e (forward only); the backward is two more products of that size"
    return [r]


def step_case(n=64, m=1632, c=102, e=512):
    keys, key_class, fs, ls = operands(n, m, c, e, 3)
    model = TipAdapterModel(keys, key_class.cpu(), c, alpha=1.0, beta=5.5, train_keys=True)
    opt = torch.optim.SGD([model.keys], lr=1e-3)
    y = torch.randint(0, c, (n,), device="cuda", dtype=torch.int32)
    w = torch.full((n,), 1.0 / n, device="cuda")
    out = []
    for name, fn in (("GraphedTipStep replay", steps.GraphedTipStep(model, opt)),
                     ("tip_step eager", lambda f, yy, ww, z: steps.tip_step(model, f, z, yy, ww, opt))):
        call = lambda i: fn(fs[0], y, w, ls[0])      # noqa: E731
        for i in range(10):
            call(i)
        t = timed(call, 50)
        out.append({"case": name, "us_min": round(t[0], 1), "us_max": round(t[1], 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("pool", "train", "step"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cache_head_probe: needs the GPU (nothing is measured without one)")
    cases = {"pool": pool_case, "train": train_case, "step": step_case}
    res = []
    for k, fn in cases.items():
        if a.only in (None, k):
            res += fn()
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
