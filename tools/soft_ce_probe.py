"""Developer probe: times the soft-target cross-entropy kernel (csrc/soft_ce.hip) in ONE process, after warm-up, with device events; the contenders'
windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5, default 7) windows.

  kernel   grip_soft_ce at 64 x 102 (a batch of 64 rows, 48 of them soft rows of a 50 000 x 102 matrix, temperature 0.5, smoothing 0.1) through the C ABI
           on preallocated outputs, against grip_weighted_ce on the same logits (what the step launches with the switch off), and against grip_soft_ce
           with soft = NULL (the same kernel on hard rows)
  torch    the same loss and gradient as a torch composition: gather the matrix rows, log, scale, log_softmax / softmax, scatter into [B, C] targets,
           smoothing, F.cross_entropy with probability targets, autograd for the gradient -- against engine.soft_ce (allocations of the call included)
  step     the graphed CoOp step on pre-encoded features at the shapes of BASELINE.json configs[1] (ViT-B/16 text tower, 102 classes, 16 context tokens,
           batch 16) with the switch off (WeightedCEFn) and on (SoftCEFn on a 50 000 x 102 matrix)

`--out FILE` also writes the JSON there."""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import grip_amd  # noqa: E402,F401
from grip_amd import clip, engine, native, rng, steps  # noqa: E402
from grip_amd.models import CustomTextEncoder, TextPrefixModel  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, summary  # noqa: E402

TINY = 2.0 ** -126


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def operands(n, c, pool=50000, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = 4 * torch.randn(n, c, device="cuda", generator=g)
    labels = torch.randint(0, c, (n,), device="cuda", generator=g, dtype=torch.int32)
    w = torch.full((n,), 1.0 / n, device="cuda")
    z = torch.softmax(2 * torch.randn(pool, c, device="cuda", generator=g), dim=1)
    rows = torch.randint(0, pool, (n,), device="cuda", generator=g, dtype=torch.int32)
    rows[::4] = -1                                    # a quarter of the batch: labelled rows
    cmap = torch.randperm(c, device="cuda", generator=g).to(torch.int32)
    return logits, labels, w, z, rows, cmap


def torch_soft_ce(logits, labels, w, z, rows, cmap, temperature, smoothing):
    x = logits.detach().clone().requires_grad_(True)
    n, c = x.shape
    soft = rows >= 0
    t = F.one_hot(labels.long(), c).float()
    s = torch.softmax(torch.log(z[rows[soft].long()].clamp_min(TINY)) / temperature, dim=1)
    full = torch.zeros(s.shape[0], c, device=x.device)
    full[:, cmap.long()] = s
    t[soft] = full
    loss = (w * F.cross_entropy(x, t, reduction="none", label_smoothing=smoothing)).sum()
    loss.backward()
    return loss.detach(), x.grad


def kernel_case(repeats, n=64, c=102, temperature=0.5, smoothing=0.1):
    lib = native.lib()
    logits, labels, w, z, rows, cmap = operands(n, c)
    loss, grad = torch.empty(1, device="cuda"), torch.empty_like(logits)
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    inv_t = 1.0 / temperature
    fns = {
        "grip_weighted_ce": lambda i: lib.grip_weighted_ce(_p(logits), _p(labels), _p(w), n, c, _p(loss), _p(grad), s()),
        "grip_soft_ce, soft = NULL": lambda i: lib.grip_soft_ce(_p(logits), _p(labels), _p(w), n, c, None, 0, 0, None, None, 1.0, 0.0, _p(loss), _p(grad), None, s()),
        "grip_soft_ce, 48 soft rows": lambda i: lib.grip_soft_ce(_p(logits), _p(labels), _p(w), n, c, _p(z), z.shape[0], c, _p(rows), _p(cmap), inv_t, smoothing,
                                                                 _p(loss), _p(grad), None, s()),
    }
    case = f"kernel n={n} c={c} (C ABI, preallocated outputs)"
    res = [summary(case, who, t) for who, t in alternate(fns, 200, repeats).items()]
    res.append({"case": case, "who": "verdict", "soft_over_weighted_ce": round(res[2]["us_median"] / res[0]["us_median"], 3),
                "null_over_weighted_ce": round(res[1]["us_median"] / res[0]["us_median"], 3)})
    case = f"call n={n} c={c} (loss + gradient, allocations included)"
    fns = {"engine.soft_ce": lambda i: engine.soft_ce(logits, labels, w, z, rows, cmap, temperature, smoothing),
           "torch composition": lambda i: torch_soft_ce(logits, labels, w, z, rows, cmap, temperature, smoothing)}
    out = [summary(case, who, t) for who, t in alternate(fns, 100, repeats).items()]
    out.append({"case": case, "who": "verdict", "native_over_torch": round(out[0]["us_median"] / out[1]["us_median"], 3)})
    ln, gn = engine.soft_ce(logits, labels, w, z, rows, cmap, temperature, smoothing)
    lt, gt = torch_soft_ce(logits, labels, w, z, rows, cmap, temperature, smoothing)
    out.append({"case": case, "who": "agreement", "loss_difference": float((ln - lt).abs()), "max_abs_difference_grad": float((gn - gt).abs().max())})
    return res + out


def step_case(repeats, C=102, P=16, B=16, pool=50000):
    dev = torch.device("cuda", 0)
    m, _ = clip.load("ViT-B/16", device=dev)
    classes = [f"class_{i}" for i in range(C)]
    enc = CustomTextEncoder(m, dev, torch.float32)
    enc._tok_cache[(P, tuple(classes))] = bench.synth_tokens(C, P).to(dev)
    _, y, w, z, rows, cmap = operands(B, C, pool)
    f = torch.randn(B, m.dims.embed_dim, device=dev)
    fns = {}
    for name, soft in (("switch off", None), ("switch on", steps.SoftTargets(z, cmap, 1.0, 0.0))):
        p0 = torch.from_numpy(rng.normal(1, rng.stream_id("scp.p"), (1, P, m.dims.transformer_width), 0.0, 0.02)).to(dev)
        tm = TextPrefixModel(p0, enc, classes, device=dev)
        opt = torch.optim.SGD([tm.prefix], lr=0.002, weight_decay=0.1)
        g = steps.GraphedCoopFeatureStep(tm, m, opt, soft=soft)
        fns[name] = (lambda i, _g=g: _g(f, y, w)) if soft is None else (lambda i, _g=g: _g(f, y, w, rows))
    case = f"graphed CoOp step C={C} P={P} B={B} (ViT-B/16 text tower, pre-encoded features)"
    res = [summary(case, who, t) for who, t in alternate(fns, 50, repeats, warm=5).items()]
    res.append({"case": case, "who": "verdict", "on_over_off": round(res[1]["us_median"] / res[0]["us_median"], 4)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernel", "step"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("soft_ce_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("soft_ce_probe: needs the GPU (nothing is measured without one)")
    res = []
    for k, fn in {"kernel": kernel_case, "step": step_case}.items():
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
