"""Cost of deep text prompts (deep CoOp, grip_text_forward_deep) at the shapes of BASELINE.json configs[1]: ViT-B/16 text tower, C = 102 classes,
P = 16 context tokens.  A graphed CoOp step on pre-encoded features (steps.GraphedCoopFeatureStep: text tower forward + backward, head, loss, SGD)
with the shallow context [1, P, d] against the same step with D deep prompts [D, P, d] as a second trained parameter, and the eager inference text
encode (CustomTextEncoder under no_grad) shallow against deep.  Deep prompts add one row-insert launch per replaced block to the forward and one
extract-and-zero launch per block to the backward.  Every figure is reported per repeat, so the run-to-run spread (min .. max) can be read off.
--deep 0 times the shallow forms only (what a build without the feature can run as well).
Usage: python tools/text_deep_probe.py [--classes 102] [--prefix 16] [--deep 11] [--batch 16] [--iters 200] [--repeats 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import grip_amd  # noqa: E402,F401
from grip_amd import clip, rng, steps  # noqa: E402
from grip_amd.models import CustomTextEncoder, TextPrefixModel  # noqa: E402


def timed_ms(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=102)
    ap.add_argument("--prefix", type=int, default=16)
    ap.add_argument("--deep", type=int, default=11)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    m, _ = clip.load("ViT-B/16", device=dev)
    C, P, B, d = a.classes, a.prefix, a.batch, m.dims.transformer_width
    classes = [f"class_{i}" for i in range(C)]
    enc = CustomTextEncoder(m, dev, torch.float32)
    enc._tok_cache[(P, tuple(classes))] = bench.synth_tokens(C, P).to(dev)
    N = lambda name, shape: torch.from_numpy(rng.normal(1, rng.stream_id(name), shape, 0.0, 0.02)).to(dev)      # noqa: E731
    f = torch.randn(B, m.dims.embed_dim, device=dev)
    y = torch.randint(0, C, (B,), device=dev, dtype=torch.int32)
    w = torch.full((B,), 1.0 / B, device=dev)
    forms = {"shallow": None}
    if a.deep:
        forms["deep"] = N("tdp.d", (a.deep, P, d))
    fns = {}
    for name, deep in forms.items():
        kw = {} if deep is None else {"deep_prefix": deep.clone()}
        tm = TextPrefixModel(N("tdp.p", (1, P, d)), enc, classes, device=dev, **kw)
        opt = torch.optim.SGD([p for p in tm.parameters() if p.requires_grad], lr=0.002, weight_decay=0.1)
        g = steps.GraphedCoopFeatureStep(tm, m, opt)
        for _ in range(10):
            g(f, y, w)

        def encode(_tm=tm):
            with torch.no_grad():
                _tm(classes)
        for _ in range(10):
            encode()
        fns[name] = (lambda _g=g: _g(f, y, w), encode)
    res = {"classes": C, "prefix": P, "deep": a.deep, "batch": B, "iters": a.iters}
    for _ in range(a.repeats):        # interleaved repeats: clock drift falls on both forms alike
        for name, (step, encode) in fns.items():
            res.setdefault(f"step_{name}_ms", []).append(round(timed_ms(step, a.iters), 4))
            res.setdefault(f"encode_{name}_ms", []).append(round(timed_ms(encode, a.iters), 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
