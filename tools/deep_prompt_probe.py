"""Cost of deep visual prompts (VPT-Deep, grip_vit_forward_deep): a graphed ViT-B/16 VPT step (steps.GraphedVptStep) with a shallow prompt [P, d]
against the same step with D deep prompts [D, P, d] as a second trained parameter, and a pool encode (pseudolabels.encode_pool) shallow against deep.
Deep prompts add one row-insert launch per replaced block to the forward and one extract-and-zero launch per block to the backward.
Usage: python tools/deep_prompt_probe.py [--batch 16] [--prefix 16] [--deep 11] [--iters 50] [--pool 8800] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import clip, pseudolabels as pl, steps  # noqa: E402
from grip_amd.models import CustomImageEncoder, ImagePrefixModel  # noqa: E402


def step_ms(m, txt, x, y, w, prefix, deep, iters):
    im = ImagePrefixModel(prefix.clone(), CustomImageEncoder(m.visual), device="cuda", deep_prefix=None if deep is None else deep.clone())
    opt = torch.optim.SGD([p for p in (im.prefix, im.deep_prefix) if p is not None], lr=1e-3)
    step = steps.GraphedVptStep(im, txt, 100.0, opt)
    for _ in range(5):
        step(x, y, w)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(x, y, w)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def encode_s(tower, pool, prefix, deep):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pl.encode_pool(tower, pool, chunk=880, prefix=prefix, deep=deep)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--prefix", type=int, default=16)
    ap.add_argument("--deep", type=int, default=11)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pool", type=int, default=8800)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, _ = clip.load("ViT-B/16", device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(a.batch, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 10, (a.batch,), device="cuda", generator=g, dtype=torch.int32)
    w = torch.full((a.batch,), 1.0 / a.batch, device="cuda")
    with torch.no_grad():
        txt = m.encode_text(clip.tokenize([f"a photo of a thing number {i}" for i in range(10)]).cuda())
    prefix = 0.02 * torch.randn(a.prefix, 768, device="cuda", generator=g)
    deep = 0.02 * torch.randn(a.deep, a.prefix, 768, device="cuda", generator=g)
    pool = torch.randn(a.pool, 3, 224, 224, device="cuda", generator=g, dtype=torch.float16)
    res = {"batch": a.batch, "prefix": a.prefix, "deep": a.deep, "iters": a.iters, "pool": a.pool}
    encode_s(m.visual.tower, pool, prefix, deep)      # warm-up: workspaces, streams
    for rnd in range(2):        # interleaved rounds: clock drift falls on both forms alike
        for name, dp in (("shallow", None), ("deep", deep)):
            med, best = step_ms(m, txt, x, y, w, prefix, dp, a.iters)
            res.setdefault(f"step_{name}_median_ms", []).append(round(med, 4))
            res.setdefault(f"step_{name}_min_ms", []).append(round(best, 4))
            res.setdefault(f"encode_{name}_s", []).append(round(encode_s(m.visual.tower, pool, prefix, dp), 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
