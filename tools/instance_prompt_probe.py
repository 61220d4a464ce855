"""Timing of a ViT-B/16 VPT forward + backward (VitPrefixFn, train mode) with one shared prompt [P, d] against one prompt per image [B, P, d]
(GRIP_FWD_PER_IMAGE_PREFIX).  The two differ only in the prompt rows' addresses in the sequence assembly and in the prompt-gradient kernel.
Usage: python tools/instance_prompt_probe.py [--batch 16] [--prefix 16] [--iters 50] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import clip  # noqa: E402
from grip_amd.engine import VitPrefixFn  # noqa: E402


def step_ms(tower, x, prefix, w, iters):
    def once():
        p = prefix.detach().requires_grad_(True)
        (VitPrefixFn.apply(tower, x, p) * w).sum().backward()
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        once()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--prefix", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, _ = clip.load("ViT-B/16", device="cuda")
    tower = m.visual.tower
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(a.batch, 3, 224, 224, device="cuda", generator=g)
    w = torch.randn(a.batch, 512, device="cuda", generator=g)
    shared = 0.02 * torch.randn(a.prefix, 768, device="cuda", generator=g)
    per_image = 0.02 * torch.randn(a.batch, a.prefix, 768, device="cuda", generator=g)
    res = {"batch": a.batch, "prefix": a.prefix, "iters": a.iters}
    for rnd in range(2):        # interleaved rounds: clock drift falls on both forms alike
        for name, p in (("shared", shared), ("per_image", per_image)):
            med, best = step_ms(tower, x, p, w, a.iters)
            res.setdefault(f"{name}_median_ms", []).append(round(med, 4))
            res.setdefault(f"{name}_min_ms", []).append(round(best, 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
