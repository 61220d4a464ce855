"""Cost of deep UPT (UPTModel(mix_deep=True), grip_upt_mixer_*_deep): a graphed UPT step (steps.GraphedUptStep) at the shapes of configs[3]
(ViT-B/16, B = 16, Pt = Pv = 4, C = 47) with the shallow mixer against the same step with D deep embeddings mixed into the sequence and fed to
the tower as deep prompts; and the mixer's forward + backward alone (UptMixerFn, device events), shallow against deep.
Usage: python tools/upt_deep_probe.py [--batch 16] [--prompts 4] [--classes 47] [--deep 11] [--iters 50] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import clip, steps  # noqa: E402
from grip_amd.models import CustomImageEncoder, CustomTextEncoder, UPTModel  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return round(times[len(times) // 2], 4), round(times[0], 4)


def model(m, enc, classes, coop, vpt, deep):
    torch.manual_seed(0)
    return UPTModel(coop.clone(), vpt.clone(), None if deep is None else deep.clone(), CustomImageEncoder(m.visual), enc, classes, 128, device="cuda",
                    dtype=torch.float32, mix_deep=deep is not None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--prompts", type=int, default=4)
    ap.add_argument("--classes", type=int, default=47)
    ap.add_argument("--deep", type=int, default=11)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m, _ = clip.load("ViT-B/16", device="cuda")
    enc = CustomTextEncoder(m, "cuda", torch.float32)
    classes = [f"texture number {i}" for i in range(a.classes)]
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(a.batch, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, a.classes, (a.batch,), device="cuda", generator=g, dtype=torch.int32)
    w = torch.full((a.batch,), 1.0 / a.batch, device="cuda")
    coop = 0.02 * torch.randn(1, a.prompts, 512, device="cuda", generator=g)
    vpt = 0.02 * torch.randn(1, a.prompts, 768, device="cuda", generator=g)
    deep = 0.02 * torch.randn(a.deep, a.prompts, 768, device="cuda", generator=g)
    res = {"batch": a.batch, "prompts": a.prompts, "classes": a.classes, "deep": a.deep, "iters": a.iters}
    for rnd in range(2):        # interleaved rounds: clock drift falls on both forms alike
        for name, dp in (("shallow", None), ("deep", deep)):
            um = model(m, enc, classes, coop, vpt, dp)
            opt = torch.optim.SGD([p for p in um.parameters() if p.requires_grad], lr=1e-3)
            step = steps.GraphedUptStep(um, 100.0, opt)
            med, best = timed(lambda: step(x, y, w), a.iters)
            res.setdefault(f"step_{name}_median_ms", []).append(med)
            res.setdefault(f"step_{name}_min_ms", []).append(best)

            def mixer(um=um):
                outs = um.mix()
                sum(o.square().sum() for o in outs).backward()
            med, best = timed(mixer, a.iters)
            res.setdefault(f"mixer_{name}_median_us", []).append(round(med * 1e3, 1))
            res.setdefault(f"mixer_{name}_min_us", []).append(round(best * 1e3, 1))
            del step, um, opt
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
