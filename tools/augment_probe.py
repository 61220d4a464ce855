"""Developer probe: times the train-time augmentation (csrc/augment.hip, grip_amd.augment) in one process, after warm-up, with device events.

  kernel  grip_augment_views at 16, 816 (51 x 16: one look-ahead group) and 4 096 views of 224 x 224 with RandomResizedCrop boxes, out of a pool of
          3 600 images (2.17 GB); every call reads other pool rows and writes another output buffer, so neither side is cache-resident.  us per call
          (min .. max over five windows) and written bytes per second next to the 6.3 TB/s streaming rate.  `with sampler`: the same call through
          ViewSampler.batch (host-side box draws + descriptor upload included, wall clock).
  vpt     a graphed ViT-B/16 VPT step (steps.GraphedVptStep, batch 16) fed its batch as it is / through ViewSampler.batch first
  coop    one CoOp epoch (TextualPrompt._train_epoch, 102 classes x 18 images, batch 16) with AUGMENT off (cached frozen features), off with
          CACHE_FROZEN_FEATURES False (the image tower on every step), and on.  The cost of augmentation is the image tower running on every step;
          the kernel's own share is the difference between the last two.

`--only kernel|vpt|coop` runs one case; `--out FILE` also writes the JSON there."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import augment, clip, steps  # noqa: E402

STREAM_TBS = 6.3


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


def kernel_case(pool_images=3600):
    g = torch.Generator(device="cuda").manual_seed(1)
    pool = torch.randn(pool_images, 3, 224, 224, device="cuda", generator=g)
    sampler = augment.ViewSampler(seed=0)
    res = [{"case": "pool", "images": pool_images, "bytes": pool.numel() * 4}]
    for V in (16, 816, 4096):
        sets = max(2, min(64, pool_images // V)) if V <= pool_images else 2     # rotating (rows, boxes, out): other sources and another destination every call
        rs = np.random.RandomState(V)
        rows = [torch.from_numpy(rs.randint(0, pool_images, V)) for _ in range(sets)]
        boxes = [sampler.boxes([f"probe/{s}/{i}" for i in range(V)], 0, 224, 224) for s in range(sets)]
        outs = [torch.empty(V, 3, 224, 224, device="cuda") for _ in range(min(sets, 3))]
        # descriptors uploaded once: the timed calls are the launch alone
        d = []
        for s in range(sets):
            rec = np.zeros(V, dtype=augment._VIEW)
            rec["row"], rec["top"], rec["left"], rec["height"], rec["width"], rec["flip"] = (rows[s].numpy(), *boxes[s].T)
            d.append(torch.from_numpy(rec.view(np.uint8)).cuda())
        fn = lambda i: augment._launch(pool, d[i % sets], V, 224, outs[i % len(outs)])      # noqa: E731
        for i in range(2 * sets):
            fn(i)
        iters = 64 if V == 16 else 2 * sets
        t = timed(fn, iters)
        written = V * 3 * 224 * 224 * 4
        tb = [written / (x * 1e-6) / 1e12 for x in (t[1], t[0])]
        r = {"case": f"kernel {V} views of 224x224", "us_min": round(t[0], 1), "us_max": round(t[1], 1), "written_bytes": written,
             "written_TBps_min": round(tb[0], 3), "written_TBps_max": round(tb[1], 3), "share_of_6.3_TBps": round(tb[1] / STREAM_TBS, 3)}
        names = [f"probe/0/{i}" for i in range(V)]
        src = pool[:V] if V <= pool_images else pool[rows[0].cuda()]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            sampler.batch(src, names, 1)
        torch.cuda.synchronize()
        r["with_sampler_wall_us"] = round((time.perf_counter() - t0) / 3 * 1e6, 1)
        res.append(r)
        del outs, d
    return res


def vpt_case(batch=16, prefix=16, iters=50):
    from grip_amd.models import CustomImageEncoder, ImagePrefixModel
    m, _ = clip.load("ViT-B/16", device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randn(batch, 3, 224, 224, device="cuda", generator=g) for _ in range(4)]
    y = torch.randint(0, 10, (batch,), device="cuda", generator=g, dtype=torch.int32)
    w = torch.full((batch,), 1.0 / batch, device="cuda")
    with torch.no_grad():
        txt = m.encode_text(clip.tokenize([f"a photo of a thing number {i}" for i in range(10)]).cuda())
    im = ImagePrefixModel(0.02 * torch.randn(prefix, 768, device="cuda", generator=g), CustomImageEncoder(m.visual), device="cuda")
    step = steps.GraphedVptStep(im, txt, 100.0, torch.optim.SGD([im.prefix], lr=1e-3))
    sampler = augment.ViewSampler(seed=0)
    names = [f"vpt/{i}" for i in range(batch)]
    plain = lambda i: step(xs[i % 4], y, w)                                       # noqa: E731
    aug = lambda i: step(sampler.batch(xs[i % 4], names, i), y, w)                # noqa: E731
    out = []
    for name, fn in (("graphed VPT step, AUGMENT off", plain), ("graphed VPT step, AUGMENT on", aug)):
        for i in range(5):
            fn(i)
        t = timed(fn, iters)
        out.append({"case": name, "batch": batch, "us_min": round(t[0], 1), "us_max": round(t[1], 1)})
    return out


def coop_case(n_classes=102, per_class=18, batch=16):
    from grip_amd import methods
    from grip_amd.data import TensorPoolDataset
    from grip_amd.methods.main import DEFAULTS, Config, synthetic_pool
    classes, files, images, names = synthetic_pool(n_classes, per_class, 224, 3)
    images = images.cuda()
    l2i = {c: i for i, c in enumerate(classes)}
    out = []
    for name, kw in (("CoOp epoch, AUGMENT off (cached frozen features)", {}),
                     ("CoOp epoch, AUGMENT off, CACHE_FROZEN_FEATURES False", dict(CACHE_FROZEN_FEATURES=False)),
                     ("CoOp epoch, AUGMENT on", dict(AUGMENT="rrc_flip"))):
        c = dict(DEFAULTS)
        c.update(OPTIM_SEED=1, VIS_ENCODER="ViT-B/16", DATASET_NAME="Synthetic", SPLIT_SEED=500, DATASET_DIR="", EPOCHS=3, WARMUP_EPOCHS=1, LR=0.002,
                 PREFIX_SIZE=16, BATCH_SIZE=batch, LEARNING_PARADIGM="ssl", MODEL="textual_prompt")
        c.update(kw)
        m = methods.TextualPrompt(Config(**c), l2i, classes, classes, classes, "cuda")
        m.define_model(classes)
        loader = m._loader(TensorPoolDataset(files, images, labels=names, label_map=l2i), True)
        times = []
        for e in range(3):                     # epoch 0 fills the cache / captures the graph: warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m._train_epoch(loader, epoch=e)
            torch.cuda.synchronize()
            times.append(round(time.perf_counter() - t0, 4))
        out.append({"case": name, "images": len(files), "batch": batch, "epoch_s": times, "steady_epoch_s": min(times[1:])})
        del m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernel", "vpt", "coop"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_probe: needs the GPU (nothing is measured without one)")
    res = []
    for k, fn in {"kernel": kernel_case, "vpt": vpt_case, "coop": coop_case}.items():
        if a.only in (None, k):
            res += fn()
            torch.cuda.empty_cache()
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
