"""Developer probe for test-time prompt tuning (tpt.TestTimeTuner, csrc/view_entropy.hip): ONE process, after warm-up, device events; the contenders'
windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5, default 7) windows.

  kernel     engine.view_entropy (loss + gradient in one call) at 1 x 64 x 102 (an episode: keep 6) and 55 x 16 x 102 (keep 1) against the torch
             composition: log_softmax, topk on the entropies, logsumexp, autograd.
  episode    TestTimeTuner.tune at the shapes of BASELINE.json configs[1] (C = 102, P = 16, V = 64, ViT-B/16 text tower): device time per episode
             with the episodes enqueued back to back, and wall clock with a host synchronisation after each (the episode runs eagerly; a graphed
             episode is not built).
  predict    `predict` of a textual strategy over a `--items` (512) item synthetic test set at the ViT-B/16 geometry, switch off and on (wall clock: the
             loader, V encodes per item and one episode per item are all in it).

The figures are call times (launches and the call's allocations included).  `--out FILE` also writes the JSON."""
import argparse
import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import grip_amd  # noqa: E402,F401
from grip_amd import engine, tpt  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, summary  # noqa: E402


def torch_view_entropy(logits, v, keep):
    """(loss, grad) of the model of include/grip_amd.h in torch ops, the selection a constant of the gradient."""
    x = logits.detach().view(-1, v, logits.shape[1]).requires_grad_(True)
    lp = torch.log_softmax(x, dim=2)
    with torch.no_grad():
        idx = (-(lp.exp() * lp).sum(2)).topk(keep, dim=1, largest=False).indices
    avg = torch.logsumexp(torch.gather(lp, 1, idx[:, :, None].expand(-1, -1, x.shape[2])), dim=1) - math.log(keep)
    loss = -(avg.exp() * avg).sum(1).mean()
    loss.backward()
    return loss.detach(), x.grad.view_as(logits)


def kernel_case(repeats):
    res = []
    for n, v, c, keep in ((1, 64, 102, 6), (55, 16, 102, 1)):
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (3 * torch.randn(n * v, c, device="cuda", generator=g)).contiguous()
        case = f"view_entropy n={n} v={v} c={c} keep={keep} (loss + gradient)"
        ts = alternate({"native": lambda i: engine.view_entropy(x, v, keep), "torch": lambda i: torch_view_entropy(x, v, keep)}, 200, repeats, warm=3)
        for who, t in ts.items():
            res.append(summary(case, who, t))
        nat, tor = res[-2]["us_median"], res[-1]["us_median"]
        (ln, gn), (lt, gt) = engine.view_entropy(x, v, keep), torch_view_entropy(x, v, keep)
        res.append({"case": case, "who": "verdict", "native_over_torch": round(nat / tor, 3), "launches_native": 1 if n == 1 else 2,
                    "abs_difference_loss": float((ln - lt).abs()), "max_abs_difference_grad": float((gn - gt).abs().max())})
    return res


def episode_case(repeats, C=102, P=16, V=64, model="ViT-B/16"):
    import bench
    from grip_amd import clip, rng
    from grip_amd.models import CustomTextEncoder, TextPrefixModel
    dev = torch.device("cuda", 0)
    m, _ = clip.load(model, device=dev)
    classes = [f"class_{i}" for i in range(C)]
    enc = CustomTextEncoder(m, dev, torch.float32)
    enc._tok_cache[(P, tuple(classes))] = bench.synth_tokens(C, P).to(dev)      # no tokenizer needed
    prefix = torch.from_numpy(rng.normal(1, rng.stream_id("bench.prefix"), (1, P, m.dims.transformer_width), 0.0, 0.02)).to(dev)
    tm = TextPrefixModel(prefix, enc, classes, device=dev)
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(8, V, m.dims.embed_dim, device="cuda", generator=g)
    tuner = tpt.TestTimeTuner(tm, m, views=V)
    case = f"episode C={C} P={P} V={V} keep={tuner.keep} steps=1 {model} text tower (tune: step + AdamW + inference forward + restore)"
    ts = alternate({"enqueued back to back (device time)": lambda i: tuner.tune(feats[i % 8])}, 20, repeats, warm=3)
    res = [summary(case, who, t) for who, t in ts.items()]
    base = []
    for i in range(8):
        base.append(tuner.tune(feats[i]).clone())
        torch.cuda.synchronize()
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for i in range(20):
            tuner.tune(feats[i % 8])
            torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / 20 * 1e6)
    res.append(summary(case, "synchronised after each (wall clock)", wall))
    queued = [tuner.tune(feats[i % 8]).clone() for i in range(40)]
    torch.cuda.synchronize()
    res.append({"case": case, "who": "verdict", "rows_enqueued_equal_rows_synchronised": all(torch.equal(r, base[i % 8]) for i, r in enumerate(queued))})
    return res


def predict_case(repeats, items, C=102, model="ViT-B/16"):
    import bench
    from grip_amd import methods
    from grip_amd.data import TensorPoolDataset
    from grip_amd.methods.main import DEFAULTS, Config
    dev = torch.device("cuda", 0)
    classes = [f"class_{i:03d}" for i in range(C)]
    l2i = {c: i for i, c in enumerate(classes)}
    res_px = 224
    images = bench.synth_pool(items, res_px, dev, 4321)
    files = [f"test/{i:06d}.jpg" for i in range(items)]
    data = TensorPoolDataset(files, images, labels=[classes[i % C] for i in range(items)], label_map=l2i)
    out = []
    case = f"predict over {items} items, C={C}, BATCH_SIZE 16, {model} (wall clock)"
    for name, kw in (("switch off", {}), ("TPT on (V = 64)", {"TPT": True})):
        conf = Config(**{**DEFAULTS, "VIS_ENCODER": model, "LEARNING_PARADIGM": "ssl", "DATASET_NAME": "Synthetic", "OPTIM_SEED": 1, **kw})
        s = methods.TextualPrompt(conf, l2i, classes, classes, classes, dev)
        s.define_model(classes)
        ts = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.predict(data, classes)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        out.append(summary(case, name, ts[1:]))      # (the first call warms up: boxes, workspaces)
        del s
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernel", "episode", "predict"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--items", type=int, default=512, help="items of the predict case")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("tpt_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("tpt_probe: needs the GPU (nothing is measured without one)")
    res = []
    if a.only in (None, "kernel"):
        res += kernel_case(a.repeats)
    if a.only in (None, "episode"):
        res += episode_case(a.repeats)
    if a.only in (None, "predict"):
        res += predict_case(a.repeats, a.items)
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
