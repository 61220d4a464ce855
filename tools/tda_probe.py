"""Developer probe for the test-time streaming cache (tda.StreamCache, csrc/stream_cache.hip): ONE process, after warm-up, device events; the
contenders' windows ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5, default 7) windows.

  stream     at n = 10 000, c = 102, e = 512 (a class-structured stream, the default settings): engine.stream_cache_plan, engine.stream_cache_head on
             its plan and engine.stream_cache (both) against the algorithm as a torch user writes it -- the literal per-item loop below: softmax and
             entropy per item, a host read of the entropy and the prediction, Python lists per class, the affinities of the item to the stacked queue
             contents.  `--shapes` adds smaller streams (where a few launches of fixed cost meet a short loop).
  predict    `predict` of a textual strategy over a `--items` (512) item synthetic test set at the ViT-B/16 geometry, switch off and on (wall clock).

The figures are call times (launches and the call's allocations included).  `--out FILE` also writes the JSON."""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import grip_amd  # noqa: E402,F401
from grip_amd import engine  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, summary  # noqa: E402


def stream(n, c, e, seed=1):
    """(base [n, c], feats [n, e]): features around unit class centres, logits from a noisy copy of the centres at CLIP's scale."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = F.normalize(torch.randn(c, e, device="cuda", generator=g), dim=1)
    y = torch.randint(0, c, (n,), device="cuda", generator=g)
    feats = centres[y] + 1.5 / e ** 0.5 * torch.randn(n, e, device="cuda", generator=g)
    head = F.normalize(centres + 0.6 / e ** 0.5 * torch.randn(c, e, device="cuda", generator=g), dim=1)
    return (15.0 * F.normalize(feats, dim=1) @ head.T).contiguous(), feats.contiguous()      # (15: about a fifth of the items fall in the negative window)


def torch_loop(base, feats, pos_cap, neg_cap, pos_alpha, pos_beta, neg_alpha, neg_beta, neg_entropy, neg_mask, entropy=None):
    """The model of include/grip_amd.h one item at a time in torch ops: what the published form looks like.  entropy (a host list, not timed): the queue
    comparisons run on THESE entropies instead of torch's own -- two f32 evaluations of H may order a near-tie differently, and one swapped resident moves a
    logit by up to pos_alpha; with the kernel's own entropies only arithmetic is left to differ."""
    n, c = base.shape
    fh = F.normalize(feats, dim=1)
    pos, neg, masks = {}, {}, torch.zeros_like(base)      # (the mask rows of the negative queue's items)
    out = base.clone()
    logc = math.log(c) if c > 1 else 1.0

    def update(queues, y, h, i, cap):
        q = queues.setdefault(y, [])
        if len(q) < cap:
            q.append((h, i))
        else:
            q.sort()
            if h < q[-1][0]:
                q[-1] = (h, i)

    def term(queues, beta, values_of):
        idx = sorted(j for q in queues.values() for _, j in q)
        if not idx:
            return None
        ix = torch.tensor(idx, device=base.device)
        a = torch.exp(-beta * (1.0 - fh[ix] @ fh[i]))
        return a @ values_of(ix)
    for i in range(n):
        lp = torch.log_softmax(base[i], 0)
        p = lp.exp()
        h, y = float(-(p * lp).sum()), int(base[i].argmax())      # (the host reads them: the lists live in Python)
        if entropy is not None:
            h = entropy[i]
        if math.isfinite(h):
            update(pos, y, h, i, pos_cap)
            if neg_cap and neg_entropy[0] < (h / logc if c > 1 else 0.0) < neg_entropy[1]:
                update(neg, y, h, i, neg_cap)
                masks[i] = ((p > neg_mask[0]) & (p < neg_mask[1])).float()
        t = term(pos, pos_beta, lambda ix: F.one_hot(base[ix].argmax(1), c).float())
        if t is not None:
            out[i] += pos_alpha * t
        t = term(neg, neg_beta, lambda ix: masks[ix])
        if t is not None:
            out[i] -= neg_alpha * t
    return out


def stream_case(repeats, shapes):
    res = []
    st = dict(engine.STREAM_CACHE_DEFAULTS)
    plan_kw = {k: st[k] for k in ("pos_cap", "neg_cap", "neg_entropy", "neg_mask")}
    head_kw = {k: st[k] for k in ("pos_alpha", "pos_beta", "neg_alpha", "neg_beta")}
    for n, c, e in shapes:
        base, feats = stream(n, c, e)
        plan = engine.stream_cache_plan(base, **plan_kw)
        counts = plan["counts"].tolist()
        case = f"stream n={n} c={c} e={e} (default settings; ever-admitted keys {counts[0]} positive, {counts[1]} negative)"
        ts = alternate({"plan": lambda i: engine.stream_cache_plan(base, **plan_kw), "head": lambda i: engine.stream_cache_head(base, feats, plan, **head_kw),
                        "native (plan + head)": lambda i: engine.stream_cache(base, feats, **st)}, 20, repeats, warm=3)
        res += [summary(case, who, t) for who, t in ts.items()]
        nat = res[-1]["us_median"]
        ts = alternate({"torch per-item loop": lambda i: torch_loop(base, feats, **st)}, 1, repeats, warm=1)
        res.append(summary(case, "torch per-item loop", ts["torch per-item loop"]))
        (got, plan), want = engine.stream_cache(base, feats, **st), torch_loop(base, feats, **st)
        same = torch_loop(base, feats, **st, entropy=plan["entropy"].tolist())
        res.append({"case": case, "who": "verdict", "native_over_torch": round(nat / res[-1]["us_median"], 5),
                    "max_abs_difference": float((got - want).abs().max()), "rows_differing_by_more_than_1e-3": int(((got - want).abs() > 1e-3).any(1).sum()),
                    "rows_whose_argmax_differs": int((got.argmax(1) != want.argmax(1)).sum()),
                    "max_abs_difference_on_the_kernels_entropies": float((got - same).abs().max())})
    return res


def predict_case(repeats, items, C=102, model="ViT-B/16"):
    import bench
    from grip_amd import methods
    from grip_amd.data import TensorPoolDataset
    from grip_amd.methods.main import DEFAULTS, Config
    dev = torch.device("cuda", 0)
    classes = [f"class_{i:03d}" for i in range(C)]
    l2i = {c: i for i, c in enumerate(classes)}
    images = bench.synth_pool(items, 224, dev, 4321)
    files = [f"test/{i:06d}.jpg" for i in range(items)]
    data = TensorPoolDataset(files, images, labels=[classes[i % C] for i in range(items)], label_map=l2i)
    strategies = {}
    for name, kw in (("switch off", {}), ("TDA on", {"TDA": True})):
        conf = Config(**{**DEFAULTS, "VIS_ENCODER": model, "LEARNING_PARADIGM": "ssl", "DATASET_NAME": "Synthetic", "OPTIM_SEED": 1, **kw})
        strategies[name] = methods.TextualPrompt(conf, l2i, classes, classes, classes, dev)
        strategies[name].define_model(classes)
    ts = {name: [] for name in strategies}
    for i in range(repeats + 1):      # alternating windows; the first of each warms up (workspaces)
        for name, s in strategies.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.predict(data, classes)
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e6)
    case = f"predict over {items} items, C={C}, BATCH_SIZE 16, {model} (wall clock)"
    return [summary(case, name, t[1:]) for name, t in ts.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("stream", "predict"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--items", type=int, default=512, help="items of the predict case")
    ap.add_argument("--shapes", default="10000x102x512", help="comma-separated n x c x e of the stream case")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("tda_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("tda_probe: needs the GPU (nothing is measured without one)")
    res = []
    if a.only in (None, "stream"):
        res += stream_case(a.repeats, [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")])
    if a.only in (None, "predict"):
        res += predict_case(a.repeats, a.items)
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
