"""Developer probe: what pseudolabels.PoolFeatureCache saves a textual GRIP run per pseudolabel pass, at BASELINE.json configs[1] shapes (one process:
N = 50 000 images, C = 102 classes, k = 16, ViT-B/16, synthetic fp16-grid weights, identical mode, the timed pool of bench.py).

Pass 1 is the frozen-CLIP pass of GRIP's first iteration (zero-shot text features, k); pass 2 is what the next iteration runs over the same pool: text
features of a CoOp prompt through the exact twin's text tower and a larger k.  Both are timed with a fresh cache (pass 1 cold, pass 2 served by it) and
without one, alternating within one process, after a warm-up of both passes; every figure is a host clock around work that ends in a device
synchronise, reported as the median of --repeats with its minimum and maximum.  Rows encoded per tower and pass come from LAST_REFINE_STATS.  The screen
stream is pinned ($GRIP_SCREEN_STREAM=hilo unless set) so that the uncached passes do not switch streams from repeat to repeat.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GRIP_SCREEN_STREAM", "hilo")
import bench  # noqa: E402
from grip_amd import clip, engine, pseudolabels as pl, rng  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=50000)
    ap.add_argument("--classes", type=int, default=102)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--k2", type=int, default=32, help="pseudo-shots per class of pass 2 (GRIP grows them every iteration)")
    ap.add_argument("--chunk", type=int, default=880)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="ViT-B/16")
    ap.add_argument("--no-cache", action="store_true", help="time only the uncached passes")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    m, _ = clip.load(a.model, device=dev)
    twin = m.exact_twin()
    d = m.dims
    n, C = a.pool, a.classes
    pool = bench.synth_pool(n, d.image_resolution, dev, 1234)
    paths = [f"pool/{i:08d}.jpg" for i in range(n)]
    labels = list(range(C))
    mid = pl.mid_tower(m, n)
    towers = {"screen": m.visual.tower, "exact": twin.visual.tower, **({"mid": mid} if mid is not None else {})}
    P = 16
    prefix = torch.from_numpy(rng.normal(1, rng.stream_id("bench.prefix"), (1, P, d.transformer_width), 0.0, 0.02)).to(dev)
    with torch.no_grad():
        txt = [twin.encode_text(bench.synth_tokens(C, 0).to(dev)),
               engine.text_prefix_forward(twin.text_tower, bench.synth_tokens(C, P).to(dev), prefix)]
    ks = (a.k, a.k2)

    def one(which, cache):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lists = pl.identical_lists(towers["screen"], towers["exact"], pool, txt[which], 100.0, paths, labels, ks[which], chunk=a.chunk, exact_chunk=a.chunk,
                                   mid_chunk=a.chunk, visual_mid=mid, cache=cache)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = pl.LAST_REFINE_STATS
        rows = {"screen": 0 if st["screen_cached"] else n, "mid": st["rows_mid_this_rank"], "exact": st["rows_exact_this_rank"],
                "cached_mid": st["rows_cached_mid"], "cached_exact": st["rows_cached_exact"]}
        return dt, rows, (list(lists[0]), list(lists[1]))

    for which in (0, 1):        # warm-up: every kernel and workspace of both passes
        one(which, None)
    modes = ["uncached"] if a.no_cache else ["cached", "uncached"]
    times = {mo: ([], []) for mo in modes}
    rows, lists, held = {}, {}, None
    for _ in range(a.repeats):
        for mo in modes:        # alternating, in one process
            cache = pl.PoolFeatureCache() if mo == "cached" else None
            for which in (0, 1):
                dt, rows[f"{mo}_pass{which + 1}"], lists[(mo, which)] = one(which, cache)
                times[mo][which].append(dt)
            if cache is not None:
                held = cache.stats()
                cache.clear()

    def summary(ts):
        med = statistics.median(ts)
        return {"seconds_median": round(med, 4), "seconds_min": round(min(ts), 4), "seconds_max": round(max(ts), 4), "images_per_sec_median": round(n / med, 1)}
    out = {"probe": "pool_cache", "model": a.model, "pool_images": n, "classes": C, "k": list(ks), "chunk": a.chunk, "repeats": a.repeats, "tiers": len(towers),
           "screen_stream": os.environ["GRIP_SCREEN_STREAM"], "rows_encoded": rows}
    for mo in modes:
        out[mo] = {"pass1": summary(times[mo][0]), "pass2": summary(times[mo][1])}
    if not a.no_cache:
        out["lists_identical_cached_vs_uncached"] = all(lists[("cached", w)] == lists[("uncached", w)] for w in (0, 1))
        out["pass2_speedup_median"] = round(statistics.median(times["uncached"][1]) / statistics.median(times["cached"][1]), 2)
        out["cache_bytes_after_pass2"] = held["bytes"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
