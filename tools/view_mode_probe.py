"""Developer probe: times the multi-view mode kernel (csrc/view_mode.hip) against the same recursion written in torch ops (bmm, sort, softmax) in ONE
process, after warm-up, with device events; native and torch windows ALTERNATE inside the run, and every figure is the median and min .. max over
`--repeats` (>= 5, default 7) windows.

  kernel     engine.view_mode at the defaults on n images x 16 views x 512, c = 102: n = 55 (a chunk of 880 views) and the pool-sized n = 50 000, against
             torch_view_mode; the achieved bytes per second against the read-once floor n V (e + c) 4 bytes.
  pass       the pseudolabel pass (pool encode + head + scan, f16 mode, wall clock) over `--pool` images of the ViT-B/16 geometry (BASELINE.json configs[1]:
             50 000; the encode is V times the rows, so a smaller --pool is the way to a quick look): switch off, V = 4 and V = 16.

Bytes are computed here from the shapes; the figures are call times (launches and the call's allocations included).  `--out FILE` also writes the JSON."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import grip_amd  # noqa: E402,F401
from grip_amd import engine, pseudolabels as pl  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, summary  # noqa: E402

TINY = 2.0 ** -126
STREAM_TBS = 6.3        # the streaming rate the floor is stated against


def torch_view_mode(f, s, rho=0.3, lam=4.0, lam_y=0.2, h2_floor=2.0 ** -20, outer=5, inner=3):
    n, v, e = f.shape
    u = torch.nn.functional.normalize(f, dim=2)
    d2 = (2 - 2 * torch.bmm(u, u.transpose(1, 2))).clamp_min(0.0)
    d2 = d2.masked_fill(torch.eye(v, dtype=torch.bool, device=f.device), float("inf"))
    r = max(1, int(rho * (v - 1)))
    h2 = (d2.sort(dim=2).values[..., :r].sum(2) / r).clamp_min(h2_floor)
    A = torch.bmm(s, s.transpose(1, 2))
    m, y = u[:, 0], torch.full((n, v), 1.0 / v, device=f.device)
    for _ in range(outer):
        k = torch.exp(-((u - m[:, None, :]) ** 2).sum(2) / (2 * h2))
        for _ in range(inner):
            y = torch.softmax((k + lam * torch.bmm(A, y[:, :, None])[:, :, 0]) / lam_y, dim=1)
        w = y * k
        m = torch.bmm(w[:, None, :], u)[:, 0] / w.sum(1, keepdim=True).clamp_min(TINY)
    return m, y


def views_of(n, v, e, c, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centre = torch.nn.functional.normalize(torch.randn(n, 1, e, device="cuda", generator=g), dim=2)
    f = centre + 0.5 * torch.nn.functional.normalize(torch.randn(n, v, e, device="cuda", generator=g), dim=2)
    s = torch.softmax(3 * torch.randn(n, v, c, device="cuda", generator=g), dim=2)
    return f.contiguous(), s.contiguous()


def kernel_case(repeats, v=16, e=512, c=102):
    res = []
    with torch.no_grad():
        for n, iters in ((880 // v, 50), (50000, 3)):
            f, s = views_of(n, v, e, c)
            case = f"view_mode n={n} v={v} e={e} c={c} defaults"
            nbytes = n * v * (e + c) * 4.0
            res.append({"case": case, "who": "floor (an estimate from the shapes, not a result)", "bytes_read_once": nbytes,
                        "stream_floor_us": round(nbytes / (STREAM_TBS * 1e12) * 1e6, 2), "launches": 1})
            ts = alternate({"native": lambda i: engine.view_mode(f, s), "torch": lambda i: torch_view_mode(f, s)}, iters, repeats)
            for who, t in ts.items():
                res.append(summary(case, who, t))
            nat, tor = res[-2]["us_median"], res[-1]["us_median"]
            res.append({"case": case, "who": "verdict", "native_over_torch": round(nat / tor, 3), "native_read_once_GBps": round(nbytes / nat / 1e3, 1),
                        "share_of_stream_floor_rate": round(nbytes / (nat * 1e-6) / (STREAM_TBS * 1e12), 4)})
            mn, yn = engine.view_mode(f, s)
            mt, yt = torch_view_mode(f, s)
            res.append({"case": case, "who": "agreement", "max_abs_difference_mode": float((mn - mt).abs().max()), "max_abs_difference_y": float((yn - yt).abs().max())})
            del f, s
            torch.cuda.empty_cache()
    return res


def pass_case(repeats, n, c=102, shots=16, model="ViT-B/16", chunk=880):
    import bench
    from grip_amd import clip
    dev = torch.device("cuda", 0)
    m, _ = clip.load(model, device=dev)
    images = bench.synth_pool(n, m.dims.image_resolution, dev, 1234)
    paths = [f"pool/{i:08d}.jpg" for i in range(n)]
    labels = list(range(c))
    with torch.no_grad():
        txt = m.encode_text(bench.synth_tokens(c, 0).to(dev))
    tower = m.visual.tower

    def run(mv):
        ts = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            emb = pl.encode_pool(tower, images, chunk=chunk) if mv is None else mv.features(tower, images, paths, txt, 100.0, chunk=chunk)
            pl.pseudolabel_from_features(emb, txt, 100.0, paths, labels, shots)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts[1:]       # (the first pass warms up: path ranks, boxes, allocations)
    case = f"pseudolabel pass n={n} c={c} shots={shots} {model} (wall clock, encode + head + host scan)"
    return [summary(case, "switch off", run(None)), summary(case, "V = 4", run(pl.MultiView(views=4))), summary(case, "V = 16", run(pl.MultiView(views=16)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernel", "pass"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pool", type=int, default=50000, help="images of the pass case")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("view_mode_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("view_mode_probe: needs the GPU (nothing is measured without one)")
    res = []
    if a.only in (None, "kernel"):
        res += kernel_case(a.repeats)
    if a.only in (None, "pass"):
        res += pass_case(a.repeats, a.pool)
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
