"""Developer probe: times the candidate-set kernels (csrc/candidate.hip) in ONE process, after warm-up, with device events; the contenders' windows
ALTERNATE inside the run, and every figure is the median and min .. max over `--repeats` (>= 5, default 7) windows.

  select   grip_candidate_select on a pool-sized matrix, 50 000 x 102, tau 0.99, intersection, claim = 2 x 16 and 2 x 490 (CPL_SLOTS x the first and
           the last K of a GRIP run on that pool) through the C ABI on preallocated outputs, against a torch composition of the same selection: topk
           of every column for the thresholds, a descending sort of every row, cumsum, the prefix test, a scatter back and the packing into mask words
  loss     grip_candidate_ce at 64 x 102 (48 candidate rows of a 50 000 x 102 pool's sets) through the C ABI on preallocated outputs, against
           grip_weighted_ce on the same logits (what the step launches with the switch off) and against grip_candidate_ce with cand = NULL; then
           engine.candidate_ce (allocations included) against a torch autograd form of -log sum_S softmax
  step     the graphed CoOp step on pre-encoded features at the shapes of BASELINE.json configs[1] (ViT-B/16 text tower, 102 classes, 16 context tokens,
           batch 16) with the switch off (WeightedCEFn) and on (CandidateCEFn on the sets of a 50 000 x 102 pool)

`--out FILE` also writes the JSON there."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import grip_amd  # noqa: E402,F401
from grip_amd import clip, engine, native, rng, steps  # noqa: E402
from grip_amd.models import CustomTextEncoder, TextPrefixModel  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from label_prop_probe import alternate, summary  # noqa: E402


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pool_probs(n=50000, c=102, seed=0):
    """Probabilities of a pool: softmax rows with one or two dominant classes."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = 2 * torch.randn(n, c, device="cuda", generator=g)
    z[torch.arange(n, device="cuda"), torch.randint(0, c, (n,), device="cuda", generator=g)] += 6.0
    return torch.softmax(z, dim=1)


def torch_select(p, claim, tau):
    """(mask, count, label, threshold) of the intersection rule as a torch composition (torch's cumsum: not the sequential sum bit for bit)."""
    n, c = p.shape
    thr = p.topk(claim, dim=0).values[-1]
    ranked, order = p.sort(dim=1, descending=True, stable=True)
    s = ranked.cumsum(1)
    keep = torch.ones_like(ranked, dtype=torch.bool)
    keep[:, 1:] = s[:, :-1] < tau
    intra = torch.zeros_like(keep).scatter_(1, order, keep)
    member = intra & (p >= thr[None])
    words = (c + 31) // 32
    padded = torch.zeros(n, 32 * words, dtype=torch.int64, device=p.device)
    padded[:, :c] = member
    word = (padded.view(n, words, 32) << torch.arange(32, device=p.device)).sum(-1)
    mask = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)
    in_rank = member.gather(1, order)
    label = torch.where(in_rank.any(1), order.gather(1, in_rank.int().argmax(1, keepdim=True))[:, 0], torch.full((n,), -1, device=p.device)).to(torch.int32)
    return mask, member.sum(1).to(torch.int32), label, thr


def select_case(repeats, n=50000, c=102, tau=0.99):
    lib = native.lib()
    p = pool_probs(n, c)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_candidate_select_workspace(n, c, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    mask = torch.empty(n, (c + 31) // 32, dtype=torch.int32, device="cuda")
    count, label = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    thr = torch.empty(c, device="cuda")
    res = []
    for claim in (2 * 16, 2 * 490):
        fns = {"grip_candidate_select": lambda i, k=claim: lib.grip_candidate_select(_p(p), n, c, k, tau, 0, _p(thr), _p(mask), _p(count), _p(label), _p(ws),
                                                                                     ws.numel(), _stream()),
               "torch composition": lambda i, k=claim: torch_select(p, k, tau)}
        case = f"select n={n} c={c} claim={claim} tau={tau} intersection"
        out = [summary(case, who, t) for who, t in alternate(fns, 20, repeats).items()]
        out.append({"case": case, "who": "verdict", "native_over_torch": round(out[0]["us_median"] / out[1]["us_median"], 3)})
        fns["grip_candidate_select"](0)
        tm, tc, tl, tt = torch_select(p, claim, tau)
        out.append({"case": case, "who": "agreement", "thresholds_equal": bool(torch.equal(tt, thr)), "rows_with_another_mask": int((tm != mask).any(1).sum()),
                    "mean_set_size": round(float(count[count > 0].float().mean()), 3), "rows_with_a_set": int((count > 0).sum())})
        res += out
    return res


def ce_operands(n=64, c=102, pool=50000, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = 4 * torch.randn(n, c, device="cuda", generator=g)
    labels = torch.randint(0, c, (n,), device="cuda", generator=g, dtype=torch.int32)
    w = torch.full((n,), 1.0 / n, device="cuda")
    mask, _, _, _ = engine.candidate_select(pool_probs(pool, c), 2 * 490, 0.99, "union")       # (union: no empty sets)
    rows = torch.randint(0, pool, (n,), device="cuda", generator=g, dtype=torch.int32)
    rows[::4] = -1                                    # a quarter of the batch: labelled rows
    cmap = torch.randperm(c, device="cuda", generator=g).to(torch.int32)
    return logits, labels, w, mask, rows, cmap


def torch_candidate_ce(logits, labels, w, mask, rows, cmap):
    x = logits.detach().clone().requires_grad_(True)
    n, c = x.shape
    j = torch.arange(c, device=x.device)
    cand = rows >= 0
    bits = ((mask[rows.clamp_min(0).long()].long()[:, j // 32] >> (j % 32)) & 1).bool()
    member = torch.zeros(n, c, dtype=torch.bool, device=x.device)
    member[:, cmap.long()] = bits
    member = torch.where(cand[:, None], member, j[None] == labels[:, None])
    logp = torch.log_softmax(x, dim=1)
    loss = -(w * torch.logsumexp(logp.masked_fill(~member, -float("inf")), dim=1)).sum()
    loss.backward()
    return loss.detach(), x.grad


def loss_case(repeats, n=64, c=102):
    lib = native.lib()
    logits, labels, w, mask, rows, cmap = ce_operands(n, c)
    loss, grad = torch.empty(1, device="cuda"), torch.empty_like(logits)
    fns = {
        "grip_weighted_ce": lambda i: lib.grip_weighted_ce(_p(logits), _p(labels), _p(w), n, c, _p(loss), _p(grad), _stream()),
        "grip_candidate_ce, cand = NULL": lambda i: lib.grip_candidate_ce(_p(logits), _p(labels), _p(w), n, c, None, 0, 0, None, None, _p(loss), _p(grad), _stream()),
        "grip_candidate_ce, 48 candidate rows": lambda i: lib.grip_candidate_ce(_p(logits), _p(labels), _p(w), n, c, _p(mask), mask.shape[0], c, _p(rows), _p(cmap),
                                                                               _p(loss), _p(grad), _stream()),
    }
    case = f"kernel n={n} c={c} (C ABI, preallocated outputs)"
    res = [summary(case, who, t) for who, t in alternate(fns, 200, repeats).items()]
    res.append({"case": case, "who": "verdict", "candidate_over_weighted_ce": round(res[2]["us_median"] / res[0]["us_median"], 3),
                "null_over_weighted_ce": round(res[1]["us_median"] / res[0]["us_median"], 3)})
    case = f"call n={n} c={c} (loss + gradient, allocations included)"
    fns = {"engine.candidate_ce": lambda i: engine.candidate_ce(logits, labels, w, mask, rows, cmap),
           "torch autograd": lambda i: torch_candidate_ce(logits, labels, w, mask, rows, cmap)}
    out = [summary(case, who, t) for who, t in alternate(fns, 100, repeats).items()]
    out.append({"case": case, "who": "verdict", "native_over_torch": round(out[0]["us_median"] / out[1]["us_median"], 3)})
    ln, gn = engine.candidate_ce(logits, labels, w, mask, rows, cmap)
    lt, gt = torch_candidate_ce(logits, labels, w, mask, rows, cmap)
    out.append({"case": case, "who": "agreement", "loss_difference": float((ln - lt).abs()), "max_abs_difference_grad": float((gn - gt).abs().max())})
    return res + out


def step_case(repeats, C=102, P=16, B=16, pool=50000):
    dev = torch.device("cuda", 0)
    m, _ = clip.load("ViT-B/16", device=dev)
    classes = [f"class_{i}" for i in range(C)]
    enc = CustomTextEncoder(m, dev, torch.float32)
    enc._tok_cache[(P, tuple(classes))] = bench.synth_tokens(C, P).to(dev)
    _, y, w, mask, rows, cmap = ce_operands(B, C, pool)
    f = torch.randn(B, m.dims.embed_dim, device=dev)
    fns = {}
    for name, soft in (("switch off", None), ("switch on", steps.CandidateTargets(mask, cmap))):
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
    ap.add_argument("--only", choices=("select", "loss", "step"), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("candidate_probe: at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("candidate_probe: needs the GPU (nothing is measured without one)")
    res = []
    for k, fn in {"select": select_case, "loss": loss_case, "step": step_case}.items():
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
