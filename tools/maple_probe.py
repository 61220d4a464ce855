"""Cost of the coupled deep multimodal prompts (MaPLeModel, csrc/couple.hip), one process:
(a) the graphed multimodal step (steps.GraphedUptStep) at the shapes of configs[3] (ViT-B/16, B = 16, P = 4, C = 47) for shallow UPT, deep UPT
    (D = 11) and MaPLe (D = 8, D = 11): five repeats of 200 replays each, ms per step;
(b) the coupling's forward and backward alone at (P, D, dt, dv) = (4, 11, 512, 768) and (16, 11, 512, 768): microseconds per call and GB/s of
    its algorithmic bytes (forward: W + b + X + Y; backward: W + d_w + d_b + X + dY + dX), hot (one operand set) and cold (operand sets rotated
    past the 256 MB Infinity Cache), five repeats of 200 calls each.
Usage: python tools/maple_probe.py [--only step|couple] [--repeats 5] [--replays 200] [--sets 16] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grip_amd  # noqa: E402,F401
from grip_amd import clip, native, steps  # noqa: E402
from grip_amd.models import CustomImageEncoder, CustomTextEncoder, MaPLeModel, UPTModel  # noqa: E402


def repeats(fn, n_rep, n_call):
    """[per-call ms] of n_rep timed groups of n_call back-to-back calls (device events around each group)."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n_call):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / n_call)
    return out


def step_times(a, res):
    m, _ = clip.load("ViT-B/16", device="cuda")
    enc, vis = CustomTextEncoder(m, "cuda", torch.float32), CustomImageEncoder(m.visual)
    classes = [f"texture number {i}" for i in range(47)]
    g = torch.Generator(device="cuda").manual_seed(7)
    B, P = 16, 4
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(0, 47, (B,), device="cuda", generator=g, dtype=torch.int32)
    w = torch.full((B,), 1.0 / B, device="cuda")
    N = lambda *shape: 0.02 * torch.randn(*shape, device="cuda", generator=g)      # noqa: E731
    coop, vpt, vdeep, tdeep = N(1, P, 512), N(1, P, 768), N(11, P, 768), N(11, P, 512)

    def upt(deep):
        torch.manual_seed(0)
        return UPTModel(coop.clone(), vpt.clone(), None if deep is None else deep.clone(), vis, enc, classes, 128, device="cuda", dtype=torch.float32,
                        mix_deep=deep is not None)

    def maple(D):
        torch.manual_seed(0)
        return MaPLeModel(coop.clone(), tdeep[:D].clone(), vis, enc, classes, device="cuda")
    forms = (("upt_shallow", lambda: upt(None)), ("upt_deep11", lambda: upt(vdeep)), ("maple_d8", lambda: maple(8)), ("maple_d11", lambda: maple(11)))
    for name, make in forms:
        model = make()
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
        step = steps.GraphedUptStep(model, 100.0, opt)
        t = repeats(lambda: step(x, y, w), a.repeats, a.replays)
        res[f"step_{name}_ms"] = [round(min(t), 4), round(max(t), 4)]
        del step, model, opt


def couple_times(a, res):
    lib = native.lib()
    g = torch.Generator(device="cuda").manual_seed(3)
    for P, D, dt, dv in ((4, 11, 512, 768), (16, 11, 512, 768)):
        L = 1 + D
        N = lambda *shape: torch.randn(*shape, device="cuda", generator=g)      # noqa: E731
        ctx, deep, b = N(P, dt), N(D, P, dt), N(L, dv)
        dy0, dyd = N(P, dv), N(D, P, dv)
        y0, yd, d_ctx, d_deep, d_b = torch.empty(P, dv, device="cuda"), torch.empty(D, P, dv, device="cuda"), torch.empty_like(ctx), torch.empty_like(deep), \
            torch.empty_like(b)
        ws_w = [N(L, dv, dt) for _ in range(a.sets)]
        ws_g = [torch.empty(L, dv, dt, device="cuda") for _ in range(a.sets)]
        n = ctypes.c_size_t()
        native.check(lib.grip_prompt_couple_workspace(P, D, dt, dv, ctypes.byref(n)))
        scratch = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        w_bytes = L * dv * dt * 4
        small = 4 * (L * dv + L * P * dt + L * P * dv)
        nbytes = {"fwd": w_bytes + small, "bwd": 2 * w_bytes + small + 4 * L * P * dt}
        it = [0]

        def fwd(k):
            native.check(lib.grip_prompt_couple_forward(ctx.data_ptr(), deep.data_ptr(), P, D, dt, dv, ws_w[k].data_ptr(), b.data_ptr(), y0.data_ptr(),
                                                        yd.data_ptr(), s))

        def bwd(k):
            native.check(lib.grip_prompt_couple_backward(ctx.data_ptr(), deep.data_ptr(), P, D, dt, dv, ws_w[k].data_ptr(), dy0.data_ptr(), dyd.data_ptr(),
                                                         d_ctx.data_ptr(), d_deep.data_ptr(), ws_g[k].data_ptr(), d_b.data_ptr(), scratch.data_ptr(), n.value, s))
        for kind, fn in (("fwd", fwd), ("bwd", bwd)):
            for temp, sets in (("hot", 1), ("cold", a.sets)):
                def call(fn=fn, sets=sets):
                    fn(it[0])
                    it[0] = (it[0] + 1) % sets
                it[0] = 0
                t = repeats(call, a.repeats, a.replays)
                us = [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)]
                res[f"couple_{kind}_{temp}_P{P}_D{D}_us"] = us
                res[f"couple_{kind}_{temp}_P{P}_D{D}_GBps"] = [round(nbytes[kind] / (u * 1e-6) / 1e9, 1) for u in reversed(us)]
        res[f"couple_P{P}_D{D}_bytes"] = nbytes
        del ws_w, ws_g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=("", "step", "couple"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--sets", type=int, default=16)      # 16 x 18.9 MB of W (and as much d_w): past the Infinity Cache
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"repeats": a.repeats, "replays": a.replays, "sets": a.sets}
    if a.only != "couple":
        step_times(a, res)
    if a.only != "step":
        couple_times(a, res)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
