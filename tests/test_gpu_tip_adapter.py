"""The Tip-Adapter cache head above the kernel: engine.CacheHeadFn against float64 autograd, the Tip-Adapter-F step (eager trajectory against float64,
graphed against eager), and the TIP_ADAPTER switch of the textual strategies on the synthetic pool (tiny towers)."""
import os

import numpy as np
import pytest
import torch

import test_gpu_cache_head as K
from conftest import write_report

pytestmark = pytest.mark.gpu


def _restate(f, keys, y, v, alpha, beta, logits):
    """The head in plain torch, in the dtype of its inputs: y [m] class of each key (keys grouped or not)."""
    fh = f / f.norm(dim=1, keepdim=True)
    A = torch.exp(-beta * (1 - fh @ keys.T))
    M = torch.zeros(keys.shape[0], logits.shape[1], dtype=f.dtype, device=f.device)
    M[torch.arange(keys.shape[0], device=f.device), y] = 1
    return logits + alpha * ((A * v) @ M)


def _wce(logits, labels, w):
    return (w * (torch.logsumexp(logits, 1) - logits.gather(1, labels[:, None].long())[:, 0])).sum()


def test_cache_head_fn_against_float64_autograd():
    import grip_amd  # noqa: F401
    from grip_amd import native
    from grip_amd.engine import CacheHeadFn
    n, sizes, e, alpha, beta = 16, [8, 0, 12, 15, 5], 64, 3.0, 5.5      # (n, m, c, e) = (16, 40, 5, 64)
    f, k, v, logits, G, cs = K._inputs(n, sizes, e, True, seed=77)
    y = torch.repeat_interleave(torch.arange(5, device="cuda"), torch.tensor(sizes, device="cuda"))
    k64 = k.double().requires_grad_(True)
    l64 = logits.double().requires_grad_(True)
    ref = _restate(f.double(), k64, y, v.double(), alpha, beta, l64)
    (ref * G.double()).sum().backward()
    _, fb, dk, bb = K._reference(f, k, cs, v, alpha, beta, logits, G)
    assert torch.allclose(dk, k64.grad, rtol=1e-9, atol=1e-12 * float(dk.abs().max()))       # the two float64 statements agree
    kp, lp = k.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    out = CacheHeadFn.apply(f, kp, cs, v, alpha, beta, lp)
    (out * G).sum().backward()
    K._check("CacheHeadFn", "logits", out.detach(), ref.detach(), fb)
    K._check("CacheHeadFn", "keys.grad", kp.grad, k64.grad, bb)
    assert torch.equal(lp.grad, G) and torch.equal(logits, lp.detach())      # the logits gradient passes through; the input logits are not written
    with pytest.raises(native.GripError, match="img_emb requires grad"):
        CacheHeadFn.apply(f.clone().requires_grad_(True), kp, cs, v, alpha, beta, lp)


def _clustered(n, m, c, e, seed):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(c, e, generator=g)
    ky = torch.arange(m) % c
    keys = centers[ky] + 0.8 * torch.randn(m, e, generator=g)
    keys = keys / keys.norm(dim=1, keepdim=True)
    labels = torch.randint(0, c, (n,), generator=g)
    f = (centers[labels] + 0.8 * torch.randn(n, e, generator=g)) * (0.5 + 4 * torch.rand(n, 1, generator=g))
    logits = torch.randn(n, c, generator=g)
    return f, keys, ky, labels, logits


def test_key_trajectory_of_five_sgd_steps():
    """Five SGD steps of steps.tip_step on the keys against the float64 restatement of the same steps.  The allowance is measured here: the same
    restatement in f32 on the CPU deviates from float64 by D32; the native trajectory may deviate by 4 x D32 (another, equally valid f32 order)."""
    import grip_amd  # noqa: F401
    from grip_amd import steps
    from grip_amd.models import TipAdapterModel
    n, m, c, e, alpha, beta, lr = 16, 40, 5, 64, 1.0, 5.5, 0.5
    f, keys, ky, labels, logits = _clustered(n, m, c, e, 3)
    w = torch.full((n,), 1.0 / n)
    model = TipAdapterModel(keys.cuda(), ky, c, alpha=alpha, beta=beta, train_keys=True)
    opt = torch.optim.SGD([model.keys], lr=lr)
    order = model.order.cpu()

    def restated(dtype):
        k = keys[order].to(dtype).clone().requires_grad_(True)
        traj, losses = [], []
        for _ in range(5):
            loss = _wce(_restate(f.to(dtype), k, ky[order], torch.ones(m, dtype=dtype), alpha, beta, logits.to(dtype)), labels, w.to(dtype))
            (g,) = torch.autograd.grad(loss, k)
            k = (k.detach() - lr * g).requires_grad_(True)
            traj.append(k.detach().clone())
            losses.append(float(loss.detach()))
        return traj, losses

    t64, l64 = restated(torch.float64)
    t32, _ = restated(torch.float32)
    fc, lc, yc, wc = f.cuda(), logits.cuda(), labels.cuda().to(torch.int32), w.cuda()
    got, losses = [], []
    for _ in range(5):
        losses.append(float(steps.tip_step(model, fc, lc, yc, wc, opt)))
        got.append(model.keys.detach().cpu().clone())
    after = float(_wce(model(fc, lc).detach().double(), yc, wc.double()))
    d32 = max(float((a.double() - b).abs().max()) for a, b in zip(t32, t64))
    dn = max(float((a.double() - b).abs().max()) for a, b in zip(got, t64))
    moved = float((t64[-1] - keys[order].double()).abs().max())
    write_report("tip_adapter_trajectory.json", {"D32": d32, "native": dn, "ratio": dn / d32, "keys_moved": moved, "loss_first": losses[0], "loss_after": after})
    print(f"key trajectory: f32 restatement {d32:.3e}, native {dn:.3e} ({dn / d32:.2f} x), keys moved {moved:.3e}; loss {losses[0]:.5f} -> {after:.5f}")
    assert d32 > 0 and moved > 1e3 * d32
    assert dn <= 4 * d32, f"native trajectory deviates {dn / d32:.2f} x the f32 restatement's own deviation"
    assert abs(losses[0] - l64[0]) <= 1e-5 * abs(l64[0])
    assert after < losses[0]


def test_graphed_tip_step_equals_eager():
    import grip_amd  # noqa: F401
    from grip_amd import steps
    from grip_amd.models import TipAdapterModel
    n, m, c, e = 16, 72, 5, 64
    batches = [_clustered(n, m, c, e, 10 + i) for i in range(4)]
    _, keys, ky, _, _ = batches[0]
    w = torch.full((n,), 1.0 / n, device="cuda")
    vw = 0.5 + torch.rand(m, generator=torch.Generator().manual_seed(1))
    out = []
    for graphed in (False, True):
        model = TipAdapterModel(keys.cuda(), ky, c, key_weight=vw, alpha=2.0, beta=5.5, train_keys=True)
        opt = torch.optim.SGD([model.keys], lr=0.3)
        step = steps.GraphedTipStep(model, opt) if graphed else None
        losses, traj = [], []
        for f, _, _, labels, logits in batches:      # the first call captures, the next three replay
            args = (f.cuda(), labels.cuda().to(torch.int32), w, logits.cuda())
            loss = step(*args) if graphed else steps.tip_step(model, args[0], args[3], args[1], w, opt)
            losses.append(float(loss))
            traj.append(model.keys.detach().clone())
        f, _, _, labels, logits = batches[0]          # another batch size: the graphed step runs the eager one
        args = (f[:5].cuda(), labels[:5].cuda().to(torch.int32), w[:5] * n / 5, logits[:5].cuda())
        losses.append(float(step(*args) if graphed else steps.tip_step(model, args[0], args[3], args[1], args[2], opt)))
        traj.append(model.keys.detach().clone())
        out.append((losses, traj))
    (l_e, t_e), (l_g, t_g) = out
    assert l_e == l_g, (l_e, l_g)
    assert all(torch.equal(a, b) for a, b in zip(t_e, t_g))
    assert not torch.equal(t_e[0], t_e[3])


# ---------------------------------------------------------------------------------------------------------------- strategies (tiny towers)
def _conf(**kw):
    import grip_amd  # noqa: F401
    from grip_amd.methods.main import DEFAULTS, Config
    c = dict(DEFAULTS)
    c.update(OPTIM_SEED=1, VIS_ENCODER="small", DATASET_NAME="Synthetic", SPLIT_SEED=500, DATASET_DIR="", EPOCHS=2, WARMUP_EPOCHS=1, N_PSEUDOSHOTS=3,
             N_LABEL=2, LR=0.05, PREFIX_SIZE=4, MODEL="textual_fpl", LEARNING_PARADIGM="ssl", BATCH_SIZE=8)
    c.update(kw)
    return Config(**c)


_RUNS = {}


def _run(tmp, **kw):
    """One TextualFPL training (ssl: two labelled shots per class + CLIP pseudolabels) on the synthetic pool; cached per switch setting."""
    key = tuple(sorted(kw.items()))
    if key in _RUNS:
        return _RUNS[key]
    from grip_amd import methods
    from grip_amd.data import ImagePool, TensorPoolDataset
    from grip_amd.methods.main import synthetic_pool
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        classes, files, images, names = synthetic_pool(5, 10, 64, 500)
        l2i = {c: i for i, c in enumerate(classes)}
        pool = ImagePool(files, images.cuda())
        ids = {"train": [i for i in range(50) if i % 10 < 2], "val": [i for i in range(50) if i % 10 == 2],
               "unl": [i for i in range(50) if 3 <= i % 10 < 8], "test": [i for i in range(50) if i % 10 >= 8]}
        sub = lambda s, lab: TensorPoolDataset([files[i] for i in ids[s]], pool, labels=[names[i] for i in ids[s]] if lab else None, label_map=l2i)      # noqa: E731
        data = {"train": sub("train", True), "val": sub("val", True), "unl": sub("unl", False), "test": sub("test", False)}
        conf = _conf(**kw)
        m = methods.TextualFPL(conf, l2i, "", classes, classes, classes, "cuda")
        best, prompt = m.train(data["train"], data["val"], data["unl"])
        _, logits = m.predict(data["test"], classes)
    finally:
        os.chdir(cwd)
    _RUNS[key] = dict(m=m, conf=conf, data=data, classes=classes, prompt=prompt, logits=logits, best=best, l2i=l2i)
    return _RUNS[key]


def test_strategy_training_free_cache(tmp_path):
    from grip_amd.utils import compute_metrics as cm
    off, on = _run(tmp_path), _run(tmp_path, TIP_ADAPTER=True, TIP_FINETUNE_EPOCHS=0, TIP_ALPHA=2.0, TIP_PSEUDO_WEIGHT=0.5)
    # the pseudolabel pass and the prompt training are untouched
    assert (on["data"]["train"].filepaths, on["data"]["train"].labels) == (off["data"]["train"].filepaths, off["data"]["train"].labels)
    assert len(on["prompt"]) == len(off["prompt"]) and all(np.array_equal(a, b) for a, b in zip(on["prompt"], off["prompt"]))
    assert off["m"].tip is None and on["best"] == off["best"]
    m, tip, train = on["m"], on["m"].tip, on["data"]["train"]
    # the cache holds exactly the training set's rows: its frozen features, unit-normalised, with their labels and weights
    n_train = len(train)
    assert n_train > 10 and tip.keys.shape[0] == n_train and not tip.keys.requires_grad      # 10 labelled shots + the pseudolabelled rows
    with torch.no_grad():
        feats = m.frozen_image_features(train.images, [p.split("/")[-1] for p in train.filepaths])
    assert torch.equal(tip.keys, (feats / feats.norm(dim=-1, keepdim=True))[tip.order])
    labs = torch.tensor([int(l) for l in train.labels], device="cuda")
    assert torch.equal(tip.key_class, labs[tip.order])
    pseudo = torch.tensor([p.split("/")[-1] in m.check_unlabeled for p in train.filepaths], device="cuda")
    assert int(pseudo.sum()) == n_train - 10 and torch.equal(tip.key_weight, torch.where(pseudo, 0.5, 1.0)[tip.order])
    assert (tip.alpha, tip.beta) == (2.0, 5.5)
    # test logits = the logits with the feature off + the float64 cache term of the same features, within the kernel's forward bound
    test = on["data"]["test"]
    with torch.no_grad():
        tf = m.frozen_image_features(test.images)
    base = off["logits"].cuda()
    ref, fb, _, _ = K._reference(tf, tip.keys, tip.class_start, tip.key_weight, tip.alpha, tip.beta, base, torch.zeros_like(base))
    K._check("strategy", "test_logits", on["logits"].cuda(), ref, fb)
    assert (on["logits"] - off["logits"]).min() >= 0 and (on["logits"] - off["logits"]).max() > 0.1
    # the cache has a parameter file of its own, and it round-trips through predict on a strategy that was trained without it
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        fn = cm.save_parameters(on["prompt"], on["conf"], cache=tip)
        path = cm.tip_cache_path(on["conf"])
        assert os.path.exists(fn) and os.path.exists(path) and fn != path
        assert all(np.array_equal(a, b) for a, b in zip(cm.load_parameters(on["conf"]), on["prompt"]))
        other = off["m"]
        other.load_tip_cache(path)
        try:
            _, again = other.predict(off["data"]["test"], off["classes"])
            # a sub-list of the classes: the term's columns are gathered
            _, part = other.predict(off["data"]["test"], off["classes"][1:4])
            term = other.tip(tf, torch.zeros_like(base))
        finally:
            other.tip = None
        _, part_plain = other.predict(off["data"]["test"], off["classes"][1:4])
    finally:
        os.chdir(cwd)
    assert torch.equal(again, on["logits"])
    assert torch.equal(part.cuda(), part_plain.cuda() + term[:, 1:4])


def test_strategy_finetune_and_search(tmp_path):
    grid = dict(TIP_ALPHA_GRID=(0.0, 1.0, 4.0), TIP_BETA_GRID=(1.0, 5.5))
    plain = _run(tmp_path, TIP_ADAPTER=True, TIP_FINETUNE_EPOCHS=0, TIP_ALPHA=2.0, TIP_PSEUDO_WEIGHT=0.5)
    tuned = _run(tmp_path, TIP_ADAPTER=True, TIP_FINETUNE_EPOCHS=2, TIP_ALPHA=2.0, TIP_PSEUDO_WEIGHT=0.5, TIP_LR=0.01, TIP_SEARCH=True, **grid)
    m, tip = tuned["m"], tuned["m"].tip
    assert all(np.array_equal(a, b) for a, b in zip(tuned["prompt"], plain["prompt"]))
    assert tip.keys.requires_grad and tip.keys.shape == plain["m"].tip.keys.shape and not torch.equal(tip.keys.detach(), plain["m"].tip.keys)
    assert len(m.tip_losses) == 2 and m.tip_losses[1] < m.tip_losses[0], m.tip_losses
    # TIP_SEARCH: the returned pair is the arg-max of the grid (first wins), by brute force on the same validation inputs
    a, b, acc = m.tip_search
    classes, _, lut = m._class_space(False)
    vf, vl, vy, _ = m._tip_inputs(tuned["data"]["val"], classes, lut)
    assert len(vy) == 5
    y = tip.key_class
    table = [(ga, gb, float((_restate(vf.double(), tip.keys.detach().double(), y, tip.key_weight.double(), ga, gb, vl.double()).argmax(1) == vy).double().mean()))
             for ga in grid["TIP_ALPHA_GRID"] for gb in grid["TIP_BETA_GRID"]]
    best = max(t[2] for t in table)
    assert acc == pytest.approx(best) and (a, b) == next((ga, gb) for ga, gb, s in table if s == pytest.approx(best))
    assert (tip.alpha, tip.beta) == (a, b)
