"""The prompt steps on soft targets (steps.SoftTargets -> engine.SoftCEFn -> csrc/soft_ce.hip), on the small synthetic model the other step tests use:
each of the eager steps and its graphed twin give bit-equal losses, logits and updated parameters over three steps with `soft` given; a replay after a
second SoftTargetStore.record() of the same shape trains on the new matrix; soft=None is the parent's step bit for bit (and so is a SoftTargets without
a matrix and without smoothing: the kernel's hard rows are grip_weighted_ce's)."""
import pytest
import torch

import soft_ce_ref as R

pytestmark = pytest.mark.gpu
B, C, CZ, POOL = 8, 7, 5, 12
IDS = [10, 11, 12, 13, 14, 15, 16]          # label ids of the training classes; the pass ranked five of them, in another order
RANKED = [15, 11, 16, 10, 13]


def _setup():
    import grip_amd  # noqa: F401
    from grip_amd import clip
    m, _ = clip.load("small", device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.randn(B, 3, 64, 64, device="cuda", generator=g) for _ in range(3)]
    ys = [torch.randint(0, C, (B,), device="cuda", generator=g, dtype=torch.int32) for _ in range(3)]
    rows = [torch.tensor(r, dtype=torch.int32, device="cuda") for r in ([0, -1, 3, 11, -1, 5, 2, 7], [-1, -1, 1, 4, 9, 10, -1, 6], [8, 2, -1, 0, 3, -1, 11, 5])]
    w = torch.full((B,), 1 / B, device="cuda")
    return m, xs, ys, rows, w


def _matrix(seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.softmax(2 * torch.randn(POOL, CZ, generator=g), dim=1)
    z[3] = 0.0
    z[5, 1] = 0.0
    return z.float().cuda()


def _store(z):
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    store = pl.SoftTargetStore()
    store.record([f"pool/img_{i}.png" for i in range(POOL)], RANKED, z)
    return store


def _soft(store, temperature=0.5, smoothing=0.1):
    from grip_amd import steps
    return steps.SoftTargets(store.matrix, store.col_map(IDS), temperature, smoothing)


def _models(kind, m):
    """(model, params, eager(soft) -> step callable, graphed(soft) -> step object) of one kind of step; fresh parameters on every call."""
    from grip_amd import clip, rng, steps
    from grip_amd.models import CustomImageEncoder, CustomTextEncoder, ImagePrefixModel, TextPrefixModel, UPTModel
    classes = [f"class {i}" for i in range(C)]
    N = lambda name, shape: torch.from_numpy(rng.normal(4, rng.stream_id(name), shape, 0.0, 0.02)).cuda()   # noqa: E731
    if kind in ("coop", "coop_feature"):
        tm = TextPrefixModel(N("sc.p", (1, 4, 256)), CustomTextEncoder(m, "cuda", torch.float32), classes, device="cuda")
        opt = torch.optim.SGD([tm.prefix], lr=0.1, weight_decay=0.1)
        if kind == "coop":
            eager = lambda soft: (lambda x, y, w, r: steps.coop_step(tm, m, x, y, w, opt, return_logits=True, soft=soft, soft_row=r))      # noqa: E731
            return [tm.prefix], eager, lambda soft: steps.GraphedCoopStep(tm, m, opt, soft=soft)
        feats = lambda x: m.encode_image(x).detach()      # noqa: E731
        eager = lambda soft: (lambda x, y, w, r: steps.coop_step(tm, m, None, y, w, opt, image_features=feats(x), return_logits=True, soft=soft, soft_row=r))      # noqa: E731

        def graphed(soft):
            g = steps.GraphedCoopFeatureStep(tm, m, opt, soft=soft)
            call = lambda x, y, w, r=None: g(feats(x), y, w, r)      # noqa: E731
            call.step = g
            return call
        return [tm.prefix], eager, graphed
    if kind == "vpt":
        txt = m.encode_text(clip.tokenize([f"a photo of a {c}" for c in classes]).cuda())
        im = ImagePrefixModel(N("sv.p", (4, 256)), CustomImageEncoder(m.visual), device="cuda")
        opt = torch.optim.SGD([im.prefix], lr=0.1, weight_decay=0.1)
        eager = lambda soft: (lambda x, y, w, r: steps.vpt_step(im, txt, 100.0, x, y, w, opt, return_logits=True, soft=soft, soft_row=r))      # noqa: E731
        return [im.prefix], eager, lambda soft: steps.GraphedVptStep(im, txt, 100.0, opt, soft=soft)
    torch.manual_seed(7)
    um = UPTModel(N("su.c", (1, 4, 256)), N("su.v", (1, 4, 256)), None, CustomImageEncoder(m.visual), CustomTextEncoder(m, "cuda", torch.float32), classes, 128,
                  device="cuda", dtype=torch.float32)
    ps = [p for p in um.parameters() if p.requires_grad]
    opt = torch.optim.SGD(ps, lr=0.01, weight_decay=0.1)
    eager = lambda soft: (lambda x, y, w, r: steps.upt_step(um, 100.0, x, y, w, opt, return_logits=True, soft=soft, soft_row=r))      # noqa: E731
    return ps, eager, lambda soft: steps.GraphedUptStep(um, 100.0, opt, soft=soft)


def _run(kind, m, xs, ys, rows, w, graphed, z_after_first=None):
    """(losses, logits, parameters) of three steps; z_after_first: a second record() of the same shape between the first step and the second."""
    store = _store(_matrix(1))
    soft = _soft(store)
    ps, eager, make_graphed = _models(kind, m)
    step = make_graphed(soft) if graphed else eager(soft)
    losses, logits = [], []
    for i, (x, y, r) in enumerate(zip(xs, ys, rows)):
        if i == 1 and z_after_first is not None:
            at = store.matrix.data_ptr()
            store.record([f"pool/img_{i}.png" for i in range(POOL)], RANKED, z_after_first)
            assert store.matrix.data_ptr() == at and store.records == 2, "a second record() of the same shape must keep the buffer where it is"
        out = step(x, y, w, r)
        if graphed:
            losses.append(out.clone())
            logits.append(getattr(step, "step", step).logits.clone())
        else:
            losses.append(out[0].clone())
            logits.append(out[1].clone())
    return losses, logits, [p.detach().clone() for p in ps]


def _same(a, b):
    return all(torch.equal(x, y) for part_a, part_b in zip(a, b) for x, y in zip(part_a, part_b)) and all(len(x) == len(y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["coop", "coop_feature", "vpt", "upt"])
def test_graphed_step_equals_eager_step_on_soft_targets(kind):
    m, xs, ys, rows, w = _setup()
    eager = _run(kind, m, xs, ys, rows, w, graphed=False)
    graphed = _run(kind, m, xs, ys, rows, w, graphed=True)
    assert _same(eager, graphed)
    assert all(torch.isfinite(l) for l in eager[0]) and not torch.equal(eager[2][0], _models(kind, m)[0][0].detach())      # (finite, and something was trained)


def test_a_replay_after_a_second_record_trains_on_the_new_matrix():
    m, xs, ys, rows, w = _setup()
    z2 = _matrix(2)
    eager = _run("coop", m, xs, ys, rows, w, graphed=False, z_after_first=z2)
    graphed = _run("coop", m, xs, ys, rows, w, graphed=True, z_after_first=z2)
    stale = _run("coop", m, xs, ys, rows, w, graphed=True)
    assert _same(eager, graphed)
    assert torch.equal(stale[0][0], graphed[0][0]) and not torch.equal(stale[0][1], graphed[0][1])      # the first step saw matrix 1, the second one matrix 2


def test_the_step_targets_are_the_float64_targets():
    """One eager CoOp step's logits gradient is engine.soft_ce's on the store's matrix and map: checked against float64 under the kernel's bound."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    m, xs, ys, rows, w = _setup()
    store = _store(_matrix(1))
    soft = _soft(store)
    assert store.col_map(IDS).tolist() == [IDS.index(c) for c in RANKED] and store.col_map(IDS) is store.col_map(list(IDS))
    logits = torch.randn(B, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 3
    loss, grad, target = engine.soft_ce(logits, ys[0], w, soft.matrix, rows[0], soft.col_map, soft.temperature, soft.smoothing, want_target=True)
    ref = R.soft_ce64(logits, ys[0], w, soft.matrix, rows[0], soft.col_map, R.inv_temperature(soft.temperature), soft.smoothing)
    assert R.check(ref, loss, grad, target) <= 1.0
    unranked = [i for i, c in enumerate(IDS) if c not in RANKED]
    soft_rows = rows[0] >= 0
    floor_ = torch.tensor(0.1, dtype=torch.float32) / C
    assert (target[soft_rows][:, unranked] == floor_.item()).all()          # a class the pass did not rank gets the smoothing floor and nothing else


@pytest.mark.parametrize("kind", ["coop", "vpt", "upt"])
def test_soft_none_is_the_parents_step(kind):
    """soft=None calls WeightedCEFn exactly as before; the reference trajectory here is the parent's step written out (forward, CosineHeadFn,
    WeightedCEFn, backward, optimizer).  A SoftTargets without matrix and smoothing goes through grip_soft_ce and lands on the same bits."""
    from grip_amd import steps
    m, xs, ys, rows, w = _setup()
    out = []
    for mode in ("none", "parent", "empty", "graphed_none"):
        ps, eager, make_graphed = _models(kind, m)
        if mode == "parent":
            real = steps.step_loss
            steps.step_loss = lambda logits, labels, row_weight, soft=None, soft_row=None: steps.WeightedCEFn.apply(logits, labels, row_weight)
        try:
            if mode == "graphed_none":
                g = make_graphed(None)
                losses = [g(x, y, w).clone() for x, y in zip(xs, ys)]
            else:
                step = eager(steps.SoftTargets() if mode == "empty" else None)
                losses = [step(x, y, w, None)[0].clone() for x, y in zip(xs, ys)]
        finally:
            if mode == "parent":
                steps.step_loss = real
        out.append((losses, [p.detach().clone() for p in ps]))
    for other in out[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out[0][0], other[0])) and all(torch.equal(a, b) for a, b in zip(out[0][1], other[1]))


def test_store_and_steps_refuse_what_they_cannot_serve():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl, steps
    store = pl.SoftTargetStore()
    with pytest.raises(ValueError, match="no pass has recorded"):
        store.rows(["a.png"])
    z = _matrix(1)
    store.record(["a/x.png", "b/x.png", "a/y.png"] + [f"p/{i}.png" for i in range(POOL - 3)], RANKED, z)
    assert store.rows(["y.png", "other/y.png", "nowhere.png", "p/4.png"]).tolist() == [2, 2, -1, 7]
    assert store.rows(["x.png", "y.png"], hard=[True, False]).tolist() == [-1, 2]          # a labelled row is not asked about
    with pytest.raises(ValueError, match="names two rows"):
        store.rows(["y.png", "x.png"])
    with pytest.raises(ValueError, match="does not hold"):
        store.col_map(IDS[:4])
    with pytest.raises(ValueError, match=r"float32 \[3, 5\]"):
        store.record(["a", "b", "c"], RANKED, z)
    with pytest.raises(TypeError):
        with pl.soft_targets(object()):
            pass
    with pl.soft_targets(None) as got:
        assert got is None and pl.soft_target_store() is None
    with pl.soft_targets(store):
        assert pl.soft_target_store() is store
    assert pl.soft_target_store() is None
    for bad in (dict(matrix=z), dict(temperature=0.0), dict(smoothing=1.0), dict(smoothing=-0.1)):
        with pytest.raises(ValueError, match="SoftTargets"):
            steps.SoftTargets(**bad)
    with pytest.raises(ValueError, match="soft_row"):
        steps.step_loss(torch.zeros(2, C, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda"), _soft(_store(z)))
