"""CPU: the launch map of tests/tower_ref.py against the mathematics, and its bounds against a float32 stand-in ("Tower pass tests").

a. The stages chained in float64 (nothing rounded, the derived weights exact) equal a plain torch float64 restatement of the tower -- pre-LN blocks,
   QuickGELU, the causal mask, CLS / EOT read rows, ln_post and the projection, shallow / deep / per-image prompts, one context or one per class -- to
   1e-10 on every output and, for a train-mode pass, on every prompt gradient against torch autograd (backward chain).  This ties the schedule (fold, statistics plumbing, read-rows-only last block, shared-prefix layout) to the model
   independently of csrc/tower.hip.
b. The same chain in float32 arithmetic with the tower's f16 stores stays inside every bound, element by element (the backward's stand-in is the float64
   value rounded as the tower stores it: it exercises the chain and the stores, not independent f32 arithmetic).
c. Every fault of tower_ref.FAULTS, applied to the value of the step it is an error of, leaves the bound of that step on every pass that has the edge;
   on a pass without the edge it changes nothing."""
import pytest
import torch
import torch.nn.functional as F

import tower_ref as T

IDS = [p.key() for p in T.CASES]


def _chain(p, family, like64, faults=()):
    """Runs the schedule on host buffers.  -> (buffers at the end, {label: worst ratio}, {fault: (applies, worst ratio, changed)})."""
    w = T.make_weights(p, family)
    sched = T.all_steps(p)
    bufs = T.derive(w, p, exact=like64)
    for k, v in T.make_inputs(p).items():
        bufs[k] = v.double() if (like64 and v.is_floating_point()) else v
    bufs.update(T.empty_buffers(p, sched, like64))
    sites = {f: T.fault_step(p, sched, f) for f in faults}
    worst, seen = {}, {}
    for i, s in enumerate(sched):
        before = {k: (v.clone() if not k.startswith(("w:", "in:")) else v) for k, v in bufs.items()}
        for region, value in s.emu(before).items():
            T.write(bufs, region, value)
        if like64:
            continue
        checks = s.ref(before, bufs)
        for name, (got, value, bound) in checks.items():
            assert got.shape == value.shape == bound.shape, (s.label, name, got.shape, value.shape, bound.shape)
            assert torch.isfinite(got.double()).all(), (s.label, name)
            r = T.worst_ratio(got, value, bound)
            worst[s.label] = max(worst.get(s.label, 0.0), r)
            assert r <= 1.0, (p.key(), family, s.label, name, r)
        if s.exact is not None:
            for region, want in s.exact(before).items():
                assert T.same_bits(T.view(bufs, region), want), (s.label, region.slot)
        for f, (at, applies) in sites.items():
            if at != i:
                continue
            faulted = s.ref(before, bufs, fault=f)
            ratio = max(T.worst_ratio(got, value, bound) for got, value, bound in faulted.values())
            changed = any(not torch.equal(faulted[n][1], checks[n][1]) for n in checks)
            seen[f] = (applies, ratio, changed)
    return bufs, worst, seen


# ------------------------------------------------------------------------------------------------ the plain restatement
def _block(x, w, l, H, causal, eps):
    pre = f"transformer.resblocks.{l}."
    B, S, d = x.shape
    y = F.layer_norm(x, (d,), w[pre + "ln_1.weight"].reshape(-1), w[pre + "ln_1.bias"].reshape(-1), eps)
    q, k, v = F.linear(y, w[pre + "attn.in_proj_weight"], w[pre + "attn.in_proj_bias"].reshape(-1)).chunk(3, -1)
    q, k, v = (t.reshape(B, S, H, d // H).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / (d // H) ** 0.5
    if causal:
        s = s + torch.full((S, S), float("-inf"), dtype=x.dtype).triu(1)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, d)
    x = x + F.linear(o, w[pre + "attn.out_proj.weight"], w[pre + "attn.out_proj.bias"].reshape(-1))
    y = F.layer_norm(x, (d,), w[pre + "ln_2.weight"].reshape(-1), w[pre + "ln_2.bias"].reshape(-1), eps)
    h = F.linear(y, w[pre + "mlp.c_fc.weight"], w[pre + "mlp.c_fc.bias"].reshape(-1))
    return x + F.linear(h * torch.sigmoid(1.702 * h), w[pre + "mlp.c_proj.weight"], w[pre + "mlp.c_proj.bias"].reshape(-1))


def _restate(p, w, inp):
    """The tower as a module would compute it, float64: embeddings [B, E].  inp may hold leaf tensors that require a gradient (prefix, deep)."""
    w = {k: v.double() for k, v in w.items()}
    d, B, P = p.d, p.B, p.P
    LN_EPS = T.FR.LN_EPS          # the kernels' 1e-5f
    ln = lambda x, n: F.layer_norm(x, (d,), w[n + ".weight"].reshape(-1), w[n + ".bias"].reshape(-1), LN_EPS)  # noqa: E731
    if p.kind == 0:
        img = inp["in:images"].double().view(B, 3, p.resolution, p.resolution)
        conv = w["conv1.weight"][:, :3 * p.patch ** 2].reshape(d, 3, p.patch, p.patch)
        tok = F.conv2d(img, conv, stride=p.patch).flatten(2).transpose(1, 2)
        cls = w["class_embedding"].reshape(1, 1, d).expand(B, 1, d)
        if not p.no_pos:
            cls, tok = cls + w["positional_embedding"][0], tok + w["positional_embedding"][1:]
        parts = [cls] + ([inp["in:prefix"].double().view(-1, P, d).expand(B, P, d)] if P else []) + [tok]
        x = ln(torch.cat(parts, 1), "ln_pre")
    else:
        x = w["token_embedding.weight"][inp["in:ids"].view(B, p.seq0).long()[:, :p.S]].clone()
        if P:
            x[:, 1:1 + P] = inp["in:prefix"].double().view(-1, P, d).expand(B, P, d)
        if not p.no_pos:
            x = x + w["positional_embedding"][:p.S]
    for l in range(p.layers):
        if 1 <= l <= p.n_deep:
            x = x.clone()
            x[:, 1:1 + P] = inp["in:deep"].double().view(p.n_deep, -1, P, d)[l - 1].expand(B, P, d)
        x = _block(x, w, l, p.H, p.causal, LN_EPS)
    read = x[torch.arange(B), torch.tensor(p.eot) if p.kind else torch.zeros(B, dtype=torch.long)]
    return ln(read, "ln_post" if p.kind == 0 else "ln_final") @ w["proj" if p.kind == 0 else "text_projection"]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("p", T.CASES, ids=IDS)
def test_float64_chain_equals_the_plain_tower(p, family):
    bufs, _, _ = _chain(p, family, like64=True)
    got = bufs["out:emb"].view(p.B, p.E)
    want = _restate(p, T.make_weights(p, family), T.make_inputs(p))
    err = (got - want).abs().max().item()
    assert torch.isfinite(got).all() and err <= 1e-10 * max(1.0, want.abs().max().item()), (p.key(), family, err)
    if not p.train:
        return
    # the backward chain against autograd of the plain tower: every prompt gradient of L = sum(embedding * grad_emb)
    inp = {k: (v.double().requires_grad_(True) if k in ("in:prefix", "in:deep") else v) for k, v in T.make_inputs(p).items()}
    (_restate(p, T.make_weights(p, family), inp) * inp["in:grad_emb"].double().view(p.B, p.E)).sum().backward()
    for name, leaf in (("out:grad_prefix", "in:prefix"), ("out:grad_deep", "in:deep")):
        if leaf in inp:
            g, a = bufs[name].reshape(-1), inp[leaf].grad.reshape(-1)
            assert g.shape == a.shape and torch.isfinite(g).all(), (p.key(), name)
            err = (g - a).abs().max().item()
            assert err <= 1e-10 * max(a.abs().max().item(), 1e-300), (p.key(), family, name, err, a.abs().max().item())


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("p", T.CASES, ids=IDS)
def test_float32_chain_stays_inside_every_bound(p, family):
    _, worst, _ = _chain(p, family, like64=False)
    assert set(worst) == {s.label for s in T.all_steps(p)}


@pytest.mark.parametrize("p", T.CASES, ids=IDS)
def test_every_fault_leaves_its_bound_where_the_edge_exists(p):
    _, _, seen = _chain(p, "randn", like64=False, faults=T.FAULTS)
    for f in T.FAULTS:
        at, applies = T.fault_step(p, T.all_steps(p), f)
        if applies:
            assert at is not None and f in seen, (p.key(), f, "the pass has the edge but no step to apply it to")
            assert seen[f][1] > 1.0, (p.key(), f, "stays inside the bound", seen[f][1])
        elif f in seen:
            assert not seen[f][2] and seen[f][1] <= 1.0, (p.key(), f, "changes a value on a pass without the edge")


def test_every_fault_has_a_pass_with_its_edge():
    for f in T.FAULTS:
        assert any(T.fault_step(p, T.all_steps(p), f)[1] for p in T.CASES), f


def test_the_schedule_names_each_region_once_per_step_and_every_label_once():
    for p in T.CASES:
        sched = T.all_steps(p)
        labels = [s.label for s in sched]
        assert len(set(labels)) == len(labels), p.key()
        for s in sched:
            assert len({(r.slot, r.col0, r.row0) for r in s.owns}) == len(s.owns), (p.key(), s.label)
            assert all(T.f16slot(r.slot) or r.slot in T.F32_SLOTS for r in s.owns), (p.key(), s.label)


def test_tower_slot_hook_reports_the_carve_and_refuses_what_it_refuses():
    """Host only (no launch): grip_debug_tower_slot on a tower handle that was never finalized."""
    import ctypes

    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    blob = (ctypes.c_char * 64)()

    def tower(kind, precision=0):
        dims = native.Dims(kind, 128 if precision != 2 else 256, 3, 2 if precision != 2 else 4, 128, 17 if kind == 0 else 16, 8 if kind == 0 else 0,
                           32 if kind == 0 else 0, 64 if kind else 0, 4, precision)
        h = ctypes.c_void_p()
        native.check(lib.grip_tower_create(ctypes.byref(dims), blob, blob, ctypes.byref(h)))
        return h

    def slots(h, batch, P, seq_len, train, shared):
        name, layer, off, n, out, i = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), [], 0
        while lib.grip_debug_tower_slot(h, batch, P, seq_len, train, shared, i, ctypes.byref(name), ctypes.byref(layer), ctypes.byref(off), ctypes.byref(n)) == 0:
            out.append((name.value.decode(), layer.value, off.value, n.value))
            i += 1
        return out

    vit, text, vit32 = tower(0), tower(1), tower(0, 1)
    for h, args in ((vit, (3, 3, 0, 0, 0)), (vit, (3, 3, 0, 1, 0)), (text, (5, 3, 12, 0, 0)), (text, (5, 3, 12, 0, 1)), (text, (5, 3, 12, 1, 1)), (vit32, (3, 0, 0, 0, 0))):
        got = slots(h, *args)
        assert got, args
        nbytes = ctypes.c_size_t()
        native.check(lib.grip_workspace_bytes(h, args[0], args[1], args[2], args[3], ctypes.byref(nbytes)))
        own = sorted((off, off + n) for name, _, off, n in got if name != "patches")
        assert all(a[1] <= b[0] for a, b in zip(own, own[1:])) and own[-1][1] <= nbytes.value and all(off % 256 == 0 for off, _ in own), args
        names = [(n, l) for n, l, _, _ in got]
        assert len(set(names)) == len(names), args
        by = {(n, l): (off, nb) for n, l, off, nb in got}
        if h is not text:
            assert by[("patches", -1)][0] == by[("h", -1)][0], "patches is reported at the offset of h"
        if args[3]:      # train: one saved stream per block boundary, by layer
            assert [l for n, l in names if n == "x_in"] == [0, 1, 2, 3] and [l for n, l in names if n == "hpre_l"] == [0, 1, 2]
        else:
            assert all(l == -1 for _, l in names)
    assert "kv_part" in {n for n, *_ in slots(text, 5, 3, 12, 1, 1)} and "kv_part" not in {n for n, *_ in slots(text, 5, 3, 12, 1, 0)}
    # what the carve refuses
    name, layer, off, n = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    refs = (ctypes.byref(name), ctypes.byref(layer), ctypes.byref(off), ctypes.byref(n))
    bad = ((vit, (0, 0, 0, 0, 0), b"batch"), (vit, (3, 5, 0, 0, 0), b"max_prefix"), (vit, (3, 3, 4, 0, 0), b"seq_len"), (vit, (3, 3, 0, 0, 1), b"shared-prefix"),
           (text, (5, 3, 17, 0, 0), b"seq_len"), (text, (5, 3, 4, 0, 0), b"does not fit"), (text, (5, 0, 12, 0, 1), b"shared-prefix"),
           (vit32, (3, 0, 0, 1, 0), b"inference-only"))
    for h, args, text_ in bad:
        assert lib.grip_debug_tower_slot(h, *args, 0, *refs) == 1 and text_ in lib.grip_last_error(), (args, lib.grip_last_error())
    assert lib.grip_debug_tower_slot(vit, 3, 3, 0, 0, 0, len(slots(vit, 3, 3, 0, 0, 0)), *refs) == 1 and b"past the end" in lib.grip_last_error()
    assert lib.grip_debug_tower_slot(vit, 3, 3, 0, 0, 0, -1, *refs) == 1
    assert lib.grip_debug_launch_budget(0) == 0
    for h in (vit, text, vit32):
        lib.grip_tower_destroy(h)


def test_the_cooperative_split_case_sits_at_the_smallest_width_that_has_one():
    """Host only: grip_debug_coop_split(M, d, 4 d) is 1 for every M at width 128, and width 256 (the next the layout accepts) has it; every train-mode
    text case carries the factor the library would choose."""
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    assert all(lib.grip_debug_coop_split(M, 128, 512) == 1 for M in range(1, 4097))
    coop = [p for p in T.CASES if p.coop_ks > 1]
    assert coop and all(p.d == 256 and p.kind == 1 and p.train for p in coop)
    for p in T.CASES:
        if p.kind == 1 and p.train:
            assert lib.grip_debug_coop_split(p.M, p.d, 4 * p.d) == p.coop_ks, p.key()
