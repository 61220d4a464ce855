"""CPU: tests/mixer_ref.py itself, and the workspace hook that tests/test_gpu_mixer_kernels.py addresses the mixer's buffers with.

Composition: the step functions chained end to end equal torch float64 autograd of the module graph (tests/test_gpu_upt_deep.py::_reference_mix_deep)
on all outputs and all 22 / 23 gradients to 1e-12 -- two float64 statements of the same mathematics.  Non-vacuity: the same statements evaluated in
float32 on the CPU (a restatement of every launch with torch's own summation orders) stay inside every bound at every case, family and
half_linears, and every fault of mixer_ref.FAULTS exceeds the bound of its step on at least one element at every case that has the edge the fault
needs (elsewhere -- no K % 64 tail, one prompt per modality, no deep tokens -- the fault is the identity, which is asserted too).  The worst
ratios go to tests/_out/mixer_ref_host.json."""
import ctypes
import functools

import pytest
import torch

import mixer_ref as M
from conftest import write_report
from test_gpu_upt_deep import _reference_mix_deep

_BLOCK = "transformer.resblocks.0."
PARAMETER_NAMES = {
    "coop": "coop_embeddings", "vpt": "vpt_embeddings", "deep": "vpt_embeddings_deep", "coop_pre_w": "proj_coop_pre.weight", "coop_pre_b": "proj_coop_pre.bias",
    "vpt_pre_w": "proj_vpt_pre.weight", "vpt_pre_b": "proj_vpt_pre.bias", "ln1_g": _BLOCK + "ln_1.weight", "ln1_b": _BLOCK + "ln_1.bias",
    "in_w": _BLOCK + "attn.in_proj_weight", "in_b": _BLOCK + "attn.in_proj_bias", "out_w": _BLOCK + "attn.out_proj.weight", "out_b": _BLOCK + "attn.out_proj.bias",
    "ln2_g": _BLOCK + "ln_2.weight", "ln2_b": _BLOCK + "ln_2.bias", "fc_w": _BLOCK + "mlp.c_fc.weight", "fc_b": _BLOCK + "mlp.c_fc.bias",
    "proj_w": _BLOCK + "mlp.c_proj.weight", "proj_b": _BLOCK + "mlp.c_proj.bias", "coop_post_w": "proj_coop_post.weight", "coop_post_b": "proj_coop_post.bias",
    "vpt_post_w": "proj_vpt_post.weight", "vpt_post_b": "proj_vpt_post.bias"}
_REPORT = {}


class _Module:
    """What _reference_mix_deep reads of a UPTModel: named_parameters() and dtype."""

    def __init__(self, case, b, hl):
        P, dt, dv, _, nd = case
        self.dtype = torch.float16 if hl else torch.float32
        deep = b["deep"] if nd else torch.zeros(0, dv)
        self._p = {PARAMETER_NAMES[n]: b[n] for n in M.MIXER_TENSORS}
        self._p.update({"coop_embeddings": b["coop"].reshape(1, P, dt), "vpt_embeddings": b["vpt"].reshape(1, P, dv), "vpt_embeddings_deep": deep.reshape(nd, P, dv)})

    def named_parameters(self):
        return self._p.items()


def _id(case):
    return "-".join(str(v) for v in case)


@pytest.mark.parametrize("hl", (0, 1))
@pytest.mark.parametrize("case", M.CASES, ids=_id)
def test_steps_compose_to_the_module_graph(case, hl):
    """eps = 1e-5 and 1.702 exactly, as the graph has them (the kernel's f32 constants differ from them by 3e-8 and 1e-8 relative); the rounding of the
    prompt gradients with half_linears is not in a graph whose leaves are float64."""
    P, dt, dv, D, nd = case
    b = {n: t.double() for n, t in M.make_inputs(case, "randn", hl, seed=1).items()}
    got = M.run(case, hl, b, eps=1e-5, c=1.702, round_prompt_grads=False)
    ref = _reference_mix_deep(_Module(case, b, hl))
    ups = (b["d_coop"].reshape(1, P, dt), b["d_vpt"].reshape(1, P, dv), b["d_deep"].reshape(nd, P, dv) if nd else torch.zeros(0, P, dv, dtype=torch.float64))
    sum((t * w).sum() for t, w in zip(ref[:3], ups)).backward()
    pairs = [("coop_out", ref[0]), ("vpt_out", ref[1])] + ([("deep_out", ref[2])] if nd else [])
    pairs += [("g:" + n, ref[3][PARAMETER_NAMES[n]].grad) for n in M.MIXER_TENSORS + (("deep",) if nd else ())]
    assert len(pairs) == (26 if nd else 24)
    for name, want in pairs:
        want = want.detach().reshape(got[name].shape)
        rel = ((got[name] - want).abs().max() / want.abs().max()).item()
        assert rel <= 1e-12, (name, rel)


@functools.lru_cache(maxsize=None)
def _restated(case, family, hl):
    """The float32 restatement of every launch, chained, as float64 images of its f32 buffers."""
    b32 = M.run(case, hl, M.make_inputs(case, family, hl))
    assert all(t.dtype == torch.float32 for t in b32.values())
    return {n: t.double() for n, t in b32.items()}


def _got(b, name):
    return M.residual16(b[name[:-4]]) if name.endswith("#f16") else b[name]


@pytest.mark.parametrize("hl", (0, 1))
@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("case", M.CASES, ids=_id)
def test_float32_restatement_is_inside_every_bound(case, family, hl):
    b = _restated(case, family, hl)
    worst = {}
    for step, _, fn in M.steps(case, hl):
        for name, (value, bound) in fn(b, None).items():
            assert value.shape == torch.Size(M.shapes(case)[name.split("#")[0]]), (step, name, value.shape)
            ratio = M.worst_ratio(_got(b, name), value, bound)
            worst[step] = max(worst.get(step, 0.0), ratio)
            assert ratio <= 1.0, (step, name, ratio)
    _REPORT[f"{_id(case)} {family} hl{hl}"] = worst
    write_report("mixer_ref_host.json", _REPORT)


@pytest.mark.parametrize("fault", M.FAULTS)
@pytest.mark.parametrize("case", M.CASES, ids=_id)
def test_every_fault_leaves_its_bound(case, fault):
    target, family, applies = M.FAULT_SITES[fault]
    b = _restated(case, family, 0)
    (fn,) = [f for n, _, f in M.steps(case, 0) if n == target]
    clean, faulty = fn(b, None), fn(b, fault)
    if not applies(case):
        assert all(torch.equal(clean[n][0], faulty[n][0]) for n in clean), "the fault is not the identity where its edge is missing"
        return
    assert all(torch.equal(clean[n][1], faulty[n][1]) for n in clean), "a fault changed a bound"
    ratios = {n: M.worst_ratio(_got(b, n), v, e) for n, (v, e) in faulty.items()}
    assert max(ratios.values()) > 1.0, ratios


# ------------------------------------------------------------------------------------------------ grip_debug_upt_mixer_slot
def _slots(lib, P, nd, dt, dv, D):
    name, off, n = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
    out, i = [], 0
    while lib.grip_debug_upt_mixer_slot(P, nd, dt, dv, D, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(n)) == 0:
        out.append((name.value.decode(), off.value, n.value))
        i += 1
    return out


@pytest.mark.parametrize("case", M.CASES + ((16, 1280, 1280, 256, 31), (4, 512, 768, 128, 1)), ids=_id)
def test_slot_hook_names_a_consistent_layout(case):
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    P, dt, dv, D, nd = case
    slots = _slots(lib, P, nd, dt, dv, D)
    names = [s[0] for s in slots]
    assert len(set(names)) == len(names)
    assert set(names) == set(M.FORWARD_SLOTS + M.BACKWARD_SLOTS) - (set() if nd else set(M.DEEP_SLOTS))
    assert all((n in names) == (nd > 0) for n in M.DEEP_SLOTS)
    sh = M.shapes(case)
    for n, off, floats in slots:
        assert off % 64 == 0 and floats > 0, (n, off)
        assert floats == torch.Size(sh[n]).numel(), (n, floats, sh[n])
    spans = sorted((off, off + floats) for _, off, floats in slots)
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "overlapping slots"
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_upt_mixer_deep_workspace(P, nd, dt, dv, D, ctypes.byref(nbytes)))
    assert spans[-1][1] * 4 <= nbytes.value - 256
    if nd == 0:
        shallow = ctypes.c_size_t()
        native.check(lib.grip_upt_mixer_workspace(P, dt, dv, D, ctypes.byref(shallow)))
        assert shallow.value == nbytes.value


def test_slot_hook_refuses_what_the_mixer_refuses():
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    name, off, n = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
    call = lambda P, nd, dt, dv, D, i=0: lib.grip_debug_upt_mixer_slot(P, nd, dt, dv, D, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(n))      # noqa: E731
    nbytes = ctypes.c_size_t()
    for (P, nd, dt, dv, D), word in (((4, 0, 63, 768, 128), b"widths"), ((4, 0, 512, 1281, 128), b"widths"), ((4, 0, 512, 768, 100), b"dim"),
                                     ((17, 0, 512, 768, 128), b"n_prompt"), ((4, 32, 512, 768, 128), b"n_deep"), ((4, -1, 512, 768, 128), b"n_deep")):
        assert call(P, nd, dt, dv, D) == 1 and word in lib.grip_last_error(), (P, nd, dt, dv, D)
        assert lib.grip_upt_mixer_deep_workspace(P, nd, dt, dv, D, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error()
    assert call(4, 0, 512, 768, 128, 28) == 1 and b"past the end" in lib.grip_last_error()
    assert call(4, 0, 512, 768, 128, -1) == 1 and call(4, 2, 512, 768, 128, 32) == 1 and call(4, 2, 512, 768, 128, 31) == 0
    assert lib.grip_debug_upt_mixer_slot(4, 0, 512, 768, 128, 0, None, None, None) == 1 and b"null pointer" in lib.grip_last_error()
