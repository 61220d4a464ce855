"""The UPT prompt mixer (csrc/mixer.hip) launch by launch against float64: grip_upt_mixer_forward / _backward and the _deep pair through ctypes on a
workspace of the test's own, every buffer of the workspace addressed by name through grip_debug_upt_mixer_slot.

Each operation of each launch is checked against tests/mixer_ref.py evaluated in float64 on the buffers THAT launch read (taken from the workspace,
so no rounding-boundary flip of an earlier stage leaks into a later check), every element against its derived bound (the module docstring of
mixer_ref.py; DESIGN.md, "Mixer kernel tests").  The worst |err| / bound per step and case goes to tests/_out/mixer_kernels.json.

The workspace, both outputs, every gradient buffer and grad_vpt_deep are NaN-prefilled; every operand and every output is followed by NaN guard
floats.  After the forward the forward slots are finite and everything else of the workspace -- backward slots, the padding between slots, the
guard -- is still NaN; after the backward every slot is finite, the padding and the guards are still NaN and the forward slots have kept their bits.
A second forward and backward on a fresh workspace repeats every bit (no atomics)."""
import ctypes

import pytest
import torch

import mixer_ref as M
from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 64          # floats
_REPORT = {}
NAN = float("nan")


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _guarded(shape, fill=None):
    """One allocation of the tensor's floats followed by GUARD NaN floats: (buffer, view of the owned floats)."""
    n = torch.Size(shape).numel()
    buf = torch.full((n + GUARD,), NAN, device="cuda", dtype=torch.float32)
    view = buf[:n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _bits(t):
    return t.contiguous().view(torch.int32)


def _slots(lib, case):
    P, dt, dv, D, nd = case
    name, off, n = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
    out, i = {}, 0
    while lib.grip_debug_upt_mixer_slot(P, nd, dt, dv, D, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(n)) == 0:
        out[name.value.decode()] = (off.value, n.value)
        i += 1
    return out


class _Run:
    """One forward and backward of a case on fresh buffers."""

    def __init__(self, case, inputs, hl):
        native, lib = _lib()
        self.case, self.lib, self.native = case, lib, native
        P, dt, dv, D, nd = case
        sh = M.shapes(case)
        self.inputs = inputs
        self.held = {n: _guarded(sh[n], t.cuda()) for n, t in inputs.items()}                               # operands and upstream gradients
        outs = ["coop_out", "vpt_out"] + (["deep_out", "g:deep"] if nd else []) + ["g:" + n for n in M.MIXER_TENSORS]
        self.held.update({n: _guarded(sh[n]) for n in outs})                                               # NaN-prefilled
        nbytes = ctypes.c_size_t()
        native.check(lib.grip_upt_mixer_deep_workspace(P, nd, dt, dv, D, ctypes.byref(nbytes)))
        assert nbytes.value % 4 == 0
        self.nbytes = nbytes.value
        self.ws = torch.full((nbytes.value // 4 + GUARD,), NAN, device="cuda", dtype=torch.float32)
        assert self.ws.data_ptr() % 256 == 0, "the hook's offsets count from the 256-byte-aligned base"
        self.slots = _slots(lib, case)
        self.owner = torch.zeros(self.ws.numel(), dtype=torch.bool, device="cuda")
        for off, n in self.slots.values():
            assert off + n <= nbytes.value // 4 - 64
            self.owner[off:off + n] = True
        ptr = lambda n: self.held[n][1].data_ptr()      # noqa: E731
        self.m = native.UptMixer(P, dt, dv, D, hl, 0, *[ptr(n) for n in M.MIXER_TENSORS])
        self.g = native.UptMixer(P, dt, dv, D, hl, 0, *[ptr("g:" + n) for n in M.MIXER_TENSORS])
        self.ptr = ptr

    def slot(self, name):
        off, n = self.slots[name]
        return self.ws[off:off + n]

    def forward(self):
        P, dt, dv, D, nd = self.case
        s, p, lib = torch.cuda.current_stream().cuda_stream, self.ptr, self.lib
        if nd:
            rc = lib.grip_upt_mixer_forward_deep(ctypes.byref(self.m), p("deep"), nd, p("coop_out"), p("vpt_out"), p("deep_out"), self.ws.data_ptr(), self.nbytes, s)
        else:
            rc = lib.grip_upt_mixer_forward(ctypes.byref(self.m), p("coop_out"), p("vpt_out"), self.ws.data_ptr(), self.nbytes, s)
        self.native.check(rc)
        torch.cuda.synchronize()

    def backward(self):
        P, dt, dv, D, nd = self.case
        s, p, lib = torch.cuda.current_stream().cuda_stream, self.ptr, self.lib
        if nd:
            rc = lib.grip_upt_mixer_backward_deep(ctypes.byref(self.m), p("deep"), nd, p("d_coop"), p("d_vpt"), p("d_deep"), ctypes.byref(self.g), p("g:deep"),
                                                  self.ws.data_ptr(), self.nbytes, s)
        else:
            rc = lib.grip_upt_mixer_backward(ctypes.byref(self.m), p("d_coop"), p("d_vpt"), ctypes.byref(self.g), self.ws.data_ptr(), self.nbytes, s)
        self.native.check(rc)
        torch.cuda.synchronize()

    def check_guards(self):
        assert torch.isnan(self.ws[~self.owner]).all(), "padding between the slots, or the guard behind the workspace, was written"
        for n, (buf, view) in self.held.items():
            assert torch.isnan(buf[view.numel():]).all(), f"{n}: the guard was written"
        for n, t in self.inputs.items():
            assert torch.equal(self.held[n][1].cpu(), t), f"{n}: an operand was written"

    def buffers(self):
        """float64 images of every buffer, shaped as mixer_ref.shapes names them."""
        sh = M.shapes(self.case)
        b = {n: view.double() for n, (_, view) in self.held.items()}
        b.update({n: self.slot(n).view(sh[n]).double() for n in self.slots})
        return b


def _id(case):
    return "-".join(str(v) for v in case)


@pytest.mark.parametrize("hl", (0, 1))
@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("case", M.CASES, ids=_id)
def test_every_launch_against_float64(case, family, hl):
    nd = case[4]
    inputs = M.make_inputs(case, family, hl)
    r = _Run(case, inputs, hl)
    fwd_slots = [n for n in M.FORWARD_SLOTS if n in r.slots]
    bwd_slots = [n for n in M.BACKWARD_SLOTS if n in r.slots]
    assert sorted(fwd_slots + bwd_slots) == sorted(r.slots) and all((n in r.slots) == (nd > 0) for n in M.DEEP_SLOTS)
    r.forward()
    for n in fwd_slots:
        assert torch.isfinite(r.slot(n)).all(), f"after the forward: {n} is not finite"
    for n in bwd_slots:
        assert torch.isnan(r.slot(n)).all(), f"the forward wrote the backward's {n}"
    assert all(torch.isnan(r.held[n][0]).all() for n in r.held if n.startswith("g:")), "the forward wrote a gradient buffer"
    r.check_guards()
    saved = {n: _bits(r.slot(n)).clone() for n in fwd_slots}
    r.backward()
    for n in r.slots:
        assert torch.isfinite(r.slot(n)).all(), f"after the backward: {n} is not finite"
    for n in fwd_slots:
        assert torch.equal(_bits(r.slot(n)), saved[n]), f"the backward changed the forward's {n}"
    r.check_guards()
    # every operation of every launch against float64 of the buffers it read
    b = r.buffers()
    worst, checked = {}, set()
    for step, _, fn in M.steps(case, hl):
        for name, (value, bound) in fn(b, None).items():
            base = name[:-4] if name.endswith("#f16") else name
            got = M.residual16(b[base]) if name.endswith("#f16") else b[base]
            assert got.shape == value.shape == bound.shape, (step, name)
            ratio = M.worst_ratio(got, value, bound)
            worst[step] = max(worst.get(step, 0.0), ratio)
            checked.add(base)
            print(f"{_id(case)} {family} hl{hl} {step:12s} {name:16s} worst |err| / bound {ratio:.4f}")
            assert ratio <= 1.0, (step, name, ratio)
    written = set(r.slots) | {n for n in r.held if n not in inputs}
    assert checked == written, checked ^ written
    if hl:      # the four fp16 rounding points of the fp16 Linears were among the checks
        for n in ("x0", "coop_out", "vpt_out", "d_x0", "g:coop", "g:vpt"):
            assert torch.equal(b[n], M.r16(b[n])), n
    _REPORT[f"{_id(case)} {family} hl{hl}"] = worst
    write_report("mixer_kernels.json", _REPORT)
    # no atomics: a second run on fresh buffers repeats every bit
    r2 = _Run(case, inputs, hl)
    r2.forward()
    r2.backward()
    assert torch.equal(_bits(r.ws), _bits(r2.ws)), "the workspace of a second run differs"
    for n, (buf, _) in r.held.items():
        assert torch.equal(_bits(buf), _bits(r2.held[n][0])), f"{n} of a second run differs"


def _untouched(r):
    return torch.isnan(r.ws).all() and all(torch.isnan(buf[view.numel():] if n in r.inputs else buf).all() for n, (buf, view) in r.held.items())


@pytest.mark.parametrize("nd", (0, 2))
def test_refusals_leave_every_buffer_untouched(nd):
    case = (4, 512, 768, 128, nd)
    r = _Run(case, M.make_inputs(case, "randn", 0), 0)
    native, lib, p, s = r.native, r.lib, r.ptr, torch.cuda.current_stream().cuda_stream
    ws = r.ws.data_ptr()

    def struct(src, **kw):
        t = native.UptMixer.from_buffer_copy(src)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def fwd(m, n_deep=nd, nbytes=r.nbytes):
        if nd:
            return lib.grip_upt_mixer_forward_deep(ctypes.byref(m), p("deep"), n_deep, p("coop_out"), p("vpt_out"), p("deep_out"), ws, nbytes, s)
        return lib.grip_upt_mixer_forward(ctypes.byref(m), p("coop_out"), p("vpt_out"), ws, nbytes, s)

    def bwd(m, g, n_deep=nd, nbytes=r.nbytes):
        if nd:
            return lib.grip_upt_mixer_backward_deep(ctypes.byref(m), p("deep"), n_deep, p("d_coop"), p("d_vpt"), p("d_deep"), ctypes.byref(g), p("g:deep"), ws, nbytes, s)
        return lib.grip_upt_mixer_backward(ctypes.byref(m), p("d_coop"), p("d_vpt"), ctypes.byref(g), ws, nbytes, s)

    bad = [(dict(text_width=63), b"widths 63 / 768 out of range"), (dict(vision_width=1281), b"widths 512 / 1281 out of range"),
           (dict(dim=100), b"dim = 100"), (dict(n_prompt=17), b"n_prompt = 17")]
    for kw, text in bad:
        assert fwd(struct(r.m, **kw)) == 1 and text in lib.grip_last_error(), kw
        assert bwd(struct(r.m, **kw), r.g) == 1 and text in lib.grip_last_error(), kw
    if nd:
        assert fwd(r.m, n_deep=32) == 1 and b"n_deep = 32 out of range" in lib.grip_last_error()
        assert bwd(r.m, r.g, n_deep=32) == 1 and b"n_deep = 32 out of range" in lib.grip_last_error()
    # at a 256-byte-aligned pointer the carve-up (its last slot padded to 64 floats) is all a call needs: one byte less is refused
    used = (max(off + n for off, n in r.slots.values()) + 63) // 64 * 64 * 4
    assert used == r.nbytes - 256
    assert fwd(r.m, nbytes=used - 1) == 1 and b"workspace too small" in lib.grip_last_error()
    assert bwd(r.m, r.g, nbytes=used - 1) == 1 and b"workspace too small" in lib.grip_last_error()
    assert bwd(r.m, struct(r.g, fc_b=None)) == 1 and b"every gradient buffer must be given" in lib.grip_last_error()
    assert bwd(r.m, struct(r.g, coop=None)) == 1 and b"every gradient buffer must be given" in lib.grip_last_error()
    torch.cuda.synchronize()
    assert _untouched(r), "a refused call wrote a buffer"
    r.check_guards()
