"""Every launch of a tower pass (csrc/tower.hip) element-wise against float64 ("Tower pass tests").

The test builds its own small towers through the C ABI (grip_layout_size / grip_layout_slot, blobs filled from grip_amd.rng, grip_tower_create,
grip_tower_finalize) and runs a pass of K launches K times with launch budgets 1 .. K (grip_debug_launch_budget) on the same inputs, the workspace, its
guard and the output filled with 0xFF bytes (a NaN in f16 and in f32) before each run.  After run k, on every element:
  1. what launch k owns is finite and within the bound of tests/tower_ref.py evaluated in float64 on the buffers as they stood after run k - 1 (bit-equal
     where the stage is exact);
  2. every other byte of the workspace, of the guard behind it and of the output has the bits it had after run k - 1 -- other slots, the padding
     between slots, rows M .. Mp, bytes never written (still 0xFF);
  3. the budget's message names launch k + 1 as tower_ref.steps expects it: the schedule itself is asserted.
The unbudgeted pass then repeats the last run bit for bit, and so does a pass on fresh buffers.  The worst |err| / bound per launch label and case goes
to tests/_out/tower_passes.json.

test_every_backward_launch_against_float64 does the same for the backward of each train-mode forward (grip_vit_backward_prefix / _deep,
grip_text_backward_prefix / _deep), the forward re-run before each budgeted backward.

Covered: the inference passes of the f16 towers, of the exact (f32) tower and of the split-f16 tower (w_exact 0 and 1), and the train-mode forwards of the f16 towers (tower_ref.CASES).  The buffers are addressed by name through grip_debug_tower_slot."""
import ctypes
import re

import pytest
import torch

import tower_ref as T
from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 4096          # bytes behind the workspace and behind the output
_REPORT = {}
_TOWERS = {}


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


class Tower:
    """A finalized tower of the pass's dims on blobs of the test's own; .w = {"w:" + slot name: CPU tensor [rows, ld]} read back after finalize."""

    def __init__(self, p, family):
        native, lib = _lib()
        self.native, self.lib = native, lib
        dims = native.Dims(p.kind, p.d, p.layers, p.H, p.E, p.seq0, p.patch if p.kind == 0 else 0, p.resolution if p.kind == 0 else 0, p.vocab, 4, p.precision)
        n16, n32 = ctypes.c_int64(), ctypes.c_int64()
        native.check(lib.grip_layout_size(ctypes.byref(dims), ctypes.byref(n16), ctypes.byref(n32)))
        self.b16 = torch.zeros(n16.value, dtype=torch.float32 if p.f32 else torch.float16, device="cuda")      # (an exact tower's operand blob holds f32 elements)
        self.b32 = torch.zeros(n32.value, dtype=torch.float32, device="cuda")
        w = T.make_weights(p, family)
        slots, s, i = [], native.Slot(), 0
        while lib.grip_layout_slot(ctypes.byref(dims), i, ctypes.byref(s)) == 0:
            slots.append((s.name.decode(), s.dtype, s.derived, s.offset, s.rows, s.cols, s.ld))
            i += 1
        assert {n for n, _, der, *_ in slots if not der} == set(w), "tower_ref.weight_shapes names the primary slots of the layout"
        for name, dt, der, off, rows, cols, ld in slots:
            if not der:
                blob = self.b16 if dt == 0 else self.b32
                blob[off:off + rows * ld].view(rows, ld)[:, :cols] = w[name][:, :cols].to(blob.dtype).cuda()
        self.handle = ctypes.c_void_p()
        native.check(lib.grip_tower_create(ctypes.byref(dims), self.b16.data_ptr(), self.b32.data_ptr(), ctypes.byref(self.handle)))
        native.check(lib.grip_tower_finalize(self.handle, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        c16, c32 = self.b16.cpu(), self.b32.cpu()
        self.w = {"w:" + name: (c16 if dt == 0 else c32)[off:off + rows * ld].view(rows, ld) for name, dt, der, off, rows, cols, ld in slots}
        self.blob_bits = (self.b16.view(torch.int32 if p.f32 else torch.int16).clone(), self.b32.view(torch.int32).clone())

    def weights_untouched(self):
        return torch.equal(self.b16.view(self.blob_bits[0].dtype), self.blob_bits[0]) and torch.equal(self.b32.view(torch.int32), self.blob_bits[1])


def _tower(p, family):
    key = (p.kind, p.d, p.layers, p.E, p.precision, p.w_grid, family)
    if key not in _TOWERS:
        _TOWERS[key] = Tower(p, family)
    return _TOWERS[key]


class Run:
    """The buffers of one pass: workspace + guard and output + guard, 0xFF-filled; the inputs on the device."""

    def __init__(self, p, tower):
        self.p, self.t = p, tower
        native, lib = tower.native, tower.lib
        self.flags = (native.FWD_STREAM_HILO if p.hilo else 0) | (native.FWD_NO_POS_EMB if p.no_pos else 0) | \
            (native.FWD_PER_IMAGE_PREFIX if p.per_image else 0) | (native.FWD_SHARED_PREFIX if p.Ps else 0) | (native.FWD_TRAIN if p.train else 0)
        train = 1 if p.train else 0
        nbytes = ctypes.c_size_t()
        native.check(lib.grip_workspace_bytes(tower.handle, p.B, p.P, p.S if p.kind else 0, train, ctypes.byref(nbytes)))
        self.nbytes = nbytes.value
        self.ws = torch.empty(self.nbytes + GUARD, dtype=torch.uint8, device="cuda")
        self.out = torch.empty(p.B * p.E * 4 + GUARD, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0 and self.out.data_ptr() % 256 == 0
        # the backward's outputs (train mode), each followed by a guard: grad_prefix [prefix sets, P, d], grad_deep [n_deep, deep sets, P, d]
        sets = (p.B if p.per_image else 1) if p.kind == 0 else p.prefix_classes
        self.grad_bytes = {"out:grad_prefix": sets * p.P * p.d * 4, "out:grad_deep": p.n_deep * (p.prefix_classes if p.kind else 1) * p.P * p.d * 4} if p.train else {}
        self.grads = {n: torch.empty(nb + GUARD, dtype=torch.uint8, device="cuda") for n, nb in self.grad_bytes.items()}
        self.inputs = T.make_inputs(p)
        self.dev = {k: v.cuda() for k, v in self.inputs.items()}
        # the carve-up by name
        self.slots = {}
        name, layer, off, n, i = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), 0
        while lib.grip_debug_tower_slot(tower.handle, p.B, p.P, p.S if p.kind else 0, train, 1 if p.Ps else 0, i, ctypes.byref(name), ctypes.byref(layer),
                                        ctypes.byref(off), ctypes.byref(n)) == 0:
            assert off.value % 256 == 0 and off.value + n.value <= self.nbytes
            self.slots[name.value.decode() + (f".{layer.value}" if layer.value >= 0 else "")] = (off.value, n.value)          # per-layer slots: "<name>.<layer>"
            i += 1
        spans = sorted(v for k, v in self.slots.items() if k != "patches")
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])), "overlapping slots"
        if p.kind == 0:
            assert self.slots["patches"][0] == self.slots["h"][0] and self.slots["patches"][1] <= self.slots["h"][1], "patches is reported as an alias of h"

    def fill(self):
        self.ws.fill_(0xFF)
        self.out.fill_(0xFF)
        for g in self.grads.values():
            g.fill_(0xFF)

    def backward(self, budget):
        """The backward entry point that belongs to the forward: _prefix without deep prompts, _deep with them."""
        p, lib, d = self.p, self.t.lib, self.dev
        s = torch.cuda.current_stream().cuda_stream
        gp, gd = self.grads["out:grad_prefix"].data_ptr(), self.grads["out:grad_deep"].data_ptr()
        if budget is not None:
            assert lib.grip_debug_launch_budget(budget) == 0
        if p.kind == 0 and p.n_deep:
            rc = lib.grip_vit_backward_deep(self.t.handle, d["in:grad_emb"].data_ptr(), d["in:prefix"].data_ptr(), gp, gd, self.ws.data_ptr(), self.nbytes, 0, s)
        elif p.kind == 0:
            rc = lib.grip_vit_backward_prefix(self.t.handle, d["in:grad_emb"].data_ptr(), d["in:prefix"].data_ptr(), gp, self.ws.data_ptr(), self.nbytes, 0, s)
        elif p.n_deep:
            rc = lib.grip_text_backward_deep(self.t.handle, d["in:grad_emb"].data_ptr(), gp, gd, self.ws.data_ptr(), self.nbytes, 0, s)
        else:
            rc = lib.grip_text_backward_prefix(self.t.handle, d["in:grad_emb"].data_ptr(), gp, self.ws.data_ptr(), self.nbytes, 0, s)
        msg = lib.grip_last_error().decode()
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a GPU fault: nothing more is started on the card in this session
            pytest.exit(f"{p.key()}: the GPU faulted in the backward after budget {budget} ({e}); last error: {msg}", returncode=3)
        if rc == 2:
            pytest.exit(f"{p.key()}: HIP error in the backward at budget {budget}: {msg}", returncode=3)
        return rc, msg

    def image_all(self):
        """{name: CPU bytes} of the workspace + guard, the embeddings + guard and every gradient output + guard."""
        img = {"ws": self.ws.cpu(), "out:emb": self.out.cpu()}
        img.update({n: g.cpu() for n, g in self.grads.items()})
        return img

    def buffers_all(self, img):
        b = self.buffers((img["ws"], img["out:emb"]))
        for n, nb in self.grad_bytes.items():
            b[n] = img[n][:nb].view(torch.float32)
        return b

    def owned_all(self, regions):
        """{name: byte mask} of the regions, over the same buffers as image_all."""
        m = {n: torch.zeros(t.numel(), dtype=torch.uint8) for n, t in [("ws", self.ws), ("out:emb", self.out)] + list(self.grads.items())}
        for r in regions:
            if r.slot.startswith("out:"):
                flat = m[r.slot][:self.grad_bytes.get(r.slot, self.p.B * self.p.E * 4)].view(torch.int32)
            else:
                off, n = self.slots[r.slot]
                flat = m["ws"][off:off + n].view(torch.int16 if self.p.is16(r.slot) else torch.int32)
            assert (r.row0 + r.rows) * r.ld <= flat.numel(), (r, "the region does not fit its slot")
            flat[r.row0 * r.ld:(r.row0 + r.rows) * r.ld].view(r.rows, r.ld)[:, r.col0:r.col0 + r.ncols] = -1
        return {n: t.bool() for n, t in m.items()}

    def forward(self, budget):
        p, lib, d = self.p, self.t.lib, self.dev
        ptr = lambda k: d[k].data_ptr() if k in d else None          # noqa: E731
        s = torch.cuda.current_stream().cuda_stream
        if budget is not None:
            assert lib.grip_debug_launch_budget(budget) == 0
        if p.kind == 0:
            rc = lib.grip_vit_forward_deep(self.t.handle, ptr("in:images"), 0, ptr("in:prefix"), p.P, ptr("in:deep"), p.n_deep, p.B, self.out.data_ptr(),
                                           self.ws.data_ptr(), self.nbytes, self.flags, None, s)
        else:
            rc = lib.grip_text_forward_deep(self.t.handle, ptr("in:ids"), ptr("in:eot"), ptr("in:prefix"), p.P, p.prefix_classes, ptr("in:deep"), p.n_deep,
                                            p.B, p.S, self.out.data_ptr(), self.ws.data_ptr(), self.nbytes, self.flags, None, s)
        msg = lib.grip_last_error().decode()
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a GPU fault: nothing more is started on the card in this session
            pytest.exit(f"{p.key()}: the GPU faulted after budget {budget} ({e}); last error: {msg}", returncode=3)
        if rc == 2:                        # GRIP_ERR_HIP
            pytest.exit(f"{p.key()}: HIP error at budget {budget}: {msg}", returncode=3)
        return rc, msg

    def image(self):
        """(workspace + guard, output + guard) as CPU bytes."""
        return self.ws.cpu(), self.out.cpu()

    def buffers(self, image):
        """The buffer set tower_ref reads, as typed flat views of a CPU image."""
        ws, out = image
        b = dict(self.t.w)
        b.update(self.inputs)
        for name, (off, n) in self.slots.items():
            b[name] = ws[off:off + n].view(torch.float16 if self.p.is16(name) else torch.float32)
        b["out:emb"] = out[:self.p.B * self.p.E * 4].view(torch.float32)
        return b

    def owned(self, regions):
        """Byte masks (workspace + guard, output + guard) of the regions."""
        mw, mo = torch.zeros(self.ws.numel(), dtype=torch.uint8), torch.zeros(self.out.numel(), dtype=torch.uint8)
        for r in regions:
            if r.slot == "out:emb":
                flat = mo[:self.p.B * self.p.E * 4].view(torch.int32)
            else:
                off, n = self.slots[r.slot]
                flat = mw[off:off + n].view(torch.int16 if self.p.is16(r.slot) else torch.int32)
            assert (r.row0 + r.rows) * r.ld <= flat.numel(), (r, "the region does not fit its slot")
            flat[r.row0 * r.ld:(r.row0 + r.rows) * r.ld].view(r.rows, r.ld)[:, r.col0:r.col0 + r.ncols] = -1
        return mw.bool(), mo.bool()


MSG = re.compile(r"launch budget: stopped after (\d+) launches, before (.*)$")


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("p", T.CASES, ids=[p.key() for p in T.CASES])
def test_every_launch_against_float64(p, family):
    tower = _tower(p, family)
    native = tower.native
    sched = T.steps(p)
    K = len(sched)
    run = Run(p, tower)
    if p.kind == 1 and p.train:
        assert tower.lib.grip_debug_coop_split(p.M, p.d, 4 * p.d) == p.coop_ks, "the cooperative split-K factor the case was written for"
    for r in {r.slot for s in sched for r in s.owns} - {"out:emb"}:
        assert r in run.slots, f"the carve has no slot {r}"
    prev = (torch.full((run.ws.numel(),), 0xFF, dtype=torch.uint8), torch.full((run.out.numel(),), 0xFF, dtype=torch.uint8))
    worst = {}
    for k in range(1, K + 1):
        step = sched[k - 1]
        run.fill()
        rc, msg = run.forward(k)
        # 3. the schedule: stopped before launch k + 1, which is the call tower_ref expects; the last budget lets the pass finish
        if k < K:
            m = MSG.match(msg)
            assert rc == native.ERR_LAUNCH_BUDGET and m, (step.label, rc, msg)
            assert int(m.group(1)) == k and m.group(2).startswith(sched[k].call), f"after {step.label}: expected {sched[k].label} = {sched[k].call}..., got: {msg}"
        else:
            assert rc == 0, (step.label, rc, msg)
        cur = run.image()
        before, after = run.buffers(prev), run.buffers(cur)
        # 1. what the launch owns
        for name, (got, value, bound) in step.ref(before, after).items():
            assert got.shape == value.shape == bound.shape, (step.label, name)
            assert torch.isfinite(got.double()).all(), f"{step.label} {name}: an owned element is not finite"
            ratio = T.worst_ratio(got, value, bound)
            worst[step.label] = max(worst.get(step.label, 0.0), ratio)
            print(f"{p.key()} {family} {step.label:20s} {name:10s} worst |err| / bound {ratio:.4f}")
            assert ratio <= 1.0, (p.key(), family, step.label, name, ratio)
        if step.exact is not None:
            for region, want in step.exact(before).items():
                assert T.same_bits(T.view(after, region), want), f"{step.label}: {region.slot} is not the exact result"
        for region in step.owns:
            if region.slot == "coop_scratch" or p.split_layout(region):      # scratch tiles not all written; f16 pairs read as f32 (decoded in `got` above)
                continue
            assert torch.isfinite(T.view(after, region).double()).all(), f"{step.label}: {region.slot} holds a non-finite element"
        # 2. everything else keeps its bits
        for what, mask, a, b in zip(("workspace", "output"), run.owned(step.owns), cur, prev):
            changed = (a != b) & ~mask
            assert not changed.any(), f"{step.label}: wrote {what} byte {int(changed.nonzero()[0])} outside what it owns ({_where(run, int(changed.nonzero()[0])) if what == 'workspace' else ''})"
        prev = cur
    assert tower.weights_untouched(), "a pass wrote the weight blobs"
    if p.split:          # the weights chose the GEMM form the case was written for: the two-pass kernel on f16-grid weights (w_exact), else the a_hi w_lo product
        assert tower.lib.grip_debug_split_last_wlo() == (0 if p.w_grid else 1), "w_exact did not take the intended value"
    assert set(worst) == {s.label for s in sched}
    _REPORT[f"{p.key()} {family}"] = {k: round(v, 4) for k, v in worst.items()}
    write_report("tower_passes.json", _REPORT)
    # the unbudgeted pass repeats the last run bit for bit (the budget switched itself off), and so does a pass on fresh buffers
    run.fill()
    rc, msg = run.forward(None)
    assert rc == 0, msg
    again = run.image()
    assert torch.equal(again[0], prev[0]) and torch.equal(again[1], prev[1]), "the unbudgeted pass differs from the last budgeted run"
    fresh = Run(p, tower)
    fresh.fill()
    rc, msg = fresh.forward(None)
    assert rc == 0, msg
    again = fresh.image()
    assert torch.equal(again[0], prev[0]) and torch.equal(again[1], prev[1]), "a second pass on fresh buffers differs"


TRAIN = [p for p in T.CASES if p.train]


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("p", TRAIN, ids=[p.key() for p in TRAIN])
def test_every_backward_launch_against_float64(p, family):
    """The backward of a train-mode forward, the same way: for k = 1 .. K the forward is run again (unbudgeted) on 0xFF-filled buffers, then the backward
    with budget k.  Launch k is held to float64 of the forward's saved slots and the backward's scratch as they stood after run k - 1; every other byte --
    the forward's slots among them, through the whole backward -- keeps its bits."""
    tower = _tower(p, family)
    native, lib = tower.native, tower.lib
    sched = T.backward_steps(p)
    K = len(sched)
    run = Run(p, tower)
    # the split-K factors the schedule assumes are the ones the carve-up reserved partial buffers for
    Mp, Bp = (p.M + 255) // 256 * 256, (p.B + 255) // 256 * 256
    assert run.slots["dln"][1] == Mp * p.d * 4 * max(T.pick_ksplit(p.M, p.d, 4 * p.d), T.pick_ksplit(p.M, p.d, 3 * p.d))
    if "row_dln" in run.slots:
        assert p.rows_only and run.slots["row_dln"][1] == Bp * p.d * 4 * T.pick_ksplit(p.B, p.d, 4 * p.d)
    for r in {r.slot for s in sched for r in s.owns if not r.slot.startswith("out:")}:
        assert r in run.slots, f"the carve has no slot {r}"
    run.fill()
    rc, msg = run.forward(None)
    assert rc == 0, msg
    prev = run.image_all()
    worst = {}
    for k in range(1, K + 1):
        step = sched[k - 1]
        run.fill()
        rc, msg = run.forward(None)
        assert rc == 0, msg
        if k == 1:
            fwd = run.image_all()
            assert all(torch.equal(fwd[n], prev[n]) for n in fwd), "the forward does not repeat its bits"
        rc, msg = run.backward(k)
        if k < K:
            m = MSG.match(msg)
            assert rc == native.ERR_LAUNCH_BUDGET and m, (step.label, rc, msg)
            assert int(m.group(1)) == k and m.group(2).startswith(sched[k].call), f"after {step.label}: expected {sched[k].label} = {sched[k].call}..., got: {msg}"
            rc2, msg2 = run.backward(None)          # a backward stopped early has consumed its forward
            assert rc2 == 4 and "already been back-propagated" in msg2, (rc2, msg2)
        else:
            assert rc == 0, (step.label, rc, msg)
        cur = run.image_all()
        before, after = run.buffers_all(prev), run.buffers_all(cur)
        for name, (got, value, bound) in step.ref(before, after).items():
            assert got.shape == value.shape == bound.shape, (step.label, name)
            assert torch.isfinite(got.double()).all(), f"{step.label} {name}: an owned element is not finite"
            ratio = T.worst_ratio(got, value, bound)
            worst[step.label] = max(worst.get(step.label, 0.0), ratio)
            print(f"{p.key()} {family} {step.label:24s} {name:20s} worst |err| / bound {ratio:.4f}")
            assert ratio <= 1.0, (p.key(), family, step.label, name, ratio)
        if step.exact is not None:
            for region, want in step.exact(before).items():
                assert T.same_bits(T.view(after, region), want), f"{step.label}: {region.slot} is not the exact result"
        for region in step.owns:
            if region.slot == "kv_part":          # per-sequence shares of the shared keys' dK / dV: the kernel's own scratch
                continue
            assert torch.isfinite(T.view(after, region).double()).all(), f"{step.label}: {region.slot} holds a non-finite element"
        masks = run.owned_all(step.owns)
        for n in cur:
            changed = (cur[n] != prev[n]) & ~masks[n]
            assert not changed.any(), f"{step.label}: wrote byte {int(changed.nonzero()[0])} of {n} outside what it owns ({_where(run, int(changed.nonzero()[0])) if n == 'ws' else ''})"
        prev = cur
    assert tower.weights_untouched(), "a pass wrote the weight blobs"
    assert set(worst) == {s.label for s in sched}
    _REPORT[f"{p.key()} {family} backward"] = {k: round(v, 4) for k, v in worst.items()}
    write_report("tower_passes.json", _REPORT)
    # the unbudgeted backward repeats the last run bit for bit, on these buffers and on fresh ones
    for r in (run, Run(p, tower)):
        r.fill()
        rc, msg = r.forward(None)
        assert rc == 0, msg
        rc, msg = r.backward(None)
        assert rc == 0, msg
        again = r.image_all()
        assert all(torch.equal(again[n], prev[n]) for n in prev), "an unbudgeted forward + backward differs from the last budgeted run"


def _where(run, byte):
    for name, (off, n) in run.slots.items():
        if off <= byte < off + n:
            return f"{name} + {byte - off}"
    return "padding between slots" if byte < run.nbytes else "the guard behind the workspace"


def test_budget_refusals_and_switch_off():
    p = T.CASES[1]
    tower = _tower(p, "randn")
    run, K = Run(p, tower), len(T.steps(p))
    run.fill()
    rc, msg = run.forward(None)
    assert rc == 0, msg
    full = run.image()
    for budget in (0, -3, K + 5):          # off, off, larger than the pass: it finishes
        run.fill()
        rc, msg = run.forward(budget)
        assert rc == 0, (budget, msg)
        got = run.image()
        assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1]), budget
        run.fill()
        rc, msg = run.forward(None)          # ... and left no budget behind
        assert rc == 0, (budget, msg)
    run.fill()
    rc, msg = run.forward(2)
    assert rc == tower.native.ERR_LAUNCH_BUDGET and MSG.match(msg)
    run.fill()
    rc, msg = run.forward(None)              # a tripped budget is off
    assert rc == 0, msg
    got = run.image()
    assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
