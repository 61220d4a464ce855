"""The attention kernels of the f32 tier (attn_fwd_f32_kernel, f32 and split-layout output) and of the split-f16 tier (attn_fwd_split_kernel: its ten KVC
instantiations x causal, four or eight waves), element by element against float64 ("Tier kernel tests").

References and bounds are tests/tier_ref.py's (attention_ref's float64 attention; derived bounds, nothing measured).  qkv is followed by 32 NaN rows, the
output is NaN-prefilled and 32 rows longer.  Every owned element must come back finite and within the bound, the guard rows untouched, no element left
out; a sequence's bits depend on neither the batch size nor its index.  The worst |err| / bound of every case goes to
tests/_out/tier_attention_kernels.json."""
import ctypes

import pytest
import torch

import tier_ref as T
from conftest import write_report

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 32
B, H = 2, 2
REPORT = {}
VISITED = set()
S_F32 = (1, 31, 32, 33, 255, 256, 257, 513)
S_SPLIT = (1, 15, 16, 17, 32, 33, 64, 96, 97, 128, 129, 160, 192, 197, 224, 256, 257, 288, 320)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """A HIP error after a launch ends the session: nothing more is started on a GPU that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a tier attention launch, stopping: %s" % e, returncode=3)


def launch(kind, qkv, nb, S, causal):
    """kind: "f32" (f32 output), "f32_split" (attn_fwd_f32_kernel writing the split layout), "split" (attn_fwd_split_kernel).
    -> (float64 [nb S, D] values, the owned part of the buffer as stored); guards and finiteness asserted."""
    native, lib = _lib()
    D = H * 64
    rows = nb * S
    qin = torch.cat([qkv, torch.full((GUARD, 3 * D), NAN, device="cuda")])
    if kind == "f32":
        out = torch.full((rows + GUARD, D), NAN, device="cuda")
        native.check(lib.grip_debug_attention_exact(_p(qin), _p(out), nb, S, H, causal, _stream()))
        VISITED.add(("attn_fwd_f32_kernel", "f32 out", causal))
    else:
        out = torch.full((rows + GUARD, 2 * D), NAN, dtype=torch.float16, device="cuda")
        native.check(lib.grip_debug_attention_split(_p(qin), _p(out), nb, S, H, causal, 1 if kind == "split" else 0, _stream()))
        if kind == "split":
            kvc = (S + 31) // 32
            VISITED.add(("attn_fwd_split_kernel", kvc, 8 if kvc >= 4 else 4, causal))
        else:
            VISITED.add(("attn_fwd_f32_kernel", "split out", causal))
    _sync()
    assert bool(torch.isnan(out[rows:]).all()), (kind, "guard touched")
    own = out[:rows]
    assert bool(torch.isfinite(own).all()), (kind, "owned element not finite")
    if kind == "f32":
        return own.double(), own
    hi, lo = T.from_layout(own, rows, D)
    return hi.double() + lo.double(), own


def bound_of(kind, res):
    return T.bound_attention_split(res) if kind == "split" else T.bound_attention_f32(res, split_out=(kind == "f32_split"))


def run_cases(kinds, S, causal, name):
    rows, failures = {}, []
    for family in T.ATT_FAMILIES:
        qkv = T.make_attention_inputs(family, B, S, H, causal, 31 * S + causal, device="cuda")
        res = T.attention_terms(qkv, B, S, H, causal)
        got = {}
        for kind in kinds:
            cid = "%s-S%d-c%d-%s" % (kind, S, causal, family)
            try:
                got[kind], _ = launch(kind, qkv, B, S, causal)
                w = ((got[kind] - res["out"]).abs() / bound_of(kind, res)).max().item()
                rows[cid] = dict(family=family, worst=w)
                if not w <= 1.0:
                    failures.append((cid, w))
            except AssertionError as e:
                failures.append((cid, str(e)[:300]))
        if "split" in got and "f32_split" in got:      # the two kernels of the tier agree to the sum of their bounds
            d = ((got["split"] - got["f32_split"]).abs() / (bound_of("split", res) + bound_of("f32_split", res))).max().item()
            if not d <= 1.0:
                failures.append(("split vs f32_split S%d c%d %s" % (S, causal, family), d))
    REPORT.update(rows)
    write_report(name, REPORT)
    print(kinds, S, causal, "worst |err| / bound:", {k: max(r["worst"] for c, r in rows.items() if c.startswith(k + "-")) for k in kinds})
    assert not failures, failures[:8]


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S", S_F32)
def test_the_f32_kernel_matches_float64(S, causal):
    run_cases(("f32", "f32_split"), S, causal, "tier_attention_kernels.json")


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S", S_SPLIT)
def test_the_split_kernel_matches_float64_and_the_f32_kernel(S, causal):
    run_cases(("split", "f32_split"), S, causal, "tier_attention_kernels.json")


@pytest.mark.parametrize("kind,S", [("f32", 33), ("f32", 257), ("f32_split", 257), ("split", 17), ("split", 97), ("split", 197), ("split", 320)])
def test_a_sequences_bits_depend_on_neither_the_batch_nor_its_index(kind, S):
    D = H * 64
    for causal in (0, 1):
        qkv = T.make_attention_inputs("randn", 3, S, H, causal, 7 * S + causal, device="cuda")
        _, a = launch(kind, qkv, 3, S, causal)
        _, a2 = launch(kind, qkv, 3, S, causal)
        _, b = launch(kind, qkv[2 * S:].contiguous(), 1, S, causal)
        assert torch.equal(a.view(torch.int16), a2.view(torch.int16)), "two identical launches differ"
        assert torch.equal(a[2 * S:].view(torch.int16), b.view(torch.int16)), (kind, S, causal)


def test_every_instantiation_named_was_reached():
    want = {("attn_fwd_f32_kernel", o, c) for o in ("f32 out", "split out") for c in (0, 1)}
    want |= {("attn_fwd_split_kernel", k, 8 if k >= 4 else 4, c) for k in range(1, 11) for c in (0, 1)}
    assert VISITED == want, VISITED ^ want
