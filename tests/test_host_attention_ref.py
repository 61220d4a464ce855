"""CPU: the float64 attention reference of the GPU kernel tests (tests/attention_ref.py) against torch autograd in float64, its one-row and
shared-prefix forms against the plain form, and the properties of the input families that the element-wise bounds rely on."""
import pytest
import torch

import attention_ref as AR


def _autograd(qkv, d_out, B, S, H, causal):
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / 8.0
    if causal:
        s = s + torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    out = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * 64)
    out.backward(d_out.double())
    D = H * 64
    return out.detach(), x.grad[:, :D], x.grad[:, D:2 * D], x.grad[:, 2 * D:]


@pytest.mark.parametrize("family", AR.FAMILIES)
@pytest.mark.parametrize("B,S,H,causal", [(2, 1, 1, 0), (2, 1, 2, 1), (3, 17, 2, 0), (2, 33, 2, 1), (2, 77, 1, 1), (1, 97, 2, 0)])
def test_closed_form_equals_autograd(family, B, S, H, causal):
    qkv, d_out = AR.make_inputs(family, B, S, H, causal, seed=S)
    res = AR.attention(qkv, B, S, H, causal, d_out)
    for got, want in zip((res["out"], res["dq"], res["dk"], res["dv"]), _autograd(qkv, d_out, B, S, H, causal)):
        torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9 * max(want.abs().max().item(), 1.0))
    # the sums of absolute terms dominate the values they bound
    for v, s in (("out", "scale_o"), ("dq", "scale_q"), ("dk", "scale_k"), ("dv", "scale_v")):
        assert (res[v].abs() <= res[s] * (1 + 1e-12) + 1e-300).all()


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("index", ["null", "zero", "last", "mixed"])
def test_one_row_form_equals_the_plain_form(causal, index):
    B, S, H = 4, 37, 2
    D = H * 64
    qkv, d_out = AR.make_inputs("randn", B, S, H, causal, seed=5)
    r = {"null": None, "zero": torch.zeros(B, dtype=torch.int32), "last": torch.full((B,), S - 1, dtype=torch.int32),
         "mixed": torch.tensor([0, S - 1, 7, 32], dtype=torch.int32)}[index]
    rr = torch.zeros(B, dtype=torch.long) if r is None else r.long()
    at = torch.arange(B) * S + rr
    masked = torch.zeros_like(d_out)
    masked[at] = d_out[at]
    full = AR.attention(qkv, B, S, H, causal, masked)
    row = AR.attention_row(qkv, B, S, H, causal, r, None, d_out[at])
    torch.testing.assert_close(row["out"], full["out"][at], rtol=1e-12, atol=1e-12)
    for n in ("dq", "dk", "dv", "scale_q", "scale_k", "scale_v", "scale2_q", "scale2_k"):
        torch.testing.assert_close(row[n], full[n], rtol=1e-10, atol=1e-12)
    other = torch.ones(B * S, dtype=torch.bool)
    other[at] = False
    assert (row["dq"][other] == 0).all()
    if causal:
        after = (torch.arange(S)[None, :] > rr[:, None]).reshape(-1)
        assert (row["dk"][after] == 0).all() and (row["dv"][after] == 0).all()
    # the compact query rows replace the packed ones
    qrows = torch.randn(B, D, generator=torch.Generator().manual_seed(1)).half()
    sub = qkv.clone()
    sub[at, :D] = qrows
    torch.testing.assert_close(AR.attention_row(qkv, B, S, H, causal, r, qrows)["out"], AR.attention(sub, B, S, H, causal)["out"][at], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,S,Ps", [(2, 9, 1), (3, 21, 5), (9, 40, 16), (5, 77, 17)])
def test_shared_layout_equals_the_plain_layout_on_identical_prefixes(B, S, Ps):
    H = 2
    qkv, d_out = AR.make_inputs("randn", B, S, H, 1, seed=Ps)
    qkv_s, d_out_s = AR.to_shared(qkv, B, S, Ps), AR.to_shared(d_out, B, S, Ps)
    assert qkv_s.shape[0] == Ps + B * (S - Ps)
    plain_qkv = AR.from_shared(qkv_s, B, S, Ps)          # the first Ps rows identical across sequences
    assert torch.equal(AR.to_shared(plain_qkv, B, S, Ps), qkv_s)
    plain_do = AR.from_shared(d_out_s, B, S, Ps).reshape(B, S, -1).clone()
    plain_do[1:, :Ps] = 0
    plain = AR.attention(plain_qkv, B, S, H, 1, plain_do.reshape(B * S, -1))
    sh = AR.attention_shared(qkv_s, B, S, H, Ps, d_out_s)
    # every sequence's copy of a shared output row is the same row
    o3 = plain["out"].reshape(B, S, -1)
    assert all(torch.equal(o3[b, :Ps], o3[0, :Ps]) for b in range(B))
    torch.testing.assert_close(AR.from_shared(sh["out"], B, S, Ps), plain["out"], rtol=0, atol=0)
    for n in ("dq", "dk", "dv"):
        p3 = plain[n].reshape(B, S, -1)
        torch.testing.assert_close(sh[n][Ps:], p3[:, Ps:].reshape(B * (S - Ps), -1), rtol=0, atol=0)
        torch.testing.assert_close(sh[n][:Ps], p3[:, :Ps].sum(0), rtol=1e-12, atol=1e-12)
    assert (plain["dq"].reshape(B, S, -1)[1:, :Ps] == 0).all()


@pytest.mark.parametrize("S,causal", [(1, 0), (1, 1), (2, 1), (16, 0), (33, 1), (77, 1), (97, 0), (209, 0), (289, 1)])
def test_peaked_family_is_peaked_and_keeps_every_sum_nonzero(S, causal):
    B, H = 2, 2
    qkv, d_out = AR.make_inputs("peaked", B, S, H, causal, seed=S)
    assert torch.isfinite(qkv.float()).all()
    q, k, v = AR.unpack(qkv, B, S, H)
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
    if S >= 64:
        finite = s[torch.isfinite(s)]
        assert finite.max() - finite.min() >= 20.0           # tens of units
        i = torch.arange(0, S, 2)                            # even rows: the dominant key is the last visible one
        want = i if causal else torch.full_like(i, S - 1)
        assert (s[:, :, i].argmax(-1) == want).double().mean() >= 0.9
    res = AR.attention(qkv, B, S, H, causal, d_out)
    assert res["A"] <= 128.0
    assert (res["scale_o"] > 0).all() and (res["scale_v"] > 0).all()
    for what, kind in (("o", "fwd_mfma"), ("q", "bwd_mfma"), ("k", "bwd_mfma"), ("v", "bwd_mfma")):
        assert (AR.bound(res, what, kind) > 0).all()
    if S >= 2:
        assert (res["scale_k"] > 0).all()
        rows_with_two_keys = torch.ones(B, S, dtype=torch.bool)
        if causal:
            rows_with_two_keys[:, 0] = False                 # one visible key: p = 1 and dS = 0 identically
        assert (res["scale_q"][rows_with_two_keys.reshape(-1)] > 0).all()
