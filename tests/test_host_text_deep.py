"""CPU: the host side of deep text prompts (deep CoOp): the two ABI additions are declared and exported, the engine's shape rules, the textual
strategies' initialisation (the shallow context is drawn first and stays bit-identical with COOP_DEEP), and the block-by-block restatement of
the oracle's text forward that tests/test_gpu_text_deep.py measures the GPU against."""
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_text_deep_forward(clip_model, token_ids, class_embeddings, deep=None, enable_pos_emb=True):
    """oracle/wrappers.py:text_forward with the transformer run block by block (its own causal attn_mask) and positions 1 .. P of every class
    replaced before blocks 1 .. D.  deep: None, [D, P, d] / [D, 1, P, d] (one context for every class) or [D, C, P, d]."""
    x = clip_model.token_embedding(token_ids.long())
    P = class_embeddings[0].size(0)
    x = x.clone()
    x[:, 1:P + 1, :] = class_embeddings
    if enable_pos_emb:
        x = x + clip_model.positional_embedding
    x = x.permute(1, 0, 2).float()                                                   # LND
    C = x.shape[1]
    D = 0 if deep is None else deep.shape[0]
    for l, block in enumerate(clip_model.transformer.resblocks):
        if 1 <= l <= D:
            rows = deep[l - 1].reshape(-1, P, x.shape[-1]).expand(C, -1, -1).permute(1, 0, 2)      # [P, C, d]
            x = torch.cat([x[:1], rows.to(x.dtype), x[1 + P:]], dim=0)
        x = block(x)
    x = clip_model.ln_final(x.permute(1, 0, 2))
    return x[torch.arange(x.shape[0]), token_ids.argmax(dim=-1)] @ clip_model.text_projection


def _inputs(name, shape, std=1.0, seed=100):
    import grip_amd  # noqa: F401
    from grip_amd import rng
    return torch.from_numpy(rng.normal(seed, rng.stream_id(name), shape, 0.0, std))


def test_restated_oracle_equals_the_wrapper_and_the_golden_entry():
    """With D = 0 the restatement IS oracle.wrappers.text_forward (torch.equal) and reproduces the reference-run g1.text_p3 at the tolerance
    tests/test_oracle_golden.py uses for it; one deep prompt moves the embedding (the deep rows have teeth)."""
    from conftest import oracle_clip
    from oracle import wrappers as W
    tiny = oracle_clip().load("tiny")[0]
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_small.npz"))
    tok = torch.from_numpy(g["g1.coop_tokens"])
    tp = _inputs("g1.tprefix", (1, 3, 128), 0.02)
    with torch.no_grad():
        got = oracle_text_deep_forward(tiny, tok, tp)
        assert torch.equal(got, W.text_forward(tiny, tok, tp))
        np.testing.assert_allclose(got.numpy(), g["g1.text_p3"], rtol=1e-5, atol=1e-5)
        assert torch.equal(oracle_text_deep_forward(tiny, tok, tp, enable_pos_emb=False), W.text_forward(tiny, tok, tp, enable_pos_emb=False))
        deep = _inputs("td.host.deep", (1, 3, 128), 0.02)
        moved = oracle_text_deep_forward(tiny, tok, tp, deep)
        assert (moved - got).abs().max().item() > 1.0
        # the three accepted forms of one deep prompt are the same function
        assert torch.equal(oracle_text_deep_forward(tiny, tok, tp, deep[:, None]), moved)
        assert torch.equal(oracle_text_deep_forward(tiny, tok, tp, deep[:, None].expand(-1, tok.shape[0], -1, -1)), moved)


def test_header_declares_and_library_exports_the_text_deep_calls():
    import grip_amd  # noqa: F401
    from grip_amd import native
    with open(os.path.join(REPO, "include", "grip_amd.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = native.lib()
    for name in ("grip_text_forward_deep", "grip_text_backward_deep"):
        assert re.search(rf"\bint {name}\s*\(", h), name
        assert name in native.EXPORTS
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define GRIP_ABI_VERSION (\d+)", h).group(1)) == native.ABI_VERSION == lib.grip_abi_version() == 9
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "grip_text_forward_deep" in doc and "grip_text_backward_deep" in doc


def test_text_deep_prompt_shape_rules():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    check = engine.check_text_deep_prompts
    check(torch.zeros(1, 4, 8), 1, 4, 8, 12)
    check(torch.zeros(11, 1, 4, 8), 1, 4, 8, 12)
    check(torch.zeros(3, 5, 4, 8), 5, 4, 8, 12)
    for bad, pc, P in ((torch.zeros(12, 4, 8), 1, 4),         # D > layers - 1
                       (torch.zeros(0, 4, 8), 1, 4),          # D = 0 given explicitly
                       (torch.zeros(2, 3, 8), 1, 4),          # not the shallow context's P
                       (torch.zeros(2, 4, 7), 1, 4),          # width
                       (torch.zeros(4, 8), 1, 4),             # not [D, P, d]
                       (torch.zeros(2, 5, 4, 8), 1, 4),       # per-class deep prompts for a shared context
                       (torch.zeros(2, 4, 8), 5, 4),          # shared deep prompts for a class-specific context
                       (torch.zeros(2, 3, 4, 8), 5, 4),       # wrong class count
                       (torch.zeros(1, 4, 8), 1, 0)):         # no shallow context
        with pytest.raises(native.GripError, match="deep text prompts"):
            check(bad, pc, P, 8, 12)
    with pytest.raises(native.GripError, match=r"expected \[D, 4, 8\] \(or \[D, 1, 4, 8\]\) with 1 <= D <= 11"):
        check(torch.zeros(2, 3, 8), 1, 4, 8, 12)
    with pytest.raises(native.GripError, match=r"expected \[D, 5, 4, 8\] with 1 <= D <= 11"):
        check(torch.zeros(2, 4, 8), 5, 4, 8, 12)
    t = types.SimpleNamespace(width=8, dims=types.SimpleNamespace(layers=3))
    deep, D = engine.Tower.text_deep(t, torch.ones(2, 4, 8, dtype=torch.float16), 1, 4)
    assert D == 2 and deep.dtype == torch.float32 and deep.is_contiguous() and deep.shape == (2, 1, 4, 8)
    deep, D = engine.Tower.text_deep(t, torch.ones(1, 5, 4, 8), 5, 4)
    assert D == 1 and deep.shape == (1, 5, 4, 8)
    assert engine.Tower.text_deep(t, None, 1, 4) == (None, 0)
    with pytest.raises(native.GripError, match=r"1 <= D <= 2"):
        engine.Tower.text_deep(t, torch.ones(3, 4, 8), 1, 4)


def _strategy(modality, **conf):
    import grip_amd  # noqa: F401
    from grip_amd import config
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    s.config = types.SimpleNamespace(OPTIM_SEED=3, PREFIX_SIZE=4, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, VAR_INIT=0.02, **conf)
    s.modality = modality
    s.clip_model = types.SimpleNamespace(dims=config.get_dims("ViT-B/16"))
    s.initialize_prompts_parameters()
    return s


def test_coop_deep_initialisation_keeps_the_shallow_context():
    plain, off, deep = _strategy("text"), _strategy("text", COOP_DEEP=False), _strategy("text", COOP_DEEP=True)
    assert torch.equal(plain.initial_prefix, deep.initial_prefix) and torch.equal(plain.initial_prefix, off.initial_prefix)
    assert plain.initial_prefix.shape == (1, 4, 512)
    assert plain.initial_deep_prefix is None and off.initial_deep_prefix is None
    assert deep.initial_deep_prefix.shape == (11, 4, 512)          # [layers - 1, P, transformer_width]
    assert not torch.equal(deep.initial_deep_prefix[0], deep.initial_prefix[0])
    assert abs(float(deep.initial_deep_prefix.std()) - 0.02) < 2e-3
    # drawn from the same generator AFTER the context: the continuation of its stream
    g = torch.Generator().manual_seed(3)
    first = torch.randn(1, 4, 512, generator=g) * 0.02
    assert torch.equal(first, deep.initial_prefix)
    assert torch.equal(torch.randn(11, 4, 512, generator=g) * 0.02, deep.initial_deep_prefix)


def test_visual_and_multimodal_strategies_ignore_coop_deep():
    for modality in ("image", "multi"):
        a, b = _strategy(modality), _strategy(modality, COOP_DEEP=True)
        assert not b.coop_deep()
        if modality == "image":
            assert torch.equal(a.initial_prefix, b.initial_prefix) and b.initial_deep_prefix is None
        else:
            assert torch.equal(a.coop_init, b.coop_init) and torch.equal(a.vpt_init, b.vpt_init) and b.vpt_deep_init is None
            assert not hasattr(b, "initial_deep_prefix")
    # ... and a textual strategy ignores the other two switches
    t = _strategy("text", VPT_DEEP=True, UPT_DEEP=True)
    assert t.initial_deep_prefix is None and not t.vpt_deep() and not t.upt_deep()


def test_text_prefix_model_registers_deep_prefix():
    import grip_amd  # noqa: F401
    from grip_amd.models import TextPrefixModel
    calls = []
    enc = lambda *a, **k: calls.append((a, k))      # noqa: E731
    m = TextPrefixModel(torch.zeros(1, 4, 8), enc, ["a"])
    assert m.deep_prefix is None and [n for n, _ in m.named_parameters()] == ["prefix"]
    m(["a"])
    assert calls[-1][1] == {}                       # without deep prompts: today's call, no keyword
    md = TextPrefixModel(torch.zeros(1, 4, 8), enc, ["a"], deep_prefix=torch.ones(2, 4, 8))
    assert sorted(n for n, _ in md.named_parameters()) == ["deep_prefix", "prefix"] and md.deep_prefix.requires_grad
    md(["a"])
    assert calls[-1][1]["deep_prompts"] is md.deep_prefix
    from grip_amd import steps
    assert steps._coop_params(m) == [m.prefix] and steps._coop_params(md)[1] is md.deep_prefix
