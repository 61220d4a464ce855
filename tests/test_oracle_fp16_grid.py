"""CPU: the on-grid oracle (oracle.clip.load(..., fp16_grid=True): every matrix weight an f16 number, as a published fp16 checkpoint holds them) and the
fixtures the reference produced on it (oracle/gen_golden_exact.py --fp16-grid, oracle/gen_golden.py vitb16grid).  Guards the switch -- the keyword and
nothing else -- and the committed files against drift; runs without a GPU and without the reference."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, oracle_clip

TAGS = ("c10", "c102")
KS = (3, 16, 10000000)
TIE = 2.0 ** -17      # = tests/test_gpu_exact.TIE: one ulp of an fp32 logit in [64, 128)


def _fixture(tag, grid=True):
    return np.load(os.path.join(REPO, "tests", "golden", f"exact_vitb16_{'fp16grid_' if grid else ''}{tag}.npz"))


def _is_matrix(key, v):
    """What a published checkpoint stores in f16 (clip.model.convert_weights): convolution / Linear / attention / projection weights -- not the embedding
    tables, not vectors."""
    return v.ndim >= 2 and not key.endswith("positional_embedding") and "token_embedding" not in key


@pytest.fixture(scope="module")
def vitb16_grid():
    return oracle_clip().load("ViT-B/16", fp16_grid=True)[0]


@pytest.mark.parametrize("name", ["small", "ViT-B/16"])
def test_fp16_grid_rounds_matrix_weights_only(name, vitb16_grid):
    import grip_amd  # noqa: F401
    from grip_amd import config, weights
    init = weights.init_state_dict(config.get_dims(name), 0)
    m = vitb16_grid if name == "ViT-B/16" else oracle_clip().load(name, fp16_grid=True)[0]
    sd = {k: v.numpy() for k, v in m.state_dict().items() if k in init}
    assert set(sd) == set(init)
    moved = 0
    for k, v in sd.items():
        if _is_matrix(k, v):
            assert np.array_equal(v, v.astype(np.float16).astype(np.float32)), f"{k}: not on the f16 grid"
            assert np.array_equal(v, init[k].reshape(v.shape).astype(np.float16).astype(np.float32)), f"{k}: not the seeded weight rounded"
            moved += int((v != init[k].reshape(v.shape)).any())
        else:
            assert np.array_equal(v, init[k].reshape(v.shape)), f"{k}: a table / vector was touched"
    n_matrix = sum(_is_matrix(k, v) for k, v in sd.items())
    assert moved == n_matrix > 0            # the seeded init is off the grid everywhere: the rounding is not a no-op
    assert any(not _is_matrix(k, v) and v.ndim >= 2 for k, v in sd.items())      # the embedding tables are in the comparison


def test_fp16_grid_is_by_keyword_only(monkeypatch):
    """bench.py sets GRIP_SYNTHETIC_FP16=1 before its CPU baseline imports the oracle: the oracle must not read it."""
    import grip_amd  # noqa: F401
    from grip_amd import config, weights
    oc = oracle_clip()
    init = weights.init_state_dict(config.get_dims("small"), 0)
    plain = {k: v.clone() for k, v in oc.load("small")[0].state_dict().items()}
    monkeypatch.setenv("GRIP_SYNTHETIC_FP16", "1")
    for m in (oc.load("small")[0], oc.load("small", fp16_grid=False)[0], oc.clip.build_model("small")):
        sd = m.state_dict()
        assert set(sd) == set(plain)
        for k, v in sd.items():
            assert torch.equal(v, plain[k]), k
            if k in init:
                assert np.array_equal(v.numpy(), init[k].reshape(v.shape)), k
    grid = oc.clip.build_model("small", fp16_grid=True).state_dict()
    assert not torch.equal(grid["visual.proj"], plain["visual.proj"])


def _tie_pairs(lists, probs, paths):
    index = {p: i for i, p in enumerate(paths)}
    fp, lab = lists
    n = 0
    for a, b, la, lb in zip(fp[:-1], fp[1:], lab[:-1], lab[1:]):
        if la == lb:
            sa, sb = float(probs[index[a], la]), float(probs[index[b], la])
            n += abs(sa - sb) <= TIE * max(sa, sb)
    return n


@pytest.mark.parametrize("tag", TAGS)
def test_on_grid_exact_fixture_is_consistent(tag):
    """The oracle's literal scan over the stored probabilities returns the stored lists (what the reference's compute_pseudo_labels returned), and the
    stored margins and tie-pair counts are those of these probabilities.  Same keys as the off-grid files plus emb_head, txt, tie_pairs_k*."""
    import grip_amd  # noqa: F401
    from grip_amd.data.synthetic import pool_paths
    from oracle import leaderboard as LB
    fx, off = _fixture(tag), _fixture(tag, grid=False)
    # emb_head is stored once, in the c10 file: the image embeddings do not depend on the class set, and with them the c102 file would pass 1 MiB
    assert set(fx.files) == set(off.files) | {"txt"} | {f"tie_pairs_k{k}" for k in KS} | ({"emb_head"} if tag == "c10" else set())
    probs = fx["probs"]
    n, C = probs.shape
    assert n == 2000 and C == off["probs"].shape[1] and probs.dtype == np.float32
    assert int(fx["seed"]) == int(off["seed"]) == 4242 and np.array_equal(fx["tokens"], off["tokens"])
    if tag == "c10":
        assert fx["emb_head"].shape == (64, 512) and fx["emb_head"].dtype == np.float32
    assert fx["txt"].shape == (C, 512) and fx["txt"].dtype == np.float32
    paths, pred, labels = pool_paths(n), probs.argmax(1), list(range(C))
    for k in KS:
        want = json.loads(str(fx[f"lists_k{k}"]))
        got = LB.leaderboard_scan(probs, pred, paths, labels, k)
        assert [list(got[0]), list(got[1])] == want, f"{tag} k={k}"
        assert float(fx[f"margin_k{k}"]) == LB.scan_margin(probs, pred, k)
        assert int(fx[f"tie_pairs_k{k}"]) == (0 if k == 10000000 else _tie_pairs(want, probs, paths))


def test_on_grid_exact_fixture_head_rows_reproduce_live(vitb16_grid):
    """Rows 0..63 recomputed on the on-grid oracle, image by image as the reference loop runs them: `emb_head`, `txt` and `probs` come back bit for bit.
    The last bits of the CPU GEMMs depend on how they are split over threads: the generator ran on 8 torch threads, and so does this test."""
    import grip_amd  # noqa: F401
    from grip_amd.data.synthetic import structured_images
    om = vitb16_grid
    fx = {tag: _fixture(tag) for tag in TAGS}
    x = structured_images(int(fx["c10"]["seed"]), 0, 64, 224)
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        _head_rows(om, fx, x)
    finally:
        torch.set_num_threads(threads)


def _head_rows(om, fx, x):
    with torch.no_grad():
        f = torch.cat([om.encode_image(x[i:i + 1]) for i in range(64)])
        assert np.array_equal(f.numpy(), fx["c10"]["emb_head"])
        fn = torch.cat([r[None] / r[None].norm(dim=1, keepdim=True) for r in f])
        for tag in TAGS:
            t = om.encode_text(torch.from_numpy(fx[tag]["tokens"]))
            assert np.array_equal(t.numpy(), fx[tag]["txt"]), tag
            tn = t / t.norm(dim=1, keepdim=True)
            logits = torch.cat([om.logit_scale.exp() * fn[i:i + 1] @ tn.t() for i in range(64)])      # oracle CLIP.forward's tail, per image
            assert np.array_equal(logits.softmax(dim=-1).numpy(), fx[tag]["probs"][:64]), tag


@pytest.mark.parametrize("tag", TAGS)
def test_on_grid_and_off_grid_fixtures_tell_the_models_apart(tag):
    """Teeth: the GPU tests hold the exact mode to 1e-4 relative of the fixture's probabilities.  On the same pool the on-grid and the off-grid oracle
    differ by 1.86e-3 (C = 10) and 1.81e-3 (C = 102) relative at ViT-B/16 (measured when the fixtures were generated): a model built from the wrong
    weights cannot satisfy the fixture of the other."""
    on, off = _fixture(tag)["probs"].astype(np.float64), _fixture(tag, grid=False)["probs"].astype(np.float64)
    rel = float((np.abs(on - off) / off).max())
    print(f"{tag}: on-grid vs off-grid probabilities differ by {rel:.3e} relative")
    assert rel > 1e-4


def test_on_grid_tower_fixture_reproduces_and_differs_from_the_off_grid_one(vitb16_grid, golden_vitb16):
    """golden_vitb16_fp16grid.npz: the g3 block of golden_vitb16.npz (same inputs, same key names) on the on-grid oracle."""
    import grip_amd  # noqa: F401
    from grip_amd import rng
    from oracle import wrappers as W
    g = np.load(os.path.join(REPO, "tests", "golden", "golden_vitb16_fp16grid.npz"))
    g3 = {k for k in golden_vitb16.files if k.startswith("g3.")}
    assert set(g.files) == g3
    for k in ("g3.zs_tokens", "g3.coop_tokens"):
        assert np.array_equal(g[k], golden_vitb16[k])
    x = torch.from_numpy(rng.normal(100, rng.stream_id("g3.x"), (2, 3, 224, 224), 0.0, 1.0))
    vp = torch.from_numpy(rng.normal(100, rng.stream_id("g3.vprefix"), (16, 768), 0.0, 0.02))
    with torch.no_grad():
        np.testing.assert_allclose(W.vision_forward(vitb16_grid.visual, x, None).numpy(), g["g3.vision_p0"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(W.vision_forward(vitb16_grid.visual, x, vp).numpy(), g["g3.vision_p16"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(W.text_forward(vitb16_grid, torch.from_numpy(g["g3.zs_tokens"]), None).numpy(), g["g3.text_p0"], rtol=1e-5, atol=1e-5)
    for k in ("g3.vision_p0", "g3.vision_p16", "g3.text_p0", "g3.text_p16", "g3.vision_p16_grad_prefix", "g3.text_p16_grad_prefix"):
        a, b = g[k].astype(np.float64), golden_vitb16[k].astype(np.float64)
        assert np.linalg.norm(a - b) / np.linalg.norm(b) > 5e-5, k       # beyond the relative L2 the f32 twin is held to: the two files cannot stand in for each other
