"""The fp16-checkpoint weight path against the reference: clip.load(..., fp16_checkpoint=True) -- every matrix weight an f16 number, what a published
CLIP checkpoint holds, what bench.py times and what any user with real weights runs -- held to fixtures the REFERENCE's own compute_pseudo_labels and
wrappers produced on the CPU oracle built from the same on-grid weights (oracle.clip.load(..., fp16_grid=True); oracle/gen_golden_exact.py --fp16-grid,
oracle/gen_golden.py vitb16grid).  On-grid weights take code off-grid weights do not: grip_tower_finalize finds no non-zero lo part and the split-f16
tier runs its two-pass GEMMs (GemmArgs::w_exact), the f16 towers round no weight, and the screen's deviation, its calibrated bound and the share of the
pool taken on trust all change.  Until this file those were compared HIP against HIP only.

Every tolerance is the one the project holds the same quantity to on off-grid weights (tests/test_gpu_exact.py, test_gpu_towers.py,
test_gpu_backward.py, test_gpu_identical.py).  Images and weights are regenerated from their seeds; nothing here reads the reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, structured_pool, write_report

pytestmark = pytest.mark.gpu

NAME = "ViT-B/16"
KS = (3, 16, 10000000)
TAGS = ("c10", "c102")


def _fixture(tag, grid=True):
    return np.load(os.path.join(REPO, "tests", "golden", f"exact_vitb16_{'fp16grid_' if grid else ''}{tag}.npz"))


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native.lib()


def _rel(got, want):
    """Largest relative deviation of the probabilities `got` from the reference's `want` (the form tests/test_gpu_exact.py holds to 1e-4)."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / want).max())


class _Ctx:
    """The on-grid models, the 2 000-image pool and what each tower makes of it, computed once per module and on first use."""

    def __init__(self):
        import grip_amd  # noqa: F401
        from grip_amd import clip
        from grip_amd.data.synthetic import pool_paths
        self.fx = {tag: _fixture(tag) for tag in TAGS}
        self.n = self.fx["c10"]["probs"].shape[0]
        self.seed = int(self.fx["c10"]["seed"])
        assert self.n == self.fx["c102"]["probs"].shape[0] == 2000 and self.seed == int(self.fx["c102"]["seed"])
        self.m, _ = clip.load(NAME, device="cuda", fp16_checkpoint=True)
        self.twin, self.split = self.m.exact_twin(), self.m.split_twin()
        assert self.twin.visual.tower.exact and self.split is not None
        self.scale = self.m.logit_scale.exp().item()
        self.paths = pool_paths(self.n)
        self.pool = structured_pool(self.seed, self.n, 224)
        self._emb, self._txt, self._probs, self.runs = {}, {}, {}, {}

    def emb(self, which):
        """[n, 512] embeddings of the pool: "f32" / "split" twins, "f16" / "hilo" screens of the f16 tower."""
        from grip_amd import pseudolabels as pl
        if which not in self._emb:
            with torch.no_grad():
                if which == "f32":
                    e = pl.encode_pool(self.twin.visual.tower, self.pool, chunk=250)
                elif which == "split":
                    e = pl.encode_pool(self.split.visual.tower, self.pool, chunk=250)
                    self.split_wlo = _lib().grip_debug_split_last_wlo()
                else:
                    e = pl.encode_pool(self.m.visual.tower, self.pool, chunk=500, screen=which)
            self._emb[which] = e
        return self._emb[which]

    def txt(self, tag):
        """The f32 twin's text features of the fixture's own token ids (what identical_lists scores every tier against)."""
        if tag not in self._txt:
            with torch.no_grad():
                self._txt[tag] = self.twin.encode_text(torch.from_numpy(self.fx[tag]["tokens"]).cuda())
        return self._txt[tag]

    def probs(self, which, tag, emb=None):
        """(probabilities [n, C], arg-max) on the host of one tower's embeddings under the twin's text features."""
        from grip_amd import engine
        if (which, tag) not in self._probs:
            _, p, _, am = engine.cosine_head(self.emb(which) if emb is None else emb, self.txt(tag), self.scale)
            self._probs[(which, tag)] = (p.cpu().numpy(), am.cpu().numpy())
        return self._probs[(which, tag)]

    def twin_deviation(self, tag, form, abs_eps):
        """The f32 twin's own deviation from the reference's probabilities in a bound form of pseudolabels.refine_scan."""
        from grip_amd import pseudolabels as pl
        return (pl._deviation if form == "relative" else pl._deviation_odds)(self.probs("f32", tag)[0], self.fx[tag]["probs"], abs_eps)


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    """Every test starts from the library's defaults, whatever the caller's environment holds."""
    for v in ("GRIP_PSEUDOLABEL_MODE", "GRIP_REFINE_BOUND", "GRIP_REFINE_AUDIT", "GRIP_SCREEN_STREAM", "GRIP_SPLIT_TIER", "GRIP_SPLIT_WLO", "GRIP_EXACT",
              "GRIP_SYNTHETIC_FP16", "CLIP_WEIGHTS"):
        monkeypatch.delenv(v, raising=False)


def _against_reference(ctx, tag, what, probs, pred, emb):
    """The three comparisons a twin is held to: probabilities within 1e-4 relative of the reference's, the first 64 embeddings at the exact towers'
    tolerance (test_exact_towers_match_golden_vitb16), and the reference's lists for k = 3, 16 and label-everything, where the only deviation allowed is
    a transposition inside a class board between two scores a TIE (one ulp of an fp32 logit) apart: the project allows one such transposition (two
    positions, tests/test_gpu_exact.py), and never more than the fixture counts tie pairs.  Returns the figures for the report."""
    from grip_amd import pseudolabels as pl
    from test_gpu_exact import _close, assert_lists_identical
    fx = ctx.fx[tag]
    o_probs = fx["probs"]
    labels = list(range(o_probs.shape[1]))
    rel = _rel(probs, o_probs)
    head = emb[:64].detach().cpu().double()
    emb_head = ctx.fx["c10"]["emb_head"]       # stored once: the image embeddings do not depend on the class set
    want = torch.from_numpy(emb_head).double()
    figures = {"max_relative_dp": rel,
               "emb_head_one_minus_cos": float((1 - torch.nn.functional.cosine_similarity(head, want, dim=-1)).max()),
               "emb_head_rel_l2": float((head - want).norm() / want.norm()), "transposed_positions": {}, "tie_pairs": {}}
    print(f"{what} {tag}: max relative dp {rel:.3e}, emb_head 1-cos {figures['emb_head_one_minus_cos']:.3e} rel L2 {figures['emb_head_rel_l2']:.3e}")
    assert rel <= 1e-4, f"{what} {tag}: probabilities are {rel:.2e} (relative) from the on-grid reference's"
    _close(emb[:64], emb_head, f"{what} {tag} emb_head", cos_tol=1e-6, rel_tol=5e-5)
    for k in KS:
        ref = json.loads(str(fx[f"lists_k{k}"]))
        got = pl.leaderboard(probs, pred, ctx.paths, labels, k)
        swapped = assert_lists_identical(got, (ref[0], ref[1]), o_probs, ctx.paths, labels, f"{what} {tag} k={k}")
        ties = int(fx[f"tie_pairs_k{k}"])
        figures["transposed_positions"][str(k)], figures["tie_pairs"][str(k)] = swapped, ties
        print(f"{what} {tag} k={k}: {len(ref[0])} pairs, transposed positions {swapped}, tie pairs in the reference boards {ties}")
        assert swapped <= 2 and -(-swapped // 2) <= min(2, ties), f"{what} {tag} k={k}: {swapped} transposed positions with {ties} tie pairs"
    return figures


# ------------------------------------------------------------------------------------------------ (a) the f32 twin
@pytest.mark.parametrize("tag", TAGS)
def test_f32_twin_on_grid_matches_the_reference(ctx, tag):
    """The twin every other tier is certified against, on the weights the bench runs, against the reference run on the same weights."""
    p, am = ctx.probs("f32", tag)
    figures = _against_reference(ctx, tag, "f32 twin", p, am, ctx.emb("f32"))
    txt, want = ctx.txt(tag).cpu().double(), torch.from_numpy(ctx.fx[tag]["txt"]).double()
    figures["txt_rel_l2"] = float((txt - want).norm() / want.norm())
    write_report(f"fp16_checkpoint_f32_twin_{tag}.json", figures)
    from test_gpu_exact import _close
    _close(ctx.txt(tag), ctx.fx[tag]["txt"], f"{tag} text features", cos_tol=1e-6, rel_tol=5e-5)


# ------------------------------------------------------------------------------------------------ (b) the split-f16 twin, both forms
@pytest.mark.parametrize("tag", TAGS)
def test_split_twin_two_pass_matches_the_reference(ctx, tag):
    """On-grid weights have no lo part: the split tower runs its two-pass GEMMs (w_exact).  Here that tower meets the reference, not another HIP tower."""
    emb = ctx.emb("split")
    assert ctx.split_wlo == 0, "the split twin formed the a_hi w_lo product on weights that are f16 numbers"
    p, am = ctx.probs("split", tag)
    figures = _against_reference(ctx, tag, "split twin (two passes)", p, am, emb)
    figures["max_relative_dp_vs_f32_twin"] = _rel(p, ctx.probs("f32", tag)[0].astype(np.float64))
    write_report(f"fp16_checkpoint_split_twin_{tag}.json", figures)


WLO_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["GRIP_REPO"]); sys.path.insert(0, os.path.join(os.environ["GRIP_REPO"], "tests"))
import numpy as np, torch
import grip_amd
from grip_amd import clip, native, pseudolabels as pl
from conftest import structured_pool
m, _ = clip.load("ViT-B/16", device="cuda", fp16_checkpoint=True)
split = m.split_twin()
pool = structured_pool(int(os.environ["GRIP_T_SEED"]), int(os.environ["GRIP_T_N"]), 224)
with torch.no_grad():
    emb = pl.encode_pool(split.visual.tower, pool, chunk=250)
np.savez(os.environ["GRIP_OUT"], emb=emb.cpu().numpy(), wlo=native.lib().grip_debug_split_last_wlo())
'''


def test_split_twin_three_pass_matches_the_reference(ctx, tmp_path):
    """GRIP_SPLIT_WLO=1: the same tower forming all three products on the same on-grid weights, held to the same bounds, so that each form is pinned to
    the reference and not only to the other.  The library reads the switch once per process: the encode runs in a fresh child, and only the child's
    environment carries the switch (this process may not have run a split GEMM yet)."""
    script = tmp_path / "wlo_child.py"
    script.write_text(WLO_CHILD)
    env = dict(os.environ, GRIP_SPLIT_WLO="1", GRIP_REPO=REPO, GRIP_OUT=str(tmp_path / "wlo.npz"), GRIP_T_SEED=str(ctx.seed), GRIP_T_N=str(ctx.n), PYTHONPATH=REPO)
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.load(tmp_path / "wlo.npz")
    assert int(got["wlo"]) == 1, "GRIP_SPLIT_WLO=1 did not reach the split GEMM"
    emb = torch.from_numpy(got["emb"]).cuda()
    report = {"max_abs_embedding_difference_from_two_pass": float((emb - ctx.emb("split")).abs().max())}
    for tag in TAGS:
        p, am = ctx.probs("split3", tag, emb=emb)
        report[tag] = _against_reference(ctx, tag, "split twin (three passes)", p, am, emb)
    write_report("fp16_checkpoint_split_twin_three_pass.json", report)


# ------------------------------------------------------------------------------------------------ (c) towers and gradients on the grid
@pytest.fixture(scope="module")
def golden_grid():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_vitb16_fp16grid.npz"))


def _g3_inputs():
    from test_gpu_towers import _inputs
    return (_inputs("g3.x", (2, 3, 224, 224)).cuda(), _inputs("g3.vprefix", (16, 768), 0.02).cuda(), _inputs("g3.tprefix", (1, 16, 512), 0.02).cuda())


def test_f16_towers_and_prompt_gradients_on_grid_match_golden(ctx, golden_grid):
    """The f16 model on f16-number weights against the on-grid oracle: forward at 1 - cos <= 1e-4 (test_gpu_towers.py), both prompt gradients at
    cosine >= 0.999 / relative L2 <= 3e-2 (test_gpu_backward.py)."""
    from grip_amd.models import CustomImageEncoder, ImagePrefixModel
    from test_gpu_backward import _full_size_text_gradient, assert_grad_close
    from test_gpu_towers import assert_embeddings_close
    m, g = ctx.m, golden_grid
    x, vprefix, tprefix = _g3_inputs()
    assert_embeddings_close(m.encode_image(x), g["g3.vision_p0"], "on-grid B/16 encode_image")
    with torch.no_grad():
        assert_embeddings_close(CustomImageEncoder(m.visual)(x, vprefix), g["g3.vision_p16"], "on-grid B/16 vision+prefix")
    assert_embeddings_close(m.encode_text(torch.from_numpy(g["g3.zs_tokens"]).cuda()), g["g3.text_p0"], "on-grid B/16 encode_text")
    out, _, _ = m.text_tower.text_forward(torch.from_numpy(g["g3.coop_tokens"]).cuda(), tprefix)
    assert_embeddings_close(out, g["g3.text_p16"], "on-grid B/16 text+prefix")
    logits, _ = m(x, torch.from_numpy(g["g3.zs_tokens"]).cuda())
    assert (logits.softmax(-1).cpu() - torch.from_numpy(g["g3.zs_probs"])).abs().max().item() <= 1e-2
    _full_size_text_gradient(m, g, "g3", 512)
    model = ImagePrefixModel(vprefix.clone(), CustomImageEncoder(m.visual), device="cuda")
    (model(x) ** 2).sum().backward()
    assert_grad_close(model.prefix.grad, g["g3.vision_p16_grad_prefix"], "on-grid g3 visual prompt grad")


def test_f32_twin_towers_on_grid_match_golden(ctx, golden_grid):
    """The f32 twin at the exact towers' tolerances (1 - cos <= 1e-6, relative L2 <= 5e-5), zero-shot probabilities within 1e-5."""
    from grip_amd.models import CustomImageEncoder
    from test_gpu_exact import _close
    m, g = ctx.twin, golden_grid
    x, vprefix, tprefix = _g3_inputs()
    _close(m.encode_image(x), g["g3.vision_p0"], "on-grid twin encode_image", rel_tol=5e-5)
    with torch.no_grad():
        _close(CustomImageEncoder(m.visual)(x, vprefix), g["g3.vision_p16"], "on-grid twin vision+prefix", rel_tol=5e-5)
    _close(m.encode_text(torch.from_numpy(g["g3.zs_tokens"]).cuda()), g["g3.text_p0"], "on-grid twin encode_text", rel_tol=5e-5)
    out, _, _ = m.text_tower.text_forward(torch.from_numpy(g["g3.coop_tokens"]).cuda(), tprefix)
    _close(out, g["g3.text_p16"], "on-grid twin text+prefix", rel_tol=5e-5)
    logits, _ = m(x, torch.from_numpy(g["g3.zs_tokens"]).cuda())
    assert (logits.softmax(-1).cpu() - torch.from_numpy(g["g3.zs_probs"])).abs().max().item() <= 1e-5


# ------------------------------------------------------------------------------------------------ (d) the default path, (e) its bound
def _run(ctx, monkeypatch, tag, tiers, screen, k):
    """One identical_lists run over the pool with the screen's embeddings handed in; cached, so that (e) looks at the very run (d) asserted on."""
    from grip_amd import pseudolabels as pl
    key = (tag, tiers, screen, k)
    if key not in ctx.runs:
        monkeypatch.setenv("GRIP_SPLIT_TIER", "1" if tiers == 3 else "0")
        mid = pl.mid_tower(ctx.m, ctx.n)        # the pool is below the automatic threshold: the switch brings the middle tier in
        assert (mid is not None) == (tiers == 3)
        labels = list(range(ctx.fx[tag]["probs"].shape[1]))
        got = pl.identical_lists(ctx.m.visual.tower, ctx.twin.visual.tower, ctx.pool, ctx.txt(tag), ctx.scale, ctx.paths, labels, k, chunk=500,
                                 emb16=ctx.emb(screen), visual_mid=mid)
        ctx.runs[key] = (got, dict(pl.LAST_REFINE_STATS), _lib().grip_debug_split_last_wlo())
    return ctx.runs[key]


def _run_report(st):
    return {"rows_refined": st["rows_refined"], "rows_mid": st["rows_mid"], "rows_exact": st["rows_exact"], "unverified_rows": st["unverified_rows"],
            "bound": st["eps"], "bound_mid": st["eps_mid"], "bound_form": st["bound_form"], "max_deviation": st["max_deviation"],
            "max_deviation_mid": st["max_deviation_mid"], "rounds": st["rounds"], "audit_widened": st.get("audit_widened", False),
            "escalated": st.get("escalated", False)}


def _assert_default_run(ctx, tag, k, got, st, wlo, tiers, what):
    from grip_amd import pseudolabels as pl
    from test_gpu_exact import assert_lists_identical
    fx = ctx.fx[tag]
    labels = list(range(fx["probs"].shape[1]))
    p32, a32 = ctx.probs("f32", tag)
    exact = pl.leaderboard(p32, a32, ctx.paths, labels, k)
    assert (list(got[0]), list(got[1])) == (list(exact[0]), list(exact[1])), f"{what}: lists differ from the f32 twin's"
    ref = json.loads(str(fx[f"lists_k{k}"]))
    swapped = assert_lists_identical(got, (ref[0], ref[1]), fx["probs"], ctx.paths, labels, what)
    assert swapped <= 2 and -(-swapped // 2) <= min(2, int(fx[f"tie_pairs_k{k}"])), f"{what}: {swapped} transposed positions against the reference"
    # ... and not emptily: the scan did not give up and re-encode everything, and rows were left to the screen's bound
    assert not st.get("escalated"), f"{what}: the scan escalated"
    assert st["unverified_rows"] > 0, f"{what}: every row was re-encoded"
    assert st["tiers"] == tiers
    if tiers == 3:
        assert st["rows_mid"] > 0, f"{what}: the middle tier encoded nothing"
        assert wlo == 0, f"{what}: the middle tier formed the a_hi w_lo product on f16-number weights"


@pytest.mark.parametrize("screen", ["f16", "hilo"])
@pytest.mark.parametrize("tiers", [2, 3])
@pytest.mark.parametrize("tag", TAGS)
def test_default_path_on_grid_returns_the_twin_and_reference_lists(ctx, monkeypatch, tag, tiers, screen):
    """pseudolabels.identical_lists as the bench runs it -- on-grid f16 screen (plain and compensated stream), two tiers and three -- for k = 3, 16 and
    label-everything: exactly the f32 twin's lists and, through (a), the reference's."""
    report = {}
    for k in KS:
        got, st, wlo = _run(ctx, monkeypatch, tag, tiers, screen, k)
        report[f"k{k}"] = _run_report(st)
        print(f"{tag} tiers={tiers} screen={screen} k={k}: {st['rows_mid']} rows split-f16 / {st['rows_exact']} rows f32 of {ctx.n}, "
              f"{st['unverified_rows']} on trust, bound {st['eps']:.3e} ({st['bound_form']}), largest deviation {st['max_deviation']:.3e}")
        _assert_default_run(ctx, tag, k, got, st, wlo, tiers, f"{tag} tiers={tiers} screen={screen} k={k}")
    write_report(f"fp16_checkpoint_default_{tag}_tiers{tiers}_{screen}.json", report)


@pytest.mark.parametrize("tag", TAGS)
def test_default_path_on_grid_encoding_its_own_screen(ctx, monkeypatch, tag):
    """The same call without emb16=: identical_lists encodes the screen itself, under GRIP_SCREEN_STREAM=hilo."""
    from grip_amd import pseudolabels as pl
    monkeypatch.setenv("GRIP_SCREEN_STREAM", "hilo")
    monkeypatch.setenv("GRIP_SPLIT_TIER", "0")
    labels = list(range(ctx.fx[tag]["probs"].shape[1]))
    got = pl.identical_lists(ctx.m.visual.tower, ctx.twin.visual.tower, ctx.pool, ctx.txt(tag), ctx.scale, ctx.paths, labels, 16, chunk=500)
    st = dict(pl.LAST_REFINE_STATS)
    assert st["screen_stream"] == "hilo"
    write_report(f"fp16_checkpoint_default_{tag}_own_screen.json", _run_report(st))
    _assert_default_run(ctx, tag, 16, got, st, None, 2, f"{tag} own screen k=16")


@pytest.mark.parametrize("screen", ["f16", "hilo"])
@pytest.mark.parametrize("tiers", [2, 3])
@pytest.mark.parametrize("tag", TAGS)
def test_screen_bound_on_grid_holds_against_the_reference(ctx, monkeypatch, tag, tiers, screen):
    """The screen's bound is calibrated on 256 rows and trusted on the rest.  Here all 2 000 true values are known -- and the project did not compute
    them: every row of the screen the scan saw, measured against the reference's probabilities in the run's own bound form, stays within the bound the
    run ended with, plus the f32 twin's own deviation from the reference in that form (a), plus 4 x the form's evaluation slack."""
    from grip_amd import pseudolabels as pl
    o_probs = ctx.fx[tag]["probs"]
    screen_probs = ctx.probs(screen, tag)[0]
    report, failures = {}, []
    for k in KS:
        _, st, _ = _run(ctx, monkeypatch, tag, tiers, screen, k)
        form, abs_eps = st["bound_form"], st["abs_eps"]
        deviation = pl._deviation if form == "relative" else pl._deviation_odds
        rows = np.array([deviation(screen_probs[i], o_probs[i], abs_eps) for i in range(ctx.n)])
        twin = ctx.twin_deviation(tag, form, abs_eps)
        held = st["eps"] + twin + 4 * pl._KR
        worst = int(rows.argmax())
        report[f"k{k}"] = {"bound_form": form, "bound": st["eps"], "twin_deviation_from_reference": twin, "held_to": held,
                           "largest_screen_row_deviation": float(rows[worst]), "row": worst, "rows_beyond": int((rows > held).sum()),
                           "unverified_rows": st["unverified_rows"]}
        print(f"{tag} tiers={tiers} screen={screen} k={k}: largest screen-row deviation from the reference {rows[worst]:.3e} (row {worst}), held to "
              f"{held:.3e} = bound {st['eps']:.3e} + twin {twin:.3e} + slack; {int((rows > held).sum())} rows beyond")
        if rows[worst] > held:
            failures.append((k, worst, float(rows[worst]), held))
    write_report(f"fp16_checkpoint_bound_{tag}_tiers{tiers}_{screen}.json", report)
    assert not failures, f"{tag} tiers={tiers} screen={screen}: screen rows beyond the bound they were trusted to (k, row, deviation, held to): {failures}"


# ------------------------------------------------------------------------------------------------ (f) teeth
def test_on_grid_twin_is_not_the_off_grid_reference_and_vice_versa(ctx):
    """A model built from the wrong weights would be noticed: the on-grid twin is further than the 1e-4 of (a) from the OFF-grid fixture, and the
    off-grid twin from the ON-grid one (C = 102)."""
    from grip_amd import clip, engine, pseudolabels as pl
    on_vs_off = _rel(ctx.probs("f32", "c102")[0], _fixture("c102", grid=False)["probs"])
    off, _ = clip.load(NAME, device="cuda", exact=True, fp16_checkpoint=False)
    with torch.no_grad():
        emb = pl.encode_pool(off.visual.tower, ctx.pool, chunk=250)
        txt = off.encode_text(torch.from_numpy(ctx.fx["c102"]["tokens"]).cuda())
    _, p, _, _ = engine.cosine_head(emb, txt, off.logit_scale.exp().item())
    off_vs_on = _rel(p.cpu().numpy(), ctx.fx["c102"]["probs"])
    off_vs_off = _rel(p.cpu().numpy(), _fixture("c102", grid=False)["probs"])
    write_report("fp16_checkpoint_teeth.json", {"on_grid_twin_vs_off_grid_fixture": on_vs_off, "off_grid_twin_vs_on_grid_fixture": off_vs_on,
                                                "off_grid_twin_vs_off_grid_fixture": off_vs_off})
    print(f"relative dp: on-grid twin vs off-grid fixture {on_vs_off:.3e}, off-grid twin vs on-grid fixture {off_vs_on:.3e} (vs its own {off_vs_off:.3e})")
    assert on_vs_off > 1e-4
    assert off_vs_on > 1e-4
