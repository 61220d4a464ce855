"""engine.gmm_transduce (the Python loop over grip_gmm_mstep / grip_gmm_estep): bit-equal to the hand-rolled loop over the two ABI calls, and the
planted-cluster case that carries the meaning of the feature: class Gaussians fitted to the pool repair 30 % wrong text labels."""
import pytest
import torch

import gmm_ref as R
from conftest import write_report

pytestmark = pytest.mark.gpu


def planted(n=512, c=8, e=64, seed=0, wrong_share=0.3):
    """(emb [n, e], probs [n, c], y [n]): unit centres, per-dimension noise 0.25 / sqrt(e); P puts 0.6 on the true class -- on a wrong one for a random
    30 % of the rows -- plus 0.02 U noise, renormalised."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(c, e, generator=g), dim=1)
    y = torch.randint(0, c, (n,), generator=g)
    emb = centres[y] + 0.25 / e ** 0.5 * torch.randn(n, e, generator=g)
    wrong = torch.rand(n, generator=g) < wrong_share
    shown = torch.where(wrong, (y + torch.randint(1, c, (n,), generator=g)) % c, y)
    probs = 0.4 / (c - 1) * torch.ones(n, c)
    probs[torch.arange(n), shown] = 0.6
    probs = probs + 0.02 * torch.rand(n, c, generator=g)
    return emb, probs / probs.sum(1, keepdim=True), y


def test_transduce_is_the_loop_over_the_two_calls_bit_for_bit():
    import grip_amd  # noqa: F401
    from grip_amd import engine
    from test_gpu_gmm_kernels import _estep, _mstep
    emb, probs, _ = planted(n=R.ROWS + 44, c=65, e=64, seed=5)
    emb, probs = (emb * 7.0).cuda(), probs.cuda()                      # (not unit rows: gmm_transduce normalises them itself)
    idx, sim = engine.knn_graph(emb, k=3)
    z, pred, mean, var, count = engine.gmm_transduce(emb, probs, idx, sim, lam=0.5, iters=3, z_iters=2, var_floor=1e-6)
    f = torch.nn.functional.normalize(emb, dim=1).contiguous()
    hz = probs
    for _ in range(3):
        hc, hm, hv = _mstep(hz, f, 1e-6)
        hz, hp = _estep(f, hm.contiguous(), hv.contiguous(), probs, idx, sim, hz.contiguous(), 0.5, 2)
    assert torch.equal(z, hz) and torch.equal(pred, hp) and torch.equal(mean, hm) and torch.equal(var, hv) and torch.equal(count, hc)
    assert z.dtype == torch.float32 and pred.dtype == torch.int32 and tuple(mean.shape) == (65, 64) and tuple(var.shape) == (64,) and tuple(count.shape) == (65,)
    with pytest.raises(engine.native.GripError, match="iters = 0"):
        engine.gmm_transduce(emb, probs, idx, sim, iters=0)


def test_planted_clusters_are_repaired_over_the_kernels_own_graph():
    """n = 512, c = 8, e = 64, k = 3, lam = 1, iters = 10, z_iters = 5, seed 0.  The graph is grip_knn_graph's and the float64 recursion runs on THAT
    graph.  Preconditions on the REFERENCE alone: its accuracy is below 0.75 before and exactly 1.0 after, and its smallest top-2 margin exceeds 100 x the
    largest bound (a float64 trial on the host with an exact graph: 0.691 -> 1.000, smallest margin 1.0, largest bound 9.5e-7).  Then the kernel's arg-max equals the
    reference's on every row."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    emb, probs, y = planted()
    emb, probs = emb.cuda(), probs.cuda()
    idx, sim = engine.knn_graph(emb, k=3)
    z, pred, mean, var, _ = engine.gmm_transduce(emb, probs, idx, sim, lam=1.0, iters=10, z_iters=5, var_floor=1e-8)
    f = torch.nn.functional.normalize(emb, dim=1).contiguous()
    z64, _, _, _, bound = R.transduce64(f, probs, idx, sim, 1.0, 10, 5, 1e-8)
    top2 = z64.topk(2, dim=1).values
    margin, ref = float((top2[:, 0] - top2[:, 1]).min()), z64.argmax(dim=1)
    before, after = float((probs.argmax(1).cpu() == y).float().mean()), float((ref.cpu() == y).float().mean())
    write_report("gmm_transduce.json", {"planted_clusters_reference": {"accuracy_before": before, "accuracy_after": after, "smallest_margin": margin,
                                                                       "largest_bound": bound},
                                        "kernel_accuracy": float((pred.cpu().long() == y).float().mean()),
                                        "largest_abs_difference": float((z.double() - z64).abs().max())})
    print(f"planted clusters: reference accuracy {before:.3f} -> {after:.3f}, smallest margin {margin:.3g}, largest bound {bound:.3g}")
    assert before < 0.75, "precondition: the text labels are already good"
    assert after == 1.0, "precondition: the float64 reference does not repair every label"
    assert margin > 100 * bound, "precondition: the reference's margins do not dominate the bound"
    assert torch.equal(pred.long(), ref), "the kernel's arg-max differs from the float64 reference's"
    assert torch.isfinite(mean).all() and (var >= 1e-8).all()
