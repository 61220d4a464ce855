"""The N > 1 path on the GPU box (which has ONE GPU): two ranks share cuda:0 and talk over gloo
(GRIP_SINGLE_DEVICE=1, GRIP_DIST_BACKEND=gloo).  Checks that the sharded pool encode + all-gather returns the
embeddings of a single-process run in dataset order (ragged last shard included), that both ranks build the
same pseudolabel lists, and that bench.py's multi-rank branch runs end to end and prints one JSON line."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

WORKER = r'''
import os, sys, pickle, torch
sys.path.insert(0, os.environ["GRIP_REPO"])
import grip_amd
from grip_amd import clip, dist as gdist, pseudolabels as pl, rng
rank, ws = gdist.init_from_env()
m, _ = clip.load("small", device="cuda")
n = 101
x = torch.from_numpy(rng.normal(5, rng.stream_id("dist.x"), (n, 3, 64, 64))) + 2 * torch.from_numpy(rng.normal(5, rng.stream_id("dist.mu"), (n, 3, 1, 1)))
with torch.no_grad():
    emb = pl.encode_pool(m.visual.tower, x, chunk=16)
    # the trained-model pass of GRIP (assign_pseudo_labels): the same sharded encode with a visual prompt
    prefix = torch.from_numpy(rng.normal(5, rng.stream_id("dist.prefix"), (1, 4, 256), 0.0, 0.05)).cuda()
    emb_p = pl.encode_pool(m.visual.tower, x, chunk=16, prefix=prefix)
    txt = m.encode_text(clip.tokenize(["a", "b c", "d e f", "g"]).cuda())
lists = pl.pseudolabel_from_features(emb, txt, 100.0, [f"p{i:03d}" for i in range(n)], [0, 1, 2, 3], 5)
# screen and refine across ranks: each rank re-encodes the marked rows of its own shard, one small all-gather per round
twin = m.exact_twin()
with torch.no_grad():
    txt32 = twin.encode_text(clip.tokenize(["a", "b c", "d e f", "g"]).cuda())
    e32 = twin.encode_image(x.cuda())
ident = pl.identical_lists(m.visual.tower, twin.visual.tower, x, txt32, 100.0, [f"p{i:03d}" for i in range(n)], [0, 1, 2, 3], 5, chunk=16, exact_chunk=8)
exact = pl.pseudolabel_from_features(e32, txt32, 100.0, [f"p{i:03d}" for i in range(n)], [0, 1, 2, 3], 5)
refined = (pl.LAST_REFINE_STATS["rows_refined"], pl.LAST_REFINE_STATS["rows_refined_this_rank"])
g = torch.ones(3, device="cuda") * (rank + 1)
gdist.allreduce_mean_([g])
with open(os.environ["GRIP_OUT"] + f".{rank}", "wb") as f:
    pickle.dump({"emb": emb.cpu(), "emb_p": emb_p.cpu(), "lists": lists, "g": g.cpu(), "ws": ws, "ident": ident, "exact": exact, "refined": refined}, f)
gdist.barrier()
'''


TRAINER = r'''
import os, sys, pickle, torch
sys.path.insert(0, os.environ["GRIP_REPO"]); sys.path.insert(0, os.path.join(os.environ["GRIP_REPO"], "tests"))
import grip_amd
from grip_amd import dist as gdist
from grip_amd.data import TensorPoolDataset
from grip_amd.methods import TextualPrompt, VisualPrompt
from grip_amd.methods.main import synthetic_pool
from test_gpu_strategies import _conf
rank, ws = gdist.init_from_env()
out = {"ws": ws}
classes, files, images, names = synthetic_pool(4, 24, 64, 3)          # 96 images: three steps of 32 per epoch
l2i = {c: i for i, c in enumerate(classes)}
for tag, cls, model in (("vpt", VisualPrompt, "visual_prompt"), ("coop", TextualPrompt, "textual_prompt")):
    conf = _conf(MODEL=model, LEARNING_PARADIGM="ssl", EPOCHS=2, LR=0.05, BATCH_SIZE=32 // ws, GRAPH_STEPS=os.environ.get("GRIP_T_GRAPH", "1") == "1")
    data = TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i)
    m = cls(conf, l2i, classes, classes, classes, "cuda")
    m.define_model(classes)
    loader = m._loader(data, True)
    stats = [m._train_epoch(loader) for _ in range(2)]
    out[tag] = (m.unwrap_model().prefix.detach().cpu(), stats, len(loader), m.initial_prefix.reshape(m.unwrap_model().prefix.shape).clone())
    # evaluation loops on a RAGGED pool (85 of the 96 images, batch 16 on every rank count): frame / validation accuracy / logits
    m.config.BATCH_SIZE = 16
    sub = TensorPoolDataset(files[:85], images[:85].cuda(), labels=names[:85], label_map=l2i)
    df = m.test_predictions(sub)
    ev = m.evaluation(sub)
    out[tag + "_eval"] = (list(df["id"]), list(df["class"]), m._run_validation(sub), ev[0], ev[1], ev[2])
with open(os.environ["GRIP_OUT"] + f".{rank}", "wb") as f:
    pickle.dump(out, f)
gdist.barrier()
'''


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env(tmp_path):
    return dict(os.environ, GRIP_SINGLE_DEVICE="1", GRIP_DIST_BACKEND="gloo", GRIP_REPO=REPO, GRIP_OUT=str(tmp_path / "out"), PYTHONPATH=REPO,
                HSA_ENABLE_IPC_MODE_LEGACY="0")


def test_sharded_encode_allgather_matches_single_process(tmp_path):
    import pickle
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = _env(tmp_path)
    one = subprocess.run([sys.executable, str(script)], env=dict(env, GRIP_OUT=str(tmp_path / "single")), capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-3000:]
    ref = pickle.load(open(str(tmp_path / "single") + ".0", "rb"))
    r0 = pickle.load(open(str(tmp_path / "out") + ".0", "rb"))
    r1 = pickle.load(open(str(tmp_path / "out") + ".1", "rb"))
    assert ref["ws"] == 1 and r0["ws"] == 2
    assert torch.equal(r0["emb"], ref["emb"]) and torch.equal(r1["emb"], ref["emb"])     # rows are independent of the chunking
    assert torch.equal(r0["emb_p"], ref["emb_p"]) and torch.equal(r1["emb_p"], ref["emb_p"]) and not torch.equal(ref["emb_p"], ref["emb"])
    assert r0["lists"] == ref["lists"] and r1["lists"] == ref["lists"]
    # identical mode: the exact lists on one rank and on two, with the re-encoding work split between the shards
    assert ref["ident"] == ref["exact"] and r0["ident"] == ref["exact"] and r1["ident"] == ref["exact"]
    assert r0["refined"][0] == r1["refined"][0] == r0["refined"][1] + r1["refined"][1] and ref["refined"][0] == ref["refined"][1]
    assert torch.allclose(r0["g"], torch.full((3,), 1.5)) and torch.allclose(r1["g"], torch.full((3,), 1.5))


@pytest.mark.parametrize("graph", ["1", "0"])
def test_trainer_is_data_parallel_like_accelerate(tmp_path, graph):
    """TrainingStrategy under N ranks = the reference under `accelerate launch`: every rank takes its OWN batches of BATCH_SIZE
    (dist.rank_batches), gradients are averaged -- so two ranks x batch 16 walk the same global batches of 32 as one rank x batch 32 (plain mean CE:
    row weights 1/32) and end an epoch with the same prompts up to summation order; and the evaluation loops (test_predictions / evaluation /
    _run_validation: sharded, gathered, padded duplicates dropped, textual_prompt.py:239, 285-294) return the single-process results on a ragged pool."""
    import pickle
    script = tmp_path / "trainer.py"
    script.write_text(TRAINER)
    env = dict(_env(tmp_path), GRIP_T_GRAPH=graph)
    one = subprocess.run([sys.executable, str(script)], env=dict(env, GRIP_OUT=str(tmp_path / "single")), capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), str(script)], env=env, capture_output=True, text=True, timeout=1200, cwd=tmp_path)
    assert two.returncode == 0, two.stderr[-3000:]
    ref = pickle.load(open(str(tmp_path / "single") + ".0", "rb"))
    r0 = pickle.load(open(str(tmp_path / "out") + ".0", "rb"))
    r1 = pickle.load(open(str(tmp_path / "out") + ".1", "rb"))
    assert ref["ws"] == 1 and r0["ws"] == r1["ws"] == 2
    for tag in ("vpt", "coop"):
        p_ref, st_ref, nb_ref, p_init = ref[tag]
        moved = float((p_ref - p_init).norm())
        assert moved > 0.02 * float(p_init.norm())                       # (the six steps did move the prompt)
        for r in (r0, r1):
            p, st, nb, _ = r[tag]
            assert nb == nb_ref == 3                                     # three optimizer steps per epoch either way
            # same global batches, same mean gradient -- up to the f16 rounding of two half-batch backwards against one (the prompt gradients are
            # accurate to a cosine of 0.999 against fp32 autograd: tests/test_gpu_backward.py), i.e. a few percent of the distance travelled
            assert float((p - p_ref).norm()) <= 5e-2 * moved, (tag, float((p - p_ref).norm()), moved)
            for (l, a), (l_ref, a_ref) in zip(st, st_ref):
                assert abs(l - l_ref) <= 2e-3 * max(1.0, abs(l_ref)) and abs(a - a_ref) <= 2.01 / 96, (tag, st, st_ref)
        assert torch.equal(r0[tag][0], r1[tag][0])                       # both ranks hold the same prompts, bit for bit
        e_ref = ref[tag + "_eval"]
        for r in (r0, r1):
            e = r[tag + "_eval"]
            assert e[0] == e_ref[0] and e[3] == e_ref[3] and len(e[0]) == 85      # the frame's ids / the evaluation's image list: dataset order, no duplicates
            assert torch.allclose(e[5], e_ref[5], rtol=2e-3, atol=5e-2)              # logits (100 x cosine; the two runs hold prompts equal to ~1e-4)
            agree = sum(a == b for a, b in zip(e[1], e_ref[1])) / 85
            assert agree >= 0.97 and abs(e[2] - e_ref[2]) <= 0.03, (tag, agree, e[2], e_ref[2])


def test_bench_two_ranks(tmp_path):
    """`bench.py --gpus 2` as the driver launches it (two ranks sharing this box's GPU over gloo): the JSON line, and -- so that the first run on a
    real multi-GPU node can only fail on RCCL, not on plumbing -- the exchange steps of the timed pass read from $GRIP_COMM_TRACE:
    exactly ONE all-gather of the pool embeddings, one all-gather per re-encode call of a refinement tier, one broadcast per bounded scan
    (root-placed), one all-gather of the selected training images, one gradient all-reduce per prompt step; and stage (iv) walks the shards
    dist.rank_batches deals (the 102-step / 13-step arithmetic of DESIGN 6 at this size)."""
    from grip_amd import dist as gdist
    env = dict(_env(tmp_path), GRIP_COMM_TRACE=str(tmp_path / "comm.log"))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--pool", "1320", "--chunk", "220", "--full"], env=env, capture_output=True, text=True, timeout=1200, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["selected_pairs"] > 0 and "cpu_baseline" not in d
    assert d["roofline"]["bound"] == "mfma" and d["roofline"]["achieved"] > 0
    # the default mode carries the index guarantee on N ranks too (each rank re-encodes the marked rows of its own shard)
    assert d["config"]["pseudolabel_mode"] == "identical" and d["identical"]["rows_reencoded_exactly"] > 0 and d["identical_images_per_sec"] > 0
    st = d["stage_seconds_over_ranks"]
    assert set(st) == {"encode_f16", "allgather", "head_scan", "refine_split", "refine_exact", "train"} and all(v["max_s"] >= v["min_s"] >= 0 for v in st.values())
    assert d["identical"]["tiers"] == 3 and d["identical"]["rows_reencoded_split_f16"] >= d["identical"]["rows_reencoded_exactly"]
    assert [r["rank"] for r in d["ranks_seen"]] == [0, 1] and len(d["ranks_seen"]) == 2
    m_pairs, n_steps = d["config"]["selected_pairs"], d["config"]["prompt_steps_per_pass"]
    assert n_steps == len(gdist.rank_batches(range(m_pairs), 16, 0, 2)) == len(gdist.rank_batches(range(m_pairs), 16, 1, 2)) == -(-(-(-m_pairs // 16)) // 2)
    for r in (0, 1):
        mine = [l.split(" ", 1)[1] for l in open(tmp_path / "comm.log").read().splitlines() if l.startswith(f"rank{r} ")]
        timed = mine[mine.index("marker timed_begin") + 1: mine.index("marker timed_end")]
        count = lambda key: sum(key in l for l in timed)      # noqa: E731
        assert count("allgather tag=pool_embeddings") == 1, timed
        assert count("allgather tag=refined_rows") == d["identical"]["tier_calls"] > 0, (timed, d["identical"])
        assert count("broadcast ") == d["identical"]["scans"] > 0, timed
        assert count("allgather tag=train_images") == 1, timed
        assert count("allreduce_mean ") == n_steps, (count("allreduce_mean "), n_steps)
        assert len(timed) == 2 + d["identical"]["tier_calls"] + d["identical"]["scans"] + n_steps, timed      # ... and nothing else


def test_bench_strong_scaling_mode_and_native_comm_single_rank(tmp_path):
    """--strong splits --pool over the ranks (2 x 660); and a 1-rank run under a launcher with GRIP_NATIVE_COMM=1 sends the bench's
    all-gather and gradient all-reduce through the C ABI's own RCCL communicator (grip_allgather_embeddings / grip_allreduce_mean)."""
    env = _env(tmp_path)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--pool", "1320", "--strong", "--chunk", "220", "--no-exact", "--no-secondary"], env=env, capture_output=True, text=True, timeout=1200, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "strong" and d["config"]["pool_images_per_gpu"] == 660 and d["config"]["pool_images_total"] == 1320
    env1 = dict(os.environ, PYTHONPATH=REPO, GRIP_NATIVE_COMM="1", HSA_ENABLE_IPC_MODE_LEGACY="0", GRIP_COMM_TRACE=str(tmp_path / "comm.log"))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                          "--pool", "1320", "--chunk", "220", "--no-exact", "--no-secondary", "--no-cpu-baseline"], env=env1, capture_output=True, text=True,
                         timeout=1200, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["value"] > 0
    calls = open(tmp_path / "comm.log").read()
    assert "allgather" in calls and "allreduce" in calls, calls


def test_native_rccl_communicator_single_rank():
    """The C ABI's RCCL entry points (grip_comm_*, grip_allgather_embeddings, grip_allreduce_mean) execute on this box's one
    GPU: a 1-rank communicator is created through RCCL, the all-gather returns the local rows, the mean all-reduce is the
    identity.  (More than one rank per GPU is refused by RCCL itself; the N > 1 data path is covered over gloo above and its
    RCCL form is measured by the driver's multi-GPU bench.)"""
    import grip_amd  # noqa: F401
    from grip_amd import dist as gdist
    torch.cuda.set_device(0)
    c = gdist.NativeComm()
    try:
        assert (c.rank, c.ws) == (0, 1)
        local = torch.randn(37, 512, device="cuda")
        out = c.allgather(local, 37)
        g = torch.randn(8192, device="cuda")
        want = g.clone()
        c.allreduce_mean_(g)
        torch.cuda.synchronize()
        assert torch.equal(out, local) and torch.equal(g, want)
    finally:
        c.close()
