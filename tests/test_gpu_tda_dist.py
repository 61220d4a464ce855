"""The test-time streaming cache under two ranks: `predict` is sharded, the logits AND the image features are gathered in dataset order, and every rank
then runs the same stream over the whole set -- so two ranks (gloo, one device, the harness of test_gpu_dist.py) return, on both ranks, the rows one
process returns, bit for bit, on a ragged test set."""
import pickle
import subprocess
import sys

import pytest
import torch

from test_gpu_dist import _env, _port

pytestmark = pytest.mark.gpu

WORKER = r'''
import os, sys, pickle, torch
sys.path.insert(0, os.environ["GRIP_REPO"]); sys.path.insert(0, os.path.join(os.environ["GRIP_REPO"], "tests"))
import grip_amd
from grip_amd import dist as gdist
from grip_amd.data import TensorPoolDataset
from grip_amd.methods import TextualPrompt
from grip_amd.methods.main import synthetic_pool
from test_gpu_strategies import _conf
rank, ws = gdist.init_from_env()
classes, files, images, names = synthetic_pool(5, 5, 64, 3)
l2i = {c: i for i, c in enumerate(classes)}
conf = _conf(MODEL="textual_prompt", LEARNING_PARADIGM="ssl", BATCH_SIZE=4, TDA=True, TDA_POS_CAP=2, TDA_NEG_CAP=1, TDA_NEG_ENTROPY=(0.0, 1.0),
             TDA_NEG_MASK=(0.01, 1.0))
m = TextualPrompt(conf, l2i, classes, classes, classes, "cuda")
m.define_model(classes)
sub = TensorPoolDataset(files[:21], images[:21].cuda(), labels=names[:21], label_map=l2i)      # ragged: six batches of 4, the last one short
pred, logits = m.predict(sub, classes)
streams, counts = m.tda.streams, m.tda.plan["counts"].cpu()
m._tda_plain = True
plain = m.predict(sub, classes)[1]
m._tda_plain = False
with open(os.environ["GRIP_OUT"] + f".{rank}", "wb") as f:
    pickle.dump({"ws": ws, "pred": pred, "logits": logits, "plain": plain, "streams": streams, "counts": counts}, f)
gdist.barrier()
'''


def test_two_ranks_return_the_rows_of_one(tmp_path):
    script = tmp_path / "tda_worker.py"
    script.write_text(WORKER)
    env = _env(tmp_path)
    one = subprocess.run([sys.executable, str(script)], env=dict(env, GRIP_OUT=str(tmp_path / "single")), capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert one.returncode == 0, one.stderr[-3000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(_port()), str(script)], env=env, capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert two.returncode == 0, two.stderr[-3000:]
    ref = pickle.load(open(str(tmp_path / "single") + ".0", "rb"))
    r0 = pickle.load(open(str(tmp_path / "out") + ".0", "rb"))
    r1 = pickle.load(open(str(tmp_path / "out") + ".1", "rb"))
    assert ref["ws"] == 1 and r0["ws"] == r1["ws"] == 2 and ref["logits"].shape == (21, 5)
    assert not torch.equal(ref["logits"], ref["plain"]), "the stream changed nothing"
    assert ref["streams"] == 1 and int(ref["counts"][0]) > 0
    for r in (r0, r1):
        assert torch.equal(r["plain"], ref["plain"])
        assert torch.equal(r["logits"], ref["logits"]) and torch.equal(r["pred"], ref["pred"]), "the stream depends on the number of ranks"
        assert r["streams"] == 1 and torch.equal(r["counts"], ref["counts"])
