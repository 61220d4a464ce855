"""bench.py as the driver runs it: a plain run prints the headline line without what moved behind --full, its `value` and `ms_per_step`
describe the --steps timed steps, and --dump-outputs writes the last timed step's arrays -- the same ones in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _plain_run(tmp_path, tag):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--pool", "1320",
                        "--chunk", "220", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_plain_bench_run_is_lean_and_its_dumped_outputs_repeat(tmp_path):
    d, a = _plain_run(tmp_path, "a")
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["metric"].startswith("images/sec") and d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["value"] > 0 and abs(d["value"] - 1320 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert not {"roofline", "exact", "secondary", "cpu_baseline"} & set(d) and d["f16_mode_loop"] is None
    assert set(a) == {"pseudolabel_image_index", "pseudolabel_class", "prompt_prefix", "pool_embeddings_sample", "pool_embeddings_sample_rows"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values()) and sum(x.nbytes for x in a.values()) <= 64 << 20
    assert len(a["pseudolabel_image_index"]) == len(a["pseudolabel_class"]) == d["config"]["selected_pairs"] > 0
    assert a["pool_embeddings_sample"].shape == (1320, 512) and np.isfinite(a["pool_embeddings_sample"]).all()
    assert a["prompt_prefix"].shape == (1, 16, 512) and np.isfinite(a["prompt_prefix"]).all()
    _, b = _plain_run(tmp_path, "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
