"""The GEMM launcher's decision (csrc/gemm_plan.cpp) against the kernel table recorded from the commit before the plan existed -- no GPU needed.

tests/golden/gemm_plan_parent.json was written by tools/gemm_plan_record.py from a `rocprofv3 --kernel-trace` run of the old launcher (one launch per
row through the debug hooks, variant and knobs as listed): for every row grip_debug_gemm_plan must name exactly the kernel instantiation, grid and
workgroup size the trace shows, and refuse the refused shapes with the same status and message.  The trace's LDS column is the kernel's static LDS
(only gemm_f16_kernel has any); the dynamic LDS of a launch is not in a kernel trace, so it is held to the tile arithmetic of the named instantiation
instead: stages x (tile rows + tile columns) x K slice x 2 bytes (+ eight 4-KiB epilogue slabs for the persistent kernel), written out here independently.
The knob parts run one process per setting: the library reads its GRIP_GEMM_* switches once."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "golden", "gemm_plan_parent.json")
KNOBS = ["GRIP_GEMM_R32=0", "GRIP_GEMM_R96=0", "GRIP_GEMM_R96=1", "GRIP_GEMM_R128=0", "GRIP_GEMM_WSPEC=0", "GRIP_GEMM_RING=0", "GRIP_GEMM_RING=3", "GRIP_GEMM_RING=4",
         "GRIP_GEMM_BIG=2", "GRIP_GEMM_BIG=5", "GRIP_GEMM_BIG=6", "GRIP_GEMM_KSPLIT=1", "GRIP_GEMM_KSPLIT=2", "GRIP_GEMM_KSPLIT=4", "GRIP_COOP_SPLIT=1", "GRIP_COOP_SPLIT=2",
         "GRIP_GEMM_EMODE=111", "GRIP_GEMM_SD=0"]


def _table():
    with open(TABLE) as f:
        return json.load(f)


def dynamic_lds(kernel):
    """Dynamic LDS bytes of one instantiation from its template arguments (csrc/gemm.hip: the kernels' own LDS layouts)."""
    name, args = re.fullmatch(r"(gemm_\w+_kernel)<(.*)>", kernel).groups()
    a = [x.strip() for x in args.split(",")]
    if name == "gemm_f16_kernel":
        return 0                                                   # two static stages
    if name == "gemm_ring_kernel":
        return int(a[1]) * (64 + 128) * 64 * 2                     # NST slots of a 64-row A tile + a 128-row W tile, 64 wide, f16
    if name == "gemm_ringw_kernel":
        return int(a[1]) * (32 * int(a[2]) + 128) * 64 * 2         # NST slots, 32 WMF rows
    if name == "gemm_big_kernel":
        return int(a[3]) * (int(a[1]) + int(a[2])) * 32 * 2        # NSTAGE slots of BMT + BNT rows, 32 wide
    if name == "gemm_k64_kernel":
        return 2 * (32 * int(a[2]) + 256) * 64 * 2                 # two stages of 32 RF + 256 rows, 64 wide
    if name == "gemm_k64p_kernel":
        return 2 * (256 + 256) * 64 * 2 + 8 * 4096                 # two stages + eight epilogue slabs: the whole 160 KiB
    raise AssertionError(kernel)


def check_rows(rows, n_cu, plan):
    """plan(row) -> (status, text).  Returns the number of rows checked."""
    assert rows
    for r in rows:
        status, text = plan(r)
        what = {k: r[k] for k in ("knob", "hook", "epi", "M", "N", "K", "m_pad", "variant", "ksplit", "present", "stat_parts", "rot_rows")}
        assert status == r["status"], (what, status, text)
        if r["status"]:
            assert text == r["error"], (what, text)
            continue
        m = re.fullmatch(r"(gemm_\w+_kernel<[^>]*>) grid (\d+)x(\d+) block (\d+) lds (\d+) static_lds (\d+) tiles .*", text)
        assert m, (what, text)
        got = dict(kernel=m.group(1), grid=[int(m.group(2)), int(m.group(3))], block=int(m.group(4)), static_lds=int(m.group(6)))
        want = {k: r[k] for k in got}
        assert got == want, (what, got, want)
        assert int(m.group(5)) == dynamic_lds(r["kernel"]), (what, text)
    return len(rows)


def _plan_fn(lib, n_cu):
    def plan(r):
        buf = ctypes.create_string_buffer(512)
        rc = lib.grip_debug_gemm_plan(r["epi"], r["M"], r["N"], r["K"], r["ldc"], r["m_pad"], r["variant"], r["ksplit"], r["f32"], r["rot_rows"], r["present"],
                                      r["stat_parts"], r["split_stride"], n_cu, buf, len(buf))
        if rc:
            assert lib.grip_last_error().decode() == buf.value.decode()
        return rc, buf.value.decode()
    return plan


def test_the_plan_names_the_recorded_kernel_for_every_default_row():
    import grip_amd  # noqa: F401
    from grip_amd import native
    for k in os.environ:
        assert not k.startswith(("GRIP_GEMM_", "GRIP_COOP_SPLIT", "GRIP_KROT_M")), f"{k} is set: the default part of the table needs the default knobs"
    t = _table()
    rows = [r for r in t["rows"] if r["knob"] == ""]
    assert check_rows(rows, t["n_cu"], _plan_fn(native.lib(), t["n_cu"])) >= 500
    # what the table must cover: every kernel family, the refused shapes, the pool-encode chunk on the persistent kernel's three default instantiations
    kernels = {r["kernel"] for r in rows if not r["status"]}
    for fam in ("gemm_f16_kernel", "gemm_ring_kernel", "gemm_ringw_kernel", "gemm_big_kernel", "gemm_k64_kernel", "gemm_k64p_kernel"):
        assert any(k.startswith(fam) for k in kernels), fam
    assert {"gemm_k64p_kernel<7, 4, true>", "gemm_k64p_kernel<8, 2, true>", "gemm_k64p_kernel<9, 1, true>"} <= {r["kernel"] for r in rows if r["M"] == 260040}
    assert sum(1 for r in rows if r["status"]) >= 4


_CHILD = """
import json, sys
sys.path.insert(0, {repo!r})
sys.path.insert(0, {tests!r})
import grip_amd
from grip_amd import native
import test_host_gemm_plan as T
t = T._table()
rows = [r for r in t["rows"] if r["knob"] == {knob!r}]
print("checked", T.check_rows(rows, t["n_cu"], T._plan_fn(native.lib(), t["n_cu"])))
"""


@pytest.mark.parametrize("knob", KNOBS)
def test_the_plan_names_the_recorded_kernel_under_a_knob(knob):
    name, value = knob.split("=")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("GRIP_GEMM_", "GRIP_COOP_SPLIT", "GRIP_KROT_M"))}
    env[name] = value
    script = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), knob=knob)
    p = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "checked" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_every_knob_part_of_the_table_is_tested():
    assert {r["knob"] for r in _table()["rows"]} == set(KNOBS) | {""}
