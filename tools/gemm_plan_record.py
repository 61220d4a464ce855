"""Record which kernel every GEMM shape of the case list gets, from a kernel trace of a built library.

    python tools/gemm_plan_record.py --lib menghini-neurips23-code_amd/libgrip_amd.so --out tests/golden/gemm_plan_parent.json

For every part (the default knobs, then one process per GRIP_* knob setting) the tool runs itself under `rocprofv3 --kernel-trace`: the child drives
grip_debug_gemm / _ln / _train / _splitk with one launch per row, and the parent joins the trace's kernel name, grid, workgroup and LDS columns with the
rows.  tests/golden/gemm_plan_parent.json was written this way from the commit BEFORE csrc/gemm_plan.cpp existed; tests/test_host_gemm_plan.py holds
gemm_plan to it on the CPU.  Run it on a new library and diff the two tables (`--compare OLD.json`) before touching a tile rule.

The trace's LDS column is the kernel's static LDS (49 152 / 65 536 bytes for gemm_f16_kernel, 0 for the kernels that take theirs at launch): the
dynamic bytes of a launch are not in a kernel trace.  The test checks them against the tile arithmetic instead.

Needs only ctypes (no torch): device buffers come from the HIP runtime the library itself links.  Buffers are uninitialised; only the launches matter.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
N_CU = 256      # MI355X; recorded in the table, the plan's grid of the persistent kernel depends on it


def up(x, m):
    return (x + m - 1) // m * m


# ---- rows: what each debug hook (csrc/tower.hip) puts into GemmArgs, as the inputs of grip_debug_gemm_plan
P_STAT_PART, P_STAT_IN, P_ROWSTAT, P_OUT2, P_COOP = 1, 2, 4, 8, 16


def row(hook, epi, M, N, K, m_pad=None, variant=0, ksplit=0, rot=0, present=0, stat_parts=0, split_stride=0):
    return dict(hook=hook, epi=epi, M=M, N=N, K=K, ldc=N, m_pad=m_pad if m_pad is not None else up(M, 256), variant=variant, ksplit=ksplit, f32=0, rot_rows=rot,
                present=present, stat_parts=stat_parts, split_stride=split_stride)


def gemm(epi, M, N, K, variant=0, rot=0, out2=False, m_pad=None):
    return row("gemm", epi, M, N, K, m_pad, variant, rot=rot, present=P_OUT2 if out2 else 0)


def ln(epi, M, N, K, variant=0, stats=False, out2=False, m_pad=None):
    return row("gemm_ln", epi, M, N, K, m_pad, variant, present=(P_STAT_PART if stats else 0) | (P_ROWSTAT if epi in (7, 8) else 0) | (P_OUT2 if out2 else 0))


def train(epi, M, N, K, stats=False, out2=False, stat_in=0, ksplit=0, coop=True, m_pad=None):
    present = (P_STAT_PART if stats else 0) | (P_ROWSTAT if epi in (7, 8) else 0) | (P_OUT2 if out2 else 0) | (P_STAT_IN if stat_in else 0) | (P_COOP if ksplit > 1 and coop else 0)
    return row("gemm_train", epi, M, N, K, m_pad, 0, ksplit=ksplit, rot=1, present=present, stat_parts=stat_in)


def splitk(M, N, K, ksplit=0, variant=0, rot=0, m_pad=None):        # ksplit = 0: gemm_pick_ksplit's factor (filled in by the child from *ksplit_used)
    r = row("gemm_splitk", 0, M, N, K, m_pad, variant, ksplit=ksplit, rot=rot)
    r["split_stride"] = r["m_pad"] * N
    r["pick_ksplit"] = ksplit == 0
    return r


def encoder_block(M, d, stats=True):      # QKV, out-proj, c_fc, c_proj of one block of a pool encode
    return [ln(7, M, 3 * d, d), ln(3, M, d, d, stats=stats), ln(8, M, 4 * d, d), ln(3, M, d, 4 * d, stats=stats)]


def prompt_step(M, d, coop_ks=0):
    rows = []
    # train-mode forward: folded QKV / c_fc reading the producer's partial sums, the pre-activation copy, residual GEMMs with statistics
    rows += [train(7, M, 3 * d, d, stat_in=d // 64), train(8, M, 4 * d, d, out2=True, stat_in=d // 64), train(7, M, 3 * d, d), train(8, M, 4 * d, d, out2=True),
             train(3, M, d, d, stats=True), train(3, M, d, 4 * d, stats=True), train(3, M, d, d), train(3, M, d, 4 * d)]
    if coop_ks != 1:
        rows += [train(3, M, d, 4 * d, stats=True, ksplit=coop_ks or -1)]      # -1: grip_debug_coop_split's factor
    # backward: input gradients (plain f16, GELU', f32 split-K), with the row rotation of the train-mode launches
    rows += [gemm(4, M, d, d, rot=1), gemm(4, M, 4 * d, d, rot=1), gemm(5, M, 4 * d, d, rot=1), gemm(4, M, d, 3 * d, rot=1), gemm(0, M, d, d, rot=1),
             splitk(M, d, 4 * d, rot=1), splitk(M, d, 3 * d, rot=1), splitk(M, d, d, rot=1)]
    return rows


EPILOGUE_TEST_SHAPES = [(128, 128, 64), (200, 384, 128), (3408, 2304, 768), (77 * 5, 512, 2048), (16, 512, 768), (50432, 768, 768), (12700, 2304, 768),
                        (25000, 768, 3072), (16500, 3072, 768), (50000, 512, 128)]


def default_rows():
    rows = []
    for images in (1320, 1160, 440):                       # a full bench chunk, the ragged tail of 50 000 images, a refinement-tier chunk (ViT-B/16, S = 197)
        rows += encoder_block(images * 197, 768)
    for B in (1320, 440, 64, 16):                          # conv1 of ViT-B/16 (K = 768), ViT-B/32 (3 072) and ViT-L/14 (588 -> 640)
        rows += [gemm(0, B * 196, 768, 768), gemm(0, B * 49, 768, 3072)]
    rows += [gemm(0, 256 * 576, 1024, 640), gemm(0, 16 * 576, 1024, 640)]
    for images in (256, 16):                               # ViT-L/14@336px: d = 1 024, S = 577
        rows += encoder_block(images * 577, 1024)
    for images in (1320, 64):                              # ViT-B/32: S = 50
        rows += encoder_block(images * 50, 768)
    rows += encoder_block(102 * 77, 512, stats=False) + [gemm(1, 102 * 77, 1536, 512), gemm(2, 102 * 77, 2048, 512), gemm(3, 102 * 77, 512, 2048)]   # text tower, inference
    rows += prompt_step(3408, 768) + prompt_step(425, 512) + prompt_step(2142, 512)
    for M in (16, 102, 1320):                              # the last block's row GEMMs (class-token rows only)
        rows += [gemm(1, M, 768, 768), gemm(3, M, 768, 768), gemm(2, M, 3072, 768), gemm(3, M, 768, 3072), ln(7, M, 768, 768), ln(8, M, 3072, 768), splitk(M, 768, 3072)]
    for d, S in ((128, 17), (256, 577), (128, 77), (256, 77)):      # the tiny and small test models, 2 and 8 images / 5 classes
        for B in (2, 8, 5):
            rows += encoder_block(B * S, d) + [gemm(1, B * S, 3 * d, d), gemm(2, B * S, 4 * d, d), gemm(3, B * S, d, 4 * d), splitk(B * S, d, 4 * d)]
    for (M, N, K) in EPILOGUE_TEST_SHAPES:                 # every forced variant on the shapes of test_gemm_epilogues
        for v in (0, 1, 2, 3, 4, 5, 6, 8):
            if (v in (2, 5, 6, 8) and N % 256) or (v in (2, 3, 5, 6, 8) and K < 128):
                continue
            rows += [gemm(e, M, N, K, variant=v, m_pad=up(M, 768)) for e in (0, 2, 3)] + [ln(3, M, N, K, variant=v, stats=True, m_pad=up(M, 768))]
            if v != 8:
                rows += [ln(7, M, N, K, variant=v, m_pad=up(M, 768))]
    # refused shapes: status and message
    rows += [gemm(1, 256, 192, 128), gemm(1, 256, 256, 96), train(3, 425, 512, 2048, ksplit=4, coop=False), train(7, 425, 1536, 512, stat_in=0)]
    rows[-1]["stat_parts"] = 8
    return rows


def knob_parts():
    vpt, text, text_l = (3408, 768), (425, 512), (2142, 512)
    small = lambda M, d: [gemm(4, M, d, d, rot=1), gemm(1, M, 3 * d, d), gemm(2, M, 4 * d, d), train(3, M, d, 4 * d, stats=True), train(3, M, d, d, stats=True), splitk(M, d, 4 * d, rot=1)]  # noqa: E731
    pool = encoder_block(1320 * 197, 768) + encoder_block(86680, 768) + [gemm(2, 260040, 3072, 768), train(8, 260040, 3072, 768, out2=True)]
    steps = small(*vpt) + small(*text) + small(*text_l)
    coop = [train(3, 425, 512, 2048, stats=True, ksplit=-1), train(3, 2142, 512, 2048, stats=True, ksplit=-1), train(3, 385, 512, 2048, ksplit=-1)]
    parts = [("GRIP_GEMM_R32=0", steps), ("GRIP_GEMM_R96=0", steps), ("GRIP_GEMM_R96=1", steps), ("GRIP_GEMM_R128=0", steps), ("GRIP_GEMM_WSPEC=0", steps),
             ("GRIP_GEMM_RING=0", steps), ("GRIP_GEMM_RING=3", steps), ("GRIP_GEMM_RING=4", steps),
             ("GRIP_GEMM_BIG=2", pool[:8] + [gemm(1, 16500, 3072, 768)]), ("GRIP_GEMM_BIG=5", pool[:8] + [gemm(1, 16500, 3072, 768)]), ("GRIP_GEMM_BIG=6", pool[:8] + [gemm(1, 16500, 3072, 768)]),
             ("GRIP_GEMM_KSPLIT=1", steps), ("GRIP_GEMM_KSPLIT=2", steps), ("GRIP_GEMM_KSPLIT=4", steps),
             ("GRIP_COOP_SPLIT=1", coop), ("GRIP_COOP_SPLIT=2", coop),
             ("GRIP_GEMM_EMODE=111", pool), ("GRIP_GEMM_SD=0", pool)]
    return parts


# ---- the child: one launch per row
def run_child(lib_path, rows_path):
    spec = json.load(open(rows_path))
    lib = ctypes.CDLL(lib_path)
    vp, ci, cf, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    lib.grip_debug_gemm.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, cf, ci, ci, vp]
    lib.grip_debug_gemm_ln.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.grip_debug_gemm_train.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, ci, vp]
    lib.grip_debug_gemm_splitk.argtypes = [vp, vp, ci, ci, ci, vp, ci, i64, vp, ci, ci, vp]
    lib.grip_debug_coop_split.argtypes = [ci, ci, ci]
    lib.grip_last_error.restype = ctypes.c_char_p
    lib.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    lib.hipMemset.argtypes = [vp, ci, ctypes.c_size_t]

    def dev(nbytes, zero=False):
        p = vp()
        assert lib.hipMalloc(ctypes.byref(p), nbytes) == 0, "hipMalloc"
        if zero:
            assert lib.hipMemset(p, 0, nbytes) == 0
        return p

    rows = spec["rows"]
    need = lambda f: max(f(r) for r in rows)  # noqa: E731
    A = dev(need(lambda r: r["m_pad"] * r["K"] * 2))
    W = dev(need(lambda r: r["N"] * r["K"] * 2))
    big = need(lambda r: r["m_pad"] * r["N"] * 4 * (8 if r["hook"] == "gemm_splitk" else 1))     # f32 [m_pad, N], eight partials under split-K
    out, out2, resid = dev(big), dev(big), dev(big)
    bias = dev(need(lambda r: r["N"] * 4))
    colsum = dev(need(lambda r: r["N"] * 4))
    stat = dev(need(lambda r: (r["N"] // 64 + 1) * r["m_pad"] * 8))
    stat_in = dev(need(lambda r: (max(r["stat_parts"], r["K"] // 64) + 1) * r["m_pad"] * 8), zero=True)
    rowstat = dev(need(lambda r: r["m_pad"] * 8), zero=True)
    scratch = dev(256 * 32768 + 4096)
    counter = dev(4096 * 4, zero=True)
    results = []
    for r in rows:
        M, N, K, Mp, pr = r["M"], r["N"], r["K"], r["m_pad"], r["present"]
        var = r["variant"] | (r["rot_rows"] << 8)
        if r["hook"] == "gemm":
            rc = lib.grip_debug_gemm(r["epi"], A, W, M, N, K, bias, resid, resid, out, out2 if pr & P_OUT2 else None, 1.0, Mp, var, None)
        elif r["hook"] == "gemm_ln":
            rc = lib.grip_debug_gemm_ln(r["epi"], A, W, M, N, K, bias, resid, out, out2 if pr & P_OUT2 else None, stat if pr & P_STAT_PART else None,
                                        rowstat if pr & P_ROWSTAT else None, colsum, Mp, r["variant"], None)
        elif r["hook"] == "gemm_train":
            if r["ksplit"] == -1:
                r["ksplit"] = lib.grip_debug_coop_split(M, N, K)
                if r["ksplit"] > 1:
                    r["present"] = pr = pr | P_COOP
            rc = lib.grip_debug_gemm_train(r["epi"], A, W, M, N, K, bias, resid, out, out2 if pr & P_OUT2 else None, stat if pr & P_STAT_PART else None,
                                           rowstat if pr & P_ROWSTAT else None, colsum, stat_in if pr & P_STAT_IN else None, r["stat_parts"], r["ksplit"],
                                           scratch if pr & P_COOP else None, counter if pr & P_COOP else None, Mp, None)
        else:
            used = ci(0)
            rc = lib.grip_debug_gemm_splitk(A, W, M, N, K, out, r["ksplit"], r["split_stride"], ctypes.byref(used), Mp, var, None)
            r["ksplit"] = used.value
        r.pop("pick_ksplit", None)
        r["status"] = rc
        if rc:
            r["error"] = lib.grip_last_error().decode()
        results.append(r)
    assert lib.hipDeviceSynchronize() == 0, "a launch failed"
    json.dump(results, open(spec["results"], "w"))


# ---- the parent: trace each part, join
def kernel_rows(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, f"expected one kernel trace under {trace_dir}, found {files}"
    recs = list(csv.DictReader(open(files[0])))
    recs.sort(key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in recs:
        name = r["Kernel_Name"]
        if name.startswith("_Z"):
            name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        m = re.search(r"(gemm_\w+_kernel<[^>]*>)", name)
        if not m:
            continue        # ln_stats_finalize and the like
        wx, wy = int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"])
        out.append(dict(kernel=m.group(1), grid=[int(r["Grid_Size_X"]) // wx, int(r["Grid_Size_Y"]) // wy], block=wx, static_lds=int(r["LDS_Block_Size"])))
    return out


def record(lib_path, parts):
    table = []
    for knob, rows in parts:
        with tempfile.TemporaryDirectory() as tmp:
            spec = dict(rows=rows, results=os.path.join(tmp, "results.json"))
            json.dump(spec, open(os.path.join(tmp, "rows.json"), "w"))
            env = dict(os.environ)
            if knob:
                k, v = knob.split("=")
                env[k] = v
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "--",
                   sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, "rows.json"), "--lib", os.path.abspath(lib_path)]
            subprocess.run(cmd, env=env, check=True, timeout=300, stdout=subprocess.DEVNULL)
            results = json.load(open(spec["results"]))
            kernels = kernel_rows(os.path.join(tmp, "trace"))
            launched = [r for r in results if r["status"] == 0]
            assert len(launched) == len(kernels), f"{knob or 'default'}: {len(launched)} launches, {len(kernels)} GEMM kernels in the trace"
            for r, k in zip(launched, kernels):
                r.update(k)
            for r in results:
                r["knob"] = knob
            table += results
            print(f"{knob or 'default'}: {len(results)} rows, {len(kernels)} launches", flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(HERE, "..", "menghini-neurips23-code_amd", "libgrip_amd.so"))
    ap.add_argument("--out")
    ap.add_argument("--compare", help="an earlier table: exit 1 unless every row is equal")
    ap.add_argument("--child")
    ap.add_argument("--list", action="store_true", help="print the row counts and exit (no GPU)")
    a = ap.parse_args()
    if a.child:
        return run_child(a.lib, a.child)
    parts = [("", default_rows())] + knob_parts()
    if a.list:
        print({k or "default": len(r) for k, r in parts}, sum(len(r) for _, r in parts))
        return 0
    table = dict(n_cu=N_CU, rows=record(a.lib, parts))
    if a.out:
        with open(a.out, "w") as f:
            f.write('{"n_cu": %d, "rows": [\n%s\n]}\n' % (N_CU, ",\n".join(json.dumps(r, sort_keys=True) for r in table["rows"])))
    if a.compare:
        old = json.load(open(a.compare))["rows"]
        diff = [(o, n) for o, n in zip(old, table["rows"]) if o != n]
        for o, n in diff[:20]:
            print("DIFF\n  old", json.dumps(o, sort_keys=True), "\n  new", json.dumps(n, sort_keys=True))
        print(f"{len(table['rows'])} rows against {len(old)}: {len(diff)} differ")
        return 1 if diff or len(old) != len(table["rows"]) else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
