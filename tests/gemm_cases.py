"""The case table of the f16 GEMM kernel tests ("f16 GEMM kernel tests"): which launches tests/test_gpu_gemm_kernels.py makes and which kernel
instantiation each of them must get.  Plain data and the call of the plan hook; no GPU.  tests/test_host_gemm_ref.py runs the whole table through
grip_debug_gemm_plan and holds the set of kernels it names against the written-out list of what csrc/gemm.hip's launch_* helpers can launch.

A case: epi (the caller's id; 3 with stats = True is instantiated as 9), M, N, K, variant, family, and the options rot_rows, ldc3 (ldc = 3 N, the window N
columns in), out2, inplace, stats, hilo, ksplit, coop, stat_parts, budget (grip_set_cu_budget), knob ("" = default knobs), kernel = the instantiation the
plan must name, expect = fields of the plan line the case depends on."""
import ctypes

ALL = tuple(range(9))           # caller-visible epilogues; (3, stats) is the tenth
KNOBS = ("GRIP_GEMM_EMODE=0", "GRIP_GEMM_EMODE=111", "GRIP_GEMM_EMODE=241", "GRIP_GEMM_SD=0", "GRIP_GEMM_WSPEC=0", "GRIP_GEMM_COLGROUP=2")
FAMILY_OF_EPI = {0: "cancel", 1: "exact", 2: "randn", 3: "exact", 4: "onehot", 5: "randn", 6: "exact", 7: "randn", 8: "randn"}

# kernel tile shapes: name template ({e} = instantiated epilogue), tile rows T, forced variant, the two N, K / 64 in {smallest accepted, nst - 1, nst,
# nst + 1, 2 nst + 1} as far as the plan sends them to this kernel, fixed M edges where the kernel needs a minimum tile count
SHAPES = {
    "ringw32": dict(kern="gemm_ringw_kernel<{e}, 4, 1>", T=32, variant=0, Ns=(128, 384), Ks=(192, 256, 320, 576), Kbig=3072),
    "ringw64": dict(kern="gemm_ringw_kernel<{e}, 4, 2>", T=64, variant=4, Ns=(128, 384), Ks=(192, 256, 320, 576), Kbig=3072),
    "ringw128s": dict(kern="gemm_ringw_kernel<{e}, 3, 4>", T=128, variant=1, Ns=(128, 384), Ks=(128, 192, 256, 448)),
    "ringw128l": dict(kern="gemm_ringw_kernel<{e}, 5, 4>", T=128, variant=1, Ns=(128, 384), Ks=(832, 1088), Kbig=3072),
    "ringw96": dict(kern="gemm_ringw_kernel<{e}, 5, 3>", T=96, variant=0, Ns=(768,), Ks=(256, 320, 384, 704), Ms=(2783, 2784, 2785), epis=(3, 4)),
    "f16x2": dict(kern="gemm_f16_kernel<{e}, 2>", T=64, variant=4, Ns=(128, 384), Ks=(64, 128)),
    "f16x4": dict(kern="gemm_f16_kernel<{e}, 4>", T=128, variant=1, Ns=(128, 384), Ks=(64,)),
    "ring3": dict(kern="gemm_ring_kernel<{e}, 3>", T=64, variant=4, Ns=(768,), Ks=(128, 192, 256, 448), Ms=(2751, 2752, 2753)),
    "big256": dict(kern="gemm_big_kernel<{e}, 256, 256, 4>", T=256, variant=2, Ns=(256, 768), Ks=(128, 192, 320, 576), Kbig=3072),
    "big128": dict(kern="gemm_big_kernel<{e}, 256, 128, 3>", T=256, variant=3, Ns=(128, 384), Ks=(128, 192, 320, 576)),
    "k64x8": dict(kern="gemm_k64_kernel<{e}, 8, 8>", T=256, variant=5, Ns=(256, 768), Ks=(128, 192, 256, 320), Kbig=3072, nostats=True),
    "k64x6": dict(kern="gemm_k64_kernel<{e}, 8, 6>", T=192, variant=8, Ns=(256, 768), Ks=(128, 192, 256, 320), nostats=True),
    "k64p": dict(kern="gemm_k64p_kernel<{e}, {m}, {sd}>", T=256, variant=6, Ns=(256, 768), Ks=(128, 192, 256, 320), Kbig=3072),
}
# under GRIP_GEMM_WSPEC=0 the 128-column launches fall to the kernels without loader waves
WSPEC0 = {
    "f16x2": dict(kern="gemm_f16_kernel<{e}, 2>", T=64, variant=4, Ns=(128,), Ks=(64, 128), knob="GRIP_GEMM_WSPEC=0"),
    "f16x4": dict(kern="gemm_f16_kernel<{e}, 4>", T=128, variant=1, Ns=(128, 384), Ks=(64, 128, 192, 256), Kbig=3072, knob="GRIP_GEMM_WSPEC=0"),
    "ring4": dict(kern="gemm_ring_kernel<{e}, 4>", T=64, variant=4, Ns=(128, 384), Ks=(192, 256, 320, 576), Kbig=3072, knob="GRIP_GEMM_WSPEC=0"),
}


def k64p_form(epi_inst, knob, out2):
    """(EMODE, SD) of the persistent kernel for an instantiated epilogue under a knob set (gemm_plan.cpp plan_persistent, restated)."""
    if epi_inst not in (7, 8, 9):
        return 0, "false"
    default = {7: 4, 8: 2, 9: 1}[epi_inst]
    emode, sd = default, True
    if knob.startswith("GRIP_GEMM_EMODE="):
        v = int(knob.split("=")[1])
        emode = v if v < 100 else {7: v // 100, 8: (v // 10) % 10, 9: v % 10}[epi_inst]
    if knob == "GRIP_GEMM_SD=0":
        sd = False
    if epi_inst == 9 and emode in (2, 4):
        emode = 1
    if emode == 4 and out2:
        emode = 1
    sd = sd and emode == default
    return (emode if emode in (0, 2, 4) else 1), ("true" if sd else "false")


def m_pad_of(M):
    """Rows allocated for A: every tile height's last tile is covered (the plan reads it for the 96-, 192- and 256-row kernels)."""
    return max(-(-M // t) * t for t in (96, 192, 256))


def _case(group, shape, epi, M, N, K, family=None, **kw):
    c = dict(group=group, epi=epi, M=M, N=N, K=K, variant=shape["variant"], family=family or FAMILY_OF_EPI[epi], rot_rows=0, ldc3=False, out2=False, inplace=False,
             stats=False, hilo=False, ksplit=1, coop=False, stat_parts=0, budget=0, knob=shape.get("knob", ""), scalar=1.0, expect={})
    c.update(kw)
    e = 9 if (epi == 3 and c["stats"]) else epi
    m, sd = k64p_form(e, c["knob"], c["out2"])
    c["kernel"] = shape["kern"].format(e=e, m=m, sd=sd)
    c["id"] = "{group}-e{e}-{M}x{N}x{K}-{family}".format(e=e, **{k: c[k] for k in ("group", "M", "N", "K", "family")}) + "".join(
        "-" + k + (str(c[k]) if not isinstance(c[k], bool) else "") for k in ("rot_rows", "ldc3", "out2", "inplace", "hilo", "stat_parts", "budget") if c[k]) + (
        "-ks%d" % c["ksplit"] if c["ksplit"] > 1 else "") + ("-coop" if c["coop"] else "")
    return c


def shape_cases(group, sh):
    """One tile shape: every epilogue it has at an awkward shape (options spread over the epilogues) and on the exact families at T + 1; the M edges with the
    statistics-carrying residual epilogue and a one-hot A; the K list with the f32 store on `cancel` and the bias store on `exact`; the wrap case."""
    T, (N0, N1) = sh["T"], (sh["Ns"][0], sh["Ns"][-1])
    Ks = sh["Ks"]
    Kmid = Ks[len(Ks) // 2]
    Ms = sh.get("Ms") or (1, T - 1, T, T + 1, 2 * T + 5)
    stats_ok = not sh.get("nostats")
    epis = sh.get("epis") or ALL
    out = []
    big_m, edge_m = Ms[-1], Ms[-2]
    for i, epi in enumerate(epis):
        for stats in ((False, True) if (epi == 3 and stats_ok) else (False,)):
            opts = dict(rot_rows=i & 1, ldc3=(i % 3 == 1), out2=(epi in (2, 8) and i % 2 == 0), inplace=(epi == 3 and not stats), stats=stats,
                        scalar=0.375 if epi == 6 else 1.0)
            out.append(_case(group, sh, epi, big_m, N1, Kmid, "randn" if epi != 0 else "cancel", **opts))
            opts.update(rot_rows=1 - opts["rot_rows"], ldc3=not opts["ldc3"], out2=epi in (2, 8) and not opts["out2"], inplace=False,
                        scalar=0.5 if epi == 6 else 1.0)
            out.append(_case(group, sh, epi, edge_m, N0, Ks[0], "exact" if i % 2 == 0 else "onehot", **opts))
    for j, M in enumerate(Ms):
        out.append(_case(group, sh, 3, M, N0, Kmid, "exact", stats=stats_ok, rot_rows=j & 1))
        if 4 in epis:
            out.append(_case(group, sh, 4, M, N1, Ks[0], "onehot", ldc3=bool(j & 1)))
    for j, K in enumerate(Ks + ((sh["Kbig"],) if "Kbig" in sh else ())):
        if 0 in epis:
            out.append(_case(group, sh, 0, edge_m, N0, K, "cancel", rot_rows=j & 1))
        out.append(_case(group, sh, 3 if 1 not in epis else 1, T + 3 if "Ms" not in sh else Ms[0], N0, K, "exact"))
    if "Ms" not in sh:       # at least five tile rows at the shortest K: the row rotation (stride 2) wraps
        out.append(_case(group, sh, 3, 5 * T + 3, N0, Ks[0], "exact", stats=stats_ok, rot_rows=1))
        out.append(_case(group, sh, 0 if 0 in epis else 4, 5 * T + 3, N0, Ks[0], "onehot", rot_rows=1))
    seen, uniq = set(), []
    for c in out:
        if c["id"] not in seen:
            seen.add(c["id"])
            uniq.append(c)
    return uniq


def all_cases():
    cases = []
    for name, sh in SHAPES.items():
        cases += shape_cases(name, sh)
    # the 96-row form on the long walk (the 128-row rule's detour): residual epilogues only
    sh96 = SHAPES["ringw96"]
    for stats in (False, True):
        cases.append(_case("ringw96", sh96, 3, 2785, 768, 832, "randn", stats=stats))
    cases.append(_case("ringw96", sh96, 3, 2784, 768, 3072, "exact", stats=True))
    # ---- split-K (EPI_F32): factors 2, 3, 4, 8 on 32-, 64- and 128-row tiles, three slices per split (two on the 3-slot ring)
    for ks in (2, 3, 4, 8):
        for group, kern, variant, M, per in (("splitk", "gemm_ringw_kernel<0, 4, 1>", 0, 69, 3), ("splitk", "gemm_ringw_kernel<0, 4, 2>", 4, 133, 3),
                                             ("splitk", "gemm_ringw_kernel<0, 3, 4>", 1, 261, 2)):
            for fam in ("cancel", "exact"):
                cases.append(_case(group, dict(kern=kern, variant=variant), 0, M, 128 if fam == "exact" else 384, 64 * ks * per, fam, ksplit=ks, rot_rows=ks & 1))
    # ---- cooperative split-K: factors 2 and 4, with and without statistics, four slices per split
    for ks in (2, 4):
        for stats in (False, True):
            for fam, M, N in (("randn", 133, 384), ("exact", 65, 128)):
                cases.append(_case("coop", dict(kern="gemm_ringw_kernel<{e}, 4, 2>", variant=0), 3, M, N, 64 * ks * 4, fam, ksplit=ks, coop=True, stats=stats, rot_rows=1))
    # ---- stat_in: 2, 16, 17 and 20 partial pairs, inside a loader-wave kernel and finalised for the persistent one
    for parts in (2, 16, 17, 20):
        K = 64 * parts
        lw = dict(kern="gemm_ringw_kernel<{e}, %d, 4>" % (3 if K // 64 <= 12 else 5), variant=1)
        for epi in (7, 8):
            cases.append(_case("stat_in", lw, epi, 261, 384, K, "randn", stat_parts=parts, out2=epi == 8, rot_rows=1, expect=dict(finalize=0)))
            cases.append(_case("stat_in", SHAPES["k64p"], epi, 261, 256, K, "randn", stat_parts=parts, expect=dict(finalize=1)))
    # ---- the persistent kernel on 8 CUs: 1, 3, 8, 9 and 30 tiles (XCDs without a tile, unequal shares, workgroups walking several tiles)
    for M, N, tiles in ((200, 256, 1), (200, 768, 3), (2048, 256, 8), (2300, 256, 9), (2305, 768, 30)):
        for epi, fam, kw in ((7, "randn", {}), (8, "randn", dict(out2=True)), (3, "exact", dict(stats=True)), (1, "onehot", {}), (0, "cancel", {})):
            cases.append(_case("persistent8", SHAPES["k64p"], epi, M, N, 192, fam, budget=8, ldc3=(M >= 2300 and epi != 3), expect=dict(tiles=tiles, grid=8), **kw))
    # ---- the compensated residual stream on variants 4, 1 and 6
    for name in ("ringw64", "ringw128s", "k64p"):
        sh = SHAPES[name]
        T = sh["T"]
        for j, M in enumerate((1, T - 1, T, T + 1, 2 * T + 5)):
            cases.append(_case("hilo", sh, 3, M, sh["Ns"][j & 1], sh["Ks"][1], "exact" if j & 1 else "randn", stats=True, hilo=True, inplace=bool(j & 1), ldc3=j >= 3))
    # ---- knob sets: what each changes
    for knob in KNOBS[:4]:
        sh = dict(SHAPES["k64p"], knob=knob)
        for epi, fam, kw in ((7, "randn", {}), (7, "exact", {}), (8, "randn", {}), (8, "randn", dict(out2=True)), (3, "randn", dict(stats=True)), (3, "exact", dict(stats=True))):
            for M, N, budget in ((517, 768, 0), (2305, 256, 8)):
                cases.append(_case("knob", sh, epi, M, N, 192, fam, budget=budget, ldc3=budget == 8, **kw))
    for name, sh in WSPEC0.items():
        cases += [dict(c, group="knob") for c in shape_cases("wspec0_" + name, sh)]
    shc = dict(SHAPES["k64p"], knob="GRIP_GEMM_COLGROUP=2")
    for epi, fam, kw in ((7, "randn", {}), (3, "exact", dict(stats=True)), (1, "onehot", {})):
        cases.append(_case("knob", shc, epi, 16385, 512, 128, fam, expect=dict(colgroup=2, tiles=130), **kw))
    ids = [c["id"] + c["knob"] for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:4]
    return cases


def present_bits(c):
    e = c["epi"]
    return (1 if c["stats"] else 0) | (2 if c["stat_parts"] else 0) | (4 if e in (7, 8) else 0) | (8 if c["out2"] else 0) | (16 if c["coop"] else 0)


def ldc_of(c):
    return 3 * c["N"] if c["ldc3"] else c["N"]


def split_stride_of(c):
    return (c["M"] + 32) * ldc_of(c) if (c["ksplit"] > 1 and not c["coop"]) else 0


def plan(lib, c, m_pad=None, present=None):
    """(status, text) of grip_debug_gemm_plan for a case: the integers exactly as the launch passes them."""
    buf = ctypes.create_string_buffer(512)
    rc = lib.grip_debug_gemm_plan(c["epi"], c["M"], c["N"], c["K"], ldc_of(c), m_pad_of(c["M"]) if m_pad is None else m_pad, c["variant"],
                                  c["ksplit"] if c["ksplit"] > 1 else 0, 0, c["rot_rows"], present_bits(c) if present is None else present, c["stat_parts"],
                                  split_stride_of(c), c["budget"] or 256, buf, len(buf))
    return rc, buf.value.decode()


def kernel_of(text):
    return text.split(" grid ")[0]


def plan_fields(text):
    """The launch part of a plan line as integers: grid (x), tiles (tiles_m x tiles_n multiplied), colgroup, rot, finalize, variant."""
    w = text.split(" grid ")[1].split()
    f = dict(zip(["grid"] + w[1::2], w[0::2]))        # "56x4 block 512 lds 81920 ...": the grid's value comes first, then name / value pairs
    tm, tn = f["tiles"].split("x")
    out = {k: int(v) for k, v in f.items() if k not in ("grid", "tiles")}
    out["grid"], out["tiles"] = int(f["grid"].split("x")[0]), int(tm) * int(tn)
    return out


def plan_is_intended(c, rc, text):
    """The plan accepts the case, names its kernel, and has the launch fields the case is there for (c["expect"]: the colgroup walk, the finalising
    launch, the persistent kernel's tile count and grid)."""
    if rc != 0 or kernel_of(text) != c["kernel"]:
        return False
    f = plan_fields(text)
    return all(f[k] == v for k, v in c["expect"].items())
