"""The cache head (csrc/cache_head.hip: grip_cache_head_forward / _backward) element by element against float64 on the same f32 inputs.

Bounds (u = 2^-24, f^ = f / |f| in float64, s = f^ . k, T_ij = sum_d |f^_id k_jd|, x = beta (1 - s), A = exp(-x), n_y keys in class y):
    r_ij           = beta (2 e + 8) u T_ij + (2 |x_ij| + 4) u
                     (an f32 dot of e terms in any order and the f32 row norm, carried through the exponential; the f32 evaluation of x and of exp)
    forward  |err| <= alpha sum_{j in y} v_j A_ij (r_ij + (n_y + 2) u) + u |ref_iy|       (class sum + two scalings; the final add into the logit)
    backward |err| <= alpha beta v_j sum_i |G_{i,y(j)}| A_ij |f^_id| (r_ij + (n + e + 8) u) + 2^-126
Nothing in them comes from a measurement.  Every element is asserted; the worst |err| / bound per output goes to tests/_out/cache_head.json.

Every operand is followed by NaN guard rows, grad_keys is NaN-prefilled, and the guard rows of both outputs must stay NaN.  Layouts are stated
relative to the kernels' key tiles: 64 keys forward (FWD_TILE), 16 keys backward."""
import ctypes

import pytest
import torch

from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 8
U = 2.0 ** -24
FWD_TILE = 64
_REPORT = {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(x):
    """x followed by GUARD rows of NaN in one allocation: the view of the owned rows."""
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), float("nan"), device="cuda", dtype=torch.float32)
    buf[:x.shape[0]] = x
    return buf, buf[:x.shape[0]]


def _workspace(lib, native, n, m, c, e):
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_cache_head_workspace(n, m, c, e, ctypes.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")


def _forward(f, k, cs, v, alpha, beta, logits):
    native, lib = _lib()
    (n, e), m, c = f.shape, k.shape[0], cs.numel() - 1
    _, fv = _padded(f)
    _, kv = _padded(k)
    vv = None if v is None else _padded(v)[1]
    obuf, out = _padded(logits)
    ws = _workspace(lib, native, n, m, c, e)
    native.check(lib.grip_cache_head_forward(_p(fv), _p(kv), _p(cs), _p(vv), alpha, beta, n, m, c, e, _p(out), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), "forward: an owned row is not finite"
    assert torch.isnan(obuf[n:]).all(), "forward: a guard row was written"
    return out


def _backward(f, k, cs, v, alpha, beta, G):
    native, lib = _lib()
    (n, e), m, c = f.shape, k.shape[0], cs.numel() - 1
    _, fv = _padded(f)
    _, kv = _padded(k)
    _, gv = _padded(G)
    vv = None if v is None else _padded(v)[1]
    dbuf = torch.full((m + GUARD, e), float("nan"), device="cuda")
    ws = _workspace(lib, native, n, m, c, e)
    native.check(lib.grip_cache_head_backward(_p(fv), _p(kv), _p(cs), _p(vv), alpha, beta, n, m, c, e, _p(gv), _p(dbuf), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(dbuf[:m]).all(), "backward: an owned row was not written (or is not finite)"
    assert torch.isnan(dbuf[m:]).all(), "backward: a guard row was written"
    return dbuf[:m]


def _inputs(n, sizes, e, weighted, seed):
    g = torch.Generator().manual_seed(seed)
    m, c = sum(sizes), len(sizes)
    f = torch.randn(n, e, generator=g) * (0.1 + 29.9 * torch.rand(n, 1, generator=g))
    k = torch.randn(m, e, generator=g)
    k = k / k.norm(dim=1, keepdim=True) * (1 + 0.1 * torch.randn(m, 1, generator=g))
    v = 2 * torch.rand(m, generator=g) if weighted else None
    logits = 10 * torch.randn(n, c, generator=g)
    G = torch.randn(n, c, generator=g)
    cs = torch.zeros(c + 1, dtype=torch.int32)
    cs[1:] = torch.cumsum(torch.tensor(sizes), 0)
    dev = lambda t: None if t is None else t.cuda()      # noqa: E731
    return dev(f), dev(k), dev(v), dev(logits), dev(G), cs.cuda()


def _reference(f, k, cs, v, alpha, beta, logits, G):
    """float64 forward, backward and the two bounds of the module docstring."""
    (n, e), m, c = f.shape, k.shape[0], cs.numel() - 1
    sizes = (cs[1:] - cs[:-1]).long()
    y = torch.repeat_interleave(torch.arange(c, device="cuda"), sizes)      # class of key j
    M = torch.zeros(m, c, dtype=torch.float64, device="cuda")
    M[torch.arange(m, device="cuda"), y] = 1
    fh = f.double() / f.double().norm(dim=1, keepdim=True)
    kd = k.double()
    vd = torch.ones(m, dtype=torch.float64, device="cuda") if v is None else v.double()
    s, T = fh @ kd.T, fh.abs() @ kd.abs().T
    x = beta * (1 - s)
    A = torch.exp(-x)
    r = beta * (2 * e + 8) * U * T + (2 * x.abs() + 4) * U
    ref = logits.double() + alpha * (A * vd) @ M
    fb = alpha * (A * vd * (r + (sizes[y].double() + 2) * U)) @ M + U * ref.abs()
    Gk = G.double()[:, y]
    dk = alpha * beta * vd[:, None] * ((Gk * A).T @ fh)
    bb = alpha * beta * vd[:, None] * ((Gk.abs() * A * (r + (n + e + 8) * U)).T @ fh.abs()) + 2.0 ** -126
    return ref, fb, dk, bb


def _check(case, what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    _REPORT.setdefault(case, {})[what] = round(ratio, 4)
    write_report("cache_head.json", _REPORT)
    print(f"{case} {what}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{case} {what}: |err| is {ratio:.2f} x its bound"


# class layouts (keys per class), relative to the forward's 64-key tile and the backward's 16-key tile
LAYOUTS = {
    "one_class_all_keys": [2 * FWD_TILE + 6],                       # c = 1: one segment across three tiles, carried twice
    "one_key_per_class_c5": [1] * 5,                                # c = 5
    "one_key_per_class_c102": [1] * 102,                            # c = 102: 64 classes in the first tile
    "empty_start_middle_end": [0, 30, 0, 40, 0],                    # class 3 straddles the tile boundary at 64 (keys 30 .. 69)
    "straddle": [20, 50, 10, 47, 3],                                # class 1 straddles key 64, class 3 straddles key 128
    "m_below_tile_multiple": [20, 50, 10, 47],                      # m = 127
    "m_above_tile_multiple": [20, 50, 10, 48, 1],                   # m = 129: the last tile holds one key
    "c102_ragged": [(7 * y) % 4 for y in range(102)],               # c = 102 with empty classes everywhere, m = 153
}
HYPER = [(1.0, 1.0), (1.0, 5.5), (3.0, 5.5)]
CASES = [(name, n, e, HYPER[i % 3], bool((i // 3 + i) % 2))
         for i, (name, n, e) in enumerate((name, n, e) for name in LAYOUTS for n in (1, 17, 130) for e in (64, 512, 768))]


@pytest.mark.parametrize("name,n,e,hyper,weighted", CASES, ids=[f"{c[0]}-n{c[1]}-e{c[2]}-a{c[3][0]:g}-b{c[3][1]:g}-{'v' if c[4] else 'nov'}" for c in CASES])
def test_forward_and_backward_against_float64(name, n, e, hyper, weighted):
    alpha, beta = hyper
    f, k, v, logits, G, cs = _inputs(n, LAYOUTS[name], e, weighted, seed=n * 1000 + e)
    ref, fb, dk, bb = _reference(f, k, cs, v, alpha, beta, logits, G)
    case = f"{name}.n{n}.e{e}.a{alpha:g}.b{beta:g}.{'v' if weighted else 'nov'}"
    _check(case, "logits", _forward(f, k, cs, v, alpha, beta, logits), ref, fb)
    _check(case, "grad_keys", _backward(f, k, cs, v, alpha, beta, G), dk, bb)


@pytest.mark.parametrize("hyper,weighted", [((1.0, 1.0), False), ((1.0, 5.5), True), ((3.0, 5.5), False)])
def test_more_classes_than_the_cosine_head_takes(hyper, weighted):
    """c = 1 030 > 1 024 (the cosine head's limit), one key per class and a few classes without: classes are walked with the key tiles, any c."""
    alpha, beta = hyper
    sizes = [0 if y % 103 == 5 else 1 for y in range(1030)]
    f, k, v, logits, G, cs = _inputs(17, sizes, 64, weighted, seed=1030)
    ref, fb, dk, bb = _reference(f, k, cs, v, alpha, beta, logits, G)
    case = f"c1030.n17.e64.a{alpha:g}.b{beta:g}.{'v' if weighted else 'nov'}"
    _check(case, "logits", _forward(f, k, cs, v, alpha, beta, logits), ref, fb)
    _check(case, "grad_keys", _backward(f, k, cs, v, alpha, beta, G), dk, bb)


def test_exact_statements_forward():
    sizes = LAYOUTS["empty_start_middle_end"]
    n = 130
    f, k, v, logits, _, cs = _inputs(n, sizes, 64, True, seed=5)
    out = _forward(f, k, cs, v, 3.0, 5.5, logits)
    for y, sz in enumerate(sizes):
        if sz == 0:
            assert torch.equal(out[:, y], logits[:, y]), f"the column of empty class {y} changed"
        else:
            assert not torch.equal(out[:, y], logits[:, y])
    assert torch.equal(_forward(f, k, cs, v, 0.0, 5.5, logits), logits), "alpha = 0 changed a logit"
    assert torch.equal(_forward(f, k, cs, v, 3.0, 5.5, logits), out), "two runs differ"
    # rows 0 .. n - 1 in one call == the same rows in two calls (70 + 60: the second call's rows sit at other places of a row tile)
    two = torch.cat([_forward(f[:70], k, cs, v, 3.0, 5.5, logits[:70]), _forward(f[70:], k, cs, v, 3.0, 5.5, logits[70:])])
    assert torch.equal(two, out), "a row's bits depend on the call it is in"
    assert torch.equal(_forward(f[129:], k, cs, v, 3.0, 5.5, logits[129:]), out[129:]), "a row's bits depend on n"


def test_rows_do_not_depend_on_the_class_split():
    """With few row tiles the forward deals the classes to several workgroups per row tile (up to one per key tile, until ~512 workgroups exist): three
    shares at n = 130, two at n = 17 000, one at n = 33 000 for these three key tiles.  The same rows come out with the same bits."""
    sizes = LAYOUTS["straddle"]
    f, k, v, logits, _, cs = _inputs(33000, sizes, 64, True, seed=8)
    whole = _forward(f, k, cs, v, 3.0, 5.5, logits)
    for n in (130, 17000):
        assert torch.equal(_forward(f[:n], k, cs, v, 3.0, 5.5, logits[:n]), whole[:n]), f"rows 0 .. {n - 1} differ from the same rows of the 33 000-row call"
    ref, fb, _, _ = _reference(f[:130], k, cs, v, 3.0, 5.5, logits[:130], torch.zeros(130, len(sizes), device="cuda"))
    _check("split.n33000", "logits", whole[:130], ref, fb)


def test_exact_statements_backward():
    sizes = LAYOUTS["straddle"]
    f, k, v, _, G, cs = _inputs(130, sizes, 64, True, seed=6)
    G[:, 1] = 0
    G[:, 4] = 0
    dk = _backward(f, k, cs, v, 3.0, 5.5, G)      # (grad_keys is NaN-prefilled by _backward: every owned element was overwritten)
    start = cs.tolist()
    for y in range(len(sizes)):
        rows = dk[start[y]:start[y + 1]]
        if y in (1, 4):
            assert (rows == 0).all(), f"class {y}: its column of G is zero but grad_keys is not"
        else:
            assert (rows != 0).any()
    assert torch.equal(_backward(f, k, cs, v, 3.0, 5.5, G), dk), "two runs differ"


def test_refusals():
    """Bad arguments return an error and a message; nothing is launched (the logits and grad_keys buffers keep their bits)."""
    native, lib = _lib()
    n, m, c = 4, 6, 2
    cs = torch.tensor([0, 3, 6], dtype=torch.int32, device="cuda")
    logits = torch.randn(n, c, device="cuda")
    before = logits.clone()
    dk = torch.full((m, 4096), float("nan"), device="cuda")
    G = torch.randn(n, c, device="cuda")
    big = torch.randn(n + m, 4096, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(rc, word):
        assert rc != 0
        msg = lib.grip_last_error().decode()
        assert word in msg, msg

    def both(e, word, keys=True, ws_bytes=None):
        f, k = big[:n, :e].contiguous(), big[n:, :e].contiguous()
        nb = ws.numel() if ws_bytes is None else ws_bytes
        refused(lib.grip_cache_head_forward(_p(f), _p(k if keys else None), _p(cs), None, 1.0, 5.5, n, m, c, e, _p(logits), _p(ws), nb, _stream()), word)
        refused(lib.grip_cache_head_backward(_p(f), _p(k if keys else None), _p(cs), None, 1.0, 5.5, n, m, c, e, _p(G), _p(dk), _p(ws), nb, _stream()), word)

    both(6, "e = 6")
    both(4096, "e = 4096")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_cache_head_workspace(n, m, c, 64, ctypes.byref(nbytes)))
    both(64, "workspace too small", ws_bytes=nbytes.value - 1)
    both(64, "null pointer", keys=False)
    refused(lib.grip_cache_head_workspace(n, m, c, 6, ctypes.byref(nbytes)), "e = 6")
    refused(lib.grip_cache_head_workspace(0, m, c, 64, ctypes.byref(nbytes)), "n = 0")
    torch.cuda.synchronize()
    assert torch.equal(logits, before) and torch.isnan(dk).all()
