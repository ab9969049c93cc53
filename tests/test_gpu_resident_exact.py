"""Exact integer sweep of the resident-W kernels of csrc/skinny.hip on the GPU: proj_kernel
(exact fp32, split-bf16, bf16), pair_kernel, pair_x3_kernel, pair_bf16_kernel and dx_kernel,
every instantiation of the host dispatch, at the smallest row counts at which each item
schedule exists (tests/resident_ref.py: whole tiles only, tail parts only with and without
item-less waves, rounds followed by a ragged tail, the split-bf16 cut-over).

Every case first asks the library which kernel family the call takes (msha_*_route: the
launch's own decision -- the tiled fallback yields the same integers, so a case that cannot
tell which kernel ran proves nothing) and then compares EVERY element bit for bit with the
fp64 reference (np.array_equal; no tolerance, no fraction clause).  Operands are small
integers, every product, partial sum, score dot and gradient an integer below 2^24
(tests/test_resident_host.py), so the fp32 MFMA, the bf16 MFMA and the split-bf16 forms
(an integer |x| <= 8, and a hadamard product <= 64, is its own ``hi`` term) owe the fp64
result in any summation order: one dropped, duplicated or misplaced element fails.  A bf16 h
is the fp64 product rounded once by torch; its scores are the fp64 dots of the rounded row.

Canaries: outputs are windows into NaN buffers with 16 guard rows either side, the gathered
tables windows (pitch > K) into NaN buffers wide enough that a wrong row offset reads NaN,
not memory outside the allocation.

The integer data leaves the ``mid`` and ``lo`` terms of the split forms zero, so one
unit-normal case per kernel family runs alongside under ``bounded_close``."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as G
import resident_ref as R
from gpu_helpers import U32, bounded_close
from gpu_helpers import wgrad_kernel  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
GUARD = R.GUARD_ROWS


def _ids(cs):
    return [c["name"] for c in cs]


@pytest.fixture(autouse=True)
def _default_routes():
    """MSHA_SKINNY and MSHA_PROJ_SPLIT_MIN_ROWS are read once per process: where the
    environment sets them off their defaults, the routes asserted here do not exist."""
    why = R.env_reason()
    if why:
        pytest.skip(why)


def dev(x, cuda, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(cuda)


def host(t):
    return t.detach().to(F64).cpu().numpy()


class Window:
    """(rows, cols) of pitch ``pitch`` inside a NaN-filled buffer with ``guard`` elements
    before and after (a multiple of 8 elements: the window keeps the buffer's 16-byte
    alignment for fp32 and bf16)."""

    def __init__(self, cuda, rows, cols, dtype=F32, pitch=None, guard=None, fill=None):
        pitch = cols if pitch is None else pitch
        guard = GUARD * pitch if guard is None else guard
        assert guard % 8 == 0 and pitch >= cols
        self.buf = torch.full((2 * guard + (rows - 1) * pitch + cols,), float("nan"), device=cuda,
                              dtype=dtype)
        self.win = self.buf.as_strided((rows, cols), (pitch, 1), guard)
        if fill is not None:
            self.win.copy_(dev(fill, cuda, dtype))
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask.as_strided((rows, cols), (pitch, 1), guard).fill_(False)

    def untouched(self):
        return bool(torch.isnan(self.buf[self.mask]).all())


def assert_equal(got, want, name):
    """Bit for bit (both exact in fp64); the message names the first difference."""
    got = host(got) if isinstance(got, torch.Tensor) else got
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        i = tuple(bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} elements differ, first at {i}: "
                             f"got {got[i]}, want {want[i]}")


# ---------------------------------------------------------------- project_scores forward
def proj_route(c_or_args, X, W, al, ar, h):
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    M, K, H, F = c_or_args
    sched = (ctypes.c_int32 * 3)()
    code = _lib.fn("msha_project_scores_route")(M, K, H, F, MF._code(X.dtype), X.data_ptr(),
                                                W.data_ptr(), _lib.ptr(al), _lib.ptr(ar),
                                                h.data_ptr(), sched)
    return code, tuple(sched)


def run_project(cuda, M, K, H, F, X, W, al, ar):
    """msha_project_scores(_bf16) into NaN-guarded windows: (route, sched, h, el, er
    windows); asserts nothing outside the windows was written."""
    from msha_gnn_amd import _lib

    bf = X.dtype == BF
    N = H * F
    oh = Window(cuda, M, N, X.dtype)
    ol = Window(cuda, M, H) if al is not None else None
    orr = Window(cuda, M, H) if ar is not None else None
    code, sched = proj_route((M, K, H, F), X, W, al, ar, oh.win)
    _lib.call("msha_project_scores_bf16" if bf else "msha_project_scores", M, K, H, F,
              X.data_ptr(), W.data_ptr(), _lib.ptr(al), _lib.ptr(ar), oh.win.data_ptr(),
              None if ol is None else ol.win.data_ptr(),
              None if orr is None else orr.win.data_ptr(), _lib.stream_handle(cuda))
    torch.cuda.synchronize()
    for o, nm in ((oh, "h"), (ol, "el"), (orr, "er")):
        assert o is None or o.untouched(), f"{nm}: wrote outside its window"
    return code, sched, oh.win, None if ol is None else ol.win, None if orr is None else orr.win


@pytest.mark.parametrize("c", R.PROJ_FWD_CASES, ids=_ids(R.PROJ_FWD_CASES))
def test_project_scores_forward_exact(cuda, c):
    """Every (K, N, FE) x {fp32, bf16} at 1,024 / 1,045 / 32,789 rows, fp32 also at 65,549
    (split-bf16); score options both / al only / ar only / none."""
    from msha_gnn_amd import functional as MF

    d = R.proj_fwd_ref(c)
    M, K, H, F = c["M"], c["K"], c["heads"], c["feat"]
    dt = BF if c["dt"] == "bf16" else F32
    X, W = dev(d["X"], cuda, dt), dev(d["W"], cuda, dt)
    al = None if d["al"] is None else dev(d["al"], cuda)
    ar = None if d["ar"] is None else dev(d["ar"], cuda)
    code, (waves, pt, _), h, el, er = run_project(cuda, M, K, H, F, X, W, al, ar)
    assert code == c["route"], f"{c['name']}: route {code}"
    kinds = R.schedule(M, waves, pt)[2]
    want = {1024: "whole", 1045: "tail", 32789: "rounds+tail", R.SPLIT_M: "rounds+tail"}[M]
    assert want in kinds, (c["name"], waves, pt, kinds)
    assert_equal(h, d["h"], c["name"] + " h")
    if el is not None:
        assert_equal(el, d["el"], c["name"] + " el")
    if er is not None:
        assert_equal(er, d["er"], c["name"] + " er")
    if ar is not None:   # the public entry: the same bits, and er marked as row-order
        out = MF.project_scores(X, W, al=al, ar=ar, heads=H, feat=F)
        assert out[-1]._msha_row_order is True
        assert_equal(out[-1], d["er"], c["name"] + " er (functional)")
        assert_equal(out[0], d["h"], c["name"] + " h (functional)")


# --------------------------------------------------------------- project_scores backward
def _leaf64(x):
    return torch.tensor(x, dtype=F64, requires_grad=True)


def run_backward(cuda, c, tag=""):
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    d = R.proj_bwd_arrays(c)
    M, K, N, H, F = c["M"], c["K"], c["N"], c["heads"], c["feat"]
    use = {"al": ("al",), "ar": ("ar",), "both": ("al", "ar")}[c["scores"]]
    names = ("X", "W") + use
    ts = {k: dev(d[k], cuda).requires_grad_(True) for k in names}
    rs = {k: _leaf64(d[k]) for k in names}
    outs = MF.project_scores(ts["X"], ts["W"], al=ts.get("al"), ar=ts.get("ar"), heads=H, feat=F)
    rh = rs["X"] @ rs["W"]
    refs = [rh] + [(rh.view(M, H, F) * rs[k]).sum(-1) for k in use]
    grads = [d["dh"]] + [d["dl"] if k == "al" else d["dr"] for k in use]
    assert len(outs) == len(refs)
    for got, want in zip(outs, refs):
        assert_equal(got, want.detach().numpy(), c["name"] + tag + " forward")
    gts = [dev(g, cuda) for g in grads]
    # the dX launch as functional's backward makes it: A = dh, B = W^T, a fresh dense C
    Wt = ts["W"].detach().t()
    probe = torch.empty(M, K, device=cuda)
    a2 = ts[use[1]].detach() if len(use) > 1 else None
    route = _lib.fn("msha_gemm_f32_head_outer_route")(
        M, K, N, gts[0].data_ptr(), gts[0].stride(0), gts[0].stride(1), Wt.data_ptr(),
        Wt.stride(0), Wt.stride(1), probe.data_ptr(), probe.stride(0), 0.0, 0, H, F,
        gts[1].data_ptr(), ts[use[0]].data_ptr(), _lib.ptr(a2))
    assert route == R.RESIDENT, f"{c['name']}: dX route {route}"
    sum((o * g).sum() for o, g in zip(outs, gts)).backward()
    sum((o * torch.tensor(g)).sum() for o, g in zip(refs, grads)).backward()
    for k in names:
        assert_equal(ts[k].grad, rs[k].grad.numpy(), f"{c['name']}{tag} d{k}")


_BWD_SMALL = [c for c in R.PROJ_BWD_CASES if c["M"] < 4096]
_BWD_LARGE = [c for c in R.PROJ_BWD_CASES if c["M"] >= 4096]


@pytest.mark.parametrize("c", _BWD_SMALL, ids=_ids(_BWD_SMALL))
def test_project_scores_backward_exact(cuda, c):
    """dX on dx_kernel (route asserted) for every (heads * feat, K_in) in {64, 128}^2 and
    every feat in {16, 32, 64, 128} dividing it, both score terms, d_el only, d_er only;
    dW, dal, dar alongside, all against torch fp64 on the same integers."""
    run_backward(cuda, c)


@pytest.mark.parametrize("c", _BWD_LARGE, ids=_ids(_BWD_LARGE))
def test_project_scores_backward_exact_rounds(cuda, wgrad_kernel, c):
    """32,789 rows: dx_kernel's round followed by a ragged tail; dW (and dal, dar with it)
    on the resident weight-gradient kernels at 128 x 128, under each of them."""
    run_backward(cuda, c, f" [{wgrad_kernel}]")


# ----------------------------------------------------------------------- msha_pair_linear
ACT_TRAIN = R.ACT_BIAS | R.ACT_RELU | R.ACT_DROPOUT


def pair_tables(cuda, d, dtype=F32, pitches=(4, 8)):
    """The two tables as windows of pitch K + 4 / K + 8 (bf16: + 8 / + 16) into NaN buffers
    whose guards hold more than a whole row either side."""
    K = d["A"].shape[1]
    pa, pb = K + pitches[0], K + pitches[1]
    return (Window(cuda, R.ROWS_A, K, dtype, pa, guard=2 * pa + 16, fill=d["A"]),
            Window(cuda, R.ROWS_B, K, dtype, pb, guard=2 * pb + 16, fill=d["B"]))


def keep_scale(cuda, P, N):
    """The kernels' own keep mask (keyed on p * N + n) times 1 / (1 - p) = 2."""
    from msha_gnn_amd import functional as MF

    keep = MF.dropout_keep_mask(P * N, R.DROP_P, R.DROP_SEED, cuda)
    keep = keep.cpu().numpy().astype(np.float64).reshape(P, N)
    assert 0.4 < keep.mean() < 0.6
    return 2.0 * keep


def run_pair(cuda, c, d, gi, gj, act, windowed, want_route=None):
    from msha_gnn_amd import _lib

    P, K, N = c["P"], c["K"], c["N"]
    ta, tb = pair_tables(cuda, d)
    W, b = dev(d["W"], cuda), dev(d["b"], cuda)
    ti, tj = torch.as_tensor(gi, device=cuda), torch.as_tensor(gj, device=cuda)
    out = Window(cuda, P, N)
    rows = (R.ROWS_A, R.ROWS_B) if windowed else (0, 0)
    args = (P, K, N, ta.win.data_ptr(), ta.win.stride(0), ti.data_ptr(), tb.win.data_ptr(),
            tb.win.stride(0), tj.data_ptr(), *rows, W.data_ptr())
    route = _lib.fn("msha_pair_linear_route")(*args, out.win.data_ptr())
    if want_route is not None:
        assert route == want_route, f"{c['name']}: route {route}"
    drop = act & R.ACT_DROPOUT
    _lib.call("msha_pair_linear", *args, b.data_ptr(), act, R.DROP_P if drop else 0.0,
              R.DROP_SEED if drop else 0, 0, out.win.data_ptr(), _lib.stream_handle(cuda))
    torch.cuda.synchronize()
    assert out.untouched(), f"{c['name']}: wrote outside the batch"
    assert not bool(torch.isnan(out.win).any()), f"{c['name']}: NaN (a read outside a table)"
    return out.win


@pytest.mark.parametrize("c", R.PAIR_CASES, ids=_ids(R.PAIR_CASES))
def test_pair_linear_exact(cuda, c):
    """pair_x3_kernel (row counts given) and pair_kernel (0) at 1,024 / 1,045 / 4,099 pairs:
    two tables of their own pitch and row count, the last row of each indexed, act = bias |
    relu | dropout(0.5)."""
    d = R.pair_arrays(c["K"], c["N"], c["P"])
    got = run_pair(cuda, c, d, d["gi"], d["gj"], ACT_TRAIN, c["form"] == "window", c["route"])
    want = np.maximum(R.pair_pre(d), 0.0) * keep_scale(cuda, c["P"], c["N"])
    assert_equal(got, want, c["name"])


@pytest.mark.parametrize("form", ["window", "plain"])
def test_pair_linear_sigmoid(cuda, form):
    """sigmoid(relu(z)) with z an exact integer: the only error is the sigmoid's, 2^-21
    absolute (derived at test_gpu_gemm_layouts.test_score_pairs_mlp_tiled: __expf's argument
    scaling and exp2, then one add and one divide on values <= 1)."""
    c = dict(name=f"pair-sigmoid-{form}", P=1045, K=128, N=64)
    d = R.pair_arrays(128, 64, 1045, bound=1, wbound=2)
    got = run_pair(cuda, c, d, d["gi"], d["gj"], R.ACT_BIAS | R.ACT_RELU | R.ACT_SIGMOID,
                   form == "window", R.SPLIT if form == "window" else R.RESIDENT)
    z = np.maximum(R.pair_pre(d), 0.0)
    assert 2 < z.max() < 60 and np.mean(z > 0) > 0.2
    err = np.abs(host(got) - 1.0 / (1.0 + np.exp(-z))).max()
    print(f"{c['name']}: max |err| {err:.3g} (bound {2.0 ** -21:.3g})")
    assert err <= 2.0 ** -21


@pytest.mark.parametrize("K,N", [(128, 128), (64, 64)])
def test_pair_linear_window_out_of_range_reads_zeros(cuda, K, N):
    """The windowed form's documented rule: an index outside [0, rows) reads zeros, so the
    pair scores act(bias).  Index == rows and index -1, on either table, in the first and
    in the ragged last tile; the tables sit inside NaN allocations with more than a row of
    guard either side, so a descriptor that let the row through would read NaN."""
    P = 1045
    c = dict(name=f"pair-oob-K{K}-N{N}", P=P, K=K, N=N)
    d = R.pair_arrays(K, N, P)
    gi, gj = d["gi"].copy(), d["gj"].copy()
    gi[[3, P - 2]] = R.ROWS_A, -1
    gj[[5, P - 4]] = -1, R.ROWS_B
    gi[7], gj[7] = R.ROWS_A, R.ROWS_B
    got = run_pair(cuda, c, d, gi, gj, R.ACT_BIAS | R.ACT_RELU, True, R.SPLIT)
    want = np.maximum(R.pair_pre(d, gi, gj), 0.0)
    for p in (3, 5, 7, P - 2, P - 4):
        assert np.array_equal(want[p], np.maximum(d["b"], 0.0))
    assert_equal(got, want, c["name"])


def _bf16_round(x):
    return R.bf16_round(x)


@pytest.mark.parametrize("c", R.PAIR_BF16_CASES, ids=_ids(R.PAIR_BF16_CASES))
def test_pair_linear_bf16_exact(cuda, c):
    """pair_bf16_kernel, all four (K, N), fp32 and bf16 scores, 1,045 pairs, the same act; a
    bf16 output is the exact result rounded once (torch's rounding)."""
    from msha_gnn_amd import _lib

    P, K, N = c["P"], c["K"], c["N"]
    d = R.pair_arrays(K, N, P)
    ta, tb = pair_tables(cuda, d, BF, pitches=(8, 16))
    W, b = dev(d["W"], cuda, BF), dev(d["b"], cuda)
    ti, tj = torch.as_tensor(d["gi"], device=cuda), torch.as_tensor(d["gj"], device=cuda)
    odt = BF if c["out"] == "bf16" else F32
    out = Window(cuda, P, N, odt)
    args = (P, K, N, ta.win.data_ptr(), ta.win.stride(0), ti.data_ptr(), tb.win.data_ptr(),
            tb.win.stride(0), tj.data_ptr(), W.data_ptr())
    route = _lib.fn("msha_pair_linear_bf16_route")(*args, out.win.data_ptr())
    assert route == R.RESIDENT, f"{c['name']}: route {route}"
    _lib.call("msha_pair_linear_bf16_ex", *args, b.data_ptr(), ACT_TRAIN, R.DROP_P, R.DROP_SEED, 0,
              1 if odt == BF else 0, out.win.data_ptr(), _lib.stream_handle(cuda))
    torch.cuda.synchronize()
    assert out.untouched(), f"{c['name']}: wrote outside the batch"
    want = np.maximum(R.pair_pre(d), 0.0) * keep_scale(cuda, P, N)
    assert_equal(out.win, _bf16_round(want) if odt == BF else want, c["name"])


# --------------------------------------------------------------------------- refusals
def test_refusals_fall_back(cuda):
    """What the resident kernels do not cover reports route 0 and still gives the exact
    integers on the tiled kernels: a base 4 bytes off, ldg % 4 != 0, 1,023 rows, feat 8
    for the fp32 scores."""
    from msha_gnn_amd import _lib

    K, H, F = 128, 8, 16
    N = H * F
    # --- projection: M = 1023; feat = 8; X 4 bytes off
    for name, M, h_, f_, off in (("M1023", 1023, H, F, 0), ("feat8", 1045, 16, 8, 0),
                                 ("X+4B", 1045, H, F, 1)):
        Xh, Wh = R.proj_X(M, K), R.proj_W(K, N)
        al, ar = R.score_vec("al", N, h_, f_), R.score_vec("ar", N, h_, f_)
        flat = torch.zeros(M * K + 4, device=cuda)
        X = flat[off:off + M * K].view(M, K)
        X.copy_(dev(Xh, cuda))
        code, sched, h, el, er = run_project(cuda, M, K, h_, f_, X, dev(Wh, cuda), dev(al, cuda),
                                             dev(ar, cuda))
        assert (code, sched) == (R.TILED, (0, 0, 0)), name
        href = Xh @ Wh
        assert_equal(h, href, f"refusal {name} h")
        assert_equal(el, R.head_dots(href, al), f"refusal {name} el")
        assert_equal(er, R.head_dots(href, ar), f"refusal {name} er")
    # --- pair scorer: P = 1023; a pitch that is no multiple of 4; a table 4 bytes off
    for name, P, pitches, off in (("P1023", 1023, (4, 8), 0), ("ldg%4", 1045, (6, 8), 0),
                                  ("G+4B", 1045, (4, 8), 1)):
        d = R.pair_arrays(K, 64, P)
        pa, pb = K + pitches[0], K + pitches[1]
        ta = Window(cuda, R.ROWS_A, K, F32, pa, guard=(2 * pa + 23) // 8 * 8, fill=d["A"])
        if off:   # the same values one element further on
            ta.win = ta.buf.as_strided((R.ROWS_A, K), (pa, 1), ta.win.storage_offset() + 1)
            ta.win.copy_(dev(d["A"], cuda))
        tb = Window(cuda, R.ROWS_B, K, F32, pb, guard=2 * pb + 16, fill=d["B"])
        W, b = dev(d["W"], cuda), dev(d["b"], cuda)
        ti, tj = torch.as_tensor(d["gi"], device=cuda), torch.as_tensor(d["gj"], device=cuda)
        out = Window(cuda, P, 64)
        args = (P, K, 64, ta.win.data_ptr(), pa, ti.data_ptr(), tb.win.data_ptr(), pb,
                tj.data_ptr(), R.ROWS_A, R.ROWS_B, W.data_ptr())
        assert _lib.fn("msha_pair_linear_route")(*args, out.win.data_ptr()) == R.TILED, name
        _lib.call("msha_pair_linear", *args, b.data_ptr(), R.ACT_BIAS | R.ACT_RELU, 0.0, 0, 0,
                  out.win.data_ptr(), _lib.stream_handle(cuda))
        torch.cuda.synchronize()
        assert out.untouched(), name
        assert_equal(out.win, np.maximum(R.pair_pre(d), 0.0), f"refusal {name}")


# ------------------------------------------------------------------ unit-normal cases
def _normal(name, shape):
    rng = np.random.default_rng(G.zlib.crc32(name.encode()))
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


# Split-bf16 forms: x = x_h + x_m + x_l with |x - (x_h + x_m + x_l)| <= 2^-27 |x|
# (csrc/skinny.hip), and of the nine term products the kernels drop ml, lm and ll, "<= 2^-26
# |x w| each" (|x_m| <= 2^-9 |x|, |x_l| <= 2^-17 |x|: ml and lm are <= 2^-26, ll <= 2^-34).
# Per product term the deterministic error is therefore at most 3 * 2^-26 for the dropped
# products plus 2 * 2^-27 for the two operands' own split remainders: 2^-24, which enters
# bounded_close as split_u (bound + split_u * sum |x| |w|).  The pair scorer splits the fp32
# hadamard product x_i * x_j, itself rounded once (2^-24 relative): split_u = 2^-23 there.
SPLIT_U = 3 * 2.0 ** -26 + 2 * 2.0 ** -27
# reduce levels on top of the K products: the score dots' in-piece fma chain and xor tree
# (<= feat terms), nothing else (no split-K in these kernels)
_NORMAL_PROJ = ([dict(name="normal-proj-f32", M=1045, K=128, N=128, heads=4, feat=32, dt="f32",
                      route=R.RESIDENT),
                 dict(name="normal-proj-bf16", M=1045, K=128, N=128, heads=4, feat=32, dt="bf16",
                      route=R.RESIDENT)]
                + [dict(name=f"normal-proj-split-K{K}-N{N}", M=R.SPLIT_M, K=K, N=N, heads=N // 32,
                        feat=32, dt="f32", route=R.SPLIT) for K in R.KS for N in R.KS])


@pytest.mark.parametrize("c", _NORMAL_PROJ, ids=_ids(_NORMAL_PROJ))
def test_project_scores_normal(cuda, c):
    """Unit-normal operands: h within 4 sqrt(K) 2^-24 sum |x| |w| (+ split_u for the
    split-bf16 form, + one bf16 rounding 2^-8 |h| for a bf16 h, see
    test_gpu_gemm_layouts.test_gemm_bf16_normal); the score dots, taken from the STORED h,
    within 4 sqrt(feat) 2^-24 sum |h| |a| of the fp64 dots of the kernel's own h."""
    M, K, N, H, F = c["M"], c["K"], c["N"], c["heads"], c["feat"]
    bf = c["dt"] == "bf16"
    rnd = _bf16_round if bf else (lambda x: x)
    Xh, Wh = rnd(_normal(c["name"] + "X", (M, K))), rnd(_normal(c["name"] + "W", (K, N)))
    al, ar = _normal(c["name"] + "al", (H, F)), _normal(c["name"] + "ar", (H, F))
    dt = BF if bf else F32
    code, _, h, el, er = run_project(cuda, M, K, H, F, dev(Xh, cuda, dt), dev(Wh, cuda, dt),
                                     dev(al, cuda), dev(ar, cuda))
    assert code == c["route"], c["name"]
    bounded_close(host(h), Xh @ Wh, np.abs(Xh) @ np.abs(Wh), K, 0.0, c["name"] + " h", u=U32,
                  store_u=2.0 ** -8 if bf else 0.0, split_u=SPLIT_U if code == R.SPLIT else 0.0)
    hs = host(h)
    for got, a, nm in ((el, al, "el"), (er, ar, "er")):
        bounded_close(host(got), R.head_dots(hs, a), R.head_dots(np.abs(hs), np.abs(a)), F, 0.0,
                      f"{c['name']} {nm}", u=U32)


@pytest.mark.parametrize("form", ["window", "plain"])
def test_pair_linear_normal(cuda, form):
    """Unit-normal tables and weight, act = bias: K terms, each the fp32-rounded hadamard
    x_i * x_j times w (two roundings a term), plus the bias add: nterms = 2 K + 1.  The
    windowed form splits the rounded hadamard and w into bf16 terms: split_u = 2^-23 (SPLIT_U
    above, doubled for the product's own rounding, which the split inherits)."""
    K, N, P = 128, 128, 1045
    c = dict(name=f"normal-pair-{form}", P=P, K=K, N=N)
    d = R.pair_arrays(K, N, P)
    d = dict(d, A=_normal("npA", (R.ROWS_A, K)), B=_normal("npB", (R.ROWS_B, K)),
             W=_normal("npW", (N, K)), b=_normal("npb", (N,)))
    got = run_pair(cuda, c, d, d["gi"], d["gj"], R.ACT_BIAS, form == "window",
                   R.SPLIT if form == "window" else R.RESIDENT)
    had = np.abs(d["A"][d["gi"]] * d["B"][d["gj"]])
    bounded_close(host(got), R.pair_pre(d), had @ np.abs(d["W"].T) + np.abs(d["b"]), 2 * K + 1, 0.0,
                  c["name"], u=U32, split_u=2.0 ** -23 if form == "window" else 0.0)


def test_dx_normal(cuda):
    """Unit-normal dX = (dh + d_el (x) al + d_er (x) ar) W^T on dx_kernel: N products of a
    three-term sum each (2 fma roundings inside a term)."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    M, K, H, F = 1045, 64, 4, 32
    N = H * F
    dh, W = _normal("ndx-dh", (M, N)), _normal("ndx-W", (K, N))
    dl, dr = _normal("ndx-dl", (M, H)), _normal("ndx-dr", (M, H))
    al, ar = _normal("ndx-al", (H, F)), _normal("ndx-ar", (H, F))
    t = {k: dev(v, cuda) for k, v in dict(dh=dh, W=W, dl=dl, dr=dr, al=al, ar=ar).items()}
    Wt = t["W"].t()
    probe = torch.empty(M, K, device=cuda)
    assert _lib.fn("msha_gemm_f32_head_outer_route")(
        M, K, N, t["dh"].data_ptr(), N, 1, Wt.data_ptr(), Wt.stride(0), Wt.stride(1),
        probe.data_ptr(), K, 0.0, 0, H, F, t["dl"].data_ptr(), t["al"].data_ptr(),
        t["ar"].data_ptr()) == R.RESIDENT
    got = MF.gemm_head_outer(t["dh"], Wt, 0, (H, F, t["dl"], t["al"], t["dr"], t["ar"]))
    terms = (dh, np.repeat(dl, F, 1) * al.reshape(-1), np.repeat(dr, F, 1) * ar.reshape(-1))
    bounded_close(host(got), sum(terms) @ W.T, sum(np.abs(x) for x in terms) @ np.abs(W.T),
                  N + 4, 0.0, "normal-dx", u=U32)


# --------------------------------------------------------------------------- coverage
def test_sweep_reaches_every_instance(msha):
    """Host queries only: the union of (K, N, FE, dtype, route) the forward table reaches is
    the full instantiation set of proj_kernel (54), the pair tables reach pair_kernel and
    pair_x3_kernel at all four (K, N) and pair_bf16_kernel at all four for both outputs, the
    backward table dx_kernel at all four; and every item schedule -- whole tiles only, tail
    parts only, rounds followed by a tail, a tail that leaves waves idle -- is reached for
    PT > 1 and for PT == 1.  (A wave with no item at all exists only for PT == 1:
    tests/test_resident_host.py::test_schedules.)"""
    from msha_gnn_amd import _lib

    base = 1 << 30
    seen, sched_seen = set(), set()
    for c in R.PROJ_FWD_CASES:
        sched = (ctypes.c_int32 * 3)()
        al = base if c["scores"] in ("both", "al") else None
        ar = base if c["scores"] in ("both", "ar") else None
        code = _lib.fn("msha_project_scores_route")(
            c["M"], c["K"], c["heads"], c["feat"], 1 if c["dt"] == "bf16" else 0, base, base, al, ar,
            base, sched)
        assert code == c["route"], c["name"]
        seen.add((c["K"], c["N"], c["FE"], c["dt"], code))
        for kind in R.schedule(c["M"], sched[0], sched[1])[2]:
            sched_seen.add((kind, sched[1] > 1, c["dt"] + ("-split" if code == R.SPLIT else "")))
    form = {"f32": ("f32", R.RESIDENT), "split": ("f32", R.SPLIT), "bf16": ("bf16", R.RESIDENT)}
    want = {(K, N, FE) + form[f] for K, N, FE, f in R.PROJ_INSTANCES}
    print(f"proj_kernel instances reached: {len(seen)} of {len(want)}")
    print("schedules reached:", sorted(sched_seen))
    assert seen == want and len(want) == 54
    for kind in ("whole", "tail", "rounds+tail", "idle"):
        for multi in (True, False):
            for f in ("f32", "bf16"):
                assert (kind, multi, f) in sched_seen, (kind, "PT > 1" if multi else "PT == 1", f)
            if kind in ("rounds+tail", "idle"):
                assert (kind, multi, "f32-split") in sched_seen
    assert ("no-item", False, "f32") in sched_seen and ("no-item", False, "bf16") in sched_seen

    pair = set()
    for c in R.PAIR_CASES:
        rows = (R.ROWS_A, R.ROWS_B) if c["form"] == "window" else (0, 0)
        code = _lib.fn("msha_pair_linear_route")(c["P"], c["K"], c["N"], base, c["K"] + 4, base,
                                                 base, c["K"] + 8, base, *rows, base, base)
        assert code == c["route"], c["name"]
        pair.add((c["K"], c["N"], {R.SPLIT: "pair_x3", R.RESIDENT: "pair"}[code]))
    assert pair == set(R.PAIR_INSTANCES)
    pbf = set()
    for c in R.PAIR_BF16_CASES:
        assert _lib.fn("msha_pair_linear_bf16_route")(c["P"], c["K"], c["N"], base, c["K"] + 8, base,
                                                      base, c["K"] + 16, base, base, base) == R.RESIDENT
        pbf.add((c["K"], c["N"], c["out"]))
    assert pbf == set(R.PAIR_BF16_INSTANCES)
    dx = set()
    for c in R.PROJ_BWD_CASES:
        Kd, Nd = c["N"], c["K"]     # dx_kernel's K is heads * feat, its N the input width
        assert _lib.fn("msha_gemm_f32_head_outer_route")(
            c["M"], Nd, Kd, base, Kd, 1, base, 1, Kd, base, Nd, 0.0, 0, c["heads"], c["feat"], base,
            base, None) == R.RESIDENT, c["name"]
        dx.add((Kd, Nd))
    assert dx == set(R.DX_INSTANCES)
    print(f"pair {len(pair)}, pair_bf16 {len(pbf)}, dx {len(dx)} instances reached")
