"""Exact layout sweep of the tiled GEMMs (csrc/gemm.hip, csrc/gemm_bf16.hip) and of the ops
that run on them, on the GPU.

Exact arithmetic is the main check: operands are small integers (tests/gemm_ref.py), every
product and partial sum an integer below 2^24 (tests/test_gemm_host.py holds the tables to
that), so the fp32 MFMA, the bf16 MFMA and the split-bf16 weight-gradient kernel (every
value its own ``hi`` term) owe the fp64 product bit for bit in any summation order: a
dropped, duplicated or misplaced element fails, and no tolerance is involved.  A bf16 C is
compared with the reference rounded once to bf16 by torch (the kernels' ``from_f32`` is the
compiler's float -> __bf16 conversion, round to nearest even like torch's: no case needs a
bound).  One unit-normal case per loader runs alongside under ``bounded_close``.

Canaries: every operand is a window into a buffer of NaN (before, after and in the pitch
padding), so an unmasked out-of-range read turns the result NaN; every output that the API
lets the caller pass is a window (``ldc >= N``) into a buffer of NaN that must stay NaN
outside the M x N window.

Every case asks the library which operand staging it takes (msha_gemm_f32_loader /
msha_gemm_bf16_loader, the launch's own decision) and compares it with the documented
rule (gemm_ref.predict_*); the last test holds the union over the tables to the full set
of loaders."""
import numpy as np
import pytest
import torch

import gemm_ref as G
from gpu_helpers import BF16_SPLIT2, U32, bounded_close, tol_close
from gpu_helpers import wgrad_kernel  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
BF16_RNE = 2.0 ** -8  # largest relative error of one round-to-nearest to bf16 (see below)


def _ids(cs):
    return [c["name"] for c in cs]


def dev_view(v, dev, dtype=F32):
    """(whole buffer, window) of a gemm_ref.View on the device."""
    buf = torch.as_tensor(v.buf).to(dtype).to(dev)
    return buf, buf.as_strided(v.shape, v.strides, v.start)


def plain(x, dev, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).to(dev)


def lib_loader(name, A, B):
    from msha_gnn_amd import _lib

    return _lib.fn(name)(A.shape[0], B.shape[1], A.shape[1], A.data_ptr(), A.stride(0),
                         A.stride(1), B.data_ptr(), B.stride(0), B.stride(1))


def check_out(buf, O, want, name):
    """The window equals ``want`` bit for bit and the NaN sentinel around it is intact."""
    got = buf.float().cpu().numpy().astype(np.float64)
    win = got[O.index()]
    bad = np.argwhere(win != want)
    assert bad.size == 0, (f"{name}: {len(bad)} of {win.size} elements differ, first at "
                           f"{tuple(bad[0])}: got {win[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
    assert np.isnan(got[O.outside()]).all(), f"{name}: wrote outside the M x N window"


def run_f32(cuda, c):
    from msha_gnn_amd import functional as MF

    A, B, ref = G.case_operands(c)
    _, tA = dev_view(A, cuda)
    _, tB = dev_view(B, cuda)
    want = G.predict_f32(c["M"], c["N"], c["K"], *G.case_strides(c, 4))
    assert lib_loader("msha_gemm_f32_loader", tA, tB) == want == c["loader"]
    prior = G.case_prior(c)
    O = G.out_view(c["M"], c["N"], c["ldc"], c["coff"], prior)
    obuf, tO = dev_view(O, cuda)
    MF.gemm(tA, tB, out=tO, accumulate=c["accumulate"], splits=c["splits"])
    check_out(obuf, O, ref if prior is None else ref + prior, c["name"])


# ----------------------------------------------------------------- fp32 msha_gemm_f32
@pytest.mark.parametrize("c", G.F32_CASES, ids=_ids(G.F32_CASES))
def test_gemm_f32_exact(cuda, c):
    """The four 16-byte loaders over ragged tiles, the scalar loader by each cause alone,
    split-K (used < splits, ragged last chunk, accumulate) and the store epilogues."""
    run_f32(cuda, c)


@pytest.mark.parametrize("c", G.WGRAD_CASES, ids=_ids(G.WGRAD_CASES))
def test_gemm_f32_wgrad_exact(cuda, wgrad_kernel, c):
    """M = N = 128, A = X^T, splits = 16: the resident weight-gradient kernels (split-bf16
    and exact fp32), K a multiple of 16, of neither 4 nor 16, of 4; beta 0 and 1."""
    run_f32(cuda, c)


def _normal(name, shape):
    rng = np.random.default_rng(G.zlib.crc32(name.encode()))
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


_NORMAL_F32 = [G._case(f"normal-f32-{code}", 132, 132, 100, G.spec(ao, off=off), G.spec(bo), code)
               for code, ao, bo, off in ((G.VEC | G.AK | G.BNF, "r", "r", 0),
                                         (G.VEC | G.AK, "r", "c", 0), (G.VEC | G.BNF, "c", "r", 0),
                                         (G.VEC, "c", "c", 0), (G.SCALAR, "r", "r", 1))]


@pytest.mark.parametrize("c", _NORMAL_F32, ids=_ids(_NORMAL_F32))
def test_gemm_f32_normal(cuda, c):
    """Unit-normal data, one case per loader: |got - ref| <= 4 sqrt(K) 2^-24 sum |a| |b|."""
    from msha_gnn_amd import functional as MF

    A = G.build_view(_normal(c["name"] + "A", (c["M"], c["K"])), c["a"])
    B = G.build_view(_normal(c["name"] + "B", (c["K"], c["N"])), c["b"])
    _, tA = dev_view(A, cuda)
    _, tB = dev_view(B, cuda)
    assert lib_loader("msha_gemm_f32_loader", tA, tB) == c["loader"]
    got = MF.gemm(tA, tB).cpu().numpy()
    bounded_close(got, A.values() @ B.values(), np.abs(A.values()) @ np.abs(B.values()),
                  c["K"], 0.0, c["name"], u=U32)


@pytest.mark.parametrize("K", [4096, 4099])
def test_gemm_f32_wgrad_normal(cuda, wgrad_kernel, K):
    """Unit-normal dW = X^T D on the resident kernels: K terms plus the row-quarter, block
    and slab reduce levels (64, as test_gemm_head_outer's bound); the split-bf16 kernel
    carries each operand as hi + mid bf16 terms (split_u = 2^-18)."""
    from msha_gnn_amd import functional as MF

    c = dict(G.WGRAD_CASES[0], K=K, name=f"normal-wgrad-{K}")
    A = G.build_view(_normal(c["name"] + "A", (128, K)), c["a"])
    B = G.build_view(_normal(c["name"] + "B", (K, 128)), c["b"])
    _, tA = dev_view(A, cuda)
    _, tB = dev_view(B, cuda)
    got = MF.gemm(tA, tB, splits=16).cpu().numpy()
    bounded_close(got, A.values() @ B.values(), np.abs(A.values()) @ np.abs(B.values()),
                  K + 64, 0.0, f"{c['name']}[{wgrad_kernel}]", u=U32,
                  split_u=BF16_SPLIT2 if wgrad_kernel == "s3" else 0.0)


# ---------------------------------------------------------------- bf16 msha_gemm_bf16
def _bf16_round(x):
    return torch.as_tensor(x, dtype=F32).to(BF).float().numpy().astype(np.float64)


@pytest.mark.parametrize("c", G.BF16_CASES, ids=_ids(G.BF16_CASES))
def test_gemm_bf16_exact(cuda, c):
    """The four loaders over the ragged grid (extents at multiples of 8 where the layout
    needs them), fp32 and bf16 C, split-K with used < splits."""
    from msha_gnn_amd import functional as MF

    A, B, ref = G.case_operands(c)
    _, tA = dev_view(A, cuda, BF)
    _, tB = dev_view(B, cuda, BF)
    want = G.predict_bf16(c["M"], c["N"], c["K"], *G.case_strides(c, 2))
    assert lib_loader("msha_gemm_bf16_loader", tA, tB) == want == c["loader"]
    got = MF.gemm(tA, tB, splits=c["splits"], out_dtype=BF if c["cbf"] else F32)
    assert got.dtype == (BF if c["cbf"] else F32) and got.shape == ref.shape
    got = got.float().cpu().numpy().astype(np.float64)
    assert np.array_equal(got, _bf16_round(ref) if c["cbf"] else ref), c["name"]


_NORMAL_BF16 = [G._case(f"normal-bf16-{code}-{'bf16' if cbf else 'f32'}", 136, 136, 104,
                        G.spec(ao), G.spec(bo), code, cbf=cbf)
                for code, ao, bo in ((G.VEC | G.AK | G.BNF, "r", "r"), (G.VEC | G.AK, "r", "c"),
                                     (G.VEC | G.BNF, "c", "r"), (G.VEC, "c", "c"))
                for cbf in (False, True)]


@pytest.mark.parametrize("c", _NORMAL_BF16, ids=_ids(_NORMAL_BF16))
def test_gemm_bf16_normal(cuda, c):
    """Unit-normal bf16 operands (the reference takes the rounded values), fp32
    accumulation: 4 sqrt(K) 2^-24 sum |a| |b|, plus one bf16 rounding of a bf16 C.  bf16
    keeps 8 significant bits: in [2^e, 2^(e+1)) its values lie 2^(e-7) apart, so round to
    nearest is off by at most 2^(e-8) <= 2^-8 |x| -- reached just above a power of two;
    2^-9 |x| (gpu_helpers.BF16_STORE) holds only at the top of a binade, and a correctly
    rounded unit-normal product misses it in a quarter of its elements by up to 2x."""
    from msha_gnn_amd import functional as MF

    A = G.build_view(_bf16_round(_normal(c["name"] + "A", (c["M"], c["K"]))), c["a"])
    B = G.build_view(_bf16_round(_normal(c["name"] + "B", (c["K"], c["N"]))), c["b"])
    _, tA = dev_view(A, cuda, BF)
    _, tB = dev_view(B, cuda, BF)
    assert lib_loader("msha_gemm_bf16_loader", tA, tB) == c["loader"]
    got = MF.gemm(tA, tB, out_dtype=BF if c["cbf"] else F32).float().cpu().numpy()
    bounded_close(got, A.values() @ B.values(), np.abs(A.values()) @ np.abs(B.values()),
                  c["K"], 0.0, c["name"], u=U32, store_u=BF16_RNE if c["cbf"] else 0.0)


@pytest.mark.parametrize("c", G.BF16_REFUSALS, ids=_ids(G.BF16_REFUSALS))
def test_gemm_bf16_refusals_launch_nothing(cuda, c):
    """Every documented refusal raises RuntimeError and leaves the output untouched: N % 8,
    K % 8 with a k-contiguous operand, rows % 8 with an m-contiguous one, an offset base, a
    pitch that is no multiple of 8, no unit stride."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    A, B, _ = G.case_operands(c)
    _, tA = dev_view(A, cuda, BF)
    _, tB = dev_view(B, cuda, BF)
    assert lib_loader("msha_gemm_bf16_loader", tA, tB) == c["loader"]
    assert G.predict_bf16(c["M"], c["N"], c["K"], *G.case_strides(c, 2)) == c["loader"]
    for cd, dt in ((0, F32), (1, BF)):
        out = torch.full((c["M"], c["ldc"]), float("nan"), device=cuda, dtype=dt)
        with pytest.raises(RuntimeError):
            _lib.call("msha_gemm_bf16", c["M"], c["N"], c["K"], tA.data_ptr(), tA.stride(0),
                      tA.stride(1), tB.data_ptr(), tB.stride(0), tB.stride(1), out.data_ptr(),
                      c["ldc"], cd, 1, None, 0, -1, 0, 0, None, None, None, None,
                      _lib.stream_handle(cuda))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), c["name"]
    with pytest.raises(RuntimeError):
        MF.gemm(tA, tB, out_dtype=F32)


# ------------------------------------------------------------------- gemm_head_outer
@pytest.mark.parametrize("c", G.HO_CASES, ids=_ids(G.HO_CASES))
def test_gemm_head_outer_exact(cuda, c):
    """dX = (dh + de (x) a [+ de2 (x) a2]) W^T (operand 0) and dW = X^T (dh + ...) (operand
    1) on the tiled kernels at 517 rows (ragged K for operand 1, heads*feat of 4, 24, 40 for
    operand 0), fp32 and bf16; ``fallback``: the updated operand's base one element off, so
    msha_gemm_f32_head_outer refuses and msha_add_head_outer + msha_gemm_f32 run."""
    from msha_gnn_amd import functional as MF

    d = G.ho_operands(c)
    dt = BF if c["dt"] == "bf16" else F32
    f = lambda x: None if x is None else plain(x, cuda)  # noqa: E731
    outer = (c["H"], c["F"], f(d["de"]), f(d["a"]), f(d["de2"]), f(d["a2"]))
    _, dh = dev_view(G.build_view(d["dh"], G.spec("r", off=c["off"])), cuda, dt)
    _, ot = dev_view(G.build_view(d["other"], G.spec("r")), cuda, dt)
    A, B = (dh, ot.t()) if c["operand"] == 0 else (ot.t(), dh)
    if c["dt"] == "f32":
        code = lib_loader("msha_gemm_f32_loader", A, B)
        assert (code == G.SCALAR) == (c["off"] != 0)
        got = MF.gemm_head_outer(A, B, c["operand"], outer).cpu().numpy().astype(np.float64)
        assert np.array_equal(got, d["ref"]), c["name"]
        return
    assert lib_loader("msha_gemm_bf16_loader", A, B) >= 0
    for odt in (F32, BF):
        got = MF.gemm_head_outer(A, B, c["operand"], outer, out_dtype=odt)
        assert got.dtype == odt
        got = got.float().cpu().numpy().astype(np.float64)
        assert np.array_equal(got, _bf16_round(d["ref"]) if odt == BF else d["ref"]), c["name"]


# ------------------------------------------------- project_scores on the tiled kernel
def _leaf64(x):
    return torch.tensor(x, dtype=torch.float64, requires_grad=True)


@pytest.mark.parametrize("c", G.PROJ_CASES, ids=_ids(G.PROJ_CASES))
def test_project_scores_tiled_exact(cuda, c):
    """256 < M < 1024: the tiled kernel's EPI_SCORE epilogue at feat 4, 8, 16 (and the plain
    store with no score vector), K = 30 on the scalar loader; forward and every gradient
    against torch fp64 on the same integers, bit for bit."""
    from msha_gnn_amd import functional as MF

    d = G.proj_arrays(c)
    M, H, F = c["M"], c["H"], c["F"]
    use = {"al": ("al",), "ar": ("ar",), "both": ("al", "ar"), "none": ()}[c["scores"]]
    names = ("X", "W") + use
    ts = {k: plain(d[k], cuda).requires_grad_(True) for k in names}
    rs = {k: _leaf64(d[k]) for k in names}
    outs = MF.project_scores(ts["X"], ts["W"], al=ts.get("al"), ar=ts.get("ar"), heads=H, feat=F)
    outs = outs if isinstance(outs, tuple) else (outs,)
    rh = rs["X"] @ rs["W"]
    refs = [rh] + [(rh.view(M, H, F) * rs[k]).sum(-1) for k in use]
    grads = [d["dh"]] + [d["dl"] if k == "al" else d["dr"] for k in use]
    assert len(outs) == len(refs)
    for got, want in zip(outs, refs):
        assert np.array_equal(got.detach().cpu().numpy().astype(np.float64),
                              want.detach().numpy()), c["name"]
    sum((o * plain(g, cuda)).sum() for o, g in zip(outs, grads)).backward()
    sum((o * torch.tensor(g)).sum() for o, g in zip(refs, grads)).backward()
    for k in names:
        assert np.array_equal(ts[k].grad.cpu().numpy().astype(np.float64),
                              rs[k].grad.numpy()), f"{c['name']} d{k}"


def test_project_scores_tiled_refuses_unsupported_feat(cuda):
    from msha_gnn_amd import functional as MF

    X, W = plain(G.ints("pX", (300, 20), 8), cuda), plain(G.ints("pW", (20, 12), 8), cuda)
    al = plain(G.ints("pal", (1, 12), 2), cuda)
    with pytest.raises(RuntimeError, match="feat must be"):
        MF.project_scores(X, W, al=al, heads=1, feat=12)


# -------------------------- matmul, linear_bias, pair_layer, score_pairs (tiled gather)
P_ROWS = 300  # below the resident-W kernels' 1024 rows: the tiled GEMM's gather loader


def _offset_table(name, rows, K, dev, dtype=F32, bound=8):
    """(values, view): ``rows`` x K integers as columns 3 .. 3+K of a table 5 columns wider
    (a misaligned base and a pitch that is no multiple of 4 for K = 6)."""
    wide = G.ints(name + "wide", (rows, K + 5), bound)
    return wide[:, 3:3 + K].copy(), plain(wide, dev, dtype)[:, 3:3 + K]


@pytest.mark.parametrize("K", [6, 32])
@pytest.mark.parametrize("N", [1, 3, 64])
def test_matmul_f32_exact(cuda, N, K):
    from msha_gnn_amd import functional as MF

    a, tA = _offset_table(f"mm{N}{K}", P_ROWS, K, cuda)
    b, g = G.ints(f"mmB{N}{K}", (K, N), 8), G.ints(f"mmG{N}{K}", (P_ROWS, N), 2)
    tA = tA.detach().requires_grad_(True)
    tB = plain(b, cuda).requires_grad_(True)
    ra, rb = _leaf64(a), _leaf64(b)
    C = MF.matmul(tA, tB)
    assert np.array_equal(C.detach().cpu().numpy(), a @ b)
    (C * plain(g, cuda)).sum().backward()
    ((ra @ rb) * torch.tensor(g)).sum().backward()
    assert np.array_equal(tA.grad.cpu().numpy(), ra.grad.numpy())
    assert np.array_equal(tB.grad.cpu().numpy(), rb.grad.numpy())


@pytest.mark.parametrize("K", [6, 32])
@pytest.mark.parametrize("N", [1, 3, 64])
def test_linear_bias_exact(cuda, N, K):
    """y = x W^T + b (msha_pair_linear's plain gather, bias tail col + u < N) and its
    backward (dW, the zero-stride ones row for db, dx)."""
    from msha_gnn_amd import functional as MF

    x, tx = _offset_table(f"lb{N}{K}", P_ROWS, K, cuda)
    w, b = G.ints(f"lbW{N}{K}", (N, K), 8), G.ints(f"lbb{N}{K}", (N,), 8)
    g = G.ints(f"lbG{N}{K}", (P_ROWS, N), 2)
    tx = tx.detach().requires_grad_(True)
    tw, tb = plain(w, cuda).requires_grad_(True), plain(b, cuda).requires_grad_(True)
    rx, rw, rb = _leaf64(x), _leaf64(w), _leaf64(b)
    y = MF.linear_bias(tx, tw, tb)
    ry = rx @ rw.t() + rb
    assert np.array_equal(y.detach().cpu().numpy(), ry.detach().numpy())
    (y * plain(g, cuda)).sum().backward()
    (ry * torch.tensor(g)).sum().backward()
    for got, want, nm in ((tx, rx, "dx"), (tw, rw, "dW"), (tb, rb, "db")):
        assert np.array_equal(got.grad.cpu().numpy(), want.grad.numpy()), nm


@pytest.mark.parametrize("K", [6, 32])
@pytest.mark.parametrize("N", [1, 3, 64])
def test_pair_layer_exact(cuda, N, K):
    """relu((x_i * x_j) W^T + b) on the gather-hadamard loader and its backward; the
    hadamard products (|x| <= 64) and every sum are exact integers."""
    from msha_gnn_amd import functional as MF

    xi, txi = _offset_table(f"pli{N}{K}", P_ROWS, K, cuda)
    xj, txj = _offset_table(f"plj{N}{K}", P_ROWS, K, cuda)
    w, b = G.ints(f"plW{N}{K}", (N, K), 8), G.ints(f"plb{N}{K}", (N,), 8)
    g = G.ints(f"plG{N}{K}", (P_ROWS, N), 2)
    assert (np.abs(xi * xj) @ np.abs(w.T) + np.abs(b)).max() < G.EXACT
    txi, txj = txi.detach().requires_grad_(True), txj.detach().requires_grad_(True)
    tw, tb = plain(w, cuda).requires_grad_(True), plain(b, cuda).requires_grad_(True)
    rxi, rxj, rw, rb = _leaf64(xi), _leaf64(xj), _leaf64(w), _leaf64(b)
    y = MF.pair_layer(txi, txj, tw, tb)
    ry = torch.relu((rxi * rxj) @ rw.t() + rb)
    assert np.array_equal(y.detach().cpu().numpy(), ry.detach().numpy())
    (y * plain(g, cuda)).sum().backward()
    (ry * torch.tensor(g)).sum().backward()
    for got, want, nm in ((txi, rxi, "dxi"), (txj, rxj, "dxj"), (tw, rw, "dW"), (tb, rb, "db")):
        assert np.array_equal(got.grad.cpu().numpy(), want.grad.numpy()), nm


@pytest.mark.parametrize("K", [6, 32])
@pytest.mark.parametrize("N", [1, 3, 64])
def test_score_pairs_mlp_tiled(cuda, N, K):
    """sigmoid(relu((h[src] * h[dst]) W^T + b)) with the gather in the loader.  The
    pre-activation is an exact integer z, so the only error is the sigmoid's: __expf(-z)
    has a relative error of at most z log2(e) 2^-24 (the rounded argument scaling) + 2^-22
    (the exp2 instruction), and z e^-z <= 1 / e, so e^-z is off by less than 2^-22 + 2^-25;
    the add and the divide round twice more on values <= 1.  Bound: 2^-21, absolute."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(N + K)
    h, th = _offset_table(f"sp{N}{K}", 50, K, cuda, bound=1)
    w, b = G.ints(f"spW{N}{K}", (N, K), 2), G.ints(f"spb{N}{K}", (N,), 2)
    src, dst = rng.integers(0, 50, P_ROWS), rng.integers(0, 50, P_ROWS)
    got = MF.score_pairs(th, torch.as_tensor(src, device=cuda), torch.as_tensor(dst, device=cuda),
                         mode="mlp", W=plain(w, cuda), b=plain(b, cuda)).cpu().numpy()
    z = np.maximum((h[src] * h[dst]) @ w.T + b, 0.0)
    assert np.abs(got - 1.0 / (1.0 + np.exp(-z))).max() <= 2.0 ** -21


@pytest.mark.parametrize("n,D,m", [(264, 64, 32), (264, 64, 30), (261, 64, 32)])
def test_matmul_bf16_fwd_bwd(cuda, n, D, m):
    """u v^T of MSHALayer.epilogue in bf16, forward and backward, against fp64 on the
    bf16-rounded inputs at the bf16-table bar of test_gpu_bf16.py (1e-2 relative, 1e-2 of
    max |ref| floor).  m = 30 recipients: the forward's N and the backward's K (dA = dC v)
    are no multiple of 8, so those products take fp32 operands; no shape raises."""
    from msha_gnn_amd import functional as MF

    u = _bf16_round(_normal(f"bu{n}{m}", (n, D)))
    v = _bf16_round(_normal(f"bv{n}{m}", (m, D)))
    g = _bf16_round(_normal(f"bg{n}{m}", (n, m)))
    tu = plain(u, cuda, BF).requires_grad_(True)
    tv = plain(v, cuda, BF).requires_grad_(True)
    C = MF.matmul(tu, tv.t())
    assert C.dtype == BF
    C.backward(plain(g, cuda, BF))
    assert tu.grad.dtype == BF and tv.grad.dtype == BF
    tol_close(C.detach().float().cpu().numpy(), u @ v.T, 1e-2, 1e-2)
    tol_close(tu.grad.float().cpu().numpy(), g @ v, 1e-2, 1e-2)
    tol_close(tv.grad.float().cpu().numpy(), g.T @ u, 1e-2, 1e-2)


# ----------------------------------------------------------------------- coverage
def test_sweep_reaches_every_loader(msha):
    """The union of the loader codes the library reports for the sweep's fp32 and bf16
    cases is the full set (host-only queries: the strides and base alignment of each case's
    views on a made-up aligned address)."""
    from msha_gnn_amd import _lib

    base = 1 << 30
    seen = {}
    for key, fn, item, cases in (("f32", "msha_gemm_f32_loader", 4, G.F32_CASES + G.WGRAD_CASES),
                                 ("bf16", "msha_gemm_bf16_loader", 2, G.BF16_CASES)):
        seen[key] = set()
        for c in cases:
            a_mis, sAm, sAk, b_mis, sBk, sBn = G.case_strides(c, item)
            code = _lib.fn(fn)(c["M"], c["N"], c["K"], base + a_mis, sAm, sAk, base + b_mis,
                               sBk, sBn)
            assert code == c["loader"], c["name"]
            seen[key].add(code)
    print("fp32 loaders:", sorted(seen["f32"]), "bf16 loaders:", sorted(seen["bf16"]))
    assert seen["f32"] == G.F32_LOADERS
    assert seen["bf16"] == G.BF16_LOADERS
