"""The representation-matching term on the device (msha_link_match_fwd / _bwd,
functional.link_match_loss, LinkPredictor.match_loss, dropin KD_cosine) and the student MLP
(layers.MLP): values against the fp64 restatement and torch autograd, determinism and
permutation invariance, the reference fixture, and one captured student step."""
import os
import sys

import numpy as np
import pytest
import torch

import match_ref as R
from conftest import golden
from gpu_helpers import bounded_close, tol_close

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BF16_RNE = 2.0 ** -8  # a bf16 gradient: the fp32 row rounded to nearest (test_gpu_link_loss)
N, N_T, P = 200, 180, 3000
HOT = 5  # the row with more than 2,500 occurrences


def _dev(x, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    return t if dtype is None else t.to(dtype)


def _table(rng, n, F, dtype, dev, scale=0.5):
    """(device table, its exact values in fp64): the reference sees the rounded inputs."""
    h = _dev(rng.standard_normal((n, F)).astype(np.float32) * scale, dev, dtype)
    return h, h.detach().to(torch.float64).cpu().numpy()


def _rows(rng):
    """P = 3000 entries over n = 200 student / n_t = 180 teacher rows: row 5 occurs 2,600
    times, rows 10..59 exactly once, rows 60..149 share 346, the other rows never; the
    padding entries -1, n_t, n - 1 (inside the student table, outside the teacher's) and
    n + 5.  Shuffled."""
    rows = np.concatenate([np.full(2600, HOT), np.arange(10, 60), rng.integers(60, 150, 346),
                           [-1, N_T, N - 1, N + 5]]).astype(np.int64)
    assert len(rows) == P
    return rows[rng.permutation(P)]


def _forward(h, T, rows, want_rows=True):
    """msha_link_match_fwd: dict(coef, cos, count, loss, npad), outputs pre-filled."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev, n = h.device, h.shape[0]
    Pn = rows.numel() if rows is not None else n
    coef = torch.full((n, 2), 7.5, dtype=torch.float32, device=dev)
    cos = torch.full((n,), 7.5, dtype=torch.float32, device=dev) if want_rows else None
    count = torch.full((n,), -7, dtype=torch.int32, device=dev) if want_rows else None
    loss = torch.full((), 7.5, dtype=torch.float32, device=dev)
    npad = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().msha_link_match_fwd_workspace_size(Pn, n), dtype=torch.uint8,
                     device=dev)
    _lib.call("msha_link_match_fwd", Pn, h.shape[1], MF._code(h.dtype), h.data_ptr(),
              h.stride(0), n, MF._code(T.dtype), T.data_ptr(), T.stride(0), T.shape[0],
              _lib.ptr(rows), coef.data_ptr(), _lib.ptr(cos), _lib.ptr(count), loss.data_ptr(),
              npad.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle(dev))
    return dict(coef=coef, cos=cos, count=count, loss=loss, npad=npad)


def _backward(h, T, coef, gloss):
    """msha_link_match_bwd: dH (n, F) fp32, pre-filled with a sentinel every row overwrites."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev = h.device
    n, F = h.shape
    dH = torch.full((n, F), 7.5, dtype=torch.float32, device=dev)
    g = torch.tensor([gloss], dtype=torch.float32, device=dev)
    _lib.call("msha_link_match_bwd", F, MF._code(h.dtype), h.data_ptr(), h.stride(0), n,
              MF._code(T.dtype), T.data_ptr(), T.stride(0), T.shape[0], coef.data_ptr(),
              g.data_ptr(), dH.data_ptr(), _lib.stream_handle(dev))
    return dH


def _terms(F):
    """Term count for the bounds: the three F-term dot products inside every coefficient,
    the scalar algebra, the two products and the difference of a gradient element."""
    return 3 * F + 8


CASES = ([("fp32", "fp32", F) for F in (4, 32, 128, 256)]
         + [("bf16", "bf16", F) for F in (8, 32, 128, 512)]
         + [("fp32", "bf16", F) for F in (8, 128, 256)]
         + [("bf16", "fp32", F) for F in (8, 128, 256)])


# ----------------------------------------------------------------- forward, backward ---

@pytest.mark.parametrize("hd,td,F", CASES)
def test_forward_and_backward_match_the_restatement(cuda, msha, hd, td, F):
    rng = np.random.default_rng(F + 1000 * (hd == "bf16") + 2000 * (td == "bf16"))
    h, h64 = _table(rng, N, F, DT[hd], cuda)
    T, T64 = _table(rng, N_T, F, DT[td], cuda)
    T[HOT] = h[HOT].to(T.dtype) * 1.5 + T[HOT] * 0.01  # the hot row nearly parallel
    T64 = T.to(torch.float64).cpu().numpy()
    rows = _rows(rng)
    name = f"{hd}x{td} F={F}"
    out = _forward(h, T, _dev(rows, cuda))
    ref = R.forward(h64, T64, rows)
    count = out["count"].cpu().numpy()
    assert np.array_equal(count, np.bincount(rows[(rows >= 0) & (rows < N_T)], minlength=N))
    assert count[HOT] == 2600 and (count[10:60] == 1).all() and (count[150:] == 0).all()
    assert int(out["npad"]) == 4 == ref["npad"]
    cos = out["cos"].cpu().numpy()
    on = count > 0
    assert np.isnan(cos[~on]).all() and np.isfinite(cos[on]).all()
    assert ref["cos"][HOT] > 0.999
    bounded_close(cos[on], ref["cos"][on], ref["A_cos"][on], _terms(F), 1e-5, f"{name} cos")
    loss = float(out["loss"])
    assert np.isfinite(loss)
    bounded_close(np.array([loss]), np.array([ref["loss"]]), ref["A_loss"], _terms(F), 1e-5,
                  f"{name} loss")
    coef = out["coef"].cpu().numpy()
    assert (coef[~on] == 0).all() and np.isfinite(coef).all()
    # coef0 has no cancellation; coef1 carries the cosine's
    bounded_close(coef[:, 0], ref["coef"][:, 0], np.abs(ref["coef"][:, 0]), _terms(F), 1e-5,
                  f"{name} coef0")
    A1 = np.zeros(N)
    A1[on] = np.abs(ref["coef"][on, 0]) * ref["A_cos"][on]  # coef1 = coef0 cos (nt / ns)
    scale = np.ones(N)
    scale[on] = (np.sqrt((T64[np.flatnonzero(on)] ** 2).sum(1))
                 / np.sqrt((h64[on] ** 2).sum(1)))
    bounded_close(coef[:, 1], ref["coef"][:, 1], A1 * scale, _terms(F), 1e-5, f"{name} coef1")
    # the gradient from the kernel's own coefficients, a gloss other than 1
    gloss = -2.5
    dH = _backward(h, T, out["coef"], gloss)
    got = dH.cpu().numpy()
    assert (got != 7.5).all() and (got[~on] == 0).all() and np.isfinite(got).all()
    want, A = R.backward(h64, T64, ref["coef"], gloss)
    bounded_close(got, want, A, _terms(F), 1e-5, f"{name} dH")
    # the same bits from a second call, and from any permutation of the list
    again = _forward(h, T, _dev(rows, cuda))
    perm = _forward(h, T, _dev(rows[rng.permutation(P)], cuda))
    for other in (again, perm):
        for k in ("coef", "cos", "count", "loss", "npad"):
            assert torch.equal(out[k].view(torch.int32), other[k].view(torch.int32)), k
        assert torch.equal(dH, _backward(h, T, other["coef"], gloss))
    # the optional outputs left out: the same loss and coefficients
    bare = _forward(h, T, _dev(rows, cuda), want_rows=False)
    assert torch.equal(bare["loss"], out["loss"]) and torch.equal(bare["coef"], out["coef"])


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_gradient_matches_torch_autograd(cuda, msha, dt):
    """End to end against fp64 autograd of 1 - cosine_similarity(h[rows], T[rows]).mean()
    with a non-unit upstream gradient, through the Python surface."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(31)
    F = 64
    h, h64 = _table(rng, N, F, DT[dt], cuda)
    T, T64 = _table(rng, N_T, F, torch.float32, cuda, scale=2.0)
    rows = _rows(rng)
    ok = (rows >= 0) & (rows < N_T)
    ht = torch.tensor(h64, requires_grad=True)
    idx = torch.as_tensor(rows[ok])
    ref_loss = 1 - torch.nn.functional.cosine_similarity(ht[idx], torch.tensor(T64)[idx],
                                                         dim=-1).mean()
    (3.0 * ref_loss).backward()
    hg = h.clone().requires_grad_(True)
    loss, cos_rows, count = MF.link_match_loss(hg, _dev(rows, cuda), T, return_rows=True)
    (3.0 * loss).backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert hg.grad.dtype == DT[dt] and hg.grad.shape == hg.shape
    assert count.dtype == torch.int32 and cos_rows.shape == (N,)
    ref = R.forward(h64, T64, rows)
    _, A = R.backward(h64, T64, ref["coef"], 3.0)
    got = hg.grad.to(torch.float64).cpu().numpy()
    bounded_close(got, ht.grad.numpy(), A, _terms(F), 1e-5, f"{dt} autograd dH",
                  store_u=BF16_RNE if dt == "bf16" else 0.0)
    assert (got[ref["count"] == 0] == 0).all()
    bounded_close(np.array([float(loss.detach())]), np.array([float(ref_loss.detach())]),
                  ref["A_loss"], _terms(F), 1e-5, f"{dt} loss against torch")
    # nothing valid: loss 0 and a zero gradient, decided on the device
    hz = h.clone().requires_grad_(True)
    lz = MF.link_match_loss(hz, _dev(np.array([-1, N_T, N + 5], np.int64), cuda), T)
    lz.backward()
    assert float(lz.detach()) == 0.0 and not hz.grad.any()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_clamped_norms_follow_torch(cuda, msha, dt):
    """A zero student row against [3, 4] (cosine 0, d cos / d h = [6e7, 8e7]) and a student
    row of norm 1e-9 against [1e3, 0] (cosine 0.1): torch's values, every output finite."""
    from msha_gnn_amd import functional as MF

    F = 8
    h = np.zeros((6, F), np.float32)
    T = np.zeros((6, F), np.float32)
    T[0, :2] = (3.0, 4.0)
    h[1, 0], T[1, 0] = 1e-9, 1e3
    rng = np.random.default_rng(4)
    h[2:], T[2:] = rng.standard_normal((4, F)), rng.standard_normal((4, F))
    T[5] = 0.0  # a zero teacher row: cosine 0, zero gradient
    h, T = _dev(h, cuda, DT[dt]), _dev(T, cuda, DT[dt])
    h64, T64 = h.to(torch.float64).cpu().numpy(), T.to(torch.float64).cpu().numpy()
    rows = np.array([0, 1, 1, 2, 3, 4, 5, 0], np.int64)
    ht = torch.tensor(h64, requires_grad=True)
    idx = torch.as_tensor(rows)
    ref_loss = 1 - torch.nn.functional.cosine_similarity(ht[idx], torch.tensor(T64)[idx],
                                                         dim=-1).mean()
    ref_loss.backward()
    hg = h.clone().requires_grad_(True)
    loss, cos, count = MF.link_match_loss(hg, _dev(rows, cuda), T, return_rows=True)
    loss.backward()
    cos = cos.cpu().numpy()
    # the stored value of 1e-9 (exact in neither type) over the clamped norm 1e-8
    assert cos[0] == 0.0 and cos[5] == 0.0 and abs(cos[1] - h64[1, 0] * 1e8) <= 1e-5 * 0.1
    if dt == "fp32":
        assert abs(cos[1] - 0.1) <= 1e-5 * 0.1
    got = hg.grad.to(torch.float64).cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(float(loss.detach())) and np.isfinite(cos).all()
    want = ht.grad.numpy()
    # two of the eight entries are row 0: d loss / d h[0] = -(2 / 8) [6e7, 8e7]
    assert np.allclose(want[0, :2], [-1.5e7, -2e7], rtol=1e-12) and not got[5].any()
    ref = R.forward(h64, T64, rows)
    _, A = R.backward(h64, T64, ref["coef"], 1.0)
    bounded_close(got, want, A, _terms(F), 1e-5, f"{dt} clamped dH",
                  store_u=BF16_RNE if dt == "bf16" else 0.0)
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * abs(float(ref_loss.detach()))


def test_count_alone_over_many_tiles(cuda, msha):
    """msha_link_match_count past one LDS table: 50,000 entries (25 tiles of 2,048) with
    about 2,000 distinct rows per tile in 4,096 slots, so some probe chains run out and take
    the direct add; then every entry in 7 rows; padding on both sides of [0, n_valid)."""
    from msha_gnn_amd import _lib

    rng = np.random.default_rng(12)
    n, n_valid, Pn = 30_000, 29_000, 50_000
    for rows in (rng.integers(-50, n + 50, Pn), rng.integers(100, 107, Pn)):
        rows = rows.astype(np.int64)
        count = torch.full((n,), -7, dtype=torch.int32, device=cuda)
        npad = torch.full((1,), -7, dtype=torch.int32, device=cuda)
        tr = _dev(rows, cuda)
        _lib.call("msha_link_match_count", Pn, n, n_valid, tr.data_ptr(), count.data_ptr(),
                  npad.data_ptr(), _lib.stream_handle(cuda))
        ok = (rows >= 0) & (rows < n_valid)
        assert np.array_equal(count.cpu().numpy(), np.bincount(rows[ok], minlength=n))
        assert int(npad) == int((~ok).sum())


# ------------------------------------------------------------------------- surface ---

def test_rows_none_is_the_identity_list(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(6)
    for n, F, dt in ((1500, 32, "fp32"), (70, 128, "bf16")):  # two row tiles; one partial
        h, _ = _table(rng, n, F, DT[dt], cuda)
        T, _ = _table(rng, n, F, torch.float32, cuda)
        a, b = h.clone().requires_grad_(True), h.clone().requires_grad_(True)
        la, ca, na = MF.link_match_loss(a, None, T, return_rows=True)
        lb, cb, nb = MF.link_match_loss(b, torch.arange(n, device=cuda), T, return_rows=True)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(ca, cb) and torch.equal(na, nb)
        assert torch.equal(a.grad, b.grad) and (na == 1).all()


def test_kd_cosine_matches_the_reference(cuda, msha):
    from msha_gnn_amd import layers

    sys.path.insert(0, os.path.join(os.path.dirname(layers.__file__), "dropin"))
    try:
        import LLP as dropin_llp
    finally:
        sys.path.pop(0)
    z = golden("llp_student.npz")
    s = _dev(z["kd.s"], cuda).requires_grad_(True)
    t = _dev(z["kd.t"], cuda).requires_grad_(True)
    loss = dropin_llp.KD_cosine(s, t)
    loss.backward()
    assert t.grad is None  # the teacher is detached (LLP.py:35)
    ref = R.forward(z["kd.s"], z["kd.t"], None)
    want, A = R.backward(z["kd.s"], z["kd.t"], ref["coef"], 1.0)
    F = s.shape[1]
    bounded_close(np.array([float(loss.detach())]), np.array([ref["loss"]]), ref["A_loss"],
                  _terms(F), 1e-5, "KD_cosine")
    bounded_close(s.grad.cpu().numpy(), want, A, _terms(F), 1e-5, "KD_cosine ds")
    # the reference's own fp32 run pins the restatement
    assert abs(float(loss.detach()) - float(z["kd.loss"])) <= 1e-5 * abs(float(z["kd.loss"]))
    tol_close(s.grad.cpu().numpy(), z["kd.ds"], 1e-4, 1e-5)


def test_link_predictor_match_loss_is_the_functional(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rng = np.random.default_rng(2)
    n, F = 100, 32
    h = torch.as_tensor(rng.standard_normal((n, F)).astype(np.float32), device=cuda)
    T = torch.as_tensor(rng.standard_normal((n, F)).astype(np.float32), device=cuda)
    rows = _dev(rng.integers(0, n, 500).astype(np.int64), cuda)
    for predictor in ("inner", "mlp"):
        pred = layers.LinkPredictor(predictor, F, F, 1, 2, 0.0).to(cuda)
        a, b = h.clone().requires_grad_(True), h.clone().requires_grad_(True)
        la = pred.match_loss(a, rows, T)
        lb = MF.link_match_loss(b, rows, T)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)


# ----------------------------------------------------------------------------- MLP ---

def _mlp64(z, k, x):
    """LLP.py:75-84 in fp64 (eval: no dropout) on the fixture's parameters: the output and
    the gradients of its sum."""
    x = torch.as_tensor(x, dtype=torch.float64).requires_grad_(True)
    ps = {}
    h = x
    for i in range(k):
        W = torch.as_tensor(z[f"mlp{k}.state.layers.{i}.weight"], dtype=torch.float64)
        b = torch.as_tensor(z[f"mlp{k}.state.layers.{i}.bias"], dtype=torch.float64)
        ps[f"layers.{i}.weight"], ps[f"layers.{i}.bias"] = W.requires_grad_(True), b.requires_grad_(True)
        h = h @ W.T + b
        if i != k - 1:
            h = torch.relu(h)
    h.sum().backward()
    return h.detach().numpy(), x.grad.numpy(), {n: p.grad.numpy() for n, p in ps.items()}


@pytest.mark.parametrize("k", [1, 2, 3])
def test_mlp_eval_matches_the_reference(cuda, msha, k):
    from msha_gnn_amd import layers

    z = golden("llp_student.npz")
    xv = z[f"mlp{k}.x"]
    torch.manual_seed(k)
    mlp = layers.MLP(k, xv.shape[1], 32, z[f"mlp{k}.y"].shape[1], 0.5).to(cuda).eval()
    x = _dev(xv, cuda).requires_grad_(True)
    y = mlp(x)
    y.sum().backward()
    y64, dx64, g64 = _mlp64(z, k, xv)
    # the bars of the pair_layer tests: 1e-5 against the fp64 restatement, the reference's
    # own fp32 run within its rounding
    tol_close(y.detach().cpu().numpy(), y64, 1e-5, 1e-6)
    tol_close(y.detach().cpu().numpy(), z[f"mlp{k}.y"], 1e-5, 1e-6)
    tol_close(x.grad.cpu().numpy(), dx64, 1e-5, 1e-5)
    tol_close(x.grad.cpu().numpy(), z[f"mlp{k}.dx"], 1e-4, 1e-5)
    names = [n for n, _ in mlp.named_parameters()]
    assert names == list(g64)
    for n, p in mlp.named_parameters():
        tol_close(p.grad.cpu().numpy(), g64[n], 1e-5, 1e-5)
        tol_close(p.grad.cpu().numpy(), z[f"mlp{k}.grad.{n}"], 1e-4, 1e-5)


def test_mlp_train_mode_dropout(cuda, msha):
    """p = 0.5 with the last layer the identity: the output is dropout(relu(z)) itself."""
    from msha_gnn_amd import layers

    torch.manual_seed(9)
    B, K, Hd = 400, 16, 32
    mlp = layers.MLP(2, K, Hd, Hd, 0.5).to(cuda)
    with torch.no_grad():
        mlp.layers[1].weight.copy_(torch.eye(Hd))
        mlp.layers[1].bias.zero_()
    x = torch.randn(B, K, device=cuda)
    pre = mlp.eval()(x).detach()  # relu(z), exactly (x 1.0 + 0.0 per column)
    xg = x.clone().requires_grad_(True)
    out = mlp.train()(xg)
    out.sum().backward()
    o = out.detach()
    kept = o != 0
    assert torch.equal(o[kept], 2.0 * pre[kept])  # 1 / (1 - p) = 2: exact in fp32
    live = pre > 0
    assert not kept[~live].any()
    n_live = int(live.sum())
    frac = float(kept[live].sum()) / n_live
    assert abs(frac - 0.5) <= 4 * 0.5 / np.sqrt(n_live), frac
    # the backward uses the same mask: dx = (2 [kept]) @ W0
    want = (2.0 * kept.to(torch.float64)) @ mlp.layers[0].weight.detach().to(torch.float64)
    tol_close(xg.grad.cpu().numpy(), want.cpu().numpy(), 1e-5, 1e-5)
    # a second forward draws another mask
    assert not torch.equal(mlp(x) != 0, kept)


# ------------------------------------------------------------------------- capture ---

def test_student_step_in_one_graph(cuda, msha):
    """MLP forward, 10 BCE + 0.1 matching + 100 distillation with the plans built inside,
    and the backward to every parameter, captured once and replayed on new index contents:
    the loss and the gradients equal the eager run bit for bit."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rng = np.random.default_rng(5)
    n, Fin, Fd, Pn, A, K = 300, 32, 32, 2000, 256, 4
    torch.manual_seed(1)
    mlp = layers.MLP(2, Fin, 32, Fd, 0.0).to(cuda)
    params = list(mlp.parameters())
    feats = torch.as_tensor(rng.standard_normal((n, Fin)).astype(np.float32), device=cuda)
    teacher = torch.as_tensor(rng.standard_normal((n, Fd)).astype(np.float32), device=cuda)

    def batch():
        src = rng.integers(0, n, Pn)
        dst = rng.integers(0, 16, Pn)
        rows = rng.integers(0, 12, Pn)  # LLP's source_index: few sources, many times
        rows[rng.integers(0, Pn, 5)] = -1
        return (_dev(src.astype(np.int64), cuda), _dev(dst.astype(np.int64), cuda),
                _dev((rng.random(Pn) < 0.5).astype(np.float32), cuda),
                _dev(rows.astype(np.int64), cuda),
                _dev(rng.integers(0, n, A).astype(np.int64), cuda),
                _dev(rng.integers(0, n, (A, K)).astype(np.int64), cuda))

    def step(src, dst, y, rows, anchors, context):
        h = mlp(feats)
        loss = (10 * MF.link_bce_loss(h, src, dst, y, plan=MF.pair_plan(src, dst, n))
                + 0.1 * MF.link_match_loss(h, rows, teacher)
                + 100 * MF.link_distill_loss(h, anchors, context, teacher_table=teacher,
                                             plan=MF.context_plan(anchors, context, n)))
        return (loss,) + torch.autograd.grad(loss, params)

    static = batch()
    step(*static)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*static)
    for _ in range(2):
        new = batch()
        for s, t in zip(static, new):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*new)
        assert len(outs) == 1 + len(params) and np.isfinite(float(outs[0].detach()))
        for got, want in zip(outs, eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
