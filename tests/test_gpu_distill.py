"""Link-prediction distillation on the device: the fused rank / KL / probability loss
(msha_link_distill_fwd), the table gradient from its per-pair g (msha_pair_grad_bwd), HIP
graph capture with the context sampler and the plan, and the module surface.

The terms and g are compared against the fp64 restatement evaluated at the kernel's own
logits with the pinned fp32 decisions (``distill_ref``), so no hinge or tie decision can
differ and nothing is excluded; the logits themselves against fp64 and, bitwise, against
``link_bce_loss``."""
import numpy as np
import pytest
import torch

import distill_ref as D
import link_ref as R
from gpu_helpers import U32, bounded_close, ref32_close

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BF16_RNE = 2.0 ** -8  # a bf16 gradient: the fp32 sum rounded to nearest into 8 bits


def _dev(x, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    return t if dtype is None else t.to(dtype)


def _table(rng, n, F, scale, dtype, dev):
    """(device table, its exact values in fp64): the reference sees the rounded inputs."""
    h = _dev(rng.standard_normal((n, F)).astype(np.float32) * scale, dev, dtype)
    return h, h.detach().to(torch.float64).cpu().numpy()


def _lists(rng, A, K, n, pad=True):
    """Anchors and context with duplicates and self pairs; with ``pad`` (and A > 1) anchors
    -1 and n, a -1 mid-row, a row with one valid slot and a row with none."""
    anchors = rng.integers(0, n, A).astype(np.int64)
    ctx = rng.integers(0, n, (A, K)).astype(np.int64)
    ctx[0, 0] = anchors[0]  # a self pair
    if pad and A > 1:
        ctx[0, K // 2] = -1
        if A >= 6:
            anchors[1], anchors[2] = -1, n
            ctx[3, :] = n + 7
            ctx[3, K - 1] = 5  # one valid slot
            ctx[4, :] = -1     # none
            ctx[A - 1, K - 1] = 10 ** 12
    return anchors, ctx


def _forward(h, anchors, ctx, tl=None, th=None, margin=0.1, tau=1.0, w=(1.0, 1.0, 0.0)):
    """msha_link_distill_fwd: dict of numpy outputs (sentinel-filled buffers)."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev = h.device
    A, K = ctx.shape
    logits = torch.full((A, K), 7.5, dtype=torch.float32, device=dev)
    g = torch.full((A, K), 7.5, dtype=torch.float32, device=dev)
    loss = torch.full((), 7.5, dtype=torch.float32, device=dev)
    terms = torch.full((3,), 7.5, dtype=torch.float32, device=dev)
    npad = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().msha_link_distill_fwd_workspace_size(A), dtype=torch.uint8,
                     device=dev)
    t_args = ((th.data_ptr(), th.shape[1], MF._code(th.dtype), th.stride(0), th.shape[0])
              if th is not None else (None, 0, 0, 0, 0))
    _lib.call("msha_link_distill_fwd", A, K, h.shape[1], MF._code(h.dtype), h.data_ptr(),
              h.stride(0), h.shape[0], anchors.data_ptr(), ctx.data_ptr(), _lib.ptr(tl), *t_args,
              margin, tau, w[0], w[1], w[2], logits.data_ptr(), g.data_ptr(), loss.data_ptr(),
              terms.data_ptr(), npad.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.stream_handle(dev))
    return dict(y=logits.cpu().numpy(), g=g.cpu().numpy(), loss=float(loss),
                terms=terms.cpu().numpy(), npad=int(npad), g_dev=g)


def _backward(h, src, dst, g, gloss, plan):
    """msha_pair_grad_bwd: dH (n, F) fp32, pre-filled with a sentinel every row overwrites."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev, P = h.device, src.numel()
    n, F = h.shape
    dH = torch.full((n, F), 7.5, dtype=torch.float32, device=dev)
    gl = torch.tensor([gloss], dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.load().msha_pair_grad_bwd_workspace_size(P, F), dtype=torch.uint8,
                     device=dev)
    _lib.call("msha_pair_grad_bwd", P, F, MF._code(h.dtype), h.data_ptr(), h.stride(0), n,
              src.data_ptr(), dst.data_ptr(), g.data_ptr(), gl.data_ptr(),
              plan.rowptr.data_ptr(), plan.ent.data_ptr(), plan.chunk_tab.data_ptr(),
              dH.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle(dev))
    return dH


def _bce_logits(MF, h, src, dst):
    zero = torch.zeros(src.numel(), device=h.device)
    return MF.link_bce_loss(h, src, dst, zero, return_logits=True)[1]


def _check(name, MF, h, h64, anchors, ctx, tl=None, th=None, margin=0.1, tau=1.0,
           w=(1.0, 1.0, 0.5), gloss=-1.5):
    """Everything about one call: logits (bitwise against link_bce_loss, bounded against
    fp64), padding, the integer rank counts, the terms and g against the fp64 restatement at
    the kernel's own logits, the loss, and dH of the kernel's g.  Returns the outputs."""
    dev = h.device
    n, F = h.shape
    A, K = ctx.shape
    ta, tc = _dev(anchors, dev), _dev(ctx, dev)
    tlt = _dev(tl, dev, torch.float32) if tl is not None else None
    out = _forward(h, ta, tc, tlt, th, margin, tau, w)
    valid = D.valid_slots(anchors, ctx, n, None if th is None else th.shape[0])
    y, g = out["y"], out["g"]
    # padding: NaN exactly there, g = 0, counted
    assert out["npad"] == int((~valid).sum())
    assert np.isnan(y[~valid]).all() and np.isfinite(y[valid]).all()
    assert (g[~valid] == 0).all() and np.isfinite(g).all()
    assert np.isfinite(out["loss"]) and np.isfinite(out["terms"]).all()
    # logits: link_bce_loss's bits on the flat pairs, and within its bound of fp64
    src, dst = D.flat_pairs(anchors, ctx)
    ts, td = _dev(src, dev), _dev(dst, dev)
    zb = _bce_logits(MF, h, ts, td).cpu().numpy().reshape(A, K)
    assert np.array_equal(y[valid].view(np.int32), zb[valid].view(np.int32)), name
    zref, Az, _ = R.logits(h64, src, dst)
    zref, Az = zref.reshape(A, K), Az.reshape(A, K)
    if valid.any():
        bounded_close(y[valid], zref[valid], Az[valid], F, 1e-5, f"{name} y")
    t = _bce_logits(MF, th, ts, td).cpu().numpy().reshape(A, K) if th is not None else \
        tlt.cpu().numpy()
    ref = D.distill(y, t, valid, margin, tau, w)
    r32 = D.smooth_torch(y, t, valid, tau, w, torch.float32)
    # the integer rank counts, from a call with the rank weight alone
    wr = w[0] if w[0] != 0 else 1.0
    gr = _forward(h, ta, tc, tlt, th, margin, tau, (wr, 0.0, 0.0))["g"].astype(np.float64)
    cf = gr * A / wr
    assert np.abs(cf - np.rint(cf)).max() <= 1e-3 * max(1.0, np.abs(cf).max())
    assert np.array_equal(np.rint(cf).astype(np.int64), ref["c"]), f"{name}: rank counts"
    # the smooth part alone against fp64, by the yardstick of the same formulas in fp32
    gs = _forward(h, ta, tc, tlt, th, margin, tau, (0.0, w[1], w[2]))["g"].astype(np.float64)
    ref32_close(gs, ref["g_smooth"], r32[2], 1e-5, f"{name} g smooth")
    # the full g: the two parts under one division (three roundings)
    gsum = gr * (w[0] / wr) + gs
    assert np.all(np.abs(g - gsum) <= 4 * U32 * (np.abs(gr) * abs(w[0] / wr) + np.abs(gs))
                  + 1e-45), f"{name}: g is not its rank part plus its smooth part"
    # terms: (L_R, L_D, L_P) / A
    npairs = np.maximum(valid.sum(1) * (valid.sum(1) - 1) // 2, 1)
    bounded_close(out["terms"][:1], ref["terms"][:1], ref["terms"][0], npairs.sum() + A, 1e-5,
                  f"{name} L_R")
    ref32_close(out["terms"][1:2], ref["terms"][1:2], np.array([r32[0].sum() / A]), 1e-5,
                f"{name} L_D")
    ref32_close(out["terms"][2:3], ref["terms"][2:3], np.array([r32[1].sum() / A]), 1e-5,
                f"{name} L_P")
    parts = np.asarray(w, np.float64) * out["terms"].astype(np.float64)
    assert abs(out["loss"] - parts.sum()) <= 4 * U32 * np.abs(parts).sum() + 1e-45
    # dH of the kernel's own g under the plan of the flat pairs
    plan = MF.context_plan(ta, tc, n)
    assert torch.equal(plan.src, ts)
    dH = _backward(h, ts, td, out["g_dev"], gloss, plan)
    dref, Ad, deg = R.table_grad(h64, src, dst, gloss * g.reshape(-1).astype(np.float64))
    got = dH.cpu().numpy()
    bounded_close(got, dref, Ad, deg + 4, 1e-5, f"{name} dH")
    assert (got[deg == 0] == 0).all()
    assert torch.equal(dH, _backward(h, ts, td, out["g_dev"], gloss, plan))
    assert torch.equal(dH, _backward(h, ts, td, out["g_dev"], gloss, MF.context_plan(ta, tc, n)))
    out.update(valid=valid, ref=ref, t=t, deg=deg)
    return out


# (dtype, F, K, A): every K in {2, 5, 16, 33, 64}, the narrowest and widest width of each
# table type plus 32 and 128, A in {1, 37, 1030} (1030: seventeen loss tiles, the last partial)
CASES = [("fp32", 4, 2, 37), ("fp32", 256, 5, 1), ("fp32", 32, 16, 1030), ("fp32", 128, 33, 37),
         ("fp32", 128, 64, 37), ("fp32", 32, 64, 1),
         ("bf16", 8, 5, 37), ("bf16", 512, 2, 1), ("bf16", 32, 33, 1030), ("bf16", 128, 16, 37),
         ("bf16", 128, 64, 37), ("bf16", 32, 2, 1030)]


@pytest.mark.parametrize("dt,F,K,A", CASES)
def test_terms_gradient_and_table_gradient(cuda, msha, dt, F, K, A):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(1000 * K + F + A)
    n = 200 if A > 100 else 60
    h, h64 = _table(rng, n, F, 1.2 / np.sqrt(np.sqrt(F)), DT[dt], cuda)
    anchors, ctx = _lists(rng, A, K, n)
    name = f"{dt} F={F} K={K} A={A}"
    if (K + A) % 2:  # a teacher table of the other type and another width, fewer rows
        tdt, tF = ("bf16", 64) if dt == "fp32" else ("fp32", 16)
        th, _ = _table(rng, n - 3, tF, 1.5 / np.sqrt(np.sqrt(tF)), DT[tdt], cuda)
        _check(name + " table", MF, h, h64, anchors, ctx, th=th, margin=0.1, tau=0.7)
    else:  # teacher logits with ties (multiples of 1/4)
        tl = (np.round(rng.standard_normal((A, K)) * 6) / 4).astype(np.float32)
        _check(name + " logits", MF, h, h64, anchors, ctx, tl=tl, margin=0.25, tau=1.0)


def test_all_teacher_logits_equal(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(3)
    A, K, n, F = 37, 16, 60, 32
    h, h64 = _table(rng, n, F, 0.5, torch.float32, cuda)
    anchors, ctx = _lists(rng, A, K, n, pad=False)
    tl = np.full((A, K), 0.375, np.float32)
    out = _check("equal teacher", MF, h, h64, anchors, ctx, tl=tl, margin=0.1, w=(1.0, 0.0, 0.0))
    pairs = A * K * (K - 1) // 2
    assert abs(out["terms"][0] * A - float(np.float32(0.1)) * pairs) <= 1e-6 * 0.1 * pairs
    assert (out["g"].view(np.int32) == 0).all()  # the rank part of g: exactly +0


@pytest.mark.parametrize("tau", [0.5, 4.0])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_saturated_logits(cuda, msha, dt, tau):
    """Student and teacher logits of +-80: exp(160) without the max subtraction, sigmoids
    that round to 0 and 1.  No NaN or Inf, and every bound of ``_check`` still holds."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(5)
    n, F, A, K = 12, 32, 37, 5
    hv = np.zeros((n, F), np.float32)
    c = np.sqrt(80.0 / F)
    hv[0], hv[1], hv[2] = c, c, -c
    hv[3:] = rng.standard_normal((n - 3, F)) * 0.3
    h = _dev(hv, cuda, DT[dt])
    h64 = h.to(torch.float64).cpu().numpy()
    anchors = rng.integers(0, 3, A).astype(np.int64)
    ctx = rng.integers(0, n, (A, K)).astype(np.int64)
    ctx[:, 0], ctx[:, 1] = 1, 2  # y = +-80 in every row
    tl = rng.choice(np.array([-80, 80, 79.5, 0.25, -3], np.float32), (A, K))
    out = _check(f"{dt} saturated tau={tau}", MF, h, h64, anchors, ctx, tl=tl, margin=0.1,
                 tau=tau, w=(1.0, 1.0, 1.0))
    assert np.abs(out["y"]).max() > 75


def test_padding_changes_nothing_else(cuda, msha):
    """A list with anchors -1 and n, a -1 in the middle of every row, a row with one valid
    slot and a row with none, against the same list with those slots and rows removed: the
    same logit bits, the same integer counts, and the same sums (A L) and A g up to the
    order of the wave's adds (the slots sit on other lanes)."""
    rng = np.random.default_rng(9)
    A0, K0, n, F = 70, 7, 60, 32
    h, _ = _table(rng, n, F, 0.5, torch.float32, cuda)
    anchors, ctx = _lists(rng, A0, K0, n, pad=False)
    tl = (np.round(rng.standard_normal((A0, K0)) * 6) / 4).astype(np.float32)
    at = rng.integers(0, K0 + 1, A0)  # where the -1 goes in each row
    pctx = np.stack([np.insert(ctx[a], at[a], -1) for a in range(A0)])
    ptl = np.stack([np.insert(tl[a], at[a], 9.0) for a in range(A0)]).astype(np.float32)
    extra_ctx = rng.integers(0, n, (4, K0 + 1))
    extra_ctx[2, :], extra_ctx[2, 3] = -1, 4  # one valid slot
    extra_ctx[3, :] = n                      # none
    pctx = np.concatenate([pctx, extra_ctx]).astype(np.int64)
    panchors = np.concatenate([anchors, [-1, n, 6, 8]]).astype(np.int64)
    ptl = np.concatenate([ptl, rng.standard_normal((4, K0 + 1)).astype(np.float32)])
    w = (1.0, 1.0, 0.0)  # (the row with one valid slot adds nothing to L_R and L_D)
    base = _forward(h, _dev(anchors, cuda), _dev(ctx, cuda), _dev(tl, cuda), w=w)
    padded = _forward(h, _dev(panchors, cuda), _dev(pctx, cuda), _dev(ptl, cuda), w=w)
    A1 = A0 + 4
    assert padded["npad"] == A0 + 2 * (K0 + 1) + K0 + (K0 + 1) and base["npad"] == 0
    keep = np.ones((A0, K0 + 1), bool)
    keep[np.arange(A0), at] = False
    py, pg = padded["y"][:A0][keep].reshape(A0, K0), padded["g"][:A0][keep].reshape(A0, K0)
    assert np.isnan(padded["y"][:A0][~keep]).all() and np.isnan(padded["y"][A0:A0 + 2]).all()
    assert np.isnan(padded["y"][A0 + 3]).all() and np.isnan(padded["y"][A0 + 2]).sum() == K0
    assert (padded["g"][:A0][~keep] == 0).all() and (padded["g"][A0:] == 0).all()
    assert np.array_equal(py.view(np.int32), base["y"].view(np.int32))
    bg, pg = base["g"].astype(np.float64) * A0, pg.astype(np.float64) * A1
    assert np.all(np.abs(pg - bg) <= 64 * U32 * np.maximum(np.abs(bg), 1.0))
    # (the row with one valid slot has no pair and p = q = 1; its L_P is its own square)
    one = (D.sigmoid(padded["y"][A0 + 2, 3]) - D.sigmoid(ptl[A0 + 2, 3])) ** 2
    for i, own in enumerate((0.0, 0.0, float(one))):
        a, b = float(padded["terms"][i]) * A1, float(base["terms"][i]) * A0 + own
        assert abs(a - b) <= 1e-6 * abs(b), (i, a, b)
    # the rank counts alone: exactly equal
    wr = (1.0, 0.0, 0.0)
    b = _forward(h, _dev(anchors, cuda), _dev(ctx, cuda), _dev(tl, cuda), w=wr)["g"]
    p = _forward(h, _dev(panchors, cuda), _dev(pctx, cuda), _dev(ptl, cuda), w=wr)["g"]
    assert np.array_equal(np.rint(p[:A0][keep].reshape(A0, K0).astype(np.float64) * A1),
                          np.rint(b.astype(np.float64) * A0))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_hot_row_goes_through_chunk_partials(cuda, msha, dt):
    """One anchor node and four context nodes: the anchor's table row holds A K endpoints
    and each context row a quarter of them, all past msha_pair_plan_chunk()."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    chunk = int(_lib.load().msha_pair_plan_chunk())
    rng = np.random.default_rng(13)
    A, K, n, F = 5 * chunk // 8 + 3, 8, 50, 32
    h, h64 = _table(rng, n, F, 0.5, DT[dt], cuda)
    anchors = np.full(A, 17, np.int64)
    ctx = rng.choice(np.array([2, 17, 30, 49]), (A, K)).astype(np.int64)
    tl = (np.round(rng.standard_normal((A, K)) * 6) / 4).astype(np.float32)
    out = _check(f"{dt} hot row", MF, h, h64, anchors, ctx, tl=tl)
    deg = out["deg"]
    assert deg[17] > 2 * chunk and min(deg[2], deg[30], deg[49]) > chunk
    assert (deg > 0).sum() == 4


def _torch_smooth(h64, anchors, ctx, t, tau, w, A):
    """torch fp64 autograd of the smooth composition (no padding): (L_D, L_P, loss, dH)."""
    import torch.nn.functional as TF

    ht = torch.tensor(h64, requires_grad=True)
    y = torch.einsum("af,akf->ak", ht[torch.as_tensor(anchors)], ht[torch.as_tensor(ctx)])
    tt = torch.as_tensor(t, dtype=torch.float64)
    LD = TF.kl_div(torch.log_softmax(y / tau, 1), torch.softmax(tt / tau, 1), reduction="sum")
    LP = TF.mse_loss(torch.sigmoid(y), torch.sigmoid(tt), reduction="sum")
    loss = (w[1] * LD + w[2] * LP) / A
    return y, LD, LP, loss, ht


def _grad_slack(w, tau, A):
    """|dg_k| <= slack max_j |dy_j| for the smooth part of g: the softmax Jacobian gives
    (w_dist / tau)(1 / tau) q_k (|dy_k| + sum_j q_j |dy_j|) <= (2 w_dist / tau^2) max |dy|, and
    |d/dy [(s(y) - s(t)) s'(y)]| <= s'^2 + |s''| <= 1/16 + 0.0963 < 0.16."""
    return (2.0 * w[1] / tau ** 2 + 0.32 * w[2]) / A


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_smooth_loss_matches_torch_autograd(cuda, msha, dt):
    """w_rank = 0 at a larger shape, end to end against fp64 autograd.  The kernel's y is
    off by at most its bound (4 sqrt(F) u A_y), so pair p's factor is within |g_p| +
    ``_grad_slack`` max_row A_y terms: A[r, f] sums that times |h[other][f]| and the term
    count grows by the F terms inside y."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(31)
    A, K, n, F = 1030, 33, 200, 128
    tau, w = 0.8, (0.0, 1.0, 2.0)
    h, h64 = _table(rng, n, F, 0.2, DT[dt], cuda)
    anchors, ctx = _lists(rng, A, K, n, pad=False)
    tl = (rng.standard_normal((A, K)) * 1.5).astype(np.float32)
    y, LD, LP, ref_loss, ht = _torch_smooth(h64, anchors, ctx, tl, tau, w, A)
    (2 * ref_loss).backward()
    hg = h.clone().requires_grad_(True)
    loss, terms = MF.link_distill_loss(hg, _dev(anchors, cuda), _dev(ctx, cuda),
                                       teacher_logits=_dev(tl, cuda), tau=tau, w_rank=w[0],
                                       w_dist=w[1], w_prob=w[2], return_terms=True)
    (2 * loss).backward()
    assert hg.grad.dtype == DT[dt] and hg.grad.shape == hg.shape
    src, dst = D.flat_pairs(anchors, ctx)
    _, Az, _ = R.logits(h64, src, dst)
    ref = D.distill(y.detach().numpy(), tl, np.ones((A, K), bool), 0.1, tau, w)
    azmax = np.repeat(Az.reshape(A, K).max(1), K)
    extra = 2.0 * (np.abs(ref["g"].reshape(-1)) + _grad_slack(w, tau, A) * azmax)
    _, Ab, deg = R.table_grad(h64, src, dst, np.zeros(A * K), extra=extra)
    got = hg.grad.to(torch.float64).cpu().numpy()
    bounded_close(got, ht.grad.numpy(), Ab, deg + F, 1e-5, f"{dt} autograd dH",
                  store_u=BF16_RNE if dt == "bf16" else 0.0)
    # |dL_D / dy_k| = |q_k - p_k| / tau <= 1 / tau and |dL_P / dy_k| <= 2 |d| / 4 <= 1 / 2
    got_t = terms.cpu().numpy().astype(np.float64) * A
    bounded_close(got_t[1:2], np.array([float(LD.detach())]),
                  np.abs(ref["LD"]).sum() + Az.sum() / tau,
                  A * K + F, 1e-5, f"{dt} L_D against torch")
    bounded_close(got_t[2:3], np.array([float(LP.detach())]), ref["LP"].sum() + 0.5 * Az.sum(),
                  A * K + F, 1e-5, f"{dt} L_P against torch")
    assert got_t[0] == 0.0 or np.isfinite(got_t[0])


def test_end_to_end_matches_torch_autograd(cuda, msha):
    """All three terms against torch fp64 autograd of the composition at A = 32, K = 8, F =
    32.  Teacher logits are multiples of 1/8 (no difference within 0.025 of the margin 0.1),
    and the test first asserts that no pair's fp64 hinge argument lies within 4x the two
    logits' bounds of zero, so every decision of the kernel is the reference's."""
    import torch.nn.functional as TF

    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(0)
    A, K, n, F = 32, 8, 100, 32
    margin, tau, w = 0.1, 1.0, (1.0, 1.0, 0.5)
    h, h64 = _table(rng, n, F, 0.5, torch.float32, cuda)
    anchors, ctx = _lists(rng, A, K, n, pad=False)
    tl = (np.round(rng.standard_normal((A, K)) * 8) / 8).astype(np.float32)
    src, dst = D.flat_pairs(anchors, ctx)
    zref, Az, _ = R.logits(h64, src, dst)
    zref, Az = zref.reshape(A, K), Az.reshape(A, K)
    ref = D.distill(zref, tl, np.ones((A, K), bool), margin, tau, w, pinned=False)
    yb = 1e-5 * np.abs(zref) + 4 * np.sqrt(F) * U32 * Az  # bounded_close's bound of a logit
    band = 4 * (yb[:, :, None] + yb[:, None, :])
    ranked = ref["pair"] & (ref["r"] != 0)
    assert ranked.sum() > 300 and (np.abs(ref["arg"])[ranked] > band[ranked]).all()
    dt_ = tl[:, :, None].astype(np.float64) - tl[:, None, :]
    assert (np.abs(np.abs(dt_) - margin) >= 0.025 - 1e-12).all()
    # torch fp64
    ht = torch.tensor(h64, requires_grad=True)
    y = torch.einsum("af,akf->ak", ht[torch.as_tensor(anchors)], ht[torch.as_tensor(ctx)])
    tt = torch.as_tensor(tl, dtype=torch.float64)
    i, j = np.triu_indices(K, 1)
    d = tt[:, i] - tt[:, j]
    r = torch.where(d.abs() > margin, torch.sign(d), torch.zeros_like(d))
    LR = TF.margin_ranking_loss(y[:, i], y[:, j], r, margin=margin, reduction="sum")
    LD = TF.kl_div(torch.log_softmax(y / tau, 1), torch.softmax(tt / tau, 1), reduction="sum")
    LP = TF.mse_loss(torch.sigmoid(y), torch.sigmoid(tt), reduction="sum")
    ref_loss = (w[0] * LR + w[1] * LD + w[2] * LP) / A
    ref_loss.backward()
    np.testing.assert_allclose(ref["loss"], float(ref_loss.detach()), rtol=1e-12)
    hg = h.clone().requires_grad_(True)
    loss, terms, logits = MF.link_distill_loss(
        hg, _dev(anchors, cuda), _dev(ctx, cuda), teacher_logits=_dev(tl, cuda), margin=margin,
        tau=tau, w_rank=w[0], w_dist=w[1], w_prob=w[2], return_terms=True, return_logits=True)
    loss.backward()
    bounded_close(logits.cpu().numpy(), zref, Az, F, 1e-5, "e2e y")
    azmax = np.repeat(Az.max(1), K)
    extra = np.abs(ref["g"].reshape(-1)) + _grad_slack(w, tau, A) * azmax
    _, Ab, deg = R.table_grad(h64, src, dst, np.zeros(A * K), extra=extra)
    bounded_close(hg.grad.cpu().numpy(), ht.grad.numpy(), Ab, deg + F, 1e-5, "e2e dH")
    got_t = terms.cpu().numpy().astype(np.float64) * A
    # each pair's hinge moves by at most |dy_i| + |dy_j|
    pair_az = ((Az[:, :, None] + Az[:, None, :]) * ref["pair"]).sum()
    bounded_close(got_t[0:1], np.array([float(LR.detach())]), ref["LR"].sum() + pair_az,
                  A * K * (K - 1) // 2 + F, 1e-5, "e2e L_R")
    bounded_close(got_t[1:2], np.array([float(LD.detach())]),
                  np.abs(ref["LD"]).sum() + Az.sum() / tau,
                  A * K + F, 1e-5, "e2e L_D")
    bounded_close(got_t[2:3], np.array([float(LP.detach())]), ref["LP"].sum() + 0.5 * Az.sum(),
                  A * K + F, 1e-5, "e2e L_P")
    lt = np.asarray(w) * np.array([float(LR.detach()), float(LD.detach()), float(LP.detach())]) / A
    bounded_close(np.array([float(loss.detach())]), np.array([float(ref_loss.detach())]),
                  np.abs(lt).sum() + (w[0] * pair_az + (w[1] / tau + 0.5 * w[2]) * Az.sum()) / A,
                  A * K * K + F, 1e-5, "e2e loss")


# ------------------------------------------------------------------------ bitwise ---

def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _step(MF, h, anchors, ctx, plan=None, **kw):
    hg = h.detach().clone().requires_grad_(True)
    loss, terms, logits = MF.link_distill_loss(hg, anchors, ctx, plan=plan, return_terms=True,
                                               return_logits=True, **kw)
    (grad,) = torch.autograd.grad(loss, hg)
    return loss, terms, logits, grad


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_bitwise_reproducible(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(41)
    A, K, n, F = 300, 16, 40, 32  # hot rows: chunk partials
    h, _ = _table(rng, n, F, 0.5, DT[dt], cuda)
    th, _ = _table(rng, n, 64, 0.4, DT["bf16" if dt == "fp32" else "fp32"], cuda)
    an, cx = _lists(rng, A, K, n)
    anchors, ctx = _dev(an, cuda), _dev(cx, cuda)
    kw = dict(teacher_table=th, margin=0.1, tau=0.9, w_prob=0.5)
    a = _step(MF, h, anchors, ctx, **kw)
    b = _step(MF, h, anchors, ctx, **kw)                                       # two calls
    c = _step(MF, h, anchors, ctx, plan=MF.context_plan(anchors, ctx, n), **kw)  # a given plan
    for other in (b, c):
        for x, y in zip(a, other):
            assert torch.equal(_bits(x), _bits(y))
    # the teacher table against its own logits from link_bce_loss
    src, dst = D.flat_pairs(an, cx)
    tl = _bce_logits(MF, th, _dev(src, cuda), _dev(dst, cuda)).reshape(A, K)
    tl = torch.nan_to_num(tl, nan=0.0)  # (padding slots: never read into a term)
    kw2 = dict(kw)
    del kw2["teacher_table"]
    d = _step(MF, h, anchors, ctx, teacher_logits=tl, **kw2)
    for x, y in zip(a, d):
        assert torch.equal(_bits(x), _bits(y))
    # graph replay against eager
    _step(MF, h, anchors, ctx, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _step(MF, h, anchors, ctx, **kw)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, outs):
        assert torch.equal(_bits(x), _bits(y))


def test_sample_plan_loss_backward_in_one_graph(cuda, msha):
    """sample_context + context_plan + loss + backward captured into one HIP graph and
    replayed three times under a replay counter: each replay draws a fresh context and
    equals the eager chain at that counter value."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(43)
    n, F, A = 64, 32, 500
    deg = rng.integers(1, 6, n)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg]).astype(np.int32)
    csr = (_dev(rowptr, cuda), _dev(col, cuda))
    h, _ = _table(rng, n, F, 0.5, torch.float32, cuda)
    th, _ = _table(rng, n, F, 0.5, torch.float32, cuda)
    anchors = _dev(rng.integers(0, 8, A).astype(np.int64), cuda)  # hot anchor rows

    def step():
        ctx = MF.sample_context(csr, anchors, walks=3, hops=2, n_rand=2, n_nodes=n, seed=77)
        plan = MF.context_plan(anchors, ctx, n)
        return (ctx,) + _step(MF, h, anchors, ctx, plan=plan, teacher_table=th, w_prob=0.3)

    counter = torch.zeros(1, dtype=torch.int64, device=cuda)
    prev = MF.set_rng_counter(counter)
    try:
        step()  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        seen = []
        for value in (1, 2, 3):
            counter.fill_(value)
            graph.replay()
            torch.cuda.synchronize()
            got = [o.clone() for o in outs]
            eager = step()
            for x, y in zip(got, eager):
                assert torch.equal(_bits(x) if x.is_floating_point() else x,
                                   _bits(y) if y.is_floating_point() else y)
            assert all(not torch.equal(got[0], s) for s in seen)
            seen.append(got[0])
    finally:
        MF.set_rng_counter(prev)


def test_link_predictor_distill_loss_is_the_functional(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rng = np.random.default_rng(2)
    n, F, A, K = 100, 32, 60, 8
    h, _ = _table(rng, n, F, 0.4, torch.float32, cuda)
    th, _ = _table(rng, n, 64, 0.4, torch.float32, cuda)
    an, cx = _lists(rng, A, K, n)
    anchors, ctx = _dev(an, cuda), _dev(cx, cuda)
    tl = _dev(rng.standard_normal((A, K)).astype(np.float32), cuda)
    pred = layers.LinkPredictor("inner", F, F, 1, 2, 0.0).to(cuda)
    for kw_m, kw_f in ((dict(teacher_logits=tl), dict(teacher_logits=tl)),
                       (dict(teacher_h=th, w_prob=1.0, tau=2.0),
                        dict(teacher_table=th, w_prob=1.0, tau=2.0))):
        a, b = h.clone().requires_grad_(True), h.clone().requires_grad_(True)
        la = pred.distill_loss(a, anchors, ctx, **kw_m)
        lb = MF.link_distill_loss(b, anchors, ctx, **kw_f)
        la.backward()
        lb.backward()
        assert la.dim() == 0 and la.dtype == torch.float32
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    with pytest.raises(ValueError, match="no scalar to rank by"):
        layers.LinkPredictor("mlp", F, F, 1, 2, 0.0).to(cuda).distill_loss(
            h, anchors, ctx, teacher_logits=tl)
