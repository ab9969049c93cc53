"""Link-prediction training on the device: the incidence plan (msha_pair_plan), the fused
BCE loss (msha_link_bce_fwd), its deterministic table gradient (msha_link_bce_bwd), HIP
graph capture, and the module surface."""
import numpy as np
import pytest
import torch

import link_ref as R
from gpu_helpers import bounded_close

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
# a bf16 gradient is the fp32 sum rounded to nearest into 8 significand bits: half an ulp,
# at most 2^-8 of the value (reached just above a power of two)
BF16_RNE = 2.0 ** -8


def _dev(x, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    return t if dtype is None else t.to(dtype)


def _table(rng, n, F, scale, dtype, dev):
    """(device table, its exact values in fp64): the reference sees the rounded inputs."""
    h = _dev(rng.standard_normal((n, F)).astype(np.float32) * scale, dev, dtype)
    return h, h.detach().to(torch.float64).cpu().numpy()


def _chunk(msha):
    from msha_gnn_amd import _lib

    return int(_lib.load().msha_pair_plan_chunk())


def _hot_pairs(rng, chunk):
    """P = 40,000 pairs, src in [32, 5000), dst in [0, 32): rows 0..3 get exactly chunk - 1,
    chunk, chunk + 1 and 2 chunk endpoints, rows 4..31 share the rest (more than two chunks
    each, so at least three chunk partials)."""
    P = 40_000
    fixed = [chunk - 1, chunk, chunk + 1, 2 * chunk]
    rest = P - sum(fixed)
    per = np.full(28, rest // 28)
    per[: rest % 28] += 1
    assert per.min() > 2 * chunk
    dst = np.repeat(np.arange(32), np.concatenate([fixed, per]))
    dst = dst[rng.permutation(P)]
    src = rng.integers(32, 5000, P)
    return src.astype(np.int64), dst.astype(np.int64), 5000, fixed


def _small_pairs(rng, P=777, n=50):
    """Duplicates, self pairs, padding pairs (-1 and n) and rows that no pair names."""
    src = rng.integers(0, n, P)
    dst = rng.integers(0, n, P)
    for idx in (src, dst):  # rows 7 and n - 1 stay without endpoints
        idx[idx == 7] = 8
        idx[idx == n - 1] = 0
    src[5], dst[5] = 11, 11  # self pairs
    src[6], dst[6] = 11, 11
    src[9] = -1  # padding pairs
    dst[10] = n
    src[P - 1], dst[P - 1] = n, -1
    return src.astype(np.int64), dst.astype(np.int64), n


# ---------------------------------------------------------------------------- plan ---

def _check_plan(MF, src, dst, n, dev):
    ts, td = _dev(src, dev), _dev(dst, dev)
    plan = MF.pair_plan(ts, td, n)
    again = MF.pair_plan(ts, td, n)
    rowptr, ent = R.plan(src, dst, n)
    assert plan.rowptr.dtype == torch.int32 and plan.ent.dtype == torch.int32
    assert np.array_equal(plan.rowptr.cpu().numpy(), rowptr)
    assert np.array_equal(plan.ent.cpu().numpy(), ent)
    for a, b in ((plan.rowptr, again.rowptr), (plan.ent, again.ent),
                 (plan.chunk_tab, again.chunk_tab)):
        assert torch.equal(a, b)
    return plan, rowptr


def test_plan_matches_the_stable_sort(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(1)
    chunk = _chunk(msha)
    _check_plan(MF, np.array([2]), np.array([0]), 3, cuda)          # P = 1
    _check_plan(MF, np.array([1]), np.array([5]), 3, cuda)          # P = 1, padding only
    src, dst, n = _small_pairs(rng)
    _, rowptr = _check_plan(MF, src, dst, n, cuda)                  # one radix pass
    assert rowptr[8] == rowptr[7] and rowptr[n] == rowptr[n - 1]    # rows without endpoints
    assert rowptr[n] == 2 * (len(src) - 3)
    src, dst, n, fixed = _hot_pairs(rng, chunk)
    _, rowptr = _check_plan(MF, src, dst, n, cuda)                  # two passes, long rows
    assert np.diff(rowptr)[:4].tolist() == fixed
    assert (np.diff(rowptr)[4:32] > 2 * chunk).all()
    # three and four radix passes (n past 2^16 and 2^24), rows far apart
    for n in (70_000, (1 << 24) + 3):
        src = rng.integers(0, n, 3000)
        dst = rng.integers(0, n, 3000)
        src[:3] = (n - 1, 0, n)
        _check_plan(MF, src, dst, n, cuda)


# ------------------------------------------------------------------------- forward ---

def _forward(h, src, dst, y, w):
    """msha_link_bce_fwd: (z, loss, padding count)."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev, P = h.device, src.numel()
    z = torch.empty(P, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    npad = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().msha_link_bce_fwd_workspace_size(P), dtype=torch.uint8,
                     device=dev)
    _lib.call("msha_link_bce_fwd", P, h.shape[1], MF._code(h.dtype), h.data_ptr(), h.stride(0),
              h.shape[0], src.data_ptr(), dst.data_ptr(), y.data_ptr(), _lib.ptr(w),
              z.data_ptr(), loss.data_ptr(), npad.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.stream_handle(dev))
    return z.cpu().numpy(), float(loss), int(npad)


def _check_forward(name, h, h64, src, dst, y, w):
    F, P = h.shape[1], len(src)
    dev = h.device
    ty = _dev(y, dev, torch.float32)
    tw = _dev(w, dev, torch.float32) if w is not None else None
    z, loss, npad = _forward(h, _dev(src, dev), _dev(dst, dev), ty, tw)
    zref, Az, ok = R.logits(h64, src, dst)
    assert npad == int((~ok).sum())
    assert np.isnan(z[~ok]).all() and np.isfinite(z[ok]).all()
    bounded_close(z[ok], zref[ok], Az[ok], F, 1e-5, f"{name} z")
    y32 = ty.cpu().numpy().astype(np.float64)
    w64 = tw.cpu().numpy().astype(np.float64) if w is not None else np.full(P, 1.0 / P)
    terms = (w64 * R.bce_terms(z.astype(np.float64), y32))[ok]  # over the kernel's own z
    assert np.isfinite(loss)
    bounded_close(np.array([loss]), np.array([terms.sum()]), np.abs(terms).sum(), P, 1e-5,
                  f"{name} loss")
    return z, loss


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_forward_logits_and_loss(cuda, msha, dt, F):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(F)
    P, n = 3000, 200  # three blocks of pairs, the last one partial
    h, h64 = _table(rng, n, F, 0.5, DT[dt], cuda)
    src = rng.integers(0, n, P).astype(np.int64)
    dst = rng.integers(0, n, P).astype(np.int64)
    src[[3, 1500]] = (-1, n)  # padding pairs
    dst[2999] = n + 5
    hard = (rng.random(P) < 0.5).astype(np.float32)
    soft = rng.random(P).astype(np.float32)
    w = (rng.random(P) * 2).astype(np.float32)
    _check_forward(f"{dt} F={F} hard/mean", h, h64, src, dst, hard, None)
    z, loss = _check_forward(f"{dt} F={F} soft/weighted", h, h64, src, dst, soft, w)
    # the Python surface returns the same numbers
    l2, z2 = MF.link_bce_loss(h, _dev(src, cuda), _dev(dst, cuda), _dev(soft, cuda),
                              weight=_dev(w, cuda), return_logits=True)
    assert float(l2) == loss and np.array_equal(z2.cpu().numpy(), z, equal_nan=True)
    assert l2.dtype == torch.float32 and l2.dim() == 0


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_forward_is_stable_at_large_logits(cuda, msha, dt):
    """|z| up to 60 on the wrong side of the target: l = 60, where the probability form
    sigmoid -> log gives -log(0) = inf."""
    F, n = 32, 8
    h = np.zeros((n, F), np.float32)
    c = np.sqrt(60.0 / F)
    h[0], h[1], h[2] = c, c, -c
    h[3:] = np.random.default_rng(0).standard_normal((n - 3, F)) * 0.3
    h = _dev(h, cuda, DT[dt])
    h64 = h.to(torch.float64).cpu().numpy()
    src = np.array([0, 0, 1, 3, 4, 0, 2], np.int64)
    dst = np.array([1, 2, 2, 4, 5, 0, 2], np.int64)
    y = np.array([0, 1, 1, 1, 0, 0.25, 0], np.float32)
    z, loss = _check_forward(f"{dt} large", h, h64, src, dst, y, np.ones(len(src), np.float32))
    assert np.abs(z).max() > 55 and np.isfinite(loss) and loss > 4 * 55


# ------------------------------------------------------------------------ backward ---

def _backward(h, src, dst, y, w, z, gloss, plan):
    """msha_link_bce_bwd: dH (n, F) fp32, pre-filled with a sentinel every row overwrites."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev, P = h.device, src.numel()
    n, F = h.shape
    dH = torch.full((n, F), 7.5, dtype=torch.float32, device=dev)
    g = torch.tensor([gloss], dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.load().msha_link_bce_bwd_workspace_size(P, F), dtype=torch.uint8,
                     device=dev)
    _lib.call("msha_link_bce_bwd", P, F, MF._code(h.dtype), h.data_ptr(), h.stride(0), n,
              src.data_ptr(), dst.data_ptr(), y.data_ptr(), _lib.ptr(w), z.data_ptr(),
              g.data_ptr(), plan.rowptr.data_ptr(), plan.ent.data_ptr(),
              plan.chunk_tab.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.stream_handle(dev))
    return dH


def _check_backward(name, MF, h, h64, src, dst, y, w, gloss):
    dev, P = h.device, len(src)
    n = h.shape[0]
    ts, td = _dev(src, dev), _dev(dst, dev)
    ty = _dev(y, dev, torch.float32)
    tw = _dev(w, dev, torch.float32) if w is not None else None
    _, z = MF.link_bce_loss(h, ts, td, ty, weight=tw, return_logits=True)
    plan = MF.pair_plan(ts, td, n)
    dH = _backward(h, ts, td, ty, tw, z, gloss, plan)
    # g from the kernel's own z, fp64
    z64 = z.cpu().numpy().astype(np.float64)
    w64 = tw.cpu().numpy().astype(np.float64) if w is not None else np.full(P, np.float32(1.0 / P))
    g = gloss * w64 * (R.sigmoid(z64) - ty.cpu().numpy().astype(np.float64))
    ref, A, deg = R.table_grad(h64, src, dst, g)
    got = dH.cpu().numpy()
    bounded_close(got, ref, A, deg + 4, 1e-5, name)
    assert (got[deg == 0] == 0).all()
    # the same bits from a second call, and from a plan built afresh
    assert torch.equal(dH, _backward(h, ts, td, ty, tw, z, gloss, plan))
    assert torch.equal(dH, _backward(h, ts, td, ty, tw, z, gloss, MF.pair_plan(ts, td, n)))
    return deg


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_backward_matches_fp64_restatement(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(8)
    chunk = _chunk(msha)
    # long rows through chunk partials (F = 32), rows 5000.. of the table without endpoints
    src, dst, n, _ = _hot_pairs(rng, chunk)
    h, h64 = _table(rng, n + 40, 32, 0.4, DT[dt], cuda)
    y = (rng.random(len(src)) < 0.5).astype(np.float32)
    deg = _check_backward(f"{dt} hot rows dH", MF, h, h64, src, dst, y, None, 1.0)
    assert (deg[n:] == 0).all() and deg[:4].tolist() == [chunk - 1, chunk, chunk + 1, 2 * chunk]
    # short rows, self pairs, padding, soft targets, weights, a non-unit upstream gradient
    src, dst, n = _small_pairs(rng)
    h, h64 = _table(rng, n, 128, 0.3, DT[dt], cuda)
    y = rng.random(len(src)).astype(np.float32)
    w = (rng.random(len(src)) * 2).astype(np.float32)
    deg = _check_backward(f"{dt} small dH", MF, h, h64, src, dst, y, w, -2.5)
    assert deg[7] == 0 and deg[n - 1] == 0


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_matches_torch_autograd(cuda, msha, dt, weighted):
    """End to end against fp64 autograd of binary_cross_entropy_with_logits.  The kernel's z
    is off by at most the z bound (4 sqrt(F) u A_z) and sigmoid' <= 1/4, so pair p's factor
    is within w (|sigmoid(z) - y| + A_z / 4) terms: A[r, f] sums that times |h[other][f]|
    and the term count grows by the F terms inside z."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(21)
    src, dst, n = _small_pairs(rng, P=2000, n=300)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    F = 32
    h, h64 = _table(rng, n, F, 0.25, DT[dt], cuda)
    zref, Az, _ = R.logits(h64, src, dst)
    assert np.abs(zref[ok]).max() <= 4.0
    y = rng.random(len(src)).astype(np.float32)
    w = (rng.random(len(src)) * 2).astype(np.float32) if weighted else None
    # torch fp64 on the pairs inside the table (a padding pair adds nothing; the mean is
    # over all P pairs)
    ht = torch.tensor(h64, requires_grad=True)
    logit = (ht[torch.as_tensor(src[ok])] * ht[torch.as_tensor(dst[ok])]).sum(-1)
    yt = torch.as_tensor(y[ok].astype(np.float64))
    wt = torch.as_tensor(w[ok].astype(np.float64)) if weighted else None
    ref_loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, yt, wt,
                                                                    reduction="sum")
    if not weighted:
        ref_loss = ref_loss / len(src)
    (2 * ref_loss).backward()
    hg = h.clone().requires_grad_(True)
    loss = MF.link_bce_loss(hg, _dev(src, cuda), _dev(dst, cuda), _dev(y, cuda),
                            weight=_dev(w, cuda) if weighted else None)
    (2 * loss).backward()  # a non-unit upstream gradient
    assert hg.grad.dtype == DT[dt] and hg.grad.shape == hg.shape
    w64 = w.astype(np.float64) if weighted else np.full(len(src), 1.0 / len(src))
    extra = 2.0 * w64 * (np.abs(R.sigmoid(zref) - y) + 0.25 * Az)
    _, A, deg = R.table_grad(h64, src, dst, np.zeros(len(src)), extra=extra)
    got = hg.grad.to(torch.float64).cpu().numpy()
    bounded_close(got, ht.grad.numpy(), A, deg + F, 1e-5, f"{dt} autograd dH",
                  store_u=BF16_RNE if dt == "bf16" else 0.0)
    assert (got[deg == 0] == 0).all()
    lterms = w64[ok] * R.bce_terms(zref[ok], y[ok])
    bounded_close(np.array([float(loss.detach())]), np.array([float(ref_loss.detach())]),
                  np.abs(lterms).sum() + (w64[ok] * Az[ok]).sum(), len(src) + F, 1e-5,
                  f"{dt} loss against torch")
    # reused plan: the same bits
    plan = MF.pair_plan(_dev(src, cuda), _dev(dst, cuda), n)
    hg2 = h.clone().requires_grad_(True)
    loss2 = MF.link_bce_loss(hg2, _dev(src, cuda), _dev(dst, cuda), _dev(y, cuda),
                             weight=_dev(w, cuda) if weighted else None, plan=plan)
    (2 * loss2).backward()
    assert torch.equal(loss2, loss) and torch.equal(hg2.grad, hg.grad)


# ------------------------------------------------------------------------- capture ---

def test_plan_loss_backward_in_one_graph(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(5)
    n, F, P = 400, 32, 5000
    h = (torch.as_tensor(rng.standard_normal((n, F)).astype(np.float32), device=cuda) * 0.3)
    h.requires_grad_(True)

    def batch():
        src = rng.integers(0, n, P)
        dst = rng.integers(0, 16, P)  # hot rows: chunk partials inside the graph
        src[rng.integers(0, P, 5)] = -1
        return (_dev(src.astype(np.int64), cuda), _dev(dst.astype(np.int64), cuda),
                _dev(rng.random(P).astype(np.float32), cuda))

    def step(src, dst, y):
        plan = MF.pair_plan(src, dst, n)
        loss, z = MF.link_bce_loss(h, src, dst, y, plan=plan, return_logits=True)
        (grad,) = torch.autograd.grad(loss, h)
        return loss, z, grad

    s_src, s_dst, s_y = batch()
    step(s_src, s_dst, s_y)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(s_src, s_dst, s_y)
    for _ in range(2):
        new = batch()
        for s, t in zip((s_src, s_dst, s_y), new):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*new)
        for got, want in zip(outs, eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))  # NaN z included


# -------------------------------------------------------------------------- module ---

def test_link_predictor_loss_is_the_functional(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rng = np.random.default_rng(2)
    n, F, P = 100, 32, 500
    h = torch.as_tensor(rng.standard_normal((n, F)).astype(np.float32), device=cuda) * 0.3
    src = _dev(rng.integers(0, n, P).astype(np.int64), cuda)
    dst = _dev(rng.integers(0, n, P).astype(np.int64), cuda)
    y = _dev((rng.random(P) < 0.5).astype(np.float32), cuda)
    w = _dev(rng.random(P).astype(np.float32), cuda)
    pred = layers.LinkPredictor("inner", F, F, 1, 2, 0.0).to(cuda)
    for weight in (None, w):
        a, b = h.clone().requires_grad_(True), h.clone().requires_grad_(True)
        la = pred.loss(a, src, dst, y, weight=weight)
        lb = MF.link_bce_loss(b, src, dst, y, weight=weight)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    with pytest.raises(ValueError, match="no scalar to rank by"):
        layers.LinkPredictor("mlp", F, F, 1, 2, 0.0).to(cuda).loss(h, src, dst, y)
