"""The 'mlp' link predictor's training loss on the device (msha_link_mlp_loss_fwd /
msha_link_mlp_bwd, functional.link_mlp_loss, LinkPredictor.llp_loss) against the fp64
restatement tests/link_mlp_ref.py.

Bounds (gpu_helpers.bounded_close, rtol 1e-5): a sum of n fp32 terms with absolute-term sum A
is held to rtol |ref| + 4 sqrt(n) 2^-24 A.  n is the true term count: F (+ bias and the
epilogue) for a pre-activation, the pairs of one row block plus the number of blocks for dW /
db, the row's endpoint count plus the N terms of dx for dH.  A bf16 table adds ONE named
operand error: the forward's loader rounds h[src] * h[dst] to bf16 before the MFMA
(gemm_bf16.hip hadamard8, skinny.hip's resident-W kernel).  bf16 keeps 8 significand bits, so
round-to-nearest moves a product by at most half an ulp = 2^-8 of it (reached just above a
power of two): ``split_u`` = gpu_helpers.BF16_U.  W is cast to bf16 before the call and the
reference sees the cast values.  The weight gradient multiplies
the two bf16 rows in fp32 (exact), so it carries no such term.  A bf16 dH is the fp32 sum
rounded once (``store_u`` 2^-8)."""
import numpy as np
import pytest
import torch

import link_mlp_ref as R
from gpu_helpers import BF16_U, bounded_close

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BF16_RNE = 2.0 ** -8  # a bf16 gradient: the fp32 sum rounded to nearest, at most 2^-8 of it
MARGIN = 1e-4         # no kept pre-activation of the reference lies this close to the kink


def _dev(x, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    return t if dtype is None else t.to(dtype)


def _split(dt):
    return BF16_U if dt == "bf16" else 0.0


def _lib():
    from msha_gnn_amd import _lib as L

    return L


def _chunk():
    return int(_lib().load().msha_pair_plan_chunk())


def _wrows():
    return int(_lib().load().msha_link_mlp_wgrad_rows())


def _params(rng, F, N, dt, dev, scale=1.0):
    """(W, b) on the device with their exact fp64 values; W is a bf16 value for a bf16 table
    (the op casts it, the reference sees what the kernel reads)."""
    W = torch.as_tensor((rng.standard_normal((N, F)) * scale / np.sqrt(F)).astype(np.float32))
    if dt == "bf16":
        W = W.to(torch.bfloat16).to(torch.float32)
    b = torch.as_tensor((rng.standard_normal(N) * 0.2).astype(np.float32))
    return W.to(dev), b.to(dev), W.double().numpy(), b.double().numpy()


def _lattice_table(rng, n, F, dt, dev):
    """Entries in {+-0.5, +-1, +-1.5, +-2}: every product h[s] * h[d] is a multiple of 0.25
    up to 4, exact in bf16, so the bf16 forward's loader rounds nothing and both dtypes
    compute the pre-activation to fp32 accumulation error (the kink tests need that)."""
    v = rng.integers(1, 5, (n, F)) * 0.5 * rng.choice([-1.0, 1.0], (n, F))
    h = _dev(v.astype(np.float32), dev, DT[dt])
    return h, h.to(torch.float64).cpu().numpy()


def _table(rng, n, F, scale, dt, dev):
    h = _dev(rng.standard_normal((n, F)).astype(np.float32) * scale, dev, DT[dt])
    return h, h.detach().to(torch.float64).cpu().numpy()


def _clear_of_kink(rng, h64, src, dst, W64, b64, lo, hi):
    """Redraw the src of every pair with a pre-activation inside (-MARGIN, MARGIN) from
    [lo, hi) until none is left (a handful of pairs, a few rounds)."""
    n = h64.shape[0]
    for _ in range(50):
        ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
        pre = (h64[np.where(ok, src, 0)] * h64[np.where(ok, dst, 0)]) @ W64.T + b64
        bad = ok & (np.abs(pre) < MARGIN).any(1)
        if not bad.any():
            return src
        src = src.copy()
        src[bad] = rng.integers(lo, hi, int(bad.sum()))
    raise AssertionError("could not clear the kink")


def _forward(h, src, dst, label, W, b, teacher, wl, wm, p=0.0, seed=0):
    """msha_link_mlp_loss_fwd: (out, terms, Pv) as device tensors."""
    from msha_gnn_amd import functional as MF

    L = _lib()
    dev, P = h.device, src.numel()
    N = W.shape[0]
    Wk = W.to(h.dtype).contiguous()
    out = torch.full((P, N), -3.0, dtype=torch.float32, device=dev)
    terms = torch.full((3,), -7.0, dtype=torch.float32, device=dev)
    pv = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(L.load().msha_link_mlp_loss_fwd_workspace_size(P), dtype=torch.uint8,
                     device=dev)
    L.call("msha_link_mlp_loss_fwd", P, h.shape[1], N, MF._code(h.dtype), h.data_ptr(),
           h.stride(0), h.shape[0], src.data_ptr(), dst.data_ptr(), L.ptr(label), Wk.data_ptr(),
           b.data_ptr(), L.ptr(teacher), wl, wm, p, seed, 0, out.data_ptr(), terms.data_ptr(),
           None, pv.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_handle(dev))
    return out, terms, pv


def _backward(h, src, dst, label, W, teacher, out, pv, wl, wm, p, gloss, plan):
    """msha_link_mlp_bwd: dz, dW, db and dH (pre-filled with a sentinel every row overwrites)."""
    from msha_gnn_amd import functional as MF

    L = _lib()
    dev, P = h.device, src.numel()
    n, F = h.shape
    N = W.shape[0]
    W32 = W.to(h.dtype).to(torch.float32).contiguous()
    dz = torch.full((P, N), 7.5, dtype=torch.float32, device=dev)
    dx = torch.empty(P, F, dtype=torch.float32, device=dev)
    dW = torch.full((N, F), 7.5, dtype=torch.float32, device=dev)
    db = torch.full((N,), 7.5, dtype=torch.float32, device=dev)
    dH = torch.full((n, F), 7.5, dtype=torch.float32, device=dev)
    g = torch.tensor([gloss], dtype=torch.float32, device=dev)
    ws = torch.empty(L.load().msha_link_mlp_bwd_workspace_size(P, F, N), dtype=torch.uint8,
                     device=dev)
    L.call("msha_link_mlp_bwd", P, F, N, MF._code(h.dtype), h.data_ptr(), h.stride(0), n,
           src.data_ptr(), dst.data_ptr(), L.ptr(label), W32.data_ptr(), L.ptr(teacher),
           out.data_ptr(), pv.data_ptr(), wl, wm, p, g.data_ptr(), plan.rowptr.data_ptr(),
           plan.ent.data_ptr(), plan.chunk_tab.data_ptr(), dz.data_ptr(), dx.data_ptr(),
           dW.data_ptr(), db.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(),
           L.stream_handle(dev))
    return dz, dW, db, dH


def _check_forward(name, dt, h, h64, src, dst, label, W, b, W64, b64, teacher, wl, wm, keep=None,
                   p=0.0, seed=0, split=None):
    """out, Pv and the three terms against fp64; returns (out, terms, pv, reference dict).
    ``split``: the per-term operand error of the pre-activation (default: the dtype's; 0 on a
    lattice table, whose products are exact in bf16)."""
    split = _split(dt) if split is None else split
    dev = h.device
    F, N = h.shape[1], W.shape[0]
    ts, td = _dev(src, dev), _dev(dst, dev)
    tl = _dev(label, dev) if label is not None else None
    tt = _dev(teacher, dev, torch.float32) if teacher is not None else None
    out, terms, pv = _forward(h, ts, td, tl, W, b, tt, wl, wm, p, seed)
    t64 = tt.double().cpu().numpy() if tt is not None else None
    f = R.forward(h64, src, dst, W64, b64, label=label, teacher=t64, w_label=wl, w_mse=wm,
                  keep=keep, p=p)
    ok = f["ok"]
    o = out.cpu().numpy()
    assert int(pv) == f["pv"]
    assert np.isnan(o[~ok]).all() and np.isfinite(o[ok]).all()
    if ok.any():
        # sigmoid' <= 1/4: the pre-activation's terms, scaled by the dropout factor
        bounded_close(o[ok], f["out"][ok], 0.25 * (f["Az"] * f["kf"])[ok], F + 8, 1e-5,
                      f"{name} out", split_u=split)
    # the terms from the kernel's own out, in fp64
    got = terms.cpu().numpy().astype(np.float64)
    o64 = o.astype(np.float64)
    if f["pv"] == 0:
        assert (got == 0).all()
        return out, terms, pv, f
    lab_terms = o64[ok, f["label"][ok]] / f["pv"]
    bounded_close(got[1:2], [-lab_terms.sum()], np.abs(lab_terms).sum(), f["pv"] + 4, 1e-5,
                  f"{name} L_lab")
    mse = 0.0
    if teacher is not None:
        sq = (o64[ok] - t64[ok]) ** 2 / (f["pv"] * N)
        mse = sq.sum()
        bounded_close(got[2:3], [mse], sq.sum(), f["pv"] * N + 4, 1e-5, f"{name} L_mse")
    else:
        assert got[2] == 0
    want = wl * got[1] + wm * got[2]
    bounded_close(got[0:1], [want], abs(wl * got[1]) + abs(wm * got[2]), 3, 1e-5, f"{name} loss")
    return out, terms, pv, f


def _padded_pairs(rng, P, n, N):
    """Pairs with every kind of padding (where P allows) and labels on their own."""
    src = rng.integers(0, n, P)
    dst = rng.integers(0, n, P)
    lab = rng.integers(0, N, P)
    if P >= 63:
        src[3], src[20], dst[P - 1], lab[7], lab[11] = -1, n, n + 5, N, -1
    return src.astype(np.int64), dst.astype(np.int64), lab.astype(np.int64)


# ------------------------------------------------------------------------- forward ---

@pytest.mark.parametrize("FN", [(32, 32), (128, 128)], ids=["32x32", "128x128"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_forward_out_terms_and_count(cuda, msha, dt, FN):
    from msha_gnn_amd import functional as MF

    F, N = FN
    rng = np.random.default_rng(F + (7 if dt == "bf16" else 0))
    n = 200
    h, h64 = _table(rng, n, F, 0.7, dt, cuda)
    W, b, W64, b64 = _params(rng, F, N, dt, cuda)
    for P in (1, 63, 65, 3000):
        src, dst, lab = _padded_pairs(rng, P, n, N)
        teacher = rng.random((P, N)).astype(np.float32)
        out, terms, pv, f = _check_forward(f"{dt} {F}x{N} P={P}", dt, h, h64, src, dst, lab, W, b,
                                           W64, b64, teacher, 10.0, 100.0)
        assert f["pv"] == (P - 5 if P >= 63 else P)
        # the Python surface returns the same numbers
        l2, o2, t2 = MF.link_mlp_loss(h, _dev(src, cuda), _dev(dst, cuda), W, b,
                                      label=_dev(lab, cuda), teacher_out=_dev(teacher, cuda),
                                      w_label=10.0, w_mse=100.0, return_output=True)
        assert torch.equal(o2.view(torch.int32), out.view(torch.int32)) and torch.equal(t2, terms)
        assert torch.equal(l2, terms[0]) and l2.dtype == torch.float32 and l2.dim() == 0
        # no teacher: the label term alone
        _check_forward(f"{dt} {F}x{N} P={P} no teacher", dt, h, h64, src, dst, lab, W, b, W64, b64,
                       None, 1.0, 0.0)
    # label=None is dst itself (a dst at or past N is then padding), bitwise
    P = 3000
    src, dst, _ = _padded_pairs(rng, P, n, N)
    dst[: P // 2] = rng.integers(0, N, P // 2)
    teacher = _dev(rng.random((P, N)).astype(np.float32), cuda)
    ts, td = _dev(src, cuda), _dev(dst, cuda)
    a = MF.link_mlp_loss(h, ts, td, W, b, teacher_out=teacher, w_mse=2.0, return_output=True)
    c = MF.link_mlp_loss(h, ts, td, W, b, label=td.clone(), teacher_out=teacher, w_mse=2.0,
                         return_output=True)
    for x, y in zip(a, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    _, _, pv, f = _check_forward(f"{dt} {F}x{N} label=dst", dt, h, h64, src, dst, None, W, b, W64,
                                 b64, teacher.cpu().numpy(), 1.0, 2.0)
    assert 0 < f["pv"] < P - 3  # the dst >= N pairs left Pv


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_all_padding_gives_zero_loss_and_gradients(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(4)
    n, F, N = 50, 32, 32
    h, _ = _table(rng, n, F, 0.5, dt, cuda)
    W, b, _, _ = _params(rng, F, N, dt, cuda)
    for P in (1, 300):
        src = _dev(np.full(P, -1, np.int64), cuda)
        dst = _dev(rng.integers(0, n, P).astype(np.int64), cuda)
        hg, Wg, bg = (x.clone().requires_grad_(True) for x in (h, W, b))
        loss, out, terms = MF.link_mlp_loss(hg, src, dst, Wg, bg,
                                            teacher_out=torch.rand(P, N, device=cuda),
                                            w_label=10.0, w_mse=100.0, return_output=True)
        (-2.5 * loss).backward()
        assert float(loss) == 0.0 and (terms == 0).all() and torch.isnan(out).all()
        for g in (hg.grad, Wg.grad, bg.grad):
            assert g is not None and (g == 0).all()


# ------------------------------------------------------------------------- dropout ---

@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dropout_follows_the_library_mask(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(12)
    n, F, N, P, p, seed = 120, 32, 32, 1500, 0.4, 77
    h, h64 = _table(rng, n, F, 0.7, dt, cuda)
    W, b, W64, b64 = _params(rng, F, N, dt, cuda)
    src, dst, lab = _padded_pairs(rng, P, n, N)
    teacher = rng.random((P, N)).astype(np.float32)
    keep = MF.dropout_keep_mask(P * N, p, seed, cuda, offset=0).cpu().numpy().reshape(P, N)
    assert 0.5 < keep.mean() < 0.7
    out, terms, _, f = _check_forward(f"{dt} dropout", dt, h, h64, src, dst, lab, W, b, W64, b64,
                                      teacher, 10.0, 100.0, keep=keep, p=p, seed=seed)
    ok = f["ok"]
    assert (out.cpu().numpy()[ok][keep[ok] == 0] == 0.5).all()  # dropped: sigmoid(0)
    args = (h, _dev(src, cuda), _dev(dst, cuda), W, b)
    kw = dict(label=_dev(lab, cuda), teacher_out=_dev(teacher, cuda), w_label=10.0, w_mse=100.0,
              return_output=True)
    l2, o2, _ = MF.link_mlp_loss(*args, p=p, training=True, seed=seed, **kw)
    assert torch.equal(l2, terms[0]) and torch.equal(o2.view(torch.int32), out.view(torch.int32))
    # p = 0, and p > 0 outside training, draw nothing
    base = MF.link_mlp_loss(*args, **kw)
    for other in (MF.link_mlp_loss(*args, p=0.0, training=True, seed=seed, **kw),
                  MF.link_mlp_loss(*args, p=p, training=False, seed=seed, **kw)):
        for x, y in zip(base, other):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------- dz rule ---

@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dz_rule_agrees_with_the_fp64_mask(cuda, msha, dt, p):
    """The backward recovers 'kept and ReLU-active' from out > 0.5.  On inputs whose fp64
    pre-activations all stay MARGIN away from 0 (asserted), that is the reference's own mask
    on every element, and dz matches the fp64 rule evaluated at the kernel's out."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(31)
    n, F, N, P, seed = 150, 128, 128, 700, 5
    h, h64 = _lattice_table(rng, n, F, dt, cuda)
    W, b, W64, b64 = _params(rng, F, N, dt, cuda, scale=0.25)
    src, dst, lab = _padded_pairs(rng, P, n, N)
    src = _clear_of_kink(rng, h64, src, dst, W64, b64, 0, n)
    teacher = rng.random((P, N)).astype(np.float32)
    keep = None
    if p > 0:
        keep = MF.dropout_keep_mask(P * N, p, seed, cuda).cpu().numpy().reshape(P, N)
    wl, wm, gloss = 10.0, 100.0, -2.5
    out, terms, pv, f = _check_forward(f"{dt} lattice p={p}", dt, h, h64, src, dst, lab, W, b, W64,
                                       b64, teacher, wl, wm, keep=keep, p=p, seed=seed,
                                       split=0.0)
    ok = f["ok"]
    kept = np.ones((P, N), bool) if keep is None else keep.astype(bool)
    relu = np.maximum(f["pre"], 0.0)
    assert not (kept & ok[:, None] & (relu > 0) & (relu < MARGIN)).any()
    assert not (ok[:, None] & (np.abs(f["pre"]) < MARGIN)).any()
    mask = kept & (f["pre"] > 0) & ok[:, None]
    o = out.cpu().numpy()
    assert np.array_equal((o > 0.5) & ok[:, None], mask)
    assert (o[ok][~mask[ok]] == 0.5).all()
    ts, td, tl = _dev(src, cuda), _dev(dst, cuda), _dev(lab, cuda)
    plan = MF.pair_plan(ts, td, n)
    dz, _, _, _ = _backward(h, ts, td, tl, W, _dev(teacher, cuda), out, pv, wl, wm, p, gloss, plan)
    dz = dz.cpu().numpy()
    o64, t64 = o.astype(np.float64), teacher.astype(np.float64)
    g = R.upstream(o64, ok, f["label"], t64, f["pv"], wl, wm, gloss)
    ref = R.dz_from(o64, g, mask, p)
    # |g|'s two terms before they cancel, times out (1 - out) / (1 - p)
    ag = np.zeros((P, N))
    rows = np.flatnonzero(ok)
    ag[rows, f["label"][rows]] = abs(gloss) * wl / f["pv"]
    ag[rows] += 2 * abs(gloss) * wm * (np.abs(o64[rows]) + np.abs(t64[rows])) / (f["pv"] * N)
    A = np.where(mask, ag * np.where(ok[:, None], o64 * (1 - o64), 0.0) / (1 - p), 0.0)
    bounded_close(dz, ref, A, 8, 1e-5, f"{dt} p={p} dz")
    assert (dz[~ok] == 0).all() and (dz[~mask] == 0).all()


# ------------------------------------------------------------------------ backward ---

def _hot_case(rng, chunk, wrows, N):
    """P = 2 wrows + 3 pairs over n = 340 rows: rows 0..3 are dst of exactly chunk - 1, chunk,
    chunk + 1 and 2 chunk pairs and of nothing else; rows 4..7 and 300.. have no endpoint; the
    rest are random pairs in [8, 300) with self pairs, repeated pairs and padding."""
    P = 2 * wrows + 3
    fixed = [chunk - 1, chunk, chunk + 1, 2 * chunk]
    assert P > sum(fixed) + 100
    dst = np.concatenate([np.repeat(np.arange(4), fixed), rng.integers(8, 300, P - sum(fixed))])
    src = rng.integers(8, 300, P)
    perm = rng.permutation(P)
    src, dst = src[perm], dst[perm]
    free = np.flatnonzero(dst >= 8)
    a, b_, c, d, e, f = free[:6]
    src[a], dst[a] = 11, 11            # self pairs
    src[b_], dst[b_] = 11, 11
    src[c], dst[c] = src[d], dst[d]    # a repeated pair
    src[e] = -1                        # padding
    dst[f] = 340
    lab = rng.integers(0, N, P)
    lab[free[6]], lab[free[7]] = N, -1
    return src.astype(np.int64), dst.astype(np.int64), lab.astype(np.int64), 340, fixed


def _small_case(rng, N, P=777, n=50):
    """Fewer pairs than one weight-gradient block: duplicates, self pairs, padding, rows that
    no pair names."""
    src = rng.integers(0, n, P)
    dst = rng.integers(0, n, P)
    for idx in (src, dst):  # rows 7 and n - 1 stay without endpoints
        idx[idx == 7] = 8
        idx[idx == n - 1] = 0
    src[5], dst[5] = 11, 11
    src[6], dst[6] = 11, 11
    src[9] = -1
    dst[10] = n
    src[P - 1], dst[P - 1] = n, -1
    lab = rng.integers(0, N, P)
    lab[12], lab[13] = N, -1
    return src.astype(np.int64), dst.astype(np.int64), lab.astype(np.int64), n


def _check_backward(name, dt, MF, h, h64, src, dst, lab, W, b, W64, teacher, wl, wm, gloss):
    dev = h.device
    n, F = h.shape
    N, P = W.shape[0], len(src)
    ts, td, tl = _dev(src, dev), _dev(dst, dev), _dev(lab, dev)
    tt = _dev(teacher, dev, torch.float32)
    out, terms, pv = _forward(h, ts, td, tl, W, b, tt, wl, wm)
    plan = MF.pair_plan(ts, td, n)
    got = _backward(h, ts, td, tl, W, tt, out, pv, wl, wm, 0.0, gloss, plan)
    dz, dW, db, dH = (x.cpu().numpy() for x in got)
    # the reference from the kernel's own out (its mask included) and its own dz
    ok, label = R.valid(src, dst, lab, n, N)
    assert int(pv) == int(ok.sum())
    o64 = out.cpu().numpy().astype(np.float64)
    g = R.upstream(o64, ok, label, tt.double().cpu().numpy(), int(ok.sum()), wl, wm, gloss)
    mask = (np.where(ok[:, None], o64, 0.5) > 0.5)
    ref = R.backward(h64, src, dst, W64, R.dz_from(o64, g, mask), ok)
    rows_blk = _wrows()
    n_w = min(P, rows_blk) + -(-P // rows_blk) + 8
    bounded_close(dW, ref["dW"], ref["A_dW"], n_w, 1e-5, f"{name} dW")
    bounded_close(db, ref["db"], ref["A_db"], n_w, 1e-5, f"{name} db")
    bounded_close(dH, ref["dH"], ref["A_dH"], ref["deg"] + N + 8, 1e-5, f"{name} dH")
    assert (dH[ref["deg"] == 0] == 0).all() and (dz[~ok] == 0).all()
    # the same bits from a second call, and from a plan built afresh
    for again in (_backward(h, ts, td, tl, W, tt, out, pv, wl, wm, 0.0, gloss, plan),
                  _backward(h, ts, td, tl, W, tt, out, pv, wl, wm, 0.0, gloss,
                            MF.pair_plan(ts, td, n))):
        for x, y in zip(got, again):
            assert torch.equal(x, y)
    return ref["deg"]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_backward_matches_fp64_restatement(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(8)
    chunk, wrows = _chunk(), _wrows()
    # hot rows through chunk partials, three weight-gradient blocks (the last: 3 pairs)
    F = N = 32
    src, dst, lab, n, fixed = _hot_case(rng, chunk, wrows, N)
    h, h64 = _table(rng, n, F, 0.6, dt, cuda)
    W, b, W64, _ = _params(rng, F, N, dt, cuda)
    teacher = rng.random((len(src), N)).astype(np.float32)
    deg = _check_backward(f"{dt} hot rows", dt, MF, h, h64, src, dst, lab, W, b, W64, teacher,
                          10.0, 100.0, -2.5)
    assert deg[:4].tolist() == fixed and (deg[4:8] == 0).all() and (deg[300:] == 0).all()
    # fewer pairs than one block, the wide shape
    F = N = 128
    src, dst, lab, n = _small_case(rng, N)
    h, h64 = _table(rng, n, F, 0.5, dt, cuda)
    W, b, W64, _ = _params(rng, F, N, dt, cuda)
    teacher = rng.random((len(src), N)).astype(np.float32)
    deg = _check_backward(f"{dt} small", dt, MF, h, h64, src, dst, lab, W, b, W64, teacher, 10.0,
                          100.0, -2.5)
    assert deg[7] == 0 and deg[n - 1] == 0
    # unequal widths
    F, N = 64, 16
    src, dst, lab, n = _small_case(rng, N, P=300, n=40)
    h, h64 = _table(rng, n, F, 0.5, dt, cuda)
    W, b, W64, _ = _params(rng, F, N, dt, cuda)
    teacher = rng.random((len(src), N)).astype(np.float32)
    _check_backward(f"{dt} 64x16", dt, MF, h, h64, src, dst, lab, W, b, W64, teacher, 1.0, 3.0, 1.0)


@pytest.mark.parametrize("FN", [(32, 32), (128, 128)], ids=["32x32", "128x128"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_gradients_match_torch_autograd(cuda, msha, dt, FN):
    """End to end against autograd of the device composition in fp64,

        out = sigmoid(relu(F.linear(h[src] * h[dst], W, b)));  wl nll_loss + wm mse_loss,

    at p = 0 and P = 777 (lattice table, pre-activations MARGIN away from the kink so both
    sides take the same ReLU branches, products exact in bf16).  The kernel's out is off by at most its own
    bound e_out = 4 sqrt(F + 8) 2^-24 Az / 4, and dz = g(out) out (1 - out) moves by at
    most (|dg/dout| / 4 + |g|) e_out with dg/dout = 2 wm gloss / (Pv N): the budget B of a dz
    element is |g| out (1 - out) + (|dg/dout| / 4 + |g|) Az / 4, and the A of dW, db, dH are
    the reference's absolute-term sums with |dz| replaced by B, the term counts grown by F."""
    from msha_gnn_amd import functional as MF

    F, N = FN
    rng = np.random.default_rng(21 + F)
    P, n, wl, wm, up = 777, 60, 10.0, 100.0, 2.0
    h, h64 = _lattice_table(rng, n, F, dt, cuda)
    W, b, W64, b64 = _params(rng, F, N, dt, cuda, scale=0.25)
    src, dst, lab, _ = _small_case(rng, N, P=P, n=n)
    src = _clear_of_kink(rng, h64, src, dst, W64, b64, 8, n - 1)  # rows 7, n - 1 stay empty
    teacher = rng.random((P, N)).astype(np.float32)
    ok, label = R.valid(src, dst, lab, n, N)
    f = R.forward(h64, src, dst, W64, b64, label=lab, teacher=teacher, w_label=wl, w_mse=wm)
    assert not (ok[:, None] & (np.abs(f["pre"]) < MARGIN)).any()
    # torch fp64 on the device, over the valid pairs (a padding pair adds nothing)
    idx = torch.as_tensor(np.flatnonzero(ok), device=cuda)
    ht = torch.tensor(h64, device=cuda, requires_grad=True)
    Wt = torch.tensor(W64, device=cuda, requires_grad=True)
    bt = torch.tensor(b64, device=cuda, requires_grad=True)
    ts, td, tl = _dev(src, cuda), _dev(dst, cuda), _dev(lab, cuda)
    tt = _dev(teacher, cuda)
    o_ref = torch.sigmoid(torch.relu(torch.nn.functional.linear(ht[ts[idx]] * ht[td[idx]], Wt, bt)))
    ref_loss = (wl * torch.nn.functional.nll_loss(o_ref, tl[idx])
                + wm * torch.nn.functional.mse_loss(o_ref, tt[idx].double()))
    (up * ref_loss).backward()
    hg = h.clone().requires_grad_(True)
    Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss = MF.link_mlp_loss(hg, ts, td, Wg, bg, label=tl, teacher_out=tt, w_label=wl, w_mse=wm)
    (up * loss).backward()
    assert hg.grad.dtype == DT[dt] and Wg.grad.dtype == torch.float32
    assert hg.grad.shape == hg.shape and Wg.grad.shape == W.shape and bg.grad.shape == b.shape
    pv = f["pv"]
    g = R.upstream(f["out"], ok, label, teacher.astype(np.float64), pv, wl, wm, up)
    o = np.where(ok[:, None], f["out"], 0.5)
    dg = 2.0 * wm * up / (pv * N)
    B = np.where(ok[:, None], np.abs(g) * o * (1 - o) + (dg / 4 + np.abs(g)) * f["Az"] / 4, 0.0)
    A = R.backward(h64, src, dst, W64, B, ok)
    split = 0.0  # a lattice table: bf16(h[s] * h[d]) is exact, nothing is rounded
    n_w = P + 1 + F + 8
    bounded_close(Wg.grad.cpu().numpy(), Wt.grad.cpu().numpy(), A["A_dW"], n_w, 1e-5,
                  f"{dt} {F}x{N} autograd dW", split_u=split)
    bounded_close(bg.grad.cpu().numpy(), bt.grad.cpu().numpy(), A["A_db"], n_w, 1e-5,
                  f"{dt} {F}x{N} autograd db", split_u=split)
    got = hg.grad.to(torch.float64).cpu().numpy()
    bounded_close(got, ht.grad.cpu().numpy(), A["A_dH"], A["deg"] + N + F + 8, 1e-5,
                  f"{dt} {F}x{N} autograd dH", split_u=split,
                  store_u=BF16_RNE if dt == "bf16" else 0.0)
    assert (got[A["deg"] == 0] == 0).all()
    lt = np.abs(wl * f["out"][ok, label[ok]] / pv).sum() + wm * f["l_mse"]
    bounded_close([float(loss.detach())], [float(ref_loss.detach())],
                  lt + (wl / pv + 2 * wm / (pv * N)) * 0.25 * f["Az"][ok].sum(), pv * N + F, 1e-5,
                  f"{dt} {F}x{N} loss against torch", split_u=split)


# ------------------------------------------------------------------- repeatability ---

@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_two_calls_and_a_fresh_plan_give_the_same_bits(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(3)
    n, F, N, P = 300, 32, 32, 5000
    h, _ = _table(rng, n, F, 0.6, dt, cuda)
    W, b, _, _ = _params(rng, F, N, dt, cuda)
    src, dst, lab = _padded_pairs(rng, P, n, N)
    dst[: P // 2] = rng.integers(0, 6, P // 2)  # hot rows: chunk partials
    ts, td, tl = _dev(src, cuda), _dev(dst, cuda), _dev(lab, cuda)
    tt = torch.rand(P, N, device=cuda)

    def run(plan):
        hg = h.clone().requires_grad_(True)
        Wg, bg = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        res = MF.link_mlp_loss(hg, ts, td, Wg, bg, label=tl, teacher_out=tt, w_label=10.0,
                               w_mse=100.0, p=0.3, training=True, seed=9, plan=plan,
                               return_output=True)
        res[0].backward()
        return [res[0].detach(), res[1], res[2], hg.grad, Wg.grad, bg.grad]

    first = run(None)
    for other in (run(None), run(MF.pair_plan(ts, td, n))):
        for x, y in zip(first, other):
            assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                               y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))


def test_table_gradient_is_a_function_of_each_rows_endpoint_order(cuda, msha):
    """fp32 h, p = 0.  Two pair lists hold the same pairs (with their labels and teacher
    rows): list 1 is group A followed by group B, list 2 interleaves them, each group in its
    own order.  A and B touch disjoint sets of table rows, so for every table row the pairs
    that name it as src, and the pairs that name it as dst, come in the same relative order
    in both lists.  Asserted: dH is bitwise equal (dW and db, summed by position blocks, are
    not claimed)."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(17)
    n, F, N, PA, PB = 200, 32, 32, 3000, 2500
    sa, da = rng.integers(0, 100, PA), rng.integers(0, 4, PA)        # rows 0..99, hot 0..3
    sb, db_ = rng.integers(100, n, PB), rng.integers(100, 104, PB)   # rows 100..199
    la, lb = rng.integers(0, N, PA), rng.integers(0, N, PB)
    ta, tb = rng.random((PA, N)).astype(np.float32), rng.random((PB, N)).astype(np.float32)
    sa[5], lb[9] = -1, N  # padding in each group
    cat = lambda x, y: np.concatenate([x, y])  # noqa: E731
    where = np.sort(rng.choice(PA + PB, PA, replace=False))  # list-2 positions of group A
    inv = np.empty(PA + PB, np.int64)
    inv[where] = np.arange(PA)
    inv[np.setdiff1d(np.arange(PA + PB), where)] = PA + np.arange(PB)
    h = _dev(rng.standard_normal((n, F)).astype(np.float32) * 0.6, cuda)
    W, b, _, _ = _params(rng, F, N, "fp32", cuda)

    def grad(order):
        hg = h.clone().requires_grad_(True)
        loss = MF.link_mlp_loss(hg, _dev(cat(sa, sb)[order], cuda), _dev(cat(da, db_)[order], cuda),
                                W, b, label=_dev(cat(la, lb)[order], cuda),
                                teacher_out=_dev(cat(ta, tb)[order], cuda), w_label=10.0,
                                w_mse=100.0)
        loss.backward()
        return hg.grad

    g1, g2 = grad(np.arange(PA + PB)), grad(inv)
    assert g1.abs().max() > 0 and torch.equal(g1, g2)


# ------------------------------------------------------------------------- capture ---

def test_plan_loss_backward_in_one_graph(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(5)
    n, F, N, P = 400, 32, 32, 5000
    h = (torch.as_tensor(rng.standard_normal((n, F)).astype(np.float32), device=cuda) * 0.5)
    h.requires_grad_(True)
    W, b, _, _ = _params(rng, F, N, "fp32", cuda)
    W.requires_grad_(True)
    b.requires_grad_(True)

    def batch():
        src = rng.integers(0, n, P)
        dst = rng.integers(0, 16, P)  # hot rows: chunk partials inside the graph
        src[rng.integers(0, P, 5)] = -1
        return (_dev(src.astype(np.int64), cuda), _dev(dst.astype(np.int64), cuda),
                _dev(rng.random((P, N)).astype(np.float32), cuda))

    def step(src, dst, teacher):
        plan = MF.pair_plan(src, dst, n)
        loss, out, terms = MF.link_mlp_loss(h, src, dst, W, b, teacher_out=teacher, w_label=10.0,
                                            w_mse=100.0, plan=plan, return_output=True)
        gh, gW, gb = torch.autograd.grad(loss, (h, W, b))
        return loss, out, terms, gh, gW, gb

    # The warm-up's results are dropped before the capture.  Kept, its loss would hold the
    # warm-up's autograd graph and with it the AccumulateGrad nodes of h, W and b made on the
    # default stream; the captured backward would then hand its gradients over to that stream
    # (an event wait on the default stream inside the capture), which breaks the capture.
    # What the graph reads and writes stays alive for the whole test: h, W, b, the static
    # batch and the captured outputs.
    statics = batch()
    step(*statics)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*statics)
    for _ in range(3):
        new = batch()
        for s, t in zip(statics, new):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*new)
        for got, want in zip(outs, eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))  # NaN rows included


# -------------------------------------------------------------------------- module ---

def test_llp_loss_is_the_functional(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rng = np.random.default_rng(2)
    n, F, P = 100, 32, 500
    h = torch.as_tensor(rng.standard_normal((n, F)).astype(np.float32), device=cuda) * 0.5
    src = _dev(rng.integers(0, n, P).astype(np.int64), cuda)
    dst = _dev(rng.integers(0, F, P).astype(np.int64), cuda)
    t_out = torch.rand(P, F, device=cuda)
    torch.manual_seed(1)
    pred = layers.LinkPredictor("mlp", F, F, 1, 2, 0.5).to(cuda).eval()
    fwd0 = pred(h[src], h[dst]).detach().clone()
    sp0 = pred.score_pairs(h, src, dst).detach().clone()
    a = h.clone().requires_grad_(True)
    la = pred.llp_loss(a, src, dst, teacher_out=t_out)
    la.backward()
    ga = [a.grad.clone(), pred.lins[0].weight.grad.clone(), pred.lins[0].bias.grad.clone()]
    assert pred.lins[1].weight.grad is None
    pred.zero_grad()
    c = h.clone().requires_grad_(True)
    lc, out, _ = MF.link_mlp_loss(c, src, dst, pred.lins[0].weight, pred.lins[0].bias,
                                  teacher_out=t_out, w_label=10.0, w_mse=100.0, p=0.5,
                                  training=False, return_output=True)
    lc.backward()
    gc = [c.grad, pred.lins[0].weight.grad, pred.lins[0].bias.grad]
    assert torch.equal(la, lc) and all(torch.equal(x, y) for x, y in zip(ga, gc))
    # the inference paths are what they were, and the loss's out is score_pairs' launch
    assert torch.equal(pred(h[src], h[dst]).detach(), fwd0)
    assert torch.equal(pred.score_pairs(h, src, dst).detach(), sp0)
    assert torch.equal(out, sp0)
    # explicit labels, a reused plan and the other defaults reach the functional too
    lab = _dev(rng.integers(0, F, P).astype(np.int64), cuda)
    plan = MF.pair_plan(src, dst, n)
    l1 = pred.llp_loss(h, src, dst, teacher_out=t_out, label=lab, true_label=2.0, kd_p=3.0,
                       plan=plan)
    l2 = MF.link_mlp_loss(h, src, dst, pred.lins[0].weight, pred.lins[0].bias, label=lab,
                          teacher_out=t_out, w_label=2.0, w_mse=3.0)
    assert torch.equal(l1, l2)
    # training mode draws the predictor's dropout
    pred.train()
    torch.manual_seed(5)
    lt = pred.llp_loss(h, src, dst, teacher_out=t_out)
    assert not torch.equal(lt, la.detach())
