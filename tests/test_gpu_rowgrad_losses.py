"""Row-sparse table training through link_mlp_loss, link_match_loss and sage_forward on the
device: the row lists (msha_link_match_rows, msha_sage_bwd_rows' own list), the compact
gradients against the dense gradient's bits and the losses' fp64 restatements, the union of
several row gradients of one table (msha_row_grad_union) against its numpy restatement and
dense accumulation, the optimizer steps against the dense optimizer and the lazy-Adam
restatement, the allocation bound, and whole steps captured into one HIP graph.

The pair lists are tests/test_gpu_rowadam.py's "small" (P = 777, n = 50) and "hot" (P = 40,000,
n = 5,000); the sage cases are ``sage_ref``'s (400 rows), shared with tests/test_gpu_sage.py."""
import numpy as np
import pytest
import torch

import link_mlp_ref as LR
import match_ref as MR
import rowadam_ref as AR
import rowunion_ref as U
import sage_ref as SR
from gpu_helpers import bounded_close, tol_close
from test_gpu_match import _terms as match_terms
from test_gpu_rowadam import (DT, PAIRS, _check_row_grad, _dev, _leaf, _load_state, _same_bits,
                              _small_pairs, _table)
from test_gpu_sage import _case as sage_case

pytestmark = pytest.mark.gpu

HOT = 5  # link_match_loss's hot row: more than 2,500 occurrences (test_gpu_match.py)


def _adam(params, accumulate=None, lr=1e-3):
    """msha Adam over ``params``; ``accumulate`` None: nothing registered, else the first
    parameter is registered with that keyword."""
    from msha_gnn_amd.optim import Adam

    opt = Adam(params, lr=lr)
    if accumulate is not None:
        opt.fuse_row_grad(params[0], accumulate=accumulate)
    return opt


def _pair(h, accumulate=False):
    """(registered leaf, its optimizer, unregistered leaf, its optimizer) from one table."""
    a, b = _leaf(h), _leaf(h)
    return a, _adam([a], accumulate), b, _adam([b])


def _match_rows(rng, n, P=3000):
    """P entries over n rows: the hot row 2,600 times, rows 7 and n - 1 never, padding entries
    -1 and n; shuffled."""
    rest = rng.integers(0, n, P - 2602)
    rest[rest == 7] = 8
    rest[rest == n - 1] = 0
    rows = np.concatenate([np.full(2600, HOT), rest, [-1, n]]).astype(np.int64)
    return rows[rng.permutation(P)]


def _mlp_inputs(rng, src, N, F, dt, dev):
    """(W, b, label, teacher_out) of a link_mlp_loss over the pair list."""
    P = len(src)
    W = _dev(rng.standard_normal((N, F)).astype(np.float32) / np.sqrt(F), dev)
    if dt == "bf16":
        W = W.to(torch.bfloat16).to(torch.float32)
    b = _dev((rng.standard_normal(N) * 0.2).astype(np.float32), dev)
    label = rng.integers(0, N, P)
    label[12], label[13] = N, -1  # padding by label
    return W, b, _dev(label.astype(np.int64), dev), _dev(rng.random((P, N)).astype(np.float32), dev)


def _sage_leaves(c, dev):
    """(registered table, W1, b1, W2, b2) and (unregistered table, W1, b1, W2, b2) leaves."""
    def leaves():
        return [torch.tensor(c[k], device=dev, requires_grad=True)
                for k in ("table", "W1", "b1", "W2", "b2")]

    return leaves(), leaves()


def _sage_graph(c, dev):
    from msha_gnn_amd.graph import graph_of

    adj = torch.tensor(c["adj"], device=dev)
    g, _ = graph_of(adj)
    return g, g.values(adj)


# ----------------------------------------------------------------- 1. the row lists ---

def _check_list(rg, ids, cap):
    want, cnt = U.listed(ids, cap)
    assert rg.rows.dtype == torch.int32 and rg.rows.shape == (cap,)
    assert rg.n_rows.dtype == torch.int32 and rg.n_rows.dim() == 0 and rg.n_rows.is_cuda
    assert int(rg.n_rows) == cnt
    assert np.array_equal(rg.rows.cpu().numpy(), want)
    assert (rg.values[cnt:] == 0).all()
    return cnt


def test_match_list_is_the_rows_that_occur(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(21)
    n, F = 50, 32
    rows = _match_rows(rng, n)
    a, oa, _, _ = _pair(_table(rng, n, F, torch.float32, cuda))
    T = _table(rng, n, F, torch.float32, cuda)
    loss, _, count = MF.link_match_loss(a, _dev(rows, cuda), T, return_rows=True)
    loss.backward()
    count = count.cpu().numpy()
    assert count[HOT] >= 2600 and count[7] == 0 and count[n - 1] == 0
    cnt = _check_list(oa.row_grad_of(a), np.flatnonzero(count), min(n, len(rows)))
    assert cnt == n - 2 and a.grad is None
    # long empty runs across scan tiles (4096 rows a tile), rows 0 and n - 1 among the named;
    # fewer entries than rows: the capacity is the entry count
    n = 100_000
    rows = rng.integers(0, n, 300)
    rows[0], rows[1], rows[2] = n - 1, 0, -1
    a, oa, _, _ = _pair(_table(rng, n, 16, torch.float32, cuda))
    T = _table(rng, n, 16, torch.float32, cuda)
    MF.link_match_loss(a, _dev(rows.astype(np.int64), cuda), T).backward()
    rg = oa.row_grad_of(a)
    cnt = _check_list(rg, rows[rows >= 0], 300)
    got = rg.rows.cpu().numpy()
    assert got[0] == 0 and got[cnt - 1] == n - 1 and cnt < 600
    # every entry padding: an empty list
    a, oa, _, _ = _pair(_table(rng, 50, 16, torch.float32, cuda))
    MF.link_match_loss(a, _dev(np.array([-1, 50, 77], np.int64), cuda),
                       _table(rng, 50, 16, torch.float32, cuda)).backward()
    assert _check_list(oa.row_grad_of(a), [], 3) == 0


@pytest.mark.parametrize("B", SR.BATCHES)
def test_sage_list_is_the_distinct_valid_sources(cuda, msha, B):
    from msha_gnn_amd import functional as MF

    c, _ = sage_case((32, 32, 32), B)
    (a, *wa), _ = _sage_leaves(c, cuda)
    oa = _adam([a], False)
    g, vals = _sage_graph(c, cuda)
    src = c["src"].copy()
    if B >= 65:
        assert len(np.unique(src)) < B   # repeated sources
        src[3] = SR.N_ROWS + 4           # one stray entry: no gradient, no row
    logp = MF.sage_forward(a, _dev(src, cuda), g, vals, *wa, check=False)
    w = torch.ones_like(logp)
    if B >= 65:
        assert torch.isnan(logp[3]).all()
        w[3] = 0
    logp.backward(w)
    assert a.grad is None
    rg = oa.row_grad_of(a)
    cnt = _check_list(rg, src[src < SR.N_ROWS], min(SR.N_ROWS, 2 * B))
    assert cnt == len(np.unique(src[src < SR.N_ROWS])) and torch.isfinite(rg.values).all()


def test_sage_list_across_scan_tiles(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import graph_of

    rng = np.random.default_rng(22)
    n, B = 100_000, 280
    adj = torch.zeros(n, 16, device=cuda)
    adj[torch.arange(n, device=cuda), torch.arange(n, device=cuda) % 16] = 0.5
    adj[:, 3] += 0.25
    g, _ = graph_of(adj)
    a = (torch.rand(n, 16, device=cuda)).requires_grad_(True)
    oa = _adam([a], False)
    W1, W2 = (torch.randn(16, 16, device=cuda) * 0.3 for _ in range(2))
    b1, b2 = (torch.randn(16, device=cuda) * 0.1 for _ in range(2))
    src = rng.integers(0, n, B)
    src[0], src[1], src[2] = n - 1, 0, 0
    MF.sage_forward(a, _dev(src.astype(np.int64), cuda), g, g.values(adj), W1, b1, W2,
                    b2).sum().backward()
    rg = oa.row_grad_of(a)
    cnt = _check_list(rg, src, 2 * B)
    got = rg.rows.cpu().numpy()
    assert got[0] == 0 and got[cnt - 1] == n - 1 and cnt < 600 and a.grad is None


# --------------------------- 2. the compact gradient is the dense gradient's rows ---

@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("FN", [(16, 16), (32, 32), (128, 128)], ids=["16x16", "32x32", "128x128"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("pairs", ["small", "hot"])
def test_mlp_row_grad_is_the_dense_gradient_rows(cuda, msha, pairs, dt, FN, p):
    from msha_gnn_amd import functional as MF

    F, N = FN
    rng = np.random.default_rng(31 + F)
    src, dst, n = PAIRS[pairs](rng)
    ts, td = _dev(src, cuda), _dev(dst, cuda)
    W, b, label, teacher = _mlp_inputs(rng, src, N, F, dt, cuda)
    a, oa, c, _ = _pair(_table(rng, n, F, DT[dt], cuda))
    plan = MF.pair_plan(ts, td, n)
    wgrads = []
    for t in (a, c):  # an upstream factor other than 1
        Wl, bl = _leaf(W), _leaf(b)
        loss = MF.link_mlp_loss(t, ts, td, Wl, bl, label=label, teacher_out=teacher, w_label=1.0,
                                w_mse=0.5, p=p, training=True, seed=77, plan=plan)
        (loss * 0.75).backward()
        wgrads.append((Wl.grad, bl.grad))
    assert a.grad is None and c.grad is not None and c.grad.shape == (n, F)
    assert oa.row_grad_of(a) is not None
    _check_row_grad(oa.row_grad_of(a), c.grad, n, F)
    for x, y in zip(*wgrads):
        assert x is not None and _same_bits(x, y)


@pytest.mark.parametrize("B", SR.BATCHES)
@pytest.mark.parametrize("widths", SR.WIDTHS, ids=[str(w) for w in SR.WIDTHS])
def test_sage_row_grad_is_the_dense_gradient_rows(cuda, msha, widths, B):
    from msha_gnn_amd import functional as MF

    c, _ = sage_case(widths, B)
    la, lb = _sage_leaves(c, cuda)
    oa = _adam([la[0]], False)
    g, vals = _sage_graph(c, cuda)
    src, target = _dev(c["src"], cuda), _dev(c["target"], cuda)
    for leaves in (la, lb):
        logp = MF.sage_forward(leaves[0], src, g, vals, *leaves[1:])
        (torch.nn.functional.nll_loss(logp, target) * 0.75).backward()
    a, b = la[0], lb[0]
    assert a.grad is None and b.grad is not None
    assert oa.row_grad_of(a) is not None
    rows, _ = _check_row_grad(oa.row_grad_of(a), b.grad, SR.N_ROWS, widths[0])
    assert rows.tolist() == np.unique(c["src"]).tolist()
    for x, y in zip(la[1:], lb[1:]):
        assert x.grad is not None and _same_bits(x.grad, y.grad)


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("td", ["fp32", "bf16"])
@pytest.mark.parametrize("hd", ["fp32", "bf16"])
def test_match_row_grad_is_the_dense_gradient_rows(cuda, msha, hd, td, F):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(41 + F)
    n, n_t = 50, 45
    rows = _dev(_match_rows(rng, n), cuda)
    a, oa, b, _ = _pair(_table(rng, n, F, DT[hd], cuda, 0.5))
    T = _table(rng, n_t, F, DT[td], cuda, 0.5)
    for t in (a, b):
        (MF.link_match_loss(t, rows, T) * -2.5).backward()
    assert a.grad is None and b.grad is not None
    assert oa.row_grad_of(a) is not None
    got, _ = _check_row_grad(oa.row_grad_of(a), b.grad, n, F)
    assert 7 not in got.tolist() and HOT in got.tolist()
    # rows=None names every row: the dense path, registered or not
    a2, oa2, b2, _ = _pair(_table(rng, n_t, F, DT[hd], cuda, 0.5))
    for t in (a2, b2):
        MF.link_match_loss(t, None, T).backward()
    assert oa2.row_grad_of(a2) is None and _same_bits(a2.grad, b2.grad)


# ------------------------------------------ 3. against the independent restatements ---

def test_mlp_row_grad_matches_the_fp64_restatement(cuda, msha):
    """tests/test_gpu_link_mlp.py's _check_backward bound for dH, on the row gradient."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(51)
    F = N = 32
    src, dst, n = _small_pairs(rng)
    ts, td = _dev(src, cuda), _dev(dst, cuda)
    W, b, label, teacher = _mlp_inputs(rng, src, N, F, "fp32", cuda)
    h = _table(rng, n, F, torch.float32, cuda, 0.6)
    a, oa, _, _ = _pair(h)
    wl, wm, gloss = 10.0, 100.0, -2.5
    loss, out, _ = MF.link_mlp_loss(a, ts, td, W, b, label=label, teacher_out=teacher, w_label=wl,
                                    w_mse=wm, return_output=True)
    (loss * gloss).backward()
    lab = label.cpu().numpy()
    ok, lab_ok = LR.valid(src, dst, lab, n, N)
    o64 = out.cpu().numpy().astype(np.float64)
    g = LR.upstream(o64, ok, lab_ok, teacher.double().cpu().numpy(), int(ok.sum()), wl, wm, gloss)
    mask = np.where(ok[:, None], o64, 0.5) > 0.5
    ref = LR.backward(h.double().cpu().numpy(), src, dst, W.double().cpu().numpy(),
                      LR.dz_from(o64, g, mask), ok)
    dH = oa.row_grad_of(a).to_dense().cpu().numpy()
    bounded_close(dH, ref["dH"], ref["A_dH"], ref["deg"] + N + 8, 1e-5, "mlp row gradient")
    assert (dH[ref["deg"] == 0] == 0).all() and dH.any()


def test_sage_row_grad_matches_the_fp64_restatement(cuda, msha):
    """tests/test_gpu_sage.py's bound for dS, on the row gradient."""
    from msha_gnn_amd import functional as MF

    widths, B = (32, 32, 32), 130
    c, refs = sage_case(widths, B)
    _, g64 = refs["nll"]
    (a, *wa), _ = _sage_leaves(c, cuda)
    oa = _adam([a], False)
    g, vals = _sage_graph(c, cuda)
    logp = MF.sage_forward(a, _dev(c["src"], cuda), g, vals, *wa)
    torch.nn.functional.nll_loss(logp, _dev(c["target"], cuda)).backward()
    dS = oa.row_grad_of(a).to_dense().cpu().numpy()
    bounded_close(dS, g64["dS"], g64["A_dS"], g64["n_dS"], 1e-5, "sage row gradient")
    assert dS.any()


def test_match_row_grad_matches_the_fp64_restatement(cuda, msha):
    """tests/test_gpu_match.py's bound for dH, on the row gradient."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(53)
    n, n_t, F, gloss = 50, 45, 32, -2.5
    rows = _match_rows(rng, n)
    h, T = _table(rng, n, F, torch.float32, cuda, 0.5), _table(rng, n_t, F, torch.float32, cuda, 0.5)
    a, oa, _, _ = _pair(h)
    (MF.link_match_loss(a, _dev(rows, cuda), T) * gloss).backward()
    h64, T64 = h.double().cpu().numpy(), T.double().cpu().numpy()
    ref = MR.forward(h64, T64, rows)
    want, A = MR.backward(h64, T64, ref["coef"], gloss)
    dH = oa.row_grad_of(a).to_dense().cpu().numpy()
    bounded_close(dH, want, A, match_terms(F), 1e-5, "match row gradient")
    assert dH[HOT].any() and not dH[7].any()


# ------------------------------------------------------------------------ 4. union ---

def _np_list(rg):
    return rg.rows.cpu().numpy(), int(rg.n_rows), rg.values.cpu().numpy()


def _check_union(merged, singles, n, dense=None):
    """The merged RowGrad against the numpy restatement of ``singles`` (in order) and, when
    given, the rows of the dense accumulated fp32 gradient."""
    rows, cnt, vals = U.union([_np_list(s) for s in singles], n)
    assert merged.rows.shape == rows.shape and int(merged.n_rows) == cnt
    assert np.array_equal(merged.rows.cpu().numpy(), rows)
    got = merged.values.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == vals.shape
    assert np.array_equal(got.view(np.int32), vals.view(np.int32))
    if dense is not None:
        ids = torch.as_tensor(rows[:cnt].astype(np.int64), device=dense.device)
        assert _same_bits(merged.values[:cnt], dense[ids])
        rest = torch.ones(n, dtype=torch.bool, device=dense.device)
        rest[ids] = False
        assert (dense[rest] == 0).all()
    return rows[:cnt]


class _LLP:
    """LLP.py:237-238's objective on one table: link_mlp_loss + 0.1 link_match_loss (rows =
    src) [+ link_bce_loss], over the "small" pair list."""

    def __init__(self, rng, dt, dev, F=32, N=32, match_rows=None):
        self.src, self.dst, self.n = _small_pairs(rng)
        self.F, self.dev = F, dev
        self.ts, self.td = _dev(self.src, dev), _dev(self.dst, dev)
        self.W, self.b, self.label, self.teacher = _mlp_inputs(rng, self.src, N, F, dt, dev)
        self.T = _table(rng, self.n, F, torch.float32, dev, 0.5)
        self.y = _dev(rng.random(len(self.src)).astype(np.float32), dev)
        self.h = _table(rng, self.n, F, DT[dt], dev)
        self.rows = self.ts if match_rows is None else _dev(match_rows, dev)

    def mlp(self, t, MF):
        return MF.link_mlp_loss(t, self.ts, self.td, self.W, self.b, label=self.label,
                                teacher_out=self.teacher, w_label=1.0, w_mse=0.5)

    def match(self, t, MF):
        return 0.1 * MF.link_match_loss(t, self.rows, self.T)

    def bce(self, t, MF):
        return 0.5 * MF.link_bce_loss(t, self.ts, self.td, self.y)

    def single(self, term, MF):
        """The RowGrad of one term alone, from a table registered without accumulate."""
        a = _leaf(self.h)
        opt = _adam([a], False)
        term(a, MF).backward()
        return opt.row_grad_of(a)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_union_of_the_llp_objective(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    L = _LLP(np.random.default_rng(61), dt, cuda)
    singles = [L.single(L.mlp, MF), L.single(L.match, MF)]
    a, oa, b, _ = _pair(L.h, accumulate=True)
    for t in (a, b):
        (L.mlp(t, MF) + L.match(t, MF)).backward()
    assert a.grad is None and len(a._msha_row_grads) == 2
    merged = oa.row_grad_of(a)
    assert oa.row_grad_of(a) is merged  # formed once
    # two lists: x1 + x2 = x2 + x1 in fp32, so the arrival order inside one backward is free
    ids = _check_union(merged, singles, L.n, b.grad if dt == "fp32" else None)
    held = [set(r[:c].tolist()) for r, c, _ in map(_np_list, singles)]
    assert set(ids.tolist()) == held[0] | held[1]
    assert 7 not in ids and (merged.rows[len(ids):] == -1).all()
    if dt == "fp32":
        assert torch.equal(merged.to_dense(), b.grad)
    # the same bits from a second run
    a2, oa2, _, _ = _pair(L.h, accumulate=True)
    (L.mlp(a2, MF) + L.match(a2, MF)).backward()
    again = oa2.row_grad_of(a2)
    assert torch.equal(again.rows, merged.rows) and _same_bits(again.values, merged.values)
    assert torch.equal(again.n_rows, merged.n_rows)


def test_union_of_three_lists_adds_left_to_right(cuda, msha):
    from msha_gnn_amd import functional as MF

    L = _LLP(np.random.default_rng(62), "fp32", cuda)
    L.rows = L.ts[:25]  # the matching term names some of the rows only
    terms = (L.mlp, L.match, L.bce)
    singles = [L.single(t, MF) for t in terms]
    assert 0 < int(singles[1].n_rows) < int(singles[0].n_rows) == int(singles[2].n_rows)
    a, oa, b, _ = _pair(L.h, accumulate=True)
    for t in (a, b):
        for term in terms:  # three backwards: the arrival order is the call order
            term(t, MF).backward()
    assert len(a._msha_row_grads) == 3 and a.grad is None
    _check_union(oa.row_grad_of(a), singles, L.n, b.grad)
    # the order is part of the result: some element differs when the lists are permuted
    _, _, other = U.union([_np_list(s) for s in (singles[2], singles[1], singles[0])], L.n)
    got = oa.row_grad_of(a).values.cpu().numpy()
    assert not np.array_equal(got.view(np.int32), other.view(np.int32))


def test_union_with_an_empty_list(cuda, msha):
    from msha_gnn_amd import functional as MF

    pad = np.array([-1, 50, 60, -7], np.int64)  # every entry padding: a list of count 0
    L = _LLP(np.random.default_rng(63), "fp32", cuda, match_rows=pad)
    singles = [L.single(L.mlp, MF), L.single(L.match, MF)]
    assert int(singles[1].n_rows) == 0 and (singles[1].rows == -1).all()
    a, oa, b, _ = _pair(L.h, accumulate=True)
    for t in (a, b):
        L.mlp(t, MF).backward()
        L.match(t, MF).backward()
    merged = oa.row_grad_of(a)
    ids = _check_union(merged, singles, L.n, b.grad)
    assert ids.tolist() == _np_list(singles[0])[0][:len(ids)].tolist()
    assert merged.rows.numel() == min(L.n, singles[0].rows.numel() + 4)


# ------------------------------------------------------------------------ 5. steps ---

def _step_state(p, opt):
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def _check_step(a, oa, b, ob, start, touched, n):
    """After one step of each: the touched rows carry the dense optimizer's bits, the others
    their bits from before; one step counted."""
    ids = _dev(np.asarray(touched, np.int64), a.device)
    rest = torch.ones(n, dtype=torch.bool, device=a.device)
    rest[ids] = False
    assert 0 < len(touched) < n
    for name, ta, tb, t0 in zip("pmv", _step_state(a, oa), _step_state(b, ob), start):
        assert _same_bits(ta[ids], tb[ids]), name
        assert name != "m" or not _same_bits(ta[ids], t0[ids])
        assert _same_bits(ta[rest], t0[rest]), name
    assert float(oa.state[a]["step"]) == 4.0 == float(ob.state[b]["step"])
    assert a.grad is None and oa.row_grad_of(a) is None and b.grad is not None


def _start_state(rng, n, F, dev):
    return (_table(rng, n, F, torch.float32, dev), _table(rng, n, F, torch.float32, dev, 1e-3),
            _table(rng, n, F, torch.float32, dev, 1e-3).abs())


def test_sage_step_is_the_dense_step_on_the_batch_rows(cuda, msha):
    from msha_gnn_amd import functional as MF

    widths, B = (32, 32, 32), 130
    c, _ = sage_case(widths, B)
    rng = np.random.default_rng(71)
    p0, m0, v0 = _start_state(rng, SR.N_ROWS, widths[0], cuda)
    a, oa, b, ob = _pair(p0)
    g, vals = _sage_graph(c, cuda)
    ws = [_dev(c[k], cuda) for k in ("W1", "b1", "W2", "b2")]
    for t, opt in ((a, oa), (b, ob)):
        _load_state(opt, t, m0, v0, 3)
        opt.zero_grad()
        logp = MF.sage_forward(t, _dev(c["src"], cuda), g, vals, *ws)
        torch.nn.functional.nll_loss(logp, _dev(c["target"], cuda)).backward()
        opt.step()
    _check_step(a, oa, b, ob, (p0, m0, v0), np.unique(c["src"]), SR.N_ROWS)


def test_llp_step_is_the_dense_step_on_the_touched_rows(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(72)
    L = _LLP(rng, "fp32", cuda)
    p0, m0, v0 = _start_state(rng, L.n, L.F, cuda)
    a, oa, b, ob = _pair(p0, accumulate=True)
    for t, opt in ((a, oa), (b, ob)):
        _load_state(opt, t, m0, v0, 3)
        opt.zero_grad()
        (L.mlp(t, MF) + L.match(t, MF)).backward()
        opt.step()
    ok = (L.src >= 0) & (L.src < L.n) & (L.dst >= 0) & (L.dst < L.n)
    touched = np.union1d(np.concatenate([L.src[ok], L.dst[ok]]), L.src[(L.src >= 0) & (L.src < L.n)])
    _check_step(a, oa, b, ob, (p0, m0, v0), touched, L.n)


@pytest.mark.parametrize("which", ["sage", "llp"])
def test_five_step_schedule_matches_the_restatement(cuda, msha, which):
    """tests/test_gpu_rowadam.py's test_sparse_schedule_matches_the_restatement, with its bound."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(73)
    lr = 1e-3
    if which == "sage":
        c, _ = sage_case((32, 32, 32), 65)
        n, F = SR.N_ROWS, 32
        g, vals = _sage_graph(c, cuda)
        ws = [_dev(c[k], cuda) for k in ("W1", "b1", "W2", "b2")]
        a = _leaf(_dev(c["table"], cuda))
    else:
        L = _LLP(rng, "fp32", cuda)
        n, F = 2000, L.F
        L.T = _table(rng, n, F, torch.float32, cuda, 0.5)
        a = _leaf(_table(rng, n, F, torch.float32, cuda))
    opt = _adam([a], which == "llp", lr=lr)
    p = a.detach().cpu().numpy().astype(np.float64)
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    for _ in range(5):
        before = [x.clone() for x in (a.detach(), *(opt.state[a].get(k, torch.zeros_like(a))
                                                    for k in ("exp_avg", "exp_avg_sq")))]
        opt.zero_grad()
        if which == "sage":
            src = rng.integers(0, n, 65).astype(np.int64)
            logp = MF.sage_forward(a, _dev(src, cuda), g, vals, *ws)
            torch.nn.functional.nll_loss(logp, _dev(c["target"], cuda)).backward()
            want = np.unique(src)
        else:
            P = len(L.src)
            src, dst = rng.integers(0, n, P), rng.integers(0, n, P)
            L.ts, L.td = _dev(src.astype(np.int64), cuda), _dev(dst.astype(np.int64), cuda)
            L.rows = L.ts
            (L.mlp(a, MF) + L.match(a, MF)).backward()
            want = np.unique(np.concatenate([src, dst]))
        rg = opt.row_grad_of(a)
        cnt = int(rg.n_rows)
        rows = rg.rows[:cnt].cpu().numpy()
        assert 0 < cnt < n and np.array_equal(rows, want)
        t = AR.lazy_adam_step(p, m, v, t, rows, rg.values[:cnt].cpu().numpy(), lr=lr)
        opt.step()
        rest = torch.ones(n, dtype=torch.bool, device=cuda)
        rest[rg.rows[:cnt].to(torch.int64)] = False
        for x0, x1 in zip(before, _step_state(a, opt)):
            assert _same_bits(x0[rest], x1[rest])
    assert float(opt.state[a]["step"]) == 5.0 == t and a.grad is None
    tol_close(a.detach().cpu().numpy(), p, 1e-6, 1e-6)
    tol_close(opt.state[a]["exp_avg"].cpu().numpy(), m, 1e-6, 1e-6)
    tol_close(opt.state[a]["exp_avg_sq"].cpu().numpy(), v, 1e-6, 1e-6)


# ------------------------------------------------------------ 6. no dense buffer ---

@pytest.mark.parametrize("which", ["sage", "mlp"])
def test_no_table_sized_buffer_in_backward_and_step(cuda, msha, which):
    """A 128 MB table: backward + step() allocate less than half of it (the row list's and the
    union's n-int workspaces, 4 MB each, fit; the dense path's (n, F) gradient does not)."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import graph_of

    rng = np.random.default_rng(81)
    n, F = 1 << 20, 32
    a = (torch.rand(n, F, device=cuda) * 0.1).requires_grad_(True)
    opt = _adam([a], False)
    table_bytes = n * F * 4
    if which == "sage":
        B, M = 512, 16
        adj = torch.zeros(n, M, device=cuda)
        adj[torch.arange(n, device=cuda), torch.arange(n, device=cuda) % M] = 0.5
        adj[:, 1] += 0.25
        g, _ = graph_of(adj)
        vals = g.values(adj)
        W1, W2 = torch.randn(M, F, device=cuda) * 0.2, torch.randn(16, M, device=cuda) * 0.2
        b1, b2 = torch.zeros(M, device=cuda), torch.zeros(16, device=cuda)
        cap = 2 * B

        def loss():
            src = _dev(rng.integers(0, n, B).astype(np.int64), cuda)
            logp = MF.sage_forward(a, src, g, vals, W1, b1, W2, b2, check=False)
            return torch.nn.functional.nll_loss(logp, _dev(rng.integers(0, 16, B), cuda))
    else:
        P, N = 1000, 32
        W, b = torch.randn(N, F, device=cuda) * 0.2, torch.zeros(N, device=cuda)
        cap = 2 * P

        def loss():
            src, dst = (_dev(rng.integers(0, n, P).astype(np.int64), cuda) for _ in range(2))
            return MF.link_mlp_loss(a, src, dst, W, b, label=_dev(rng.integers(0, N, P), cuda))

    opt.zero_grad()
    loss().backward()  # warm-up: the moments and the workspaces exist
    opt.step()
    assert a.grad is None
    opt.zero_grad()
    out = loss()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    out.backward()
    assert a.grad is None and opt.row_grad_of(a).values.shape == (cap, F)
    opt.step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(cuda) - base
    assert peak < table_bytes // 2, (peak, table_bytes)
    assert a.grad is None and float(opt.state[a]["step"]) == 2.0


# ------------------------------------------------------------------- 7. capture ---

def test_whole_steps_in_one_graph(cuda, msha):
    """plan + link_mlp_loss + link_match_loss + backward + union + step(), and sage_forward +
    nll + backward + step(), each captured into one HIP graph (as tests/test_gpu_rowadam.py's
    test_whole_step_in_one_graph) and replayed three times on fresh batches: the bits of the
    eager schedule."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(91)
    n, F, N, P = 4000, 32, 32, 500
    h = _table(rng, n, F, torch.float32, cuda)
    T = _table(rng, n, F, torch.float32, cuda, 0.5)
    W = _dev(rng.standard_normal((N, F)).astype(np.float32) / np.sqrt(F), cuda)
    b = _dev((rng.standard_normal(N) * 0.2).astype(np.float32), cuda)

    def llp_batch(repeats=0):
        src, dst = rng.integers(0, n, P), rng.integers(0, n, P)
        src[:150 * repeats], dst[:150 * repeats] = 3, 3  # fewer distinct rows
        src[rng.integers(0, P, 5)] = -1
        return (_dev(src.astype(np.int64), cuda), _dev(dst.astype(np.int64), cuda),
                _dev(rng.integers(0, N, P), cuda), _dev(rng.random((P, N)).astype(np.float32), cuda))

    def llp_step(p, opt, src, dst, label, teacher):
        opt.zero_grad()
        plan = MF.pair_plan(src, dst, n)
        loss = MF.link_mlp_loss(p, src, dst, W, b, label=label, teacher_out=teacher, w_mse=0.5,
                                plan=plan) + 0.1 * MF.link_match_loss(p, src, T)
        loss.backward()
        n_rows = opt.row_grad_of(p).n_rows  # the merged list's count
        opt.step()
        return n_rows

    c, _ = sage_case((32, 32, 32), 65)
    g, vals = _sage_graph(c, cuda)
    ws = [_dev(c[k], cuda) for k in ("W1", "b1", "W2", "b2")]

    def sage_batch(repeats=0):
        src = rng.integers(0, SR.N_ROWS, 65)
        src[:20 * repeats] = 3
        return _dev(src.astype(np.int64), cuda), _dev(rng.integers(0, 32, 65), cuda)

    def sage_step(p, opt, src, target):
        opt.zero_grad()
        logp = MF.sage_forward(p, src, g, vals, *ws, check=False)
        torch.nn.functional.nll_loss(logp, target).backward()
        n_rows = opt.row_grad_of(p).n_rows
        opt.step()
        return n_rows

    def state(p, opt):
        return (*_step_state(p, opt), opt.state[p]["step"])

    for step, batch, table, accumulate in ((llp_step, llp_batch, h, True),
                                           (sage_step, sage_batch, _dev(c["table"], cuda), False)):
        p, q = _leaf(table), _leaf(table)
        opt, oq = _adam([p], accumulate, lr=1e-2), _adam([q], accumulate, lr=1e-2)
        warm = batch()
        statics = [t.clone() for t in warm]
        step(p, opt, *statics)  # warm-up outside the capture
        step(q, oq, *warm)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            n_rows = step(p, opt, *statics)
        counts = []
        for k in range(3):
            new = batch(repeats=k)
            for s, t in zip(statics, new):
                s.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            counts.append((int(n_rows), int(step(q, oq, *new))))
            for got, want in zip(state(p, opt), state(q, oq)):
                assert _same_bits(got, want)
            assert float(opt.state[p]["step"]) == 2.0 + k
        assert all(x == y for x, y in counts)
        assert len({x for x, _ in counts}) == 3  # the row count is read on the device
        assert p.grad is None
