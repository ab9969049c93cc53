"""Row-sparse table training on the device: the touched-row list of a plan (msha_plan_rows),
the compact row gradient (msha_link_bce_bwd_rows / msha_pair_grad_bwd_rows) against the
dense gradient's bits, the lazy Adam over the rows (msha_adam_rows_step) against the dense
optimizer's bits and the fp64 restatement (``rowadam_ref``), the Python rules of
``optim.Adam.fuse_row_grad``, and the capture of a whole training step into one HIP graph.

The pair lists restate the shapes of tests/test_gpu_link_loss.py: "small" (P = 777, n = 50:
rows no pair names, self pairs, padding pairs) and "hot" (P = 40,000, n = 5,000: rows of
chunk - 1, chunk, chunk + 1, 2 chunk and more than two chunks of endpoints)."""
import copy

import numpy as np
import pytest
import torch

import rowadam_ref as R
from gpu_helpers import tol_close

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _dev(x, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _chunk():
    from msha_gnn_amd import _lib

    return int(_lib.load().msha_pair_plan_chunk())


def _hot_pairs(rng):
    chunk = _chunk()
    P = 40_000
    fixed = [chunk - 1, chunk, chunk + 1, 2 * chunk]
    rest = P - sum(fixed)
    per = np.full(28, rest // 28)
    per[: rest % 28] += 1
    assert per.min() > 2 * chunk
    dst = np.repeat(np.arange(32), np.concatenate([fixed, per]))
    dst = dst[rng.permutation(P)]
    src = rng.integers(32, 5000, P)
    return src.astype(np.int64), dst.astype(np.int64), 5000


def _small_pairs(rng, P=777, n=50):
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


PAIRS = {"small": _small_pairs, "hot": _hot_pairs}


def _table(rng, n, F, dtype, dev, scale=0.3):
    return _dev(rng.standard_normal((n, F)).astype(np.float32) * scale, dev, dtype)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


# ----------------------------------------------------------------- 1. the row list ---

def _check_rows(MF, src, dst, n, dev):
    ts, td = _dev(src, dev), _dev(dst, dev)
    plan = MF.pair_plan(ts, td, n)
    rows, n_rows = MF.plan_rows(plan)
    assert MF.plan_rows(plan)[0] is rows  # kept on the plan
    again, n_again = MF.plan_rows(MF.pair_plan(ts, td, n))
    cap = min(n, 2 * len(src))
    want, cnt = R.touched_rows(plan.rowptr.cpu().numpy(), cap)
    assert rows.dtype == torch.int32 and rows.shape == (cap,)
    assert n_rows.dtype == torch.int32 and n_rows.dim() == 0 and n_rows.is_cuda
    assert int(n_rows) == cnt
    assert np.array_equal(rows.cpu().numpy(), want)
    assert torch.equal(rows, again) and torch.equal(n_rows, n_again)
    return want, cnt


def test_plan_rows_matches_the_restatement(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(1)
    src, dst, n = _small_pairs(rng)
    want, cnt = _check_rows(MF, src, dst, n, cuda)
    assert 7 not in want and n - 1 not in want and cnt == n - 2
    src, dst, n = _hot_pairs(rng)
    _, cnt = _check_rows(MF, src, dst, n, cuda)
    assert 32 < cnt <= n
    # long empty runs across scan tiles (4096 rows a tile), the last row touched
    n = 100_000
    src, dst = rng.integers(0, n, 300), rng.integers(0, n, 300)
    src[0], dst[0], src[1] = n - 1, 0, -1
    want, cnt = _check_rows(MF, src, dst, n, cuda)
    assert want[0] == 0 and want[cnt - 1] == n - 1 and cnt < 600
    _, cnt = _check_rows(MF, np.array([0]), np.array([0]), 1, cuda)           # n = 1
    assert cnt == 1
    _, cnt = _check_rows(MF, np.full(5, -1), np.array([3, 10, 0, -1, 2]), 10, cuda)
    assert cnt == 0                                                           # all padding


# ------------------------------------------------------- 2. the compact gradient ---

def _registered(h):
    """(registered leaf, its optimizer, unregistered leaf, its optimizer) from one table."""
    from msha_gnn_amd.optim import Adam

    a, b = _leaf(h), _leaf(h)
    oa, ob = Adam([a], lr=1e-3), Adam([b], lr=1e-3)
    oa.fuse_row_grad(a)
    return a, oa, b, ob


def _check_row_grad(rg, dense, n, F):
    """RowGrad against the dense gradient of the unregistered clone."""
    cap = rg.rows.numel()
    cnt = int(rg.n_rows)
    assert rg.shape == (n, F) and rg.values.shape == (cap, F)
    assert rg.values.dtype == torch.float32
    rows = rg.rows[:cnt].to(torch.int64)
    assert cnt > 0 and (rg.rows[cnt:] == -1).all()
    vals = rg.values[:cnt]
    if dense.dtype == torch.bfloat16:
        vals = vals.to(torch.bfloat16)
    assert _same_bits(vals, dense[rows])
    rest = torch.ones(n, dtype=torch.bool, device=dense.device)
    rest[rows] = False
    assert (dense[rest] == 0).all()
    assert (rg.values[cnt:] == 0).all()
    if dense.dtype == torch.float32:
        assert torch.equal(rg.to_dense(), dense)
    return rows, rest


@pytest.mark.parametrize("F", [16, 32, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("pairs", ["small", "hot"])
def test_row_grad_is_the_dense_gradient_rows(cuda, msha, pairs, dt, F):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(7 + F)
    src, dst, n = PAIRS[pairs](rng)
    P = len(src)
    ts, td = _dev(src, cuda), _dev(dst, cuda)
    y = _dev(rng.random(P).astype(np.float32), cuda)
    w = _dev(rng.random(P).astype(np.float32) / P, cuda) if F == 32 else None
    a, oa, b, _ = _registered(_table(rng, n, F, DT[dt], cuda))
    plan = MF.pair_plan(ts, td, n)
    for t in (a, b):  # an upstream factor other than 1
        (MF.link_bce_loss(t, ts, td, y, weight=w, plan=plan) * 0.75).backward()
    assert a.grad is None and b.grad is not None and b.grad.shape == (n, F)
    _check_row_grad(oa.row_grad_of(a), b.grad, n, F)


def _distill_lists(rng, which):
    if which == "hot":  # test_gpu_distill's hot row: one anchor node, four context nodes
        chunk = _chunk()
        A, K, n = 5 * chunk // 8 + 3, 8, 50
        anchors = np.full(A, 17, np.int64)
        ctx = rng.choice(np.array([2, 17, 30, 49]), (A, K)).astype(np.int64)
    else:  # K not a power of two, padding slots
        A, K, n = 37, 5, 60
        anchors = rng.integers(0, n, A).astype(np.int64)
        ctx = rng.integers(0, n, (A, K)).astype(np.int64)
        anchors[1], anchors[2] = -1, n
        ctx[0, 2], ctx[4, :] = -1, -1
    return anchors, ctx, n


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["hot", "k5"])
def test_distill_row_grad_is_the_dense_gradient_rows(cuda, msha, which, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(13)
    anchors, ctx, n = _distill_lists(rng, which)
    F = 32
    ta, tc = _dev(anchors, cuda), _dev(ctx, cuda)
    tl = _dev((np.round(rng.standard_normal(ctx.shape) * 6) / 4).astype(np.float32), cuda)
    a, oa, b, _ = _registered(_table(rng, n, F, DT[dt], cuda, 0.5))
    plan = MF.context_plan(ta, tc, n)
    for t in (a, b):
        (MF.link_distill_loss(t, ta, tc, teacher_logits=tl, w_prob=0.5, plan=plan) * 1.5).backward()
    assert a.grad is None and b.grad is not None
    rows, _ = _check_row_grad(oa.row_grad_of(a), b.grad, n, F)
    if which == "hot":
        assert rows.tolist() == [2, 17, 30, 49]
        deg = np.diff(plan.rowptr.cpu().numpy())
        assert deg[17] > 2 * _chunk()


# ------------------------------------------- 3. one step against the dense optimizer ---

def _load_state(opt, p, m, v, step):
    opt.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32, device=p.device),
                    "exp_avg": m.clone(), "exp_avg_sq": v.clone()}


def _bce_step(MF, opt, p, ts, td, y, plan=None):
    opt.zero_grad()
    MF.link_bce_loss(p, ts, td, y, plan=plan).backward()
    opt.step()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("pairs", ["small", "hot"])
def test_one_step_is_the_dense_step_on_the_touched_rows(cuda, msha, pairs, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(3)
    src, dst, n = PAIRS[pairs](rng)
    F, P = 32, len(src)
    ts, td = _dev(src, cuda), _dev(dst, cuda)
    y = _dev((rng.random(P) < 0.5).astype(np.float32), cuda)
    p0 = _table(rng, n, F, DT[dt], cuda)
    m0 = _table(rng, n, F, DT[dt], cuda, 1e-3)
    v0 = _table(rng, n, F, DT[dt], cuda, 1e-3).abs()
    a, oa, b, ob = _registered(p0)
    _load_state(oa, a, m0, v0, 3)
    _load_state(ob, b, m0, v0, 3)
    plan = MF.pair_plan(ts, td, n)
    rows, cnt = R.touched_rows(plan.rowptr.cpu().numpy())
    _bce_step(MF, oa, a, ts, td, y, plan)
    _bce_step(MF, ob, b, ts, td, y, plan)
    assert a.grad is None and oa.row_grad_of(a) is None and b.grad is not None
    rows = _dev(rows.astype(np.int64), cuda)
    rest = torch.ones(n, dtype=torch.bool, device=cuda)
    rest[rows] = False
    assert 0 < cnt <= n and int(rest.sum()) == n - cnt
    assert pairs == "hot" or cnt == n - 2  # rows 7 and n - 1 of the small list are untouched
    for name, ta, tb, t0 in (("p", a.detach(), b.detach(), p0),
                             ("m", oa.state[a]["exp_avg"], ob.state[b]["exp_avg"], m0),
                             ("v", oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"], v0)):
        assert _same_bits(ta[rows], tb[rows]), name        # the dense optimizer's bits
        # ... and the step was taken (a bf16 v or p can round back to itself; m moves by a
        # tenth of its distance to the gradient)
        assert name != "m" or not _same_bits(ta[rows], t0[rows])
        assert _same_bits(ta[rest], t0[rest]), name         # untouched rows: unchanged
    assert float(oa.state[a]["step"]) == 4.0 and float(ob.state[b]["step"]) == 4.0


# --------------------------------------------------------- 4. every-row schedule ---

@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_every_row_schedule_is_the_dense_optimizer(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(4)
    n, F, P = 400, 32, 5000
    a, oa, b, ob = _registered(_table(rng, n, F, DT[dt], cuda))
    for _ in range(5):
        src = np.concatenate([rng.permutation(n), rng.integers(0, n, P - n)]).astype(np.int64)
        dst = rng.integers(0, 16, P).astype(np.int64)  # hot rows: chunk partials
        ts, td = _dev(src, cuda), _dev(dst, cuda)
        y = _dev(rng.random(P).astype(np.float32), cuda)
        _bce_step(MF, oa, a, ts, td, y)
        _bce_step(MF, ob, b, ts, td, y)
    assert a.grad is None
    assert _same_bits(a.detach(), b.detach())
    for k in ("exp_avg", "exp_avg_sq"):
        assert _same_bits(oa.state[a][k], ob.state[b][k]), k
    assert float(oa.state[a]["step"]) == 5.0 == float(ob.state[b]["step"])


# ------------------------------------- 5. sparse schedule against the restatement ---

def test_sparse_schedule_matches_the_restatement(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    rng = np.random.default_rng(5)
    n, F, P, lr = 5000, 32, 500, 1e-3
    a = _leaf(_table(rng, n, F, torch.float32, cuda))
    opt = Adam([a], lr=lr)
    opt.fuse_row_grad(a)
    p = a.detach().cpu().numpy().astype(np.float64)
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    for _ in range(5):
        src = rng.integers(0, n, P).astype(np.int64)
        dst = rng.integers(0, n, P).astype(np.int64)
        ts, td = _dev(src, cuda), _dev(dst, cuda)
        y = _dev((rng.random(P) < 0.5).astype(np.float32), cuda)
        before = [x.clone() for x in (a.detach(), *(opt.state[a].get(k, torch.zeros_like(a))
                                                    for k in ("exp_avg", "exp_avg_sq")))]
        opt.zero_grad()
        MF.link_bce_loss(a, ts, td, y).backward()
        rg = opt.row_grad_of(a)
        cnt = int(rg.n_rows)
        rows = rg.rows[:cnt].cpu().numpy()
        assert 0 < cnt <= 2 * P and np.array_equal(rows, np.unique(np.concatenate([src, dst])))
        t = R.lazy_adam_step(p, m, v, t, rows, rg.values[:cnt].cpu().numpy(), lr=lr)
        opt.step()
        rest = torch.ones(n, dtype=torch.bool, device=cuda)
        rest[rg.rows[:cnt].to(torch.int64)] = False
        after = (a.detach(), opt.state[a]["exp_avg"], opt.state[a]["exp_avg_sq"])
        for x0, x1 in zip(before, after):
            assert _same_bits(x0[rest], x1[rest])
    assert float(opt.state[a]["step"]) == 5.0 == t
    tol_close(a.detach().cpu().numpy(), p, 1e-6, 1e-6)
    tol_close(opt.state[a]["exp_avg"].cpu().numpy(), m, 1e-6, 1e-6)
    tol_close(opt.state[a]["exp_avg_sq"].cpu().numpy(), v, 1e-6, 1e-6)


# ------------------------------------------------------------ 6. no dense buffer ---

def test_no_table_sized_buffer_in_backward_and_step(cuda, msha):
    """A 128 MB table, 1,000 pairs: backward + step() allocate far less than the table (the
    dense path allocates the (n, F) gradient, and torch keeps it as .grad)."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    rng = np.random.default_rng(6)
    n, F, P = 1 << 20, 32, 1000
    a = (torch.randn(n, F, device=cuda) * 0.1).requires_grad_(True)
    opt = Adam([a], lr=1e-3)
    opt.fuse_row_grad(a)
    table_bytes = n * F * 4

    def batch():
        return (_dev(rng.integers(0, n, P).astype(np.int64), cuda),
                _dev(rng.integers(0, n, P).astype(np.int64), cuda),
                _dev((rng.random(P) < 0.5).astype(np.float32), cuda))

    _bce_step(MF, opt, a, *batch())  # warm-up: the moments and the workspaces exist
    assert a.grad is None
    ts, td, y = batch()
    opt.zero_grad()
    loss = MF.link_bce_loss(a, ts, td, y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    loss.backward()
    assert a.grad is None and opt.row_grad_of(a).values.shape == (2 * P, F)
    opt.step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(cuda) - base
    assert peak < table_bytes // 2, (peak, table_bytes)
    assert a.grad is None and float(opt.state[a]["step"]) == 2.0


# --------------------------------------------------------------------- 7. rules ---

def test_rules_of_the_registered_table(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    rng = np.random.default_rng(8)
    src, dst, n = _small_pairs(rng)
    F, P = 16, len(src)
    ts, td = _dev(src, cuda), _dev(dst, cuda)
    y = _dev(rng.random(P).astype(np.float32), cuda)
    h = _table(rng, n, F, torch.float32, cuda)
    a, oa, b, ob = _registered(h)
    # one row gradient per step
    MF.link_bce_loss(a, ts, td, y).backward()
    with pytest.raises(RuntimeError, match="second backward before step"):
        MF.link_bce_loss(a, ts, td, y).backward()
    # a .grad beside the row gradient: another consumer
    a.grad = torch.zeros_like(a)
    with pytest.raises(RuntimeError, match="another consumer"):
        oa.step()
    oa.zero_grad()
    assert a.grad is None and oa.row_grad_of(a) is None
    # zero_grad drops the stash
    MF.link_bce_loss(a, ts, td, y).backward()
    assert oa.row_grad_of(a) is not None
    oa.zero_grad()
    assert oa.row_grad_of(a) is None and a.grad is None
    # not the leaf itself: the dense path
    MF.link_bce_loss(a * 1.0, ts, td, y).backward()
    assert oa.row_grad_of(a) is None and a.grad is not None and a.grad.shape == (n, F)
    # an unregistered table: as before
    MF.link_bce_loss(b, ts, td, y).backward()
    assert b.grad is not None and b.grad.shape == (n, F) and not b.grad.is_sparse
    assert torch.equal(a.grad, b.grad) and ob.row_grad_of(b) is None
    oa.step()  # a registered table with a dense .grad alone takes the dense step
    ob.step()
    assert _same_bits(a.detach(), b.detach())
    # state_dict: dense moments and a scalar step, through torch.optim.Adam and back
    oa.zero_grad()
    _bce_step(MF, oa, a, ts, td, y)
    sd = copy.deepcopy(oa.state_dict())  # (a state_dict holds the optimizer's own tensors)
    st = sd["state"][0]
    assert st["exp_avg"].shape == (n, F) and st["exp_avg_sq"].shape == (n, F)
    assert float(st["step"]) == 2.0
    c = _leaf(a)
    ot = torch.optim.Adam([c], lr=1e-3)
    ot.load_state_dict(sd)
    d = _leaf(a)
    od = Adam([d], lr=1e-3)
    od.load_state_dict(ot.state_dict())
    od.fuse_row_grad(d)
    assert float(od.state[d]["step"]) == 2.0
    for k in ("exp_avg", "exp_avg_sq"):
        assert _same_bits(od.state[d][k], oa.state[a][k])
    _bce_step(MF, oa, a, ts, td, y)
    _bce_step(MF, od, d, ts, td, y)
    assert _same_bits(a.detach(), d.detach()) and float(od.state[d]["step"]) == 3.0


# ------------------------------------------------------------------- 8. capture ---

def test_whole_step_in_one_graph(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    rng = np.random.default_rng(9)
    n, F, P = 4000, 32, 500
    h = _table(rng, n, F, torch.float32, cuda)

    def batch(repeats=0):
        src = rng.integers(0, n, P)
        dst = rng.integers(0, n, P)
        src[:repeats], dst[:repeats] = 3, 3  # fewer distinct rows
        src[rng.integers(0, P, 5)] = -1
        return (_dev(src.astype(np.int64), cuda), _dev(dst.astype(np.int64), cuda),
                _dev(rng.random(P).astype(np.float32), cuda))

    def make():
        p = _leaf(h)
        opt = Adam([p], lr=1e-2)
        opt.fuse_row_grad(p)
        return p, opt

    def step(p, opt, src, dst, y):
        opt.zero_grad()
        plan = MF.pair_plan(src, dst, n)
        _, n_rows = MF.plan_rows(plan)
        MF.link_bce_loss(p, src, dst, y, plan=plan).backward()
        opt.step()
        return n_rows

    def state(p, opt):
        return (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"],
                opt.state[p]["step"])

    warm = batch()
    p, opt = make()
    q, oq = make()
    statics = [t.clone() for t in warm]
    step(p, opt, *statics)  # warm-up outside the capture
    step(q, oq, *warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        n_rows = step(p, opt, *statics)
    counts = []
    for k in range(2):
        new = batch(repeats=200 * k)
        for s, t in zip(statics, new):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        counts.append((int(n_rows), int(step(q, oq, *new))))
        for got, want in zip(state(p, opt), state(q, oq)):
            assert _same_bits(got, want)
        assert float(opt.state[p]["step"]) == 2.0 + k
    assert counts[0][0] == counts[0][1] and counts[1][0] == counts[1][1]
    assert counts[0][0] != counts[1][0]  # the row count is read on the device
    assert p.grad is None
