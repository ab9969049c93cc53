"""The row-sparse Adam that replays missed steps (``fuse_row_grad(replay=True)``,
msha_adam_rows_replay) against the dense optimizer's bits: the optimizer alone over a
constructive schedule (rows with lags 0, 1 and 10, rows never named), the chunked flush, the
five losses that read the table, SGAE.py's configuration, a hyperparameter change, a
checkpoint taken mid-run, and the capture of a whole step into one HIP graph.

Every comparison is bitwise: a row that misses k steps takes, in the dense optimizer, k
updates with gradient +0.0 (plus wd * p), and the replay applies exactly those, with the
same element update and each step's own bias corrections."""
import copy

import numpy as np
import pytest
import torch

import rowreplay_ref as R
from gpu_helpers import tol_close

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
N, STEPS, PAIRS = 193, 12, 48
SCHED = R.schedule(N, STEPS, PAIRS)
TOUCHED = R.schedule_facts(SCHED)  # the four facts, asserted on the lists themselves
LR = 1e-2  # a step moves a bf16 entry of size 0.3 by several ulps


def _dev(x, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device=dev)
    return t if dtype is None else t.to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _table0(F, dt, dev, seed=11):
    rng = np.random.default_rng(seed)
    return _dev(rng.standard_normal((N, F)).astype(np.float32) * 0.3, dev, DT[dt])


def _state(p, opt):
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def _assert_state_bits(got, want, rows=None):
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
        if rows is not None:
            a, b = a[rows], b[rows]
        assert _same_bits(a, b), name


# ------------------------------------------------- synthetic gradients and the twin ---

_GRADS, _TWINS = {}, {}


def _row_grads(dev, F):
    """One RowGrad per step of the schedule, independent of the table: the step's distinct
    rows, values from 1e-3 to 1 with an exact zero, in plan_rows' layout."""
    from msha_gnn_amd import functional as MF

    if F not in _GRADS:
        rng = np.random.default_rng(100 + F)
        out = []
        for src, dst in SCHED:
            rows = R.rows_of((src, dst))
            cap, cnt = min(N, 2 * PAIRS), len(rows)
            r = np.full(cap, -1, np.int32)
            r[:cnt] = rows
            vals = np.zeros((cap, F), np.float32)
            vals[:cnt] = (rng.standard_normal((cnt, F))
                          * 10.0 ** rng.uniform(-3, 0, (cnt, 1))).astype(np.float32)
            vals[0, 0] = 0.0
            out.append(MF.RowGrad(_dev(r, dev), torch.tensor(cnt, dtype=torch.int32, device=dev),
                                  _dev(vals, dev), (N, F)))
        _GRADS[F] = out
    return _GRADS[F]


def _twin(dev, F, dt, wd, halve_after=None):
    """The unregistered table stepped by the dense kernel on ``RowGrad.to_dense()`` in the
    table's dtype (exact zeros elsewhere); run once per configuration and left unchanged."""
    from msha_gnn_amd.optim import Adam

    key = (F, dt, wd, halve_after)
    if key not in _TWINS:
        b = _leaf(_table0(F, dt, dev))
        ob = Adam([b], lr=LR, weight_decay=wd)
        for s, rg in enumerate(_row_grads(dev, F)):
            if s == halve_after:
                ob.param_groups[0]["lr"] = LR / 2
            b.grad = rg.to_dense().to(DT[dt])
            ob.step()
        assert float(ob.state[b]["step"]) == STEPS
        _TWINS[key] = tuple(t.clone() for t in _state(b, ob))
    return _TWINS[key]


def _replay_run(dev, F, dt, wd, first=0, last=STEPS, table=None, opt=None, halve_after=None):
    """Steps ``first`` .. ``last - 1`` of the schedule on a replay-registered table, the
    gradients handed in through ``stash_row_grad``; no catch_up."""
    from msha_gnn_amd.optim import Adam

    if table is None:
        table = _leaf(_table0(F, dt, dev))
        opt = Adam([table], lr=LR, weight_decay=wd)
        opt.fuse_row_grad(table, replay=True)
    for s, rg in list(enumerate(_row_grads(dev, F)))[first:last]:
        if s == halve_after:
            opt.param_groups[0]["lr"] = LR / 2
        opt.stash_row_grad(table, rg)
        opt.step()
    assert table.grad is None and opt.row_grad_of(table) is None
    return table, opt


# ------------------------------------------------------------- 1. optimizer alone ---

@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("dt,F", [("fp32", 16), ("fp32", 32), ("fp32", 128), ("bf16", 16),
                                  ("bf16", 128)])
def test_replay_equals_the_dense_kernel_bitwise(cuda, msha, dt, F, wd):
    want = _twin(cuda, F, dt, wd)
    p0 = _table0(F, dt, cuda)
    a, oa = _replay_run(cuda, F, dt, wd)
    st = oa.state[a]
    assert float(st["step"]) == STEPS and st["row_step"].dtype == torch.int32
    last = _dev(np.sort(np.fromiter(TOUCHED[-1], np.int64)), cuda)
    # before the flush: the last step's rows are current, the never-named rows untouched
    assert int(oa.stale_rows(a)) == N - last.numel()
    assert (st["row_step"][last] == STEPS).all() and not st["row_step"][150:].any()
    _assert_state_bits(_state(a, oa), want, last)
    assert _same_bits(a.detach()[150:], p0[150:])
    assert not st["exp_avg"][150:].any() and not st["exp_avg_sq"][150:].any()
    assert not _same_bits(a.detach()[:150], want[0][:150])  # (rows are behind: work to do)
    # the dense optimizer moved the never-named rows exactly when it decays them
    assert _same_bits(want[0][150:], p0[150:]) == (wd == 0)
    oa.catch_up(a)
    _assert_state_bits(_state(a, oa), want)
    assert (st["row_step"] == STEPS).all() and int(oa.stale_rows(a)) == 0
    assert float(st["step"]) == STEPS  # a catch-up is not a step


# ------------------------------------------------------------------- 2. chunking ---

@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_flush_chunking_gives_the_same_bits(cuda, msha, dt):
    F, wd = 32 if dt == "fp32" else 16, 5e-4
    want = _twin(cuda, F, dt, wd)
    for chunk in (1, 5, 4096):
        a, oa = _replay_run(cuda, F, dt, wd)
        oa.catch_up(a, chunk=chunk)
        _assert_state_bits(_state(a, oa), want)
        assert (oa.state[a]["row_step"] == STEPS).all()
        oa.catch_up(a)  # twice changes nothing
        oa.catch_up(a, chunk=1)
        _assert_state_bits(_state(a, oa), want)
    # a partial flush: one launch of 5 steps leaves the never-named rows at step 5
    from msha_gnn_amd import _lib

    a, oa = _replay_run(cuda, F, dt, wd)
    st = oa.state[a]
    _lib.call("msha_adam_rows_replay", N, F, 0 if dt == "fp32" else 1, a.data_ptr(),
              st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
              st["row_step"].data_ptr(), None, None, N, None, 5, LR, 0.9, 0.999, 1e-8, wd,
              _lib.stream_handle(a.device))
    assert (st["row_step"][150:] == 5).all() and int(st["row_step"].max()) == STEPS
    assert int(st["row_step"][2]) == 9  # row 2: valid after step 4, five steps on
    oa.catch_up(a)
    _assert_state_bits(_state(a, oa), want)


# ------------------------------------------------------------ 3. through each loss ---

def _loss_case(name, dev):
    """(loss(table, extras, step), initial extra parameters) of one of the five losses on
    the schedule's lists, widths 16."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import graph_of

    rng = np.random.default_rng(21)
    F = 16
    lists = [(_dev(s, dev), _dev(d, dev)) for s, d in SCHED]
    y = _dev((rng.random((STEPS, PAIRS)) < 0.5).astype(np.float32), dev)
    W = _dev(rng.standard_normal((16, F)).astype(np.float32) * 0.5, dev)
    b = _dev(rng.standard_normal(16).astype(np.float32) * 0.1, dev)
    teacher = _dev(rng.standard_normal((N, F)).astype(np.float32), dev)
    tl = _dev((np.round(rng.standard_normal((PAIRS, 4)) * 6) / 4).astype(np.float32), dev)
    adj = _dev((rng.random((N, 16)) * (rng.random((N, 16)) < 0.4)).astype(np.float32), dev)
    target = _dev(rng.integers(0, 16, 2 * PAIRS).astype(np.int64), dev)

    def mlp(table, extras, s):
        src, dst = lists[s]
        return MF.link_mlp_loss(table, src, dst, extras[0], extras[1], label=(src + dst) % 16)

    def match(table, extras, s):
        return MF.link_match_loss(table, torch.cat(lists[s]), teacher)

    if name == "bce":
        return (lambda table, extras, s: MF.link_bce_loss(table, *lists[s], y[s])), []
    if name == "mlp":
        return mlp, [W, b]
    if name == "distill":
        def distill(table, extras, s):
            src, dst = lists[s]
            ctx = torch.stack([dst.roll(k) for k in range(4)], dim=1).contiguous()
            return MF.link_distill_loss(table, src, ctx, teacher_logits=tl, w_prob=0.5)
        return distill, []
    if name == "match":
        return match, []
    if name == "mlp+match":
        return (lambda table, extras, s: mlp(table, extras, s)
                + 0.1 * match(table, extras, s)), [W, b]
    assert name == "sage"
    g, transposed = graph_of(adj)
    assert not transposed
    vals = g.values(adj)

    def sage(table, extras, s):
        logp = MF.sage_forward(table, torch.cat(lists[s]), g, vals, *extras)
        return torch.nn.functional.nll_loss(logp, target)

    return sage, [W, b, _dev(rng.standard_normal((16, 16)).astype(np.float32) * 0.5, dev),
                  _dev(rng.standard_normal(16).astype(np.float32) * 0.1, dev)]


def _train(dev, loss_fn, extras0, register, steps, accumulate=False):
    from msha_gnn_amd.optim import Adam

    table = _leaf(_table0(16, "fp32", dev))
    extras = [_leaf(e) for e in extras0]
    opt = Adam([table] + extras, lr=LR, weight_decay=5e-4)
    if register:
        opt.fuse_row_grad(table, accumulate=accumulate, replay=True)
    losses = []
    for s in range(steps):
        opt.zero_grad()
        loss = loss_fn(table, extras, s)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return table, extras, opt, losses


@pytest.mark.parametrize("name", ["bce", "mlp", "distill", "match", "sage", "mlp+match"])
def test_losses_on_a_replay_table_follow_the_dense_run(cuda, msha, name):
    loss_fn, extras0 = _loss_case(name, cuda)
    steps = 4
    a, ea, oa, la = _train(cuda, loss_fn, extras0, True, steps, accumulate="+" in name)
    b, eb, ob, lb = _train(cuda, loss_fn, extras0, False, steps)
    assert a.grad is None and b.grad is not None
    for s, (x, y) in enumerate(zip(la, lb)):
        assert _same_bits(x, y), (name, s, float(x), float(y))
    assert int(oa.stale_rows(a)) >= N - 150  # rows 150.. were never read
    assert not _same_bits(a.detach(), b.detach())
    with torch.no_grad():  # a read without grad catches its rows up too
        stale = int(oa.stale_rows(a))
        x, y = loss_fn(a, ea, steps), loss_fn(b, eb, steps)
        assert _same_bits(x, y) and int(oa.stale_rows(a)) < stale
    oa.catch_up(a)
    _assert_state_bits(_state(a, oa), _state(b, ob))
    assert int(oa.stale_rows(a)) == 0
    for x, y in zip(ea, eb):
        assert _same_bits(x.detach(), y.detach())


# ------------------------------------------------------ 4. SGAE.py's configuration ---

def test_graphsage_with_weight_decay_follows_the_dense_run(cuda, msha):
    """layers.GraphSAGE(16, 16, 16) under Adam(lr 1e-3, weight_decay 5e-4), three batches,
    ``Sfeatures`` replay-registered against the unregistered run: bitwise; and the table
    within 1e-6 of torch.optim.Adam stepped on the unregistered run's dense gradients."""
    from msha_gnn_amd import layers
    from msha_gnn_amd.optim import Adam

    rng = np.random.default_rng(31)
    gdp = {i: float(v) for i, v in enumerate(rng.random(N).astype(np.float32))}
    adj = _dev((rng.random((N, 16)) * (rng.random((N, 16)) < 0.4)).astype(np.float32), cuda)
    batches = [_dev(np.concatenate(SCHED[s]), cuda) for s in range(3)]
    target = _dev(rng.integers(0, 16, 2 * PAIRS).astype(np.int64), cuda)

    def run(register, mirror=None):
        torch.manual_seed(5)
        model = layers.GraphSAGE(16, 16, 16, gdp).to(cuda)
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
        if register:
            opt.fuse_row_grad(model.Sfeatures, replay=True)
        losses = []
        for src in batches:
            opt.zero_grad()
            loss = torch.nn.functional.nll_loss(model(src, adj), target)
            loss.backward()
            if mirror is not None:
                mirror[0].grad = model.Sfeatures.grad.clone()
                mirror[1].step()
            opt.step()
            losses.append(loss.detach().clone())
        return model, opt, losses

    torch.manual_seed(5)
    t_ref = _leaf(layers.GraphSAGE(16, 16, 16, gdp).Sfeatures.detach().to(cuda))
    o_ref = torch.optim.Adam([t_ref], lr=1e-3, weight_decay=5e-4)
    ma, oa, la = run(True)
    mb, ob, lb = run(False, (t_ref, o_ref))
    assert ma.Sfeatures.grad is None and int(oa.stale_rows(ma.Sfeatures)) > 0
    for x, y in zip(la, lb):
        assert _same_bits(x, y)
    oa.catch_up(ma.Sfeatures)
    for (k, x), y in zip(ma.named_parameters(), mb.parameters()):
        assert _same_bits(x.detach(), y.detach()), k
    _assert_state_bits(_state(ma.Sfeatures, oa), _state(mb.Sfeatures, ob))
    tol_close(ma.Sfeatures.detach().cpu().numpy(), t_ref.detach().cpu().numpy(), 1e-6, 1e-6)


# ---------------------------------------------------- 5. a hyperparameter change ---

def test_lr_change_flushes_under_the_old_values(cuda, msha):
    F, dt, wd = 32, "fp32", 5e-4
    want = _twin(cuda, F, dt, wd, halve_after=6)
    assert not _same_bits(want[0], _twin(cuda, F, dt, wd)[0])
    a, oa = _replay_run(cuda, F, dt, wd, halve_after=6)
    assert oa.param_groups[0]["lr"] == LR / 2 and int(oa.stale_rows(a)) > 0
    oa.catch_up(a)
    _assert_state_bits(_state(a, oa), want)


# ------------------------------------------------------------------ 6. checkpoint ---

@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_checkpoint_without_a_flush_resumes_the_run(cuda, msha, dt):
    from msha_gnn_amd.optim import Adam

    F, wd = 16, 5e-4
    want = _twin(cuda, F, dt, wd)
    a, oa = _replay_run(cuda, F, dt, wd, last=6)
    assert int(oa.stale_rows(a)) > 0
    sd = copy.deepcopy(oa.state_dict())  # (a state_dict holds the optimizer's own tensors)
    assert sd["state"][0]["row_step"].dtype == torch.int32
    c = _leaf(a)
    oc = Adam([c], lr=LR, weight_decay=wd)
    oc.fuse_row_grad(c, replay=True)
    oc.load_state_dict(sd)
    assert oc.state[c]["row_step"].dtype == torch.int32
    assert torch.equal(oc.state[c]["row_step"], oa.state[a]["row_step"])
    _replay_run(cuda, F, dt, wd, first=6, table=c, opt=oc)
    _replay_run(cuda, F, dt, wd, first=6, table=a, opt=oa)
    _assert_state_bits(_state(c, oc), _state(a, oa))  # before the flush already
    assert torch.equal(oc.state[c]["row_step"], oa.state[a]["row_step"])
    oc.catch_up(c)
    _assert_state_bits(_state(c, oc), want)


# --------------------------------------------------------------------- 7. capture ---

def test_whole_replay_step_in_one_graph(cuda, msha):
    """Plan + link_bce_loss + backward + step() of a replay table in one HIP graph with
    static index buffers: the catch-up launch is inside (a readback would fail the capture),
    and five replays over the schedule's first five batches leave the eager run's bits."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    F, wd = 32, 5e-4
    rng = np.random.default_rng(41)
    ys = _dev((rng.random((STEPS, PAIRS)) < 0.5).astype(np.float32), cuda)
    lists = [(_dev(s, cuda), _dev(d, cuda), ys[i]) for i, (s, d) in enumerate(SCHED)]

    def make(register=True):
        p = _leaf(_table0(F, "fp32", cuda))
        opt = Adam([p], lr=LR, weight_decay=wd)
        if register:
            opt.fuse_row_grad(p, replay=True)
        return p, opt

    def step(p, opt, src, dst, y):
        opt.zero_grad()
        plan = MF.pair_plan(src, dst, N)
        loss = MF.link_bce_loss(p, src, dst, y, plan=plan)
        loss.backward()
        opt.step()
        return loss

    p, opt = make()
    q, oq = make()
    d, od = make(register=False)
    statics = [t.clone() for t in lists[11]]
    for t, o in ((p, opt), (q, oq), (d, od)):  # warm-up outside the capture
        step(t, o, *(statics if t is p else lists[11]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step(p, opt, *statics)
    for k in range(5):
        for s, t in zip(statics, lists[k]):
            s.copy_(t)
        graph.replay()
        want = step(q, oq, *lists[k])
        dense = step(d, od, *lists[k])
        torch.cuda.synchronize()
        assert _same_bits(loss, want) and _same_bits(loss, dense), k
        _assert_state_bits(_state(p, opt), _state(q, oq))
        assert torch.equal(opt.state[p]["row_step"], oq.state[q]["row_step"])
        assert float(opt.state[p]["step"]) == 2.0 + k
    assert p.grad is None and int(opt.stale_rows(p)) > 0
    opt.catch_up(p)
    _assert_state_bits(_state(p, opt), _state(d, od))
