"""Host-side checks of the row-sparse Adam that replays missed steps: the float32 restatement
(``rowreplay_ref``: the lazy scheme against the dense step, exactly), the registration's
``replay`` keyword and its ``row_step`` state, the new entry point's declaration and its
argument errors (no launch)."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import rowreplay_ref as R
from conftest import ROOT

F32, BF16 = 0, 1  # MSHA_DTYPE_*


def test_schedule_facts():
    sched = R.schedule()
    assert len(sched) == 12 and all(s.shape == d.shape == (48,) for s, d in sched)
    touched = R.schedule_facts(sched)
    assert set().union(*touched) == set(range(150))  # every other row is in some step


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_lazy_scheme_equals_dense_exactly(wd):
    """The schedule's 12 steps: the rows of ``src`` are read (caught up) before the step,
    the rows of ``dst`` meet their gap inside the step; lr is small enough that decay,
    momentum and gradient all matter.  After a chunked flush the lazy table is the dense one,
    bit for bit, and before it the rows of the last step already are."""
    sched = R.schedule()
    n, F = 193, 8
    hp = (1e-2, 0.9, 0.999, 1e-8, wd)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal((n, F)).astype(np.float32)
    dp, dm, dv, t = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), 0
    lazy = R.LazyTable(p0)
    for src, dst in sched:
        rows = R.rows_of((src, dst))
        g = rng.standard_normal((len(rows), F)).astype(np.float32)
        g[0, 0] = 0.0
        dense_g = np.zeros((n, F), np.float32)
        dense_g[rows] = g
        t = R.dense_step(dp, dm, dv, t, dense_g, hp)
        lazy.catch_up(np.unique(src), hp)
        lazy.step_rows(rows, g, hp)
    assert t == lazy.step == 12
    assert lazy.stale_rows() == n - len(rows)
    np.testing.assert_array_equal(lazy.p[rows], dp[rows])  # the last step's rows: current
    np.testing.assert_array_equal(lazy.p[150:], p0[150:])  # never named: not yet moved
    assert (not np.array_equal(dp[150:], p0[150:])) == (wd != 0)
    assert not np.array_equal(lazy.p[:150], dp[:150])      # (the flush has work to do)
    assert lazy.flush(hp, 5) == 3
    assert lazy.stale_rows() == 0 and (lazy.row_step == 12).all()
    for a, b in ((lazy.p, dp), (lazy.m, dm), (lazy.v, dv)):
        assert a.tobytes() == b.tobytes()
    before = lazy.replayed
    lazy.flush(hp, 4096)  # twice changes nothing
    assert lazy.replayed == before and lazy.p.tobytes() == dp.tobytes()


def test_chunk_size_does_not_matter():
    sched = R.schedule()
    hp = (1e-2, 0.9, 0.999, 1e-8, 5e-4)
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal((193, 4)).astype(np.float32)
    tabs = [R.LazyTable(p0) for _ in range(3)]
    for src, dst in sched:
        rows = R.rows_of((src, dst))
        g = rng.standard_normal((len(rows), 4)).astype(np.float32)
        for tab in tabs:
            tab.step_rows(rows, g, hp)
    assert [tab.flush(hp, c) for tab, c in zip(tabs, (1, 5, 4096))] == [12, 3, 1]
    assert tabs[0].p.tobytes() == tabs[1].p.tobytes() == tabs[2].p.tobytes()
    assert tabs[0].v.tobytes() == tabs[1].v.tobytes() == tabs[2].v.tobytes()


def test_header_declares_the_new_symbol(msha):
    from msha_gnn_amd import _lib

    text = open(os.path.join(ROOT, "include", "msha_gnn.h"), encoding="utf-8").read()
    lib = _lib.load()
    name = "msha_adam_rows_replay"
    assert re.search(r"MSHA_API\s+[\w\s\*]+\b" + name + r"\(", text)
    assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert re.search(r"#define\s+MSHA_ABI_VERSION\s+16\b", text) and _lib.ABI_VERSION == 16
    assert lib.msha_abi_version() == 16


def test_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers are aligned
    dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20

    def replay(n=1000, feat=128, dt=F32, param=p, m=p, v=p, step=p, row_step=p, rows=p,
               n_rows=p, cap=200, vals=p, max_steps=1, b1=0.9, wd=5e-4):
        return _lib.call("msha_adam_rows_replay", n, feat, dt, param, m, v, step, row_step,
                         rows, n_rows, cap, vals, max_steps, 1e-3, b1, 0.999, 1e-8, wd, None)

    for arg in ("param", "m", "v", "step", "row_step", "n_rows"):
        with pytest.raises(RuntimeError, match="null pointer"):
            replay(**{arg: None})
    with pytest.raises(RuntimeError, match="unsupported width"):
        replay(feat=24)
    with pytest.raises(RuntimeError, match="unsupported width"):
        replay(feat=4, dt=BF16)
    with pytest.raises(RuntimeError, match="unsupported width"):
        replay(dt=7)
    with pytest.raises(RuntimeError, match="cap must be in"):
        replay(cap=1001)
    with pytest.raises(RuntimeError, match="cap must be in"):
        replay(cap=0)
    with pytest.raises(RuntimeError, match="max_steps must be at least 1"):
        replay(max_steps=0)
    with pytest.raises(RuntimeError, match="bad hyperparameters"):
        replay(wd=-1e-4)
    with pytest.raises(RuntimeError, match="bad hyperparameters"):
        replay(b1=1.0)
    with pytest.raises(RuntimeError, match="cap must be n"):
        replay(rows=None, n_rows=None, cap=200)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        replay(vals=p + 8)
    with pytest.raises(RuntimeError, match="bad sizes"):
        replay(n=0)


def test_replay_registration_and_row_step_state(msha):
    from msha_gnn_amd.optim import FLUSH_CHUNK, Adam, row_optimizer_of

    table = torch.nn.Parameter(torch.zeros(8, 16))
    vec = torch.nn.Parameter(torch.zeros(16))
    opt = Adam([table, vec], lr=1e-3, weight_decay=5e-4)
    with pytest.raises(ValueError, match="weight_decay == 0"):
        opt.fuse_row_grad(table)  # the default registration: as before
    assert row_optimizer_of(table) is None
    assert opt.fuse_row_grad(table, replay=True) is table and row_optimizer_of(table) is opt
    rs = opt.state[table]["row_step"]
    assert rs.dtype == torch.int32 and rs.shape == (8,) and not rs.any()
    assert int(opt.stale_rows(table)) == 0
    assert FLUSH_CHUNK >= 1
    # a round trip keeps it int32 (torch's loader would cast it to the table's dtype)
    rs.copy_(torch.arange(8, dtype=torch.int32) * 300)
    for dtype in (torch.float32, torch.bfloat16):
        t2 = torch.nn.Parameter(torch.zeros(8, 16, dtype=dtype))
        opt2 = Adam([t2, torch.nn.Parameter(torch.zeros(16))], lr=1e-3, weight_decay=5e-4)
        opt2.fuse_row_grad(t2, replay=True)
        opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
        got = opt2.state[t2]["row_step"]
        assert got.dtype == torch.int32 and got.tolist() == rs.tolist()
        assert got.data_ptr() != rs.data_ptr()
        assert opt2.state_dict()["state"][0]["row_step"].dtype == torch.int32
    # a state without row_step: every row is current, the loaded step
    sd = copy.deepcopy(opt.state_dict())
    del sd["state"][0]["row_step"]
    sd["state"][0]["step"] = torch.tensor(7.0)
    t3 = torch.nn.Parameter(torch.zeros(8, 16))
    opt3 = Adam([t3, torch.nn.Parameter(torch.zeros(16))], lr=1e-3, weight_decay=5e-4)
    opt3.fuse_row_grad(t3, replay=True)
    opt3.load_state_dict(sd)
    assert int(opt3.stale_rows(t3)) == 0
    assert opt3.state[t3]["row_step"].tolist() == [7] * 8
    # the default registration is untouched by the keyword
    plain = torch.nn.Parameter(torch.zeros(8, 16))
    opt4 = Adam([plain], lr=1e-3)
    opt4.fuse_row_grad(plain)
    assert "row_step" not in opt4.state[plain]
    with pytest.raises(ValueError, match="replay=True"):
        opt4.catch_up(plain)
    with pytest.raises(ValueError, match="replay=True"):
        opt4.stale_rows(plain)


def test_catch_up_is_gpu_only(msha):
    from msha_gnn_amd.optim import Adam

    table = torch.nn.Parameter(torch.zeros(8, 16))
    opt = Adam([table], lr=1e-3, weight_decay=5e-4)
    opt.fuse_row_grad(table, replay=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.catch_up(table)
    rows = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.catch_up(table, (rows, torch.tensor(4, dtype=torch.int32)))
