"""Host-side checks of the row-sparse table training: the fp64 restatement of the lazy Adam
(``rowadam_ref``) against ``torch.optim.SparseAdam`` on the CPU, the header's declarations,
the new entry points' argument errors (no launch) and the registration's argument checks."""
import os
import re

import numpy as np
import pytest
import torch

import rowadam_ref as R
from conftest import ROOT

F32, BF16 = 0, 1  # MSHA_DTYPE_*

NEW_SYMBOLS = ("msha_plan_rows_workspace_size", "msha_plan_rows", "msha_link_bce_bwd_rows",
               "msha_pair_grad_bwd_rows", "msha_adam_rows_step")


def test_touched_rows_restatement():
    rowptr = np.array([0, 0, 2, 2, 2, 5, 6, 6])
    rows, cnt = R.touched_rows(rowptr)
    assert rows.tolist() == [1, 4, 5] and cnt == 3 and rows.dtype == np.int32
    rows, cnt = R.touched_rows(rowptr, cap=6)
    assert rows.tolist() == [1, 4, 5, -1, -1, -1] and cnt == 3
    assert R.touched_rows(np.zeros(4, np.int64), cap=2)[0].tolist() == [-1, -1]


def test_restatement_is_sparse_adam_with_rescaled_eps():
    """8 steps, a different row subset each, gradients from 1e-6 to 10 with an exact zero
    element: torch.optim.SparseAdam with eps * sqrt(1 - beta2^t) at step t, in fp64."""
    rng = np.random.default_rng(0)
    n, F, lr, betas, eps = 37, 8, 1e-2, (0.9, 0.999), 1e-8
    p0 = rng.standard_normal((n, F))
    p, m, v, t = p0.copy(), np.zeros((n, F)), np.zeros((n, F)), 0
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.SparseAdam([tp], lr=lr, betas=betas, eps=eps)
    for step in range(1, 9):
        rows = np.sort(rng.choice(n, size=rng.integers(1, n), replace=False))
        g = rng.standard_normal((len(rows), F)) * 10.0 ** rng.uniform(-6, 1, (len(rows), 1))
        g[0, 0] = 0.0
        t = R.lazy_adam_step(p, m, v, t, rows, g, lr, betas, eps)
        assert t == step
        opt.param_groups[0]["eps"] = R.sparse_adam_eps(eps, betas[1], step)
        tp.grad = torch.sparse_coo_tensor(torch.tensor(rows[None, :]), torch.tensor(g),
                                          (n, F)).coalesce()
        opt.step()
    st = opt.state[tp]
    np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert float(st["step"]) == 8 and not np.array_equal(p, p0)


def test_header_declares_every_new_symbol(msha):
    from msha_gnn_amd import _lib

    text = open(os.path.join(ROOT, "include", "msha_gnn.h"), encoding="utf-8").read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"MSHA_API\s+[\w\s\*]+\b" + name + r"\(", text), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert re.search(r"#define\s+MSHA_ABI_VERSION\s+16\b", text) and _lib.ABI_VERSION == 16
    assert lib.msha_abi_version() == 16


def test_plan_rows_workspace_size(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    sizes = [lib.msha_plan_rows_workspace_size(n) for n in (1, 1000, 100_000, 2_000_000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] >= 2_000_000 * 4       # an offset per row
    assert sizes[-1] < 2 * 2_000_000 * 4    # and nothing (n, F)-sized
    assert lib.msha_plan_rows_workspace_size(0) == 0
    assert lib.msha_plan_rows_workspace_size(2 ** 31) == 0


def test_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20
    big = 1 << 30

    def plan_rows(n=1000, P=100, rowptr=p, rows=p, n_rows=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_plan_rows", n, P, rowptr, rows, n_rows, ws, ws_bytes, None)

    with pytest.raises(RuntimeError, match="null pointer"):
        plan_rows(rowptr=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        plan_rows(rows=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        plan_rows(n_rows=None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        plan_rows(n=0)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        plan_rows(P=big)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        plan_rows(ws_bytes=8)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        plan_rows(ws=None)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        plan_rows(ws=p + 8)

    def bce(P=100, feat=128, dt=F32, h=p, ld=128, n=1000, src=p, rows=p, n_rows=p, cap=200,
            vals=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_bce_bwd_rows", P, feat, dt, h, ld, n, src, p, p, None, p, p,
                         p, p, p, rows, n_rows, cap, vals, ws, ws_bytes, None)

    def pgb(P=100, feat=128, dt=F32, h=p, ld=128, n=1000, src=p, rows=p, n_rows=p, cap=200,
            vals=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_pair_grad_bwd_rows", P, feat, dt, h, ld, n, src, p, p, p, p, p, p,
                         rows, n_rows, cap, vals, ws, ws_bytes, None)

    for call in (bce, pgb):
        for arg in ("h", "src", "rows", "n_rows", "vals"):
            with pytest.raises(RuntimeError, match="null pointer"):
                call(**{arg: None})
        with pytest.raises(RuntimeError, match="cap must be min"):
            call(cap=1000)           # n, not min(n, 2P)
        with pytest.raises(RuntimeError, match="cap must be min"):
            call(n=150, cap=200)     # 2P, not min(n, 2P)
        call_ok_cap = dict(n=150, cap=150, ws_bytes=8)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(**call_ok_cap)      # the capacity itself is accepted
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=24)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(dt=7)
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            call(P=big)
        with pytest.raises(RuntimeError, match="vals must be 16-byte aligned"):
            call(vals=p + 4)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws=None)

    def adam(n=1000, feat=128, dt=F32, param=p, m=p, v=p, step=p, rows=p, n_rows=p, cap=200,
             vals=p, b1=0.9):
        return _lib.call("msha_adam_rows_step", n, feat, dt, param, m, v, step, rows, n_rows, cap,
                         vals, 1e-3, b1, 0.999, 1e-8, None)

    for arg in ("param", "m", "v", "step", "rows", "n_rows", "vals"):
        with pytest.raises(RuntimeError, match="null pointer"):
            adam(**{arg: None})
    with pytest.raises(RuntimeError, match="unsupported width"):
        adam(feat=24)
    with pytest.raises(RuntimeError, match="unsupported width"):
        adam(feat=4, dt=BF16)
    with pytest.raises(RuntimeError, match="unsupported width"):
        adam(dt=7)
    with pytest.raises(RuntimeError, match="cap must be in"):
        adam(cap=1001)
    with pytest.raises(RuntimeError, match="cap must be in"):
        adam(cap=0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        adam(param=p + 8)
    with pytest.raises(RuntimeError, match="bad hyperparameters"):
        adam(b1=1.0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        adam(n=0)


def test_fuse_row_grad_argument_checks(msha):
    from msha_gnn_amd.optim import Adam, row_optimizer_of

    table = torch.nn.Parameter(torch.zeros(8, 16))
    vec = torch.nn.Parameter(torch.zeros(16))
    other = torch.nn.Parameter(torch.zeros(8, 16))
    decayed = Adam([table, vec], lr=1e-3, weight_decay=5e-4)
    with pytest.raises(ValueError, match="weight_decay == 0"):
        decayed.fuse_row_grad(table)
    assert row_optimizer_of(table) is None
    opt = Adam([table, vec], lr=1e-3)
    with pytest.raises(ValueError, match="2-D leaf table"):
        opt.fuse_row_grad(vec)
    with pytest.raises(ValueError, match="not in this optimizer"):
        opt.fuse_row_grad(other)
    assert opt.fuse_row_grad(table) is table and row_optimizer_of(table) is opt
    assert opt.row_grad_of(table) is None and table.grad is None
    # the rule is checked again at step(): a group whose decay was set after registration
    opt.param_groups[0]["weight_decay"] = 5e-4
    with pytest.raises(ValueError, match="weight_decay == 0"):
        opt.step()
    # a mixed optimizer: the table's group without decay, the rest with
    opt2 = Adam([{"params": [other], "weight_decay": 0.0}, {"params": [vec]}], lr=1e-3,
                weight_decay=5e-4)
    assert opt2.fuse_row_grad(other) is other


def test_plan_rows_and_row_grad_python_checks(msha):
    from msha_gnn_amd import functional as MF

    with pytest.raises(ValueError, match="must be a PairPlan"):
        MF.plan_rows((1, 2, 3))
    with pytest.raises(ValueError, match="must be a PairPlan"):
        MF.plan_rows(MF.PairPlan(5, 3, None, None, None))
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.plan_rows(MF.PairPlan(3, 2, torch.zeros(4, dtype=torch.int32), None, None))
    # RowGrad.to_dense is a scatter into zeros (CPU tensors work: plain torch)
    rows = torch.tensor([1, 3, -1, -1], dtype=torch.int32)
    vals = torch.tensor([[1.0, 2.0], [3.0, 4.0], [0.0, 0.0], [0.0, 0.0]])
    rg = MF.RowGrad(rows, torch.tensor(2, dtype=torch.int32), vals, (5, 2))
    assert rg.to_dense().tolist() == [[0, 0], [1, 2], [0, 0], [3, 4], [0, 0]]
    assert rg.shape == (5, 2)
