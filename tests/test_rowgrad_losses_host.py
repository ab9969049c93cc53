"""Host-side checks of the row-sparse paths of link_mlp_loss, link_match_loss and
sage_forward and of the union of several row gradients: the header's declarations, the new
entry points' argument errors (no launch), the numpy restatement of the union
(``rowunion_ref``) on hand-made lists, and the optimizer's accumulate rules."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rowunion_ref as U
from conftest import ROOT

F32, BF16 = 0, 1  # MSHA_DTYPE_*

NEW_SYMBOLS = ("msha_link_mlp_bwd_rows", "msha_sage_rows_workspace_size", "msha_sage_bwd_rows",
               "msha_link_match_rows", "msha_link_match_bwd_rows",
               "msha_row_grad_union_workspace_size", "msha_row_grad_union")


def test_header_declares_every_new_symbol(msha):
    from msha_gnn_amd import _lib

    text = open(os.path.join(ROOT, "include", "msha_gnn.h"), encoding="utf-8").read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"MSHA_API\s+[\w\s\*]+\b" + name + r"\(", text), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert re.search(r"#define\s+MSHA_ABI_VERSION\s+16\b", text) and _lib.ABI_VERSION == 16
    assert lib.msha_abi_version() == 16
    fields = [f for f, _ in _lib.MshaRowList._fields_]
    assert fields == ["rows", "n_rows", "cap", "vals"] and _lib.MAX_ROW_LISTS == 4
    assert re.search(r"typedef struct msha_row_list \{\s*const int32_t\* rows;\s*"
                     r"const int32_t\* n_rows;\s*int64_t cap;\s*const float\* vals;", text)


def test_workspace_sizes(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    for n in (1, 1000, 100_000, 1 << 20):
        rows_ws = lib.msha_plan_rows_workspace_size(n)
        un = lib.msha_row_grad_union_workspace_size(n)
        assert un >= rows_ws + 4 * n and un < rows_ws + 4 * n + 4096  # n marks + the list's
        for B in (0, 1, 512):
            base = lib.msha_sage_workspace_size(B, n, 32, 16, 64)
            both = lib.msha_sage_rows_workspace_size(B, n, 32, 16, 64)
            assert base > 0 and rows_ws <= both - base < rows_ws + 256
    assert lib.msha_row_grad_union_workspace_size(0) == 0
    assert lib.msha_row_grad_union_workspace_size(2 ** 31) == 0
    assert lib.msha_sage_rows_workspace_size(4, 100, 24, 16, 16) == 0
    assert lib.msha_sage_rows_workspace_size(-1, 100, 16, 16, 16) == 0


def test_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20
    big = 1 << 30

    def mlp(P=100, feat=128, hidden=128, dt=F32, h=p, ld=128, n=1000, src=p, W32=p, out=p,
            dz=p, dx=p, rows=p, n_rows=p, cap=200, vals=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_mlp_bwd_rows", P, feat, hidden, dt, h, ld, n, src, p, None,
                         W32, None, out, p, 1.0, 0.0, 0.0, p, p, p, p, dz, dx, None, None, rows,
                         n_rows, cap, vals, ws, ws_bytes, None)

    for arg in ("h", "src", "out", "dz", "rows", "n_rows", "vals"):
        with pytest.raises(RuntimeError, match="null pointer"):
            mlp(**{arg: None})
    with pytest.raises(RuntimeError, match="vals needs W, dx and the plan"):
        mlp(dx=None)
    with pytest.raises(RuntimeError, match="cap must be min"):
        mlp(cap=1000)           # n, not min(n, 2P)
    with pytest.raises(RuntimeError, match="cap must be min"):
        mlp(n=150, cap=200)     # 2P, not min(n, 2P)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        mlp(n=150, cap=150, ws_bytes=8)  # the capacity itself is accepted
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        mlp(ws=None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        mlp(vals=p + 4)
    with pytest.raises(RuntimeError, match="link_mlp_bwd_rows"):
        mlp(feat=24)
    with pytest.raises(RuntimeError, match="link_mlp_bwd_rows"):
        mlp(P=big)

    def match_rows(P=100, n=1000, count=p, rows=p, n_rows=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_match_rows", P, n, count, rows, n_rows, ws, ws_bytes, None)

    for arg in ("count", "rows", "n_rows"):
        with pytest.raises(RuntimeError, match="null pointer"):
            match_rows(**{arg: None})
    with pytest.raises(RuntimeError, match="bad sizes"):
        match_rows(P=0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        match_rows(n=0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        match_rows(n=2 ** 31 - 1)
    for bad in (dict(ws_bytes=8), dict(ws=None), dict(ws=p + 8)):
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            match_rows(**bad)

    def match_bwd(P=100, feat=128, hd=F32, h=p, ld=128, n=1000, td=BF16, T=p, n_t=900, coef=p,
                  gloss=p, rows=p, n_rows=p, cap=100, vals=p):
        return _lib.call("msha_link_match_bwd_rows", P, feat, hd, h, ld, n, td, T, 128, n_t, coef,
                         gloss, rows, n_rows, cap, vals, None)

    for arg in ("h", "T", "coef", "gloss", "rows", "n_rows", "vals"):
        with pytest.raises(RuntimeError, match="null pointer"):
            match_bwd(**{arg: None})
    with pytest.raises(RuntimeError, match="cap must be min"):
        match_bwd(cap=1000)          # n, not min(n, P)
    with pytest.raises(RuntimeError, match="cap must be min"):
        match_bwd(n=50, cap=100)     # P, not min(n, P)
    with pytest.raises(RuntimeError, match="vals must be 16-byte aligned"):
        match_bwd(vals=p + 4)
    with pytest.raises(RuntimeError, match="coef must be 8-byte aligned"):
        match_bwd(coef=p + 4)
    with pytest.raises(RuntimeError, match="unsupported width"):
        match_bwd(feat=24)
    with pytest.raises(RuntimeError, match="bad sizes"):
        match_bwd(P=0)

    g = _lib.MshaGraph()
    g.n_rows, g.n_cols, g.n_edges, g.rowptr, g.col = 1000, 16, 5000, p, p

    def sage(graph=g, B=100, src=p, fin=32, out=64, table=p, ld=32, logp=p, dlogp=p, dW1=None,
             db1=None, rows=p, n_rows=p, cap=200, vals=p, ws=p, ws_bytes=1 << 30):
        gp = ctypes.byref(graph) if graph is not None else None
        return _lib.call("msha_sage_bwd_rows", gp, B, src, fin, out, table, ld, p, p, p, p, p,
                         logp, dlogp, dW1, db1, None, None, rows, n_rows, cap, vals, ws,
                         ws_bytes, None)

    for arg in ("src", "table", "logp", "dlogp", "rows", "n_rows", "vals"):
        with pytest.raises(RuntimeError, match="null pointer"):
            sage(**{arg: None})
    with pytest.raises(RuntimeError, match="graph CSR or edge values missing"):
        sage(graph=None)
    with pytest.raises(RuntimeError, match="cap must be min"):
        sage(cap=1000)           # n, not min(n, 2B)
    with pytest.raises(RuntimeError, match="cap must be min"):
        sage(B=600, cap=1200)    # 2B, not min(n, 2B)
    with pytest.raises(RuntimeError, match="msha_sage_rows_workspace_size"):
        sage(B=600, cap=1000, ws_bytes=8)  # the capacity itself is accepted
    small = _lib.load().msha_sage_workspace_size(100, 1000, 32, 16, 64)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        sage(ws_bytes=small)     # the dense backward's size is not enough
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        sage(ws=None)
    with pytest.raises(RuntimeError, match="vals must be 16-byte aligned"):
        sage(vals=p + 4)
    with pytest.raises(RuntimeError, match="unsupported widths"):
        sage(fin=24)
    with pytest.raises(RuntimeError, match="come together or not at all"):
        sage(dW1=p)

    def union(n=1000, feat=32, k=2, caps=(200, 300), cap=500, rows=p, n_rows=p, vals=p, ws=p,
              ws_bytes=1 << 30, lists="make", bad=None):
        arr = (_lib.MshaRowList * 4)()
        for d, c in zip(arr, caps):
            d.rows, d.n_rows, d.cap, d.vals = p, p, c, p
        if bad is not None:
            setattr(arr[1], bad[0], bad[1])
        return _lib.call("msha_row_grad_union", n, feat, k, ctypes.byref(arr) if lists else None,
                         rows, n_rows, cap, vals, ws, ws_bytes, None)

    for k in (0, -1, 5):
        with pytest.raises(RuntimeError, match=r"k must be in \[1, 4\]"):
            union(k=k)
    for arg in ("rows", "n_rows", "vals", "lists"):
        with pytest.raises(RuntimeError, match="null pointer"):
            union(**{arg: None})
    for field in ("rows", "n_rows", "vals"):
        with pytest.raises(RuntimeError, match="null pointer in a list"):
            union(bad=(field, None))
    with pytest.raises(RuntimeError, match="a list's cap must be in"):
        union(bad=("cap", 1001))
    with pytest.raises(RuntimeError, match="a list's cap must be in"):
        union(bad=("cap", 0))
    with pytest.raises(RuntimeError, match="cap must be min"):
        union(cap=1000)                       # n, not min(n, sum)
    with pytest.raises(RuntimeError, match="cap must be min"):
        union(caps=(700, 600), cap=1300)      # the sum, not min(n, sum)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        union(caps=(700, 600), cap=1000, ws_bytes=8)  # the capacity itself is accepted
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        union(k=4, caps=(1, 2, 3, 4), cap=10, ws=None)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        union(ws=p + 8)
    with pytest.raises(RuntimeError, match="vals must be 16-byte aligned"):
        union(vals=p + 4)
    with pytest.raises(RuntimeError, match="vals must be 16-byte aligned"):
        union(bad=("vals", p + 4))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        union(feat=6)
    with pytest.raises(RuntimeError, match="bad sizes"):
        union(n=0)


def _lst(rows, vals, cap=None):
    rows = np.asarray(rows, np.int32)
    cap = len(rows) if cap is None else cap
    r = np.full(cap, -1, np.int32)
    r[: len(rows)] = rows
    v = np.zeros((cap, 2), np.float32)
    v[: len(rows)] = vals
    return r, len(rows), v


def test_union_restatement_on_hand_made_lists():
    f = np.float32
    # disjoint
    rows, cnt, vals = U.union([_lst([1, 4], [[1, 2], [3, 4]]), _lst([0, 6], [[5, 6], [7, 8]])], 10)
    assert rows.tolist() == [0, 1, 4, 6] and cnt == 4 and rows.dtype == np.int32
    assert vals.tolist() == [[5, 6], [1, 2], [3, 4], [7, 8]] and vals.dtype == np.float32
    # nested, with capacity past the counts: -1 and zeros past the union's count
    rows, cnt, vals = U.union([_lst([2, 3, 5], [[1, 1], [2, 2], [3, 3]], cap=4),
                               _lst([3], [[10, 20]], cap=2)], 10)
    assert rows.tolist() == [2, 3, 5, -1, -1, -1] and cnt == 3
    assert vals.tolist() == [[1, 1], [12, 22], [3, 3], [0, 0], [0, 0], [0, 0]]
    # identical lists, three of them: left to right in fp32 -- (1 + 2^-24) + 2^-24 stays 1,
    # while 2^-24 + 2^-24 first would reach 1 + 2^-23
    e = f(2.0 ** -24)
    one = _lst([7], [[1, e]])
    rows, cnt, vals = U.union([one, _lst([7], [[e, e]]), _lst([7], [[e, 1]])], 10)
    assert rows.tolist() == [7, -1, -1] and cnt == 1
    assert vals[0, 0] == f(1.0) and vals[0, 1] == f(1.0) + f(2.0 ** -23)
    # an empty list beside a full one
    rows, cnt, vals = U.union([_lst([], np.zeros((0, 2)), cap=3), _lst([8], [[1, -1]])], 10)
    assert rows.tolist() == [8, -1, -1, -1] and cnt == 1 and vals[0].tolist() == [1, -1]
    # -0.0 in the second list only: +0.0 + -0.0 = +0.0 where the first list lacks the row or
    # holds +0.0, and -0.0 + -0.0 = -0.0
    rows, cnt, vals = U.union([_lst([1, 2], [[0.0, -0.0], [0.0, 5.0]]),
                               _lst([1, 3], [[-0.0, -0.0], [-0.0, 1.0]])], 10)
    assert rows.tolist() == [1, 2, 3, -1] and cnt == 3
    sign = np.signbit(vals)
    assert sign[0].tolist() == [False, True]    # +0 + -0, -0 + -0
    assert sign[2].tolist() == [False, False]   # the first list lacks row 3: +0 + -0
    assert vals[1].tolist() == [0.0, 5.0]
    # capacities whose sum passes n: cap = n
    rows, cnt, vals = U.union([_lst([0, 1, 2], np.ones((3, 2))), _lst([1, 2, 3], np.ones((3, 2)))],
                              4)
    assert rows.tolist() == [0, 1, 2, 3] and cnt == 4 and vals.shape == (4, 2)
    assert vals[:, 0].tolist() == [1, 2, 2, 1]
    # the row lists' restatement
    rows, cnt = U.listed([5, 2, 5, 9], 6)
    assert rows.tolist() == [2, 5, 9, -1, -1, -1] and cnt == 3


def _rg(MF, rows, n=8, F=4):
    rows = torch.tensor(rows, dtype=torch.int32)
    return MF.RowGrad(rows, torch.tensor(len(rows), dtype=torch.int32),
                      torch.ones(len(rows), F), (n, F))


def test_accumulate_rules(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import MAX_ROW_GRADS, Adam

    assert MAX_ROW_GRADS == 4
    one = torch.nn.Parameter(torch.zeros(8, 4))
    many = torch.nn.Parameter(torch.zeros(8, 4))
    opt = Adam([one, many], lr=1e-3)
    assert opt.fuse_row_grad(one) is one
    assert opt.fuse_row_grad(many, accumulate=True) is many
    # the default: one row gradient per step, today's message
    first = _rg(MF, [1, 2])
    opt.stash_row_grad(one, first)
    assert opt.row_grad_of(one) is first
    with pytest.raises(RuntimeError, match="second backward before step"):
        opt.stash_row_grad(one, _rg(MF, [3]))
    assert opt.row_grad_of(one) is first
    # accumulate: four in arrival order, a fifth raises
    assert opt.row_grad_of(many) is None
    got = [_rg(MF, [k]) for k in range(4)]
    for g in got:
        opt.stash_row_grad(many, g)
    assert many._msha_row_grads == got
    with pytest.raises(RuntimeError, match="at most 4 row gradients"):
        opt.stash_row_grad(many, _rg(MF, [5]))
    # zero_grad drops every pending gradient, and the table takes gradients again
    opt.zero_grad()
    assert opt.row_grad_of(one) is None and opt.row_grad_of(many) is None
    with pytest.raises(ValueError, match="not of this table's shape"):
        opt.stash_row_grad(many, _rg(MF, [5], n=9))
    assert opt.row_grad_of(many) is None
    single = _rg(MF, [6])
    opt.stash_row_grad(many, single)
    assert opt.row_grad_of(many) is single  # one pending: itself, nothing merged
    opt.zero_grad()
    # registering again without the keyword restores the default rule
    opt.fuse_row_grad(many)
    opt.stash_row_grad(many, _rg(MF, [1]))
    with pytest.raises(RuntimeError, match="second backward before step"):
        opt.stash_row_grad(many, _rg(MF, [2]))
    # the union takes 2 to 4 gradients of one table
    with pytest.raises(ValueError, match="2 to 4 row gradients"):
        MF.row_grad_union([first])
    with pytest.raises(ValueError, match="2 to 4 row gradients"):
        MF.row_grad_union([first] * 5)
    with pytest.raises(ValueError, match="not of one table"):
        MF.row_grad_union([first, _rg(MF, [1], n=9)])
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.row_grad_union([first, first])
    # weight decay still raises
    decayed = Adam([torch.nn.Parameter(torch.zeros(8, 4))], lr=1e-3, weight_decay=1e-2)
    with pytest.raises(ValueError, match="weight_decay == 0"):
        decayed.fuse_row_grad(decayed.param_groups[0]["params"][0], accumulate=True)
