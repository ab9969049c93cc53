"""The dense side of the GAT step at the sizes where its kernels change form.

The fp32 projection takes the split-bf16 kernel (three bf16 W images in LDS, filled
column-wise with 16-byte stores) from ``SPLIT_MIN_ROWS`` rows: the existing projection tests
stop far below it, so the smallest sizes that reach it are checked here against torch fp64
at the same 1e-5 bar, with the row-order ``er`` contract of the row-score kernels.  The
bf16 projection's image fill is checked at a ragged size, and the row-statistics pass of
the fused backward (row terms forced) at row counts that are no multiple of its 8-row trip.
"""
import os

import numpy as np
import pytest
import torch

from gpu_helpers import t, tol_close
from oracle import gnn_oracle as O
from test_gpu_bf16 import BF, rb
from test_gpu_kernels import EMB_RTOL, _edge_case, _u_only_grads

pytestmark = pytest.mark.gpu

SPLIT_MIN_ROWS = 65536  # skinny_project's fp32 cut-over (MSHA_PROJ_SPLIT_MIN_ROWS unset)


def _short_row_graph(rng, n, dev):
    """n rows of 1 to 3 distinct, sorted columns out of n."""
    from msha_gnn_amd.graph import Graph

    deg = rng.integers(1, 4, n)
    first = rng.integers(0, n - 3, n)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = (np.repeat(first, deg) + np.arange(rowptr[-1]) - np.repeat(rowptr[:-1], deg))
    return Graph.from_csr(rowptr, col.astype(np.int64), n, dev)


@pytest.mark.parametrize("extra", [0, 13], ids=["cut", "cut+13"])
@pytest.mark.parametrize("K,H,F", [(128, 8, 16), (128, 2, 64), (64, 2, 64)])
def test_split_projection_at_the_cutover(cuda, msha, K, H, F, extra):
    """h, el, er of the split-bf16 projection at its smallest sizes (whole tiles only, and
    a ragged last tile with a partial tail round) vs torch fp64; er is tagged row-order,
    and the backward that reads it gives the bits of the one that recomputes it."""
    from msha_gnn_amd import functional as MF

    M = SPLIT_MIN_ROWS + extra
    g = torch.Generator().manual_seed(K + H + extra)
    X = torch.randn(M, K, generator=g)
    W = torch.randn(K, H * F, generator=g) * K ** -0.5
    al = torch.randn(H, F, generator=g)
    ar = torch.randn(H, F, generator=g)
    with torch.no_grad():
        h, el, er = MF.project_scores(X.to(cuda), W.to(cuda), al.to(cuda), ar.to(cuda), heads=H)
    rh = X.double() @ W.double()
    rel = (rh.view(M, H, F) * al.double()).sum(-1)
    rer = (rh.view(M, H, F) * ar.double()).sum(-1)
    for name, got, want in (("h", h, rh), ("el", el, rel), ("er", er, rer)):
        got, want = got.cpu().numpy(), want.numpy()
        err = np.abs(got - want) - 1e-5 * np.abs(want)
        print(f"{name}: max (err - 1e-5 |ref|) / max|ref| {err.max() / np.abs(want).max():.3g}")
        tol_close(got, want, 1e-5, 1e-5)
    assert getattr(er, "_msha_row_order", False)
    graph = _short_row_graph(np.random.default_rng(M + K), M, cuda)
    dU = torch.randn(M, H, F, generator=g).to(cuda)
    arc = ar.to(cuda)
    os.environ["MSHA_ROW_SCORES"] = "1"
    try:
        runs = []
        for er_in in (er, er.clone()):  # the clone carries no tag: recompute from a_r
            leaves = [el.clone().requires_grad_(True), er_in.requires_grad_(True),
                      h.view(M, H, F).clone().requires_grad_(True)]
            u = MF.edge_attention(graph, *leaves, ar=arc)
            u.backward(dU)
            runs.append([u.detach()] + [x.grad for x in leaves])
            er.requires_grad_(False)
    finally:
        os.environ.pop("MSHA_ROW_SCORES", None)
    for a, b, name in zip(*runs, ("u", "d_el", "d_er", "d_hc")):
        assert torch.equal(a, b), name


def test_bf16_projection_ragged(cuda, msha):
    """The bf16 projection's [n][k] image (column-wise fill) at 4,099 rows, K = 128: the
    bars of test_project_scores_bf16."""
    from msha_gnn_amd import functional as MF

    M, K, H, F = 4099, 128, 8, 16
    rng = np.random.default_rng(M)
    X = rb(rng.standard_normal((M, K)))
    W = rb(rng.standard_normal((K, H * F)) / np.sqrt(K))
    al = rng.standard_normal((H, F)).astype(np.float32)
    ar = rng.standard_normal((H, F)).astype(np.float32)
    with torch.no_grad():
        h, el, er = MF.project_scores(t(X, cuda, BF), t(W, cuda, BF), t(al, cuda), t(ar, cuda),
                                      heads=H)
    assert h.dtype == BF and el.dtype == torch.float32
    rh = X.astype(np.float64) @ W.astype(np.float64)
    tol_close(h.float().cpu().numpy(), rh, 1e-2, 1e-2)
    hs_ = h.float().cpu().numpy().astype(np.float64).reshape(M, H, F)
    tol_close(el.cpu().numpy(), (hs_ * al).sum(-1), 1e-5, 1e-6)
    tol_close(er.cpu().numpy(), (hs_ * ar).sum(-1), 1e-5, 1e-6)
    tol_close(el.cpu().numpy(), (rh.reshape(M, H, F) * al).sum(-1), 1e-2, 1e-2)
    tol_close(er.cpu().numpy(), (rh.reshape(M, H, F) * ar).sum(-1), 1e-2, 1e-2)


@pytest.mark.parametrize("n", [13, 1031])
def test_row_stats_ragged_trip(cuda, msha, n):
    """The fused backward with the row terms forced (bwd_row_stats_kernel writes the row
    records and d_el): row counts that are no multiple of the 8-row trip, 8 x 16, one
    virtual row.  d_el and d_hc against the oracle; everything but d_el the bits of the
    backward without row terms, d_el within 1e-5 of its de row sum."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import Graph

    m, H, F = 40, 8, 16
    rng = np.random.default_rng(n)
    c, rowptr, col, empty, el, er, hc, hs, dU, dV = _edge_case(rng, n, m, H, F, 9,
                                                               empty_rows=(n - 2,))
    graph = Graph.from_dense(t(c, cuda))
    base = _u_only_grads(MF, graph, el, er, hc, dU, 0.0, 3, cuda, torch.float32, True,
                         rowterms=False)
    rt = _u_only_grads(MF, graph, el, er, hc, dU, 0.0, 3, cuda, torch.float32, True,
                       rowterms=True)
    ref = O.edge_aggregate_fwd(rowptr, col, el, er, hc, rowflag=empty)
    bw = O.edge_aggregate_bwd(rowptr, col, ref, hc, dU)
    tol_close(rt[1].cpu().numpy(), bw["d_el"], 1e-4, 1e-5)
    tol_close(rt[3].cpu().numpy(), bw["d_hc"], EMB_RTOL, 1e-5)
    for a, b, name in zip(rt, base, ("u", "d_el", "d_er", "d_hc")):
        if name != "d_el":
            assert torch.equal(a, b), name
    tol_close(rt[1].cpu().numpy(), base[1].cpu().numpy(), 1e-5, 1e-5)
