"""Device negative sampler (``functional.sample_negatives``, msha_negative_sample): every
draw is a non-edge, exactly uniform over the row's non-edges, reproducible from (seed,
replay counter)."""
import numpy as np
import pytest
import torch

from gpu_helpers import random_counts

pytestmark = pytest.mark.gpu

N, M = 64, 32
VIRTUAL, FULL, ONE, SEVEN = 3, 5, 9, 11
ONE_COL = 13
SEED = 20240611


@pytest.fixture(scope="module")
def graph(cuda, msha):
    from msha_gnn_amd.graph import Graph

    rng = np.random.default_rng(17)
    counts = random_counts(rng, N, M, 12, empty_rows=(VIRTUAL,), full_rows=(FULL,))
    counts[ONE] = 1
    counts[ONE, ONE_COL] = 0  # exactly one non-edge
    counts[SEVEN] = 0
    counts[SEVEN, rng.choice(M, 7, replace=False)] = 2  # degree 7
    g = Graph.from_dense(torch.as_tensor(counts, device=cuda))
    edges = counts > 0
    non_edges = [set(np.nonzero(~edges[i])[0].tolist()) for i in range(N)]
    non_edges[VIRTUAL] = set(range(M))  # a virtual full row counts as having no edges
    assert bool(g.rowflag[VIRTUAL]) and not bool(g.rowflag[FULL])
    assert len(non_edges[SEVEN]) == 25 and non_edges[ONE] == {ONE_COL} and not non_edges[FULL]
    return g, non_edges


def test_draws_are_non_edges_and_cover_them(cuda, graph):
    from msha_gnn_amd import functional as MF

    g, non_edges = graph
    k = 4096
    src = torch.arange(N, device=cuda)
    s, d = MF.sample_negatives(g, src, k=k, seed=SEED)
    assert s.dtype == d.dtype == torch.int64 and s.shape == d.shape == (N * k,)
    assert torch.equal(s, src.repeat_interleave(k))
    d = d.cpu().numpy().reshape(N, k)
    for i in range(N):
        drawn = set(d[i].tolist())
        if i == FULL:
            assert drawn == {-1}
            continue
        assert min(drawn) >= 0 and max(drawn) < M, i
        assert drawn == non_edges[i], i  # only non-edges, and all of them in 4,096 draws
    assert set(d[ONE].tolist()) == {ONE_COL}
    assert set(d[VIRTUAL].tolist()) == set(range(M))


def test_uniform_over_the_non_edges(cuda, graph):
    """Pearson's chi-square of 25 x 4,096 draws on the degree-7 row against uniform, 24
    degrees of freedom: an exactly uniform sampler exceeds 80 with probability ~1e-7."""
    from msha_gnn_amd import functional as MF

    g, non_edges = graph
    draws = 25 * 4096
    _, d = MF.sample_negatives(g, torch.tensor([SEVEN], device=cuda), k=draws, seed=SEED)
    cnt = np.bincount(d.cpu().numpy(), minlength=M)
    cols = sorted(non_edges[SEVEN])
    assert cnt.sum() == draws and cnt[cols].sum() == draws
    chi2 = float((((cnt[cols] - 4096.0) ** 2) / 4096.0).sum())
    print(f"chi-square {chi2:.2f} at 24 degrees of freedom")
    assert chi2 < 80.0


def test_reproducible_from_seed_and_replay_counter(cuda, graph):
    from msha_gnn_amd import functional as MF

    g, _ = graph
    src = torch.arange(N, device=cuda).repeat(8)
    a = MF.sample_negatives(g, src, k=3, seed=SEED)[1]
    assert torch.equal(a, MF.sample_negatives(g, src, k=3, seed=SEED)[1])
    assert not torch.equal(a, MF.sample_negatives(g, src, k=3, seed=SEED + 1)[1])
    assert not torch.equal(a, MF.sample_negatives(g, src, k=3, seed=SEED, offset=1)[1])
    counter = torch.zeros(1, dtype=torch.int64, device=cuda)
    prev = MF.set_rng_counter(counter)
    try:
        c0 = MF.sample_negatives(g, src, k=3, seed=SEED)[1]
        assert torch.equal(c0, a)  # counter 0: the plain offset
        assert torch.equal(c0, MF.sample_negatives(g, src, k=3, seed=SEED)[1])
        counter.add_(1)
        c1 = MF.sample_negatives(g, src, k=3, seed=SEED)[1]
        assert not torch.equal(c0, c1)
        assert torch.equal(c1, MF.sample_negatives(g, src, k=3, seed=SEED)[1])
    finally:
        MF.set_rng_counter(prev)


def test_col_offset_and_rows_outside_the_csr(cuda, graph):
    from msha_gnn_amd import functional as MF

    g, non_edges = graph
    src = torch.tensor([0, -1, N, 10 ** 12, FULL, SEVEN, N - 1], device=cuda)
    s0, d0 = MF.sample_negatives(g, src, k=5, seed=SEED)
    s1, d1 = MF.sample_negatives(g, src, k=5, seed=SEED, col_offset=1000)
    assert torch.equal(s0, src.repeat_interleave(5)) and torch.equal(s0, s1)
    d0, d1 = d0.cpu().numpy().reshape(-1, 5), d1.cpu().numpy().reshape(-1, 5)
    for row in (1, 2, 3, 4):  # outside the CSR's rows, and the full row
        assert (d0[row] == -1).all() and (d1[row] == -1).all()
    for row, i in ((0, 0), (5, SEVEN), (6, N - 1)):
        assert set(d0[row].tolist()) <= non_edges[i]
        assert (d1[row] == d0[row] + 1000).all()
    # a bare CSR without the row flags: the virtual row's listed columns are edges again
    _, d = MF.sample_negatives((g.rowptr, g.col), torch.tensor([VIRTUAL], device=cuda), k=4,
                               n_cand=M, seed=SEED)
    assert (d.cpu().numpy() == -1).all()
