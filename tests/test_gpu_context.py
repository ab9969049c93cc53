"""Device context sampler (``functional.sample_context``, msha_context_sample): every walk
slot is a CSR neighbour of the slot before it, walks stop at dead ends, the two-hop law is
the transition matrix squared, and the draws follow (seed, offset, replay counter)."""
import numpy as np
import pytest
import torch

import distill_ref as D

pytestmark = pytest.mark.gpu

N = 64
EMPTY, VIRTUAL, ONE, ONE_NB, FORK, Q = 3, 5, 9, 20, 12, 30
SEVEN = 42  # degree 7, also a neighbour of Q
Q_NB = {40: list(range(44, 48)), 41: list(range(48, 54)), 42: list(range(54, 61)),
        43: list(range(16, 24))}  # Q's neighbours: degrees 4, 6, 7, 8, disjoint rows
SEED = 20250117


@pytest.fixture(scope="module")
def csr(cuda, msha):
    """64-node square graph: an empty row, a virtual full row (all columns listed, flagged),
    a degree-1 row, FORK whose neighbours are the two dead ends and the degree-1 row, and Q
    with 25 two-hop outcomes."""
    rng = np.random.default_rng(11)
    rows = [sorted(rng.choice(N, int(rng.integers(1, 7)), replace=False).tolist())
            for _ in range(N)]
    rows[EMPTY] = []
    rows[VIRTUAL] = list(range(N))
    rows[ONE] = [ONE_NB]
    rows[FORK] = [EMPTY, VIRTUAL, ONE]
    rows[Q] = sorted(Q_NB)
    for v, nb in Q_NB.items():
        rows[v] = nb
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.concatenate([np.asarray(r, np.int32) for r in rows]).astype(np.int32)
    flag = np.zeros(N, np.uint8)
    flag[VIRTUAL] = 1
    dev = tuple(torch.as_tensor(x, device=cuda) for x in (rowptr, col, flag))
    nbrs = [set(r) for r in rows]
    nbrs[VIRTUAL] = set()  # a virtual full row counts as having no edges
    return dev, nbrs, (rowptr, col, flag)


def _check_walks(ctx, anchors, nbrs, walks, hops, n_rand, n_nodes):
    A, K = ctx.shape
    assert K == walks * hops + n_rand
    stops = 0
    for a in range(A):
        inside = 0 <= anchors[a] < N
        for w in range(walks):
            prev = int(anchors[a])
            for s in range(hops):
                got = int(ctx[a, w * hops + s])
                if not 0 <= prev < N or not nbrs[prev]:
                    assert got == -1, (a, w, s, prev, got)
                    stops += 1
                else:
                    assert got in nbrs[prev], (a, w, s, prev, got)
                prev = got
        rand = ctx[a, walks * hops:]
        if inside:
            assert ((rand >= 0) & (rand < n_nodes)).all(), a
        else:
            assert (rand == -1).all(), a
    return stops


def test_walks_follow_edges_and_stop_at_dead_ends(cuda, csr):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import Graph

    dev, nbrs, _ = csr
    anchors = np.concatenate([np.arange(N), [-1, N, 10 ** 12], np.full(64, FORK)]).astype(np.int64)
    ta = torch.as_tensor(anchors, device=cuda)
    ctx = MF.sample_context(dev, ta, walks=4, hops=3, n_rand=4, n_nodes=50, seed=SEED)
    assert ctx.dtype == torch.int64 and ctx.shape == (len(anchors), 16)
    c = ctx.cpu().numpy()
    stops = _check_walks(c, anchors, nbrs, 4, 3, 4, 50)
    assert stops > 100
    assert (c[EMPTY, :12] == -1).all() and (c[VIRTUAL, :12] == -1).all()
    assert (c[N:N + 3] == -1).all()  # anchors -1, n and 10**12: walk and random slots
    fork = c[N + 3:, :12].reshape(-1, 3)  # FORK's walks: a dead end, or ONE -> ONE_NB -> ...
    assert set(fork[:, 0].tolist()) == {EMPTY, VIRTUAL, ONE}
    dead = np.isin(fork[:, 0], (EMPTY, VIRTUAL))
    assert (fork[dead, 1:] == -1).all() and (fork[~dead, 1] == ONE_NB).all()
    assert len(set(c[:N, 12:].reshape(-1).tolist())) > 40  # random slots spread over [0, 50)
    # a Graph object: n_nodes defaults to its column count; the same walk slots
    g = Graph(N, N, dev[0], dev[1], dev[2])
    cg = MF.sample_context(g, ta, walks=4, hops=3, n_rand=4, seed=SEED).cpu().numpy()
    assert np.array_equal(cg[:, :12], c[:, :12])
    _check_walks(cg, anchors, nbrs, 4, 3, 4, N)
    # a bare CSR without the flags: the virtual row's listed columns are edges again
    cb = MF.sample_context(dev[:2], torch.full((8,), VIRTUAL, device=cuda), 4, 1, seed=SEED)
    assert (cb.cpu().numpy() >= 0).all()


def test_one_hop_covers_the_neighbours(cuda, csr):
    """4,096 one-hop walks from the degree-7 node: its seven neighbours, all of them."""
    from msha_gnn_amd import functional as MF

    dev, nbrs, _ = csr
    ctx = MF.sample_context(dev, torch.full((64,), SEVEN, device=cuda), walks=64, hops=1,
                            seed=SEED)
    assert ctx.shape == (64, 64)
    assert len(nbrs[SEVEN]) == 7 and set(ctx.cpu().numpy().reshape(-1).tolist()) == nbrs[SEVEN]


def test_two_hop_law_is_the_transition_matrix_squared(cuda, csr):
    """Pearson's chi-square of 32,768 two-hop walks from Q against row Q of P^2 (fp64): 25
    outcomes, every expected count >= 1,024; 24 degrees of freedom, bound 80 (tail ~1e-7)."""
    from msha_gnn_amd import functional as MF

    dev, _, (rowptr, col, flag) = csr
    P = D.transition(rowptr, col, flag)
    law = (P @ P)[Q]
    outcomes = np.flatnonzero(law)
    assert len(outcomes) == 25 and abs(law.sum() - 1.0) < 1e-12
    assert len(set(np.round(law[outcomes], 12).tolist())) == 4  # 1/16, 1/24, 1/28, 1/32
    A, walks = 1024, 32  # K = 64
    draws = A * walks
    assert draws * law[outcomes].min() >= 1000
    ctx = MF.sample_context(dev, torch.full((A,), Q, device=cuda), walks=walks, hops=2, seed=SEED)
    c = ctx.cpu().numpy().reshape(A, walks, 2)
    cnt = np.bincount(c[:, :, 1].reshape(-1), minlength=N)
    assert cnt.sum() == draws and cnt[outcomes].sum() == draws
    expect = draws * law[outcomes]
    chi2 = float((((cnt[outcomes] - expect) ** 2) / expect).sum())
    print(f"chi-square {chi2:.2f} at 24 degrees of freedom")
    assert chi2 < 80.0
    # the first hop alone: uniform over Q's four neighbours (3 degrees of freedom)
    c1 = np.bincount(c[:, :, 0].reshape(-1), minlength=N)[sorted(Q_NB)]
    chi1 = float((((c1 - draws / 4) ** 2) / (draws / 4)).sum())
    print(f"first hop: chi-square {chi1:.2f} at 3 degrees of freedom")
    assert c1.sum() == draws and chi1 < 40.0  # tail ~1e-8


def test_reproducible_from_seed_offset_and_replay_counter(cuda, csr):
    from msha_gnn_amd import functional as MF

    dev, nbrs, _ = csr
    anchors = torch.arange(N, device=cuda).repeat(4)
    kw = dict(walks=3, hops=2, n_rand=2, n_nodes=N)
    a = MF.sample_context(dev, anchors, seed=SEED, **kw)
    assert torch.equal(a, MF.sample_context(dev, anchors, seed=SEED, **kw))
    assert not torch.equal(a, MF.sample_context(dev, anchors, seed=SEED + 1, **kw))
    assert not torch.equal(a, MF.sample_context(dev, anchors, seed=SEED, offset=1, **kw))
    counter = torch.zeros(1, dtype=torch.int64, device=cuda)
    prev = MF.set_rng_counter(counter)
    try:
        c0 = MF.sample_context(dev, anchors, seed=SEED, **kw)
        assert torch.equal(c0, a)  # counter 0: the plain offset
        counter.add_(1)
        c1 = MF.sample_context(dev, anchors, seed=SEED, **kw)
        assert not torch.equal(c0, c1)
        assert torch.equal(c1, MF.sample_context(dev, anchors, seed=SEED, **kw))
        # K = 1 and K = 64
        k1 = MF.sample_context(dev, anchors, 1, 1, seed=SEED)
        k64 = MF.sample_context(dev, anchors, 15, 4, n_rand=4, n_nodes=N, seed=SEED)
        assert k1.shape == (4 * N, 1) and k64.shape == (4 * N, 64)
        _check_walks(k1.cpu().numpy(), anchors.cpu().numpy(), nbrs, 1, 1, 0, N)
        _check_walks(k64.cpu().numpy(), anchors.cpu().numpy(), nbrs, 15, 4, 4, N)
        # a captured graph draws afresh on every replay: each equals eager at that counter
        MF.sample_context(dev, anchors, seed=SEED, **kw)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = MF.sample_context(dev, anchors, seed=SEED, **kw)
        seen = []
        for step in (2, 3, 4):
            counter.fill_(step)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            assert torch.equal(got, MF.sample_context(dev, anchors, seed=SEED, **kw))
            assert all(not torch.equal(got, s) for s in seen + [c0, c1])
            seen.append(got)
    finally:
        MF.set_rng_counter(prev)
