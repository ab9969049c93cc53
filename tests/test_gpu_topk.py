"""Top-K link retrieval on the GPU (csrc/topk.hip) against the lexsort reference of
topk_ref.py (fp64 logits, then (index, -logit): logit descending, index ascending).

Tile sizes of the kernel, so the edges can be seen: the candidate tile is 64 rows of the
table; the query tile is 64 rows for K <= 64 and 32 rows for K > 64; a row's candidate
buffer holds 64 (K <= 64) or 128 keys before a merge; the merge entry cuts rows longer
than 4,096 into chunks."""
import numpy as np
import pytest
import torch

import topk_ref as R
from gpu_helpers import STAT_C, U32, bounded_close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
NEG_INF = float("-inf")


def _ints(rng, shape, dev, dt, lo=-3, hi=3):
    """Integer-valued entries in [lo, hi]: every product and partial sum is exact in fp32
    and in bf16 operands."""
    x = rng.integers(lo, hi + 1, shape).astype(np.float32)
    return x, torch.as_tensor(x, device=dev).to(dt)


def _assert_exact(got, want, name=""):
    gv, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    wv, wi = want
    assert gv.dtype == np.float32 and gi.dtype == np.int64
    assert gv.shape == wv.shape and gi.shape == wi.shape, name
    assert np.array_equal(gi, wi), f"{name}: indices differ in {(gi != wi).sum()} slots"
    assert np.array_equal(gv.astype(np.float64), wv, equal_nan=True), f"{name}: values differ"


# (F, n_cand, B, K): every value of the issue's grid, and each tile edge +-1 -- candidate
# tile 64 (63, 64, 65, 127, 129), query tile 64 for K <= 64 (B 63, 64, 65, 130) and 32 for
# K > 64 (B 31, 32, 33, 65); K > n_cand gives filler slots
EXACT = [(16, 1, 1, 1), (16, 31, 5, 20), (64, 33, 65, 50), (128, 257, 130, 128),
         (256, 1000, 130, 50), (128, 1000, 65, 20), (64, 63, 63, 1), (64, 64, 64, 50),
         (64, 65, 65, 128), (16, 257, 33, 128), (16, 129, 31, 128), (48, 127, 32, 65),
         (256, 33, 5, 64), (16, 1000, 1, 128)]


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_exact_grid(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(1)
    for F, n, B, K in EXACT:
        qn, q = _ints(rng, (B, F), cuda, dt)
        tn, t = _ints(rng, (n, F), cuda, dt)
        logits = qn.astype(np.float64) @ tn.astype(np.float64).T
        got = MF.topk_inner(q, t, K, sigmoid=False)
        _assert_exact(got, R.topk_rows(logits, K), f"F{F} n{n} B{B} K{K} {dt}")
        if F == 16 and n >= 257:  # the heavy-tie cases pin the index-ascending rule
            v = got[0].cpu().numpy()
            assert (v[:, 1:] == v[:, :-1]).any()


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_filler_and_empty(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(2)
    qn, q = _ints(rng, (5, 32), cuda, dt)
    tn, t = _ints(rng, (7, 32), cuda, dt)
    logits = qn.astype(np.float64) @ tn.astype(np.float64).T
    # K > n_cand: logits, then -inf / -1
    _assert_exact(MF.topk_inner(q, t, 20, sigmoid=False), R.topk_rows(logits, 20))
    # under the sigmoid the filler value is 0.0; the ranking is still by the logit
    v, i = MF.topk_inner(q, t, 20, sigmoid=True)
    wv, wi = R.topk_rows(logits, 20)
    assert torch.equal(i.cpu(), torch.as_tensor(wi))
    v = v.cpu().numpy()
    assert (v[:, 7:] == 0.0).all() and (wi[:, 7:] == -1).all()
    np.testing.assert_allclose(v[:, :7], 1.0 / (1.0 + np.exp(-wv[:, :7])), rtol=1e-5, atol=1e-7)
    # n_cand = 0: only the filler; B = 0: nothing
    v, i = MF.topk_inner(q, t[:0], 3, sigmoid=False)
    assert v.shape == (5, 3) and (v.cpu() == NEG_INF).all() and (i.cpu() == -1).all()
    v, i = MF.topk_inner(q[:0], t, 3)
    assert v.shape == (0, 3) and i.shape == (0, 3) and i.dtype == torch.int64
    # col_offset shifts real indices only
    v, i = MF.topk_inner(q, t, 9, sigmoid=False, col_offset=1000)
    wv, wi = R.topk_rows(logits, 9, col_offset=1000)
    _assert_exact((v, i), (wv, wi))
    assert (wi[:, 7:] == -1).all() and (wi[:, :7] >= 1000).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 64, 128])
def test_topk_buffer_overflow_path(cuda, msha, dt, K):
    """The query is the first unit vector and candidate j's first feature grows with j:
    every candidate beats the row's threshold in stream order, so the buffers fill and
    merge over and over.  fp32: j, n = 5,000; bf16: j // 8 (exact up to 255), n = 2,048,
    ties resolved by index.  The reverse order: nothing after the first K survives."""
    from msha_gnn_amd import functional as MF

    F = 16
    n = 5000 if dt == torch.float32 else 2048
    first = (np.arange(n) if dt == torch.float32 else np.arange(n) // 8).astype(np.float32)
    qn = np.zeros((3, F), np.float32)
    qn[0, 0], qn[1, 0], qn[2, 0] = 1.0, -1.0, 1.0  # ascending, descending, ascending
    q = torch.as_tensor(qn, device=cuda).to(dt)
    for tab_first in (first, first[::-1].copy()):
        tn = np.zeros((n, F), np.float32)
        tn[:, 0] = tab_first
        t = torch.as_tensor(tn, device=cuda).to(dt)
        logits = qn.astype(np.float64) @ tn.astype(np.float64).T
        for splits in (1, None):
            _assert_exact(MF.topk_inner(q, t, K, sigmoid=False, splits=splits),
                          R.topk_rows(logits, K), f"K{K} {dt} splits {splits}")


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_splits_do_not_change_a_bit(cuda, msha, dt):
    """The summation order of a logit is fixed by f alone, so the result cannot depend on
    the column split that computed it: torch.equal, also for random bf16 operands."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(3)
    _, qe = _ints(rng, (70, 64), cuda, dt)
    _, te = _ints(rng, (1000, 64), cuda, dt)
    g = torch.Generator().manual_seed(4)
    qr = torch.rand(70, 128, generator=g).to(cuda).to(dt)
    tr = (torch.rand(4099, 128, generator=g) - 0.3).to(cuda).to(dt)
    for q, t, K in ((qe, te, 50), (qr, tr, 50), (qr, tr, 100)):
        base = MF.topk_inner(q, t, K, sigmoid=False, splits=1)
        for s in (3, 7, None, 64):
            got = MF.topk_inner(q, t, K, sigmoid=False, splits=s)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (s, K, dt)


@pytest.fixture(scope="module")
def rnd():
    """torch.rand table and queries, like the c5 fixture of test_gpu_sharded.py but small."""
    n, F, B = 4099, 128, 130
    g = torch.Generator().manual_seed(21)
    return dict(n=n, F=F, B=B, h=torch.rand(n, F, generator=g), q=torch.rand(B, F, generator=g))


def _rnd_ref(rnd, dt):
    """fp64 logits of the exact operand values of dtype dt, and A = sum_f |q_f t_f|."""
    h = rnd["h"].to(dt).double().numpy()
    q = rnd["q"].to(dt).double().numpy()
    return q @ h.T, np.abs(q) @ np.abs(h).T


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_random_floats(cuda, msha, rnd, dt):
    """Values: each returned value against the fp64 logit of the returned index,
    |err| <= rtol |ref| + 4 sqrt(F + 1) u A with A = sum |q_f t_f| and rtol 1e-5 for both
    types.  The project's bf16 figure is 1e-2 (test_gpu_sharded.py), but the bf16 path
    feeds exact bf16 operands to fp32 accumulators and the reference gets the same operand
    values, so it rounds like the fp32 path: measured worst err / bound 2.3e-5 at 1e-2,
    hence the fp32 figure here (measured at 1e-5: fp32 0.050, bf16 about 0.02 of the bound).
    Index set, e = the row's largest such bound, no element exempt: every returned logit
    >= (K-th largest) - 2e; every logit not returned <= (smallest returned) + 2e."""
    from msha_gnn_amd import functional as MF

    K, F, B, n = 50, rnd["F"], rnd["B"], rnd["n"]
    rtol = 1e-5
    L, A = _rnd_ref(rnd, dt)
    v, i = MF.topk_inner(rnd["q"].to(cuda).to(dt), rnd["h"].to(cuda).to(dt), K, sigmoid=False)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    assert ((i >= 0) & (i < n)).all()
    rows = np.arange(B)[:, None]
    worst, _ = bounded_close(v, L[rows, i], A[rows, i], F + 1, rtol, f"topk values {dt}")
    print(f"topk values {dt}: worst err / bound {worst:.3g}")
    e = (rtol * np.abs(L) + STAT_C * np.sqrt(F + 1) * U32 * A).max(axis=1)
    kth = np.sort(L, axis=1)[:, -K]
    got = L[rows, i]
    assert (got >= (kth - 2 * e)[:, None]).all()
    out = np.ones((B, n), bool)
    out[rows, i] = False
    assert out.sum() == B * (n - K)  # distinct indices
    assert (np.where(out, L, -np.inf).max(axis=1) <= got.min(axis=1) + 2 * e).all()
    # each row sorted: values non-increasing, equal neighbours by ascending index
    assert (v[:, 1:] <= v[:, :-1]).all()
    tie = v[:, 1:] == v[:, :-1]
    assert (i[:, 1:][tie] > i[:, :-1][tie]).all()
    # sigmoid: the same indices, probabilities within the 0.25 A scaled bound
    vs, js = MF.topk_inner(rnd["q"].to(cuda).to(dt), rnd["h"].to(cuda).to(dt), K, sigmoid=True)
    assert np.array_equal(js.cpu().numpy(), i)
    bounded_close(vs.cpu().numpy(), 1.0 / (1.0 + np.exp(-got)), 0.25 * A[rows, i], F + 1, rtol,
                  f"topk sigmoid {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_gather_and_bounds(cuda, msha, dt):
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(6)
    _, h = _ints(rng, (300, 64), cuda, dt)
    rows = torch.as_tensor(rng.permutation(300)[:100].tolist() + [5, 5, 299, 0, 5], device=cuda)
    K = 10
    want = MF.topk_inner(h[rows].contiguous(), h, K)
    got = MF.topk_inner(h, h, K, rows=rows)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    neg = rows.clone()
    neg[3] -= 300  # torch's wrap
    got = MF.topk_inner(h, h, K, rows=neg)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a stray index: IndexError before any launch with check=True ...
    stray = rows.clone()
    stray[7] = 300
    with pytest.raises(IndexError):
        MF.topk_inner(h, h, K, rows=stray)
    # ... and with check=False the row comes back as filler, the others untouched: the
    # kernel decides validity from the index alone and reads nothing through it
    v, i = MF.topk_inner(h, h, K, rows=stray, check=False, sigmoid=False)
    wv, wi = MF.topk_inner(h, h, K, rows=rows, sigmoid=False)
    keep = torch.arange(rows.numel(), device=cuda) != 7
    assert torch.equal(v[keep], wv[keep]) and torch.equal(i[keep], wi[keep])
    assert (v[7].cpu() == NEG_INF).all() and (i[7].cpu() == -1).all()
    # err is set at the ABI level (and stays clear without a stray index)
    for idx, flag in ((stray, 1), (rows, 0)):
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        ov = torch.empty(rows.numel(), K, device=cuda)
        oi = torch.empty(rows.numel(), K, dtype=torch.int64, device=cuda)
        _lib.call("msha_topk_inner", rows.numel(), 64, 1 if dt == torch.bfloat16 else 0,
                  h.data_ptr(), h.stride(0), idx.data_ptr(), 300, h.data_ptr(), h.stride(0), 300,
                  0, None, None, K, 0, 1, ov.data_ptr(), oi.data_ptr(), err.data_ptr(), None, 0,
                  _lib.stream_handle(cuda))
        assert int(err.item()) == flag


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_exclusion(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(7)
    n, F, K = 200, 32, 20
    qn, q = _ints(rng, (6, F), cuda, dt)
    tn, t = _ints(rng, (n, F), cuda, dt)
    logits = qn.astype(np.float64) @ tn.astype(np.float64).T
    _, top = R.topk_rows(logits, K)
    excl = [[int(top[0, 0])],                 # removes the best candidate
            top[1].tolist(),                  # removes K candidates from the top
            [],                               # an empty list
            list(range(n)),                   # every candidate excluded: all filler
            list(range(n - K + 5)),           # n_cand - |excluded| < K
            [int(top[5, 3]), int(top[5, 3]), 0, n - 1]]  # duplicates, the two ends
    qpos = np.concatenate([np.full(len(e), b) for b, e in enumerate(excl)]).astype(np.int64)
    cols = np.concatenate([np.asarray(e, np.int64) for e in excl])
    perm = rng.permutation(len(qpos))
    ex = MF.exclude_from_pairs(torch.as_tensor(qpos[perm], device=cuda),
                               torch.as_tensor(cols[perm], device=cuda), 6)
    rp_ref, col_ref = R.exclude_csr(excl)
    assert np.array_equal(ex[0].cpu().numpy(), rp_ref) and np.array_equal(ex[1].cpu().numpy(), col_ref)
    want = R.topk_rows(logits, K, excl)
    assert (want[1][3] == -1).all() and (want[1][4, 15:] == -1).all() and want[1][4, 14] >= 0
    for splits in (1, 3):
        _assert_exact(MF.topk_inner(q, t, K, exclude=ex, sigmoid=False, splits=splits), want)
    # an exclusion CSR with no columns at all is the plain call
    empty = MF.exclude_from_pairs(torch.zeros(0, dtype=torch.int64, device=cuda),
                                  torch.zeros(0, dtype=torch.int64, device=cuda), 6)
    _assert_exact(MF.topk_inner(q, t, K, exclude=empty, sigmoid=False), R.topk_rows(logits, K))


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_non_finite(cuda, msha, dt):
    """+inf first, NaN after -inf, NaN before the filler; NaNs among themselves by index."""
    from msha_gnn_amd import functional as MF

    F, n, K = 16, 10, 12
    tn = np.zeros((n, F), np.float32)
    tn[:, 0] = [1, -2, np.inf, 3, np.nan, -np.inf, 0, np.nan, 2, -1]
    q = torch.ones(2, F, device=cuda, dtype=dt)
    v, i = MF.topk_inner(q, torch.as_tensor(tn, device=cuda).to(dt), K, sigmoid=False)
    assert i[0].tolist() == [2, 3, 8, 0, 6, 9, 1, 5, 4, 7, -1, -1]
    assert torch.equal(i[0], i[1])
    v = v[0].cpu().numpy()
    assert v[0] == np.inf and v[7] == -np.inf and np.isnan(v[8:10]).all()
    assert (v[10:] == -np.inf).all() and list(v[1:7]) == [3, 2, 1, 0, -1, -2]


def test_topk_merge_alone(cuda, msha):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(8)
    for rows in (1, 3):
        for lists in (1, 2, 8):
            for ln in (1, 50, 128):
                for K in (1, 20, 128):
                    vn = rng.integers(-4, 5, (rows, lists, ln)).astype(np.float32)
                    idn = rng.permutation(rows * lists * ln).reshape(rows, lists, ln).astype(np.int64)
                    idn[rng.random(idn.shape) < 0.2] = -1
                    v = torch.as_tensor(vn, device=cuda)
                    name = f"rows{rows} lists{lists} len{ln} K{K}"
                    _assert_exact(MF.topk_merge(v, None, K),
                                  R.merge_rows(vn.reshape(rows, -1), None, K), name)
                    _assert_exact(MF.topk_merge(v, torch.as_tensor(idn, device=cuda), K),
                                  R.merge_rows(vn.reshape(rows, -1), idn.reshape(rows, -1), K),
                                  name + " idx")
    # one long row: cut into chunks, selected per chunk, merged again
    vn = rng.integers(-1000, 1001, (1, 300_001)).astype(np.float32)
    _assert_exact(MF.topk_merge(torch.as_tensor(vn, device=cuda), None, 50),
                  R.merge_rows(vn, None, 50), "long row")
    vn = rng.integers(-5, 6, (2, 20_000)).astype(np.float32)  # heavy ties, two levels
    _assert_exact(MF.topk_merge(torch.as_tensor(vn, device=cuda), None, 128),
                  R.merge_rows(vn, None, 128), "two rows")
    # sigmoid maps the winners; the filler is 0.0
    v, i = MF.topk_merge(torch.tensor([[0.0, 2.0, -1.0]], device=cuda), None, 5, sigmoid=True)
    assert i[0].tolist() == [1, 0, 2, -1, -1] and v[0, 3:].tolist() == [0.0, 0.0]
    np.testing.assert_allclose(v[0, :3].cpu().numpy(), 1 / (1 + np.exp([-2.0, 0.0, 1.0])), rtol=1e-6)


@pytest.mark.parametrize("dt", DTYPES)
def test_link_predictor_topk(cuda, msha, rnd, dt):
    """The returned probabilities agree with score_pairs on the returned pairs (the pair
    kernel sums in another order, so a bound, not equality)."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rtol = 1e-2 if dt == torch.bfloat16 else 1e-5
    h = rnd["h"][:1000].to(cuda).to(dt) - 0.45  # logits around zero: probabilities spread
    cand = rnd["h"][1000:1700].to(cuda).to(dt) - 0.45
    pred = layers.LinkPredictor("inner", 128, 128, 1, 2, 0.0)
    src = torch.as_tensor(np.random.default_rng(9).integers(0, 1000, 70), device=cuda)
    K = 50
    hd = h.double().cpu().numpy()
    for c, cd in ((None, hd), (cand, cand.double().cpu().numpy())):
        p, idx = pred.topk(h, src, K, candidates=c)
        assert p.shape == (70, K) and ((idx >= 0) & (idx < cd.shape[0])).all()
        s = src.repeat_interleave(K)
        if c is None:
            pair = pred.score_pairs(h, s, idx.reshape(-1))
        else:
            both = torch.cat([h, c])
            pair = pred.score_pairs(both, s, idx.reshape(-1) + 1000)
        A = 0.25 * (np.abs(hd[s.cpu().numpy()]) * np.abs(cd[idx.reshape(-1).cpu().numpy()])).sum(1)
        bounded_close(p.reshape(-1).cpu().numpy(), pair.double().cpu().numpy(), A, 128 + 1, rtol,
                      f"LinkPredictor.topk vs score_pairs {dt}")
        assert (p[:, 1:] <= p[:, :-1]).all()


def test_topk_never_materialises_the_scores(cuda, msha):
    """B = 2,048 against 100,000 x 128 fp32, K = 50: the (B, n) matrix would be 819 MB; the
    call's peak allocation stays under 64 MB.  A condition, not a measurement."""
    from msha_gnn_amd import functional as MF

    g = torch.Generator(device=cuda).manual_seed(31)
    h = torch.rand(100_000, 128, device=cuda, generator=g)
    rows = torch.randint(0, 100_000, (2048,), device=cuda, generator=g)
    MF.topk_inner(h[:256], h[:4096], 50)  # library load and first-launch allocations
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    v, i = MF.topk_inner(h, h, 50, rows=rows, check=False)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"topk_inner peak allocation rise: {rise / 2 ** 20:.1f} MiB")
    assert rise < 64 * 2 ** 20
    # every query's best match is itself or a row that scores at least as high
    assert v.shape == (2048, 50) and ((i >= 0) & (i < 100_000)).all()
    assert (v[:, 1:] <= v[:, :-1]).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_topk_captures_into_a_graph(cuda, msha, dt):
    """check=False: no host sync and no allocation beyond torch's, so the call records into
    a torch.cuda.graph (one chain, no side streams) and replays to the same bits."""
    from msha_gnn_amd import functional as MF

    g = torch.Generator().manual_seed(41)
    h = torch.rand(3000, 64, generator=g).to(cuda).to(dt)
    rows = torch.randint(0, 3000, (40,), generator=g).to(cuda)
    want = MF.topk_inner(h, h, 20, rows=rows, check=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = MF.topk_inner(h, h, 20, rows=rows, check=False)
    for _ in range(2):
        got[0].zero_()
        got[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # new inputs in the captured buffers, same graph
    h2 = torch.rand(3000, 64, generator=g).to(dt)
    want2 = MF.topk_inner(h2.to(cuda), h2.to(cuda), 20, rows=rows, check=False)
    h.copy_(h2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want2[0]) and torch.equal(got[1], want2[1])


def test_hits_at_k(cuda, msha):
    from msha_gnn_amd import metrics

    rng = np.random.default_rng(10)
    # ties at the threshold: strictly greater
    neg = np.array([5, 5, 5, 4, 3, 2, 1, 0], np.float32)
    pos = np.array([5, 6, 4.5, 5, 7], np.float32)
    for k in (1, 3, 4, 8):
        got = metrics.hits_at_k(torch.as_tensor(pos, device=cuda), torch.as_tensor(neg, device=cuda), k)
        assert got == R.hits_at_k(pos, neg, k), k
    assert metrics.hits_at_k(torch.as_tensor(pos, device=cuda), torch.as_tensor(neg, device=cuda), 3) == 0.4
    # fewer than K negatives
    assert metrics.hits_at_k(torch.as_tensor(pos, device=cuda), torch.as_tensor(neg, device=cuda), 9) == 1.0
    assert metrics.hits_at_k(torch.as_tensor(pos, device=cuda), torch.zeros(0, device=cuda), 1) == 1.0
    # the hierarchical selection
    neg = rng.integers(-50_000, 50_001, 300_001).astype(np.float32) / 8
    pos = rng.integers(-50_000, 60_001, 1000).astype(np.float32) / 8
    pt, nt = torch.as_tensor(pos, device=cuda), torch.as_tensor(neg, device=cuda)
    for k in (20, 50, 128):
        assert metrics.hits_at_k(pt, nt, k) == R.hits_at_k(pos, neg, k), k
    # bf16 widens exactly
    pb, nb = pt[:500].to(torch.bfloat16), nt[:5000].to(torch.bfloat16)
    want = R.hits_at_k(pb.float().cpu().numpy(), nb.float().cpu().numpy(), 50)
    assert metrics.hits_at_k(pb, nb, 50) == want and 0.0 < want < 1.0
    # non-finite -> NaN; empty pos -> ValueError
    bad = nt[:100].clone()
    bad[3] = float("inf")
    assert np.isnan(metrics.hits_at_k(pt, bad, 5))
    badp = pt.clone()
    badp[0] = float("nan")
    assert np.isnan(metrics.hits_at_k(badp, nt[:100], 5))
    with pytest.raises(ValueError):
        metrics.hits_at_k(pt[:0], nt, 5)
