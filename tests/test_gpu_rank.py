"""Filtered link ranks on the GPU (csrc/rank.hip) against the numpy reference of
rank_ref.py (fp64 logits, counts under the library's order).

Tile sizes of the kernel, so the edges can be seen: the candidate tile is 64 rows of the
table, the query tile 128 rows (wave w holds rows 32 w .. +31); a column split is a whole
number of candidate tiles."""
import numpy as np
import pytest
import torch

import rank_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _ints(rng, shape, dev, dt, lo=-3, hi=3):
    """Integer-valued entries in [lo, hi]: every product and partial sum is exact in fp32
    and in bf16 operands."""
    x = rng.integers(lo, hi + 1, shape).astype(np.float32)
    return x, torch.as_tensor(x, device=dev).to(dt)


def _np(t):
    return t.cpu().numpy()


def _assert_counts(got, want, name=""):
    g, e = _np(got[0]), _np(got[1])
    assert g.dtype == np.int64 and e.dtype == np.int64 and got[2].dtype == torch.float32
    assert np.array_equal(g, want[0]), f"{name}: greater differs in {(g != want[0]).sum()} rows"
    assert np.array_equal(e, want[1]), f"{name}: equal differs in {(e != want[1]).sum()} rows"


def _csr(lists, dev):
    import topk_ref

    rp, col = topk_ref.exclude_csr(lists)
    return torch.as_tensor(rp, device=dev), torch.as_tensor(col, device=dev)


# every value of the grid, each candidate-tile edge +-1 (63, 64, 65, 129, 257) and each
# query-tile edge +-1 (127, 128, 129) besides the 64-row edges of the top-K kernel
GRID_F = (16, 48, 128, 256)
GRID_N = (1, 63, 64, 65, 129, 257, 1000)
GRID_B = (1, 63, 64, 65, 127, 128, 129, 130)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_exact_grid(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(1)
    for F in GRID_F:
        for n in GRID_N:
            tn, t = _ints(rng, (n, F), cuda, dt)
            for B in GRID_B:
                qn, q = _ints(rng, (B, F), cuda, dt)
                target = rng.integers(0, n, B)
                logits = qn.astype(np.float64) @ tn.astype(np.float64).T
                want = R.counts(logits, target)
                got = MF.rank_inner(q, t, torch.as_tensor(target, device=cuda))
                name = f"F{F} n{n} B{B} {dt}"
                _assert_counts(got, want, name)
                assert np.array_equal(_np(got[2]).astype(np.float64),
                                      logits[np.arange(B), target]), name
                if F == 16 and n >= 257:  # the heavy-tie cases pin the == count
                    assert (want[1] > 0).any(), name


@pytest.fixture(scope="module")
def rnd():
    """The fixture of test_gpu_topk.py: torch.rand, seed 21."""
    n, F, B = 4099, 128, 130
    g = torch.Generator().manual_seed(21)
    return dict(n=n, F=F, B=B, h=torch.rand(n, F, generator=g), q=torch.rand(B, F, generator=g))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", (50, 128))
@pytest.mark.parametrize("F", (16, 48, 128, 256))
def test_rank_consistent_with_topk(cuda, msha, rnd, F, K, dt):
    """The K-th entry of topk_inner's list has exactly K better-ordered candidates; those
    are above it or tie with it, so greater <= K <= greater + equal -- and its logit is the
    listed value, bit for bit.  No tolerance.

    The two kernels meet in every shape of the shared tile: F = 16 and 48 end inside a
    256-byte chunk, 128 and 256 fill one to four of them; K = 50 runs the top-K kernel's
    64-row query tile (two 16-candidate groups a wave), K = 128 its 32-row tile (one group),
    against the rank kernel's four groups.  200 candidates are four candidate tiles, the
    last ragged; 130 queries two rank tiles, the last ragged.  The fixture's first 200 table
    rows, cut to F columns (256: the next 200 rows and 130 rows after them as columns
    128 .. 255 of the table and the queries)."""
    from msha_gnn_amd import functional as MF

    n, B = 200, rnd["B"]
    h, q = rnd["h"][:n], rnd["q"]
    if F > rnd["F"]:
        h = torch.cat([h, rnd["h"][n:2 * n]], 1)
        q = torch.cat([q, rnd["h"][2 * n:2 * n + B]], 1)
    q, h = q[:, :F].to(cuda).to(dt), h[:, :F].to(cuda).to(dt)
    vals, idx = MF.topk_inner(q, h, K, sigmoid=False)
    pos = torch.arange(B, device=cuda) % K
    target = idx[torch.arange(B, device=cuda), pos]
    g, e, z = MF.rank_inner(q, h, target)
    assert (g <= pos).all() and (pos <= g + e).all()
    assert torch.equal(z.view(torch.int32), vals[torch.arange(B, device=cuda), pos].view(torch.int32))


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_same_chain_tie(cuda, msha, rnd, dt):
    """Copies of the target row tie with it exactly: the target's logit comes from the
    same accumulation chain as every candidate's."""
    from msha_gnn_amd import functional as MF

    q = rnd["q"].to(cuda).to(dt)
    h = rnd["h"].to(cuda).to(dt).clone()
    B = rnd["B"]
    target = torch.full((B,), 7, dtype=torch.int64, device=cuda)
    ex = _csr([[70, 3000]] * B, cuda)
    g0, e0, z0 = MF.rank_inner(q, h, target, exclude=ex)
    h[70] = h[7]
    h[3000] = h[7]
    g1, e1, z1 = MF.rank_inner(q, h, target)
    assert torch.equal(g1, g0) and torch.equal(e1, e0 + 2) and (e1 >= 2).all()
    assert torch.equal(z1.view(torch.int32), z0.view(torch.int32))


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_random_floats(cuda, msha, dt):
    """Random floats against fp64 on the dtype-rounded operands: greater >= lo and
    greater + equal <= hi with the brackets of rank_ref.bracket (delta = 4 sqrt(F) 2^-24
    sum |q_f t_f| per logit).  test_rank_host.py guards that the brackets decide all but at
    most 13 of the 130 queries, and those to one place."""
    from msha_gnn_amd import functional as MF

    p = R.random_problem(dt)
    lo, hi = R.bracket(p["qd"], p["hd"], p["target"])
    g, e, z = MF.rank_inner(p["q"].to(cuda), p["h"].to(cuda),
                            torch.as_tensor(p["target"], device=cuda))
    g, e = _np(g), _np(e)
    print(f"{dt}: greater - lo max {(g - lo).max()}, hi - (greater + equal) min {(hi - g - e).min()}")
    assert (g >= lo).all() and (g + e <= hi).all()
    assert (e >= 0).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_splits_do_not_change_a_bit(cuda, msha, rnd, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(3)
    _, qe = _ints(rng, (70, 64), cuda, dt)
    _, te = _ints(rng, (1000, 64), cuda, dt)
    qr, tr = rnd["q"].to(cuda).to(dt), (rnd["h"] - 0.3).to(cuda).to(dt)
    for q, t in ((qe, te), (qr, tr)):
        target = torch.as_tensor(rng.integers(0, t.shape[0], q.shape[0]), device=cuda)
        ex = _csr([rng.integers(0, t.shape[0], 40).tolist() for _ in range(q.shape[0])], cuda)
        for exclude in (None, ex):
            base = MF.rank_inner(q, t, target, exclude=exclude, splits=1)
            for s in (1, 3, 7, None, 64):
                got = MF.rank_inner(q, t, target, exclude=exclude, splits=s)
                assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                       b.view(torch.int32) if b.dtype == torch.float32 else b)
                           for a, b in zip(got, base)), (s, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_exclusion(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(7)
    n, F, B = 200, 32, 6
    qn, q = _ints(rng, (B, F), cuda, dt)
    tn, t = _ints(rng, (n, F), cuda, dt)
    logits = qn.astype(np.float64) @ tn.astype(np.float64).T
    target = rng.integers(0, n, B)
    order = np.argsort(-logits, axis=1, kind="stable")
    excl = [order[0, :10].tolist(),                         # the strongest candidates
            [int(target[1])],                               # the target alone
            [],                                             # an empty list
            list(range(n)),                                 # every candidate: 0 / 0
            [int(target[4])] + order[4, :30].tolist(),      # the target among others
            rng.integers(0, n, 50).tolist()]                # a random list, duplicates
    ex = _csr(excl, cuda)
    want = R.counts(logits, target, excl)
    assert want[0][3] == 0 and want[1][3] == 0
    tg = torch.as_tensor(target, device=cuda)
    for splits in (1, 3):
        _assert_counts(MF.rank_inner(q, t, tg, exclude=ex, splits=splits), want, f"s{splits}")
    # a target in its own list changes nothing: it never counts
    plain = R.counts(logits, target)
    assert want[0][1] == plain[0][1] and want[1][1] == plain[1][1]
    # an exclusion CSR with no columns at all is the plain call
    empty = MF.exclude_from_pairs(torch.zeros(0, dtype=torch.int64, device=cuda),
                                  torch.zeros(0, dtype=torch.int64, device=cuda), B)
    _assert_counts(MF.rank_inner(q, t, tg, exclude=empty), plain)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_known_edges_of_one_table(cuda, msha, dt):
    """The evaluation loop's shape: q is the table, rows = src, the known edges of every
    source and the source itself filtered out."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    rng = np.random.default_rng(8)
    n, F, B = 300, 64, 150
    hn, h = _ints(rng, (n, F), cuda, dt)
    src, dst = rng.integers(0, n, B), rng.integers(0, n, B)
    es, ed = rng.integers(0, n, 2000), rng.integers(0, n, 2000)  # the known graph
    known = [set(ed[es == s].tolist()) | {int(s)} for s in src]
    qpos = np.concatenate([np.full(len(k), b) for b, k in enumerate(known)])
    cols = np.concatenate([np.asarray(sorted(k)) for k in known])
    ex = MF.exclude_from_pairs(torch.as_tensor(qpos, device=cuda),
                               torch.as_tensor(cols, device=cuda), B)
    logits = hn[src].astype(np.float64) @ hn.astype(np.float64).T
    want = R.counts(logits, dst, [sorted(k) for k in known])
    s, d = torch.as_tensor(src, device=cuda), torch.as_tensor(dst, device=cuda)
    _assert_counts(MF.rank_inner(h, h, d, rows=s, exclude=ex), want)
    pred = layers.LinkPredictor("inner", F, F, 1, 2, 0.0)
    _assert_counts(pred.rank(h, s, d, exclude=ex), want)
    cand = h[:100]
    want_c = R.counts(logits[:, :100], dst % 100)
    _assert_counts(pred.rank(h, s, d % 100, candidates=cand), want_c)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_special_values(cuda, msha, dt):
    """Logits +inf, -inf, NaN and zero as candidates and as targets: +inf highest, NaNs tie
    among themselves below -inf.  A chain that starts from +0.0 never ends in -0.0, so the
    folded zero comes in as a given target logit: -0.0 ties every zero candidate."""
    from msha_gnn_amd import functional as MF

    F = 16
    first = [1, -2, np.inf, 3, np.nan, -np.inf, 0.0, np.nan, 2, -1, 0.0, 0.0, np.inf, -np.inf]
    n = len(first)
    tn = np.zeros((n, F), np.float32)  # one live feature: 0 * inf never arises
    tn[:, 0] = first
    t = torch.as_tensor(tn, device=cuda).to(dt)
    qn = np.zeros((2 * n, F), np.float32)
    qn[:n, 0] = 1.0   # logit = the candidate's first feature
    qn[n:, 0] = -1.0  # and its negative
    q = torch.as_tensor(qn, device=cuda).to(dt)
    target = np.concatenate([np.arange(n), np.arange(n)])
    with np.errstate(invalid="ignore"):
        logits = qn.astype(np.float64) @ tn.astype(np.float64).T
    want = R.counts(logits, target)
    got = MF.rank_inner(q, t, torch.as_tensor(target, device=cuda))
    _assert_counts(got, want)
    # spelled out for the +1 query: (greater, equal) of each target
    assert (want[0][2], want[1][2]) == (0, 1)        # +inf ties the other +inf
    assert (want[0][4], want[1][4]) == (n - 2, 1)    # a NaN: below all, ties the other NaN
    assert (want[0][5], want[1][5]) == (n - 4, 1)    # -inf: above the NaNs only
    assert (want[0][6], want[1][6]) == (5, 2)        # a zero ties the other zeros
    z = _np(got[2])
    assert z[2] == np.inf and z[5] == -np.inf and np.isnan(z[4]) and z[n + 2] == -np.inf
    # given target logits, targets outside the table: every candidate counts
    given = np.asarray([-0.0, 0.0, np.nan, np.inf, -np.inf, 2.0, -np.nan], np.float32)
    assert np.signbit(given[0]) and not np.signbit(given[1])
    qg = q[:1].expand(len(given), F).contiguous()
    far = torch.full((len(given),), n + 3, dtype=torch.int64, device=cuda)
    got = MF.rank_inner(qg, t, far, target_logit=torch.as_tensor(given, device=cuda))
    want = R.counts(np.repeat(logits[:1], len(given), 0), _np(far), None, 0, given)
    _assert_counts(got, want)
    assert (want[0][0], want[1][0]) == (5, 3) and (want[0][1], want[1][1]) == (5, 3)
    assert (want[0][2], want[1][2]) == (n - 2, 2) and (want[0][6], want[1][6]) == (n - 2, 2)
    assert torch.equal(got[2].view(torch.int32),
                       torch.as_tensor(given, device=cuda).view(torch.int32))


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_layout(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(9)
    n, F, B = 257, 48, 70
    esz = 4 if dt == torch.float32 else 2
    _, wide_t = _ints(rng, (n, 2 * F + 16), cuda, dt)
    _, wide_q = _ints(rng, (B, 2 * F + 16), cuda, dt)
    target = torch.as_tensor(rng.integers(0, n, B), device=cuda)
    for c0 in (0, F, 16 // esz * 5):  # column slices: pitch > F, 16-byte aligned starts
        t, q = wide_t[:, c0:c0 + F], wide_q[:, c0:c0 + F]
        assert t.stride(0) > F and t.data_ptr() % 16 == 0
        want = MF.rank_inner(q.contiguous(), t.contiguous(), target)
        got = MF.rank_inner(q, t, target)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a start that is not 16-byte aligned goes through .contiguous()
    t, q = wide_t[:, 1:1 + F], wide_q[:, 1:1 + F]
    assert t.data_ptr() % 16 != 0
    logits = q.double().cpu().numpy() @ t.double().cpu().numpy().T
    _assert_counts(MF.rank_inner(q, t, target), R.counts(logits, _np(target)))


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_stray_indices(cuda, msha, dt):
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(6)
    n, F = 300, 64
    hn, h = _ints(rng, (n, F), cuda, dt)
    rows = torch.as_tensor(rng.permutation(n)[:100].tolist() + [5, 5, 299, 0, 5], device=cuda)
    B = rows.numel()
    target = torch.as_tensor(rng.integers(0, n, B), device=cuda)
    want = MF.rank_inner(h[rows].contiguous(), h, target)
    logits = hn[_np(rows)].astype(np.float64) @ hn.astype(np.float64).T
    _assert_counts(want, R.counts(logits, _np(target)))
    # negatives wrap, for rows and for targets
    neg_r, neg_t = rows.clone(), target.clone()
    neg_r[3] -= n
    neg_t[11] -= n
    neg_t[12] = -n
    target[12] = 0
    want = MF.rank_inner(h, h, target, rows=rows)
    got = MF.rank_inner(h, h, neg_t, rows=neg_r)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # IndexError at n and at -(n + 1), for rows and for targets, before any launch
    for bad in (n, -(n + 1)):
        stray = rows.clone()
        stray[7] = bad
        with pytest.raises(IndexError):
            MF.rank_inner(h, h, target, rows=stray)
        stray = target.clone()
        stray[9] = bad
        with pytest.raises(IndexError):
            MF.rank_inner(h, h, stray, rows=rows)
    # check=False: -1 / -1 on those rows only; the kernel reads nothing through them
    sr, st = rows.clone(), target.clone()
    sr[7], sr[8] = n, -(n + 1)
    st[9], st[10] = n, -(n + 1)
    g, e, z = MF.rank_inner(h, h, st, rows=sr, check=False)
    keep = torch.ones(B, dtype=torch.bool, device=cuda)
    keep[7:11] = False
    assert torch.equal(g[keep], want[0][keep]) and torch.equal(e[keep], want[1][keep])
    assert torch.equal(z[keep], want[2][keep])
    assert (g[~keep] == -1).all() and (e[~keep] == -1).all() and torch.isnan(z[~keep]).all()
    # err at the ABI level: bit 1 a stray row, bit 2 a target that is not local
    for r_, t_, flag in ((sr, target, 1), (rows, st, 2), (sr, st, 3), (rows, target, 0)):
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        og = torch.empty(B, dtype=torch.int64, device=cuda)
        oe = torch.empty(B, dtype=torch.int64, device=cuda)
        ws = torch.empty(_lib.fn("msha_rank_inner_workspace_size")(B, n, 1), dtype=torch.uint8,
                         device=cuda)
        _lib.call("msha_rank_inner", B, F, 1 if dt == torch.bfloat16 else 0, h.data_ptr(),
                  h.stride(0), r_.data_ptr(), n, h.data_ptr(), h.stride(0), n, 0, t_.data_ptr(),
                  None, None, None, 1, og.data_ptr(), oe.data_ptr(), None, err.data_ptr(),
                  ws.data_ptr(), ws.numel(), _lib.stream_handle(cuda))
        assert int(err.item()) == flag


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_empties(cuda, msha, dt):
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(2)
    _, q = _ints(rng, (5, 32), cuda, dt)
    _, t = _ints(rng, (7, 32), cuda, dt)
    none = torch.zeros(0, dtype=torch.int64, device=cuda)
    g, e, z = MF.rank_inner(q[:0], t, none)
    assert g.shape == (0,) and e.shape == (0,) and z.shape == (0,)
    assert g.dtype == torch.int64 and z.dtype == torch.float32
    g, e, z = MF.rank_inner(q, t, none, rows=none)
    assert g.shape == (0,)
    # no candidates, the targets' logits given: nothing is above or equal
    tl = torch.arange(5, dtype=torch.float32, device=cuda)
    g, e, z = MF.rank_inner(q, t[:0], torch.arange(5, device=cuda), target_logit=tl)
    assert (g == 0).all() and (e == 0).all() and torch.equal(z, tl)
    # no candidates and no logit: no target is local
    g, e, z = MF.rank_inner(q, t[:0], torch.arange(5, device=cuda), check=False)
    assert (g == -1).all() and (e == -1).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_col_offset_shards(cuda, msha, rnd, dt):
    """Two shard views table[lo:hi] with col_offset = lo, global targets and the targets'
    logits from a full-table call: each reproduces the reference on its columns, and their
    counts add up to the full call's, exactly."""
    from msha_gnn_amd import functional as MF

    rng = np.random.default_rng(4)
    n, cut = 1000, 437
    for kind in ("ints", "rand"):
        if kind == "ints":
            hn, h = _ints(rng, (n, 32), cuda, dt)
            qn, q = _ints(rng, (70, 32), cuda, dt)
        else:
            h, q = (rnd["h"][:n] - 0.4).to(cuda).to(dt), (rnd["q"][:70] - 0.4).to(cuda).to(dt)
        target = rng.integers(0, n, 70)
        excl = [rng.integers(0, n, 30).tolist() for _ in range(70)]
        tg = torch.as_tensor(target, device=cuda)
        for lists in (None, excl):
            full = MF.rank_inner(q, h, tg, exclude=None if lists is None else _csr(lists, cuda))
            total_g = torch.zeros_like(full[0])
            total_e = torch.zeros_like(full[1])
            for lo, hi in ((0, cut), (cut, n)):
                loc = None
                if lists is not None:
                    loc = [[c - lo for c in l if lo <= c < hi] for l in lists]
                g, e, z = MF.rank_inner(q, h[lo:hi], tg, col_offset=lo, target_logit=full[2],
                                        exclude=None if loc is None else _csr(loc, cuda))
                assert torch.equal(z, full[2])
                if kind == "ints":
                    logits = qn.astype(np.float64) @ hn[lo:hi].astype(np.float64).T
                    _assert_counts((g, e, z), R.counts(logits, target, loc, lo, _np(full[2])),
                                   f"shard {lo}:{hi}")
                total_g += g
                total_e += e
            assert torch.equal(total_g, full[0]) and torch.equal(total_e, full[1])
            # without the logit a target on the other shard has no rank
            g, e, z = MF.rank_inner(q, h[:cut], tg, check=False)
            other = torch.as_tensor(target >= cut, device=cuda)
            assert (g[other] == -1).all() and (g[~other] >= 0).all()


def test_rank_metrics(cuda, msha):
    from msha_gnn_amd import metrics

    rng = np.random.default_rng(12)
    for n in (1, 300, 40_000):  # 40,000: more than one block of the summary
        g = rng.integers(0, 50, n)
        e = rng.integers(0, 4, n)
        drop = rng.random(n) < 0.1 if n > 1 else np.zeros(n, bool)
        g[drop], e[drop] = -1, -1
        gd, ed = torch.as_tensor(g, device=cuda), torch.as_tensor(e, device=cuda)
        for ties in ("optimistic", "mean", "pessimistic"):
            for ks in ((1, 3, 10), (1, 2, 3, 5, 10, 20, 50, 100), ()):
                want = R.metrics(g, e, ks, ties)
                got = metrics.rank_metrics(gd, ed, ks, ties)
                assert got["n"] == want["n"] == int((~drop).sum())
                for k in ks:  # integer count / integer count on both sides
                    assert got[f"hits@{k}"] == want[f"hits_count@{k}"] / want["n"]
                assert abs(got["mrr"] - want["mrr"]) <= 1e-12 * want["mrr"]
                assert abs(got["mean_rank"] - want["mean_rank"]) <= 1e-12 * want["mean_rank"]
                assert metrics.rank_metrics(gd, ed, ks, ties) == got  # the same bits
    minus = torch.full((5,), -1, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="no valid rows"):
        metrics.rank_metrics(minus, minus)
    with pytest.raises(ValueError, match="ties must be"):
        metrics.rank_metrics(minus, minus, ties="best")
    with pytest.raises(ValueError, match="at most 8"):
        metrics.rank_metrics(minus, minus, ks=range(1, 10))


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_graph_capture(cuda, msha, rnd, dt):
    """rank_inner(check=False) and the summary in one captured graph on one stream;
    replayed after the inputs changed in place it equals the eager calls."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import metrics

    rng = np.random.default_rng(13)
    n, B, ks = 1000, 130, [1, 3, 10]
    h = (rnd["h"][:n] - 0.4).to(cuda).to(dt)
    q = (rnd["q"] - 0.4).to(cuda).to(dt)
    target = torch.as_tensor(rng.integers(0, n, B), device=cuda)
    ex = _csr([rng.integers(0, n, 20).tolist() for _ in range(B)], cuda)
    warm = MF.rank_inner(q, h, target, exclude=ex, check=False)  # outside the capture
    metrics.rank_summary(warm[0], warm[1], ks, "mean")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g, e, z = MF.rank_inner(q, h, target, exclude=ex, check=False)
        summ = metrics.rank_summary(g, e, ks, "mean")
    h.copy_((rnd["h"][n:2 * n] - 0.5).to(dt))
    q.copy_((rnd["q"].flip(0) - 0.45).to(dt))
    target.copy_(torch.as_tensor(rng.integers(0, n, B)))
    target[17] = n + 5  # a row without a rank
    graph.replay()
    torch.cuda.synchronize()
    eg, ee, ez = MF.rank_inner(q, h, target, exclude=ex, check=False)
    assert torch.equal(g, eg) and torch.equal(e, ee)
    assert torch.equal(z.view(torch.int32), ez.view(torch.int32))
    assert int(g[17]) == -1
    assert torch.equal(summ, metrics.rank_summary(eg, ee, ks, "mean"))
    want = R.metrics(_np(eg), _np(ee), ks, "mean")
    assert int(summ[3]) == want["n"] == B - 1
