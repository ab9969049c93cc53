"""Host-side checks of the filtered link ranks: the ABI's capability / size queries and
argument errors (no launch), the Python surface's own argument checks, the numpy reference
against a brute-force sort, the bracket guard of the random-float GPU test, and
``sharding.rank_sharded`` over gloo with a torch-CPU ``rank_fn`` that implements
``functional.rank_inner``'s contract."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

import rank_ref as R

F32, BF16 = 0, 1  # MSHA_DTYPE_*


def test_rank_inner_supported(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    for feat, dt in [(128, F32), (16, BF16), (256, F32), (48, BF16)]:
        assert lib.msha_rank_inner_supported(feat, dt) == 1, (feat, dt)
    for feat, dt in [(24, F32), (0, F32), (272, BF16), (512, F32), (128, 7)]:
        assert lib.msha_rank_inner_supported(feat, dt) == 0, (feat, dt)


def test_rank_workspace_and_splits(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    sizes = [lib.msha_rank_inner_workspace_size(512, 100_000, s) for s in (1, 2, 8, 32)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[3] >= 512 * 32 * 2 * 4  # (splits, n_q, 2) uint32 partial counts
    for dt in (F32, BF16):
        for n_q in (1, 512, 4096):
            s = lib.msha_rank_inner_splits(n_q, 100_000, 128, dt)
            assert s >= 1
            # the default-split workspace covers either dtype's default
            assert (lib.msha_rank_inner_workspace_size(n_q, 100_000, 0)
                    >= lib.msha_rank_inner_workspace_size(n_q, 100_000, s))
        assert lib.msha_rank_inner_splits(1, 100_000, 128, dt) > 1  # a small batch is split
        assert lib.msha_rank_inner_splits(1 << 20, 100_000, 128, dt) == 1
        assert lib.msha_rank_inner_splits(512, 0, 128, dt) == 1
        assert lib.msha_rank_inner_splits(512, 100, 128, dt) == 1  # under 512 candidates
    assert lib.msha_rank_inner_splits(512, 100_000, 24, F32) == 1
    small, big = (lib.msha_rank_summary_workspace_size(n) for n in (10, 10_000_000))
    assert 0 < small <= big


def test_rank_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20

    def inner(Q=p, ldq=128, ws=p, ws_bytes=1 << 30, rowptr=None, col=None, feat=128, splits=4,
              target=p, dtype=F32, T=p):
        return _lib.call("msha_rank_inner", 64, feat, dtype, Q, ldq, None, 100, T, 128, 100_000,
                         0, target, None, rowptr, col, splits, p, p, None, None, ws, ws_bytes,
                         None)

    with pytest.raises(RuntimeError, match="null pointer"):
        inner(Q=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        inner(target=None)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        inner(feat=24)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        inner(feat=272)
    with pytest.raises(RuntimeError, match="dtype must be"):
        inner(dtype=7)
    with pytest.raises(RuntimeError, match="go together"):
        inner(rowptr=p)
    with pytest.raises(RuntimeError, match="go together"):
        inner(col=p)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        inner(Q=p + 4)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        inner(T=p + 8)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        inner(ldq=130)
    with pytest.raises(RuntimeError, match="workspace too small"):
        inner(ws_bytes=8)
    with pytest.raises(RuntimeError, match="workspace too small"):
        inner(ws=None)
    with pytest.raises(RuntimeError, match=r"splits must be in"):
        inner(splits=-1)

    ks = (torch.tensor([1, 3, 10], dtype=torch.int64)).numpy()

    def summary(n=100, ties=1, nk=3, ws_bytes=1 << 20, kptr=ks.ctypes.data, out=p):
        return _lib.call("msha_rank_summary", n, p, p, ties, kptr, nk, out, p, p, ws_bytes, None)

    with pytest.raises(RuntimeError, match="ties must be"):
        summary(ties=3)
    with pytest.raises(RuntimeError, match="at most 8"):
        summary(nk=9)
    with pytest.raises(RuntimeError, match="null pointer"):
        summary(out=None)
    with pytest.raises(RuntimeError, match="workspace too small"):
        summary(ws_bytes=8)
    bad = np.asarray([1, 0, 10], np.int64)
    with pytest.raises(RuntimeError, match="k must be >= 1"):
        summary(kptr=bad.ctypes.data)


def test_rank_python_argument_checks(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers, metrics

    pred = layers.LinkPredictor("mlp", 16, 16, 1, 2, 0.0)
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="no scalar to rank by"):
        pred.rank(torch.zeros(4, 16), idx, idx)
    # rejected before the library (or the device) is touched: CPU tensors get this far
    tgt = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError, match="share a dtype"):
        MF.rank_inner(torch.zeros(4, 16), torch.zeros(9, 16, dtype=torch.bfloat16), tgt)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        MF.rank_inner(torch.zeros(4, 16, dtype=torch.float64),
                      torch.zeros(9, 16, dtype=torch.float64), tgt)
    with pytest.raises(ValueError, match="one feature width"):
        MF.rank_inner(torch.zeros(4, 16), torch.zeros(9, 32), tgt)
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.rank_inner(torch.zeros(4, 16), torch.zeros(9, 16), tgt)
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.rank_metrics(tgt, tgt)


def test_dropin_link_predictor_has_rank(msha):
    import importlib
    import sys

    d = os.path.join(ROOT, "msha--gnn_amd", "dropin")
    sys.path.insert(0, d)
    try:
        LLP = importlib.import_module("LLP")
    finally:
        sys.path.remove(d)
    assert callable(LLP.LinkPredictor.rank) and callable(LLP.Teacher_LinkPredictor.rank)
    pred = LLP.LinkPredictor("mlp", 16, 16, 1, 2, 0.0)
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="needs the 'inner' predictor"):
        pred.rank(torch.zeros(4, 16), idx, idx)


def test_rank_ref_matches_brute_force():
    rng = np.random.default_rng(3)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 2.0]
    for trial in range(40):
        n = int(rng.integers(1, 12))
        vals = rng.choice(special, n) if trial % 2 else rng.integers(-2, 3, n).astype(np.float64)
        for t in range(n):
            g, e = R.counts(vals[None, :], [t])
            assert (int(g[0]), int(e[0])) == R.brute_counts(vals, t), (vals, t)
    # spelled out: +inf on top, NaNs tie among themselves at the bottom, the zeros tie
    v = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 5.0])
    want = {0: (5, 1), 1: (0, 0), 2: (4, 0), 3: (2, 1), 4: (2, 1), 5: (5, 1), 6: (1, 0)}
    for t, ge in want.items():
        g, e = R.counts(v[None, :], [t])
        assert (int(g[0]), int(e[0])) == ge, t
    # exclusion, col_offset and an external logit
    L = np.asarray([[3.0, 1.0, 2.0, 2.0, 5.0]])
    assert [int(x[0]) for x in R.counts(L, [2])] == [2, 1]
    assert [int(x[0]) for x in R.counts(L, [2], exclude=[[4, 3, 2]])] == [1, 0]
    assert [int(x[0]) for x in R.counts(L, [102], col_offset=100)] == [2, 1]
    assert [int(x[0]) for x in R.counts(L, [7], col_offset=100)] == [-1, -1]
    assert [int(x[0]) for x in R.counts(L, [7], col_offset=100, target_logit=[2.0])] == [2, 2]
    # ranks and metrics: greater 2, equal 1 -> rank 3 / 3.5 / 4
    assert [int(R.rank2([2], [1], t)[0]) for t in ("optimistic", "mean", "pessimistic")] == [6, 7, 8]
    m = R.metrics([0, 2, -1, 9], [0, 1, -1, 0], ks=(1, 3, 10), ties="mean")
    assert m["n"] == 3 and m["hits@1"] == 1 / 3 and m["hits@3"] == 1 / 3 and m["hits@10"] == 1.0
    assert m["mean_rank"] == (1 + 3.5 + 10) / 3
    assert abs(m["mrr"] - (1 + 1 / 3.5 + 0.1) / 3) < 1e-15
    with pytest.raises(ValueError):
        R.metrics([-1], [-1])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_random_float_brackets_are_tight(dt):
    """The guard of test_gpu_rank's random-float test: the error brackets of its inputs
    leave at most 13 of the 130 queries undecided, none by more than one place, and a plain
    fp32 numpy product lies inside every bracket."""
    p = R.random_problem(dt)
    lo, hi = R.bracket(p["qd"], p["hd"], p["target"])
    width = hi - lo
    print(f"{dt}: {(width > 0).sum()} undecided queries, widest {width.max()}")
    assert (width >= 0).all()
    assert (width > 0).sum() <= 13
    assert width.max() <= 1
    z32 = p["qd"].astype(np.float32) @ p["hd"].astype(np.float32).T
    g, e = R.counts(z32, p["target"])
    assert (g >= lo).all() and (g + e <= hi).all()


# ------------------------------------------------------------ rank_sharded over gloo ---

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem():
    rng = np.random.default_rng(11)
    n, F, B = 1001, 16, 37  # ragged: n not divisible by the world
    h = rng.integers(-3, 4, (n, F)).astype(np.float32)  # integers: exact sums, many ties
    q = rng.integers(-3, 4, (B, F)).astype(np.float32)
    logits = q.astype(np.float64) @ h.astype(np.float64).T
    target = rng.integers(0, n, B)
    target[:6] = [0, 333, 334, 500, 501, 1000]  # the shard edges of world 2 and 3
    best = [np.argsort(-logits[b], kind="stable")[:5].tolist() for b in range(B)]
    excl = [None] * B
    # lists that straddle the shard boundaries, take out strong candidates and, for query
    # 5, name the target itself
    excl[3] = list(range(495, 510)) + best[3]
    excl[5] = list(range(330, 340)) + list(range(660, 675)) + best[5] + [int(target[5])]
    excl[9] = best[9]
    return n, F, B, h, q, logits, target, excl


def _cpu_rank_fn(calls=None):
    """functional.rank_inner's contract (check=False) in numpy on CPU tensors."""
    def rank_fn(qq, local, target, ex_local, off, target_logit):
        lg = qq.numpy().astype(np.float64) @ local.numpy().astype(np.float64).T
        lists = None
        if ex_local is not None:
            rp, cl = ex_local[0].numpy(), ex_local[1].numpy()
            assert ((cl >= 0) & (cl < local.shape[0])).all()  # renumbered, own range only
            lists = [cl[rp[b]:rp[b + 1]] for b in range(lg.shape[0])]
        tl = None if target_logit is None else target_logit.numpy()
        g, e = R.counts(lg, target.numpy(), lists, off, tl)
        t = target.numpy() - off
        ok = (t >= 0) & (t < local.shape[0])
        z = np.full(lg.shape[0], np.nan, np.float32)
        z[ok] = lg[np.arange(lg.shape[0])[ok], t[ok]]
        if tl is not None:
            z = tl.astype(np.float32)
        if calls is not None:
            calls.append((tuple(local.shape), ex_local, off, target_logit))
        return torch.as_tensor(g), torch.as_tensor(e), torch.as_tensor(z)
    return rank_fn


def _worker(rank, world, port, out):
    import sys

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import msha_loader

        msha_loader.load()
        from msha_gnn_amd import functional as MF
        from msha_gnn_amd import sharding

        n, F, B, h, q, logits, target, excl = _problem()
        tab = sharding.ShardedTable(n, F, world, rank, "cpu")
        lo, hi = sharding.row_range(n, world, rank)
        tab.set_local(torch.as_tensor(h[lo:hi]))
        assert tab.path() == "gloo"
        full_before = tab.full.fill_(-7.0).clone()  # a sentinel no gather may overwrite
        qpos = np.concatenate([np.full(len(e), b) for b, e in enumerate(excl) if e])
        cols = np.concatenate([np.asarray(e) for e in excl if e])
        ex = MF.exclude_from_pairs(torch.as_tensor(qpos), torch.as_tensor(cols), B)
        tgt = torch.as_tensor(target)
        ok = True
        for exclude, lists in ((None, None), (ex, excl)):
            want_g, want_e = R.counts(logits, target, lists)
            g, e, z = sharding.rank_sharded(tab, torch.as_tensor(q), tgt, _cpu_rank_fn(),
                                            exclude=exclude)
            ok = ok and g.dtype == torch.int64 and e.dtype == torch.int64
            ok = ok and np.array_equal(g.numpy(), want_g) and np.array_equal(e.numpy(), want_e)
            ok = ok and np.array_equal(z.numpy().astype(np.float64),
                                       logits[np.arange(B), target])
        ok = ok and (want_g >= 0).all()
        ok = ok and torch.equal(tab.full, full_before)  # the table was never gathered
        # targets on other ranks exist for this rank
        ok = ok and bool(((target < lo) | (target >= hi)).any())
        out.put((rank, bool(ok)))
    except Exception as e:  # report instead of hanging the parent
        out.put((rank, f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_rank_sharded_gloo(world):
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(out.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert all(res[r] is True for r in range(world)), res


def test_rank_sharded_without_group_is_the_local_call(msha):
    from msha_gnn_amd import sharding

    n, F, B, h, q, logits, target, _ = _problem()
    tab = sharding.ShardedTable(n, F, 1, 0, "cpu")
    tab.set_local(torch.as_tensor(h))
    assert tab.path() == "copy"
    calls = []
    g, e, z = sharding.rank_sharded(tab, torch.as_tensor(q), torch.as_tensor(target),
                                    _cpu_rank_fn(calls))
    assert calls == [((n, F), None, 0, None)]
    want_g, want_e = R.counts(logits, target)
    assert np.array_equal(g.numpy(), want_g) and np.array_equal(e.numpy(), want_e)
