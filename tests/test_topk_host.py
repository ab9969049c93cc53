"""Host-side checks of the top-K link retrieval: the ABI's capability / size queries and
argument errors (no launch), the Python surface's own argument checks, the CSR builder,
and ``sharding.topk_sharded`` over gloo with torch-CPU ranking functions that implement
the library's order (logit descending, index ascending)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

F32, BF16 = 0, 1  # MSHA_DTYPE_*


def test_topk_inner_supported(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    for feat, k, dt in [(128, 50, F32), (16, 1, BF16), (256, 128, F32)]:
        assert lib.msha_topk_inner_supported(feat, k, dt) == 1, (feat, k, dt)
    for feat, k, dt in [(24, 10, F32), (128, 0, F32), (128, 129, F32), (512, 10, F32)]:
        assert lib.msha_topk_inner_supported(feat, k, dt) == 0, (feat, k, dt)
    assert lib.msha_topk_inner_supported(128, 50, 7) == 0


def test_topk_workspace_and_splits(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    sizes = [lib.msha_topk_inner_workspace_size(512, 100_000, 50, s) for s in (1, 2, 8, 32)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # the partial lists of every split fit: (n_q, splits, k) 64-bit keys
    assert sizes[3] >= 512 * 32 * 50 * 8
    assert lib.msha_topk_inner_workspace_size(512, 100_000, 50, 0) > 0
    assert lib.msha_topk_merge_workspace_size(1, 1, 300_001, 50) > 0
    assert (lib.msha_topk_merge_workspace_size(1, 1, 3_000_001, 50)
            > lib.msha_topk_merge_workspace_size(1, 1, 300_001, 50))
    for n_q in (1, 512, 4096):
        assert lib.msha_topk_inner_splits(n_q, 100_000, 128, 50, F32) >= 1
    assert lib.msha_topk_inner_splits(1, 100_000, 128, 50, F32) > 1  # a small batch is split
    assert lib.msha_topk_inner_splits(64 * 256, 100_000, 128, 50, F32) == 1
    assert lib.msha_topk_inner_splits(1 << 20, 100_000, 128, 50, BF16) == 1
    assert lib.msha_topk_inner_splits(512, 0, 128, 50, F32) == 1


def test_topk_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20

    def inner(Q=p, k=50, ws=p, ws_bytes=1 << 30, rowptr=None, col=None, feat=128, splits=4):
        return _lib.call("msha_topk_inner", 64, feat, F32, Q, 128, None, 100, p, 128, 100_000, 0,
                         rowptr, col, k, 0, splits, p, p, None, ws, ws_bytes, None)

    with pytest.raises(RuntimeError, match="null pointer"):
        inner(Q=None)
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 128\]"):
        inner(k=0)
    with pytest.raises(RuntimeError, match="workspace too small"):
        inner(ws_bytes=8)
    with pytest.raises(RuntimeError, match="go together"):
        inner(rowptr=p)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        inner(feat=24)
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 128\]"):
        _lib.call("msha_topk_merge", 1, 1, 100, 129, p, None, 0, p, p, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("msha_topk_merge", 1, 1, 300_001, 50, p, None, 0, p, p, p, 8, None)


def test_topk_python_argument_checks(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    pred = layers.LinkPredictor("mlp", 16, 16, 1, 2, 0.0)
    with pytest.raises(ValueError, match="no scalar to rank by"):
        pred.topk(torch.zeros(4, 16), torch.zeros(2, dtype=torch.int64), 3)
    # rejected before the library (or the device) is touched: CPU tensors get this far
    with pytest.raises(TypeError, match="share a dtype"):
        MF.topk_inner(torch.zeros(4, 16), torch.zeros(9, 16, dtype=torch.bfloat16), 3)
    with pytest.raises(ValueError, match="one feature width"):
        MF.topk_inner(torch.zeros(4, 16), torch.zeros(9, 32), 3)
    with pytest.raises(ValueError, match="k must be in"):
        MF.topk_inner(torch.zeros(4, 16), torch.zeros(9, 16), 0)


def test_dropin_link_predictor_has_topk(msha):
    import importlib
    import sys

    d = os.path.join(ROOT, "msha--gnn_amd", "dropin")
    sys.path.insert(0, d)
    try:
        LLP = importlib.import_module("LLP")
    finally:
        sys.path.remove(d)
    assert callable(LLP.LinkPredictor.topk) and callable(LLP.Teacher_LinkPredictor.topk)


def test_exclude_from_pairs_matches_numpy(msha):
    from msha_gnn_amd import functional as MF

    from topk_ref import exclude_csr

    rng = np.random.default_rng(5)
    n_q = 9
    qpos = rng.integers(0, n_q, 200)
    qpos = qpos[qpos != 4]  # row 4 stays empty
    cols = rng.integers(0, 40, len(qpos))  # 40 columns: duplicates abound
    lists = [[int(c) for q, c in zip(qpos, cols) if q == b] for b in range(n_q)]
    assert any(len(l) != len(set(l)) for l in lists) and lists[4] == []
    rp_ref, col_ref = exclude_csr(lists)
    rp, col = MF.exclude_from_pairs(torch.as_tensor(qpos), torch.as_tensor(cols), n_q)
    assert rp.dtype == torch.int32 and col.dtype == torch.int32
    assert np.array_equal(rp.numpy(), rp_ref) and np.array_equal(col.numpy(), col_ref)
    rp, col = MF.exclude_from_pairs(torch.zeros(0, dtype=torch.int64),
                                    torch.zeros(0, dtype=torch.int64), 3)
    assert rp.tolist() == [0, 0, 0, 0] and col.numel() == 0
    with pytest.raises(IndexError):
        MF.exclude_from_pairs(torch.tensor([3]), torch.tensor([1]), 3)


# ------------------------------------------------------------ topk_sharded over gloo ---

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
    # queries 3 and 5: exclusion lists that straddle the shard boundaries of world 2
    # (501) and world 3 (334, 668), and that take out their best candidates
    best = [np.argsort(-logits[b], kind="stable")[:5].tolist() for b in range(B)]
    excl = [None] * B
    excl[3] = list(range(495, 510)) + best[3]
    excl[5] = list(range(330, 340)) + list(range(660, 675)) + best[5]
    return n, F, B, h, q, logits, excl


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

        import topk_ref as R

        n, F, B, h, q, logits, excl = _problem()
        tab = sharding.ShardedTable(n, F, world, rank, "cpu")
        lo, hi = sharding.row_range(n, world, rank)
        tab.set_local(torch.as_tensor(h[lo:hi]))
        assert tab.path() == "gloo"
        full_before = tab.full.fill_(-7.0).clone()  # a sentinel no gather may overwrite
        qpos = np.concatenate([np.full(len(e), b) for b, e in enumerate(excl) if e])
        cols = np.concatenate([np.asarray(e) for e in excl if e])
        ex = MF.exclude_from_pairs(torch.as_tensor(qpos), torch.as_tensor(cols), B)

        def topk_fn(qq, local, k, ex_local, off):
            lg = qq.numpy().astype(np.float64) @ local.numpy().astype(np.float64).T
            lists = None
            if ex_local is not None:
                rp, cl = ex_local[0].numpy(), ex_local[1].numpy()
                assert ((cl >= 0) & (cl < local.shape[0])).all()  # renumbered, own range only
                lists = [cl[rp[b]:rp[b + 1]] for b in range(lg.shape[0])]
            v, i = R.topk_rows(lg, k, lists, off)
            return torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(i)

        def merge_fn(v, i, k):
            assert v.shape == (B, world, k) and i.shape == (B, world, k)
            mv, mi = R.merge_rows(v.numpy().reshape(B, -1), i.numpy().reshape(B, -1), k)
            return torch.as_tensor(mv, dtype=torch.float32), torch.as_tensor(mi)

        ok = True
        for k in (20, 400):  # 400: more than one shard's rows
            want_v, want_i = R.topk_rows(logits, k, excl)
            got_v, got_i = sharding.topk_sharded(tab, torch.as_tensor(q), k, topk_fn, merge_fn,
                                                 exclude=ex)
            ok = ok and np.array_equal(got_i.numpy(), want_i)
            ok = ok and np.array_equal(got_v.numpy().astype(np.float64), want_v)
            ok = ok and int(got_i.max()) < n  # padding rows of the last shard never appear
            for b in (3, 5):
                ok = ok and not (set(got_i[b].tolist()) & set(excl[b]))
        ok = ok and torch.equal(tab.full, full_before)  # the table was never gathered
        out.put((rank, bool(ok)))
    except Exception as e:  # report instead of hanging the parent
        out.put((rank, f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_topk_sharded_gloo(world):
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


def test_topk_sharded_without_group_is_the_local_call(msha):
    from msha_gnn_amd import sharding

    import topk_ref as R

    n, F, B, h, q, logits, _ = _problem()
    tab = sharding.ShardedTable(n, F, 1, 0, "cpu")
    tab.set_local(torch.as_tensor(h))
    assert tab.path() == "copy"
    calls = []

    def topk_fn(qq, local, k, ex, off):
        calls.append((tuple(local.shape), ex, off))
        v, i = R.topk_rows(qq.numpy().astype(np.float64) @ local.numpy().astype(np.float64).T, k)
        return torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(i)

    def merge_fn(v, i, k):
        assert v.shape == (B, 1, k)
        return v[:, 0], i[:, 0]

    v, i = sharding.topk_sharded(tab, torch.as_tensor(q), 7, topk_fn, merge_fn)
    want_v, want_i = R.topk_rows(logits, 7)
    assert calls == [((n, F), None, 0)]
    assert np.array_equal(i.numpy(), want_i) and np.array_equal(v.numpy(), want_v)
