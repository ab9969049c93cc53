"""Host-side checks of the link-prediction training path: the numpy references themselves
(``link_ref``), the ABI's capability / size queries and argument errors (no launch), and
the Python surface's own argument checks."""
import numpy as np
import pytest
import torch

import link_ref as R

F32, BF16 = 0, 1  # MSHA_DTYPE_*


def test_rth_non_edge_matches_brute_force():
    rng = np.random.default_rng(3)
    n_cand = 32
    degs = [0, 1, 7, n_cand - 1, n_cand] + [int(d) for d in rng.integers(0, n_cand + 1, 40)]
    for deg in degs:
        cols = np.sort(rng.choice(n_cand, deg, replace=False))
        cnt = n_cand - deg
        got = [R.rth_non_edge(cols, r) for r in range(cnt)]
        want = [R.rth_non_edge_brute(cols, r, n_cand) for r in range(cnt)]
        assert got == want, (deg, cols)
        assert len(set(got)) == cnt and not (set(got) & set(cols.tolist()))
    # the row's ends: leading and trailing runs of edges
    assert R.rth_non_edge(np.array([0, 1, 2]), 0) == 3
    assert R.rth_non_edge(np.array([29, 30, 31]), 28) == 28


def test_plan_reference_layout():
    n = 6
    #              dup    dup    self   pad(-1) pad(n)  self
    src = np.array([1, 1, 4, 3, -1, 2, 0, 3])
    dst = np.array([2, 2, 4, 3, 5, n, 1, 1])
    P = len(src)
    rowptr, ent = R.plan(src, dst, n)
    assert rowptr.dtype == np.int32 and ent.dtype == np.int32
    assert rowptr.shape == (n + 1,) and ent.shape == (2 * P,)
    assert rowptr[0] == 0 and rowptr[n] == 2 * (P - 2)  # two padding pairs
    assert (ent[rowptr[n]:] == -1).all() and (ent[:rowptr[n]] >= 0).all()
    for r in range(n):
        e = ent[rowptr[r]:rowptr[r + 1]]
        assert (np.diff(e) > 0).all(), r  # ascending: the stable order
        pair, is_src = R.endpoint_pair(e, P)
        assert (np.where(is_src, src[pair], dst[pair]) == r).all()
    assert ent[rowptr[4]:rowptr[5]].tolist() == [2, 2 + P]  # the self pair: twice in its row
    assert ent[rowptr[3]:rowptr[4]].tolist() == [3, 7, 3 + P]
    assert rowptr[5] == rowptr[6]  # row 5: only named by a padding pair
    assert ent[rowptr[1]:rowptr[2]].tolist() == [0, 1, 6 + P, 7 + P]
    listed = set(ent[:rowptr[n]].tolist())
    assert not (listed & {4, 5, 4 + P, 5 + P})  # padding pairs appear in no row


def test_link_queries(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    for feat, dt in [(32, F32), (128, F32), (4, F32), (256, F32), (8, BF16), (128, BF16),
                     (512, BF16)]:
        assert lib.msha_link_bce_supported(feat, dt) == 1, (feat, dt)
    for feat, dt in [(24, F32), (2, F32), (512, F32), (4, BF16), (1024, BF16), (0, F32),
                     (128, 7)]:
        assert lib.msha_link_bce_supported(feat, dt) == 0, (feat, dt)
    chunk = lib.msha_pair_plan_chunk()
    assert chunk > 0
    Ps = [1, 1000, 100_000, 4_000_000]
    for sizes in ([lib.msha_pair_plan_workspace_size(p) for p in Ps],
                  [lib.msha_link_bce_fwd_workspace_size(p) for p in Ps],
                  [lib.msha_link_bce_bwd_workspace_size(p, 128) for p in Ps],
                  [lib.msha_pair_plan_chunk_slots(p) for p in Ps]):
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] < sizes[-1]
    # the sort's double buffers of 4-byte keys and payloads; one partial row per chunk slot
    assert lib.msha_pair_plan_workspace_size(4_000_000) >= 4 * 4 * 2 * 4_000_000
    assert lib.msha_pair_plan_chunk_slots(4_000_000) * chunk >= 2 * 4_000_000
    assert (lib.msha_link_bce_bwd_workspace_size(4_000_000, 128)
            >= 2 * lib.msha_pair_plan_chunk_slots(4_000_000) * 128 * 4)
    assert lib.msha_pair_plan_workspace_size(1 << 30) == 0  # 2P >= 2^31: no such plan


def test_link_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20
    big = 1 << 30  # 2P = 2^31

    def sample(src=p, rowptr=p, k=1, n_cand=32):
        return _lib.call("msha_negative_sample", 10, k, src, 64, n_cand, 100, rowptr, p, None, 0,
                         1, 0, p, p, None)

    with pytest.raises(RuntimeError, match="null pointer"):
        sample(src=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        sample(rowptr=None)
    with pytest.raises(RuntimeError, match="k >= 1"):
        sample(k=0)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        sample(n_cand=1 << 31)

    def plan(P=100, n=50, src=p, rowptr=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_pair_plan", P, n, src, p, rowptr, p, p, ws, ws_bytes, None)

    with pytest.raises(RuntimeError, match="null pointer"):
        plan(src=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        plan(rowptr=None)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        plan(P=big)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        plan(ws_bytes=8)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        plan(ws=p + 4)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        plan(ws=None)

    def fwd(P=100, feat=128, dt=F32, h=p, ld=128, src=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_bce_fwd", P, feat, dt, h, ld, 1000, src, p, p, None, p, p, p,
                         ws, ws_bytes, None)

    def bwd(P=100, feat=128, dt=F32, h=p, ld=128, gloss=p, dH=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_bce_bwd", P, feat, dt, h, ld, 1000, p, p, p, None, p, gloss,
                         p, p, p, dH, ws, ws_bytes, None)

    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(h=None)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(h=p + 4)
        with pytest.raises(RuntimeError, match="16-byte row pitch"):
            call(ld=130)
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            call(P=big)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=24)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=512)  # fp32: past 64 lanes x 16 bytes
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(dt=7)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws_bytes=8)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws=p + 8)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(src=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(gloss=None)
    with pytest.raises(RuntimeError, match="dH must be 16-byte aligned"):
        bwd(dH=p + 4)


def test_link_python_argument_checks(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    idx = torch.zeros(3, dtype=torch.int64)
    y = torch.zeros(3)
    pred = layers.LinkPredictor("mlp", 16, 16, 1, 2, 0.0)
    with pytest.raises(ValueError, match="no scalar to rank by"):
        pred.loss(torch.zeros(4, 16), idx, idx, y)
    # rejected before the library's kernels (or the device) are touched: CPU tensors get here
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        MF.link_bce_loss(torch.zeros(4, 16, dtype=torch.float64), idx, idx, y)
    with pytest.raises(TypeError, match="int64"):
        MF.link_bce_loss(torch.zeros(4, 16), idx.to(torch.int32), idx, y)
    with pytest.raises(ValueError, match="one length"):
        MF.link_bce_loss(torch.zeros(4, 16), idx, idx[:2], y)
    with pytest.raises(ValueError, match="target must be"):
        MF.link_bce_loss(torch.zeros(4, 16), idx, idx, y[:2])
    with pytest.raises(ValueError, match="weight must be"):
        MF.link_bce_loss(torch.zeros(4, 16), idx, idx, y, weight=torch.zeros(3, 1))
    with pytest.raises(ValueError, match="not supported"):
        MF.link_bce_loss(torch.zeros(4, 24), idx, idx, y)
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.link_bce_loss(torch.zeros(4, 16), idx, idx, y)
    with pytest.raises(TypeError, match="int64"):
        MF.pair_plan(idx.to(torch.int32), idx, 4)
    with pytest.raises(ValueError, match="n must be in"):
        MF.pair_plan(idx, idx, 0)
    with pytest.raises(ValueError, match="k must be at least 1"):
        MF.sample_negatives((torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)),
                            idx, k=0, n_cand=4)
