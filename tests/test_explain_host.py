"""Host-side checks of the attention explanation: the tests' own restatement
(``explain_ref``) against a brute-force float statement on dense rows, the tie band on the
reference's attention dump (``ours_record.npz``), and the ABI's size queries and argument
errors (no launch)."""
import numpy as np
import pytest

from conftest import golden

import explain_ref as X
import topk_ref


def _brute_ties(row, rtol):
    """Float statement on one dense row without NaN: Explainer.py:25's
    ``argwhere(row == max(row))``, widened by the relative band."""
    row = np.asarray(row, np.float32)
    mx = row.max()
    if rtol == 0 or not np.isfinite(mx):
        return np.nonzero(row == mx)[0]
    thr = np.float32(mx) - np.float32(np.float32(rtol) * np.abs(mx))
    return np.nonzero(row >= thr)[0]


def test_restatement_matches_brute_force_dense():
    rng = np.random.default_rng(3)
    pool = np.array([0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, 0.25, -3.5, np.inf, -np.inf, 1e-30],
                    np.float32)
    for trial in range(40):
        n, m = rng.integers(1, 9), rng.integers(1, 40)
        A = pool[rng.integers(0, len(pool) - (trial % 3 == 0) * 2, (n, m))]
        for rtol in (0.0, 2.0 ** -16, 2.0 ** -22):
            got = X.dense_ties(A, rtol)
            for i in range(n):
                assert np.array_equal(got[i], _brute_ties(A[i], rtol)), (trial, i, rtol)
        for k in (1, 5, 64):
            v, idx = X.dense_topk(A, k)
            for i in range(n):
                o = topk_ref.order(A[i], np.arange(m))[:k]
                assert np.array_equal(idx[i, :len(o)], o) and (idx[i, len(o):] == -1).all()
                # numpy's == : -0.0 equals the +0.0 the image folds it onto
                assert np.array_equal(v[i, :len(o)], A[i, o])
                assert np.isneginf(v[i, len(o):]).all()


def test_restatement_nan_order_and_empty_segments():
    x = np.array([np.nan, -np.inf, np.nan, 2.0, 2.0], np.float32)
    ptr = np.array([0, 0, 3, 5, 5])
    mx, n_tie, tp, ti = X.segment_ties(ptr, x)
    assert np.isneginf(mx[0]) and mx[1] == -np.inf and mx[2] == 2.0 and np.isneginf(mx[3])
    assert n_tie.tolist() == [0, 1, 2, 0] and tp.tolist() == [0, 0, 1, 3, 3]
    assert ti.tolist() == [1, 0, 1]
    v, i = X.segment_topk(ptr, x, 3)
    assert i.tolist() == [[-1] * 3, [1, 0, 2], [0, 1, -1], [-1] * 3]  # NaN below -inf, by id
    mx, n_tie, _, ti = X.segment_ties(np.array([0, 2]), np.array([np.nan, np.nan], np.float32))
    assert np.isnan(mx[0]) and n_tie.tolist() == [2] and ti.tolist() == [0, 1]


def test_reference_dump_has_no_value_in_the_tie_band(msha):
    """On the reference's own dump the tie sets at rtol = 0 and at DEFAULT_RTOL are the
    same for all 64 rows and 29 columns: widening the equality to the band merges no
    near-tie of the reference."""
    from msha_gnn_amd.explain import DEFAULT_RTOL

    assert 0 < DEFAULT_RTOL <= 2e-5
    r = golden("ours_record.npz")
    A = r["rec.coeff12new.1"]
    assert A.shape == (64, 29)
    for rtol in (DEFAULT_RTOL, 2e-5):
        for M in (A, np.ascontiguousarray(A.T)):
            exact, band = X.dense_ties(M, 0.0), X.dense_ties(M, rtol)
            assert len(exact) == M.shape[0]
            for a, b in zip(exact, band):
                assert np.array_equal(a, b)
    cols = X.dense_ties(np.ascontiguousarray(A.T), DEFAULT_RTOL)
    sizes = [len(c) for c in cols]
    assert sum(s > 1 for s in sizes) == 8 and max(sizes) == 4  # the exact ties of the dump
    # the sparse statement over the stored edges gives the dense rows' and columns' sets
    rowptr, col, vals = X.csr_of_dense(A)
    _, _, tp, ti = X.segment_ties(rowptr, vals, col, DEFAULT_RTOL)
    for a, b in zip(X.lists(tp, ti), X.dense_ties(A, DEFAULT_RTOL)):
        assert np.array_equal(a, b)


def test_segment_select_sizes_and_argument_errors(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    lib = _lib.load()
    size = lib.msha_segment_select_workspace_size
    assert size(1000, 50_000, 0, 0) > 0
    assert size(1000, 50_000, 128, 0) > size(1000, 50_000, 1, 0) > size(1000, 50_000, 0, 0)
    assert size(1000, 50_000, 100, 64) > size(1000, 50_000, 100, 4096)  # more chunk lists
    assert size(1000, 50_000, 129, 0) == 0 and size(1000, 50_000, 5, 63) == 0
    assert size(0, 0, 0, 0) > 0
    p = 1 << 20

    def topk(k=5, ptr=p, ws_bytes=1 << 30, chunk=0, vals=p):
        return _lib.call("msha_segment_topk", 10, 100, ptr, vals, 100, 1, 0, None, None, k,
                         chunk, p, p, p, ws_bytes, None)

    def ties(ptr=p, rtol=0.0, out=p, ld=1, off=0, n_vals=100):
        return _lib.call("msha_segment_ties", 10, 100, ptr, p, n_vals, ld, off, None, None,
                         rtol, 0, out, p, p, p, p, 1 << 30, None)

    for k in (0, 129, 200):  # 200: the K of the reference's commented-out variant
        with pytest.raises(RuntimeError, match=r"k must be in \[1, 128\]"):
            topk(k=k)
    with pytest.raises(RuntimeError, match="null ptr"):
        topk(ptr=None)
    with pytest.raises(RuntimeError, match="null vals"):
        topk(vals=None)
    with pytest.raises(RuntimeError, match="workspace too small"):
        topk(ws_bytes=8)
    with pytest.raises(RuntimeError, match="chunk must be"):
        topk(chunk=5000)
    with pytest.raises(RuntimeError, match="null ptr"):
        ties(ptr=None)
    with pytest.raises(RuntimeError, match="null output pointer"):
        ties(out=None)
    with pytest.raises(RuntimeError, match="rtol must be"):
        ties(rtol=-1.0)
    with pytest.raises(RuntimeError, match="off < ld"):
        ties(ld=2, off=2)
    with pytest.raises(RuntimeError, match="a row per slot"):
        ties(n_vals=99)
    # n_seg = 0 launches nothing
    assert _lib.call("msha_segment_ties", 0, 0, p, None, 0, 1, 0, None, None, 0.0, 0, p, p, p,
                     None, p, 1 << 30, None) == 0


def test_segment_python_argument_checks(msha):
    import torch

    from msha_gnn_amd import functional as MF

    ptr = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="int32"):
        MF.segment_ties(ptr.long(), torch.zeros(4))
    with pytest.raises(ValueError, match="k must be in"):
        MF.segment_topk(ptr, torch.zeros(4), 200)
    with pytest.raises(ValueError, match="col"):
        MF.segment_ties(ptr, torch.zeros(4, 2))
