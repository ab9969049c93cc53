"""Host tests (no GPU) of the column-range cut and the route query of the column pass that
carries the weight gradient (csrc/col_ranges.h through msha_col_ranges and
msha_edge_attention_bwd_fused_wgrad_route)."""
import numpy as np
import pytest


def _cut(colptr, nb):
    from msha_gnn_amd import _lib

    colptr = np.ascontiguousarray(colptr, np.int64)
    out = np.full(nb + 2, -7, np.int32)  # one guard word past the nb + 1 the call writes
    _lib.call("msha_col_ranges", colptr.ctypes.data, len(colptr) - 1, nb, out.ctypes.data)
    assert out[-1] == -7
    return out[:-1].astype(np.int64)


def _degrees(kind, n, rng):
    if kind == "empty":
        return np.zeros(n, np.int64)
    if kind == "uniform":
        return np.full(n, 3, np.int64)
    if kind == "cycle":
        return np.array([(0, 1, 8, 9, 17, 40)[j % 6] for j in range(n)], np.int64)
    if kind == "huge":
        d = np.ones(n, np.int64)
        d[n // 2] = 100000
        return d
    if kind == "half_empty":
        return np.where(np.arange(n) < n // 2, 0, 7).astype(np.int64)
    return rng.integers(0, 41, n)


@pytest.mark.parametrize("kind", ["empty", "uniform", "cycle", "huge", "half_empty", "random"])
@pytest.mark.parametrize("n", [1, 2, 17, 255, 256, 257, 1045, 4099])
def test_cut_covers_every_column_once(msha, kind, n):
    """Ranges are contiguous, cover [0, n) once, are non-empty (nb <= n), and a range whose
    two ends sit where the slot rule puts them holds within one column's degree of
    n_slots / nb slots."""
    rng = np.random.default_rng(n)
    deg = _degrees(kind, n, rng)
    colptr = np.concatenate([[0], np.cumsum(deg)])
    total, maxdeg = int(colptr[-1]), int(deg.max())
    full = min(n, 256)
    for nb in sorted({1, full, max(1, full // 3), max(1, full - 1)}):
        cut = _cut(colptr, nb)
        assert cut[0] == 0 and cut[-1] == n
        assert (np.diff(cut) >= 1).all()
        tgt = (total * np.arange(nb + 1) + nb - 1) // nb
        ruled = np.ones(nb + 1, bool)  # the cut sits at the first column reaching its target
        for b in range(1, nb):
            ruled[b] = colptr[cut[b]] >= tgt[b] and colptr[cut[b] - 1] < tgt[b]
        slots = colptr[cut[1:]] - colptr[cut[:-1]]
        both = ruled[:-1] & ruled[1:]
        assert (np.abs(slots[both] * nb - total) <= (maxdeg + 1) * nb).all()
        if kind in ("uniform", "cycle", "random") and nb * 41 <= n:
            assert both.all()  # no column is heavy enough to push a cut off its rule


def test_cut_refuses_bad_sizes(msha):
    from msha_gnn_amd import _lib

    colptr = np.arange(11, dtype=np.int64)
    out = np.zeros(300, np.int32)
    f = _lib.fn("msha_col_ranges")
    assert f(colptr.ctypes.data, 10, 11, out.ctypes.data) != 0  # more blocks than columns
    assert f(colptr.ctypes.data, 10, 0, out.ctypes.data) != 0
    assert f(None, 10, 4, out.ctypes.data) != 0
    big = np.arange(1001, dtype=np.int64)
    assert f(big.ctypes.data, 1000, 257, out.ctypes.data) != 0  # the reduce reads <= 256 slabs


def test_route_null_graph(msha):
    """A NULL graph answers no (nothing is dereferenced)."""
    from msha_gnn_amd import _lib

    f = _lib.fn("msha_edge_attention_bwd_fused_wgrad_route")
    assert f(None, 8, 16, 0, 128, 128, 1, 1, 4096, 4096, 4096) == 0
