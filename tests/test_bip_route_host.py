"""Host tests (no GPU) of the bipartite attention's route (csrc/bip_route.h through
msha_bip_route): which kernel family msha_bip_attention_fwd / _bwd run -- CSR walk, mask or
MFMA -- at the boundaries of the rule in DESIGN §4.  The expected kinds are written out
here; the query reads only the descriptor's sizes and whether rowmask is set."""
import ctypes

import pytest

NONE, WALK, MASK, MFMA = 0, 1, 2, 3
CUT = 256
F32, BF16 = 0, 1


@pytest.fixture
def cut256(msha):
    from msha_gnn_amd import _lib

    prev = _lib.fn("msha_bip2_bwd_min_rows")(CUT)
    yield
    _lib.fn("msha_bip2_bwd_min_rows")(prev)


def _graph(n, m, edges=None, rowmask=True):
    from msha_gnn_amd import _lib

    g = _lib.MshaGraph()
    g.n_rows, g.n_cols, g.n_edges = n, m, 2 * n if edges is None else edges
    g.rowmask = 0x1000 if rowmask else None  # never dereferenced: only its null-ness is read
    return g


def _route(g, H, F, dtype, slope=0.2, p=0.0, u_lo=False):
    from msha_gnn_amd import _lib

    code = int(_lib.fn("msha_bip_route")(ctypes.byref(g), H, F, dtype, slope, p, int(u_lo)))
    fwd, bwd = code % 16, code // 16
    assert bool(_lib.fn("msha_bip_supported")(ctypes.byref(g), H, F, dtype)) == (code != 0)
    assert (fwd == NONE) == (bwd == NONE)
    return fwd, bwd


def _bwd32(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("MSHA_BIP3_BWD32", raising=False)
    else:
        monkeypatch.setenv("MSHA_BIP3_BWD32", str(value))


def test_abi_version_unchanged(msha):
    from msha_gnn_amd import _lib

    assert _lib.ABI_VERSION == 16 and int(_lib.load().msha_abi_version()) == 16


@pytest.mark.parametrize("bwd32", [None, 0, 1])
def test_2x64_at_the_cut(msha, cut256, monkeypatch, bwd32):
    _bwd32(monkeypatch, bwd32)
    below, at = _graph(CUT - 1, 32), _graph(CUT, 32)
    for dtype in (F32, BF16):
        for p in (0.0, 0.3):
            # below the cut: the mask forward, the CSR-walk backward, whatever the knob
            assert _route(below, 2, 64, dtype, p=p) == (MASK, WALK)
            assert _route(below, 2, 64, dtype, p=p, u_lo=True) == (WALK, WALK)
    # at the cut: MFMA forward; bf16 backward MFMA always
    for p in (0.0, 0.3):
        assert _route(at, 2, 64, BF16, p=p) == (MFMA, MFMA)
        # u_lo moves the forward to the walk and plays no part in the backward
        assert _route(at, 2, 64, BF16, p=p, u_lo=True) == (WALK, MFMA)
    # fp32 backward: forced by 1, refused by 0, unset: MFMA only without dropout
    want = {None: {0.0: MFMA, 0.3: MASK}, 0: {0.0: MASK, 0.3: MASK}, 1: {0.0: MFMA, 0.3: MFMA}}
    for p in (0.0, 0.3):
        assert _route(at, 2, 64, F32, p=p) == (MFMA, want[bwd32][p])
        assert _route(at, 2, 64, F32, p=p, u_lo=True) == (WALK, want[bwd32][p])


@pytest.mark.parametrize("bwd32", [None, 0, 1])
def test_not_maskable_is_the_walk_in_every_setting(msha, cut256, monkeypatch, bwd32):
    _bwd32(monkeypatch, bwd32)
    for n in (CUT - 1, CUT):
        for dtype in (F32, BF16):
            for p in (0.0, 0.3):
                # no row masks
                assert _route(_graph(n, 32, rowmask=False), 2, 64, dtype, p=p) == (WALK, WALK)
                # slope outside [0, 1]
                assert _route(_graph(n, 32), 2, 64, dtype, slope=-0.1, p=p) == (WALK, WALK)
                assert _route(_graph(n, 32), 2, 64, dtype, slope=1.5, p=p) == (WALK, WALK)
                # shapes other than 2 x 64
                assert _route(_graph(n, 8), 8, 16, dtype, p=p) == (WALK, WALK)
                assert _route(_graph(n, 17), 1, 64, dtype, p=p) == (WALK, WALK)
                assert _route(_graph(n, 16), 2, 128, dtype, p=p) == (WALK, WALK)
    # slopes 0 and 1 are inside
    assert _route(_graph(CUT, 32), 2, 64, BF16, slope=0.0) == (MFMA, MFMA)
    assert _route(_graph(CUT, 32), 2, 64, BF16, slope=1.0) == (MFMA, MFMA)


def test_not_covered(msha, cut256):
    for dtype in (F32, BF16):
        assert _route(_graph(CUT, 33), 2, 64, dtype) == (NONE, NONE)      # M > 32
        assert _route(_graph(CUT, 9), 8, 16, dtype) == (NONE, NONE)       # M H > 64
        assert _route(_graph(CUT, 17), 2, 128, dtype) == (NONE, NONE)     # M H F > 4096
        assert _route(_graph(CUT, 32), 2, 16, dtype) == (NONE, NONE)      # H F % 64
        assert _route(_graph(0, 32, edges=0), 2, 64, dtype) == (NONE, NONE)
    assert _route(_graph(CUT, 32), 2, 64, 7) == (NONE, NONE)              # no such dtype
    from msha_gnn_amd import _lib

    assert int(_lib.fn("msha_bip_route")(None, 2, 64, F32, 0.2, 0.0, 0)) == 0


def test_byte_limits(msha, cut256, monkeypatch):
    _bwd32(monkeypatch, None)
    rows = (1 << 31) // (128 * 4)  # n_rows H F 4 = 2^31
    assert _route(_graph(rows - 1, 32, edges=8), 2, 64, F32) == (MFMA, MFMA)
    assert _route(_graph(rows, 32, edges=8), 2, 64, F32) == (NONE, NONE)
    assert _route(_graph(rows, 32, edges=8), 2, 64, BF16) == (NONE, NONE)  # (the same bound)
    rows = (1 << 31) // (256 * 4)
    assert _route(_graph(rows - 1, 16, edges=8), 4, 64, F32) == (WALK, WALK)
    assert _route(_graph(rows, 16, edges=8), 4, 64, F32) == (NONE, NONE)
    edges = (1 << 31) // (2 * 4)   # n_edges H 4 = 2^31
    assert _route(_graph(1000, 32, edges=edges - 1), 2, 64, F32) == (MFMA, MFMA)
    assert _route(_graph(1000, 32, edges=edges), 2, 64, F32) == (NONE, NONE)
