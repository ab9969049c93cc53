"""The tables of tests/resident_ref.py hold what the GPU sweep of the resident-W kernels
(tests/test_gpu_resident_exact.py) relies on (CPU only):

* the instance tables enumerate proj_kernel 54, pair_kernel + pair_x3_kernel 4 + 4,
  pair_bf16_kernel 8 and dx_kernel 4 times;
* every product, partial sum, score dot and gradient element is an integer whose sum of
  absolute terms stays below 2^24, so fp32 accumulation is exact in any order;
* bf16 tables: every operand and every hadamard product is an exact bf16 value, while a
  bf16 h is NOT representable (|h| reaches the thousands) and the reference rounds it once;
* the data is not degenerate: a swap of two k or n positions of W, or of two heads, changes
  the fp64 reference;
* the row counts produce the item schedules their names promise.
"""
import itertools

import numpy as np
import pytest

import resident_ref as R
from gemm_ref import EXACT


def test_instance_counts():
    assert len(R.PROJ_INSTANCES) == len(set(R.PROJ_INSTANCES)) == 54
    kinds = [k for _, _, k in R.PAIR_INSTANCES]
    assert (kinds.count("pair"), kinds.count("pair_x3")) == (4, 4)
    assert len(set(R.PAIR_INSTANCES)) == 8
    assert len(R.PAIR_BF16_INSTANCES) == len(set(R.PAIR_BF16_INSTANCES)) == 8
    assert len(R.DX_INSTANCES) == len(set(R.DX_INSTANCES)) == 4
    # the shape rule itself: FE = N appears once (N = 64: FE 64 is the one head)
    assert R.fes(128) == [0, 16, 32, 64, 128] and R.fes(64) == [0, 16, 32, 64]


def test_tables_reach_every_instance():
    """Host side of the GPU coverage test: the forward cases name every (K, N, FE, form),
    the backward cases every dx (K, N) at every feat dividing K, the pair cases every
    (K, N) in both forms and both output types."""
    form = {("f32", R.RESIDENT): "f32", ("f32", R.SPLIT): "split", ("bf16", R.RESIDENT): "bf16"}
    seen = {(c["K"], c["N"], c["FE"], form[c["dt"], c["route"]]) for c in R.PROJ_FWD_CASES}
    assert seen == set(R.PROJ_INSTANCES)
    assert {(c["N"], c["K"]) for c in R.PROJ_BWD_CASES} == set(R.DX_INSTANCES)
    for M in R.SIZES:
        got = {(c["N"], c["K"], c["feat"]) for c in R.PROJ_BWD_CASES if c["M"] == M}
        assert got == {(n, k, f) for n in R.KS for k in R.KS for f in (16, 32, 64, 128)
                       if n % f == 0}
        assert {c["scores"] for c in R.PROJ_BWD_CASES if c["M"] == M} == {"both", "al", "ar"}
    kern = {"window": "pair_x3", "plain": "pair"}
    assert {(c["K"], c["N"], kern[c["form"]]) for c in R.PAIR_CASES} == set(R.PAIR_INSTANCES)
    assert {(c["K"], c["N"], c["out"]) for c in R.PAIR_BF16_CASES} == set(R.PAIR_BF16_INSTANCES)
    for K, N in itertools.product(R.KS, R.KS):
        for sc in ("al", "ar", "both", "none"):
            for dt in ("f32", "bf16"):
                assert any(c["scores"] == sc and c["dt"] == dt and (c["K"], c["N"]) == (K, N)
                           for c in R.PROJ_FWD_CASES), (K, N, sc, dt)
    names = [c["name"] for c in R.PROJ_FWD_CASES + R.PROJ_BWD_CASES + R.PAIR_CASES
             + R.PAIR_BF16_CASES]
    assert len(names) == len(set(names))


def test_schedules():
    """With 8 waves (every exact-fp32 and bf16 instance) the three row counts are the
    whole-tile item, tail parts only (an item-less wave with PT = 1, several items per wave
    with PT = 4) and a round followed by a ragged 2-tile tail; 65,549 rows are a round and
    a long tail at 8 or 12 waves.  A wave with no item at all needs PT = 1: with R = 0 the
    grid has fewer than tiles + waves waves, and PT tiles >= 2 tiles >= tiles + 64."""
    for pt in (1, 2, 4):
        assert R.schedule(1024, 8, pt) == (1, 0, {"whole"})
        r, tail, kinds = R.schedule(1045, 8, pt)
        assert (r, tail) == (0, 66) and "tail" in kinds
        assert ("no-item" in kinds) == (pt == 1)
        r, tail, kinds = R.schedule(32789, 8, pt)
        assert (r, tail) == (1, 2) and kinds == {"rounds+tail", "idle"}
    assert R.schedule(R.SPLIT_M, 12, 4)[:2] == (1, 1025)
    assert R.schedule(R.SPLIT_M, 8, 4)[:2] == (2, 1)
    assert 1045 % 16 == 5 and 32789 % 16 == 5 and R.SPLIT_M % 16 == 13
    assert R.SPLIT_M > R.SPLIT_MIN_ROWS > R.SIZES[-1]


def _is_bf16(x):
    return np.array_equal(R.bf16_round(x), x)


def test_operands_are_small_integers():
    for K in R.KS:
        X = R.proj_X(R.SPLIT_M, K)
        assert np.array_equal(X, np.rint(X)) and np.abs(X).max() == R.BOUND and _is_bf16(X)
        # the smaller tables are what their names say, not slices of one another
        assert R.proj_X(1024, K).shape == (1024, K)
        for N in R.KS:
            W = R.proj_W(K, N)
            assert np.array_equal(W, np.rint(W)) and np.abs(W).max() == R.BOUND and _is_bf16(W)


@pytest.mark.parametrize("K,N", list(itertools.product(R.KS, R.KS)))
def test_projection_sums_are_exact(K, N):
    """Forward at the largest row count (integers: max |h| over 65,549 rows bounds the
    smaller tables' too, same generator bound), backward at 32,789 rows, per feat."""
    for M in (R.SIZES[-1], R.SPLIT_M):
        habs = np.abs(R.proj_X(M, K)) @ np.abs(R.proj_W(K, N))
        assert habs.max() * 2 * N < EXACT       # any score dot: |a| <= 2 over <= N columns
    for feat in (16, 32, 64, 128):
        if N % feat == 0:
            worst = R.proj_abs_max(K, N, N // feat, feat)
            assert worst < EXACT, (K, N, feat, worst)


@pytest.mark.parametrize("K,N", list(itertools.product(R.KS, R.KS)))
def test_bf16_h_is_rounded_and_its_dots_exact(K, N):
    h = R.proj_h(R.SIZES[-1], K, N)
    hb = R.bf16_round(h)
    # integers are exact bf16 values up to 256: |h| is far past that (thousands at K = 128)
    assert np.abs(h).max() >= (1000 if K == 128 else 512)
    assert not np.array_equal(hb, h)            # the rounding is exercised ...
    assert np.mean(hb != h) > 0.05
    assert np.array_equal(hb, np.rint(hb))      # ... and leaves integers
    assert np.abs(hb).max() * 2 * N < EXACT


@pytest.mark.parametrize("K,N", list(itertools.product(R.KS, R.KS)))
def test_w_is_not_degenerate(K, N):
    W = R.proj_W(K, N)
    assert len({tuple(r) for r in W}) == K          # rows pairwise distinct
    assert len({tuple(c) for c in W.T}) == N        # columns pairwise distinct
    X = R.proj_X(1045, K)
    h = X @ W
    rng = np.random.default_rng(K * 1000 + N)
    for _ in range(8):
        i, j = rng.choice(K, 2, replace=False)
        Ws = W.copy()
        Ws[[i, j]] = Ws[[j, i]]
        assert not np.array_equal(X @ Ws, h), ("k swap", i, j)
        i, j = rng.choice(N, 2, replace=False)
        Ws = W.copy()
        Ws[:, [i, j]] = Ws[:, [j, i]]
        assert not np.array_equal(X @ Ws, h), ("n swap", i, j)
    # the pair scorer's weight (N, K) and tables
    d = R.pair_arrays(K, N, 1045)
    assert len({tuple(r) for r in d["W"]}) == N and len({tuple(c) for c in d["W"].T}) == K
    assert len({tuple(r) for r in d["A"]}) == R.ROWS_A and len({tuple(r) for r in d["B"]}) == R.ROWS_B


@pytest.mark.parametrize("N", R.KS)
def test_score_vectors_are_not_degenerate(N):
    h = R.proj_h(1045, 64, N)
    for feat in (16, 32, 64, 128):
        if N % feat:
            continue
        H = N // feat
        for which in ("al", "ar"):
            a = R.score_vec(which, N, H, feat)
            assert a.shape == (H, feat) and np.all(a != 0) and np.abs(a).max() <= 2
            assert len({tuple(r) for r in a}) == H      # no two heads share a slice
            ref = R.head_dots(h, a)
            for i, j in itertools.combinations(range(H), 2):
                sw = a.copy()
                sw[[i, j]] = sw[[j, i]]
                assert not np.array_equal(R.head_dots(h, sw), ref), (which, feat, i, j)
        assert not np.array_equal(R.score_vec("al", N, H, feat), R.score_vec("ar", N, H, feat))


@pytest.mark.parametrize("K,N", list(itertools.product(R.KS, R.KS)))
def test_pair_tables(K, N):
    for P in R.PAIR_SIZES:
        d = R.pair_arrays(K, N, P)
        for k in ("A", "B", "W", "b"):
            assert np.array_equal(d[k], np.rint(d[k])) and _is_bf16(d[k])
        gi, gj = d["gi"], d["gj"]
        assert gi.min() >= 0 and gi.max() == R.ROWS_A - 1 and gi[P - 1] == R.ROWS_A - 1
        assert gj.min() >= 0 and gj.max() == R.ROWS_B - 1 and gj[P - 1] == R.ROWS_B - 1
        had = d["A"][gi] * d["B"][gj]
        assert _is_bf16(had)                       # every hadamard product an exact bf16
        worst = (np.abs(had) @ np.abs(d["W"].T) + np.abs(d["b"])).max()
        assert 2 * worst < EXACT                   # the dropout scale 1 / (1 - 0.5) = 2 is exact
        z = R.pair_pre(d)
        assert np.array_equal(z, np.rint(z))
        assert 0.2 < np.mean(z > 0) < 0.8          # relu cuts on both sides
        # an index outside a table reads zeros: the pre-activation is the bias
        out = R.pair_pre(d, gi=np.where(np.arange(P) % 2 == 0, R.ROWS_A, -1), gj=gj)
        assert np.array_equal(out, np.broadcast_to(d["b"], out.shape))
    assert R.ROWS_A != R.ROWS_B and 1.0 / (1.0 - R.DROP_P) == 2.0


def test_env_reason(monkeypatch):
    monkeypatch.delenv("MSHA_SKINNY", raising=False)
    monkeypatch.delenv("MSHA_PROJ_SPLIT_MIN_ROWS", raising=False)
    assert R.env_reason() is None
    monkeypatch.setenv("MSHA_SKINNY", "1")
    monkeypatch.setenv("MSHA_PROJ_SPLIT_MIN_ROWS", "65536")
    assert R.env_reason() is None
    monkeypatch.setenv("MSHA_PROJ_SPLIT_MIN_ROWS", "50000")
    assert "MSHA_PROJ_SPLIT_MIN_ROWS" in R.env_reason()
    monkeypatch.setenv("MSHA_SKINNY", "0")
    assert "MSHA_SKINNY" in R.env_reason()


# ------------------------------------------------ the route queries (host-only library calls)
BASE = 1 << 30      # a made-up 16-byte aligned address: the queries dereference nothing


def _proj_route(lib, M, K, H, F, dt="f32", X=BASE, W=BASE, h=BASE, al=BASE, ar=BASE):
    import ctypes

    sched = (ctypes.c_int32 * 3)()
    code = lib.fn("msha_project_scores_route")(M, K, H, F, 0 if dt == "f32" else 1, X, W, al, ar,
                                               h, sched)
    return code, tuple(sched)


def _pt(N, FE, esize):
    """Column parts per tail tile, as csrc/skinny.hip words it: 4, or fewer when a head would
    straddle the parts or a part's staged row would cover fewer than 4 lanes."""
    epl = 16 // esize
    for pt in (4, 2):
        if N // pt >= 4 * epl and (FE == 0 or FE <= N // pt):
            return pt
    return 1


@pytest.fixture()
def lib(msha):
    from msha_gnn_amd import _lib

    if R.env_reason():
        pytest.skip(R.env_reason())
    assert _lib.fn("msha_project_scores_route") is not None
    return _lib


def test_dtype_codes(msha):
    from msha_gnn_amd import functional as MF
    import torch

    assert (MF._code(torch.float32), MF._code(torch.bfloat16)) == (0, 1)


def test_project_route_over_the_table(lib):
    seen = set()
    for c in R.PROJ_FWD_CASES:
        al = BASE if c["scores"] in ("both", "al") else None
        ar = BASE if c["scores"] in ("both", "ar") else None
        code, (waves, pt, sw) = _proj_route(lib, c["M"], c["K"], c["heads"], c["feat"], c["dt"],
                                            al=al, ar=ar)
        assert code == c["route"], c["name"]
        assert waves in (8, 12) and sw in (c["N"], c["N"] // 2), c["name"]
        assert waves == 8 or code == R.SPLIT, c["name"]
        assert pt == _pt(c["N"], c["FE"], 4 if c["dt"] == "f32" else 2), c["name"]
        assert sw == c["N"] or c["FE"] <= sw, c["name"]   # no head straddles the staging halves
        seen.add((c["K"], c["N"], c["FE"], c["dt"], code))
    assert len(seen) == 54


def test_project_route_refusals(lib):
    ok = dict(M=1024, K=128, H=8, F=16)
    assert _proj_route(lib, **ok)[0] == R.RESIDENT
    assert _proj_route(lib, **dict(ok, M=1023)) == (R.TILED, (0, 0, 0))
    assert _proj_route(lib, **dict(ok, M=R.SPLIT_MIN_ROWS - 1))[0] == R.RESIDENT
    assert _proj_route(lib, **dict(ok, M=R.SPLIT_MIN_ROWS))[0] == R.SPLIT
    assert _proj_route(lib, **dict(ok, M=R.SPLIT_MIN_ROWS), dt="bf16")[0] == R.RESIDENT
    for which in ("X", "W", "h"):
        assert _proj_route(lib, **ok, **{which: BASE + 4})[0] == R.TILED, which
    assert _proj_route(lib, 1024, 128, 16, 8)[0] == R.TILED              # fp32 feat 8
    assert _proj_route(lib, 1024, 128, 16, 8, al=None, ar=None)[0] == R.RESIDENT   # no scores
    assert _proj_route(lib, 1024, 128, 16, 8, "bf16")[0] == R.TILED      # FE 8 has no instance
    assert _proj_route(lib, 1024, 128, 32, 4)[0] == R.TILED
    assert _proj_route(lib, 1024, 96, 8, 16)[0] == R.TILED               # K outside the table
    assert _proj_route(lib, 1024, 128, 6, 16)[0] == R.TILED              # N = 96
    # M K sizeof(T) at 2^31: the last covered row count and the first refused
    assert _proj_route(lib, (1 << 22) - 1, 128, 8, 16)[0] == R.SPLIT
    assert _proj_route(lib, 1 << 22, 128, 8, 16)[0] == R.TILED
    assert _proj_route(lib, (1 << 23) - 1, 128, 8, 16, "bf16")[0] == R.RESIDENT
    assert _proj_route(lib, 1 << 23, 128, 8, 16, "bf16")[0] == R.TILED


def _pair_route(lib, P, K, N, G=BASE, ldg=None, G2=BASE + (1 << 20), ldg2=None, rows=(37, 53),
                W=BASE, out=BASE, gi=BASE, gj=BASE):
    return lib.fn("msha_pair_linear_route")(P, K, N, G, K if ldg is None else ldg, gi, G2,
                                            K if ldg2 is None else ldg2, gj, rows[0], rows[1], W,
                                            out)


def test_pair_route(lib):
    for K, N in itertools.product(R.KS, R.KS):
        assert _pair_route(lib, 1024, K, N) == R.SPLIT
        assert _pair_route(lib, 1024, K, N, rows=(0, 0)) == R.RESIDENT
        assert _pair_route(lib, 1024, K, N, rows=(37, 0)) == R.RESIDENT
        assert _pair_route(lib, 1024, K, N, G2=None) == R.SPLIT      # one table gathered twice
        assert _pair_route(lib, 1024, K, N, G2=None, rows=(0, 53)) == R.RESIDENT
        assert _pair_route(lib, 1024, K, N, ldg=K + 4, ldg2=K + 8) == R.SPLIT
        bf = lib.fn("msha_pair_linear_bf16_route")
        assert bf(1024, K, N, BASE, K + 8, BASE, BASE, K + 16, BASE, BASE, BASE) == R.RESIDENT
        assert bf(1024, K, N, BASE, K + 4, BASE, BASE, K, BASE, BASE, BASE) == R.TILED
        assert bf(1023, K, N, BASE, K, BASE, BASE, K, BASE, BASE, BASE) == R.TILED
        assert bf(1024, K, N, BASE, K, None, BASE, K, BASE, BASE, BASE) == R.TILED
        assert bf(1024, K, N, BASE, K, BASE, None, K, BASE, BASE, BASE) == R.RESIDENT
    K = N = 128
    assert _pair_route(lib, 1023, K, N) == R.TILED
    assert _pair_route(lib, 1024, K, N, G=BASE + 4) == R.TILED
    assert _pair_route(lib, 1024, K, N, G2=BASE + 4) == R.TILED
    assert _pair_route(lib, 1024, K, N, W=BASE + 4) == R.TILED
    assert _pair_route(lib, 1024, K, N, out=BASE + 4) == R.TILED
    assert _pair_route(lib, 1024, K, N, ldg=K + 2) == R.TILED
    assert _pair_route(lib, 1024, K, N, ldg2=K + 2) == R.TILED
    assert _pair_route(lib, 1024, K, N, gi=None) == R.TILED
    assert _pair_route(lib, 1024, K, N, gj=None) == R.TILED
    assert _pair_route(lib, 1024, 32, N) == R.TILED
    # the window: tables within 4 GiB and an output below 2^31 bytes
    rows = (1 << 32) // (4 * K)
    assert _pair_route(lib, 1024, K, N, rows=(rows - 1, 53)) == R.SPLIT
    assert _pair_route(lib, 1024, K, N, rows=(rows, 53)) == R.RESIDENT   # 512 bytes below 4 GiB
    assert _pair_route(lib, 1024, K, N, rows=(rows + 1, 53)) == R.RESIDENT
    assert _pair_route(lib, (1 << 22) - 1, K, N) == R.SPLIT
    assert _pair_route(lib, 1 << 22, K, N) == R.RESIDENT
    assert _pair_route(lib, 1 << 31, K, N) == R.TILED


def test_dx_route(lib):
    q = lib.fn("msha_gemm_f32_head_outer_route")

    def dx(M, N, K, H, F, A=BASE, B=BASE, C=BASE, sA=None, sB=None, ldc=None, beta=0.0, operand=0,
           de=BASE, a=BASE, a2=None):
        sA = (K, 1) if sA is None else sA
        sB = (1, K) if sB is None else sB       # W (N, K) row-major seen as B (K, N)
        return q(M, N, K, A, sA[0], sA[1], B, sB[0], sB[1], C, N if ldc is None else ldc, beta,
                 operand, H, F, de, a, a2)

    for K, N in R.DX_INSTANCES:
        for F in (16, 32, 64, 128):
            assert dx(1024, N, K, K // F if K % F == 0 else 1, F) == (
                R.RESIDENT if K % F == 0 else R.TILED), (K, N, F)
    assert dx(1023, 128, 128, 8, 16) == R.TILED
    assert dx(1024, 128, 128, 16, 8) == R.TILED                 # feat 8
    assert dx(1024, 128, 128, 8, 16, A=BASE + 4) == R.TILED
    assert dx(1024, 128, 128, 8, 16, C=BASE + 4) == R.TILED
    assert dx(1024, 128, 128, 8, 16, a=BASE + 4) == R.TILED     # the fused call itself refuses
    assert dx(1024, 128, 128, 8, 16, ldc=132) == R.TILED
    assert dx(1024, 128, 128, 8, 16, beta=1.0) == R.TILED
    assert dx(1024, 128, 128, 8, 16, sB=(128, 1)) == R.TILED    # B n-contiguous: not W^T
    assert dx(1024, 128, 128, 8, 16, operand=1) == R.TILED
    assert dx((1 << 22) - 1, 128, 128, 8, 16) == R.RESIDENT
    assert dx(1 << 22, 128, 128, 8, 16) == R.TILED
