"""Case tables and integer operands of the exact sweep of the resident-W kernels
(csrc/skinny.hip: proj_kernel, pair_kernel, pair_x3_kernel, pair_bf16_kernel, dx_kernel).

TEST INFRASTRUCTURE ONLY, host-side numpy.  The instance tables are derived from the
documented shape rule (include/msha_gnn.h, msha_*_route): K and N = heads * feat in
{64, 128}; the projection's FE in {0, 16, 32, 64, N} (0: no score vector) in three forms,
exact fp32, split-bf16 (fp32 from 65,536 rows) and bf16.  tests/test_resident_host.py holds
every table to what the GPU test (tests/test_gpu_resident_exact.py) relies on: integers
below 2^24 everywhere, bf16-exact operands and hadamard products, non-degenerate data.

Row counts (``schedule`` below restates the kernels' item schedule: persistent blocks of
WAVES waves, grid = min(ceil(tiles / WAVES), 256), R whole-tile rounds, then the leftover
tiles cut into PT column parts):

  1,024   64 tiles, R = 1, no tail: the whole-tile item
  1,045   66 tiles in 9 blocks, R = 0: every item a column part, several per wave with
          PT > 1, none for some waves with PT = 1; the last tile has 5 rows
  32,789  2,050 tiles on 256 blocks: R = 1, then a 2-tile tail with a ragged end
  65,549  (fp32 only) the smallest ragged size past the split-bf16 cut-over
"""
import functools
import os

import numpy as np

from gemm_ref import EXACT, ints

KS = (128, 64)
SIZES = (1024, 1045, 32789)
SPLIT_MIN_ROWS = 65536      # MSHA_PROJ_SPLIT_MIN_ROWS unset
SPLIT_M = 65549
TILED, RESIDENT, SPLIT = 0, 1, 2   # MSHA_ROUTE_*
GUARD_ROWS = 16             # untouched rows asked for past every output batch
BOUND = 8                   # |x| of X, W, the gathered tables and the pair weight


def env_reason():
    """Why the route-asserting tests cannot run in this environment, or None."""
    v = os.environ.get("MSHA_SKINNY", "")
    if v.strip() and int(v) == 0:
        return "MSHA_SKINNY=0 routes every call to the tiled kernels"
    v = os.environ.get("MSHA_PROJ_SPLIT_MIN_ROWS", "")
    if v.strip() and int(v) != SPLIT_MIN_ROWS:
        return f"MSHA_PROJ_SPLIT_MIN_ROWS={v} moves the split-bf16 cut-over"
    return None


# ------------------------------------------------------------------- instance tables
def fes(N):
    """FE of proj_kernel<T, K, N, FE, SPLIT> for a given N: none, 16, 32, 64, one head."""
    return sorted({0, 16, 32, 64, N})


PROJ_INSTANCES = [(K, N, FE, form) for K in KS for N in KS for FE in fes(N)
                  for form in ("f32", "split", "bf16")]
PAIR_INSTANCES = [(K, N, kern) for K in KS for N in KS for kern in ("pair", "pair_x3")]
PAIR_BF16_INSTANCES = [(K, N, out) for K in KS for N in KS for out in ("f32", "bf16")]
DX_INSTANCES = [(K, N) for K in KS for N in KS]   # K = heads * feat, N = the input width


def schedule(M, waves, pt):
    """The item schedule of a persistent launch over M rows: (R, tail tiles, kinds), kinds a
    set of 'whole' (every item a whole tile), 'tail' (every item a column part), 'rounds+tail',
    'idle' (a tail exists and some wave gets no part of it) and 'no-item' (a wave with no
    item at all: the kernel's n_items == 0 return)."""
    tiles = (M + 15) // 16
    grid = min((tiles + waves - 1) // waves, 256)
    nw = grid * waves
    R = tiles // nw
    tail = tiles - R * nw
    kinds = set()
    if tail == 0:
        kinds.add("whole")
    else:
        kinds.add("tail" if R == 0 else "rounds+tail")
        if pt * tail < nw:
            kinds.add("idle")
            if R == 0:
                kinds.add("no-item")
    return R, tail, kinds


# -------------------------------------------------------------------------- operands
def signs(name, shape):
    """Score vectors: entries in {-2, -1, 1, 2} (no zero entry)."""
    v = ints(name, shape, 2)
    z = ints(name + "z", shape, 1)
    return np.where(v == 0, np.where(z >= 0, 1.0, -1.0), v)


@functools.lru_cache(maxsize=None)
def proj_X(M, K):
    return ints(f"res-X-{K}", (M, K), BOUND)


@functools.lru_cache(maxsize=None)
def proj_W(K, N):
    return ints(f"res-W-{K}x{N}", (K, N), BOUND)


@functools.lru_cache(maxsize=8)
def proj_h(M, K, N):
    return proj_X(M, K) @ proj_W(K, N)


def score_vec(which, N, heads, feat):
    return signs(f"res-{which}-{N}-{heads}x{feat}", (heads, feat))


def bf16_round(x):
    """fp64 -> bf16 (one rounding, torch's round to nearest even) -> fp64."""
    import torch

    return torch.as_tensor(np.asarray(x), dtype=torch.float64).to(torch.bfloat16).double().numpy()


def head_dots(h, a):
    M = h.shape[0]
    H, F = a.shape
    return (h.reshape(M, H, F) * a).sum(-1)


def _heads_feat(N, FE):
    return (N // 16, 16) if FE == 0 else (N // FE, FE)


def _fwd_cases():
    cs = []
    for dt in ("f32", "bf16"):
        for M in SIZES + ((SPLIT_M,) if dt == "f32" else ()):
            route = SPLIT if dt == "f32" and M >= SPLIT_MIN_ROWS else RESIDENT
            for K in KS:
                for N in KS:
                    for FE in fes(N):
                        H, F = _heads_feat(N, FE)
                        opts = ["none"] if FE == 0 else ["both"]
                        if FE == 32 and M != SPLIT_M:   # the one-sided options: one FE per (K, N)
                            opts += ["al", "ar"]
                        for sc in opts:
                            cs.append(dict(name=f"proj-{dt}-M{M}-K{K}-N{N}-fe{FE}-{sc}", dt=dt,
                                           M=M, K=K, N=N, FE=FE, heads=H, feat=F, scores=sc,
                                           route=route))
    return cs


PROJ_FWD_CASES = _fwd_cases()


def proj_fwd_ref(c):
    """X, W, al, ar (None where absent) and the expected h, el, er of a forward case."""
    M, K, N, H, F = c["M"], c["K"], c["N"], c["heads"], c["feat"]
    al = score_vec("al", N, H, F) if c["scores"] in ("both", "al") else None
    ar = score_vec("ar", N, H, F) if c["scores"] in ("both", "ar") else None
    h = proj_h(M, K, N)
    if c["dt"] == "bf16":
        h = bf16_round(h)   # the kernel's contract: the score dots of the STORED row
    return dict(X=proj_X(M, K), W=proj_W(K, N), al=al, ar=ar, h=h,
                el=None if al is None else head_dots(h, al),
                er=None if ar is None else head_dots(h, ar))


# backward through functional.project_scores: N = heads * feat is dx_kernel's K, the input
# width K its N; hF over every feat that divides N
def _bwd_cases():
    cs = []
    for M in SIZES:
        for N in KS:
            for K in KS:
                for F in (16, 32, 64, 128):
                    if N % F:
                        continue
                    for sc in ("both", "al", "ar") if F == 32 else ("both",):
                        cs.append(dict(name=f"bwd-M{M}-K{K}-N{N}-hf{F}-{sc}", M=M, K=K, N=N,
                                       heads=N // F, feat=F, scores=sc))
    return cs


PROJ_BWD_CASES = _bwd_cases()


def proj_bwd_arrays(c):
    """Forward operands and the output gradients dh (|x| <= 2), dl, dr (|x| <= 1)."""
    M, K, N, H, F = c["M"], c["K"], c["N"], c["heads"], c["feat"]
    return dict(X=proj_X(M, K), W=proj_W(K, N), al=score_vec("al", N, H, F),
                ar=score_vec("ar", N, H, F), dh=ints(f"res-dh-{N}", (M, N), 2),
                dl=ints(f"res-dl-{H}", (M, H), 1), dr=ints(f"res-dr-{H}", (M, H), 1))


# ------------------------------------------------------------------------ pair scorer
PAIR_SIZES = (1024, 1045, 4099)
ROWS_A, ROWS_B = 37, 53     # two tables of different row counts
ACT_BIAS, ACT_RELU, ACT_DROPOUT, ACT_SIGMOID = 1, 2, 4, 8
DROP_P, DROP_SEED = 0.5, 20240607


def pair_arrays(K, N, P, bound=BOUND, wbound=BOUND):
    """Tables A (ROWS_A, K), B (ROWS_B, K), the nn.Linear weight (N, K), bias (N,) and the
    int64 gathers gi, gj (P,): random rows, the last row of each table among them, also in
    the ragged last tile."""
    A = ints(f"res-pA-{K}", (ROWS_A, K), bound)
    B = ints(f"res-pB-{K}", (ROWS_B, K), bound)
    W = ints(f"res-pW-{K}x{N}", (N, K), wbound)
    b = ints(f"res-pb-{N}", (N,), wbound)
    gi = ints(f"res-gi-{P}", (P,), ROWS_A).astype(np.int64) % ROWS_A
    gj = ints(f"res-gj-{P}", (P,), ROWS_B).astype(np.int64) % ROWS_B
    gi[0] = gi[P - 1] = ROWS_A - 1
    gj[1] = gj[P - 1] = ROWS_B - 1
    return dict(A=A, B=B, W=W, b=b, gi=gi, gj=gj)


def pair_pre(d, gi=None, gj=None):
    """(x_i * x_j) W^T + b in fp64; rows with an index outside a table read zeros."""
    gi = d["gi"] if gi is None else gi
    gj = d["gj"] if gj is None else gj
    A = np.vstack([d["A"], np.zeros((1, d["A"].shape[1]))])
    B = np.vstack([d["B"], np.zeros((1, d["B"].shape[1]))])
    ia = np.where((gi >= 0) & (gi < ROWS_A), gi, ROWS_A)
    ib = np.where((gj >= 0) & (gj < ROWS_B), gj, ROWS_B)
    return (A[ia] * B[ib]) @ d["W"].T + d["b"]


PAIR_CASES = [dict(name=f"pair-{form}-P{P}-K{K}-N{N}", P=P, K=K, N=N, form=form,
                   route=SPLIT if form == "window" else RESIDENT)
              for form in ("window", "plain") for P in PAIR_SIZES for K in KS for N in KS]
PAIR_BF16_CASES = [dict(name=f"pairbf16-K{K}-N{N}-{out}", P=1045, K=K, N=N, out=out)
                   for K, N, out in PAIR_BF16_INSTANCES]


# --------------------------------------------------------------------------- bounds
def proj_abs_max(K, N, heads, feat, M=SIZES[-1]):
    """The largest sum of absolute terms over the forward and every gradient of a
    projection at M rows, all score terms present (the other options sum fewer terms)."""
    c = dict(M=M, K=K, N=N, heads=heads, feat=feat)
    s = proj_bwd_arrays(c)
    d = {k: np.abs(v) for k, v in s.items()}
    h = d["X"] @ d["W"]
    sc = head_dots(h, d["al"]) + head_dots(h, d["ar"])
    tot = d["dh"] + np.repeat(d["dl"], feat, 1) * d["al"].reshape(-1) \
        + np.repeat(d["dr"], feat, 1) * d["ar"].reshape(-1)
    dX, dW = tot @ d["W"].T, d["X"].T @ tot
    # the score-vector gradients sum d[m, head] h[m, head, f] over the rows, h the STORED
    # forward output (an exact integer): its own magnitude, not the sum behind it
    h3 = np.abs(s["X"] @ s["W"]).reshape(M, heads, feat)
    dal = np.maximum(np.einsum("mh,mhf->hf", d["dl"], h3), np.einsum("mh,mhf->hf", d["dr"], h3))
    # ... or, in the fused weight-gradient pass, (d^T X) W: G = d^T X, then G W
    W3 = d["W"].reshape(K, heads, feat)
    G_abs = np.einsum("mh,mk->hk", d["dl"] + d["dr"], d["X"])
    dal_w = max(np.einsum("hk,khf->hf", np.abs(np.einsum("mh,mk->hk", s[g], s["X"])), W3).max()
                for g in ("dl", "dr"))
    return max([x.max() for x in (h, sc, tot, dX, dW, dal, G_abs)] + [dal_w])


assert EXACT == 2 ** 24
