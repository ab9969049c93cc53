"""Shared helpers for the GPU parity tests (inputs, oracle adapters)."""
import numpy as np
import pytest
import torch

from oracle import gnn_oracle as O


@pytest.fixture(params=["s3", "fp32"])
def wgrad_kernel(request, msha):
    """Run under each fp32 weight-gradient kernel: split-bf16 in registers (the default)
    and the exact-fp32 MFMA (msha_wgrad_kernel)."""
    from msha_gnn_amd import _lib

    lib = _lib.load()
    prev = lib.msha_wgrad_kernel({"s3": 3, "fp32": 1}[request.param])
    yield request.param
    lib.msha_wgrad_kernel(prev)


def random_counts(rng, n, m, max_deg, empty_rows=(), hot_col=None, full_rows=()):
    c = np.zeros((n, m), np.float32)
    for i in range(n):
        d = int(rng.integers(1, max_deg + 1))
        c[i, rng.choice(m, min(d, m), replace=False)] = rng.integers(1, 4, min(d, m))
    for i in full_rows:
        c[i, :] = 1
    if hot_col is not None:
        c[:, hot_col] = np.maximum(c[:, hot_col], 1)
    for i in empty_rows:
        c[i, :] = 0
    return c


def virtual_csr(counts):
    """Oracle CSR with virtual full rows (what msha_graph_count/fill must produce)."""
    mask = counts > 0
    empty = ~mask.any(axis=1)
    mask = mask.copy()
    mask[empty] = True
    rowptr, col = O.dense_to_csr(mask.astype(np.float32))
    return rowptr, col, empty


def t(x, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev).to(dtype)


def tol_close(a, b, rtol, atol_rel):
    """assert |a-b| <= rtol*|b| + atol_rel*max|b|."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol_rel * scale)


U32 = 2.0 ** -24  # fp32 unit roundoff


STAT_C = 4.0  # standard deviations of the rounding-error random walk allowed


BF16_U = 2.0 ** -8  # bf16 unit roundoff with one extra bit of slack (stored bf16 values)
BF16_STORE = 2.0 ** -9  # one round-to-nearest bf16 storage rounding, relative
# an fp32 value carried as hi + mid bf16 terms (RNE each): |x - hi - mid| <= 2^-18 |x|
BF16_SPLIT2 = 2.0 ** -18


def bounded_close(got, ref, absterms, nterms, rtol, name="", u=U32, store_u=0.0, split_u=0.0,
                  floor=0.0):
    """Sums against an fp64 reference, EVERY element (no fraction clause):

        |got - ref| <= rtol |ref| + store_u |ref| + 4 sqrt(n) u A  (+ split_u A + floor)

    A = the sum of the absolute values of the terms (incl. the magnitudes inside each
    term, e.g. |g| + |D| of a score gradient), n = the number of terms plus the ops
    inside a term and the reduce levels (``nterms``, scalar or per element).  The
    rounding errors of an n-term fp32 sum are a random walk of n steps of at most
    u |partial| each, so 4 sqrt(n) u A is a four-sigma statistical bound (the worst-case
    n u A is ~sqrt(n) times looser: 2e-3 A for the 70k-edge bip1m columns).  A small
    element is held to its own terms, never to the tensor's largest.  ``u``: the unit
    roundoff of the accumulation (fp32 2^-24, also on the bf16 paths: their operands are
    exact bf16 values, fed to the reference as such, and they accumulate in fp32);
    ``store_u``: the result's own storage rounding (a bf16 output: 2^-9, BF16_STORE);
    ``split_u``: a deterministic per-term operand error, bound + split_u A (an fp32 operand
    carried as two bf16 terms on the matrix cores: 2^-18, BF16_SPLIT2; a softmax weight
    whose exp argument is large: ``cond_split_u``); ``floor``: an absolute term (terms that
    underflow to 0 in fp32: COND_FLOOR).
    Returns (max err / bound, fraction within rtol |ref| alone) for reporting."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    A = np.broadcast_to(np.asarray(absterms, np.float64), ref.shape)
    n = np.asarray(nterms, np.float64)
    if n.ndim == 1 and ref.ndim > 1:  # per leading index (row / column)
        n = n.reshape((-1,) + (1,) * (ref.ndim - 1))
    n = np.broadcast_to(n, ref.shape)
    err = np.abs(got - ref)
    bound = ((rtol + store_u) * np.abs(ref) + (STAT_C * np.sqrt(n) * u + split_u) * A + floor
             + 1e-300)
    worst = float((err / bound).max()) if err.size else 0.0
    assert np.all(err <= bound), (
        f"{name}: {int((err > bound).sum())} of {err.size} elements beyond "
        f"rtol|ref| + 4 sqrt(n) u A (worst {worst:.3g}x the bound)")
    inside = float(np.mean(err <= rtol * np.abs(ref))) if err.size else 1.0
    print(f"{name}: worst err / bound {worst:.3g}; {inside:.2%} within rtol |ref| alone")
    return worst, inside


def rel_close(got, ref, rtol, floor, name=""):
    """Elementwise relative check above a stated magnitude floor: every element within
    rtol max(|ref|, floor) -- the floor is an absolute magnitude of the quantity (not a
    fraction of the tensor's largest element)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    bound = rtol * np.maximum(np.abs(ref), floor)
    worst = float((err / bound).max()) if err.size else 0.0
    assert np.all(err <= bound), (f"{name}: {int((err > bound).sum())} of {err.size} elements "
                                  f"beyond {rtol} max(|ref|, {floor}) (worst {worst:.3g}x)")
    return worst


def _row_rms(x):
    """RMS over each row (leading index) of x, broadcast back to x's shape; a 1-D or 0-D x
    is one row."""
    x = np.asarray(x, np.float64)
    if x.ndim <= 1 or x.size == x.shape[0]:  # a vector (also (n, 1)): one row
        return np.full(x.shape, np.sqrt(np.mean(x * x)) if x.size else 0.0)
    r = np.sqrt(np.mean(x.reshape(x.shape[0], -1) ** 2, axis=1))
    return np.broadcast_to(r.reshape((-1,) + (1,) * (x.ndim - 1)), x.shape)


def _row_max(x):
    """max |x| over each row (leading index), broadcast back; a vector: one row."""
    x = np.abs(np.asarray(x, np.float64))
    if x.ndim <= 1 or x.size == x.shape[0]:  # a vector (also (n, 1)): one row
        return np.full(x.shape, x.max() if x.size else 0.0)
    r = x.reshape(x.shape[0], -1).max(axis=1)
    return np.broadcast_to(r.reshape((-1,) + (1,) * (x.ndim - 1)), x.shape)


def ref32_close(got, ref64, ref32, rtol, name="", k=4.0):
    """Against the reference's fp64 run, EVERY element:

        |got - ref64| <= rtol |ref64| + k e_row,

    e_row = the largest |ref32 - ref64| on the element's row: the worst error the
    reference's own fp32 run (the north_star's CPU path, same formulation, parameters
    and LeakyReLU branches) makes on that row.  A cancelled element is held to a few times
    the accuracy fp32 arithmetic reaches on its row, never to a fraction of the tensor's
    largest element (no max|ref| floor, no fraction clause)."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    e = _row_max(np.asarray(ref32, np.float64) - ref64)
    err = np.abs(got - ref64)
    bound = rtol * np.abs(ref64) + k * e + 1e-300
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"{name}: worst err / bound {worst:.3g} (rtol {rtol}, {k} x the row's largest "
          f"fp32-reference error)")
    assert np.all(err <= bound), (
        f"{name}: {int((err > bound).sum())} of {err.size} elements beyond rtol |ref| + "
        f"{k} x the reference's fp32 row error (worst {worst:.3g}x the bound)")
    return worst


def rms_close(got, ref, rtol, name=""):
    """EVERY element within rtol max(|ref|, RMS of its row of ref): relative above the
    row's typical magnitude, absolute at that magnitude below it (a cancelled element's
    error is set by the size of its terms, of the order of its row's typical element);
    no max|ref| floor."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    bound = rtol * np.maximum(np.abs(ref), _row_rms(ref)) + 1e-300
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"{name}: worst err / bound {worst:.3g} (rtol {rtol} of max(|ref|, row RMS))")
    assert np.all(err <= bound), (f"{name}: {int((err > bound).sum())} of {err.size} elements "
                                  f"beyond {rtol} max(|ref|, row RMS) (worst {worst:.3g}x)")
    return worst


def _seg_sum(x, ptr):
    """Sums of x over the contiguous segments [ptr[k], ptr[k+1]) of axis 0 (empty ones 0),
    each segment summed on its own: a difference of running sums would lose a segment of
    tiny terms (underflowing softmax weights) against the total before it."""
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros((len(ptr) - 1,) + x.shape[1:])
    nz = np.flatnonzero(ptr[1:] > ptr[:-1])
    if len(nz):
        out[nz] = np.add.reduceat(x[:ptr[-1]], ptr[nz], axis=0)
    return out


def edge_abs_terms(rowptr, col, fwd, hc, dU, hs=None, dV=None, keep=None, p=0.0, slope=0.2):
    """Absolute-term sums A for ``bounded_close`` of the OursLayer3 core (fp64, from the
    oracle's forward dict: att, attd, pre): per row u (att |hc_j|), d_hs (att |dV_j|),
    d_el; per column v (att |hs_i|), d_hc (att |dU_i|), d_er.  The score gradient
    de = att (keep g - D) lrelu' has A_e = att (keep |g|_abs + |D|_abs) |lrelu'| with
    |g|_abs = sum_f |dU_if hc_jf| + |hs_if dV_jf|, |D|_abs = sum_row attd |g|_abs.
    Also n_row / n_col, the term counts for the bound."""
    rowptr = np.asarray(rowptr, np.int64)
    n = len(rowptr) - 1
    m, H, F = hc.shape
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    c64 = np.asarray(col, np.int64)
    perm = np.argsort(c64, kind="stable")
    nnz = np.bincount(c64, minlength=m)
    colptr = np.concatenate([[0], np.cumsum(nnz)])
    att, attd = fwd["att"].astype(np.float64), fwd["attd"].astype(np.float64)
    kf = np.ones_like(att) if keep is None else keep.astype(np.float64) / (1.0 - p)
    dl = np.where(fwd["pre"] > 0, 1.0, slope)
    out = {k: np.zeros(s) for k, s in (("u", (n, H, F)), ("d_hs", (n, H, F)),
                                         ("v", (m, H, F)), ("d_hc", (m, H, F)),
                                         ("d_el", (n, H)), ("d_er", (m, H)))}
    for h in range(H):
        ah, adu = np.abs(hc[:, h].astype(np.float64)), np.abs(dU[:, h].astype(np.float64))
        w = attd[:, h:h + 1]
        hcj, dui = ah[c64], adu[rows]
        gabs = np.einsum("ef,ef->e", dui, hcj)
        out["u"][:, h] = _seg_sum(w * hcj, rowptr)
        out["d_hc"][:, h] = _seg_sum((w * dui)[perm], colptr)
        del hcj
        if hs is not None:
            ahs = np.abs(hs[:, h].astype(np.float64))
            hsi = ahs[rows]
            out["v"][:, h] = _seg_sum((w * hsi)[perm], colptr)
            if dV is not None:
                dvj = np.abs(dV[:, h].astype(np.float64))[c64]
                gabs += np.einsum("ef,ef->e", hsi, dvj)
                out["d_hs"][:, h] = _seg_sum(w * dvj, rowptr)
                del dvj
            del hsi
        del dui
        dabs = _seg_sum(attd[:, h] * gabs, rowptr)
        T = att[:, h] * (kf[:, h] * gabs + dabs[rows]) * dl[:, h]
        out["d_el"][:, h] = _seg_sum(T, rowptr)
        out["d_er"][:, h] = _seg_sum(T[perm], colptr)
    # terms per output: the outer sum, the 2F-term dots inside g, 16 elementwise ops, and
    # up to 80 levels of the wave / block partial reduce
    k_in = 2 * F + 96
    out["n_row"] = np.diff(rowptr).astype(np.float64) + k_in
    out["n_col"] = nnz.astype(np.float64) + k_in
    return out


# ---------------------------------------------------------------- ill-conditioned scores
COND_C = 8.0  # roundings of a softmax weight's exp argument allowed for (cond_split_u)
COND_FLOOR = 2.0 ** -100
REGIMES = ("shift_up", "shift_down", "ramp_up", "ramp_down", "dominant", "kink")

# (n, m, H, F, max_deg, extra): the smallest graphs that reach every path of the
# edge-softmax family -- G*: the general kernels (rows longer than one wavefront, several
# online chunks; a hot column; QPL > 1), S*: short rows (gather layout), B*: bipartite
COND_CASES = {
    "G1": (150, 80, 1, 8, 80, dict(empty_rows=(0,), full_rows=(2,))),
    "G2": (400, 400, 8, 16, 70, dict(hot_col=9)),
    "G3": (64, 40, 8, 128, 12, dict(empty_rows=(1,))),
    "S1": (400, 32, 2, 64, 12, dict()),
    "S2": (300, 40, 8, 16, 5, dict(empty_rows=(0,))),
    "B1": (700, 32, 2, 64, 32, dict(full_rows=(1, 2, 3, 40), empty_rows=(5,))),
    "B2": (900, 8, 8, 16, 5, dict(empty_rows=(0,))),
}


def score_regimes(rng, n, m, H):
    """Named (el, er) pairs in float32, each from a standard_normal base, that leave the
    few-units-around-0 range every other parity test draws its scores from:

    shift_up    el += 96: exp overflows without the max subtraction (96 > 88.7)
    shift_down  el -= 600: scores near -120 after the 0.2 slope; l underflows to 0 without
                the max subtraction, lse is large and negative
    ramp_up     er[j] += 3 j: CSR columns ascend, so every chunk of a long row raises the
                running max (the rescale of acc, l, lc, uc, qc; alpha underflowing to 0)
    ramp_down   er[j] -= 3 j: later chunks whose weights underflow (alpha == 1, psum == 0)
    dominant    er[5] += 200 on every head: att is exactly 1 on one edge and 0 on the rest
                of the row (ds == 0, no NaN from 0 * inf)
    kink        el, er = rint(base): pre == 0 exactly on many edges (the forward branch and
                lrelu'(0) = slope, the oracle's pre > 0)"""
    el = rng.standard_normal((n, H)).astype(np.float32)
    er = rng.standard_normal((m, H)).astype(np.float32)
    ramp = (3.0 * np.arange(m, dtype=np.float32))[:, None]
    dom = er.copy()
    dom[5] += np.float32(200)
    return {
        "shift_up": (el + np.float32(96), er.copy()),
        "shift_down": (el - np.float32(600), er.copy()),
        "ramp_up": (el.copy(), er + ramp),
        "ramp_down": (el.copy(), er - ramp),
        "dominant": (el.copy(), dom),
        "kink": (np.rint(el), np.rint(er)),
    }


def score_span(rowptr, col, el, er):
    """S of ``cond_split_u``: the largest |el_i + er_j| over the edges plus ln(max degree)
    (|s| <= |pre|, and |lse| <= max |s| + ln(deg))."""
    rowptr = np.asarray(rowptr, np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    pre = np.asarray(el, np.float64)[rows] + np.asarray(er, np.float64)[np.asarray(col, np.int64)]
    return float(np.abs(pre).max() + np.log(np.diff(rowptr).max()))


def cond_split_u(S):
    """``split_u`` of ``bounded_close`` for softmax weights at scores of magnitude up to S:
    COND_C 2^-24 S.  A weight exp(s - lse) inherits, as a relative error, the absolute error
    of its argument: one rounding each of el + er, of the slope multiply, of m + log(l) in
    the forward, of the stored lse, of lse * log2e (or m2) and of the difference (none where
    it is an fma) -- six roundings of at most 2^-24 max(|s|, |lse|) <= 2^-24 S, and two
    spare."""
    return COND_C * U32 * S


def cond_inputs(key, seed=0):
    """One COND_CASES graph with its tables and every score regime (float32), from a fixed
    seed: dict(c, rowptr, col, empty, hc, hs, dU, dV, regimes, shape)."""
    n, m, H, F, max_deg, kw = COND_CASES[key]
    rng = np.random.default_rng(1000 + seed + n + 7 * H + F)
    c = random_counts(rng, n, m, max_deg, **kw)
    rowptr, col, empty = virtual_csr(c)
    tab = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    hc, hs, dU, dV = tab(m, H, F), tab(n, H, F), tab(n, H, F), tab(m, H, F)
    return dict(c=c, rowptr=rowptr, col=col, empty=empty, hc=hc, hs=hs, dU=dU, dV=dV,
                regimes=score_regimes(rng, n, m, H), shape=(n, m, H, F))


COND_NAMES = ("u", "v", "d_el", "d_er", "d_hc", "d_hs")
_COND_PER = {"u": "n_row", "d_hs": "n_row", "d_el": "n_row", "v": "n_col", "d_hc": "n_col",
             "d_er": "n_col"}


def cond_reference(rowptr, col, empty, el, er, hc, dU, hs=None, dV=None, keep=None, p=0.0):
    """The fp64 oracle (forward and backward) on the given stored values, with the absolute
    terms and the score span: (refs by COND_NAMES, A of edge_abs_terms, S, forward dict)."""
    d = lambda x: None if x is None else np.asarray(x, np.float64)  # noqa: E731
    fwd = O.edge_aggregate_fwd(rowptr, col, d(el), d(er), d(hc), hs=d(hs), keep=keep, p=p,
                               rowflag=empty)
    bw = O.edge_aggregate_bwd(rowptr, col, fwd, d(hc), d(dU), hs=d(hs), dV=d(dV), keep=keep, p=p)
    A = edge_abs_terms(rowptr, col, fwd, d(hc), d(dU), hs=d(hs), dV=d(dV), keep=keep, p=p)
    refs = dict(u=fwd["u"], v=fwd["v"], d_el=bw["d_el"], d_er=bw["d_er"], d_hc=bw["d_hc"],
                d_hs=bw["d_hs"])
    return refs, A, score_span(rowptr, col, el, er), fwd


def cond_close(got, refs, A, S, rtol, tag=""):
    """``bounded_close`` of every output in ``got`` (name -> array) at the ill-conditioned
    bound: rtol |ref| + (4 sqrt(n) 2^-24 + cond_split_u(S)) A + COND_FLOOR (a weight below
    2^-126 of its row's largest is 0 in fp32; with |values| <= 2^4 and at most 2^13 terms
    nothing lost that way reaches 2^-100).  Returns the worst error-to-bound ratio."""
    worst = 0.0
    for name, x in got.items():
        w, _ = bounded_close(x, refs[name], A[name], A[_COND_PER[name]], rtol, f"{tag} {name}",
                             split_u=cond_split_u(S), floor=COND_FLOOR)
        worst = max(worst, w)
    return worst
