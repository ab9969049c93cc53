"""numpy references of the link-prediction training path: the stable incidence plan, the
r-th non-edge map of the negative sampler (and its brute-force restatement), and the fp64
loss and table gradient."""
import numpy as np


# ------------------------------------------------------------------ incidence plan ---

def plan(src, dst, n):
    """(rowptr int32 (n + 1), ent int32 (2P)): endpoint e < P is the src end of pair e,
    e >= P the dst end of pair e - P; row r's endpoints ascending at
    ent[rowptr[r]:rowptr[r + 1]] (a stable sort by row); a pair with either index outside
    [0, n) is in no row and ent past rowptr[n] is -1."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    P = len(src)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    rows = np.concatenate([np.where(ok, src, n), np.where(ok, dst, n)])
    order = np.argsort(rows, kind="stable")
    counts = np.bincount(rows, minlength=n + 1)[:n]
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ent = order.astype(np.int32)
    ent[rowptr[n]:] = -1
    assert len(ent) == 2 * P
    return rowptr, ent


def endpoint_pair(ent, P):
    """(pair, is the src end) of endpoint ids."""
    ent = np.asarray(ent, np.int64)
    return np.where(ent < P, ent, ent - P), ent < P


# ---------------------------------------------------------------- negative sampler ---

def rth_non_edge(cols, r):
    """The r-th (0-based) column not in the ascending list ``cols``: r + t for the smallest
    t in [0, deg] with cols[t] - t > r (cols[deg] = +inf), by binary search."""
    lo, hi = 0, len(cols)
    while lo < hi:
        mid = (lo + hi) // 2
        if int(cols[mid]) - mid > r:
            hi = mid
        else:
            lo = mid + 1
    return r + lo


def rth_non_edge_brute(cols, r, n_cand):
    present = set(int(c) for c in cols)
    return [c for c in range(n_cand) if c not in present][r]


# ------------------------------------------------------------- loss and gradient ---

def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_terms(z, y):
    """l = max(z, 0) - z y + log1p(exp(-|z|)), fp64."""
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) - z * np.asarray(y, np.float64) + np.log1p(np.exp(-np.abs(z)))


def logits(h, src, dst):
    """(z, A_z = sum_f |h_i h_j|) in fp64 for the pairs inside the table; NaN / 0 outside."""
    h = np.asarray(h, np.float64)
    n = h.shape[0]
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    z = np.full(len(src), np.nan)
    A = np.zeros(len(src))
    prod = h[src[ok]] * h[dst[ok]]
    z[ok] = prod.sum(-1)
    A[ok] = np.abs(prod).sum(-1)
    return z, A, ok


def table_grad(h, src, dst, g, extra=None):
    """dH[r] = sum over row r's endpoints of g_p h[other] (fp64), the absolute-term sums
    A[r] = sum |g_p| |h[other]| (with ``extra`` (P,): sum extra_p |h[other]| instead) and the
    endpoint count of each row.  Padding pairs contribute nothing."""
    h = np.asarray(h, np.float64)
    n = h.shape[0]
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    g = np.where(ok, np.asarray(g, np.float64), 0.0)
    a = np.abs(g) if extra is None else np.where(ok, np.asarray(extra, np.float64), 0.0)
    s, d = src[ok], dst[ok]
    dH = np.zeros_like(h)
    A = np.zeros_like(h)
    np.add.at(dH, s, g[ok, None] * h[d])
    np.add.at(dH, d, g[ok, None] * h[s])
    np.add.at(A, s, a[ok, None] * np.abs(h[d]))
    np.add.at(A, d, a[ok, None] * np.abs(h[s]))
    deg = np.bincount(s, minlength=n) + np.bincount(d, minlength=n)
    return dH, A, deg
