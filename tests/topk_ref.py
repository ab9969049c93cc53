"""The CPU reference of the top-K order, shared by the top-K tests: fp64 logits, then
``np.lexsort`` on (index, -logit) -- logit descending, index ascending, +inf first, NaN
after -inf, filler (-inf / -1) last.  ``torch.topk`` is not used: its tie order is
unspecified."""
import numpy as np


def order(vals, idx):
    """Positions of one candidate row sorted by (NaN last, value descending, index
    ascending).  -0.0 and +0.0 compare equal, as in numpy."""
    vals = np.asarray(vals, np.float64)
    nan = np.isnan(vals)
    neg = np.where(nan, 0.0, -vals)
    return np.lexsort((np.asarray(idx, np.int64), neg, nan))


def topk_rows(logits, k, exclude=None, col_offset=0, fill=-np.inf):
    """Top k of every row of an (B, n) fp64 logit matrix; ``exclude``: per row a collection
    of column numbers never returned (or None).  Returns (B, k) fp64 values and int64
    indices + col_offset, filler ``fill`` / -1."""
    logits = np.asarray(logits, np.float64)
    B, n = logits.shape
    vals = np.full((B, k), fill, np.float64)
    idx = np.full((B, k), -1, np.int64)
    cols = np.arange(n)
    for b in range(B):
        keep = np.ones(n, bool)
        if exclude is not None and exclude[b] is not None and len(exclude[b]):
            keep[np.asarray(sorted(exclude[b]), np.int64)] = False
        c = cols[keep]
        o = order(logits[b, c], c)[:k]
        vals[b, :len(o)] = logits[b, c[o]]
        idx[b, :len(o)] = c[o] + col_offset
    return vals, idx


def merge_rows(vals, idx, k, fill=-np.inf):
    """Top k of every row of (rows, m) candidate lists; ``idx`` None: the position in the
    row; entries with idx < 0 are ignored."""
    vals = np.asarray(vals, np.float64)
    rows, m = vals.shape
    if idx is None:
        idx = np.broadcast_to(np.arange(m, dtype=np.int64), (rows, m))
    idx = np.asarray(idx, np.int64)
    ov = np.full((rows, k), fill, np.float64)
    oi = np.full((rows, k), -1, np.int64)
    for r in range(rows):
        keep = idx[r] >= 0
        v, i = vals[r, keep], idx[r, keep]
        o = order(v, i)[:k]
        ov[r, :len(o)] = v[o]
        oi[r, :len(o)] = i[o]
    return ov, oi


def exclude_csr(lists):
    """(rowptr, col) int32 numpy arrays of per-row exclusion collections (sorted, unique)."""
    rowptr = np.zeros(len(lists) + 1, np.int32)
    cols = []
    for b, l in enumerate(lists):
        u = sorted(set(int(x) for x in (l if l is not None else ())))
        cols.extend(u)
        rowptr[b + 1] = len(cols)
    return rowptr, np.asarray(cols, np.int32)


def hits_at_k(pos, neg, k):
    """OGB Hits@K in numpy: fraction of pos strictly above the k-th largest neg; 1.0 with
    fewer than k negatives; NaN on a non-finite score."""
    pos = np.asarray(pos, np.float64)
    neg = np.asarray(neg, np.float64)
    if not (np.isfinite(pos).all() and np.isfinite(neg).all()):
        return float("nan")
    if len(neg) < k:
        return 1.0
    kth = np.sort(neg)[-k]
    return float((pos > kth).sum() / len(pos))
