"""fp64 numpy restatement of the representation-matching term (msha_link_match_fwd / _bwd,
LLP.py:34-35 and :237), with the absolute-term sums ``gpu_helpers.bounded_close`` needs.

    loss  = 1 - (1 / P_v) sum_r c_r cos_r
    dH[r] = -(gloss / P_v) c_r (T[r] / (ns_r nt_r) - cos_r h[r] / (ns_r |h[r]|))
    ns = max(|h[r]|, eps), nt = max(|T[r]|, eps), cos = <h[r], T[r]> / (ns nt)

torch clamps the norms in place outside autograd, so the second term keeps d|h| / dh =
h / |h| of the unclamped norm: cos h / ns^2 above eps, 0 for a zero row.

c_r counts the entries equal to r among the valid ones (inside [0, min(n, n_t))), P_v is
their number.  Tables are given as the exact values the device holds (fp32 or bf16 widened
to fp64).
"""
import numpy as np

EPS = 1e-8


def counts(rows, n, n_t):
    """(count (n,) int32, npad): occurrences of every student row among the valid entries."""
    rows = np.asarray(rows, np.int64)
    m = min(n, n_t)
    ok = (rows >= 0) & (rows < m)
    return np.bincount(rows[ok], minlength=n).astype(np.int32), int((~ok).sum())


def forward(h, T, rows):
    """dict(count, npad, pv, cos (NaN where absent), A_cos, coef (n, 2), loss, A_loss):
    A_cos[r] = sum_f |h T| / (ns nt), the absolute terms of row r's cosine; A_loss the
    absolute terms of the loss sum (1 plus every c |cos| / P_v, the cosines' own terms
    inside: c A_cos / P_v)."""
    h = np.asarray(h, np.float64)
    T = np.asarray(T, np.float64)
    n, n_t = h.shape[0], T.shape[0]
    m = min(n, n_t)
    rows = np.arange(m) if rows is None else rows
    c, npad = counts(rows, n, n_t)
    pv = int(c.sum())
    cos = np.full(n, np.nan)
    A_cos = np.zeros(n)
    coef = np.zeros((n, 2))
    on = np.flatnonzero(c > 0)
    hs, ts = h[on], T[on]
    raw = np.sqrt((hs * hs).sum(1))
    ns = np.maximum(raw, EPS)
    nt = np.maximum(np.sqrt((ts * ts).sum(1)), EPS)
    cos[on] = (hs * ts).sum(1) / (ns * nt)
    A_cos[on] = np.abs(hs * ts).sum(1) / (ns * nt)
    if pv > 0:
        coef[on, 0] = c[on] / (pv * ns * nt)
        coef[on, 1] = np.where(raw > 0, c[on] * cos[on] / (pv * ns * np.where(raw > 0, raw, 1)), 0)
        loss = 1.0 - (c[on] * cos[on]).sum() / pv
        A_loss = 1.0 + (c[on] * A_cos[on]).sum() / pv
    else:
        loss, A_loss = 0.0, 0.0
    return dict(count=c, npad=npad, pv=pv, cos=cos, A_cos=A_cos, coef=coef, loss=loss,
                A_loss=A_loss)


def backward(h, T, coef, gloss):
    """(dH (n, F), A (n, F)): dH[r] = -gloss (coef0 T[r] - coef1 h[r]) and its absolute terms
    |gloss| (|coef0 T| + |coef1 h|); rows of T past its end count as absent."""
    h = np.asarray(h, np.float64)
    T = np.asarray(T, np.float64)
    n = h.shape[0]
    Tp = np.zeros_like(h)
    m = min(n, T.shape[0])
    Tp[:m] = T[:m]
    c0, c1 = coef[:, :1], coef[:, 1:]
    return -gloss * (c0 * Tp - c1 * h), abs(gloss) * (np.abs(c0 * Tp) + np.abs(c1 * h))
