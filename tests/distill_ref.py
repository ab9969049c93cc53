"""numpy fp64 references of the link-prediction distillation path: the context walk's
transition law, the pinned fp32 decisions of the rank term, the three loss terms and the
logit gradient.  The table gradient is ``link_ref.table_grad`` on the flat pairs."""
import numpy as np


# ------------------------------------------------------------------ context walks ---

def transition(rowptr, col, rowflag=None, n=None):
    """Row-stochastic one-step matrix (n, n) of the sampler's walk in fp64: uniform over a
    row's CSR slots (a duplicate column counts twice); a row that is empty, flagged (a
    virtual full row) or outside the CSR is all zero: the walk stops there."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    rows = len(rowptr) - 1
    n = rows if n is None else n
    P = np.zeros((n, n))
    for i in range(min(rows, n)):
        if rowflag is not None and rowflag[i]:
            continue
        c = col[rowptr[i]:rowptr[i + 1]]
        if len(c):
            np.add.at(P[i], c, 1.0 / len(c))
    return P


def flat_pairs(anchors, context):
    """(src, dst) of the flat pairs (anchors[p // K], context.flat[p])."""
    context = np.asarray(context, np.int64)
    return np.repeat(np.asarray(anchors, np.int64), context.shape[1]), context.reshape(-1)


def valid_slots(anchors, context, n, n_t=None):
    a = np.asarray(anchors, np.int64)[:, None]
    c = np.asarray(context, np.int64)
    lim = n if n_t is None else min(n, n_t)
    return (a >= 0) & (a < lim) & (c >= 0) & (c < lim)


# ------------------------------------------------------------------ pinned decisions ---

def rank_sign(t, margin):
    """r[a, i, j] in {-1, 0, 1} by the kernel's rule, in np.float32: d = fl32(t_i - t_j), one
    subtraction; r = sign(d) where |d| > fl32(margin), one compare, else 0."""
    t32 = np.asarray(t, np.float32)
    d = t32[:, :, None] - t32[:, None, :]
    assert d.dtype == np.float32
    return np.where(np.abs(d) > np.float32(margin), np.sign(d), np.float32(0)).astype(np.float32)


def hinge_active(y, r, margin):
    """The hinge decision by the kernel's rule, in np.float32: fl32(fl32(margin) - r fl32(y_i -
    y_j)) > 0 (r = +-1 or 0, so r times the difference is exact: two roundings in all)."""
    y32 = np.asarray(y, np.float32)
    dy = y32[:, :, None] - y32[:, None, :]
    arg = np.float32(margin) - np.asarray(r, np.float32) * dy
    assert arg.dtype == np.float32
    return arg > 0


# ------------------------------------------------------------------ loss and gradient ---

def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def distill(y, t, valid, margin=0.1, tau=1.0, w=(1.0, 1.0, 0.0), pinned=True):
    """The three terms and the logit gradient in fp64 from logits y, t (A, K) over the valid
    slots.  ``pinned``: the sign r and the hinge decision follow the kernel's fp32 rule
    (``rank_sign``, ``hinge_active``; margin is fl32(margin)); otherwise they are taken in
    fp64.  Returns a dict: LR, LD, LP (per-anchor sums (A,)), terms (3,) = sums / A, loss,
    c (A, K) the integer rank counts, g_rank / g_smooth / g (A, K), r."""
    valid = np.asarray(valid, bool)
    A, K = valid.shape
    y64 = np.where(valid, np.asarray(y, np.float64), 0.0)
    t64 = np.where(valid, np.asarray(t, np.float64), 0.0)
    dy = y64[:, :, None] - y64[:, None, :]
    if pinned:
        m = float(np.float32(margin))
        r = rank_sign(t64, margin).astype(np.float64)
        pos = hinge_active(y64, r, margin)
    else:
        m = float(margin)
        dt = t64[:, :, None] - t64[:, None, :]
        r = np.where(np.abs(dt) > m, np.sign(dt), 0.0)
        pos = (m - r * dy) > 0
    arg = m - r * dy
    pair = valid[:, :, None] & valid[:, None, :] & ~np.eye(K, dtype=bool)[None]
    upper = np.triu(np.ones((K, K), bool), 1)[None]
    l = np.where(pos, np.maximum(arg, 0.0), 0.0)
    LR = (l * (pair & upper)).sum(axis=(1, 2))
    active = pair & (r != 0) & pos
    c = -(r * active).sum(axis=2)
    # distribution term over the valid slots
    has = valid.any(axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        yt = np.where(valid, y64 / tau, -np.inf)
        tt = np.where(valid, t64 / tau, -np.inf)
        my = np.where(has, yt.max(axis=1), 0.0)[:, None]
        mt = np.where(has, tt.max(axis=1), 0.0)[:, None]
        ey, et = np.exp(yt - my), np.exp(tt - mt)
        sy = np.where(has, ey.sum(axis=1), 1.0)[:, None]
        st = np.where(has, et.sum(axis=1), 1.0)[:, None]
        q, p = ey / sy, et / st
        logq = np.where(valid, (yt - my) - np.log(sy), 0.0)
        logp = np.where(valid, (tt - mt) - np.log(st), 0.0)
    LD = np.where(valid, p * (logp - logq), 0.0).sum(axis=1)
    sy_, st_ = sigmoid(y64), sigmoid(t64)
    # sigmoid(y) - sigmoid(t) from the small sides (no cancellation at saturation)
    both = (y64 >= 0) & (t64 >= 0)
    d = np.where(both, sigmoid(-t64) - sigmoid(-y64), sy_ - st_)
    LP = np.where(valid, d * d, 0.0).sum(axis=1)
    g_rank = np.where(valid, w[0] * c, 0.0) / A
    g_smooth = np.where(valid, (w[1] / tau) * (q - p) + 2.0 * w[2] * d * sy_ * sigmoid(-y64),
                        0.0) / A
    terms = np.array([LR.sum(), LD.sum(), LP.sum()]) / A
    loss = float(np.dot(np.asarray(w, np.float64), terms))
    return dict(LR=LR, LD=LD, LP=LP, terms=terms, loss=loss,
                c=c.astype(np.int64), g_rank=g_rank, g_smooth=g_smooth, g=g_rank + g_smooth, r=r,
                arg=arg, pair=pair & upper)


def smooth_torch(y, t, valid, tau, w, dtype):
    """The smooth parts by the same formulas in torch at ``dtype`` on the host (float32: the
    yardstick of ``gpu_helpers.ref32_close``): per-anchor (LD, LP) and g_smooth (A, K)."""
    import torch

    valid_t = torch.as_tensor(np.asarray(valid, bool))
    A = valid_t.shape[0]
    yv = torch.as_tensor(np.where(valid, np.asarray(y, np.float64), 0.0)).to(dtype)
    tv = torch.as_tensor(np.where(valid, np.asarray(t, np.float64), 0.0)).to(dtype)
    ninf = torch.full_like(yv, -float("inf"))
    has = valid_t.any(1, keepdim=True)
    ys = torch.where(valid_t | ~has, yv / tau, ninf)  # a row without valid slots: kept finite
    ts = torch.where(valid_t | ~has, tv / tau, ninf)
    logq, logp = torch.log_softmax(ys, 1), torch.log_softmax(ts, 1)
    q, p = logq.exp(), logp.exp()
    zero = torch.zeros_like(yv)
    LD = torch.where(valid_t, p * (logp - logq), zero).sum(1)
    sy, st = torch.sigmoid(yv), torch.sigmoid(tv)
    d = sy - st
    LP = torch.where(valid_t, d * d, zero).sum(1)
    g = torch.where(valid_t, (w[1] / tau) * (q - p) + 2.0 * w[2] * d * sy * (1 - sy), zero) / A
    return LD.double().numpy(), LP.double().numpy(), g.double().numpy()
