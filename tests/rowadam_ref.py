"""fp64 numpy restatements for the row-sparse table training: the touched-row list of an
incidence plan (msha_plan_rows) and the lazy Adam over it (msha_adam_rows_step).

The rule is the project's dense Adam restricted to the touched rows, with one global step
count per parameter:

    m <- m + (1 - b1) (g - m)
    v <- b2 v + (1 - b2) g^2
    p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

which is ``torch.optim.SparseAdam`` run with ``eps * sqrt(1 - b2^t)`` in place of ``eps`` at
step t (torch adds eps before the bias correction)."""
import numpy as np


def touched_rows(rowptr, cap=None):
    """(rows, count): the ascending ids of the rows with an endpoint, int32, -1 from the
    count to ``cap`` (the whole list when None)."""
    rowptr = np.asarray(rowptr, np.int64)
    ids = np.flatnonzero(np.diff(rowptr) > 0).astype(np.int32)
    if cap is None:
        return ids, len(ids)
    out = np.full(cap, -1, np.int32)
    out[: len(ids)] = ids
    return out, len(ids)


def lazy_adam_step(p, m, v, t, rows, g, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """One step in place on the fp64 arrays ``p, m, v`` (n, F): ``rows`` (R,) distinct row
    ids, ``g`` (R, F) their gradients, ``t`` the step count before the step.  Returns t + 1."""
    b1, b2 = betas
    t = t + 1
    rows = np.asarray(rows, np.int64)
    g = np.asarray(g, np.float64)
    m[rows] = m[rows] + (1.0 - b1) * (g - m[rows])
    v[rows] = b2 * v[rows] + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    bc2_sqrt = np.sqrt(1.0 - b2 ** t)
    p[rows] = p[rows] - step_size * (m[rows] / (np.sqrt(v[rows]) / bc2_sqrt + eps))
    return t


def sparse_adam_eps(eps, beta2, t):
    """The eps that makes ``torch.optim.SparseAdam``'s step t the rule above."""
    return eps * np.sqrt(1.0 - beta2 ** t)
