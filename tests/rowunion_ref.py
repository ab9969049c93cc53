"""Restatements for the row-sparse paths of link_mlp_loss, link_match_loss and sage_forward:
the list of the rows that occur, and the union of several row gradients of one table
(msha_row_grad_union) in numpy fp32 with the adds in list order."""
import numpy as np


def listed(ids, cap):
    """(rows int32 (cap,), count): the ascending distinct ``ids``, -1 past the count."""
    ids = np.unique(np.asarray(ids, np.int64))
    out = np.full(cap, -1, np.int32)
    out[: len(ids)] = ids
    return out, len(ids)


def union(lists, n):
    """``lists``: (rows (cap_j,), count_j, vals (cap_j, F) fp32) each, rows ascending and
    distinct below the count.  Returns (rows int32 (cap,), count, vals fp32 (cap, F)) with
    cap = min(n, sum cap_j): the ascending union, and per row x_1 + x_2 + .. + x_k added left
    to right in fp32, x_j = +0.0 where list j does not hold the row."""
    F = lists[0][2].shape[1]
    cap = min(n, sum(len(r) for r, _, _ in lists))
    held = [{int(x): i for i, x in enumerate(np.asarray(r)[:c]) if 0 <= x < n}
            for r, c, _ in lists]
    ids = sorted(set().union(*held))
    assert len(ids) <= cap
    rows = np.full(cap, -1, np.int32)
    rows[: len(ids)] = ids
    vals = np.zeros((cap, F), np.float32)
    for i, r in enumerate(ids):
        s = None
        for at, (_, _, v) in zip(held, lists):
            x = (np.asarray(v[at[r]], np.float32) if r in at else np.zeros(F, np.float32))
            s = x.copy() if s is None else (s + x).astype(np.float32)
        vals[i] = s
    return rows, len(ids), vals
