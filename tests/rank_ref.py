"""The CPU reference of the filtered link ranks, shared by the rank tests: fp64 logits,
counts under the library's order (+inf highest, every NaN below -inf and all NaNs equal
among themselves, -0.0 == +0.0), exclusion lists, ``col_offset``, the three tie rules and
the metrics built on them."""
import numpy as np

TIES = {"optimistic": 0, "mean": 1, "pessimistic": 2}


def above_equal(c, t):
    """Elementwise (c above t, c equal to t) under the order."""
    c = np.asarray(c, np.float64)
    cn, tn = np.isnan(c), np.isnan(t)
    with np.errstate(invalid="ignore"):
        gt = ~cn & (tn | (c > t))
        eq = (cn & tn) | (~cn & ~tn & (c == t))
    return gt, eq


def counts(logits, target, exclude=None, col_offset=0, target_logit=None):
    """(greater, equal) int64 of every row of a (B, n) fp64 logit matrix over the candidates
    [col_offset, col_offset + n) for GLOBAL targets; ``exclude``: per row a collection of
    local column numbers (or None).  A target outside the range gives -1 / -1 unless
    ``target_logit`` supplies its logit, in which case every non-excluded column counts."""
    logits = np.asarray(logits, np.float64)
    B, n = logits.shape
    greater = np.full(B, -1, np.int64)
    equal = np.full(B, -1, np.int64)
    for b in range(B):
        t = int(target[b]) - col_offset
        local = 0 <= t < n
        if not local and target_logit is None:
            continue
        keep = np.ones(n, bool)
        if exclude is not None and exclude[b] is not None and len(exclude[b]):
            keep[np.asarray(sorted(set(int(x) for x in exclude[b])), np.int64)] = False
        if local:
            keep[t] = False
        z = np.float64(target_logit[b]) if target_logit is not None else logits[b, t]
        gt, eq = above_equal(logits[b, keep], z)
        greater[b], equal[b] = gt.sum(), eq.sum()
    return greater, equal


def rank2(greater, equal, ties="mean"):
    """2 * rank of the valid rows (integers: the mean-tie half is exact)."""
    g, e = np.asarray(greater, np.int64), np.asarray(equal, np.int64)
    ok = g >= 0
    return 2 + 2 * g[ok] + TIES[ties] * e[ok]


def metrics(greater, equal, ks=(1, 3, 10), ties="mean"):
    r2 = rank2(greater, equal, ties)
    if len(r2) == 0:
        raise ValueError("no valid rows to rank")
    out = {"mrr": float(np.sum(2.0 / r2.astype(np.float64)) / len(r2)),
           "mean_rank": float(r2.sum()) / (2 * len(r2)), "n": int(len(r2))}
    for k in ks:
        out[f"hits@{k}"] = int((r2 <= 2 * k).sum()) / len(r2)
        out[f"hits_count@{k}"] = int((r2 <= 2 * k).sum())
    return out


def brute_counts(values, t):
    """(greater, equal) of candidate t of one score vector by a plain sort: the key is
    (not NaN, value) with -0.0 folded, compared as tuples."""
    def key(v):
        v = float(v)
        return (0, 0.0) if v != v else (1, v + 0.0 if v != 0 else 0.0)

    keys = [key(v) for j, v in enumerate(values) if j != t]
    kt = key(values[t])
    order = sorted(keys, reverse=True)
    greater = sum(1 for k in order if k > kt)
    equal = sum(1 for k in order if k == kt)
    return greater, equal


STAT_C, U32 = 4.0, 2.0 ** -24  # gpu_helpers' four-sigma constant and fp32 unit roundoff


def bracket(q, h, target):
    """The interval a correct fp32-accumulated count must fall in, from fp64 operands
    ``q`` (B, F) and ``h`` (n, F): delta = 4 sqrt(F) 2^-24 sum_f |q_f t_f| per logit,
    lo = #{z_j > z_t + d_j + d_t}, hi = #{z_j >= z_t - d_j - d_t} over j != t.
    ``greater >= lo`` and ``greater + equal <= hi``."""
    q, h = np.asarray(q, np.float64), np.asarray(h, np.float64)
    F = q.shape[1]
    z = q @ h.T
    d = STAT_C * np.sqrt(F) * U32 * (np.abs(q) @ np.abs(h).T)
    B = q.shape[0]
    lo = np.zeros(B, np.int64)
    hi = np.zeros(B, np.int64)
    for b in range(B):
        t = int(target[b])
        keep = np.ones(h.shape[0], bool)
        keep[t] = False
        lo[b] = (z[b, keep] > z[b, t] + d[b, keep] + d[b, t]).sum()
        hi[b] = (z[b, keep] >= z[b, t] - d[b, keep] - d[b, t]).sum()
    return lo, hi


def random_problem(dt):
    """The random-float problem of the GPU test: torch.rand, seed 21, n = 1000, F = 128,
    B = 130, targets from default_rng(5); fp64 views of the dtype-rounded operands."""
    import torch

    n, F, B = 1000, 128, 130
    g = torch.Generator().manual_seed(21)
    h = torch.rand(n, F, generator=g).to(dt)
    q = torch.rand(B, F, generator=g).to(dt)
    target = np.random.default_rng(5).integers(0, n, B)
    return dict(n=n, F=F, B=B, h=h, q=q, target=target, hd=h.double().numpy(),
                qd=q.double().numpy())
