"""fp64 restatement of ``functional.sage_forward`` (the GraphSAGE baseline of SGAE.py:41-56)
in the CSR-walk form the kernels use, with the test cases both sage test files share.

    x  = table[src_b]
    for each edge (src_b, j) with value a, in CSR order:
        p1_j = x . W1[j, :] + b1[j];  y_j = a relu(p1_j);  p2 += y_j W2[:, j]
    p2 += b2;  logp = relu(p2) - logsumexp(relu(p2))

A virtual row (rowflag set) has no edges here; a source outside [0, n) is padding (NaN row,
no gradient).  Everything is numpy in float64; nothing is imported from the package.

Every output comes with the sum of absolute terms ``A`` and the term count ``n`` that
``gpu_helpers.bounded_close`` takes.  The magnitudes nest: a term's factor that is itself a
rounded sum enters with its own A (y_j with a A1_j, dr with A_dr, ...).  For logp the
log-sum-exp adds the largest A2 of the row (an error of the exponents moves lse by at most
their largest), |lse| and 1 (exp and log themselves: a few ulp of a sum in [1, out]).  dr reads
exp(logp) from the fp32 logp, whose error scales the softmax term by (1 + A_logp).
"""
import numpy as np

XP = np.float64  # the precision of the sums
N_ROWS = 400
WIDTHS = [(32, 32, 32), (16, 16, 64), (64, 64, 16)]
BATCHES = [1, 65, 130]
DEG_LAW = ([1, 2, 3, 5, 8, 30], [0.45, 0.3, 0.15, 0.05, 0.03, 0.02])  # make_golden_hgane.py


def csr_of(adj):
    """(rowptr, col, rowflag, vals) of the mask adj > 0, columns ascending; an empty row is
    virtual: rowflag 1 and, as in ``Graph.from_dense``, a full row of zero values."""
    adj = np.asarray(adj)
    n, m = adj.shape
    rowptr, col, vals, flag = [0], [], [], np.zeros(n, np.uint8)
    for i in range(n):
        js = np.flatnonzero(adj[i] > 0)
        if len(js) == 0:
            flag[i] = 1
            js = np.arange(m)
        col += list(js)
        vals += list(adj[i, js])
        rowptr.append(len(col))
    return (np.asarray(rowptr, np.int64), np.asarray(col, np.int64), flag,
            np.asarray(vals, np.float64))


def forward(table, src, rowptr, col, rowflag, vals, W1, b1, W2, b2):
    """dict: logp (B, out) (NaN rows for padding), p2, A2 (nested), A2own and n2 (B, out),
    A_logp, n_logp, lse (B,), ok (B,), and per entry the edge list ``edges[b]`` of
    (j, a, p1, A1)."""
    table, vals, W1, b1, W2, b2 = (np.asarray(t, XP) for t in (table, vals, W1, b1, W2, b2))
    src = np.asarray(src, np.int64)
    n, in_f = table.shape
    out = W2.shape[0]
    B = len(src)
    ok = (src >= 0) & (src < n)
    p2 = np.zeros((B, out), XP)
    A2 = np.zeros((B, out), XP)
    A2own = np.zeros((B, out), XP)
    n2 = np.ones((B, out))
    edges = []
    for b in range(B):
        es = []
        if ok[b] and not rowflag[src[b]]:
            x = table[src[b]]
            for e in range(rowptr[src[b]], rowptr[src[b] + 1]):
                j, a = int(col[e]), vals[e]
                p1 = x @ W1[j] + b1[j]
                A1 = np.abs(x) @ np.abs(W1[j]) + abs(b1[j])
                es.append((j, a, p1, A1))
                y = a * max(p1, XP(0))
                p2[b] += y * W2[:, j]
                A2own[b] += abs(y) * np.abs(W2[:, j])
                if p1 > 0:
                    A2[b] += a * A1 * np.abs(W2[:, j])
                n2[b] += in_f + 3
        p2[b] += b2
        A2[b] += np.abs(b2)
        A2own[b] += np.abs(b2)
        edges.append(es)
    r = np.maximum(p2, XP(0))
    m = r.max(1, keepdims=True)
    lse = (m + np.log(np.exp(r - m).sum(1, keepdims=True)))[:, 0]
    logp = r - lse[:, None]
    logp[~ok] = np.nan
    A_logp = A2 + A2.max(1, keepdims=True) + np.abs(lse)[:, None] + 1.0
    n_logp = n2 + out + 4
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    return dict(logp=f64(logp), p2=f64(p2), A2=f64(A2), A2own=f64(A2own), n2=n2,
                A_logp=f64(A_logp), n_logp=n_logp, lse=f64(lse), ok=ok, edges=edges, xlogp=logp)


def backward(table, src, W1, W2, f, dlogp):
    """The five gradients of sum(logp * dlogp) from ``f = forward(...)``: dict with dS, dW1,
    db1, dW2, db2, dx (B, in), each with A_<name> and n_<name> (n per element)."""
    table, W1, W2, dlogp = (np.asarray(t, XP) for t in (table, W1, W2, dlogp))
    src = np.asarray(src, np.int64)
    n, in_f = table.shape
    M, out = W1.shape[0], W2.shape[0]
    B = len(src)
    g = {k: np.zeros(s, XP) for k, s in (("dS", (n, in_f)), ("dW1", (M, in_f)), ("db1", (M,)),
                                     ("dW2", (out, M)), ("db2", (out,)), ("dx", (B, in_f)))}
    A = {k: np.zeros_like(v) for k, v in g.items()}
    cnt = {k: np.ones(v.shape) for k, v in g.items()}
    for b in range(B):
        if not f["ok"][b]:
            continue
        x = table[src[b]]
        p = np.exp(f["xlogp"][b])
        act = f["p2"][b] > 0
        dr = np.where(act, dlogp[b] - p * dlogp[b].sum(), XP(0))
        A_dr = np.where(act, np.abs(dlogp[b]) + p * np.abs(dlogp[b]).sum() * (1.0 + f["A_logp"][b]),
                        0.0)
        n_dr = out + f["n_logp"][b].max()
        g["db2"] += dr
        A["db2"] += A_dr
        cnt["db2"] += n_dr
        for j, a, p1, A1 in f["edges"][b]:
            y = a * max(p1, XP(0))
            g["dW2"][:, j] += dr * y
            A["dW2"][:, j] += A_dr * a * A1 * (p1 > 0)
            cnt["dW2"][:, j] += n_dr + in_f + 3
            if p1 <= 0:
                continue
            dz = a * (W2[:, j] @ dr)
            A_dz = a * (np.abs(W2[:, j]) @ A_dr)
            n_dz = n_dr + out + 2
            g["dW1"][j] += dz * x
            A["dW1"][j] += A_dz * np.abs(x)
            cnt["dW1"][j] += n_dz + 1
            g["db1"][j] += dz
            A["db1"][j] += A_dz
            cnt["db1"][j] += n_dz
            g["dx"][b] += dz * W1[j]
            A["dx"][b] += A_dz * np.abs(W1[j])
            cnt["dx"][b] += n_dz + 1
        g["dS"][src[b]] += g["dx"][b]
        A["dS"][src[b]] += A["dx"][b]
        cnt["dS"][src[b]] += cnt["dx"][b]
    res = {k: np.asarray(v, np.float64) for k, v in g.items()}
    res.update({"A_" + k: np.asarray(v, np.float64) for k, v in A.items()})
    res.update({"n_" + k: v for k, v in cnt.items()})
    return res


def kink_ratio(f):
    """Smallest |p| / A over the pre-activations that reach the output: layer 1 on the edge
    columns of the batch rows, layer 2 on every output of every entry (A: the
    pre-activation's own sum of absolute terms)."""
    r1 = min((abs(p1) / A1 for es in f["edges"] for _, _, p1, A1 in es), default=np.inf)
    okr = f["ok"]
    r2 = float((np.abs(f["p2"][okr]) / f["A2own"][okr]).min()) if okr.any() else np.inf
    return float(r1), r2


def make_adjacency(M, seed, n=N_ROWS):
    """(adj float32 (n, M) normalised by column sum, rows): integer counts 1-3 on edges whose
    row degrees follow the 2015 law, +1 on the diagonal block (no empty column), then
    ``normalize_adjacency_matrix``'s (adj * d) * d with d = colsum ** -0.5 in float32.
    rows: the forced rows full (degree M), one (degree 1), zero (all zero: a virtual row)."""
    rng = np.random.default_rng(seed)
    degs, p = DEG_LAW
    deg = np.minimum(rng.choice(degs, n, p=p), M)
    counts = np.zeros((n, M), np.float32)
    for i in range(n):
        counts[i, rng.choice(M, deg[i], replace=False)] = rng.integers(1, 4, deg[i])
    counts[np.arange(M), np.arange(M)] += 1
    rows = dict(full=M + 3, one=M + 7, zero=M + 11)
    counts[rows["full"]] = rng.integers(1, 4, M)
    counts[rows["one"]] = 0
    counts[rows["one"], rng.integers(0, M)] = 2
    counts[rows["zero"]] = 0
    d = counts.sum(0, dtype=np.float32) ** np.float32(-0.5)
    return (counts * d) * d, rows


def make_batch(B, rows, seed, n=N_ROWS):
    """int64 (B,) sources: the forced rows (full, one, zero, 0, n - 1, as many as fit), then
    distinct others; from 65 entries on the last ten repeat earlier sources, one of them
    three times over; shuffled."""
    rng = np.random.default_rng(seed + 1000)
    forced = [rows["full"], rows["one"], rows["zero"], 0, n - 1][:B]
    rep = 10 if B >= 65 else 0
    pool = np.setdiff1d(np.arange(n), forced)
    k = B - len(forced) - rep
    # more entries than rows: twenty rows stay outside the batch, the rest are further repeats
    if k > len(pool) - 20:
        pool = pool[:-20]
    fresh = list(rng.choice(pool, min(k, len(pool)), replace=False))
    batch = forced + fresh
    batch += list(rng.choice(batch, k - len(fresh), replace=True)) if k > len(fresh) else []
    if rep:
        first = batch[len(forced)]
        batch += [first, first] + list(rng.choice(batch[:B - rep], rep - 2, replace=False))
    return rng.permutation(np.asarray(batch, np.int64))


def make_params(widths, seed, n=N_ROWS):
    """(gdp dict, table, W1, b1, W2, b2) float32, drawn in the reference's init order after
    ``torch.manual_seed(seed)``: the table (``rand`` with the GDP column), linear1, linear2."""
    import torch

    in_f, M, out = widths
    rng = np.random.default_rng(seed + 2000)
    gdp = {i: float(v) for i, v in enumerate(rng.uniform(0.1, 1.0, n).astype(np.float32))}
    torch.manual_seed(seed)
    gdp_values = torch.tensor(list(gdp.values())).view(-1, 1)
    table = torch.cat((torch.rand([n, in_f])[:, :-1], gdp_values), dim=1)
    l1 = torch.nn.Linear(in_f, M)
    l2 = torch.nn.Linear(M, out)
    return (gdp, table.numpy(), l1.weight.detach().numpy(), l1.bias.detach().numpy(),
            l2.weight.detach().numpy(), l2.bias.detach().numpy())


# The seed of each case (0 where none is named).  A seed has to keep every pre-activation of the
# case clear of its ReLU kink (|p| >= 1e-5 A, kink_ratio), and every element of logp and of the
# five gradients clear of heavy cancellation: the host test holds the restatement to torch's fp64
# autograd at 1e-12 |ref| per element, both sides round at about 2e-16 A, so an element that
# cancels to a few 1e-5 A would sit at that bound by rounding alone.  These are the first seeds
# found under which the comparison stays below a fifth of its bound with this file's sums in
# float64 and in long double (XP) alike; tests/test_sage_host.py asserts a margin on both.
SEEDS = {((32, 32, 32), 130): 15,
         ((16, 16, 64), 1): 1, ((16, 16, 64), 65): 3, ((16, 16, 64), 130): 21,
         ((64, 64, 16), 65): 64, ((64, 64, 16), 130): 29}


def make_case(widths, B, seed=None):
    """Everything a test needs, float32 / int64 numpy: adj, rows, src, gdp, table, W1, b1, W2,
    b2, the CSR of adj, and target (B,) / dlogp (B, out) for the two upstream gradients."""
    seed = SEEDS.get((tuple(widths), B), 0) if seed is None else seed
    in_f, M, out = widths
    adj, rows = make_adjacency(M, seed)
    src = make_batch(B, rows, seed)
    gdp, table, W1, b1, W2, b2 = make_params(widths, seed)
    rng = np.random.default_rng(seed + 3000)
    rowptr, col, rowflag, vals = csr_of(adj)
    return dict(widths=tuple(widths), B=B, seed=seed, adj=adj, rows=rows, src=src, gdp=gdp,
                table=table, W1=W1, b1=b1, W2=W2, b2=b2, rowptr=rowptr, col=col,
                rowflag=rowflag, vals=vals, target=rng.integers(0, out, B),
                dlogp=rng.standard_normal((B, out)).astype(np.float32))


def reference_forward(c):
    return forward(c["table"], c["src"], c["rowptr"], c["col"], c["rowflag"], c["vals"], c["W1"],
                   c["b1"], c["W2"], c["b2"])


def reference_backward(c, f, dlogp):
    return backward(c["table"], c["src"], c["W1"], c["W2"], f, dlogp)


def reference(c, dlogp):
    """(forward dict, backward dict) of case ``c`` under the upstream gradient ``dlogp``."""
    f = reference_forward(c)
    return f, reference_backward(c, f, dlogp)


def nll_dlogp(target, out):
    """d F.nll_loss(logp, target) / d logp (mean reduction)."""
    B = len(target)
    g = np.zeros((B, out))
    g[np.arange(B), target] = -1.0 / B
    return g
