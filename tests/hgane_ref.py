"""fp64 torch restatement of HGANE's batch attention layer (HGANE.py:37-76) in the sparse
form a device implementation computes (group segments, no (B, B, 2F) tensor), with injected
keep masks: the oracle for device kernels, itself held to the reference's outputs
(tests/golden/hgane.npz) by tests/test_hgane_host.py.

Batch entries b, k in [0, B); g_b the group of src[b]; N(b) the inter row of src[b]:

    x_bj = exp(lrelu(el_b + er_j)),  j in N(b)     Z1_b = sum_j x_bj
    y_bk = exp(lrelu(pl_b + pr_k)),  g_k = g_b     Zc_b = Z1_b + sum_k y_bk
    alpha = x / Z1 * keep / (1 - p),  beta = y / Zc * keep / (1 - p)
    U = alpha @ h1 + beta @ h2,   V = alpha.T @ h3
    out = elu(lrelu(bn1(U)) @ lrelu(bn2(V)).T)

Dense over (B, M) and (B, B): for the small batches of the tests only.
"""
import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.2
M_GOLDEN = 32
CASES = {"A.": (16, 16, 31), "B.": (128, 64, 32)}  # tag -> (in, F, seed) of hgane.npz


def dout_weights(seed, B, M=M_GOLDEN):
    """The loss weights of the fixture's case with that seed (make_golden_hgane.py)."""
    return np.random.default_rng(seed + 100).standard_normal((B, M)).astype(np.float32)


def source_embedding(seed, n, fin):
    """The (n, in) ``source_embedding`` the reference's constructor draws after
    ``torch.manual_seed(seed)``: the second ``torch.rand([n, in])`` (``features`` is first,
    HGANE.py:19-20).  Case B's table is not stored in the fixture."""
    torch.manual_seed(seed)
    torch.rand([n, fin])
    return torch.rand([n, fin])


def masks(counts, gid, src):
    """(inter (B, M) bool, same (B, B) bool) of a batch."""
    src = np.asarray(src, np.int64)
    g = np.asarray(gid)[src]
    return (torch.as_tensor(np.asarray(counts)[src] > 0),
            torch.as_tensor(g[:, None] == g[None, :]))


def core(el, er, pl, pr, h1, h2, h3, inter, same, keep_inter=None, keep_intra=None, p=0.0):
    """dict(U, V, Z1, Zc, alpha, beta, x, y, s, t): torch tensors of the inputs' dtype.
    keep_* are 0/1 masks of shape (B, M) / (B, B) (None: all kept)."""
    s = F.leaky_relu(el[:, None] + er[None, :], SLOPE)
    t = F.leaky_relu(pl[:, None] + pr[None, :], SLOPE)
    zero = torch.zeros((), dtype=s.dtype)
    x = torch.where(inter, torch.exp(s), zero)
    y = torch.where(same, torch.exp(t), zero)
    Z1 = x.sum(1)
    Zc = Z1 + y.sum(1)
    alpha = x / Z1[:, None]
    beta = y / Zc[:, None]
    if keep_inter is not None:
        alpha = alpha * keep_inter.to(s.dtype) / (1.0 - p)
    if keep_intra is not None:
        beta = beta * keep_intra.to(s.dtype) / (1.0 - p)
    return dict(U=alpha @ h1 + beta @ h2, V=alpha.t() @ h3, Z1=Z1, Zc=Zc, alpha=alpha, beta=beta,
                x=x, y=y, s=el[:, None] + er[None, :], t=pl[:, None] + pr[None, :])


def _bn_lrelu(x, weight, bias, running, eps=1e-5):
    if running is None:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = running
    return F.leaky_relu((x - mean) / torch.sqrt(var + eps) * weight + bias, SLOPE)


def projections(P, src):
    """(el, er, pl, pr, h1, h2, h3) of the layer's parameters ``P`` (state_dict names)."""
    Fd = P["W1.weight"].shape[0]
    E = P["source_embedding"][torch.as_tensor(np.asarray(src, np.int64))]
    h1 = P["recipient_embedding"] @ P["W1.weight"].t()
    h2 = E @ P["W2.weight"].t()
    h3 = E @ P["W1.weight"].t()  # HGANE.py:73 applies W1 to the source aggregate
    a12, a3 = P["a12.weight"].reshape(-1), P["a3.weight"].reshape(-1)
    return h2 @ a12[Fd:], h1 @ a12[:Fd], h2 @ a3[:Fd], h2 @ a3[Fd:], h1, h2, h3


def layer(P, src, counts, gid, training=True, running=None, keep_inter=None, keep_intra=None,
          p=0.0):
    """The layer's output from parameters ``P`` (dict of torch tensors by state_dict name).
    running: ((mean1, var1), (mean2, var2)) for eval mode."""
    inter, same = masks(counts, gid, src)
    c = core(*projections(P, src), inter, same, keep_inter, keep_intra, p)
    r1, r2 = (None, None) if training else running
    u = _bn_lrelu(c["U"], P["bn1.weight"], P["bn1.bias"], r1)  # bn1 normalises U
    v = _bn_lrelu(c["V"], P["bn2.weight"], P["bn2.bias"], r2)
    return F.elu(u @ v.t())


def params64(z, tag, extra=None):
    """The fixture's init state as fp64 leaves that require grad."""
    P = {}
    for k in z.files:
        if k.startswith(tag + "init.") and "running" not in k and "num_batches" not in k:
            name = k[len(tag) + 5:]
            if name != "features":
                P[name] = torch.tensor(np.asarray(z[k], np.float64), requires_grad=True)
    for k, v in (extra or {}).items():
        P[k] = torch.tensor(np.asarray(v, np.float64), requires_grad=True)
    return P


def abs_terms(c, h1, h2, h3, dU, dV, kin=None, kra=None, p=0.0):
    """Absolute-term sums A and term counts n for gpu_helpers.bounded_close of every output
    of the core and of its backward (numpy fp64), from ``core``'s dict in fp64.

    A term's magnitude includes the magnitudes inside it: the score gradient
    ds_bj = x_bj (kf d alpha / Z1 - D1 / Z1 - D2 / Zc) has
    A = x (kf |d alpha|_abs / Z1 + |D1|_abs / Z1 + |D2|_abs / Zc) lrelu' with
    |d alpha|_abs = |dU| . |h1| + |dV| . |h3|, |D1|_abs = sum alpha |d alpha|_abs and
    |D2|_abs = sum beta |d beta|_abs, |d beta|_abs = |dU| . |h2|; dt likewise."""
    n = lambda t: np.abs(t.detach().numpy().astype(np.float64))  # noqa: E731
    raw = lambda t: t.detach().numpy().astype(np.float64)  # noqa: E731
    alpha, beta, x, y = raw(c["alpha"]), raw(c["beta"]), raw(c["x"]), raw(c["y"])
    Z1, Zc = raw(c["Z1"])[:, None], raw(c["Zc"])[:, None]
    B, M = alpha.shape
    Fd = h1.shape[1]
    kf_in = np.ones_like(alpha) if kin is None else raw(kin) / (1.0 - p)
    kf_ra = np.ones_like(beta) if kra is None else raw(kra) / (1.0 - p)
    ah1, ah2, ah3, adU, adV = n(h1), n(h2), n(h3), n(dU), n(dV)
    da = adU @ ah1.T + ah3 @ adV.T  # (B, M)
    db = adU @ ah2.T  # (B, B)
    D1 = (alpha * da).sum(1, keepdims=True)
    D2 = (beta * db).sum(1, keepdims=True)
    ls = np.where(raw(c["s"]) > 0, 1.0, SLOPE)
    lt = np.where(raw(c["t"]) > 0, 1.0, SLOPE)
    ds = x * (kf_in * da / Z1 + D1 / Z1 + D2 / Zc) * ls
    dt = y * (kf_ra * db + D2) / Zc * lt
    deg = (x > 0).sum(1).astype(np.float64)
    ng = (y > 0).sum(1).astype(np.float64)
    colin = (x > 0).sum(0).astype(np.float64)
    colra = (y > 0).sum(0).astype(np.float64)
    # inside a term: the 2F-term dots of d alpha / d beta, ~16 elementwise ops and up to 80
    # levels of the wave / tile / block partial reduces; D1 and D2 are row sums themselves
    k_in = 2 * Fd + 96
    A = dict(U=alpha @ ah1 + beta @ ah2, V=alpha.T @ ah3, Zc=Zc[:, 0],
             d_el=ds.sum(1), d_er=ds.sum(0), d_pl=dt.sum(1), d_pr=dt.sum(0),
             dh1=alpha.T @ adU, dh3=alpha @ adV, dh2=beta.T @ adU)
    row = deg + ng + k_in
    N = dict(U=row, V=colin + k_in, Zc=row, d_el=2 * row, d_er=colin + deg.max() + ng.max() + k_in,
             d_pl=2 * row, d_pr=colra + ng.max() + k_in, dh1=colin + k_in, dh3=row,
             dh2=colra + ng.max() + k_in)
    return A, N
