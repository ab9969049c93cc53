"""The GraphSAGE baseline on the device (csrc/sage.hip) against the fp64 CSR-walk
restatement ``sage_ref`` fed the same fp32 inputs: logp and the five gradients under
``bounded_close(rtol=1e-5)`` for the nll and a dense upstream gradient, against torch
autograd on the device, the exactness claims (zero rows, repeated sources, two calls,
virtual row), the argument rules that need the device, the module, three optimiser steps and
one captured forward + backward.

N = 400 sources; widths (in, M, out) and batches as ``sage_ref.WIDTHS`` / ``BATCHES``, and
one batch of 8209 entries at 32 / 32 / 32: above 8192 entries the weight-gradient blocks own
more than one round of 16 entries each (at most 512 blocks)."""
import numpy as np
import pytest
import torch

import sage_ref as R
from gpu_helpers import bounded_close

pytestmark = pytest.mark.gpu

CASES = [(w, B) for w in R.WIDTHS for B in R.BATCHES] + [((32, 32, 32), 8209)]
IDS = [f"{w[0]}-{w[1]}-{w[2]}-B{B}" for w, B in CASES]
GRADS = ("dS", "dW1", "db1", "dW2", "db2")
_CASES: dict = {}


def _case(widths, B):
    """The case and its fp64 references for both upstream gradients, computed once."""
    key = (tuple(widths), B)
    if key not in _CASES:
        c = R.make_case(widths, B)
        f = R.reference_forward(c)
        refs = {"nll": (f, R.reference_backward(c, f, R.nll_dlogp(c["target"], widths[2]))),
                "dense": (f, R.reference_backward(c, f, c["dlogp"]))}
        _CASES[key] = (c, refs)
    return _CASES[key]


def _dev(c, dev, grad=True):
    """(table, W1, b1, W2, b2) leaves, src, adj, graph, vals on the device."""
    from msha_gnn_amd.graph import graph_of

    leaves = [torch.tensor(c[k], device=dev, requires_grad=grad)
              for k in ("table", "W1", "b1", "W2", "b2")]
    adj = torch.tensor(c["adj"], device=dev)
    g, transposed = graph_of(adj)
    assert not transposed and g.n_cols == c["widths"][1]
    return leaves, torch.tensor(c["src"], device=dev), adj, g, g.values(adj)


def _run(MF, c, dev, upstream):
    leaves, src, adj, g, vals = _dev(c, dev)
    logp = MF.sage_forward(leaves[0], src, g, vals, *leaves[1:])
    if upstream == "nll":
        torch.nn.functional.nll_loss(logp, torch.tensor(c["target"], device=dev)).backward()
    else:
        logp.backward(torch.tensor(c["dlogp"], device=dev))
    return logp.detach(), [t.grad for t in leaves]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("upstream", ["nll", "dense"])
@pytest.mark.parametrize("widths,B", CASES, ids=IDS)
def test_logp_and_gradients_match_fp64_restatement(cuda, msha, widths, B, upstream):
    from msha_gnn_amd import functional as MF

    c, refs = _case(widths, B)
    f, g = refs[upstream]
    r1, r2 = R.kink_ratio(f)
    assert r1 >= 1e-5 and r2 >= 1e-5, (r1, r2)  # no pre-activation within rounding of its kink
    logp, grads = _run(MF, c, cuda, upstream)
    name = f"{widths} B={B} {upstream}"
    assert logp.shape == (B, widths[2]) and logp.dtype == torch.float32
    bounded_close(logp.cpu().numpy(), f["logp"], f["A_logp"], f["n_logp"], 1e-5, f"{name} logp")
    for key, got in zip(GRADS, grads):
        assert got.shape == g[key].shape and got.dtype == torch.float32
        bounded_close(got.cpu().numpy(), g[key], g["A_" + key], g["n_" + key], 1e-5,
                      f"{name} {key}")
    # rows of the table outside the batch: exact zeros
    dS = grads[0].cpu().numpy()
    outside = np.setdiff1d(np.arange(R.N_ROWS), c["src"])
    assert len(outside) and not dS[outside].any()
    assert (dS[np.unique(c["src"])] != 0).any()


@pytest.mark.parametrize("widths", R.WIDTHS, ids=[str(w) for w in R.WIDTHS])
def test_gradients_match_torch_autograd(cuda, msha, widths):
    """End to end against autograd of SGAE.py:52-56 in fp64 on the device (B = 130, dense
    upstream gradient), under the restatement's A and n."""
    from msha_gnn_amd import functional as MF

    c, refs = _case(widths, 130)
    f, g = refs["dense"]
    t64 = lambda k: torch.tensor(np.asarray(c[k], np.float64), device=cuda,  # noqa: E731
                                 requires_grad=True)
    table, W1, b1, W2, b2 = (t64(k) for k in ("table", "W1", "b1", "W2", "b2"))
    adj = torch.tensor(np.asarray(c["adj"], np.float64), device=cuda)
    src = torch.tensor(c["src"], device=cuda)
    x = torch.relu(torch.nn.functional.linear(table[src], W1, b1))
    x = torch.relu(torch.nn.functional.linear(torch.mul(adj[src], x), W2, b2))
    ref = torch.log_softmax(x, dim=1)
    ref.backward(torch.tensor(c["dlogp"], device=cuda).double())
    logp, grads = _run(MF, c, cuda, "dense")
    bounded_close(logp.cpu().numpy(), ref.detach().cpu().numpy(), f["A_logp"], f["n_logp"], 1e-5,
                  f"{widths} autograd logp")
    for key, got, want in zip(GRADS, grads, (table, W1, b1, W2, b2)):
        bounded_close(got.cpu().numpy(), want.grad.cpu().numpy(), g["A_" + key], g["n_" + key],
                      1e-5, f"{widths} autograd {key}")


def test_repeated_sources_two_calls_and_the_virtual_row(cuda, msha):
    from msha_gnn_amd import functional as MF

    c, refs = _case((32, 32, 32), 130)
    f, g = refs["dense"]
    first = _run(MF, c, cuda, "dense")
    again = _run(MF, c, cuda, "dense")
    for x, y in zip([first[0]] + first[1], [again[0]] + again[1]):
        assert torch.equal(_bits(x), _bits(y))
    logp = first[0].cpu().numpy()
    src = c["src"]
    counts = np.bincount(src, minlength=R.N_ROWS)
    assert counts.max() >= 3
    for r in np.flatnonzero(counts > 1):
        rows = logp[src == r].view(np.int32)
        assert (rows == rows[0]).all()
    # the virtual row: log_softmax(relu(b2)), and no gradient to its table row
    b = int(np.flatnonzero(src == c["rows"]["zero"])[0])
    relu_b2 = np.maximum(c["b2"].astype(np.float64), 0)
    want = relu_b2 - np.log(np.exp(relu_b2).sum())
    np.testing.assert_allclose(f["logp"][b], want, rtol=1e-13, atol=1e-13)
    bounded_close(logp[b], want, f["A_logp"][b], f["n_logp"][b], 1e-5, "virtual row logp")
    assert counts[c["rows"]["zero"]] == 1
    assert not first[1][0][c["rows"]["zero"]].any().item()
    # the table gradient is a function of the index list: a copy of the list, the same bits
    leaves, tsrc, adj, gr, vals = _dev(c, cuda)
    lp = MF.sage_forward(leaves[0], tsrc.clone(), gr, vals, *leaves[1:])
    lp.backward(torch.tensor(c["dlogp"], device=cuda))
    assert torch.equal(_bits(leaves[0].grad), _bits(first[1][0]))


def test_index_rules_and_the_empty_batch(cuda, msha):
    from msha_gnn_amd import functional as MF

    c, _ = _case((16, 16, 64), 65)
    leaves, src, adj, g, vals = _dev(c, cuda)
    n = R.N_ROWS
    for bad in (n, -n - 1):
        s = src.clone()
        s[7] = bad
        with pytest.raises(IndexError, match="out of bounds"):
            MF.sage_forward(leaves[0], s, g, vals, *leaves[1:])
    # negative indices wrap as table[src] does
    s = src.clone()
    s[5], s[9] = int(src[5]) - n, -1
    want = src.clone()
    want[9] = n - 1
    with torch.no_grad():
        a = MF.sage_forward(leaves[0], s, g, vals, *leaves[1:])
        b = MF.sage_forward(leaves[0], want, g, vals, *leaves[1:])
    assert torch.equal(_bits(a), _bits(b))
    # unchecked: a stray entry is padding (NaN row, no gradient), nothing else moves
    s = want.clone()
    s[3] = n + 4
    lp = MF.sage_forward(leaves[0], s, g, vals, *leaves[1:], check=False)
    assert torch.isnan(lp[3]).all() and torch.equal(_bits(lp[4:]), _bits(b[4:]))
    w = torch.ones_like(lp)
    w[3] = 0
    lp.backward(w)
    assert torch.isfinite(leaves[0].grad).all() and torch.isfinite(leaves[3].grad).all()
    # B = 0: an empty (0, out) result and zero gradients
    for t in leaves:
        t.grad = None
    empty = MF.sage_forward(leaves[0], src[:0], g, vals, *leaves[1:])
    assert empty.shape == (0, 64) and empty.dtype == torch.float32
    empty.sum().backward()
    for t in leaves:
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any().item()


def test_module_equals_the_functional_and_saves_nothing_in_eval(cuda, msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    widths = (32, 32, 32)
    c, _ = _case(widths, 130)
    torch.manual_seed(c["seed"])
    model = layers.GraphSAGE(*widths, c["gdp"]).to(cuda)
    for key, want in zip(model.state_dict().values(), ("table", "W1", "b1", "W2", "b2")):
        assert np.array_equal(key.cpu().numpy(), c[want])
    leaves, src, adj, g, vals = _dev(c, cuda)
    out = model(src, adj)
    ref = MF.sage_forward(leaves[0], src, g, vals, *leaves[1:])
    assert out.grad_fn is not None and torch.equal(_bits(out), _bits(ref))
    target = torch.tensor(c["target"], device=cuda)
    torch.nn.functional.nll_loss(out, target).backward()
    torch.nn.functional.nll_loss(ref, target).backward()
    for p, t in zip(model.parameters(), leaves):
        assert torch.equal(_bits(p.grad), _bits(t.grad))
    model.eval()
    ev = model(src, adj)  # eval changes nothing (no dropout in SGAE.py:50-56)
    assert torch.equal(_bits(ev), _bits(out))
    with torch.no_grad():
        ng = model(src, adj)
    assert ng.grad_fn is None and not ng.requires_grad and torch.equal(_bits(ng), _bits(out))
    frozen = MF.sage_forward(leaves[0].detach(), src, g, vals, *(t.detach() for t in leaves[1:]))
    assert frozen.grad_fn is None and torch.equal(_bits(frozen), _bits(out))
    with pytest.raises(TypeError, match="dense adjacency"):
        model(src, g)


def test_three_adam_steps_follow_the_composition(cuda, msha):
    """SGAE.py:88-102 for three batches of 65: the module with msha_gnn_amd.optim.Adam (lr
    1e-3, weight decay 5e-4) against three eager steps of the torch composition of
    SGAE.py:52-56 with torch.optim.Adam, run in fp64 on the device so that the reference side
    adds no rounding of its own.  Losses and parameters under ``bounded_close(rtol=1e-5)``.

    A loss is a mean of B logp entries: their A and n.  A parameter after three steps is
    p0 - sum_t lr m_t / (sqrt(v_t) + eps) with m, v averages of g' = g + wd p and g'^2: A =
    |p0| + 3 lr, n = 12.  The step depends on g' through ratios, so a relative error e of g'
    moves one step by at most about 4 lr e (the bias-corrected weights w_i / sqrt(w'_i) of
    three steps sum to under 2, the v term as much again), and never by more than the step
    itself, lr a step.  e is the gradient's own bound over |g'|, (1e-5 |g| + 4 sqrt(n) u A_g) /
    |g'|, and since m and v carry a step's error on, every step is charged the largest e of
    the three: floor = min(12 lr max_t e_t, 3 lr).  A row outside all three batches has e = 0
    (its g' = wd p is exact on both sides)."""
    from msha_gnn_amd import layers
    from msha_gnn_amd.optim import Adam

    widths, lr, wd, u, B = (32, 32, 32), 1e-3, 5e-4, 2.0 ** -24, 65
    c, _ = _case(widths, B)
    torch.manual_seed(c["seed"])
    model = layers.GraphSAGE(*widths, c["gdp"]).to(cuda)
    opt = Adam(model.parameters(), lr=lr, weight_decay=wd)
    adj = torch.tensor(c["adj"], device=cuda)
    names = ("table", "W1", "b1", "W2", "b2")
    ref = [torch.tensor(np.asarray(c[k], np.float64), device=cuda, requires_grad=True)
           for k in names]
    ref_opt = torch.optim.Adam(ref, lr=lr, weight_decay=wd)
    adj64 = adj.double()
    p0 = {k: np.asarray(c[k], np.float64) for k in names}
    emax = {k: np.zeros_like(v) for k, v in p0.items()}
    rng = np.random.default_rng(11)
    batches = [(R.make_batch(B, c["rows"], c["seed"] + t), rng.integers(0, widths[2], B))
               for t in range(1, 4)]

    def ref_loss(src, target):
        table, W1, b1, W2, b2 = ref
        x = torch.relu(torch.nn.functional.linear(table[src], W1, b1))
        x = torch.relu(torch.nn.functional.linear(torch.mul(adj64[src], x), W2, b2))
        return torch.nn.functional.nll_loss(torch.log_softmax(x, dim=1), target)

    first = None
    for t, (src, target) in enumerate(batches, 1):
        # the oracle at the reference's parameters: kinks, and the gradients' A and n
        cc = dict(c, src=src, **{k: v.detach().cpu().numpy() for k, v in zip(names, ref)})
        f, g = R.reference(cc, R.nll_dlogp(target, widths[2]))
        r1, r2 = R.kink_ratio(f)
        assert r1 >= 1e-5 and r2 >= 1e-5, (t, r1, r2)
        for k, gk in zip(names, GRADS):
            gp = g[gk] + wd * cc[k]
            bound = 1e-5 * np.abs(g[gk]) + 4 * np.sqrt(g["n_" + gk]) * u * g["A_" + gk]
            with np.errstate(divide="ignore"):
                e = np.divide(bound, np.abs(gp), out=np.zeros_like(bound), where=bound > 0)
            emax[k] = np.maximum(emax[k], e)
        ts, tt = torch.tensor(src, device=cuda), torch.tensor(target, device=cuda)
        ref_opt.zero_grad()
        want = ref_loss(ts, tt)
        want.backward()
        ref_opt.step()
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(model(ts, adj), tt)
        loss.backward()
        opt.step()
        rows = np.arange(B)
        bounded_close([float(loss.detach())], [float(want.detach())],
                      f["A_logp"][rows, target].mean(), f["n_logp"][rows, target].max() + B,
                      1e-5, f"adam step {t} loss")
        first = float(loss.detach()) if first is None else first
    # the first batch again: lower than before the three steps
    with torch.no_grad():
        after = float(torch.nn.functional.nll_loss(
            model(torch.tensor(batches[0][0], device=cuda), adj),
            torch.tensor(batches[0][1], device=cuda)))
    assert after < first
    for k, p, r in zip(names, model.parameters(), ref):
        bounded_close(p.detach().cpu().numpy(), r.detach().cpu().numpy(),
                      np.abs(p0[k]) + 3 * lr, 12, 1e-5, f"adam x3 {k}",
                      floor=np.minimum(12 * lr * emax[k], 3 * lr))


def test_forward_backward_in_one_graph(cuda, msha):
    """One captured forward + backward (check=False: nothing is read back), replayed over
    three batches, bitwise equal to eager."""
    from msha_gnn_amd import functional as MF

    widths, B = (32, 32, 32), 130
    c, _ = _case(widths, B)
    leaves, _, adj, g, vals = _dev(c, cuda)
    rng = np.random.default_rng(5)

    def batch(k):
        src = R.make_batch(B, c["rows"], c["seed"] + 10 + k)
        return (torch.tensor(src, device=cuda),
                torch.tensor(rng.standard_normal((B, widths[2])).astype(np.float32), device=cuda))

    def step(src, dlogp):
        logp = MF.sage_forward(leaves[0], src, g, vals, *leaves[1:], check=False)
        grads = torch.autograd.grad(logp, leaves, grad_outputs=dlogp)
        return (logp.detach(),) + grads  # (no autograd graph outlives the step)

    # The warm-up's results are dropped before the capture (its autograd graph would hold
    # nodes made on the default stream).  What the graph reads and writes stays alive for the
    # whole test: the leaves, the graph's arrays, vals, the static batch, the captured outputs.
    statics = batch(0)
    step(*statics)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*statics)
    for k in range(1, 4):
        new = batch(k)
        for s, t in zip(statics, new):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*new)
        for got, want in zip(outs, eager):
            assert torch.equal(_bits(got), _bits(want))
