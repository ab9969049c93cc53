"""The column pass that carries the projection's weight gradient
(msha_edge_attention_bwd_fused_wgrad + msha_wgrad_reduce) against the two launches it
replaces, and the Python hand-off between project_scores and edge_attention."""
import numpy as np
import pytest
import torch

from gpu_helpers import bounded_close

CYC = (0, 1, 8, 9, 17, 40, 3, 5)  # column degrees: empty, one trip, trip edges, several trips


CYC_V = (0, 7, 8, 16, 39, 2, 4, 0)  # the same with one edge of every column in a virtual row


def _square_graph(n, dev):
    """n x n graph, chunks of 512 slots (no multi-chunk column).  n >= 3000: column degrees
    CYC[j % 8] (empty columns included) and a stretch of 400 mostly empty columns, so one
    block's range spans several tiles; no virtual row.  n < 3000: row 5 is an empty row of
    the mask, held as a virtual full row (an edge to every column, flagged), and the other
    rows give the columns CYC_V[j % 8] more.  Columns j % 8 == 6 also take one edge from each
    row that would otherwise be empty."""
    from msha_gnn_amd.graph import Graph

    virt = n < 3000
    deg = np.array([(CYC_V if virt else CYC)[j % 8] for j in range(n)], np.int64)
    if n >= 3000:
        deg[2000:2400] = np.where(np.arange(400) % 8 == 2, 1, 0)
    rows = [np.array([(j * 7 + k * 13 + 1) % n for k in range(deg[j])], np.int64) for j in range(n)]
    cols = [np.full(deg[j], j, np.int64) for j in range(n)]
    r, c = np.concatenate(rows), np.concatenate(cols)
    if virt:
        keep = r != 5
        r, c = np.concatenate([r[keep], np.full(n, 5)]), np.concatenate([c[keep], np.arange(n)])
    lonely = np.setdiff1d(np.arange(n), r)
    fix = np.nonzero(np.arange(n) % 8 == 6)[0]
    r = np.concatenate([r, lonely])
    c = np.concatenate([c, fix[np.arange(len(lonely)) % len(fix)]])
    assert len(np.unique(r * n + c)) == len(r)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    perm = np.argsort(c, kind="stable")
    colptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=n), out=colptr[1:])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.int32), device=dev)  # noqa: E731
    flag = np.zeros(n, np.uint8)
    flag[5] = 1 if virt else 0
    g = Graph(n, n, t(rowptr), t(c), torch.as_tensor(flag, device=dev), t(colptr), t(r[perm]),
              t(perm), chunk=512)
    assert g._plan["n_multi"] == 0
    cdeg = np.diff(colptr)
    assert ({1, 8, 9, 17, 40} if virt else {0, 1, 8, 9, 17, 40}) <= set(cdeg.tolist())
    return g


_GRAPHS: dict = {}


def _graph(n, dev):
    if n not in _GRAPHS:
        _GRAPHS[n] = _square_graph(n, dev)
    return _GRAPHS[n]


def _params(n, H, F, dev, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed + n + H)
    X = torch.rand(n, 128, generator=g).to(dev, dtype)
    W = (torch.randn(128, H * F, generator=g) * 128 ** -0.5).to(dev, dtype).requires_grad_(True)
    al = torch.randn(H, F, generator=g).to(dev).requires_grad_(True)
    ar = torch.randn(H, F, generator=g).to(dev).requires_grad_(True)
    dU = torch.randn(n, H, F, generator=g).to(dev, dtype)
    return X, W, al, ar, dU


def _step(MF, graph, X, W, al, ar, dU, H, p, pass_ar=True, second=False, hook=False):
    """One project_scores -> edge_attention -> backward; returns the gradients, the layer
    output and the column-side gradients autograd carried."""
    for q in (W, al, ar):
        q.grad = None
    h, el, er = MF.project_scores(X, W, al, ar, heads=H)
    hc = h.view(X.shape[0], H, -1)
    for q in (hc, el, er):
        q.retain_grad()
    if hook:
        hc.register_hook(lambda g: g * 1.0)  # a new tensor with the same values
    out = MF.edge_attention(graph, el, er, hc, p=p, training=p > 0, seed=1234,
                            ar=ar if pass_ar else None)
    if second:
        (out.to(torch.float32) * dU.to(torch.float32)).sum().add(h.sum() * 0.5).backward()
    else:
        out.backward(dU)
    return dict(dW=W.grad, dal=al.grad, dar=ar.grad, u=out.detach(), d_hc=hc.grad, d_el=el.grad,
                d_er=er.grad, h=h.detach())


def _equal(a, b, names):
    for k in names:
        assert torch.equal(a[k], b[k]), k


def _check_wgrad(r, X, al, ar, H, F, name):
    """dW, dal, dar against the fp64 restatement over the gradients the pass itself wrote."""
    n = X.shape[0]
    f64 = lambda x: x.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    Xn, d_hc, d_el, d_er, h = f64(X), f64(r["d_hc"]).reshape(n, -1), f64(r["d_el"]), \
        f64(r["d_er"]), f64(r["h"])
    a1, a2 = f64(al).reshape(-1), f64(ar).reshape(-1)
    e1, e2 = np.repeat(d_el, F, 1), np.repeat(d_er, F, 1)
    tot = d_hc + e1 * a1 + e2 * a2
    mag = np.abs(d_hc) + np.abs(e1 * a1) + np.abs(e2 * a2)
    worst = {}
    worst["dW"], _ = bounded_close(f64(r["dW"]), Xn.T @ tot, np.abs(Xn).T @ mag, n + 64, 1e-5,
                                   f"dW[{name}]")
    worst["dal"], _ = bounded_close(f64(r["dal"]).reshape(-1), (e1 * h).sum(0),
                                    (np.abs(e1) * np.abs(h)).sum(0), n + 64, 1e-5, f"dal[{name}]")
    worst["dar"], _ = bounded_close(f64(r["dar"]).reshape(-1), (e2 * h).sum(0),
                                    (np.abs(e2) * np.abs(h)).sum(0), n + 64, 1e-5, f"dar[{name}]")
    print(f"{name}: worst / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("pass_ar", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("n", [1045, 4099])
@pytest.mark.parametrize("H,F", [(8, 16), (2, 64), (4, 32), (1, 128)])
def test_fused_wgrad(cuda, msha, monkeypatch, H, F, n, p, pass_ar):
    """8 x 16 (head-per-lane column pass) and 2 x 64, 4 x 32, 1 x 128 (quad-per-lane) on a
    square graph: the column pass carries the weight gradient (route query and call
    counters), d_hc / d_er / d_el / u are the two-launch bits, dW / dal / dar meet the fp64
    restatement's bound, and a second run gives the same bits."""
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    monkeypatch.setenv("MSHA_ROWTERMS", "1")
    graph = _graph(n, cuda)
    X, W, al, ar, dU = _params(n, H, F, cuda)
    nb = int(_lib.fn("msha_edge_attention_bwd_fused_wgrad_route")(
        graph.desc, H, F, 0, 128, 128, 1, 1, X.data_ptr(), al.data_ptr(), ar.data_ptr()))
    assert nb == 256
    cut = graph.col_ranges(nb).cpu().numpy()
    if n < 3000:
        assert (np.diff(cut) == 1).any(), "a range that is a single column"
    assert (np.diff(cut) % 48 != 0).any()  # range ends inside a tile
    if n >= 3000:
        assert np.diff(cut).max() > 96  # one block walks several tiles
    assert nb > (n + 15) // 16 or n >= 3000  # more blocks than 16-column tiles at 1,045

    monkeypatch.setenv("MSHA_BWD_WGRAD", "0")
    before = dict(MF.WGRAD_FUSED_CALLS)
    off = _step(MF, graph, X, W, al, ar, dU, H, p, pass_ar)
    assert MF.WGRAD_FUSED_CALLS == before
    monkeypatch.setenv("MSHA_BWD_WGRAD", "1")
    on = _step(MF, graph, X, W, al, ar, dU, H, p, pass_ar)
    assert MF.WGRAD_FUSED_CALLS == {"cols": before["cols"] + 1, "reduce": before["reduce"] + 1}
    _equal(on, off, ("u", "d_hc", "d_er", "d_el"))
    _check_wgrad(on, X, al, ar, H, F, f"{H}x{F}, {n}, p={p}")
    again = _step(MF, graph, X, W, al, ar, dU, H, p, pass_ar)
    _equal(again, on, ("dW", "dal", "dar", "d_hc", "d_er", "d_el"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["second_consumer", "hook", "bf16", "bipartite", "4x16",
                                  "frozen_W"])
def test_fused_wgrad_not_taken(cuda, msha, monkeypatch, case):
    """Where the slabs would not be the weight gradient of what autograd hands the
    projection (h has a second consumer, a hook replaced d_hc), or the library does not cover
    the call (bf16, a bipartite graph whose recipient projection carries the tag, 4 x 16), or
    W wants no gradient (no tag: the column pass does no extra work), the projection's backward
    runs its own weight gradient: every gradient equals the knob-off run bit for bit."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import Graph

    monkeypatch.setenv("MSHA_ROWTERMS", "1")
    n = 1045
    H, F = (4, 16) if case == "4x16" else (8, 16)
    p = 0.0
    dtype = torch.bfloat16 if case == "bf16" else torch.float32
    X, W, al, ar, dU = _params(n, H, F, cuda, dtype)
    if case == "frozen_W":
        W.requires_grad_(False)
    kw = dict(second=case == "second_consumer", hook=case == "hook")
    if case == "bipartite":
        m = 32 * 40
        rng = np.random.default_rng(3)
        col = np.concatenate([np.sort(rng.choice(m, 12, replace=False)) for _ in range(n)])
        graph = Graph.from_csr(np.arange(n + 1) * 12, col, m, cuda)
        Xr = torch.rand(m, 128, device=cuda)

        def run():
            for q in (W, al, ar):
                q.grad = None
            h1, _, er = MF.project_scores(Xr, W, al, ar, heads=H)  # tagged: al and ar
            assert getattr(h1, "_msha_proj", None) is not None
            h2, el = MF.project_scores(X, W, al=al, heads=H)
            out = MF.edge_attention(graph, el, er, h1.view(m, H, F), p=p, ar=ar)
            out.backward(dU)
            return dict(dW=W.grad, dal=al.grad, dar=ar.grad, u=out.detach())
    else:
        graph = _graph(n, cuda)

        def run():
            return _step(MF, graph, X, W, al, ar, dU, H, p, **kw)

    monkeypatch.setenv("MSHA_BWD_WGRAD", "0")
    off = run()
    monkeypatch.setenv("MSHA_BWD_WGRAD", "1")
    before = dict(MF.WGRAD_FUSED_CALLS)
    on = run()
    assert MF.WGRAD_FUSED_CALLS["reduce"] == before["reduce"]
    if case not in ("second_consumer", "hook"):
        assert MF.WGRAD_FUSED_CALLS["cols"] == before["cols"]
    _equal(on, off, ("dal", "dar", "u") if case == "frozen_W" else ("dW", "dal", "dar", "u"))


@pytest.mark.gpu
def test_fused_wgrad_graph_replay(cuda, msha, monkeypatch):
    """One step captured into a HIP graph and replayed twice gives the eager bits."""
    from msha_gnn_amd import functional as MF

    monkeypatch.setenv("MSHA_ROWTERMS", "1")
    monkeypatch.setenv("MSHA_BWD_WGRAD", "1")
    n, H, F = 1045, 8, 16
    graph = _graph(n, cuda)
    X, W, al, ar, dU = _params(n, H, F, cuda)

    def step():
        for q in (W, al, ar):
            q.grad = None
        h, el, er = MF.project_scores(X, W, al, ar, heads=H)
        out = MF.edge_attention(graph, el, er, h.view(n, H, F), p=0.3, training=True, seed=77,
                                ar=ar)
        out.backward(dU)

    step()
    eager = [q.grad.clone() for q in (W, al, ar)]
    before = MF.WGRAD_FUSED_CALLS["reduce"]
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        step()
    assert MF.WGRAD_FUSED_CALLS["reduce"] == before + 1
    for _ in range(2):
        for q in (W, al, ar):
            q.grad.fill_(7.0)
        cg.replay()
        torch.cuda.synchronize()
        for q, e in zip((W, al, ar), eager):
            assert torch.equal(q.grad, e)
