"""OursLayer2 / ablation2 on the GPU (Ablation.py:140-231): the split intra core against
the dense fp64 restatement (tests/ablation_ref.py, tied to the reference by
tests/test_ablation_host.py) with the kernels' own Philox masks, the layer and the model
against the reference's own outputs (tests/golden/ablations.npz), and the model inside the
training loops.

Tolerances are the ones the Ours tests hold: 1e-5 of each tensor's scale for
fp32 outputs and golden gradients, 1e-4 for the Ours kernels' gradients against fp64, 1e-2
for bf16 tables.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from gpu_helpers import t, tol_close

import ablation_ref as AR

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- split intra core ---
def _split_inputs(B):
    """test_ours_attention_kernels_vs_dense's shape: province groups of ~250 members (a
    gather chunk is 64), two virtual rows, repeated sources."""
    rng = np.random.default_rng(21)
    n, m, H, Fd = 1500, 32, 2, 64
    counts = np.zeros((n, m), np.float32)
    for i in range(n):
        k = int(rng.integers(1, 8))
        counts[i, rng.choice(m, k, replace=False)] = 1
    counts[[7, 100]] = 0  # virtual rows (uniform attention)
    city = rng.integers(0, 60, n)
    prov = city // 10
    src = rng.integers(0, n, B)
    src[:4] = [7, 7, 100, 3]  # repeats + virtual rows in the batch
    src[-1] = 3
    tabs = dict(el=rng.standard_normal((n, H)), er=rng.standard_normal((m, H)),
                h1=rng.standard_normal((m, H, Fd)) * 0.3, h2=rng.standard_normal((n, H, Fd)) * 0.3,
                a3s=rng.standard_normal((H, Fd)) * 0.2, a4s=rng.standard_normal((H, Fd)) * 0.2,
                dU=rng.standard_normal((n, H, Fd)), dV=rng.standard_normal((m, H, Fd)))
    return counts, city, prov, src, tabs


def _run_split(cuda, graph, groups, src, tabs, dtype, p, seed, split=True):
    from msha_gnn_amd import functional as MF

    tg = [t(tabs[k], cuda).requires_grad_(True) for k in ("el", "er", "h1", "h2", "a3s", "a4s")]
    tg[2] = t(tabs["h1"], cuda, dtype).requires_grad_(True)
    tg[3] = t(tabs["h2"], cuda, dtype).requires_grad_(True)
    if split:
        u, v = MF.ours_split_attention(graph, groups, torch.as_tensor(src, device=cuda), *tg,
                                       p=p, training=p > 0, seed=seed)
    else:  # the inter attention alone
        u, v = MF.edge_attention(graph, tg[0], tg[1], tg[2], hs=tg[3], p=p, training=p > 0,
                                 seed=seed)
    (u.float() * t(tabs["dU"], cuda)).sum().add_((v.float() * t(tabs["dV"], cuda)).sum()).backward()
    return u.detach(), v.detach(), tg


@pytest.mark.parametrize("dtype,tol_out,tol_grad", [(torch.float32, 1e-5, 1e-4),
                                                    (torch.bfloat16, 1e-2, 1e-2)],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [48, 130])
@pytest.mark.parametrize("p", [0.0, 0.4])
def test_split_core_vs_dense(cuda, msha, p, B, dtype, tol_out, tol_grad):
    """ours_split_attention: u, v and every gradient against ablation_ref with the
    kernels' masks; B = 130 takes the batch loop (three 64-entry ballots).  The weights
    hang on no table, so the el / er gradients are those of the inter attention alone, bit
    for bit, and a3s / a4s get exact zeros; two runs give the same bits."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import Graph, Groups

    counts, city, prov, src, tabs = _split_inputs(B)
    n, m = counts.shape
    H = tabs["el"].shape[1]
    if dtype != torch.float32:  # the values the bf16 kernels read
        for k in ("h1", "h2", "dU", "dV"):
            tabs[k] = torch.as_tensor(tabs[k]).to(dtype).double().numpy()
    graph = Graph.from_dense(t(counts, cuda))
    groups = Groups(city, prov, cuda)
    seed = 5
    u, v, tg = _run_split(cuda, graph, groups, src, tabs, dtype, p, seed)
    assert u.dtype == dtype and v.dtype == dtype
    u2, v2, tg2 = _run_split(cuda, graph, groups, src, tabs, dtype, p, seed)
    assert torch.equal(u, u2) and torch.equal(v, v2)
    for a, b in zip(tg, tg2):
        assert torch.equal(a.grad, b.grad)
    _, v_i, tg_i = _run_split(cuda, graph, groups, src, tabs, dtype, p, seed, split=False)
    assert torch.equal(v, v_i)
    assert torch.equal(tg[0].grad, tg_i[0].grad), "d_el differs from the inter attention's"
    assert torch.equal(tg[1].grad, tg_i[1].grad), "d_er differs from the inter attention's"
    assert torch.equal(tg[2].grad, tg_i[2].grad)
    assert tg[4].grad.shape == tg[4].shape and not tg[4].grad.any() and not tg[5].grad.any()
    mask = torch.as_tensor(counts > 0)
    full = mask.clone()
    full[~full.any(1)] = True
    rows, cols = torch.nonzero(full, as_tuple=True)
    E = len(rows)
    keep_all = None
    if p > 0:
        keep_all = MF.dropout_keep_mask(E * H, p, seed, cuda).cpu().numpy().reshape(E, H)
    for h in range(H):
        rs = [torch.tensor(tabs[k][:, h], dtype=torch.float64, requires_grad=True)
              for k in ("el", "er", "h1", "h2")]
        ke = k3 = k4 = None
        if p > 0:
            ke = torch.zeros(n, m, dtype=torch.float64)
            ke[rows, cols] = torch.as_tensor(keep_all[:, h], dtype=torch.float64)
            k3, k4 = (torch.as_tensor(
                MF.dropout_keep_mask(B * n, p, seed, cuda, offset=1 + h // 2,
                                     word=2 * (h % 2) + kind).cpu().numpy().reshape(B, n),
                dtype=torch.float64) for kind in (0, 1))
        ru, rv = AR.dense_split_core(*rs, mask, torch.as_tensor(city), torch.as_tensor(prov),
                                     torch.as_tensor(src), ke, k3, k4, p)
        tol_close(u[:, h].float().cpu().numpy(), ru.detach().numpy(), tol_out, tol_out)
        tol_close(v[:, h].float().cpu().numpy(), rv.detach().numpy(), tol_out, tol_out)
        ((ru * torch.tensor(tabs["dU"][:, h])).sum()
         + (rv * torch.tensor(tabs["dV"][:, h])).sum()).backward()
        atol_rel = 1e-5 if tol_grad < 1e-3 else tol_grad
        for k in range(4):
            tol_close(tg[k].grad[:, h].float().cpu().numpy(), rs[k].grad.numpy(), tol_grad,
                      atol_rel)


# ------------------------------------------------- layers and models vs the reference ---
def _adjacencies(msha, cuda, counts):
    o = golden("ours_small.npz")
    inter = msha.normalize_adjacency_matrix(t(counts, cuda))
    city = torch.as_tensor((o["city"][:, None] == o["city"][None, :]).astype(np.float32),
                           device=cuda)
    prov = torch.as_tensor((o["prov"][:, None] == o["prov"][None, :]).astype(np.float32),
                           device=cuda)
    return inter, city, prov


def _zero_grad_names(name):
    """Parameters whose reference gradient is rounding noise around an exact 0 (the score
    is constant along its softmax row: OursLayer2's a3 / a4, test_ablation_host.py; the
    GraphAttentionLayer's a, layers.GraphAttentionLayer) and is an exact 0 here."""
    return name.endswith(".a3") or name.endswith(".a4") or name in ("a3", "a4", "out_att.a")


@pytest.mark.parametrize("tag", ["", "B."])
def test_ours_layer2_matches_reference(cuda, msha, tag):
    from msha_gnn_amd import layers

    z = golden("ablations.npz")
    o = golden("ours_small.npz")
    counts = o[tag + "counts"] if tag + "counts" in o.files else o["counts"]
    torch.manual_seed(10)
    layer = layers.OursLayer2(16, 8, 0.0).to(cuda)
    inter, city, prov = _adjacencies(msha, cuda, counts)
    S = t(z[tag + "S"], cuda).requires_grad_(True)
    R = t(z[tag + "R"], cuda).requires_grad_(True)
    src = torch.as_tensor(z[tag + "source_index"], device=cuda)
    layer.eval()
    with torch.no_grad():
        y = layer(S, R, inter, city, prov, src)
    tol_close(y.cpu().numpy(), z[tag + "out_eval"], 1e-5, 1e-5)
    layer.train()
    y = layer(S, R, inter, city, prov, src)
    tol_close(y.detach().cpu().numpy(), z[tag + "out"], 1e-5, 1e-5)
    y.backward(t(z[tag + "dout"], cuda))
    tol_close(S.grad.cpu().numpy(), z[tag + "grad.S"], 1e-5, 1e-5)
    tol_close(R.grad.cpu().numpy(), z[tag + "grad.R"], 1e-5, 1e-5)
    for k, p in layer.named_parameters():
        key = f"{tag}grad.{k}"
        if _zero_grad_names(k):
            assert p.grad is not None and not p.grad.any(), k
        elif key in z.files:
            tol_close(p.grad.cpu().numpy(), z[key], 1e-5, 1e-5)
        else:
            assert p.grad is None, k


def _model(msha, cuda, tag="a2.", dropout=0.0):
    from msha_gnn_amd import layers

    z = golden("ablations.npz")
    n, m = z[tag + "logp"].shape
    gdp = {i: float(x) for i, x in enumerate(z["gdp"])}
    model = layers.ablation2(16, 8, m, 2, dropout, gdp, n, m)
    sd = {k[len(tag + "state."):]: torch.as_tensor(z[k]) for k in z.files
          if k.startswith(tag + "state.")}
    model.load_state_dict(sd, strict=True)
    return z, model.to(cuda)


def test_ablation2_matches_reference(cuda, msha, tag="a2."):
    """Log-probabilities in eval and train mode, the loss and every gradient, from the
    fixture's state_dict (strict)."""
    z, model = _model(msha, cuda, tag)
    inter, city, prov = _adjacencies(msha, cuda, golden("ours_small.npz")["counts"])
    si = torch.as_tensor(z[tag + "source_index"], device=cuda)
    ri = torch.as_tensor(z[tag + "recipient_index"], device=cuda)
    model.eval()
    with torch.no_grad():
        lp = model(inter, city, prov, si)
    tol_close(lp.cpu().numpy(), z[tag + "logp_eval"], 1e-5, 1e-5)
    with torch.no_grad():  # the record arguments are accepted and ignored
        lp2 = model(inter, city, prov, si, record=True, Coeff12=torch.zeros_like(inter),
                    Coeff3=None, Coeff4=None)
    assert torch.equal(lp, lp2)
    model.train()
    out = model(inter, city, prov, si)
    tol_close(out.detach().cpu().numpy(), z[tag + "logp"], 1e-5, 1e-5)
    loss = F.nll_loss(out[si], ri)
    ref = float(z[tag + "loss"])
    assert abs(float(loss.detach()) - ref) <= 1e-5 * max(1.0, abs(ref))
    loss.backward()
    for k, p in model.named_parameters():
        key = f"{tag}grad.{k}"
        if _zero_grad_names(k):
            assert p.grad is not None and not p.grad.any(), k
        elif key in z.files:
            tol_close(p.grad.cpu().numpy(), z[key], 1e-5, 1e-5)
        else:
            assert p.grad is None, k


# --------------------------------------------------------------------- integration ---
def test_ablation2_uses_the_fused_head(cuda, msha, tag="a2."):
    """Training (eager and inside the replay path's captured forward) and no_grad route
    the tail through the fused head; eval with autograd takes the unfused composition."""
    from msha_gnn_amd import layers, replay

    name = "model_head"

    class Probe:
        calls = 0
        captured = 0

    orig = getattr(layers.MF, name)

    def probe(*a, **k):
        Probe.calls += 1
        Probe.captured += int(torch.cuda.is_current_stream_capturing())
        return orig(*a, **k)

    z, model = _model(msha, cuda, tag, dropout=0.5)
    inter, city, prov = _adjacencies(msha, cuda, golden("ours_small.npz")["counts"])
    src = torch.as_tensor(z[tag + "source_index"], device=cuda)
    setattr(layers.MF, name, probe)
    prev = replay.REPLAY
    try:
        model.train()
        replay.REPLAY = False
        model(inter, city, prov, src).sum().backward()
        assert Probe.calls == 1 and Probe.captured == 0
        replay.REPLAY = True
        model(inter, city, prov, src).sum().backward()
        assert model.__dict__.get("_msha_graphs"), "replay path not taken"
        assert Probe.captured == 1, "captured forward did not route through the fused head"
        before = Probe.calls
        model(inter, city, prov, src).sum().backward()  # pure replay: no Python head call
        assert Probe.calls == before
        model.eval()
        with torch.no_grad():
            model(inter, city, prov, src)
        assert Probe.calls == before + 1
        out = model(inter, city, prov, src)  # eval with autograd: the unfused tail
        assert Probe.calls == before + 1 and out.requires_grad
    finally:
        setattr(layers.MF, name, orig)
        replay.REPLAY = prev


def test_graphed_step_replays_the_eager_step(cuda, msha, tag="a2."):
    """One training step at dropout 0.5 inside step.GraphedStep replays to the eager step's
    loss: the same seeds (torch's CPU generator, drawn in the same order) and the same
    replay-counter values (1 for the warm-up step, 2 for the compared one)."""
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import replay
    from msha_gnn_amd.step import GraphedStep

    inter, city, prov = _adjacencies(msha, cuda, golden("ours_small.npz")["counts"])
    losses = {}
    prev = replay.REPLAY
    replay.REPLAY = False  # the whole step is the graph here, not the model's own replay
    try:
        for graphed in (False, True):
            z, model = _model(msha, cuda, tag, dropout=0.5)
            si = torch.as_tensor(z[tag + "source_index"], device=cuda)
            ri = torch.as_tensor(z[tag + "recipient_index"], device=cuda)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-4,
                                   capturable=True)
            model.train()

            def body():
                opt.zero_grad(set_to_none=True)
                loss = MF.nll_loss_rows(model(inter, city, prov, si), si, ri)
                loss.backward()
                opt.step()
                return loss

            torch.manual_seed(123)
            if graphed:
                gs = GraphedStep(body, cuda, warmup=1)
                losses[graphed] = float(gs.replay().detach())
                gs.close()
            else:
                ctr = torch.zeros(1, dtype=torch.int64, device=cuda)
                old = MF.set_rng_counter(ctr)
                try:
                    ctr.fill_(1)
                    body()  # the graphed run's warm-up step
                    ctr.fill_(2)
                    losses[graphed] = float(body().detach())
                finally:
                    MF.set_rng_counter(old, cuda)
    finally:
        replay.REPLAY = prev
    assert np.isfinite(losses[True])
    np.testing.assert_allclose(losses[True], losses[False], rtol=1e-6)


@pytest.fixture()
def sub512_dir(tmp_path):
    from msha_gnn_amd import trainpy

    z = golden("sub512.npz")
    rng = np.random.default_rng(0)
    trainpy.write_year(str(tmp_path), "2015", rng.integers(0, 40, 512), rng.integers(0, 9, 512),
                       z["gdp"], z["flows"], 32)
    return str(tmp_path)


def test_train_py_runs_ablation2(cuda, msha, sub512_dir, kind="ablation2"):
    """train.py with line 206 changed to the model: three iterations on one batch at dropout
    0 (deterministic) have finite losses that do not rise (each within 0.1 % of the one
    before, or below it)."""
    from msha_gnn_amd import trainpy

    z = golden("sub512.npz")
    batch = (torch.as_tensor(z["source_index"]), torch.as_tensor(z["recipient_index"]))
    with trainpy.namespace(sub512_dir, cuda) as ns:
        tp = trainpy.TrainPy(ns, cuda, dropout=0.0, model_kind=kind)
        assert type(tp.model).__name__ == kind
        losses = [tp.iteration(batch) for _ in range(3)]
    assert np.isfinite(losses).all(), losses
    for a, b in zip(losses, losses[1:]):
        assert b <= a * (1 + 1e-3), losses
