"""Host-side checks of the link-prediction distillation path: the numpy references
(``distill_ref``) against torch fp64, the pinned fp32 decisions of the rank term, the ABI's
size queries and argument errors (no launch), and the Python surface's argument checks."""
import numpy as np
import pytest
import torch

import distill_ref as D
import link_ref as R

F32, BF16 = 0, 1  # MSHA_DTYPE_*


def _case(seed=0, A=9, K=7, n=20, F=8):
    """A small list with padding slots (anchor -1 and n, a -1 mid-row, a row with one valid
    slot) and tied teacher logits (multiples of 1/4)."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n, F)) * 0.6
    anchors = rng.integers(0, n, A)
    ctx = rng.integers(0, n, (A, K))
    anchors[2], anchors[5] = -1, n
    ctx[0, 3] = -1
    ctx[1, :] = n + 3
    ctx[1, 4] = 2
    t = np.round(rng.standard_normal((A, K)) * 4) / 4
    t[3, :] = 0.5  # every teacher logit of the anchor equal
    return h, anchors, ctx, t


def _torch_composition(h, anchors, ctx, t, margin, tau, w):
    """torch fp64 autograd of the composition over the valid slots: (terms, loss, dH, g)."""
    import torch.nn.functional as TF

    A, K = ctx.shape
    n = h.shape[0]
    valid = D.valid_slots(anchors, ctx, n)
    ht = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    ys, LR, LD, LP = [], 0.0, 0.0, 0.0
    for a in range(A):
        ks = np.flatnonzero(valid[a])
        if len(ks) == 0:
            ys.append(None)
            continue
        y = (ht[int(anchors[a])][None, :] * ht[torch.as_tensor(ctx[a, ks])]).sum(-1)
        y.retain_grad()
        ys.append(y)
        ta = torch.as_tensor(t[a, ks], dtype=torch.float64)
        i, j = np.triu_indices(len(ks), 1)
        if len(i):
            d = ta[i] - ta[j]
            r = torch.where(d.abs() > margin, torch.sign(d), torch.zeros_like(d))
            LR = LR + TF.margin_ranking_loss(y[i], y[j], r, margin=margin, reduction="sum")
        LD = LD + TF.kl_div(torch.log_softmax(y / tau, 0), torch.softmax(ta / tau, 0),
                            reduction="sum")
        LP = LP + TF.mse_loss(torch.sigmoid(y), torch.sigmoid(ta), reduction="sum")
    loss = (w[0] * LR + w[1] * LD + w[2] * LP) / A
    loss.backward()
    g = np.zeros((A, K))
    for a in range(A):
        if ys[a] is not None:
            g[a, np.flatnonzero(valid[a])] = ys[a].grad.numpy()
    terms = np.array([float(torch.as_tensor(x).detach()) for x in (LR, LD, LP)]) / A
    return terms, float(loss.detach()), ht.grad.numpy(), g, valid


@pytest.mark.parametrize("w", [(1.0, 1.0, 0.0), (0.7, 1.3, 2.0)])
def test_reference_matches_torch_fp64(w):
    margin, tau = 0.1, 0.8
    h, anchors, ctx, t = _case()
    terms, loss, dH, g, valid = _torch_composition(h, anchors, ctx, t, margin, tau, w)
    src, dst = D.flat_pairs(anchors, ctx)
    y, _, ok = R.logits(h, src, dst)
    assert np.array_equal(ok.reshape(ctx.shape), valid)
    assert valid[1].sum() == 1 and not valid[2].any() and not valid[0, 3]
    ref = D.distill(y.reshape(ctx.shape), t, valid, margin, tau, w, pinned=False)
    np.testing.assert_allclose(ref["terms"], terms, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref["loss"], loss, rtol=1e-12)
    np.testing.assert_allclose(ref["g"], g, rtol=1e-11, atol=1e-15)
    got_dH, _, _ = R.table_grad(h, src, dst, ref["g"].reshape(-1))
    np.testing.assert_allclose(got_dH, dH, rtol=1e-11, atol=1e-15)
    # all teacher logits equal: every pair adds the constant margin and no gradient
    assert np.isclose(ref["LR"][3], margin * 7 * 6 / 2) and (ref["c"][3] == 0).all()
    assert (ref["g"][~valid] == 0).all() and ref["c"].dtype == np.int64
    # the multiples of 1/4 sit far from the margin: the fp32 rule takes the same decisions
    pin = D.distill(y.reshape(ctx.shape), t, valid, margin, tau, w, pinned=True)
    assert np.array_equal(pin["c"], ref["c"])
    np.testing.assert_allclose(pin["terms"], ref["terms"], rtol=1e-6)
    # the torch restatement of the smooth parts, in fp64, is the same function
    LD, LP, gs = D.smooth_torch(y.reshape(ctx.shape), t, valid, tau, w, torch.float64)
    np.testing.assert_allclose(LD, ref["LD"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(LP, ref["LP"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(gs, ref["g_smooth"], rtol=1e-10, atol=1e-15)


def test_pinned_decisions_one_ulp_either_side_of_the_margin():
    """The rule: d = fl32(t_i - t_j) and |d| > fl32(margin); fl32(fl32(margin) - r fl32(y_i -
    y_j)) > 0.  Pairs whose difference is fl32(margin) exactly and one ulp either side."""
    margin = 0.1
    m = np.float32(margin)
    up, down = np.nextafter(m, np.float32(1)), np.nextafter(m, np.float32(0))
    assert down < m < up and float(m) != margin  # 0.1 is not an fp32 number
    # slots 0..3: t = 0, m, up, down (differences from slot 0 are exact)
    t = np.array([[0, m, up, down]], np.float32)
    r = D.rank_sign(t, margin)
    assert r[0, 1, 0] == 0 and r[0, 0, 1] == 0          # |d| == fl32(margin): not beyond it
    assert r[0, 2, 0] == 1 and r[0, 0, 2] == -1         # one ulp above
    assert r[0, 3, 0] == 0 and r[0, 0, 3] == 0          # one ulp below
    assert (r == -np.swapaxes(r, 1, 2)).all() and (np.diagonal(r, 0, 1, 2) == 0).all()
    # in fp64 with the decimal 0.1, fl32(0.1) - 0 = 0.100000001... > 0.1: the other decision
    assert abs(float(m) - 0.0) > margin
    # hinge: with r = 1 the argument is m - (y_i - y_j): zero at y_i - y_j == m (inactive),
    # positive one ulp below, negative one ulp above
    y = np.array([[m, 0, up, down]], np.float32)
    ones = np.ones((1, 4, 4), np.float32)
    act = D.hinge_active(y, ones, margin)
    assert not act[0, 0, 1] and not act[0, 2, 1] and act[0, 3, 1]
    # r = 0 leaves the constant margin: active as an argument, no gradient (distill masks it)
    assert D.hinge_active(y, 0 * ones, margin).all()
    # the counts and the loss follow these decisions
    valid = np.ones((1, 4), bool)
    out = D.distill(y, t, valid, margin, 1.0, (1.0, 0.0, 0.0))
    # only the pairs with slot 2 rank (t_2 - t_0 = up): r_20 = 1; r_21, r_23 = 0 (2 ulp apart)
    assert (out["r"] != 0).sum() == 2
    # pair (0, 2): r_02 = -1, argument m + (y_0 - y_2) = m + (m - up) > 0: active
    assert out["c"].tolist() == [[1, 0, -1, 0]]
    assert np.isclose(out["LR"][0], 5 * float(m) + (float(m) + float(m) - float(up)))


def test_transition_reference():
    rowptr = np.array([0, 2, 2, 3, 5])
    col = np.array([1, 2, 0, 0, 3])
    P = D.transition(rowptr, col, rowflag=np.array([0, 0, 0, 1], bool))
    assert P[0].tolist() == [0, 0.5, 0.5, 0] and not P[1].any() and not P[3].any()
    assert P[2].tolist() == [1, 0, 0, 0]


def test_distill_queries(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    As = [1, 1000, 100_000, 4_000_000]
    for sizes in ([lib.msha_link_distill_fwd_workspace_size(a) for a in As],
                  [lib.msha_pair_grad_bwd_workspace_size(a, 128) for a in As]):
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] < sizes[-1]
    # the table gradient's partials: link_bce_bwd's own layout
    for p in As:
        assert (lib.msha_pair_grad_bwd_workspace_size(p, 64)
                == lib.msha_link_bce_bwd_workspace_size(p, 64))
    assert lib.msha_link_distill_fwd_workspace_size(1 << 30) == 0
    assert lib.msha_pair_grad_bwd_workspace_size(1 << 30, 64) == 0


def test_distill_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20

    def sample(A=10, walks=2, hops=3, n_rand=1, anchors=p, n_nodes=64, n_edges=100, rowptr=p,
               ctx=p):
        return _lib.call("msha_context_sample", A, walks, hops, n_rand, anchors, 64, n_nodes,
                         n_edges, rowptr, p, None, 1, 0, ctx, None)

    with pytest.raises(RuntimeError, match="null pointer"):
        sample(anchors=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        sample(rowptr=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        sample(ctx=None)
    with pytest.raises(RuntimeError, match=r"must be in \[1, 64\]"):
        sample(walks=0, n_rand=0)
    with pytest.raises(RuntimeError, match=r"must be in \[1, 64\]"):
        sample(walks=8, hops=8, n_rand=1)
    with pytest.raises(RuntimeError, match="bad sizes"):
        sample(walks=-1)
    with pytest.raises(RuntimeError, match="n_nodes must be in"):
        sample(n_nodes=1 << 31)
    with pytest.raises(RuntimeError, match="n_nodes must be in"):
        sample(n_nodes=0)
    with pytest.raises(RuntimeError, match="n_edges must be below"):
        sample(n_edges=1 << 31)

    def fwd(A=100, K=8, feat=128, dt=F32, h=p, ld=128, ctx=p, tl=p, th=None, t_feat=0, t_dt=F32,
            t_ld=0, margin=0.1, tau=1.0, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_distill_fwd", A, K, feat, dt, h, ld, 1000, p, ctx, tl, th,
                         t_feat, t_dt, t_ld, 1000, margin, tau, 1.0, 1.0, 0.0, p, p, p, p, p, ws,
                         ws_bytes, None)

    for K in (1, 65, 0):
        with pytest.raises(RuntimeError, match=r"K must be in \[2, 64\]"):
            fwd(K=K)
    with pytest.raises(RuntimeError, match="below 2\\^30"):
        fwd(A=1 << 28)
    with pytest.raises(RuntimeError, match="exactly one of"):
        fwd(tl=None)
    with pytest.raises(RuntimeError, match="exactly one of"):
        fwd(th=p, t_feat=64, t_ld=64)
    with pytest.raises(RuntimeError, match="teacher table.*unsupported width"):
        fwd(tl=None, th=p, t_feat=24, t_ld=24)
    with pytest.raises(RuntimeError, match="teacher table.*16-byte aligned"):
        fwd(tl=None, th=p + 4, t_feat=64, t_ld=64)
    with pytest.raises(RuntimeError, match="tau > 0"):
        fwd(tau=0.0)
    with pytest.raises(RuntimeError, match="margin >= 0"):
        fwd(margin=-0.5)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(ctx=None)

    def bwd(P=100, feat=128, dt=F32, h=p, ld=128, g=p, gloss=p, dH=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_pair_grad_bwd", P, feat, dt, h, ld, 1000, p, p, g, gloss, p, p, p,
                         dH, ws, ws_bytes, None)

    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(h=None)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(h=p + 4)
        with pytest.raises(RuntimeError, match="16-byte row pitch"):
            call(ld=130)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=24)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=512)  # fp32: past 64 lanes x 16 bytes
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=4, dt=BF16)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(dt=7)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws_bytes=8)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws=p + 8)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws=None)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        bwd(P=1 << 30)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(g=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(gloss=None)
    with pytest.raises(RuntimeError, match="dH must be 16-byte aligned"):
        bwd(dH=p + 4)


def test_distill_python_argument_checks(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    h = torch.zeros(6, 16)
    anchors = torch.zeros(3, dtype=torch.int64)
    ctx = torch.zeros(3, 4, dtype=torch.int64)
    t = torch.zeros(3, 4)
    pred = layers.LinkPredictor("mlp", 16, 16, 1, 2, 0.0)
    with pytest.raises(ValueError, match="no scalar to rank by"):
        pred.distill_loss(h, anchors, ctx, teacher_logits=t)
    # rejected before the library's kernels (or the device) are touched: CPU tensors get here
    with pytest.raises(TypeError, match="float32 or bfloat16 table"):
        MF.link_distill_loss(h.double(), anchors, ctx, teacher_logits=t)
    with pytest.raises(TypeError, match="int64"):
        MF.link_distill_loss(h, anchors.to(torch.int32), ctx, teacher_logits=t)
    with pytest.raises(TypeError, match="int64"):
        MF.link_distill_loss(h, anchors, ctx.to(torch.int32), teacher_logits=t)
    with pytest.raises(ValueError, match=r"anchors must be \(A,\) and context \(A, K\)"):
        MF.link_distill_loss(h, anchors[:2], ctx, teacher_logits=t)
    with pytest.raises(ValueError, match=r"anchors must be \(A,\) and context \(A, K\)"):
        MF.link_distill_loss(h, anchors, ctx.reshape(-1), teacher_logits=t)
    with pytest.raises(ValueError, match=r"K must be in \[2, 64\]"):
        MF.link_distill_loss(h, anchors, ctx[:, :1], teacher_logits=t[:, :1])
    with pytest.raises(ValueError, match=r"K must be in \[2, 64\]"):
        MF.link_distill_loss(h, anchors, torch.zeros(3, 65, dtype=torch.int64),
                             teacher_logits=torch.zeros(3, 65))
    with pytest.raises(ValueError, match="exactly one of"):
        MF.link_distill_loss(h, anchors, ctx)
    with pytest.raises(ValueError, match="exactly one of"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t, teacher_table=h)
    with pytest.raises(ValueError, match="teacher_logits must be"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t[:, :3])
    with pytest.raises(ValueError, match="teacher_logits must be"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=ctx)
    with pytest.raises(TypeError, match="teacher table"):
        MF.link_distill_loss(h, anchors, ctx, teacher_table=h.double())
    with pytest.raises(ValueError, match="tau must be positive"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t, tau=0.0)
    with pytest.raises(ValueError, match="margin must not be negative"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t, margin=-1.0)
    with pytest.raises(ValueError, match="not a context_plan"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t, plan=object())
    bare = MF.PairPlan(6, 12, None, None, None)  # a pair_plan: no flat src with it
    with pytest.raises(ValueError, match="not a context_plan"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t, plan=bare)
    with pytest.raises(ValueError, match="not supported"):
        MF.link_distill_loss(torch.zeros(6, 24), anchors, ctx, teacher_logits=t)
    with pytest.raises(ValueError, match="not supported"):
        MF.link_distill_loss(h, anchors, ctx, teacher_table=torch.zeros(6, 24))
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.link_distill_loss(h, anchors, ctx, teacher_logits=t)
    with pytest.raises(TypeError, match="int64"):
        MF.context_plan(anchors.to(torch.int32), ctx, 6)
    with pytest.raises(ValueError, match="n must be in"):
        MF.context_plan(anchors, ctx, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.context_plan(anchors, ctx, 6)
    csr = (torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"must be in \[1, 64\]"):
        MF.sample_context(csr, anchors, 0, 1)
    with pytest.raises(ValueError, match=r"must be in \[1, 64\]"):
        MF.sample_context(csr, anchors, 13, 5)
    with pytest.raises(ValueError, match="n_nodes is needed with a bare CSR"):
        MF.sample_context(csr, anchors, 1, 1, n_rand=2)
    with pytest.raises(TypeError, match="1-D int64"):
        MF.sample_context(csr, anchors.to(torch.int32), 1, 1)
    with pytest.raises(TypeError, match="int32 tensors"):
        MF.sample_context((csr[0].long(), csr[1]), anchors, 1, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.sample_context(csr, anchors, 2, 2, n_rand=1, n_nodes=2)
