"""Host-side checks of the representation-matching term and the student MLP: the numpy
restatement itself (``match_ref``) against torch fp64 autograd, the ABI's size query and
argument errors (no launch), the Python surface's own argument checks, and the MLP's
construction against the reference fixture."""
import numpy as np
import pytest
import torch

import match_ref as R
from conftest import golden

F32, BF16 = 0, 1  # MSHA_DTYPE_*


def _torch_ref(h, T, rows, gloss=1.0):
    """fp64 autograd of 1 - cosine_similarity(h[rows], T[rows]).mean() over the valid rows."""
    m = min(h.shape[0], T.shape[0])
    rows = np.arange(m) if rows is None else np.asarray(rows)
    ok = (rows >= 0) & (rows < m)
    idx = torch.as_tensor(rows[ok])
    ht = torch.tensor(np.asarray(h, np.float64), requires_grad=True)
    Tt = torch.tensor(np.asarray(T, np.float64))
    loss = 1 - torch.nn.functional.cosine_similarity(ht[idx], Tt[idx], dim=-1).mean()
    (gloss * loss).backward()
    return float(loss.detach()), ht.grad.numpy()


def test_restatement_matches_torch_autograd():
    rng = np.random.default_rng(0)
    n, n_t, F = 50, 44, 16
    h = rng.standard_normal((n, F))
    T = rng.standard_normal((n_t, F))
    rows = rng.integers(0, n_t, 4000)
    rows[rows == 9] = 10            # a row that never occurs
    rows[:5] = (-1, n_t, n - 1, n + 5, 3)  # padding: n - 1 is inside h, outside T
    f = R.forward(h, T, rows)
    assert f["npad"] == 4 and f["pv"] == 3996 and f["count"][9] == 0
    assert np.isnan(f["cos"][9]) and np.isnan(f["cos"][n_t:]).all()
    loss, grad = _torch_ref(h, T, rows, gloss=-2.5)
    assert abs(f["loss"] - loss) <= 1e-14
    dH, A = R.backward(h, T, f["coef"], -2.5)
    assert np.abs(dH - grad).max() <= 1e-15 * max(1.0, np.abs(grad).max()) + 1e-16
    assert (dH[f["count"] == 0] == 0).all() and (A >= np.abs(dH) - 1e-18).all()
    # rows=None is the identity list
    g = R.forward(h[:n_t], T, None)
    loss, grad = _torch_ref(h[:n_t], T, None)
    assert abs(g["loss"] - loss) <= 1e-14 and (g["count"] == 1).all()
    assert np.abs(R.backward(h[:n_t], T, g["coef"], 1.0)[0] - grad).max() <= 1e-15
    # nothing valid: loss 0, zero gradient
    z = R.forward(h, T, np.array([-1, n]))
    assert z["loss"] == 0.0 and z["pv"] == 0 and not z["coef"].any()


def test_restatement_eps_cases_are_torchs():
    """Each norm is clamped on its own at 1e-8.  torch clamps in place outside autograd, so
    the gradient of a clamped nonzero row keeps d|h| / dh of the unclamped norm: 1e8 - 1e7
    for [1e-9, 0] against [1e3, 0], where ns^2 in the second term would give 1e8 - 1e6."""
    h = np.array([[1e-9, 0.0], [0.0, 0.0]])
    T = np.array([[1e3, 0.0], [3.0, 4.0]])
    f = R.forward(h, T, np.array([0, 1]))
    assert abs(f["cos"][0] - 0.1) <= 1e-15 and f["cos"][1] == 0.0
    ht = torch.tensor(h, requires_grad=True)
    cos = torch.nn.functional.cosine_similarity(ht, torch.tensor(T), dim=-1)
    assert abs(float(cos[0].detach()) - 0.1) <= 1e-15 and float(cos[1].detach()) == 0.0
    cos.sum().backward()
    assert np.allclose(ht.grad[1].numpy(), [6e7, 8e7], rtol=1e-12)
    assert np.allclose(ht.grad[0].numpy(), [9e7, 0.0], rtol=1e-12)
    # d cos / d h = -P_v d loss / d h
    dH, _ = R.backward(h, T, f["coef"], 1.0)
    assert np.allclose(-2 * dH, ht.grad.numpy(), rtol=1e-12, atol=0)


def test_match_size_query(msha):
    from msha_gnn_amd import _lib

    size = _lib.load().msha_link_match_fwd_workspace_size
    ns = [1, 1000, 100_000, 4_000_000]
    sizes = [size(4096, n) for n in ns]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert sizes[2] >= 4 * 100_000  # the int32 counts
    assert size(4_000_000, 100_000) == size(1, 100_000)  # nothing per entry
    assert size(0, 10) == 0 and size(1 << 31, 10) == 0 and size((1 << 31) - 1, 10) > 0
    assert size(10, 0) == 0 and size(10, 1 << 31) == 0


def test_match_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20

    def fwd(P=100, feat=128, hd=F32, h=p, ld=128, n=1000, td=F32, T=p, t_ld=128, n_t=900,
            rows=p, coef=p, loss=p, npad=p, ws=p, ws_bytes=1 << 30):
        return _lib.call("msha_link_match_fwd", P, feat, hd, h, ld, n, td, T, t_ld, n_t, rows,
                         coef, None, None, loss, npad, ws, ws_bytes, None)

    def bwd(feat=128, hd=F32, h=p, ld=128, n=1000, td=F32, T=p, t_ld=128, n_t=900, coef=p,
            gloss=p, dH=p):
        return _lib.call("msha_link_match_bwd", feat, hd, h, ld, n, td, T, t_ld, n_t, coef,
                         gloss, dH, None)

    for call, name in ((fwd, "link_match_fwd"), (bwd, "link_match_bwd")):
        with pytest.raises(RuntimeError, match=f"{name}: null pointer"):
            call(h=None)
        with pytest.raises(RuntimeError, match=f"{name}: null pointer"):
            call(T=None)
        with pytest.raises(RuntimeError, match=f"{name}: null pointer"):
            call(coef=None)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(h=p + 4)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(T=p + 8)
        with pytest.raises(RuntimeError, match="16-byte row pitch"):
            call(ld=130)
        with pytest.raises(RuntimeError, match="16-byte row pitch"):
            call(td=BF16, t_ld=132)  # a bf16 row pitch is a multiple of 8 elements
        with pytest.raises(RuntimeError, match="16-byte row pitch"):
            call(t_ld=64)  # shorter than a row
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=24)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=512, ld=512, t_ld=512)  # fp32: past 64 lanes x 16 bytes
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=512, ld=512, t_ld=512, hd=BF16)  # the teacher is still fp32
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=4, ld=4, t_ld=8, td=BF16)  # bf16: below 16 bytes
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(hd=7)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(td=7)
        with pytest.raises(RuntimeError, match="bad sizes"):
            call(n=0)
        with pytest.raises(RuntimeError, match="bad sizes"):
            call(n_t=0)
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            call(n=1 << 31)
        with pytest.raises(RuntimeError, match="coef must be 8-byte aligned"):
            call(coef=p + 4)
    with pytest.raises(RuntimeError, match="bad sizes"):
        fwd(P=0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        fwd(P=1 << 31)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(loss=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(npad=None)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        fwd(ws_bytes=8)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        fwd(ws=p + 8)
    with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
        fwd(ws=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(gloss=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(dH=None)
    with pytest.raises(RuntimeError, match="dH must be 16-byte aligned"):
        bwd(dH=p + 4)

    def count(P=100, n=1000, n_valid=900, rows=p, cnt=p, npad=p):
        return _lib.call("msha_link_match_count", P, n, n_valid, rows, cnt, npad, None)

    for kw in (dict(P=0), dict(P=1 << 31), dict(n=0), dict(n=1 << 31), dict(n_valid=-1),
               dict(n_valid=1001)):
        with pytest.raises(RuntimeError, match="link_match_count: bad sizes"):
            count(**kw)
    for kw in (dict(rows=None), dict(cnt=None), dict(npad=None)):
        with pytest.raises(RuntimeError, match="link_match_count: null pointer"):
            count(**kw)


def test_match_python_argument_checks(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    h, t = torch.zeros(4, 16), torch.zeros(4, 16)
    idx = torch.zeros(3, dtype=torch.int64)
    # rejected before the library's kernels (or the device) are touched: CPU tensors get here
    with pytest.raises(TypeError, match="float32 or bfloat16 table"):
        MF.link_match_loss(h.double(), idx, t)
    with pytest.raises(TypeError, match="float32 or bfloat16 teacher"):
        MF.link_match_loss(h, idx, t.half())
    with pytest.raises(ValueError, match="h must be"):
        MF.link_match_loss(h[0], idx, t)
    with pytest.raises(ValueError, match="teacher_table must be"):
        MF.link_match_loss(h, idx, t[0])
    with pytest.raises(ValueError, match="one width"):
        MF.link_match_loss(h, idx, torch.zeros(4, 32))
    with pytest.raises(TypeError, match="int64"):
        MF.link_match_loss(h, idx.to(torch.int32), t)
    with pytest.raises(ValueError, match="rows must be 1-D"):
        MF.link_match_loss(h, idx.view(3, 1), t)
    with pytest.raises(ValueError, match="rows must be 1-D"):
        MF.link_match_loss(h, idx[:0], t)
    with pytest.raises(ValueError, match="equal row counts"):
        MF.link_match_loss(h, None, torch.zeros(5, 16))
    with pytest.raises(ValueError, match="not supported"):
        MF.link_match_loss(torch.zeros(4, 24), idx, torch.zeros(4, 24))
    with pytest.raises(ValueError, match="not supported"):  # fp32 x bf16 at F = 4
        MF.link_match_loss(torch.zeros(4, 4), idx, torch.zeros(4, 4, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.link_match_loss(h, idx, t)
    for predictor in ("inner", "mlp"):  # the term does not depend on the head
        with pytest.raises(RuntimeError, match="GPU only"):
            layers.LinkPredictor(predictor, 16, 16, 1, 2, 0.0).match_loss(h, idx, t)
    with pytest.raises(ValueError, match="linear_bias"):
        MF.linear_bias(torch.zeros(4, 16), torch.zeros(8, 12), torch.zeros(8))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_mlp_is_the_references_module(msha, k):
    from msha_gnn_amd import layers

    z = golden("llp_student.npz")
    pre = f"mlp{k}.state."
    want = {name[len(pre):]: z[name] for name in z.files if name.startswith(pre)}
    x = z[f"mlp{k}.x"]
    torch.manual_seed(k)
    mlp = layers.MLP(k, x.shape[1], 32, z[f"mlp{k}.y"].shape[1], 0.5)
    sd = mlp.state_dict()
    assert list(sd) == list(want)  # names and order
    for name, v in want.items():
        assert np.array_equal(sd[name].numpy(), v), name  # bit-identical init
    assert isinstance(mlp.dropout, torch.nn.Dropout) and mlp.dropout.p == 0.5
    assert len(mlp.norms) == 0 and mlp.num_layers == k and mlp.norm_type == "none"
    torch.manual_seed(k + 10)
    mlp.reset_parameters()
    torch.manual_seed(k + 10)
    again = layers.MLP(k, x.shape[1], 32, z[f"mlp{k}.y"].shape[1], 0.5)
    for a, b in zip(mlp.parameters(), again.parameters()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("norm,cls", [("batch", torch.nn.BatchNorm1d),
                                      ("layer", torch.nn.LayerNorm)])
def test_mlp_norm_variants_build_and_raise(msha, norm, cls):
    from msha_gnn_amd import layers

    mlp = layers.MLP(3, 16, 32, 8, 0.1, norm_type=norm)
    assert len(mlp.norms) == 2 and all(isinstance(m, cls) for m in mlp.norms)
    keys = list(mlp.state_dict())
    assert "norms.0.weight" in keys and "norms.1.bias" in keys and "layers.2.weight" in keys
    assert len(layers.MLP(1, 16, 32, 8, 0.1, norm_type=norm).norms) == 0
    with pytest.raises(NotImplementedError, match="LLP.py:57-60"):
        mlp(torch.zeros(4, 16))


def test_dropin_llp_exports_the_student(msha):
    import importlib
    import os
    import sys

    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "msha--gnn_amd", "dropin")
    sys.path.insert(0, d)
    try:
        saved = sys.modules.pop("LLP", None)
        mod = importlib.import_module("LLP")
    finally:
        sys.path.remove(d)
        sys.modules.pop("LLP", None)
        if saved is not None:
            sys.modules["LLP"] = saved
    from msha_gnn_amd import layers

    assert mod.MLP is layers.MLP and callable(mod.KD_cosine)
    assert mod.LinkPredictor is layers.LinkPredictor
    with pytest.raises(ValueError, match="equal row counts"):
        mod.KD_cosine(torch.zeros(4, 16), torch.zeros(5, 16))
