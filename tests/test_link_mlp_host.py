"""Host-side checks of the 'mlp' predictor's training loss: the fp64 restatement
(``link_mlp_ref``) against the reference's own run (tests/golden/llp_mlp.npz), the ABI's
queries and argument errors (no launch), the Python surface's argument checks, and the
header's declarations."""
import os
import re

import numpy as np
import pytest
import torch

import link_mlp_ref as R
from conftest import ROOT, golden

F32, BF16 = 0, 1  # MSHA_DTYPE_*

NEW_SYMBOLS = ("msha_link_mlp_supported", "msha_link_mlp_wgrad_rows",
               "msha_link_mlp_loss_fwd_workspace_size", "msha_link_mlp_loss_fwd",
               "msha_link_mlp_bwd_workspace_size", "msha_link_mlp_bwd")


def _scalar(x):
    return float(np.asarray(x).reshape(-1)[0])


def test_restatement_matches_the_reference_run():
    """LLP.py:233, :235, :238 in fp64 (eval mode, no padding) at 1e-12."""
    z = golden("llp_mlp.npz")
    wl, wm = _scalar(z["true_label"]), _scalar(z["kd_p"])
    assert (wl, wm) == (10.0, 100.0) and z["h"].shape == (40, 32) and len(z["src"]) == 96
    f = R.forward(z["h"], z["src"], z["dst"], z["W"], z["b"], teacher=z["t_out"], w_label=wl,
                  w_mse=wm)
    assert f["ok"].all() and f["pv"] == 96
    np.testing.assert_allclose(f["out"], z["output"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f["l_lab"], _scalar(z["label_loss"]), rtol=1e-12)
    np.testing.assert_allclose(f["l_mse"], _scalar(z["mse"]), rtol=1e-12)
    np.testing.assert_allclose(f["loss"], _scalar(z["loss"]), rtol=1e-12)
    g = R.upstream(f["out"], f["ok"], f["label"], z["t_out"], f["pv"], wl, wm, 1.0)
    bw = R.backward(z["h"], z["src"], z["dst"], z["W"], R.dz_from(f["out"], g, f["pre"] > 0),
                    f["ok"])
    for got, key in ((bw["dH"], "dh"), (bw["dW"], "dW"), (bw["db"], "db")):
        np.testing.assert_allclose(got, z[key], rtol=1e-12, atol=1e-12 * np.abs(z[key]).max())
    # label=None is dst itself
    f2 = R.forward(z["h"], z["src"], z["dst"], z["W"], z["b"], label=z["dst"], teacher=z["t_out"],
                   w_label=wl, w_mse=wm)
    assert f2["loss"] == f["loss"]


def test_restatement_padding_and_empty():
    rng = np.random.default_rng(0)
    n, F, N, P = 9, 16, 16, 12
    h, W, b = rng.standard_normal((n, F)), rng.standard_normal((N, F)), rng.standard_normal(N)
    src, dst = rng.integers(0, n, P), rng.integers(0, n, P)
    lab = rng.integers(0, N, P)
    t = rng.random((P, N))
    full = R.forward(h, src, dst, W, b, label=lab, teacher=t, w_label=2.0, w_mse=3.0)
    src2, dst2, lab2 = src.copy(), dst.copy(), lab.copy()
    src2[0], src2[1], dst2[2], lab2[3], lab2[4] = -1, n, n + 5, N, -1
    pad = R.forward(h, src2, dst2, W, b, label=lab2, teacher=t, w_label=2.0, w_mse=3.0)
    assert pad["pv"] == P - 5 and np.isnan(pad["out"][:5]).all()
    keep = R.forward(h, src[5:], dst[5:], W, b, label=lab[5:], teacher=t[5:], w_label=2.0,
                     w_mse=3.0)
    np.testing.assert_allclose(pad["loss"], keep["loss"], rtol=1e-14)
    assert full["pv"] == P and full["loss"] != pad["loss"]
    none = R.forward(h, np.full(P, -1), dst, W, b, label=lab, teacher=t)
    assert none["pv"] == 0 and none["loss"] == 0.0
    g = R.upstream(none["out"], none["ok"], none["label"], t, 0, 1.0, 1.0, 1.0)
    assert not g.any()


def test_header_declares_every_new_symbol(msha):
    from msha_gnn_amd import _lib

    text = open(os.path.join(ROOT, "include", "msha_gnn.h"), encoding="utf-8").read()
    for name in NEW_SYMBOLS:
        assert re.search(r"MSHA_API\s+[\w\s\*]+\b" + name + r"\(", text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+MSHA_ABI_VERSION\s+16\b", text) and _lib.ABI_VERSION == 16


def test_link_mlp_queries(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()
    for dt in (F32, BF16):
        for feat, hid in [(32, 32), (128, 128), (16, 16), (128, 32), (32, 128), (64, 16)]:
            assert lib.msha_link_mlp_supported(feat, hid, dt) == 1, (feat, hid, dt)
            assert lib.msha_link_bce_supported(feat, dt) == 1
        for feat, hid in [(24, 32), (32, 24), (8, 32), (32, 8), (256, 128), (128, 256), (0, 32),
                          (32, 0)]:
            assert lib.msha_link_mlp_supported(feat, hid, dt) == 0, (feat, hid, dt)
    assert lib.msha_link_mlp_supported(32, 32, 7) == 0
    rows = lib.msha_link_mlp_wgrad_rows()
    assert rows > 0
    Ps = [1, 1000, 100_000, 4_000_000]
    for sizes in ([lib.msha_link_mlp_loss_fwd_workspace_size(p) for p in Ps],
                  [lib.msha_link_mlp_bwd_workspace_size(p, 128, 128) for p in Ps]):
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] < sizes[-1]
    # one (N F + N) partial per row block and one F-row per chunk slot
    blocks = -(-4_000_000 // rows)
    assert (lib.msha_link_mlp_bwd_workspace_size(4_000_000, 128, 128)
            >= blocks * (128 * 128 + 128) * 4
            + 2 * lib.msha_pair_plan_chunk_slots(4_000_000) * 128 * 4)
    # nothing (P, F)- or (P, N)-sized hides in a workspace
    assert lib.msha_link_mlp_bwd_workspace_size(4_000_000, 128, 128) < 4_000_000 * 128
    assert lib.msha_link_mlp_loss_fwd_workspace_size(4_000_000) < 4_000_000 * 32
    assert lib.msha_link_mlp_loss_fwd_workspace_size(1 << 30) == 0
    assert lib.msha_link_mlp_bwd_workspace_size(1 << 30, 32, 32) == 0


def test_link_mlp_argument_errors_are_reported(msha):
    """Every rejection happens on the host, before any launch: the pointers here are
    aligned dummies that nothing dereferences."""
    from msha_gnn_amd import _lib

    p = 1 << 20
    big = 1 << 30

    def fwd(P=100, feat=128, hid=128, dt=F32, h=p, ld=128, src=p, W=p, out=p, drop=0.0, ws=p,
            ws_bytes=1 << 30):
        return _lib.call("msha_link_mlp_loss_fwd", P, feat, hid, dt, h, ld, 1000, src, p, None, W,
                         p, None, 1.0, 0.0, drop, 0, 0, out, p, None, p, ws, ws_bytes, None)

    def bwd(P=100, feat=128, hid=128, dt=F32, h=p, ld=128, src=p, W=p, out=p, drop=0.0, ws=p,
            ws_bytes=1 << 30, dW=p, db=p, dx=p, gloss=p):
        return _lib.call("msha_link_mlp_bwd", P, feat, hid, dt, h, ld, 1000, src, p, None, W, None,
                         out, p, 1.0, 0.0, drop, gloss, p, p, p, p, dx, dW, db, p, ws, ws_bytes,
                         None)

    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(h=None)
        with pytest.raises(RuntimeError, match="null pointer"):
            call(src=None)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(h=p + 4)
        with pytest.raises(RuntimeError, match="16-byte row pitch"):
            call(ld=130)
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            call(P=big)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(feat=24)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            call(feat=256, ld=256)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            call(hid=24)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            call(feat=8, ld=8, dt=BF16)
        with pytest.raises(RuntimeError, match="unsupported width"):
            call(dt=7)
        with pytest.raises(RuntimeError, match="drop_p must be in"):
            call(drop=1.0)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(out=p + 4)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws_bytes=8)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws=p + 8)
        with pytest.raises(RuntimeError, match="workspace too small or unaligned"):
            call(ws=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(W=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(gloss=None)
    with pytest.raises(RuntimeError, match="come together"):
        bwd(dW=None)
    with pytest.raises(RuntimeError, match="dH needs W, dx and the plan"):
        bwd(W=None)
    with pytest.raises(RuntimeError, match="dH needs W, dx and the plan"):
        bwd(dx=None)


def test_link_mlp_python_argument_checks(msha):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import layers

    idx = torch.zeros(3, dtype=torch.int64)
    h, W, b = torch.zeros(4, 16), torch.zeros(16, 16), torch.zeros(16)
    # rejected before the library's kernels (or the device) are touched: CPU tensors get here
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        MF.link_mlp_loss(h.double(), idx, idx, W, b)
    with pytest.raises(ValueError, match=r"h must be \(n, F\)"):
        MF.link_mlp_loss(torch.zeros(16), idx, idx, W, b)
    with pytest.raises(TypeError, match="int64"):
        MF.link_mlp_loss(h, idx.to(torch.int32), idx, W, b)
    with pytest.raises(ValueError, match="one length"):
        MF.link_mlp_loss(h, idx, idx[:2], W, b)
    with pytest.raises(ValueError, match="at least one pair"):
        MF.link_mlp_loss(h, idx[:0], idx[:0], W, b)
    with pytest.raises(ValueError, match="W must be"):
        MF.link_mlp_loss(h, idx, idx, torch.zeros(16, 32), b)
    with pytest.raises(ValueError, match="W must be"):
        MF.link_mlp_loss(h, idx, idx, torch.zeros(16), b)
    with pytest.raises(ValueError, match="b must be"):
        MF.link_mlp_loss(h, idx, idx, W, torch.zeros(8))
    with pytest.raises(ValueError, match="label must be"):
        MF.link_mlp_loss(h, idx, idx, W, b, label=idx.to(torch.int32))
    with pytest.raises(ValueError, match="label must be"):
        MF.link_mlp_loss(h, idx, idx, W, b, label=idx[:2])
    with pytest.raises(ValueError, match="teacher_out must be"):
        MF.link_mlp_loss(h, idx, idx, W, b, teacher_out=torch.zeros(3, 8))
    with pytest.raises(ValueError, match="teacher_out must be"):
        MF.link_mlp_loss(h, idx, idx, W, b, teacher_out=torch.zeros(3, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match="p must be in"):
        MF.link_mlp_loss(h, idx, idx, W, b, p=1.0, training=True)
    foreign = MF.PairPlan(5, 3, None, None, None)  # another table's plan
    with pytest.raises(ValueError, match="not a PairPlan of this pair list"):
        MF.link_mlp_loss(h, idx, idx, W, b, plan=foreign)
    with pytest.raises(ValueError, match="not a PairPlan of this pair list"):
        MF.link_mlp_loss(h, idx, idx, W, b, plan=MF.PairPlan(4, 2, None, None, None))
    with pytest.raises(ValueError, match="not a PairPlan of this pair list"):
        MF.link_mlp_loss(h, idx, idx, W, b, plan=(1, 2, 3))
    with pytest.raises(ValueError, match="not supported"):
        MF.link_mlp_loss(torch.zeros(4, 24), idx, idx, torch.zeros(16, 24), b)
    with pytest.raises(ValueError, match="not supported"):
        MF.link_mlp_loss(h, idx, idx, torch.zeros(8, 16), torch.zeros(8))
    with pytest.raises(ValueError, match="not supported"):
        MF.link_mlp_loss(torch.zeros(4, 256), idx, idx, torch.zeros(16, 256), b)
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.link_mlp_loss(h, idx, idx, W, b)
    # the module surface
    with pytest.raises(ValueError, match="needs the 'mlp' predictor"):
        layers.LinkPredictor("inner", 16, 16, 1, 2, 0.0).llp_loss(h, idx, idx)
    with pytest.raises(ValueError, match="deeper head is out of scope"):
        layers.LinkPredictor("mlp", 16, 16, 1, 3, 0.0).llp_loss(h, idx, idx)
    with pytest.raises(RuntimeError, match="GPU only"):
        layers.LinkPredictor("mlp", 16, 16, 1, 2, 0.0).llp_loss(h, idx, idx)
    # the 'inner only' methods keep raising for 'mlp'
    with pytest.raises(ValueError, match="no scalar to rank by"):
        layers.LinkPredictor("mlp", 16, 16, 1, 2, 0.0).loss(h, idx, idx, torch.zeros(3))
