"""CPU-side checks for HGANE's batch attention layer (HGANE.py:11-76), which is not on the
device yet: the sparse fp64 restatement tests/hgane_ref.py (group segments, joint normaliser,
injected keep masks -- the oracle a device implementation will be held to) against the
reference's own fp64 outputs in tests/golden/hgane.npz, the fixture's own shape, and the
drop-in module's stand-in.  Nothing here reaches the GPU."""
import numpy as np
import pytest
import torch

from conftest import golden

import hgane_ref as HR


def _rel_max(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)


def _extra(z, tag):
    """Case B's (N, in) embedding table is not stored: the constructor's second draw."""
    if tag + "init.source_embedding" in z.files:
        return {}
    fin, _, seed = HR.CASES[tag]
    return {"source_embedding": HR.source_embedding(seed, len(z[tag + "gid"]), fin).numpy()}


def test_embedding_regeneration_matches_the_stored_table():
    """The regeneration case B relies on reproduces case A's stored table bit for bit."""
    z = golden("hgane.npz")
    fin, _, seed = HR.CASES["A."]
    got = HR.source_embedding(seed, len(z["A.gid"]), fin).numpy()
    assert np.array_equal(got, z["A.init.source_embedding"])


@pytest.mark.parametrize("tag", ["A.", "B."])
def test_restatement_reproduces_the_reference_fp64(tag):
    """Output and every parameter gradient of the restatement's fp64 autograd within 1e-12
    of the reference's fp64 run, relative to each tensor's largest element; the embedding
    gradient is exactly zero outside the batch rows."""
    z = golden("hgane.npz")
    seed = HR.CASES[tag][2]
    src, counts, gid = z[tag + "src"], z[tag + "counts"], z[tag + "gid"]
    P = HR.params64(z, tag, _extra(z, tag))
    if tag == "A.":
        run = lambda b: (torch.tensor(z[f"A.init.{b}.running_mean"], dtype=torch.float64),  # noqa
                         torch.tensor(z[f"A.init.{b}.running_var"], dtype=torch.float64))
        with torch.no_grad():
            ev = HR.layer(P, src, counts, gid, training=False, running=(run("bn1"), run("bn2")))
        assert _rel_max(ev.numpy(), z["A.out_eval64"]) <= 1e-12
    out = HR.layer(P, src, counts, gid)
    assert _rel_max(out.detach().numpy(), z[tag + "out64"]) <= 1e-12
    (out * torch.as_tensor(HR.dout_weights(seed, len(src))).double()).sum().backward()
    rows = np.unique(src)
    for k, leaf in P.items():
        g = leaf.grad.numpy()
        if k == "source_embedding":
            assert not np.delete(g, rows, axis=0).any()
            if tag == "B.":
                assert np.array_equal(rows, z["B.emb_rows"])
                g = g[rows]
        assert _rel_max(g, z[f"{tag}grad64.{k}"]) <= 1e-12, k


@pytest.mark.parametrize("tag", ["A.", "B."])
def test_dropout_masks_enter_after_normalisation(tag):
    """With injected keep masks the restatement equals the reference's formula written out
    densely (HGANE.py:57-73: normalise, then drop): Z1 and Zc are dropout-free."""
    z = golden("hgane.npz")
    src, counts, gid = z[tag + "src"], z[tag + "counts"], z[tag + "gid"]
    P = {k: v.detach() for k, v in HR.params64(z, tag, _extra(z, tag)).items()}
    B, M, p = len(src), counts.shape[1], 0.4
    rng = np.random.default_rng(3)
    kin = torch.as_tensor(rng.random((B, M)) >= p)
    kra = torch.as_tensor(rng.random((B, B)) >= p)
    el, er, pl, pr, h1, h2, h3 = HR.projections(P, src)
    inter, same = HR.masks(counts, gid, src)
    c = HR.core(el, er, pl, pr, h1, h2, h3, inter, same, kin, kra, p)
    # HGANE.py:46-73 on the induced batch, with F.dropout's mask supplied
    neg = torch.full((), -9e15, dtype=torch.float64)
    e12 = torch.where(inter, torch.nn.functional.leaky_relu(el[:, None] + er[None, :], 0.2), neg)
    e3 = torch.where(same, torch.nn.functional.leaky_relu(pl[:, None] + pr[None, :], 0.2), neg)
    county = torch.exp(e3).sum(1, keepdim=True) + torch.exp(e12).sum(1, keepdim=True)
    a_intra = torch.exp(e3) / county * kra / (1 - p)
    a_inter = torch.exp(e12) / torch.exp(e12).sum(1, keepdim=True) * kin / (1 - p)
    assert _rel_max(c["U"].numpy(), (a_inter @ h1 + a_intra @ h2).numpy()) <= 1e-13
    assert _rel_max(c["V"].numpy(), (a_inter.t() @ h3).numpy()) <= 1e-13
    assert _rel_max(c["Zc"].numpy(), county[:, 0].numpy()) <= 1e-13


def test_fixture_shape():
    """The batch the fixture promises: segments of 1, 31, 32, 33, 65 and 130 entries, 25
    repeated sources, every inter row and every recipient column in use, a finite fp32
    reference within 1e-5 of its fp64 run."""
    z = golden("hgane.npz")
    for tag in ("A.", "B."):
        src, gid, counts = z[tag + "src"], z[tag + "gid"], z[tag + "counts"]
        sizes = np.bincount(gid[src], minlength=int(gid.max()) + 1)
        assert sorted(sizes.tolist()) == [0, 1, 31, 32, 33, 65, 130]
        assert len(src) == 292 and len(src) - len(np.unique(src)) == 25
        assert (counts.sum(1) >= 1).all() and ((counts[src] > 0).sum(0) >= 15).all()
        assert np.isfinite(z[tag + "out32"]).all()
        assert _rel_max(z[tag + "out32"], z[tag + "out64"]) <= 1e-5
        for k in z.files:
            if k.startswith(tag + "grad32."):
                assert _rel_max(z[k], z[k.replace("grad32", "grad64")]) <= 1e-5, k


def test_dropin_stand_in_still_says_so(msha, tmp_path):
    """HGANE's class is not on the device: the drop-in's stand-in raises on construction and
    the module exports the reference module's other names."""
    from msha_gnn_amd import trainpy

    with trainpy.namespace(tmp_path, "cpu"):
        import HGANE

        with pytest.raises(NotImplementedError):
            HGANE.GraphAttentionLayer(16, 16, 4, 4, {i: 0.0 for i in range(4)})
        for name in ("roc_auc_score", "label_binarize", "np", "torch", "nn", "F", "random",
                     "sys"):
            assert hasattr(HGANE, name), name
