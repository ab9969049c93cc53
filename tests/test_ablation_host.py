"""CPU-side checks of OursLayer2 / ablation2 (Ablation.py:140-231): the dense restatement
tests/ablation_ref.py against the reference's own outputs (tests/golden/ablations.npz), the
fixture's licence for the device's exact-zero a3 / a4 gradients, the new ABI symbols, the
drop-in's exports and the constructors.  No compute call reaches the GPU here."""
import numpy as np
import pytest
import torch

from conftest import golden

import ablation_ref as AR


def _rel_max(got, ref):
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)


def _layer2_restated(z, tag, training):
    """OursLayer2 (Ablation.py:165-205) in fp64 from the fixture's init state, through
    ablation_ref: (out, leaves by name)."""
    o = golden("ours_small.npz")
    d = lambda x: torch.tensor(np.asarray(x, np.float64), requires_grad=True)  # noqa: E731
    p = {k: d(z[f"init.{k}"]) for k in ("W1", "W2", "a", "bn1.weight", "bn1.bias", "bn2.weight",
                                        "bn2.bias")}
    S, R = d(z[tag + "S"]), d(z[tag + "R"])
    counts = o[tag + "counts"] if tag + "counts" in o.files else o["counts"]
    Fd = p["W1"].shape[1]
    h1, h2 = R @ p["W1"], S @ p["W2"]
    er, el = h1 @ p["a"][:Fd, 0], h2 @ p["a"][Fd:, 0]  # Ablation.py:174-175
    u, v = AR.dense_split_core(el, er, h1, h2, torch.as_tensor(counts > 0),
                               torch.as_tensor(o["city"]), torch.as_tensor(o["prov"]),
                               torch.as_tensor(z[tag + "source_index"]))
    running = None
    if not training:
        running = tuple((torch.tensor(z[f"init.{b}.running_mean"], dtype=torch.float64),
                         torch.tensor(z[f"init.{b}.running_var"], dtype=torch.float64))
                        for b in ("bn2", "bn1"))
    out = AR.dense_layer_tail(u, v, (p["bn2.weight"], p["bn2.bias"]),
                              (p["bn1.weight"], p["bn1.bias"]), running=running)
    return out, dict(p, S=S, R=R)


def test_restatement_reproduces_the_reference_fp64():
    """Case B (fp64 reference, a repeated source, an empty inter row): outputs to 1e-10 and
    gradients to 1e-9 of max |ref|.  Ties ablation_ref's closed form (weights 1 / group
    size, no a3 / a4) to Ablation.py's masked softmaxes."""
    z = golden("ablations.npz")
    out_eval, _ = _layer2_restated(z, "B.", training=False)
    assert _rel_max(out_eval.detach().numpy(), z["B.out_eval"]) <= 1e-10
    out, leaves = _layer2_restated(z, "B.", training=True)
    assert _rel_max(out.detach().numpy(), z["B.out"]) <= 1e-10
    (out * torch.tensor(z["B.dout"])).sum().backward()
    for k, leaf in leaves.items():
        assert _rel_max(leaf.grad.numpy(), z[f"B.grad.{k}"]) <= 1e-9, k


@pytest.mark.parametrize("tag", ["", "B."])
def test_reference_score_vector_gradients_are_noise(tag):
    """The reference's a3 / a4 gradients of OursLayer2 are rounding noise around an exact 0
    (at most 1e-5 of max |grad a|; measured ~1e-7 in fp32): the licence for the device's
    exact zeros."""
    z = golden("ablations.npz")
    scale = np.abs(z[tag + "grad.a"]).max()
    assert scale > 0
    for k in ("a3", "a4"):
        assert np.abs(z[f"{tag}grad.{k}"]).max() <= 1e-5 * scale, k


def test_new_abi_symbols_and_argument_errors(msha):
    from msha_gnn_amd import _lib

    lib = _lib.load()  # loads without touching the GPU
    assert lib.msha_abi_version() == 16  # pure additions
    for name in ("msha_ours_split_fwd", "msha_ours_split_bwd", "msha_ours_split_workspace_size"):
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None, name
    assert lib.msha_ours_split_workspace_size(None, 4, 2, 8) == 0  # host-only query
    # bad arguments: an error code (raised by _lib.call), no launch
    with pytest.raises(RuntimeError, match="graph CSR missing"):
        _lib.call("msha_ours_split_fwd", None, None, 4, None, 2, 8, 0, None, None, 0.0, 0, 0,
                  None, None, None)
    with pytest.raises(RuntimeError, match="graph CSR missing"):
        _lib.call("msha_ours_split_bwd", None, None, 4, None, 2, 8, 0, None, None, 0, 0.0, 0, 0,
                  None, None, None, None, None, 0, None)


def test_ablation_dropin_exports_the_models(msha, tmp_path):
    from msha_gnn_amd import layers, trainpy

    with trainpy.namespace(tmp_path, "cpu") as ns:
        import Ablation

        for name in ("OursLayer", "OursLayer2", "ablation2", "OursLayer3", "ablation3",
                     "GraphAttentionLayer"):
            assert getattr(Ablation, name) is getattr(layers, name), name
            if name != "GraphAttentionLayer":  # (HGANE's star import rebinds that one)
                assert ns[name] is getattr(layers, name), name  # train.py:6's star import


def test_constructors_match_the_reference(msha):
    """state_dict keys, shapes and bit-identical init under the reference's seeds."""
    from msha_gnn_amd import layers

    z = golden("ablations.npz")
    torch.manual_seed(10)
    layer = layers.OursLayer2(16, 8, 0.0)
    sd = layer.state_dict()
    assert list(sd) == [k[len("init."):] for k in z.files if k.startswith("init.")]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), z[f"init.{k}"]), k
    gdp = {i: float(x) for i, x in enumerate(z["gdp"])}
    m = z["a2.logp"].shape[1]
    torch.manual_seed(21)
    model = layers.ablation2(16, 8, n_classes=m, n_heads=2, dropout=0.0, gdp=gdp, Scount=64,
                             Rcount=m)
    sd = model.state_dict()
    want = [k[len("a2.state."):] for k in z.files if k.startswith("a2.state.")]
    assert list(sd) == want and len(want) == 44
    for k, v in sd.items():
        assert v.shape == z[f"a2.state.{k}"].shape, k
        assert np.array_equal(v.numpy(), z[f"a2.state.{k}"]), k
