"""Writes tests/golden/ablations.npz: what the reference's ``OursLayer2`` and ``ablation2``
(Ablation.py:140-231) compute on seeded inputs.

    python tests/golden/make_golden_ablations.py /path/to/the/reference/checkout

Ablation.py imports cleanly, so it is imported as a module (with the reference's
``model.normalize_adjacency_matrix`` for the adjacencies).  Needs the reference checkout
and tests/golden/ours_small.npz (the 64-source graph: ``counts``, ``city``, ``prov``, case
B's batch with a repeated source and its empty inter row); the tests only read the .npz
(numeric arrays only).

``OursLayer2(16, 8, 0.0)`` after ``torch.manual_seed(10)``, case A (no prefix) in fp32 and
case B (``B.``) in fp64: ``init.<key>`` the state_dict at init, ``S`` / ``R`` the inputs,
``source_index``, ``out_eval`` (eval mode, BatchNorm statistics at init), ``out`` (train
mode, p = 0), ``dout`` the weights w of the loss ``(out * w).sum()``, ``grad.S`` / ``grad.R``
/ ``grad.<parameter>`` its gradients.

``ablation2`` (``a2.``), ``(16, 8, n_classes=M, n_heads=2, dropout=0.0, gdp, 64, M)`` after
``torch.manual_seed(21)``, fp32 on case A's graph: ``state.<key>`` the state_dict,
``source_index`` / ``recipient_index`` the batch (with a repeated source), ``logp_eval`` / ``logp`` the (N, M) log-probabilities in eval / train mode, ``loss`` =
``nll_loss(logp[source_index], recipient_index)`` and ``grad.<parameter>`` its gradients.
``gdp`` (64,) the GDP values of the constructor's dict (keys 0..63 in order).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))


def main(reference):
    sys.path.insert(0, reference)
    import Ablation as ref  # noqa: E402  (reference)
    from model import normalize_adjacency_matrix  # noqa: E402  (reference)

    z = np.load(os.path.join(OUT, "ours_small.npz"))
    city, prov = z["city"], z["prov"]
    city_adj = torch.as_tensor((city[:, None] == city[None, :]).astype(np.float32))
    prov_adj = torch.as_tensor((prov[:, None] == prov[None, :]).astype(np.float32))
    res = {}
    for tag, dt in (("", torch.float32), ("B.", torch.float64)):
        c = torch.as_tensor(z[tag + "counts"] if tag + "counts" in z.files else z["counts"])
        inter = normalize_adjacency_matrix(c).to(dt)
        city_n = normalize_adjacency_matrix(city_adj).to(dt)
        prov_n = normalize_adjacency_matrix(prov_adj).to(dt)
        torch.manual_seed(10)
        layer = ref.OursLayer2(16, 8, 0.0)
        if tag == "":
            for k, v in layer.state_dict().items():
                res[f"init.{k}"] = v.numpy().copy()
        layer = layer.to(dt)
        S = torch.as_tensor(z[tag + "S"]).to(dt).requires_grad_(True)
        R = torch.as_tensor(z[tag + "R"]).to(dt).requires_grad_(True)
        si = torch.as_tensor(z[tag + "source_index"])
        res[tag + "S"], res[tag + "R"] = S.detach().numpy(), R.detach().numpy()
        res[tag + "source_index"] = si.numpy()
        layer.eval()  # before the train forward: BN running stats still at init
        with torch.no_grad():
            res[tag + "out_eval"] = layer(S, R, inter, city_n, prov_n, si).numpy()
        layer.train()
        y = layer(S, R, inter, city_n, prov_n, si)
        w = torch.randn(y.shape, generator=torch.Generator().manual_seed(12),
                        dtype=torch.float64).to(dt)
        (y * w).sum().backward()
        res[tag + "out"], res[tag + "dout"] = y.detach().numpy(), w.numpy()
        res[tag + "grad.S"], res[tag + "grad.R"] = S.grad.numpy(), R.grad.numpy()
        for k, p in layer.named_parameters():
            if p.grad is not None:
                res[f"{tag}grad.{k}"] = p.grad.numpy()

    counts = torch.as_tensor(z["counts"])
    n, m = counts.shape
    inter = normalize_adjacency_matrix(counts)
    city_n = normalize_adjacency_matrix(city_adj)
    prov_n = normalize_adjacency_matrix(prov_adj)
    gdp = {i: 0.1 * i for i in range(n)}
    res["gdp"] = np.asarray(list(gdp.values()), np.float32)
    si = torch.as_tensor([5, 17, 5, 40, 33, 5, 60, 12, 1, 2, 3, 8])  # a repeated source
    ri = torch.randint(0, m, si.shape, generator=torch.Generator().manual_seed(13))
    for tag, cls, seed in (("a2.", ref.ablation2, 21),):
        torch.manual_seed(seed)
        model = cls(16, 8, m, 2, 0.0, gdp, n, m)
        for k, v in model.state_dict().items():
            res[f"{tag}state.{k}"] = v.numpy().copy()
        res[tag + "source_index"], res[tag + "recipient_index"] = si.numpy(), ri.numpy()
        model.eval()
        with torch.no_grad():
            res[tag + "logp_eval"] = model(inter, city_n, prov_n, si).numpy()
        model.train()
        out = model(inter, city_n, prov_n, si)
        loss = F.nll_loss(out[si], ri)
        loss.backward()
        res[tag + "logp"] = out.detach().numpy()
        res[tag + "loss"] = loss.detach().numpy()
        for k, p in model.named_parameters():
            if p.grad is not None:
                res[f"{tag}grad.{k}"] = p.grad.numpy()
    path = os.path.join(OUT, "ablations.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
