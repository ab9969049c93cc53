"""Writes tests/golden/hgane.npz: what the reference's HGANE ``GraphAttentionLayer``
(HGANE.py:11-76) computes on seeded inputs, in fp32 and in fp64.

    python tests/golden/make_golden_hgane.py /path/to/the/reference/checkout

HGANE.py imports cleanly (it needs sklearn), so it is imported as a module.  The tests only
read the .npz (numeric arrays only).

Two cases, ``A.`` (in = 16, F = 16, seed 31) and ``B.`` (in = 128, F = 64, seed 32), both on
N = 400 sources and M = 32 recipients:

  gid           (N,) group of each node: seven groups; the batch draws from six of them
                segments of 1, 31, 32, 33, 65 and 130 entries (B = 292, on both sides of the
                32 and 64 tile edges, one single-member group), 25 of them repeated sources
  src           (B,) the shuffled batch
  counts        (N, M) uint8 inter adjacency; degrees drawn from the 2015 graph's law (mostly
                1-3, some 5 / 8 / 30), every row >= 1
  gdp           (N,) the constructor's GDP values (keys 0..N-1 in order)
  init.<key>    the state_dict after ``torch.manual_seed(seed)`` (case B: without the two
                (N, in) tables ``features`` and ``source_embedding``: they are the first two
                ``torch.rand([N, in])`` draws under the seed, as case A's stored tables show)
  out_eval32/64 eval-mode output (BatchNorm statistics at init), case A only
  out32/64      train-mode output, dropout 0
  (dout)        the weights w of the loss ``(out * w).sum()`` are not stored:
                ``dout_weights(seed, B)`` below (numpy's PCG64 stream), which
                tests/hgane_ref.py repeats
  grad32/64.<parameter>   its gradients; ``features`` has none.  Case B's
                ``source_embedding``: ``grad64`` on the rows ``emb_rows`` (the sources that
                occur; the rest are exact zeros) and, instead of ``grad32``,
                ``graderr.source_embedding`` = max |grad32 - grad64| of each of those rows
                (all the tests' bound takes from the fp32 run)
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
N, M = 400, 32
SEGMENTS = ((1, 1, 0), (40, 28, 3), (40, 28, 4), (40, 29, 4), (80, 60, 5), (150, 121, 9))


def dout_weights(seed, B):
    """(B, M) float32 weights of the loss functional of the case with that seed."""
    return np.random.default_rng(seed + 100).standard_normal((B, M)).astype(np.float32)


def graph(rng):
    """(gid, src, counts): node groups, the shuffled batch and the inter adjacency."""
    nodes = rng.permutation(N)
    gid = np.full(N, len(SEGMENTS), np.int64)  # the rest: a group outside the batch
    batch, at = [], 0
    for g, (size, distinct, dup) in enumerate(SEGMENTS):
        members = nodes[at:at + size]
        at += size
        gid[members] = g
        picked = rng.choice(members, distinct, replace=False)
        batch += list(picked) + list(rng.choice(picked, dup, replace=True))
    src = rng.permutation(np.asarray(batch, np.int64))
    deg = rng.choice([1, 2, 3, 5, 8, 30], N, p=[0.45, 0.3, 0.15, 0.05, 0.03, 0.02])
    counts = np.zeros((N, M), np.uint8)
    for i in range(N):
        counts[i, rng.choice(M, deg[i], replace=False)] = 1
    return gid, src, counts


def main(reference):
    sys.path.insert(0, reference)
    import HGANE as ref  # noqa: E402  (reference)

    res = {}
    for tag, fin, fout, seed in (("A.", 16, 16, 31), ("B.", 128, 64, 32)):
        rng = np.random.default_rng(seed)
        gid, src, counts = graph(rng)
        gdp = {i: float(x) for i, x in enumerate(rng.random(N).astype(np.float32))}
        res[tag + "gid"], res[tag + "src"], res[tag + "counts"] = gid, src, counts
        res[tag + "gdp"] = np.asarray(list(gdp.values()), np.float32)
        dout = torch.as_tensor(dout_weights(seed, len(src))).double()
        rows = np.unique(src)
        if tag == "B.":
            res[tag + "emb_rows"] = rows
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            torch.manual_seed(seed)
            layer = ref.GraphAttentionLayer(fin, fout, N, M, gdp, dropout=0.0)
            if bits == 32:
                for k, v in layer.state_dict().items():
                    if not (tag == "B." and k in ("features", "source_embedding")):
                        res[f"{tag}init.{k}"] = v.numpy().copy()
            layer = layer.to(dt)
            inter = torch.as_tensor(counts).to(dt)
            intra = torch.as_tensor(gid[:, None] == gid[None, :]).to(dt)
            si = torch.as_tensor(src)
            layer.eval()  # before the train forward: BN running stats still at init
            with torch.no_grad():
                out_eval = layer(inter, intra, si).numpy()
            if tag == "A.":
                res[f"{tag}out_eval{bits}"] = out_eval
            layer.train()
            y = layer(inter, intra, si)
            (y * dout.to(dt)).sum().backward()
            res[f"{tag}out{bits}"] = y.detach().numpy()
            assert np.isfinite(res[f"{tag}out{bits}"]).all()
            for k, p in layer.named_parameters():
                if p.grad is None:
                    assert k == "features", k
                    continue
                g = p.grad.numpy()
                if k == "source_embedding":
                    other = np.setdiff1d(np.arange(N), rows)
                    assert not g[other].any()
                    if tag == "B.":
                        g = g[rows]
                res[f"{tag}grad{bits}.{k}"] = g.copy()
        if tag == "B.":
            g32 = res.pop("B.grad32.source_embedding").astype(np.float64)
            res["B.graderr.source_embedding"] = np.abs(
                g32 - res["B.grad64.source_embedding"]).max(axis=1)
    path = os.path.join(OUT, "hgane.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
