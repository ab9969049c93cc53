"""Writes tests/golden/llp_student.npz: what the reference's student encoder ``MLP``
(LLP.py:36-84) and ``KD_cosine`` (LLP.py:34-35) compute on seeded inputs.

    python tests/golden/make_golden_llp_student.py /path/to/the/reference/checkout

LLP.py runs as a script (argument parsing and training at import), so the two definitions
are taken out of its syntax tree and executed on their own, as make_golden.py does for such
files.  Needs the reference checkout; the tests only read the .npz (numeric arrays only).

Per ``k`` in 1, 2, 3 (``MLP(k, 16, 32, 8, 0.5)`` built after ``torch.manual_seed(k)``, eval
mode): ``mlp{k}.state.<key>`` the state_dict tensors, ``mlp{k}.x`` (40, 16) the input,
``mlp{k}.y`` the output, ``mlp{k}.dx`` and ``mlp{k}.grad.<key>`` the gradients of
``y.sum()``.  ``kd.s`` / ``kd.t`` (64, 32), ``kd.loss`` = KD_cosine(s, t) and ``kd.ds`` its
gradient.  All fp32 as the reference computes them.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

IN_DIM, HIDDEN, OUT_DIM, ROWS = 16, 32, 8, 40


def extract(path, names):
    """exec the named top-level ClassDef / FunctionDef nodes of a reference file."""
    tree = ast.parse(open(path, encoding="utf-8", errors="replace").read())
    ns = dict(torch=torch, nn=nn, F=F, np=np, cosine_similarity=F.cosine_similarity)
    found = {}
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
            found[node.name] = ns[node.name]
    return found


def main(reference):
    ref = extract(os.path.join(reference, "LLP.py"), {"MLP", "KD_cosine"})
    z = {}
    for k in (1, 2, 3):
        torch.manual_seed(k)
        mlp = ref["MLP"](k, IN_DIM, HIDDEN, OUT_DIM, 0.5)
        mlp.eval()
        x = torch.randn(ROWS, IN_DIM, generator=torch.Generator().manual_seed(100 + k))
        x.requires_grad_(True)
        y = mlp(x)
        y.sum().backward()
        for key, v in mlp.state_dict().items():
            z[f"mlp{k}.state.{key}"] = v.detach().numpy().copy()
        for key, p in mlp.named_parameters():
            z[f"mlp{k}.grad.{key}"] = p.grad.numpy().copy()
        z[f"mlp{k}.x"] = x.detach().numpy().copy()
        z[f"mlp{k}.y"] = y.detach().numpy().copy()
        z[f"mlp{k}.dx"] = x.grad.numpy().copy()
    g = torch.Generator().manual_seed(7)
    s = torch.randn(64, 32, generator=g).requires_grad_(True)
    t = torch.randn(64, 32, generator=g)
    loss = ref["KD_cosine"](s, t)
    loss.backward()
    z["kd.s"], z["kd.t"] = s.detach().numpy().copy(), t.numpy().copy()
    z["kd.loss"] = loss.detach().numpy().copy()
    z["kd.ds"] = s.grad.numpy().copy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "llp_student.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
