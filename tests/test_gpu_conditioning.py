"""Every softmax path on ill-conditioned scores and scaled tables.

The other parity tests draw el, er and the tables from standard_normal: the scores stay
within a few units of 0, the online softmax's rescale factor near 1, lse near 0 and no exp
argument near the fp32 limits.  Here the edge-softmax family (edge_attention.hip,
edge_fwd_gl.hip, edge_bwd_gl.hip, edge_bip*.hip, the inter part of ours.hip, head.hip's
log-softmax) runs the regimes of gpu_helpers.score_regimes -- shifted, ramped, dominated
and kinked scores -- against the fp64 oracle on the stored values with the kernels' own
Philox masks, EVERY element within

    rtol |ref| + (4 sqrt(n) 2^-24 + 8 2^-24 S) A + 2^-100        (gpu_helpers.cond_close)

(rtol 1e-5 for fp32 tables, 1e-2 for bf16; S the largest |el_i + er_j| plus ln(max degree)),
and scales tables and upstream gradients by powers of two, which must scale every output
bit for bit.  tests/test_conditioning_host.py holds the reference itself to that bound."""
import os

import numpy as np
import pytest
import torch

from gpu_helpers import (COND_NAMES, REGIMES, cond_close, cond_inputs, cond_reference,
                         edge_abs_terms, t, tol_close)
from oracle import gnn_oracle as O
from test_gpu_bip import _run as _bip_run
from test_gpu_bip import bip_path  # noqa: F401  (the three bipartite settings)
from test_gpu_head import _run as _head_run
from test_gpu_kernels import _keep_mask, _u_only_grads
from test_gpu_ours import check_ours_attention_vs_dense
from test_gpu_row_scores import _rs_grads, _supported
from test_gpu_short_rows import _run as _general_run

pytestmark = pytest.mark.gpu

SEED = 29
F32, BF16 = torch.float32, torch.bfloat16
# every regime at p = 0; shift_up and ramp_up also under dropout
REGIME_P = [(r, 0.0) for r in REGIMES] + [("shift_up", 0.5), ("ramp_up", 0.5)]
_RP_IDS = [f"{r}-p{p}" for r, p in REGIME_P]
_DT_IDS = {F32: "f32", BF16: "bf16"}

_INPUTS, _GRAPHS, _REFS = {}, {}, {}


def _case(key, cuda):
    from msha_gnn_amd.graph import Graph

    if key not in _INPUTS:
        _INPUTS[key] = cond_inputs(key)
        _GRAPHS[key] = Graph.from_dense(t(_INPUTS[key]["c"], cuda))
    return _INPUTS[key], _GRAPHS[key]


def _stored(x, cuda, dtype):
    return t(x, cuda, dtype).double().cpu().numpy()


def _reference(key, regime, p, dtype, with_v, cuda):
    """The fp64 oracle on the stored values with the kernels' keep mask, computed once per
    (case, regime, p, dtype, branch) and shared by the paths (read-only)."""
    k = (key, regime, p, dtype, with_v)
    if k not in _REFS:
        x, graph = _case(key, cuda)
        el, er = x["regimes"][regime]
        H = x["shape"][2]
        keep = _keep_mask(graph.n_edges, H, p, SEED, cuda)
        st = lambda a: _stored(a, cuda, dtype)  # noqa: E731
        _REFS[k] = cond_reference(x["rowptr"], x["col"], x["empty"], el, er, st(x["hc"]),
                                  st(x["dU"]), hs=st(x["hs"]) if with_v else None,
                                  dV=st(x["dV"]) if with_v else None, keep=keep, p=p)[:3]
    return _REFS[k]


def _np(d):
    return {k: v.detach().float().cpu().numpy() for k, v in d.items()}


def _report(path, key, dtype, regime, p, worst):
    print(f"COND path={path} case={key} dtype={_DT_IDS[dtype]} regime={regime} p={p} "
          f"worst={worst:.3g}")


def _check_uv(path, runner, key, regime, p, dtype, cuda):
    """A u+v path (runner(MF, graph, el, er, hc, hs, dU, dV, p, seed, dev, dtype) -> the six
    outputs) against the oracle."""
    from msha_gnn_amd import functional as MF

    x, graph = _case(key, cuda)
    el, er = x["regimes"][regime]
    got = runner(MF, graph, el, er, x["hc"], x["hs"], x["dU"], x["dV"], p, SEED, cuda, dtype)
    refs, A, S = _reference(key, regime, p, dtype, True, cuda)
    worst = cond_close(_np(dict(zip(COND_NAMES, got))), refs, A, S,
                       1e-5 if dtype == F32 else 1e-2, f"{path} {key} {regime}")
    _report(path, key, dtype, regime, p, worst)


# --------------------------------------------- general score-layout kernels, u+v branch
def _split_runner(*a):
    return _general_run(*a, False)  # MF.BIP False, MSHA_FWD_GL=0, MSHA_BWD_GL=0


def _gather_runner(*a):
    return _general_run(*a, True)  # MF.BIP False, MSHA_FWD_GL=1, MSHA_BWD_GL=1


@pytest.mark.parametrize("regime,p", REGIME_P, ids=_RP_IDS)
@pytest.mark.parametrize("key,dtype", [("G1", F32), ("G2", F32), ("G3", F32), ("G1", BF16)],
                         ids=lambda v: _DT_IDS.get(v, v))
def test_split_uv_vs_oracle(cuda, msha, key, dtype, regime, p):
    """Score-layout forward with the attention export, bwd_rows + csc_aggregate."""
    _check_uv("split", _split_runner, key, regime, p, dtype, cuda)


# ------------------------------------------------------------------ gather-layout kernels
@pytest.mark.parametrize("regime,p", REGIME_P, ids=_RP_IDS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("key", ["S1", "S2"])
def test_gather_layout_vs_oracle(cuda, msha, key, dtype, regime, p):
    x, graph = _case(key, cuda)
    assert graph.n_edges <= 8 * x["shape"][0]  # the short-row dispatch
    _check_uv("gather", _gather_runner, key, regime, p, dtype, cuda)


# ---------------------------------------------------------------- u-only fused backward
_U_NAMES = ("u", "d_el", "d_er", "d_hc")


def _check_fused(path, key, regime, p, dtype, cuda, env=None):
    from msha_gnn_amd import functional as MF

    x, graph = _case(key, cuda)
    el, er = x["regimes"][regime]
    os.environ.update(env or {})
    try:
        runs = {rt: _u_only_grads(MF, graph, el, er, x["hc"], x["dU"], p, SEED, cuda, dtype, True,
                                  rowterms=rt) for rt in (False, True)}
    finally:
        for k in env or {}:
            os.environ.pop(k, None)
    refs, A, S = _reference(key, regime, p, dtype, False, cuda)
    for rt, got in runs.items():
        tag = f"{path}{'+rowterms' if rt else ''}"
        worst = cond_close(_np(dict(zip(_U_NAMES, got))), refs, A, S,
                           1e-5 if dtype == F32 else 1e-2, f"{tag} {key} {regime}")
        _report(tag, key, dtype, regime, p, worst)
    # the row terms change d_el's summation only
    for a, b, name in zip(runs[True], runs[False], _U_NAMES):
        if name != "d_el":
            assert torch.equal(a, b), name


@pytest.mark.parametrize("regime,p", REGIME_P, ids=_RP_IDS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("key", ["G1", "G2", "G3"])
def test_fused_backward_vs_oracle(cuda, msha, key, dtype, regime, p):
    """msha_edge_attention_bwd_fused with the row terms off and on (uc, qc through the
    forward's rescale)."""
    _check_fused("fused", key, regime, p, dtype, cuda)


@pytest.mark.parametrize("regime,p", REGIME_P, ids=_RP_IDS)
def test_fused_backward_pointer_loads_vs_oracle(cuda, msha, regime, p):
    _check_fused("fused-nobuf", "G2", regime, p, F32, cuda, env={"MSHA_COLS_NOBUF": "1"})


# -------------------------------------------------------------------------- row scores
@pytest.mark.parametrize("regime,p", [("none", 0.0), ("shift_up", 0.0), ("shift_down", 0.0),
                                      ("shift_up", 0.5)],
                         ids=["none-p0.0", "shift_up-p0.0", "shift_down-p0.0", "shift_up-p0.5"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("key", ["G1", "G2"])
def test_row_scores_vs_oracle(cuda, msha, key, dtype, regime, p):
    """er_j = hc_j . a_r recomputed from the gathered row with a_r = 16 standard_normal (er in
    the tens to hundreds), el shifted or not; the oracle is fed er in fp64 from the stored
    table, and S = max(|el_i| + sum_f |hc_jf a_rf|) over the edges."""
    from msha_gnn_amd import functional as MF

    x, graph = _case(key, cuda)
    n, m, H, F = x["shape"]
    rng = np.random.default_rng(5 + n + H)
    ar = (rng.standard_normal((H, F)) * 16).astype(np.float32)
    el = (rng.standard_normal((n, H)).astype(np.float32) if regime == "none"
          else x["regimes"][regime][0])
    hc_s, dU_s = _stored(x["hc"], cuda, dtype), _stored(x["dU"], cuda, dtype)
    ar64 = ar.astype(np.float64)
    er64 = np.einsum("mhf,hf->mh", hc_s, ar64)
    keep = _keep_mask(graph.n_edges, H, p, SEED, cuda)
    d = lambda a: a.astype(np.float64)  # noqa: E731
    fwd = O.edge_aggregate_fwd(x["rowptr"], x["col"], d(el), er64, hc_s, keep=keep, p=p,
                               rowflag=x["empty"])
    bw = O.edge_aggregate_bwd(x["rowptr"], x["col"], fwd, hc_s, dU_s, keep=keep, p=p)
    A = edge_abs_terms(x["rowptr"], x["col"], fwd, hc_s, dU_s, keep=keep, p=p)
    refs = dict(u=fwd["u"], d_el=bw["d_el"], d_er=bw["d_er"], d_hc=bw["d_hc"])
    rows = O.edge_rows(x["rowptr"])
    er_abs = np.einsum("mhf,hf->mh", np.abs(hc_s), np.abs(ar64))
    S = float((np.abs(d(el))[rows] + er_abs[x["col"].astype(np.int64)]).max())
    # where the row-score kernels apply, the er handed over is never read (a wrong one
    # proves it); elsewhere the op falls back to reading er
    hint = None if _supported(MF, graph, H, F, dtype) else er64.astype(np.float32)
    runs = {rt: _rs_grads(MF, graph, el, x["hc"], ar, x["dU"], p, SEED, cuda, dtype, rt,
                          er_hint=hint) for rt in (False, True)}
    for rt, got in runs.items():
        tag = f"rowscores{'+rowterms' if rt else ''}"
        worst = cond_close(_np(dict(zip(_U_NAMES, got))), refs, A, S,
                           1e-5 if dtype == F32 else 1e-2, f"{tag} {key} {regime}")
        _report(tag, key, dtype, regime, p, worst)
    for a, b, name in zip(runs[True], runs[False], _U_NAMES):
        if name != "d_el":
            assert torch.equal(a, b), name


# -------------------------------------------------------------------- bipartite kernels
def _bip_runner(*a):
    return _bip_run(*a, True)


@pytest.mark.parametrize("regime,p", REGIME_P, ids=_RP_IDS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("key", ["B1", "B2"])
def test_bip_vs_oracle(cuda, msha, bip_path, key, dtype, regime, p):  # noqa: F811
    """edge_bip.hip / edge_bip2.hip / edge_bip3.hip under the three settings (B2 is not
    2 x 64: it stays on the CSR walk of edge_bip.hip under every setting)."""
    from msha_gnn_amd import _lib

    x, graph = _case(key, cuda)
    _, _, H, F = x["shape"]
    assert _lib.load().msha_bip_supported(graph.desc, H, F, 1 if dtype == BF16 else 0) == 1
    bip_path.expect(graph, H, F, dtype, p)
    _check_uv(f"bip-{bip_path}", _bip_runner, key, regime, p, dtype, cuda)


# --------------------------------------------------------------------------------- Ours
@pytest.mark.parametrize("regime", ["shift_up", "dominant"])
def test_ours_inter_scores(cuda, msha, regime):
    """The inter softmax of ours.hip (a3s / a4s left alone: the reference's intra softmax is
    a raw exp sum)."""
    def hook(el, er):
        if regime == "shift_up":
            return el + np.float32(96), er
        er = er.copy()
        er[5] += np.float32(200)
        return el, er

    check_ours_attention_vs_dense(cuda, 0.0, score_hook=hook)


# --------------------------------------------------------------------------------- head
@pytest.mark.parametrize("w_scale", [2.0 ** 6, 2.0 ** -12], ids=["w2^6", "w2^-12"])
def test_head_scaled_w(cuda, msha, w_scale):
    """The 3000 x 32, 2 x 64 training case with W scaled: logits in the hundreds with elu
    saturated at -1, and expm1 near 0; the 1e-5 bar of test_head_train_matches_fp64."""
    out, ref, gr, _, (u, v, W, bns) = _head_run(cuda, 3000, 32, 2, 64, 0.0, True, sparse=True,
                                                 w_scale=w_scale)
    assert torch.isfinite(out).all()
    print(f"head w_scale {w_scale}: max |log-softmax| {float(ref.abs().max()):.4g}")
    tol_close(out.detach().cpu().numpy(), ref.numpy(), 1e-5, 1e-5)
    tol_close(u.grad.cpu().numpy(), gr["u"].numpy(), 1e-5, 1e-5)
    tol_close(v.grad.cpu().numpy(), gr["v"].numpy(), 1e-5, 1e-5)
    tol_close(W.grad.cpu().numpy(), gr["W"].numpy(), 1e-5, 1e-5)
    for h, (bu, bv) in enumerate(bns):
        tol_close(bu.weight.grad.cpu().numpy(), gr["uw"][h].numpy(), 1e-5, 1e-5)
        tol_close(bu.bias.grad.cpu().numpy(), gr["ub"][h].numpy(), 1e-5, 1e-5)
        tol_close(bv.weight.grad.cpu().numpy(), gr["vw"][h].numpy(), 1e-5, 1e-5)
        tol_close(bv.bias.grad.cpu().numpy(), gr["vb"][h].numpy(), 1e-5, 1e-5)


# ------------------------------------------------------------ exact scale invariance
SCALES = [(20, 20), (-20, 0), (0, -20)]


def _scaled_outputs(run, x, k, j):
    """run(hc, hs, dU, dV) -> the six outputs, with the tables scaled by 2^k and the
    upstream gradients by 2^j (exact in float32 and in bf16)."""
    a, b = np.float32(2.0 ** k), np.float32(2.0 ** j)
    return run(x["hc"] * a, x["hs"] * a, x["dU"] * b, x["dV"] * b)


def _check_scaling(run, x, names):
    """Scores untouched: u, v scale by 2^k, d_hc, d_hs by 2^j, d_el, d_er by 2^(k+j), bit
    for bit (bf16 RNE, the hi/mid/lo split and the u_lo residual are invariant under powers
    of two, and the summation order is fixed).  No reference needed."""
    base = _scaled_outputs(run, x, 0, 0)
    again = _scaled_outputs(run, x, 0, 0)
    for name, a, b in zip(names, base, again):
        assert torch.equal(a, b), f"{name}: two runs of the same input differ"
        assert torch.isfinite(a.float()).all() and bool((a != 0).any()), name
    for k, j in SCALES:
        got = _scaled_outputs(run, x, k, j)
        for name, g, b in zip(names, got, base):
            e = {"u": k, "v": k, "d_hc": j, "d_hs": j, "d_el": k + j, "d_er": k + j}[name]
            want = (b.double() * 2.0 ** e).to(b.dtype)
            bad = int((g != want).sum())
            assert bad == 0, (f"{name} at (k, j) = ({k}, {j}): {bad} of {g.numel()} elements "
                              f"are not the baseline times 2^{e}")


def _uv_scaling(runner, key, p, dtype, cuda):
    from msha_gnn_amd import functional as MF

    x, graph = _case(key, cuda)
    rng = np.random.default_rng(3)
    n, m, H, _ = x["shape"]
    el = rng.standard_normal((n, H)).astype(np.float32)
    er = rng.standard_normal((m, H)).astype(np.float32)
    _check_scaling(lambda hc, hs, dU, dV: runner(MF, graph, el, er, hc, hs, dU, dV, p, SEED,
                                                 cuda, dtype), x, COND_NAMES)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("path", ["split", "gather"])
def test_scale_invariance_general(cuda, msha, path, dtype, p):
    if path == "split":
        _uv_scaling(_split_runner, "G1", p, dtype, cuda)
    else:
        _uv_scaling(_gather_runner, "S1", p, dtype, cuda)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rowterms", [False, True], ids=["de", "rowterms"])
def test_scale_invariance_fused(cuda, msha, rowterms, dtype, p):
    from msha_gnn_amd import functional as MF

    x, graph = _case("G1", cuda)
    rng = np.random.default_rng(4)
    n, m, H, _ = x["shape"]
    el = rng.standard_normal((n, H)).astype(np.float32)
    er = rng.standard_normal((m, H)).astype(np.float32)
    _check_scaling(lambda hc, hs, dU, dV: _u_only_grads(MF, graph, el, er, hc, dU, p, SEED, cuda,
                                                        dtype, True, rowterms=rowterms),
                   x, _U_NAMES)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_scale_invariance_bip(cuda, msha, bip_path, dtype, p):  # noqa: F811
    x, graph = _case("B1", cuda)
    bip_path.expect(graph, x["shape"][2], x["shape"][3], dtype, p)
    _uv_scaling(_bip_runner, "B1", p, dtype, cuda)
