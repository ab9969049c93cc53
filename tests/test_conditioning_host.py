"""Host-side guard of the ill-conditioned score regimes (gpu_helpers.score_regimes) that
tests/test_gpu_conditioning.py feeds the edge-softmax kernels: the regimes do what their
table claims, and the reference alone -- the oracle's own fp32 run against its fp64 run --
stays well inside the bound the kernels are held to (gpu_helpers.cond_close)."""
import numpy as np
import pytest

from gpu_helpers import COND_CASES, REGIMES, cond_close, cond_inputs, cond_reference
from oracle import gnn_oracle as O


@pytest.fixture(scope="module", params=["G1", "S1", "B1"])
def case(request):
    return request.param, cond_inputs(request.param)


@pytest.mark.parametrize("regime", REGIMES)
def test_oracle_finite_and_fp32_run_within_bound(case, regime):
    key, x = case
    el, er = x["regimes"][regime]
    refs, A, S, fwd = cond_reference(x["rowptr"], x["col"], x["empty"], el, er, x["hc"], x["dU"],
                                     hs=x["hs"], dV=x["dV"])
    for name, r in refs.items():
        assert np.isfinite(r).all(), (key, regime, name)
    assert np.isfinite(fwd["att"]).all()
    f32 = O.edge_aggregate_fwd(x["rowptr"], x["col"], el, er, x["hc"], hs=x["hs"],
                               rowflag=x["empty"])
    b32 = O.edge_aggregate_bwd(x["rowptr"], x["col"], f32, x["hc"], x["dU"], hs=x["hs"],
                               dV=x["dV"])
    got = dict(u=f32["u"], v=f32["v"], d_el=b32["d_el"], d_er=b32["d_er"], d_hc=b32["d_hc"],
               d_hs=b32["d_hs"])
    assert all(v.dtype == np.float32 for v in got.values())
    worst = cond_close(got, refs, A, S, 1e-5, f"{key} {regime} oracle fp32")
    print(f"{key} {regime}: S {S:.1f}, oracle fp32 worst err / bound {worst:.3g}")
    assert worst <= 0.25


def test_kink_hits_zero_exactly(case):
    key, x = case
    el, er = x["regimes"]["kink"]
    rows = O.edge_rows(x["rowptr"])
    pre = el[rows] + er[x["col"].astype(np.int64)]
    share = float((pre == 0).mean())
    print(f"{key} kink: pre == 0 on {share:.1%} of the edges")
    assert share >= 0.20


def test_dominant_underflows_the_rest_of_its_rows(case):
    key, x = case
    n, m, H, F = x["shape"]
    el, er = x["regimes"]["dominant"]
    fwd = O.edge_aggregate_fwd(x["rowptr"], x["col"], el.astype(np.float64),
                               er.astype(np.float64), x["hc"].astype(np.float64),
                               rowflag=x["empty"])
    rows = O.edge_rows(x["rowptr"])
    holds = np.zeros(n, bool)
    holds[rows[x["col"] == 5]] = True
    att = fwd["att"][holds[rows]]
    share = float((att < 2.0 ** -126).mean())
    print(f"{key} dominant: {holds.mean():.1%} of the rows hold column 5; {share:.1%} of their "
          f"weights are below 2^-126")
    assert holds.mean() >= 0.10
    assert share >= 0.80
    # the dominant edge's weight is exactly 1 in fp32 on the real rows
    on5 = (x["col"] == 5) & ~x["empty"][rows]
    assert (fwd["att"][on5].astype(np.float32) == 1).all()


def test_cases_are_the_shapes_the_gpu_tests_name():
    assert COND_CASES["G1"][:5] == (150, 80, 1, 8, 80)
    assert COND_CASES["S1"][:5] == (400, 32, 2, 64, 12)
    assert COND_CASES["B1"][:5] == (700, 32, 2, 64, 32)
