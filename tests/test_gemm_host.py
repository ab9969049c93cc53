"""Host checks of the GEMM layout sweep's inputs (tests/gemm_ref.py): what
tests/test_gpu_gemm_layouts.py relies on is a property of its tables, checked here without
a GPU -- the views have the strides, misalignment and NaN surround each case asks for, every
integer case's sums stay below 2^24 (so bit equality is owed by any summation order), and
the documented layout rules send each case to the loader it was written for."""
import numpy as np
import pytest
import torch

import gemm_ref as G

GEMM_TABLES = G.F32_CASES + G.WGRAD_CASES + G.BF16_CASES + G.BF16_REFUSALS


def _ids(cs):
    return [c["name"] for c in cs]


def test_case_names_unique():
    names = _ids(GEMM_TABLES + G.HO_CASES + G.PROJ_CASES)
    assert len(names) == len(set(names))


@pytest.mark.parametrize("c", GEMM_TABLES, ids=_ids(GEMM_TABLES))
def test_views_are_what_the_case_asks(c):
    A, B, ref = G.case_operands(c)
    M, N, K = c["M"], c["N"], c["K"]
    for v, sp, (R, C) in ((A, c["a"], (M, K)), (B, c["b"], (K, N))):
        assert v.shape == (R, C)
        vals = v.values()
        assert np.isfinite(vals).all() and np.abs(vals).max() <= 8
        if sp["order"] == "zero":
            assert v.strides == (0, 0) and np.all(vals == 1)
        else:
            line, other = (1, 0) if sp["order"] == "r" else (0, 1)
            assert v.strides[line] == sp["step"]
            if sp["pitch"] is not None:
                assert v.strides[other] == sp["pitch"]
            else:
                assert v.strides[other] % 8 == 0  # default pitch: vector loads allowed
            # pitch padding exists between the lines (a NaN right after each line)
            assert v.strides[other] > (v.shape[line] - 1) * sp["step"] or v.shape[other] == 1
        for itemsize in (2, 4):
            assert v.misalign(itemsize) == (sp["off"] * itemsize) % 16
        # NaN before, after and between: everything that is not an element of the window
        out = v.outside()
        assert np.isnan(v.buf[out]).all() and np.isfinite(v.buf[~out]).all()
        assert out[:G.GUARD].all() and out[-G.GUARD:].all()
        assert v.buf.size * 4 < 4 << 20  # the largest device buffer stays under 4 MB
    np.testing.assert_array_equal(ref, A.values() @ B.values())
    O = G.out_view(M, N, c["ldc"], c["coff"], G.case_prior(c))
    assert O.strides == (c["ldc"], 1) and O.misalign(4) == (c["coff"] * 4) % 16
    assert np.isnan(O.buf[O.outside()]).all()
    assert np.isfinite(O.values()).all() == bool(c["accumulate"])


@pytest.mark.parametrize("c", GEMM_TABLES, ids=_ids(GEMM_TABLES))
def test_integer_sums_below_2_24(c):
    """sum |A| |B| (+ |C| when accumulating) < 2^24: every partial sum, in any order, is an
    exactly representable integer; a bf16 C's reference is finite once rounded."""
    A, B, ref = G.case_operands(c)
    absum = np.abs(A.values()) @ np.abs(B.values())
    if c["accumulate"]:
        absum = absum + np.abs(G.case_prior(c))
    assert absum.max() < G.EXACT
    if c.get("cbf"):
        assert torch.isfinite(torch.as_tensor(ref, dtype=torch.float32).to(torch.bfloat16)).all()


@pytest.mark.parametrize("c", G.HO_CASES, ids=_ids(G.HO_CASES))
def test_head_outer_sums_below_2_24(c):
    d = G.ho_operands(c)
    assert d["absum"].max() < G.EXACT
    # the operand sum itself is an integer a bf16 holds exactly (the bf16 kernel rounds it)
    assert np.abs(d["tot"]).max() <= 256
    np.testing.assert_array_equal(
        d["ref"], d["tot"] @ d["other"].T if c["operand"] == 0 else d["other"].T @ d["tot"])


@pytest.mark.parametrize("c", G.PROJ_CASES, ids=_ids(G.PROJ_CASES))
def test_project_scores_sums_below_2_24(c):
    assert 256 < c["M"] < 1024
    assert G.proj_abs_max(c) < G.EXACT


@pytest.mark.parametrize("c", G.F32_CASES + G.WGRAD_CASES, ids=_ids(G.F32_CASES + G.WGRAD_CASES))
def test_f32_rule_predicts_the_intended_loader(c):
    assert G.predict_f32(c["M"], c["N"], c["K"], *G.case_strides(c, 4)) == c["loader"]


@pytest.mark.parametrize("c", G.BF16_CASES + G.BF16_REFUSALS,
                         ids=_ids(G.BF16_CASES + G.BF16_REFUSALS))
def test_bf16_rule_predicts_the_intended_loader(c):
    assert G.predict_bf16(c["M"], c["N"], c["K"], *G.case_strides(c, 2)) == c["loader"]


def test_tables_reach_every_loader():
    assert {c["loader"] for c in G.F32_CASES} == G.F32_LOADERS
    assert {c["loader"] for c in G.BF16_CASES} == G.BF16_LOADERS
    # the scalar loader by each cause alone: the named cases exist
    names = set(_ids(G.F32_CASES))
    for n in ("a-base+1", "b-base+1", "K1-a-kcontig", "K3-a-kcontig", "K31-a-kcontig",
              "K33-a-kcontig", "N130-b-ncontig", "M130-a-mcontig", "a-pitch37", "a-step2",
              "ones-row-N3", "M1", "N1", "K1"):
        assert "edge-" + n in names


def test_each_scalar_cause_stands_alone():
    """Undoing the one named condition of a scalar case gives a vector loader: nothing else
    in the case would have sent it to the scalar path."""
    by = {c["name"]: c for c in G.F32_CASES}

    def with_(c, **kw):
        d = dict(c)
        d.update(kw)
        return G.predict_f32(d["M"], d["N"], d["K"], *G.case_strides(d, 4))

    r, cc = G.spec("r"), G.spec("c")
    assert with_(by["edge-a-base+1"], a=r) & G.VEC
    assert with_(by["edge-b-base+1"], b=r) & G.VEC
    assert with_(by["edge-at-base+1"], a=cc) & G.VEC
    for k in (1, 3, 31, 33):
        assert with_(by[f"edge-K{k}-a-kcontig"], K=36) & G.VEC
    for k in (3, 33):
        assert with_(by[f"edge-K{k}-b-kcontig"], K=36) & G.VEC
    assert with_(by["edge-N130-b-ncontig"], N=132) & G.VEC
    assert with_(by["edge-M130-a-mcontig"], M=132) & G.VEC
    assert with_(by["edge-a-pitch37"], a=r) & G.VEC
    assert with_(by["edge-b-pitch133"], b=r) & G.VEC
    assert with_(by["edge-at-pitch134"], a=cc) & G.VEC
    assert with_(by["edge-bt-pitch38"], b=cc) & G.VEC
    assert with_(by["edge-a-step2"], a=r) & G.VEC
    assert with_(by["edge-b-step2"], b=r) & G.VEC
