"""Host side of the device evaluation: the numpy oracle (tests/eval_ref.py) and
``metrics.metrics_from_confusion`` / ``auc_columns`` / ``auc_from_counts`` against the
reference's recorded outputs (tests/golden/eval_metrics.npz) and, where it imports,
against sklearn.  No GPU."""
import numpy as np
import pytest

import eval_ref as R
from conftest import golden

import msha_loader

msha_loader.load()
from msha_gnn_amd import metrics as M  # noqa: E402

KEYS = ("accuracy", "precision_macro", "recall_macro", "precision_micro", "recall_micro")


@pytest.fixture(scope="module")
def fx():
    z = golden("eval_metrics.npz")
    return {str(n): {k: z[f"{n}.{k}"] for k in ("table", "src", "y", "pred", "ref")}
            for n in z["names"]}


def test_fixture_covers_the_cases(fx):
    assert set(fx) == {"c32", "three", "dup", "missing", "two", "pred_never_true",
                       "true_never_pred"}
    assert fx["c32"]["table"].shape[1] == 32
    assert len(np.unique(fx["three"]["table"])) == 3
    assert len(np.unique(fx["dup"]["src"])) < len(fx["dup"]["src"])
    assert 2 not in fx["missing"]["y"] and len(np.unique(fx["missing"]["y"])) == 5
    assert len(np.unique(fx["two"]["y"])) == 2
    c = fx["pred_never_true"]
    assert (c["pred"] == 4).any() and not (c["y"] == 4).any()
    c = fx["true_never_pred"]
    assert (c["y"] == 4).any() and not (c["pred"] == 4).any()


def test_oracle_matches_reference_outputs(fx):
    for name, c in fx.items():
        rows = c["table"][c["src"]]
        np.testing.assert_array_equal(R.argmax_lowest(rows), c["pred"], err_msg=name)
        assert abs(R.calculate_auc(rows, c["y"]) - c["ref"][0]) <= 1e-12, name
        got = R.prf(c["y"], c["pred"])
        for k, want in zip(KEYS, c["ref"][1:]):
            assert got[k] == want, (name, k, got[k], want)


def test_metrics_from_confusion_matches_reference_outputs(fx):
    for name, c in fx.items():
        C = c["table"].shape[1]
        got = M.metrics_from_confusion(R.confusion(c["y"], c["pred"], C))
        for k, want in zip(KEYS, c["ref"][1:]):
            assert got[k] == want, (name, k, got[k], want)


def test_auc_columns_keeps_the_pairing_quirks(fx):
    assert M.auc_columns([0, 1, 3, 4, 5], 6) == [0, 1, 3, 4, 5]
    assert M.auc_columns([1, 3], 4) == [3]
    for name, c in fx.items():
        C = c["table"].shape[1]
        assert M.auc_columns(np.unique(c["y"]), C) == R.auc_classes(c["y"], C), name


def test_auc_from_counts_is_the_oracle_quotient(fx):
    for name, c in fx.items():
        rows = c["table"][c["src"]]
        cls = R.auc_classes(c["y"], rows.shape[1])
        counts = [R.rank_counts(rows[:, k], c["y"] == q) + (0,) for k, q in enumerate(cls)]
        assert M.auc_from_counts(counts) == R.calculate_auc(rows, c["y"]), name
        assert abs(M.auc_from_counts(counts) - c["ref"][0]) <= 1e-12, name


def test_rank_counts_edge_cases():
    # all equal: exactly one half; -0.0 ties +0.0; a denormal is above zero
    assert R.column_auc(np.zeros(7), np.arange(7) < 3) == 0.5
    assert R.column_auc(np.array([-0.0, 0.0]), np.array([True, False])) == 0.5
    tiny = np.float32(1e-45)
    assert R.column_auc(np.array([0.0, tiny], np.float32), np.array([False, True])) == 1.0
    assert R.rank_counts([0.1, 0.4, 0.35, 0.8], [False, False, True, True]) == (2, 2, 6)


def test_value_and_index_errors():
    with pytest.raises(ValueError):
        M.auc_columns([3], 4)
    with pytest.raises(ValueError):
        M.auc_columns([], 4)
    with pytest.raises(ValueError):
        M.auc_columns([0, 1, 2], 2)
    with pytest.raises(ValueError):
        M.auc_from_counts([[0, 5, 0, 0]])
    with pytest.raises(ValueError):
        R.calculate_auc(np.zeros((4, 3)), np.array([1, 1, 1, 1]))
    with pytest.raises(ValueError):
        R.calculate_auc(np.zeros((4, 2)), np.array([0, 1, 2, 2]))
    with pytest.raises(ValueError):
        M.metrics_from_confusion(np.zeros((2, 3), np.int64))
    with pytest.raises(IndexError):
        R.confusion([0, 5], [0, 1], 4)
    assert np.isnan(M.auc_from_counts([[3, 4, 10, 0], [2, 5, 9, 1]]))


def test_oracle_matches_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for n, vals in ((2, None), (65, None), (4097, 3), (23389, None), (23389, 5)):
        s = (rng.standard_normal(n) if vals is None
             else rng.choice(rng.standard_normal(vals), n)).astype(np.float32)
        pos = rng.random(n) < 0.3
        pos[0], pos[1] = True, False
        assert abs(R.column_auc(s, pos) - sk.roc_auc_score(pos, s)) <= 1e-12, (n, vals)
    y = rng.integers(0, 7, 500)
    p = rng.integers(0, 9, 500)
    got = M.metrics_from_confusion(R.confusion(y, p, 9))
    assert got["accuracy"] == sk.accuracy_score(y, p)
    for avg in ("macro", "micro"):
        assert got[f"precision_{avg}"] == sk.precision_score(y, p, average=avg, zero_division=1)
        assert got[f"recall_{avg}"] == sk.recall_score(y, p, average=avg, zero_division=1)
