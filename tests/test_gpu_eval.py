"""Device-side evaluation (csrc/eval.hip, metrics.Evaluator / binary_auc, TrainPy.test_epoch)
against the numpy oracle tests/eval_ref.py and the reference's recorded outputs
(tests/golden/eval_metrics.npz).  The rank statistic is integer arithmetic on the device,
so P, Nn and U2 are compared for equality and the AUC bitwise."""
import numpy as np
import pytest
import torch

import eval_ref as R
from conftest import golden

import msha_loader

msha_loader.load()
from msha_gnn_amd import _lib as L  # noqa: E402
from msha_gnn_amd import metrics as M  # noqa: E402
from msha_gnn_amd import trainpy  # noqa: E402

pytestmark = pytest.mark.gpu

CMAX = 128
COLUMNS = (1, 2, 3, 32, 33, 128)
KINDS = ("normal", "equal", "three", "zeros", "denormal", "bf16")
BIG = 70001


def _cut():
    return int(L.load().msha_rank_auc_block_keys())


def _sizes():
    cut = _cut()
    return sorted({2, 63, 64, 65, 255, 256, 257, 4097, cut, cut + 1, 2 * cut + 1, BIG})


def _scores(kind, n, c, rng):
    if kind == "normal":
        return rng.standard_normal((n, c)).astype(np.float32)
    if kind == "equal":
        return np.full((n, c), 0.5, np.float32)
    if kind == "three":
        return rng.choice(np.array([-1.5, 0.25, 3.0], np.float32), (n, c))
    if kind == "zeros":
        return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], np.float32), (n, c))
    if kind == "denormal":
        tiny = np.array([1, 2, 0x80000001, 0x80000002, 0, 0x80000000, 0x00800000], np.uint32)
        return rng.choice(tiny.view(np.float32), (n, c))
    x = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32))
    return x.bfloat16().float().numpy()


def _labels(n, rng):
    """Labels over [0, L), L = min(n, CMAX), each present: with cls[k] = k % L every column
    has a positive and (L >= 2) a negative."""
    nl = min(n, CMAX)
    y = np.concatenate([np.arange(nl), rng.integers(0, nl, n - nl)])
    rng.shuffle(y)
    return y.astype(np.int64), nl


def _rank_auc(dev, scores, y, columns, cls=None, binary=False):
    s = torch.as_tensor(np.ascontiguousarray(scores), device=dev)
    yt = torch.as_tensor(y, device=dev)
    ct = None if cls is None else torch.as_tensor(np.asarray(cls, np.int32), device=dev)
    out = M._rank_auc(s, s.shape[0], columns, s.shape[1], yt, ct, binary, {})
    return out.cpu().numpy()


def _oracle(scores, y, cls):
    return np.array([R.rank_counts(scores[:, k], y == q) for k, q in enumerate(cls)], np.int64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", _sizes() if L.available() else [2])
def test_rank_auc_matches_oracle(cuda, n, kind):
    rng = np.random.default_rng(n * 7 + KINDS.index(kind))
    cmax = 3 if n == BIG else CMAX
    scores = _scores(kind, n, cmax, rng)
    y, nl = _labels(n, rng)
    cls = np.arange(cmax) % nl
    want = _oracle(scores, y, cls)  # column k's counts do not depend on the column count
    assert (want[:, 0] > 0).all() and (want[:, 1] > 0).all()
    for c in COLUMNS:
        if c > cmax:
            continue
        got = _rank_auc(cuda, scores, y, c, cls=None if c <= nl else cls[:c])
        np.testing.assert_array_equal(got[:, :3], want[:c], err_msg=f"C={c}")
        assert (got[:, 3] == 0).all()
        for k in range(c):
            auc = M.auc_from_counts(got[k:k + 1])
            assert auc == R.auc_from(*(int(v) for v in want[k])), (c, k)
            if kind == "equal":
                assert auc == 0.5
    got = _rank_auc(cuda, scores, y, min(3, cmax), cls=cls[:min(3, cmax)])  # explicit map
    np.testing.assert_array_equal(got[:, :3], want[:min(3, cmax)])


@pytest.mark.parametrize("n", _sizes() if L.available() else [2])
def test_rank_auc_binary_mode(cuda, n):
    rng = np.random.default_rng(n)
    for kind in KINDS:
        scores = _scores(kind, n, 1, rng)
        y = rng.integers(0, 3, n).astype(np.int64)  # any non-zero label is positive
        y[0], y[1] = 0, 2
        got = _rank_auc(cuda, scores, y, 1, binary=True)
        assert tuple(int(v) for v in got[0, :3]) == R.rank_counts(scores[:, 0], y != 0), kind
        assert got[0, 3] == 0


@pytest.mark.parametrize("n", [257, "cut+1"])
def test_rank_auc_reports_nonfinite_per_column(cuda, n):
    n = _cut() + 1 if n == "cut+1" else n
    rng = np.random.default_rng(3)
    scores = _scores("normal", n, 3, rng)
    y = rng.integers(0, 3, n).astype(np.int64)
    y[:3] = [0, 1, 2]
    clean = _rank_auc(cuda, scores, y, 3)
    scores[5, 1], scores[n - 1, 1], scores[n // 2, 1] = np.nan, np.inf, -np.inf
    scores[7, 1] = -np.nan
    got = _rank_auc(cuda, scores, y, 3)
    assert got[:, 3].tolist() == [0, 4, 0]
    np.testing.assert_array_equal(got[[0, 2]], clean[[0, 2]])
    assert np.isnan(M.auc_from_counts(got)) and not np.isnan(M.auc_from_counts(got[[0, 2]]))


def test_binary_auc(cuda):
    rng = np.random.default_rng(11)
    for n in (1000, _cut() + 1):
        s = rng.standard_normal(n).astype(np.float32).round(2)
        y = rng.random(n) < 0.4
        y[0], y[1] = True, False
        want = R.column_auc(s, y)
        st = torch.as_tensor(s, device=cuda)
        for yt in (torch.as_tensor(y), torch.as_tensor(y.astype(np.uint8)),
                   torch.as_tensor(y.astype(np.int64) * 3)):
            assert M.binary_auc(st, yt.to(cuda)) == want
        sb = st.bfloat16()
        assert M.binary_auc(sb, torch.as_tensor(y, device=cuda)) == R.column_auc(
            sb.float().cpu().numpy(), y)
    with pytest.raises(ValueError):
        M.binary_auc(st, torch.ones(n, dtype=torch.bool, device=cuda))


# ------------------------------------------------------------------------ eval_rows ----

def _eval_rows(dev, table_t, C, capacity, launches):
    """Run msha_eval_rows once per (src, y) in ``launches`` into fresh buffers; returns
    numpy (store, labels, nll, pred, conf, counters) of the rows written."""
    store = torch.full((capacity, C), 7.0, dtype=torch.float32, device=dev)
    lab = torch.full((capacity,), 99, dtype=torch.int64, device=dev)
    nll = torch.full((capacity,), 7.0, dtype=torch.float32, device=dev)
    pred = torch.full((capacity,), 99, dtype=torch.int64, device=dev)
    state = torch.zeros(C * C + 2, dtype=torch.int64, device=dev)
    n = 0
    for s, yy in launches:
        st = None if s is None else torch.as_tensor(s, device=dev)
        yt = torch.as_tensor(yy, device=dev)
        L.call("msha_eval_rows", table_t.shape[0], C, len(yy),
               1 if table_t.dtype == torch.bfloat16 else 0, L.ptr(table_t), table_t.stride(0),
               L.ptr(st), L.ptr(yt), n, L.ptr(store), L.ptr(lab), L.ptr(nll), L.ptr(pred),
               state.data_ptr(), state.data_ptr() + 8 * C * C, L.stream_handle(dev))
        n += len(yy)
    torch.cuda.synchronize()
    assert (store[n:] == 7.0).all() and (pred[n:] == 99).all()  # nothing past the cursor
    h = state.cpu().numpy()
    return (store[:n].cpu().numpy(), lab[:n].cpu().numpy(), nll[:n].cpu().numpy(),
            pred[:n].cpu().numpy(), h[:C * C].reshape(C, C), h[C * C:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 2, 31, 32, 33, 64, 1024])
def test_eval_rows_exact(cuda, C, dtype):
    rng = np.random.default_rng(C)
    N = 37
    # few distinct values: ties in the row maximum at every width
    vals = np.array([-3.0, -1.5, -0.75, -0.125, -4.0], np.float32)
    table = rng.choice(vals, (N, C))
    tt = torch.as_tensor(table, device=cuda).to(dtype)  # the values are exact in bf16
    rep = rng.integers(0, 5, 70).astype(np.int64)
    neg = rng.integers(-N, 0, 41).astype(np.int64)
    launches = [(None, rng.integers(0, C, N)), (rep, rng.integers(0, C, 70)),
                (neg, rng.integers(0, C, 41))]
    store, lab, nll, pred, conf, counters = _eval_rows(cuda, tt, C, N + 70 + 41 + 3, launches)
    idx = np.concatenate([np.arange(N), rep, neg + N])
    y = np.concatenate([yy for _, yy in launches]).astype(np.int64)
    rows = table[idx]
    np.testing.assert_array_equal(store, rows)
    np.testing.assert_array_equal(lab, y)
    np.testing.assert_array_equal(nll, -rows[np.arange(len(y)), y])
    np.testing.assert_array_equal(pred, R.argmax_lowest(rows))
    np.testing.assert_array_equal(conf, R.confusion(y, pred, C))  # second launch accumulates
    assert counters.tolist() == [0, 0]


def test_eval_rows_counts_nonfinite(cuda):
    rng = np.random.default_rng(0)
    table = rng.standard_normal((20, 33)).astype(np.float32)
    table[3, 32], table[3, 0], table[9, 17] = np.inf, -np.inf, np.nan
    src = np.array([3, 9, 3, 1, 0], np.int64)
    y = np.array([1, 2, 3, 4, 5], np.int64)
    store, _, _, pred, _, counters = _eval_rows(cuda, torch.as_tensor(table, device=cuda), 33, 5,
                                                [(src, y)])
    assert counters.tolist() == [5, 0]
    np.testing.assert_array_equal(store, table[src])
    np.testing.assert_array_equal(pred, np.argmax(table[src], axis=1))  # a NaN is the maximum


def test_eval_rows_bad_rows_are_bounded(cuda):
    """One out-of-range source index and one out-of-range label: counted, written as
    zeros / -1, never loaded through; every other row as in a run without them."""
    rng = np.random.default_rng(1)
    N, C = 50, 32
    table = rng.standard_normal((N, C)).astype(np.float32)
    tt = torch.as_tensor(table, device=cuda)
    src = rng.integers(-N, N, 90).astype(np.int64)
    y = rng.integers(0, C, 90).astype(np.int64)
    good = _eval_rows(cuda, tt, C, 90, [(src, y)])
    src2, y2 = src.copy(), y.copy()
    src2[17], y2[60] = N, C
    src3, y3 = src.copy(), y.copy()
    src3[17], y3[60] = -N - 1, -1
    keep = np.ones(90, bool)
    keep[[17, 60]] = False
    without = _eval_rows(cuda, tt, C, 88, [(src[keep], y[keep])])
    for s, yy in ((src2, y2), (src3, y3)):
        store, lab, nll, pred, conf, counters = _eval_rows(cuda, tt, C, 90, [(s, yy)])
        assert counters.tolist() == [0, 2]
        for got, ref in zip((store, lab, nll, pred), good):
            np.testing.assert_array_equal(got[keep], ref[keep])
        for got, ref in zip((store[keep], lab[keep], nll[keep], pred[keep], conf), without):
            np.testing.assert_array_equal(got, ref)
        assert (store[~keep] == 0).all() and (pred[~keep] == -1).all() and (nll[~keep] == 0).all()


# ------------------------------------------------------------------------ Evaluator ----

@pytest.fixture(scope="module")
def fx():
    z = golden("eval_metrics.npz")
    return {str(n): {k: z[f"{n}.{k}"] for k in ("table", "src", "y", "pred", "ref")}
            for n in z["names"]}


KEYS = ("accuracy", "precision_macro", "recall_macro", "precision_micro", "recall_micro")
CASES = ("c32", "three", "dup", "missing", "two", "pred_never_true", "true_never_pred")


@pytest.mark.parametrize("name", CASES)
def test_evaluator_matches_reference_outputs(cuda, fx, name):
    c = fx[name]
    table, src, y = c["table"], c["src"], c["y"]
    B, C, bs = len(y), table.shape[1], 64
    tt = torch.as_tensor(table, device=cuda)
    ev = M.Evaluator(C, B, cuda)
    with torch.no_grad():
        for i in range(0, B, bs):  # a short last batch
            ev.update(tt, torch.as_tensor(src[i:i + bs], device=cuda),
                      torch.as_tensor(y[i:i + bs], device=cuda))
    m = ev.compute()
    mb = ev.compute(batch_size=bs)
    assert abs(m["auc"] - c["ref"][0]) <= 1e-12
    assert m["auc"] == R.calculate_auc(table[src], y)  # the oracle's quotient, bitwise
    for k, want in zip(KEYS, c["ref"][1:]):
        assert m[k] == want, (k, m[k], want)
    assert m["f1_macro"] == 2 * (c["ref"][2] * c["ref"][3]) / (c["ref"][2] + c["ref"][3])
    assert m["f1_micro"] == 2 * (c["ref"][4] * c["ref"][5]) / (c["ref"][4] + c["ref"][5])
    assert m["n"] == B and m["n_nonfinite"] == 0
    np.testing.assert_array_equal(m["pred"].cpu().numpy(), c["pred"])
    np.testing.assert_array_equal(m["confusion"], R.confusion(y, c["pred"], C))
    tol = B * 2.0 ** -24  # an fp32 sum of B terms in a fixed order, relative
    for got, want in ((m["loss"], R.loss_all(table[src], y)),
                      (mb["loss"], R.loss_chunked(table[src], y, bs))):
        assert abs(got - want) <= tol * abs(want), (got, want)
    again = ev.compute()
    for k in KEYS + ("loss", "auc", "f1_macro", "f1_micro"):
        assert np.float64(again[k]).tobytes() == np.float64(m[k]).tobytes(), k
    assert np.float64(ev.compute(batch_size=bs)["loss"]).tobytes() == \
        np.float64(mb["loss"]).tobytes()


def test_evaluator_errors(cuda, fx):
    c = fx["dup"]
    tt = torch.as_tensor(c["table"], device=cuda)
    C = tt.shape[1]
    ev = M.Evaluator(C, 300, cuda)
    src, y = torch.as_tensor(c["src"], device=cuda), torch.as_tensor(c["y"], device=cuda)
    ev.update(tt, src, torch.full_like(y, 2))
    with pytest.raises(ValueError):  # one class present
        ev.compute()
    ev.update(tt, torch.full_like(src, tt.shape[0]), y)
    with pytest.raises(IndexError):
        ev.compute()
    with pytest.raises(ValueError):  # capacity
        ev.update(tt, src, y)
    ev.reset()
    bad = tt.clone()
    bad[int(c["src"][0]), 1] = float("nan")
    ev.update(bad, src, y)
    m = ev.compute()
    assert np.isnan(m["auc"]) and m["n_nonfinite"] == int((c["src"] == c["src"][0]).sum())
    assert m["accuracy"] == M.metrics_from_confusion(m["confusion"])["accuracy"]
    with pytest.raises(RuntimeError):
        M.Evaluator(C, 4, cuda).update(tt.cpu(), src, y)


# -------------------------------------------------------------------------- TrainPy ----

def test_trainpy_test_epoch_device_matches_host(cuda, tmp_path):
    pytest.importorskip("sklearn", reason="test_epoch(False) is the reference's sklearn path")
    rng = np.random.default_rng(2)
    n, m, bs = 200, 32, 64
    flows = np.stack([np.concatenate([np.arange(n), rng.integers(0, n, 1380)]),
                      np.concatenate([np.arange(n) % m, rng.integers(0, m, 1380)])], 1)
    trainpy.write_year(str(tmp_path), "2015", rng.integers(0, 12, n), rng.integers(0, 4, n),
                       rng.random(n), flows, m)
    with trainpy.namespace(str(tmp_path), cuda) as ns:
        tp = trainpy.TrainPy(ns, cuda, dropout=0.5, seed=0, batch_size=bs)
        assert tp.test_size == 158 and tp.test_size % bs != 0  # a short last batch
        tp.iteration(next(iter(tp.train_loader)))
        host = tp.test_epoch(False)
        dev = tp.test_epoch(True)
        assert tp.model.training
    assert set(host) == set(dev)
    assert abs(dev["auc"] - host["auc"]) <= 1e-12
    # two fp32 sums of at most bs non-negative terms in different orders, a division each
    assert abs(dev["loss"] - host["loss"]) <= 2 * (bs + 1) * 2.0 ** -24 * abs(host["loss"])
    for k in host:
        if k not in ("auc", "loss"):
            assert dev[k] == host[k], (k, dev[k], host[k])
