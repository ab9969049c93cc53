"""numpy fp64 oracle of the device-side evaluation (msha--gnn_amd/metrics.py, csrc/eval.hip).

The AUC of one column is the tie-aware rank statistic in integers,

    U2 = sum over groups g of equal score of pos_g * (2 * neg_below_g + neg_g)
    AUC = U2 / (2 * P * Nn)                              (one fp64 division)

from a stable argsort of the scores; it agrees with sklearn's ``roc_auc_score`` to 1.2e-16
for n from 2 to 23,389, heavily tied scores included.  ``calculate_auc`` keeps the two
quirks of model.py:66-77: column k is paired with the k-th class PRESENT in the labels, and
with exactly two present classes there is one column, scores column 0 against the second.
"""
import numpy as np


def rank_counts(scores, positive):
    """(P, Nn, U2) of one column as Python ints.  ``scores``: (n,) float (-0.0 == +0.0, as
    numpy compares them; denormals distinct); ``positive``: (n,) bool."""
    s = np.asarray(scores, dtype=np.float64)
    pos = np.asarray(positive, dtype=bool)
    order = np.argsort(s, kind="stable")
    s, pos = s[order], pos[order]
    start = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    pos_g = np.add.reduceat(pos.astype(np.int64), start)
    neg_g = np.add.reduceat((~pos).astype(np.int64), start)
    neg_below = np.cumsum(neg_g) - neg_g
    assert len(s) < 2 ** 30  # U2 <= n^2 / 2 stays inside int64
    u2 = int(np.dot(pos_g, 2 * neg_below + neg_g))
    return int(pos.sum()), int((~pos).sum()), u2


def auc_from(P, Nn, U2):
    if P == 0 or Nn == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined "
                         "in that case.")
    return U2 / (2 * P * Nn)


def column_auc(scores, positive):
    return auc_from(*rank_counts(scores, positive))


def auc_classes(y_true, n_columns):
    """The class each scored column is judged against (model.py:66-77)."""
    present = [int(c) for c in np.unique(y_true)]
    if len(present) < 2:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined "
                         "in that case.")
    if len(present) > n_columns:
        raise ValueError("more classes present than score columns")
    return present[1:] if len(present) == 2 else present


def calculate_auc(y_pred, y_true):
    y_pred, y_true = np.asarray(y_pred), np.asarray(y_true)
    cls = auc_classes(y_true, y_pred.shape[1])
    return float(np.mean([column_auc(y_pred[:, k], y_true == c) for k, c in enumerate(cls)]))


def confusion(y_true, y_pred, n_classes):
    y_true, y_pred = np.asarray(y_true, np.int64), np.asarray(y_pred, np.int64)
    if ((y_true < 0) | (y_true >= n_classes) | (y_pred < 0) | (y_pred >= n_classes)).any():
        raise IndexError("label out of range")
    conf = np.zeros((n_classes, n_classes), np.int64)
    np.add.at(conf, (y_true, y_pred), 1)
    return conf


def prf(y_true, y_pred):
    """accuracy, macro precision / recall, micro precision / recall with sklearn's rules:
    labels = union of true and predicted classes, zero_division=1 both ways."""
    y_true, y_pred = np.asarray(y_true, np.int64), np.asarray(y_pred, np.int64)
    labels = np.union1d(y_true, y_pred)
    tp = np.array([np.sum((y_true == c) & (y_pred == c)) for c in labels], np.int64)
    true = np.array([np.sum(y_true == c) for c in labels], np.int64)
    pred = np.array([np.sum(y_pred == c) for c in labels], np.int64)
    prec = np.where(pred > 0, tp / np.maximum(pred, 1), 1.0)
    rec = np.where(true > 0, tp / np.maximum(true, 1), 1.0)
    acc = float(np.sum(y_true == y_pred) / len(y_true))
    return {"accuracy": acc, "precision_macro": float(np.mean(prec)),
            "recall_macro": float(np.mean(rec)), "precision_micro": acc, "recall_micro": acc}


def argmax_lowest(rows):
    return np.argmax(np.asarray(rows), axis=1)  # numpy: the first maximum


def loss_all(logp_rows, y):
    nll = -np.asarray(logp_rows, np.float64)[np.arange(len(y)), y]
    return float(nll.mean())


def loss_chunked(logp_rows, y, batch_size):
    nll = -np.asarray(logp_rows, np.float64)[np.arange(len(y)), y]
    return float(np.mean([nll[i:i + batch_size].mean() for i in range(0, len(y), batch_size)]))
