"""Writes tests/golden/eval_metrics.npz: seeded inputs and what the reference's three
evaluation functions (model.py:66-92, sklearn underneath) return for them.

    python tests/golden/make_golden_eval.py /path/to/the/reference/checkout

Needs the reference checkout and sklearn; the tests only read the .npz.  Per case ``c``:
``c.table`` (N, C) fp32 scores, ``c.src`` (B,) rows of it, ``c.y`` (B,) labels,
``c.pred`` (B,) the lowest index of each gathered row's maximum, and ``c.ref`` =
[auc, accuracy, precision_macro, recall_macro, precision_micro, recall_micro] in fp64,
computed as train.py:264-271 calls them.
"""
import os
import sys

import numpy as np


def log_softmax(x):
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    # 32 classes, random log-probabilities, every class present, sources repeat
    t = log_softmax(rng.standard_normal((400, 32)))
    src = rng.integers(0, 400, 500)
    y = np.concatenate([np.arange(32), rng.integers(0, 32, 468)])
    out["c32"] = (t, src, y)
    # scores drawn from 3 distinct values: heavy ties in every column and in the argmax
    t = rng.choice(np.array([-2.5, -1.0, -0.25], np.float32), (200, 8))
    out["three"] = (t, np.arange(200), np.concatenate([np.arange(8), rng.integers(0, 8, 192)]))
    # rows duplicated through a repeated source index
    t = log_softmax(rng.standard_normal((64, 5)))
    out["dup"] = (t, rng.integers(0, 20, 150), np.concatenate([np.arange(5),
                                                               rng.integers(0, 5, 145)]))
    # class 2 missing from the labels: column k is paired with the k-th PRESENT class
    t = log_softmax(rng.standard_normal((120, 6)))
    y = rng.choice(np.array([0, 1, 3, 4, 5]), 120)
    y[:5] = [0, 1, 3, 4, 5]
    out["missing"] = (t, np.arange(120), y)
    # exactly two present classes: one column, scores column 0 against the second class
    t = log_softmax(rng.standard_normal((90, 4)))
    y = rng.choice(np.array([1, 3]), 90)
    y[:2] = [1, 3]
    out["two"] = (t, np.arange(90), y)
    # class 4 predicted but never true
    t = log_softmax(rng.standard_normal((100, 5)))
    t[::7, 4] = 0.0
    y = rng.integers(0, 4, 100)
    y[:4] = np.arange(4)
    out["pred_never_true"] = (t, np.arange(100), y)
    # class 4 true but never predicted
    t = log_softmax(rng.standard_normal((100, 5)))
    t[:, 4] = -30.0
    y = rng.integers(0, 5, 100)
    y[:5] = np.arange(5)
    out["true_never_pred"] = (t, np.arange(100), y)
    return out


def main(reference):
    sys.path.insert(0, reference)
    import model as ref  # the reference's model.py

    z = {}
    names = []
    for name, (table, src, y) in cases().items():
        table = np.ascontiguousarray(table, np.float32)
        src, y = np.asarray(src, np.int64), np.asarray(y, np.int64)
        rows = table[src]
        pred = np.argmax(rows, axis=1).astype(np.int64)
        y_pred_test = np.array(rows.tolist())  # train.py:261,265
        auc = ref.calculate_auc(y_pred_test, y)
        acc = ref.calculate_accuracy(pred, y)
        pma, rma = ref.calculate_precision_recall(pred, y, "macro")
        pmi, rmi = ref.calculate_precision_recall(pred, y, "micro")
        z[f"{name}.table"], z[f"{name}.src"], z[f"{name}.y"], z[f"{name}.pred"] = table, src, y, pred
        z[f"{name}.ref"] = np.array([auc, acc, pma, rma, pmi, rmi], np.float64)
        names.append(name)
    z["names"] = np.array(names)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_metrics.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
