"""Device-side evaluation against the host path on the same box ("Measured"):

    python scripts/eval_ab.py [out.json]

- ``Evaluator.update`` at B = 64 (one test batch) and B = 23,389 (the 2015 test split at
  once), against the bulk host hand-off of the same rows (``output[source_index]``,
  its argmax and the labels to the host in three copies) and, at B = 64, against
  train.py:256-263 as written (a ``.cpu().item()`` per value).
- ``Evaluator.compute`` at 23,389 x 32, against ``metrics.py``'s sklearn functions on the
  host arrays (the numpy oracle of tests/eval_ref.py if sklearn is not installed).
- ``binary_auc`` at 4M pair scores, against a ``.cpu()`` copy plus ``roc_auc_score``.
- the sort inside ``msha_rank_auc`` alone (HIP events, no host read): achieved bytes/s
  against its algorithmic bytes, passes x (read + write) x n x key bytes.

Device times are HIP-event times per call; where the call ends in a host read the event
interval contains it.  Host times are wall clock (median of 3; one run above a second).
Prints one JSON object; writes it to ``out.json`` if given.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_SRC, C, N_TEST, BATCH, PAIRS = 39179, 32, 23389, 64, 4_000_000


def wall(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
        if ts[-1] > 1e6:
            break
    return float(np.median(ts))


def host_metrics():
    try:
        import sklearn  # noqa: F401
        from msha_gnn_amd import metrics as M

        return "sklearn", M.calculate_auc, M.calculate_accuracy, M.calculate_precision_recall
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import eval_ref as R

        def pr(pred, true, avg):
            m = R.prf(true, pred)
            return m[f"precision_{avg}"], m[f"recall_{avg}"]

        return ("numpy oracle", R.calculate_auc,
                lambda pred, true: R.prf(true, pred)["accuracy"], pr)


def main(out_path=None):
    import msha_loader

    msha_loader.load()
    from gemm_ab import timeit
    from msha_gnn_amd import metrics as M

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    output = torch.log_softmax(torch.randn(N_SRC, C, device=dev, generator=g), 1)
    src = torch.randint(0, N_SRC, (N_TEST,), device=dev, generator=g)
    y = torch.randint(0, C, (N_TEST,), device=dev, generator=g)
    which, h_auc, h_acc, h_pr = host_metrics()
    res = {"host_metrics": which, "shape": [N_TEST, C]}

    ev = M.Evaluator(C, N_TEST, dev)

    def update(b):
        ev.n = 0
        ev.update(output, src[:b], y[:b])

    def host_bulk(b):
        preds = output[src[:b]]
        return preds.max(1)[1].cpu(), preds.cpu(), y[:b].cpu()

    def host_literal(b):  # train.py:256-263
        y_preds, y_pred_test, y_true_test = [], [], []
        preds = output[src[:b]]
        pred_label = preds.max(1)[1].type_as(y)
        for tag in pred_label:
            y_preds.append(tag.cpu().item())
        for pred in preds:
            y_pred_test.append(pred.detach().cpu().numpy().tolist())
        for t in y[:b]:
            y_true_test.append(t.cpu().item())

    for b in (BATCH, N_TEST):
        res[f"update_B{b}_us"] = round(timeit(lambda: update(b)), 2)
        res[f"host_bulk_copy_B{b}_us"] = round(wall(lambda: host_bulk(b)), 1)
    res[f"host_train_py_loop_B{BATCH}_us"] = round(wall(lambda: host_literal(BATCH)), 1)

    ev.reset()
    ev.update(output, src, y)
    res["compute_us"] = round(timeit(lambda: ev.compute(batch_size=BATCH), reps=10), 1)
    res["compute_wall_us"] = round(wall(lambda: ev.compute(batch_size=BATCH)), 1)
    m = ev.compute(batch_size=BATCH)
    pred_h, rows_h, y_h = (t.numpy() for t in host_bulk(N_TEST))
    rows64 = np.array(rows_h.tolist())  # train.py:261,265

    def host_compute():
        h_auc(rows64, y_h), h_acc(pred_h, y_h), h_pr(pred_h, y_h, "macro"), h_pr(pred_h, y_h,
                                                                               "micro")

    res["host_compute_us"] = round(wall(host_compute), 1)
    res["auc_device_minus_host"] = m["auc"] - float(h_auc(rows64, y_h))
    res["accuracy_equal"] = bool(m["accuracy"] == h_acc(pred_h, y_h))

    scores = torch.sigmoid(torch.randn(PAIRS, device=dev, generator=g))
    lab = torch.rand(PAIRS, device=dev, generator=g) < 0.5
    res["binary_auc_4M_us"] = round(timeit(lambda: M.binary_auc(scores, lab), reps=10), 1)

    def host_binary():
        s, l = scores.cpu().numpy(), lab.cpu().numpy()
        if which == "sklearn":
            from sklearn.metrics import roc_auc_score

            return roc_auc_score(l, s)
        import eval_ref as R

        return R.column_auc(s, l)

    res["host_binary_auc_4M_us"] = round(wall(host_binary), 1)
    res["binary_auc_device_minus_host"] = M.binary_auc(scores, lab) - float(host_binary())

    # the rank statistic alone (sort + scan, no host read) and its algorithmic bytes
    lab64 = lab.to(torch.int64)
    for name, s, n, cols, ld, yy, cls, binary in (
            ("4M_x1", scores, PAIRS, 1, 1, lab64, None, True),
            ("23389_x32", ev.store, N_TEST, C, C, ev.labels, None, False)):
        ws = {}
        us = timeit(lambda: M._rank_auc(s, n, cols, ld, yy, cls, binary, ws), reps=20)
        sort_bytes = 4 * 2 * n * cols * 4
        res[f"rank_auc_{name}_us"] = round(us, 1)
        res[f"rank_auc_{name}_sort_bytes"] = sort_bytes
        res[f"rank_auc_{name}_GBps"] = round(sort_bytes / us / 1e3, 1)
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
