"""Evaluation.  First the host-side helpers train.py reaches through ``from model import *``
(model.py:66-92): plain sklearn on host arrays, kept as the reference's path.  Below them
the device-side path (csrc/eval.hip): ``Evaluator``, ``binary_auc`` and the numpy pieces
they finish with (``metrics_from_confusion``, ``auc_columns``, ``auc_from_counts``)."""
import numpy as np


def calculate_auc(y_pred, y_true):
    """Macro one-vs-rest AUC over the classes present in y_true."""
    from sklearn.metrics import roc_auc_score
    from sklearn.preprocessing import label_binarize

    classes = np.unique(y_true)
    yb = label_binarize(y_true, classes=classes)
    return float(np.mean([roc_auc_score(yb[:, c], np.asarray(y_pred)[:, c])
                          for c in range(yb.shape[1])]))


def calculate_accuracy(predicted_labels, true_labels):
    from sklearn.metrics import accuracy_score

    return accuracy_score(true_labels, predicted_labels)


def calculate_precision_recall(predicted_labels, true_labels, model):
    from sklearn.metrics import precision_score, recall_score

    return (precision_score(true_labels, predicted_labels, average=model, zero_division=1),
            recall_score(true_labels, predicted_labels, average=model, zero_division=1))


# ---------------------------------------------------------------------------------------
# Device-side evaluation (csrc/eval.hip): the same numbers without the per-value
# .cpu().item() of train.py:256-263 and without sklearn.  The three functions above stay
# the reference's host path.

def metrics_from_confusion(conf):
    """Accuracy and macro / micro precision and recall of a confusion matrix
    (``conf[true, predicted]`` counts) with sklearn's rules, in numpy fp64: the labels are
    the union of the true and the predicted classes, and ``zero_division=1`` applies to
    precision (class never predicted) and to recall (class never true) alike."""
    conf = np.asarray(conf, dtype=np.int64)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError("confusion matrix must be square")
    n = int(conf.sum())
    if n == 0:
        raise ValueError("empty confusion matrix")
    true_sum, pred_sum, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    keep = (true_sum + pred_sum) > 0
    tp_k, true_k, pred_k = tp[keep], true_sum[keep], pred_sum[keep]

    def divide(num, den):
        out = np.ones(len(num), dtype=np.float64)
        nz = den != 0
        out[nz] = num[nz] / den[nz]
        return out

    micro = float(tp.sum() / n)
    return {"accuracy": float(tp.sum() / n),
            "precision_macro": float(np.mean(divide(tp_k, pred_k))),
            "recall_macro": float(np.mean(divide(tp_k, true_k))),
            "precision_micro": micro, "recall_micro": micro}


def auc_columns(present, n_columns):
    """model.py:66-77's pairing of score columns with classes: ``label_binarize`` over the
    classes PRESENT in the labels, column k of the scores against the k-th of them -- not
    against class k -- and, with exactly two present classes, one column: scores column 0
    against the second class.  Returns the class of each scored column.  Fewer than two
    present classes raises ValueError (one class: sklearn's roc_auc_score), and so do more
    present classes than score columns."""
    present = [int(c) for c in present]
    if len(present) < 2:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined "
                         "in that case.")
    if len(present) > n_columns:
        raise ValueError(f"{len(present)} classes present in the labels but the scores have "
                         f"{n_columns} columns")
    return present[1:] if len(present) == 2 else present


def auc_from_counts(counts):
    """Mean over columns of U2 / (2 P Nn) in fp64 from msha_rank_auc's (columns, 4) int64
    {P, Nn, U2, non-finite}; NaN if any scored column holds a non-finite score."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    if (counts[:, 3] != 0).any():
        return float("nan")
    if (counts[:, 0] == 0).any() or (counts[:, 1] == 0).any():
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined "
                         "in that case.")
    return float(np.mean([int(u2) / (2 * int(p) * int(nn)) for p, nn, u2, _ in counts]))


def _f1(p, r):
    return 2 * (p * r) / (p + r)  # train.py:270,272


def _rank_auc(store, n, columns, ld, labels, cls, binary, ws_cache):
    """msha_rank_auc on the current stream; returns the (columns, 4) int64 device tensor."""
    import torch

    from . import _lib as L

    out = torch.empty((columns, 4), dtype=torch.int64, device=store.device)
    need = L.load().msha_rank_auc_workspace_size(n, columns)
    ws = ws_cache.get("ws")
    if need and (ws is None or ws.numel() < need):
        ws = ws_cache["ws"] = torch.empty(need, dtype=torch.uint8, device=store.device)
    L.call("msha_rank_auc", n, columns, L.ptr(store), ld, L.ptr(labels), L.ptr(cls),
           1 if binary else 0, L.ptr(out), L.ptr(ws) if need else None, need,
           L.stream_handle(store.device))
    return out


class Evaluator:
    """train.py:239-282 on the device.  ``update`` is one launch per test batch, no sync;
    ``compute`` makes at most two small device-to-host reads.

        ev = Evaluator(Rcount, len(test_dataset), device)
        for source_index, recipient_index in test_loader:       # under torch.no_grad()
            output = model(inter_adj, city_adj, province_adj, source_index)
            ev.update(output, source_index, recipient_index)
        m = ev.compute(batch_size=args.batch_size)
    """

    def __init__(self, n_classes, capacity, device):
        import torch

        if not 1 <= int(n_classes) <= 1024:
            raise ValueError("n_classes must be in [1, 1024]")
        if int(capacity) < 1:
            raise ValueError("capacity must be positive")
        self.C, self.capacity, self.device = int(n_classes), int(capacity), torch.device(device)
        dev, C = self.device, self.C
        self.store = torch.empty((self.capacity, C), dtype=torch.float32, device=dev)
        self.labels = torch.empty(self.capacity, dtype=torch.int64, device=dev)
        self.nll = torch.empty(self.capacity, dtype=torch.float32, device=dev)
        self.pred = torch.empty(self.capacity, dtype=torch.int64, device=dev)
        # conf (C x C), counters {non-finite, bad}, and one word for the fp32 loss: one read
        self.state = torch.zeros(C * C + 3, dtype=torch.int64, device=dev)
        self.n = 0
        self._ws = {}

    def reset(self):
        self.state.zero_()
        self.n = 0

    def update(self, output, source_index, recipient_index):
        """Append ``output[source_index]`` (``source_index`` None: the rows of ``output``
        themselves) with labels ``recipient_index``: one msha_eval_rows launch."""
        import torch

        from . import _lib as L

        L.require_cuda(output, source_index, recipient_index)
        if output.dim() != 2 or output.shape[1] != self.C or output.stride(1) != 1:
            raise ValueError(f"output must be (N, {self.C}) with unit column stride")
        if output.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("output must be float32 or bfloat16")
        B = int(recipient_index.shape[0])
        for idx in (source_index, recipient_index):
            if idx is not None and (idx.dtype != torch.int64 or idx.dim() != 1
                                    or not idx.is_contiguous() or idx.shape[0] != B):
                raise ValueError("indices must be contiguous int64 vectors of one length")
        if source_index is None and B != output.shape[0]:
            raise ValueError("without source_index the labels must cover every row of output")
        if self.n + B > self.capacity:
            raise ValueError(f"Evaluator capacity {self.capacity} exceeded")
        if B == 0:
            return
        C, st = self.C, self.state.data_ptr()
        L.call("msha_eval_rows", output.shape[0], C, B,
               1 if output.dtype == torch.bfloat16 else 0, L.ptr(output), output.stride(0),
               L.ptr(source_index), L.ptr(recipient_index), self.n, L.ptr(self.store),
               L.ptr(self.labels), L.ptr(self.nll), L.ptr(self.pred), st, st + 8 * C * C,
               L.stream_handle(self.device))
        self.n += B

    def compute(self, batch_size=None):
        """The metrics train.py:264-282 prints, as a dict: ``loss`` (the mean of nll over
        all rows, or with ``batch_size`` the mean of the per-chunk means, which is what
        train.py:253-254,274 prints), ``auc``, ``accuracy``, macro / micro ``precision_*``,
        ``recall_*``, ``f1_*``, ``n``, ``n_nonfinite``, ``pred`` (device int64) and
        ``confusion`` (numpy int64).

        The AUC keeps model.py:66-77's pairing (see ``auc_columns``).  A non-finite score
        in a scored column makes ``auc`` NaN and is counted in ``n_nonfinite`` (all
        columns); sklearn raises ValueError there instead.  Rows whose source index or
        label was out of range raise IndexError."""
        import torch

        from . import _lib as L

        if self.n == 0:
            raise ValueError("no rows to evaluate")
        C, n = self.C, self.n
        chunk = n if batch_size is None else int(batch_size)
        if chunk < 1:
            raise ValueError("batch_size must be positive")
        L.call("msha_eval_loss", n, chunk, L.ptr(self.nll), self.state.data_ptr() + 8 * (C * C + 2),
               L.stream_handle(self.device))
        host = self.state.cpu()  # read 1: confusion matrix, counters, loss
        conf = host[:C * C].numpy().reshape(C, C).copy()
        n_nonfinite, bad = int(host[C * C]), int(host[C * C + 1])
        if bad:
            raise IndexError(f"{bad} row(s) had a source index or a label out of range")
        loss = float(host[C * C + 2:].view(torch.float32)[0])
        cols = auc_columns(np.flatnonzero(conf.sum(axis=1)), C)
        cls = torch.tensor(cols, dtype=torch.int32).to(self.device)
        counts = _rank_auc(self.store, n, len(cols), C, self.labels, cls, False, self._ws)
        auc = auc_from_counts(counts.cpu().numpy())  # read 2: the AUC integers
        m = metrics_from_confusion(conf)
        m.update(loss=loss, auc=auc, n=n, n_nonfinite=n_nonfinite, pred=self.pred[:n],
                 confusion=conf,
                 f1_macro=_f1(m["precision_macro"], m["recall_macro"]),
                 f1_micro=_f1(m["precision_micro"], m["recall_micro"]))
        return m


def binary_auc(scores, labels):
    """ROC AUC of pair scores on the device: ``scores`` (P,) float32 or bfloat16 (what
    ``score_pairs(..., 'inner')`` returns), ``labels`` bool, uint8 or int64 (non-zero:
    positive).  Ties count half, as sklearn's roc_auc_score.  NaN if a score is not
    finite; ValueError if one class is absent.  Scores of a ``ShardedTable`` stay on their
    rank: this is the local AUC."""
    import torch

    from . import _lib as L

    L.require_cuda(scores, labels)
    if scores.dim() != 1 or labels.shape != scores.shape:
        raise ValueError("scores and labels must be vectors of one length")
    if scores.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("scores must be float32 or bfloat16")
    if labels.dtype not in (torch.bool, torch.uint8, torch.int64):
        raise TypeError("labels must be bool, uint8 or int64")
    s = scores.to(torch.float32).contiguous()  # bf16 widens exactly
    y = labels.to(torch.int64).contiguous()
    counts = _rank_auc(s, s.shape[0], 1, 1, y, None, True, {})
    return auc_from_counts(counts.cpu().numpy())


def hits_at_k(pos, neg, k):
    """Hits@K of link scores, the OGB definition: the fraction of ``pos`` scores strictly
    greater than the K-th largest ``neg`` score; 1.0 with fewer than K negatives.  ``pos``
    and ``neg``: score vectors on the device, float32 or bfloat16 (widened exactly).  The
    K-th largest negative is selected on the device (``msha_topk_merge``, hierarchically
    for long vectors); only the final count comes to the host (one read).  NaN if a score
    is not finite; ValueError on an empty ``pos``."""
    import torch

    from . import _lib as L
    from . import functional as MF

    L.require_cuda(pos, neg)
    if pos.dim() != 1 or neg.dim() != 1:
        raise ValueError("pos and neg must be score vectors")
    for s in (pos, neg):
        if s.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("scores must be float32 or bfloat16")
    if pos.numel() == 0:
        raise ValueError("no positive scores")
    k = int(k)
    if not 1 <= k <= MF.TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {MF.TOPK_MAX_K}]")
    p = pos.detach().to(torch.float32)
    n = neg.detach().to(torch.float32).contiguous()
    bad = (~torch.isfinite(p)).any() | (~torch.isfinite(n)).any()
    if n.numel() < k:
        hits = torch.full((), p.numel(), dtype=torch.int64, device=p.device)
    else:
        kth = MF.topk_merge(n.view(1, -1), None, k)[0][0, k - 1]
        hits = (p > kth).sum()
    hits, bad = torch.stack([hits, bad.to(torch.int64)]).tolist()
    return float("nan") if bad else hits / p.numel()


RANK_TIES = {"optimistic": 0, "mean": 1, "pessimistic": 2}


def rank_metrics(greater, equal, ks=(1, 3, 10), ties="mean"):
    """MRR, mean rank and Hits@K of filtered link ranks from the counts of
    ``functional.rank_inner``: rank = 1 + greater + {0, equal / 2, equal} for ``ties`` =
    'optimistic', 'mean' or 'pessimistic'.  Rows with ``greater < 0`` (no rank) are left
    out.  One ``msha_rank_summary`` call and one readback: the hit counts and the rank sum
    are integers (2 * rank, so the mean-tie half is exact), the reciprocal-rank sum is fp64
    in a fixed order -- two calls give the same bits.  Returns ``{"mrr", "mean_rank",
    "hits@k" for k in ks, "n"}``; ValueError on zero valid rows."""
    import ctypes

    import torch

    from . import _lib as L

    L.require_cuda(greater, equal)
    if (greater.dim() != 1 or greater.shape != equal.shape or greater.dtype != torch.int64
            or equal.dtype != torch.int64):
        raise ValueError("greater and equal must be int64 vectors of one length")
    if ties not in RANK_TIES:
        raise ValueError(f"ties must be one of {sorted(RANK_TIES)}, got {ties!r}")
    ks = [int(k) for k in ks]
    if len(ks) > 8 or any(k < 1 for k in ks):
        raise ValueError("ks: at most 8 values of k >= 1")
    g, e = greater.contiguous(), equal.contiguous()
    out = rank_summary(g, e, ks, ties).tolist()
    hits, valid, sum2r = out[:len(ks)], out[len(ks)], out[len(ks) + 1]
    rr = ctypes.c_double.from_buffer(ctypes.c_int64(out[len(ks) + 2])).value
    if valid == 0:
        raise ValueError("no valid rows to rank")
    res = {"mrr": rr / valid, "mean_rank": sum2r / (2 * valid), "n": valid}
    for k, h in zip(ks, hits):
        res[f"hits@{k}"] = h / valid
    return res


def rank_summary(greater, equal, ks, ties="mean", out=None):
    """The device half of ``rank_metrics``: an int64 tensor of ``len(ks) + 3`` words -- the
    hit counts, the valid rows, the sum of 2 * rank and the bits of the fp64 sum of
    1 / rank.  No host sync: it can be captured into a HIP graph (``out`` reused)."""
    import ctypes

    import torch

    from . import _lib as L
    from . import functional as MF

    n, nk = greater.numel(), len(ks)
    dev = greater.device
    if out is None:
        out = torch.empty(nk + 3, dtype=torch.int64, device=dev)
    ws = MF._workspace(dev, L.fn("msha_rank_summary_workspace_size")(n))
    kbuf = (ctypes.c_int64 * max(nk, 1))(*ks)
    L.call("msha_rank_summary", n, greater.data_ptr() if n else None,
           equal.data_ptr() if n else None, RANK_TIES[ties], ctypes.addressof(kbuf), nk,
           out.data_ptr(), out.data_ptr() + 8 * (nk + 2), ws.data_ptr(), ws.numel(),
           L.stream_handle(dev))
    return out
