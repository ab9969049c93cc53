"""fp64 restatement of ``functional.link_mlp_loss`` (the 'mlp' link predictor with one used
Linear under LLP's nll + mse objective), padding and the valid-pair count included.

    x_p   = h[src_p] * h[dst_p]
    out_p = sigmoid(keep / (1 - p) * relu(W x_p + b))
    L_lab = -(1 / Pv) sum_p out_p[label_p]
    L_mse = (1 / (Pv N)) sum_p sum_j (out_pj - t_pj)^2      (0 without a teacher)
    loss  = w_label L_lab + w_mse L_mse

A pair is padding when src or dst lies outside [0, n) or its label outside [0, N); Pv counts
the others.  Everything here is numpy in float64; nothing is imported from the package.
"""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def valid(src, dst, label, n, N):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    label = dst if label is None else np.asarray(label, np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n) & (label >= 0) & (label < N)
    return ok, label


def forward(h, src, dst, W, b, label=None, teacher=None, w_label=1.0, w_mse=0.0, keep=None,
            p=0.0):
    """dict: ok, label, pv, x (P, F), z = relu'd and dropped pre-sigmoid (P, N), pre = W x + b,
    out (NaN rows for padding), l_lab, l_mse, loss, and Az = sum_f |W_jf x_pf| + |b_j|."""
    h, W, b = (np.asarray(a, np.float64) for a in (h, W, b))
    n, N = h.shape[0], W.shape[0]
    ok, lab = valid(src, dst, label, n, N)
    P = len(ok)
    s = np.where(ok, src, 0)
    d = np.where(ok, dst, 0)
    x = h[s] * h[d]
    pre = x @ W.T + b
    Az = np.abs(x) @ np.abs(W).T + np.abs(b)
    kf = np.ones((P, N)) if keep is None else np.asarray(keep, np.float64).reshape(P, N) / (1.0 - p)
    z = np.maximum(pre, 0.0) * kf
    out = sigmoid(z)
    out[~ok] = np.nan
    pv = int(ok.sum())
    l_lab = l_mse = 0.0
    if pv:
        l_lab = -out[ok, lab[ok]].sum() / pv
        if teacher is not None:
            t = np.asarray(teacher, np.float64)
            l_mse = ((out[ok] - t[ok]) ** 2).sum() / (pv * N)
    return dict(ok=ok, label=lab, pv=pv, x=x, pre=pre, z=z, kf=kf, out=out, l_lab=l_lab,
                l_mse=l_mse, loss=w_label * l_lab + w_mse * l_mse, Az=Az)


def upstream(out, ok, label, teacher, pv, w_label, w_mse, gloss):
    """g (P, N): d loss / d out times gloss; rows of padding pairs zero."""
    P, N = out.shape
    g = np.zeros((P, N))
    if pv == 0:
        return g
    rows = np.flatnonzero(ok)
    g[rows, label[rows]] += -gloss * w_label / pv
    if teacher is not None:
        t = np.asarray(teacher, np.float64)
        g[rows] += 2.0 * gloss * w_mse * (out[rows] - t[rows]) / (pv * N)
    return g


def dz_from(out, g, mask, p=0.0):
    """dz = g out (1 - out) / (1 - p) where ``mask`` (kept and ReLU-active), else 0."""
    o = np.where(np.isnan(out), 0.5, out)
    return np.where(mask, g * o * (1.0 - o) / (1.0 - p), 0.0)


def backward(h, src, dst, W, dz, ok):
    """(dH, dW, db, dx) of dz through z = W (h[src] * h[dst]) + b, with the absolute-term sums
    (A_dH, A_dW, A_db) and the endpoint count per table row; pairs outside ``ok`` add nothing."""
    h, W, dz = (np.asarray(a, np.float64) for a in (h, W, dz))
    n = h.shape[0]
    rows = np.flatnonzero(ok)
    s, d = np.asarray(src, np.int64)[rows], np.asarray(dst, np.int64)[rows]
    dzv = dz[rows]
    x = h[s] * h[d]
    dW, A_dW = dzv.T @ x, np.abs(dzv).T @ np.abs(x)
    db, A_db = dzv.sum(0), np.abs(dzv).sum(0)
    dxv = dzv @ W
    A_dx = np.abs(dzv) @ np.abs(W)
    dH, A_dH = np.zeros_like(h), np.zeros_like(h)
    np.add.at(dH, s, dxv * h[d])
    np.add.at(dH, d, dxv * h[s])
    np.add.at(A_dH, s, A_dx * np.abs(h[d]))
    np.add.at(A_dH, d, A_dx * np.abs(h[s]))
    deg = np.bincount(s, minlength=n) + np.bincount(d, minlength=n)
    dx = np.zeros((len(ok), h.shape[1]))
    dx[rows] = dxv
    return dict(dH=dH, dW=dW, db=db, dx=dx, A_dH=A_dH, A_dW=A_dW, A_db=A_db, deg=deg)
