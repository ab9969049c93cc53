"""Autograd functions over the HIP kernels (include/msha_gnn.h).

``edge_attention``       Ablation.py:266-274 (OursLayer3 inter attention: scores,
                         masked softmax, dropout, u = att @ h1 and, optionally,
                         v = att.T @ h2), forward AND backward on the GPU.
``gal``                  GAT.py:20-35 GraphAttentionLayer row scale (after x @ W).
``dropout_keep_mask``    the Philox mask the kernels draw (for tests / oracles).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import functools
import os
import struct

import torch

from . import _lib
from .graph import Graph

NEG_SLOPE = 0.2

# Optional live kernel timing: when a dict is installed here, the forward edge
# kernel launch is bracketed by HIP events on its own stream (bench.py).
KERNEL_EVENTS = None


def _timed(name):
    if KERNEL_EVENTS is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    KERNEL_EVENTS.setdefault(name, []).append(ev)
    ev[0].record()
    return ev


def _f32c(t):
    return t.to(torch.float32).contiguous() if t is not None else None


BF16 = torch.bfloat16


def _table_dtype(*ts):
    """Storage type of node tables: bf16 when any given table is bf16, else fp32."""
    return BF16 if any(t is not None and t.dtype == BF16 for t in ts) else torch.float32


def _code(dt) -> int:
    """MSHA_DTYPE_* of a torch dtype."""
    return 1 if dt == BF16 else 0


def _tc(t, dt):
    return t.to(dt).contiguous() if t is not None else None


def new_seed() -> int:
    """Per-call dropout seed drawn from torch's CPU generator (no device sync;
    reproducible under torch.manual_seed)."""
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


_RNG_COUNTERS: dict = {}  # device index -> installed counter tensor (kept alive)


def set_rng_counter(counter: torch.Tensor | None, device=None):
    """Install (or remove, None) a device int64 replay counter for every dropout draw
    the library launches on ``device`` (default: the counter's device, else the
    current one; msha_set_rng_counter keeps one slot per device): increment it inside
    a captured HIP graph (``counter.add_(1)``) and each replay draws fresh masks.
    Returns the counter previously installed for that device (None if none), so a
    caller can restore it."""
    if counter is not None:
        _lib.require_cuda(counter)
        if counter.dtype != torch.int64 or counter.numel() < 1:
            raise ValueError("rng counter: a CUDA int64 tensor")
        dev = counter.device.index if device is None else torch.device(device).index
    else:
        dev = torch.device(device).index if device is not None else None
    if dev is None:
        dev = torch.cuda.current_device()
    if counter is not None and counter.device.index != dev:
        raise ValueError(f"rng counter lives on cuda:{counter.device.index}, not cuda:{dev}")
    prev = _RNG_COUNTERS.pop(dev, None)
    if counter is not None:
        _RNG_COUNTERS[dev] = counter
    _lib.call("msha_set_rng_counter", dev, None if counter is None else counter.data_ptr())
    return prev


def rng_counter(device=None):
    """The replay counter installed for ``device`` (default: current), or None."""
    dev = torch.device(device).index if device is not None else None
    return _RNG_COUNTERS.get(torch.cuda.current_device() if dev is None else dev)


def feed_step(dst: torch.Tensor, src: torch.Tensor, counter: torch.Tensor | None = None):
    """``dst.copy_(src)`` plus ``counter += 1`` in one launch (msha_feed_step): the feed of a
    replayed step whose graph leaves its replay-counter increment to the feed
    (``step.GraphedStep.replay(feed=...)``).  Same-size contiguous tensors on one device."""
    _lib.require_cuda(dst)
    if (src.device != dst.device or src.dtype != dst.dtype or src.numel() != dst.numel()
            or not (src.is_contiguous() and dst.is_contiguous())):
        raise ValueError("feed_step: same-shape contiguous tensors of one dtype and device")
    if counter is not None and (counter.dtype != torch.int64 or counter.device != dst.device):
        raise ValueError("feed_step: the counter is an int64 tensor on the feed's device")
    _lib.call("msha_feed_step", dst.data_ptr(), src.data_ptr(), dst.numel() * dst.element_size(),
              None if counter is None else counter.data_ptr(), _lib.stream_handle(dst.device))


def _stream(t):
    return _lib.stream_handle(t.device)


# Host-side caches for the per-call work around each launch (the eager train.py step is
# host-bound: ~40 launches behind ~1 ms of Python per step).
_WS: dict = {}  # (device index, stream) -> uint8 scratch tensor


def _workspace(dev, nbytes: int):
    """A scratch buffer of at least ``nbytes`` for one call's launches, shared by every
    call on the same device and stream (the library's workspaces are transient within a
    call; stream order keeps consecutive users apart).

    Under HIP-graph capture every call gets a fresh buffer from the graph's private pool:
    a cached buffer recorded into a graph could later be replaced (and freed) by a larger
    eager request while replays still write to it, and capture streams are pooled handles
    whose keys can collide with an eager stream's."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    key = (dev.index, _lib.stream_handle(dev))
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        t = _WS[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    return t


def _memo(obj, key, make):
    """Per-object memo (a graph's capability answers and workspace sizes)."""
    d = obj.__dict__.setdefault("_msha_memo", {})
    v = d.get(key)
    if v is None:
        v = d[key] = make()
    return v


class _ProjTag:
    """What project_scores leaves on its output h (``h._msha_proj``) for a square graph's
    edge_attention backward: the projection's input and score vectors, so the column pass
    can add the weight gradient's X^T D' for its own columns
    (msha_edge_attention_bwd_fused_wgrad), and ``record``: what that pass left for
    _ProjectScores.backward (the slab workspace, the block count and the identity of the
    gradient tensors the slabs were computed from)."""

    __slots__ = ("X", "al", "ar", "record")

    def __init__(self, X, al, ar):
        self.X, self.al, self.ar, self.record = X, al, ar, None

    def take(self):
        """The record, once: it holds the slab workspace and the gradient tensors."""
        rec, self.record = self.record, None
        return rec


# how often the column pass carried the weight gradient / the reduce ran alone (tests)
WGRAD_FUSED_CALLS = {"cols": 0, "reduce": 0}


def _same(t, ident):
    """``t`` is the tensor (or a view of the whole of it) whose (data_ptr, _version) is ident."""
    return t is not None and (t.data_ptr(), t._version) == ident


class _EdgeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, el, er, hc, hs, graph: Graph, p: float, seed: int, slope: float, ar=None):
        n, H = el.shape
        # hc is (a view of the whole of) a projection's own output: its tag
        base = hc._base if hc._base is not None else hc
        tag = getattr(base, "_msha_proj", None)
        if tag is not None and not (base.dim() == 2 and base.is_contiguous()
                                    and hc.is_contiguous() and base.data_ptr() == hc.data_ptr()
                                    and base.numel() == hc.numel()
                                    and base.shape[0] == hc.shape[0]):
            tag = None
        ctx.proj_tag = tag
        m, H2, F = hc.shape
        assert H2 == H and m == graph.n_cols and n == graph.n_rows
        dt = _table_dtype(hc, hs)
        el, er = _f32c(el), _f32c(er)
        hc, hs = _tc(hc, dt), _tc(hs, dt)
        dev = el.device
        s = _stream(el)
        g = graph.desc
        ctx.graph, ctx.p, ctx.seed, ctx.slope = graph, p, seed, slope
        ctx.has_hs = hs is not None
        # (u-only with a_r keeps the row-score contract: er is then never read)
        if hs is not None or (ar is None and bip_ok(graph, H, F, dt)):
            # u and v: the bipartite kernels on the repo's adjacency shape (M <= 32
            # recipients; u-only too), else the general forward + the CSC aggregate
            it = _inter_fwd(graph, el, er, hc, hs, slope, p, seed,
                            keep_u_lo=any(ctx.needs_input_grad[:4]), timed=True)
            ctx.bip = it.bip
            ctx.rowterms = ctx.rs = ctx.er_exact = False
            empty = el.new_empty(0)
            ctx.save_for_backward(el, er, hc, hs if hs is not None else empty, it.lse,
                                  *(() if it.bip else
                                    (it.u, it.u_lo if it.u_lo is not None else empty, empty)))
            return it.u if it.v is None else (it.u, it.v)
        # the general kernels, u-only.  Scores from the gathered row
        # (msha_edge_attention_fwd_rs): er_j = hc_j . a_r is recomputed from the row the
        # kernel gathers anyway, in the forward and in the fused backward's column pass (the
        # same bits in both)
        rs = (ar is not None and ROW_SCORES and FUSED_BWD
              and _lib.load().msha_edge_attention_row_scores_preferred(g, H, F, _code(dt)))
        # er from project_scores in the kernels' order is exactly what the forward
        # recomputes: the backward then reads er per column (no recompute from a_r)
        ctx.er_exact = bool(rs and getattr(er, "_msha_row_order", False))
        ar = ar.detach().to(torch.float32).contiguous().view(H, F) if rs else None
        u = torch.empty(n, H, F, device=dev, dtype=dt)
        # bf16 tables under autograd: keep the rounding residual of u for the backward's
        # D = dU . u (include/msha_gnn.h, u_lo)
        u_lo = torch.empty_like(u) if dt == BF16 and any(ctx.needs_input_grad[:4]) else None
        lse = torch.empty(n, H, device=dev, dtype=torch.float32)
        # row terms for the fused backward on large graphs (include/msha_gnn.h
        # msha_edge_attention_fwd_ex): d_el without a per-edge de crossing CSC -> CSR
        uc = qc = None
        if (FUSED_BWD and ctx.needs_input_grad[0] and ROWTERMS
                and _lib.load().msha_edge_attention_rowterms_preferred(g, H, F, _code(dt))):
            uc = torch.empty(n, H, F, device=dev, dtype=torch.float32)
            qc = torch.empty(n, H, device=dev, dtype=torch.float32)
        with _events("edge_attention_fwd", True):
            if rs:
                _lib.call("msha_edge_attention_fwd_rs", g, H, F, _code(dt), el.data_ptr(),
                          ar.data_ptr(), hc.data_ptr(), slope, p, seed, 0, u.data_ptr(),
                          _lib.ptr(u_lo), lse.data_ptr(), _lib.ptr(uc), _lib.ptr(qc), s)
            else:
                _lib.call("msha_edge_attention_fwd_ex", g, H, F, _code(dt), el.data_ptr(),
                          er.data_ptr(), hc.data_ptr(), slope, p, seed, 0, u.data_ptr(),
                          _lib.ptr(u_lo), lse.data_ptr(), None, _lib.ptr(uc), _lib.ptr(qc), s)
        ctx.bip = False
        ctx.rowterms = uc is not None
        ctx.rs = bool(rs)
        ctx.save_for_backward(el, er, hc, el.new_empty(0), lse, u,
                              u_lo if u_lo is not None else el.new_empty(0),
                              ar if rs else el.new_empty(0),
                              *((uc, qc) if uc is not None else ()))
        return u

    @staticmethod
    def backward(ctx, dU, dV=None):
        el, er, hc, hs, lse, *rest = ctx.saved_tensors
        u, u_lo, ar, *rowterms = rest if rest else (None, el.new_empty(0), None)
        u_lo = u_lo if u_lo.numel() else None
        ar = ar if ctx.rs and not ctx.er_exact else None
        n, H = el.shape
        dt, dev = hc.dtype, el.device
        dU = torch.zeros(n, H, hc.shape[2], device=dev, dtype=dt) if dU is None else _tc(dU, dt)
        use_dv = ctx.has_hs and dV is not None
        dV = _tc(dV, dt) if use_dv else None
        if not ctx.bip and not use_dv and FUSED_BWD:
            d_el = torch.empty(n, H, device=dev, dtype=torch.float32)
            return _bwd_fused(ctx, el, er, hc, lse, u, u_lo, dU, d_el, hs, rowterms, ar)
        d_el, d_er, d_hc, d_hs = _inter_bwd(ctx.graph, ctx.bip, el, er, hc, lse, u, u_lo, dU, hs,
                                            dV, None, ctx.slope, ctx.p, ctx.seed, timed=True)
        if ctx.has_hs and d_hs is None:
            d_hs = torch.zeros_like(hs)
        return d_el, d_er, d_hc, (d_hs if ctx.has_hs else None), None, None, None, None, None


# bipartite small-M kernels (msha_bip_attention_fwd/_bwd) wherever the library covers
# the graph (M * heads * feat <= 4096: every shipped year, bip1m).  Module switch for A/B.
BIP = True


def bip_ok(graph, H, F, dtype) -> bool:
    """The bipartite kernels cover the graph: the library's shape rule (M <= 32,
    M * H <= 64, M * H * F <= 4096) and rows with distinct columns, at most 64 / H each
    (every graph from_dense builds; checked on the host for from_csr)."""
    return bool(BIP and graph.distinct_cols and graph.max_deg * H <= 64 and _memo(
        graph, ("bip", H, F, _code(dtype)),
        lambda: bool(_lib.fn("msha_bip_supported")(graph.desc, H, F, _code(dtype)))))


def _bip_ws(graph, H, F, dev):
    return _workspace(dev, _memo(graph, ("bip_ws", H, F), lambda: int(
        _lib.fn("msha_bip_workspace_size")(graph.desc, H, F))))


# the bipartite kernels' block-partial reduce rides in the Ours layer's prep / finish
# launches (msha_bip_defer_reduce; one graph node fewer each way); MSHA_BIP_DEFER=0: separate
# reduce launches (A/B)
BIP_DEFER_REDUCE = os.environ.get("MSHA_BIP_DEFER", "1") != "0"


@contextlib.contextmanager
def _deferred_reduce(on):
    """While open (``on``), the block-partial reduce of a bipartite forward / backward is
    handed to the next Ours-layer launch on the stream; leaving -- on an error too -- ends
    the hand-over and launches a reduce that nothing took."""
    if not on:
        yield
        return
    _lib.call("msha_bip_defer_reduce", 1)
    try:
        yield
    finally:
        _lib.call("msha_bip_defer_reduce", 0)


@contextlib.contextmanager
def _events(name, on):
    """KERNEL_EVENTS bracket of the launches inside (``on``: edge_attention's calls only)."""
    ev = _timed(name) if on else None
    yield
    if ev is not None:
        ev[1].record()


# what the inter forward leaves: u (N,H,F), lse (N,H), v (M,H,F) with hs, the post-dropout
# attention attd (E,H) where it was exported or the general kernels needed it, the bf16
# rounding residual u_lo of u (general kernels only)
_Inter = collections.namedtuple("_Inter", "bip u lse v attd u_lo")


def _inter_fwd(graph, el, er, hc, hs, slope, p, seed, *, export_attd=False, keep_u_lo=False,
               intra=None, timed=False):
    """Inter attention forward, u and (with hs) v: one bipartite pass where bip_ok says so,
    else msha_edge_attention_fwd + the CSC aggregate (needs hs).  ``intra(inter)``: the
    caller's own launch on the result (the Ours layers' intra attention); on the bipartite
    path it carries the v reduce (BIP_DEFER_REDUCE).  ``keep_u_lo``: a backward will follow."""
    n, H = el.shape
    m, _, F = hc.shape
    dt, dev, s, g = hc.dtype, el.device, _stream(el), graph.desc
    bip = bip_ok(graph, H, F, dt)
    assert bip or hs is not None
    u = torch.empty(n, H, F, device=dev, dtype=dt)
    lse = torch.empty(n, H, device=dev, dtype=torch.float32)
    v = torch.empty(m, H, F, device=dev, dtype=dt) if hs is not None else None
    attd = u_lo = None
    if export_attd or not bip:
        attd = torch.empty(max(graph.n_edges, 1), H, device=dev, dtype=torch.float32)
    with _deferred_reduce(bip and BIP_DEFER_REDUCE and intra is not None):
        if bip:
            ws = _bip_ws(graph, H, F, dev)
            with _events("bip_attention_fwd", timed):
                _lib.call("msha_bip_attention_fwd", g, H, F, _code(dt), el.data_ptr(),
                          er.data_ptr(), hc.data_ptr(), _lib.ptr(hs), slope, p, seed, 0,
                          u.data_ptr(), None, lse.data_ptr(), _lib.ptr(attd), _lib.ptr(v),
                          ws.data_ptr(), ws.numel(), s)
        else:
            # bf16 tables under autograd: keep the rounding residual of u for the backward's
            # D = dU . u (include/msha_gnn.h, u_lo)
            u_lo = torch.empty_like(u) if dt == BF16 and keep_u_lo else None
            with _events("edge_attention_fwd", timed):
                _lib.call("msha_edge_attention_fwd", g, H, F, _code(dt), el.data_ptr(),
                          er.data_ptr(), hc.data_ptr(), slope, p, seed, 0, u.data_ptr(),
                          _lib.ptr(u_lo), lse.data_ptr(), attd.data_ptr(), s)
            _csc_aggregate(graph, H, F, attd, None, hs, v, None, s)
        inter = _Inter(bip, u, lse, v, attd, u_lo)
        if intra is not None:
            intra(inter)
    return inter


def _inter_bwd(graph, bip, el, er, hc, lse, u, u_lo, dU, hs, dV, row_coef, slope, p, seed, *,
               intra=None, timed=False):
    """Backward of _inter_fwd -> d_el, d_er, d_hc, d_hs (with hs and dV, else None): one
    bipartite row pass (the column gradients through per-wave LDS slabs; u / u_lo unused),
    else the row pass into one (de, attd) record of 2H floats per edge -- the column pass
    reads it as one 64-B segment at C4, the CSC visits edges in random order -- and the CSC
    aggregate.  ``intra(d_hs)``: the caller's launch after the row pass (the Ours layers'
    stage 1); on the bipartite path it carries the d_hc / d_er reduce."""
    n, H = el.shape
    m, _, F = hc.shape
    dt, dev, s, g = hc.dtype, el.device, _stream(el), graph.desc
    d_el = torch.empty(n, H, device=dev, dtype=torch.float32)
    d_er = torch.empty(m, H, device=dev, dtype=torch.float32)
    d_hc = torch.empty(m, H, F, device=dev, dtype=dt)
    d_hs = torch.empty(n, H, F, device=dev, dtype=dt) if dV is not None else None
    hs = hs if dV is not None else None
    if bip:
        ws = _bip_ws(graph, H, F, dev)
        with _deferred_reduce(BIP_DEFER_REDUCE and intra is not None):
            with _events("bip_attention_bwd", timed):
                _lib.call("msha_bip_attention_bwd", g, H, F, _code(dt), el.data_ptr(),
                          er.data_ptr(), hc.data_ptr(), lse.data_ptr(), dU.data_ptr(),
                          _lib.ptr(hs), _lib.ptr(dV), _lib.ptr(row_coef), slope, p, seed, 0,
                          d_el.data_ptr(), d_er.data_ptr(), d_hc.data_ptr(), _lib.ptr(d_hs),
                          ws.data_ptr(), ws.numel(), s)
            if intra is not None:
                intra(d_hs)
        return d_el, d_er, d_hc, d_hs
    rec = torch.empty(max(graph.n_edges, 1), 2, H, device=dev, dtype=torch.float32)
    de, attd = rec[:, 0], rec[:, 1]
    with _events("edge_attention_bwd_rows", timed):
        _lib.call("msha_edge_attention_bwd_rows", g, H, F, _code(dt), el.data_ptr(),
                  er.data_ptr(), hc.data_ptr(), lse.data_ptr(), u.data_ptr(), _lib.ptr(u_lo),
                  dU.data_ptr(), _lib.ptr(hs), _lib.ptr(dV), _lib.ptr(row_coef), slope, p, seed,
                  0, d_el.data_ptr(), de.data_ptr(), attd.data_ptr(), 2 * H, _lib.ptr(d_hs), s)
    if intra is not None:
        intra(d_hs)
    with _events("csc_aggregate", timed):
        _csc_aggregate(graph, H, F, attd, de, dU, d_hc, d_er, s, ld=2 * H)
    return d_el, d_er, d_hc, d_hs


# u-only backward as one column pass (msha_edge_attention_bwd_fused) instead of
# bwd_rows + csc_aggregate; same bits.  Module switch for A/B measurements.
FUSED_BWD = True
# row terms (uc, qc) from the forward where the library prefers them (large graphs);
# module switch for A/B measurements
ROWTERMS = True
# scores from the gathered row when the caller passes a_r (msha_edge_attention_fwd_rs);
# module switch for A/B measurements
ROW_SCORES = True


def _bwd_fused(ctx, el, er, hc, lse, u, u_lo, dU, d_el, hs, rowterms=(), ar=None):
    graph = ctx.graph
    n, H = el.shape
    m, _, F = hc.shape
    dev = el.device
    s = _stream(el)
    g = graph.desc
    if not graph.has_csc:
        raise RuntimeError("graph has no CSC view (build it with_csc=True)")
    uc, qc = rowterms if rowterms else (None, None)
    de = None if uc is not None else torch.empty(max(graph.n_edges, 1), H, device=dev,
                                                 dtype=torch.float32)
    wsb = int(_lib.load().msha_edge_attention_bwd_fused_workspace_size(g, H, F))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d_hc = torch.empty(m, H, F, device=dev, dtype=hc.dtype)
    d_er = torch.empty(m, H, device=dev, dtype=torch.float32)
    tag = getattr(ctx, "proj_tag", None)
    if tag is not None:
        tag.record = None
    nb = 0
    if (tag is not None and uc is not None and ar is None and hc.dtype == torch.float32
            and not ctx.has_hs and tag.X.shape[0] == m == n and tag.X.stride(1) == 1):
        # square graph over the projection's own rows: the column pass carries the weight
        # gradient where the library covers the call (host-only query)
        nb = int(_lib.fn("msha_edge_attention_bwd_fused_wgrad_route")(
            g, H, F, _code(hc.dtype), tag.X.shape[1], tag.X.stride(0), 1, 1, tag.X.data_ptr(),
            tag.al.data_ptr(), tag.ar.data_ptr()))
    if nb > 0:
        cut = graph.col_ranges(nb)
        wgb = int(_lib.fn("msha_edge_attention_bwd_fused_wgrad_workspace_size")(nb))
        wg = torch.empty(wgb, dtype=torch.uint8, device=dev)
        ev = _timed("edge_attention_bwd_fused")
        _lib.call("msha_edge_attention_bwd_fused_wgrad", g, H, F, _code(hc.dtype), el.data_ptr(),
                  er.data_ptr(), hc.data_ptr(), lse.data_ptr(), u.data_ptr(), None, dU.data_ptr(),
                  ctx.slope, ctx.p, ctx.seed, 0, uc.data_ptr(), qc.data_ptr(), d_el.data_ptr(),
                  d_er.data_ptr(), d_hc.data_ptr(), None, ws.data_ptr(), wsb, tag.X.data_ptr(),
                  tag.X.stride(0), tag.X.shape[1], tag.al.data_ptr(), tag.ar.data_ptr(),
                  cut.data_ptr(), nb, wg.data_ptr(), wgb, s)
        if ev is not None:
            ev[1].record()
        WGRAD_FUSED_CALLS["cols"] += 1
        # the slabs hold X^T (d_hc + d_el (x) al + d_er (x) ar) of exactly these tensors
        tag.record = (wg, nb, tuple((t, (t.data_ptr(), t._version)) for t in (d_hc, d_el, d_er)))
        return d_el, d_er, d_hc, None, None, None, None, None, None
    ev = _timed("edge_attention_bwd_fused")
    _lib.call("msha_edge_attention_bwd_fused_rs" if ar is not None else
              "msha_edge_attention_bwd_fused_ex", g, H, F, _code(hc.dtype), el.data_ptr(),
              ar.data_ptr() if ar is not None else er.data_ptr(), hc.data_ptr(), lse.data_ptr(),
              u.data_ptr(), _lib.ptr(u_lo), dU.data_ptr(), ctx.slope, ctx.p, ctx.seed, 0,
              _lib.ptr(uc), _lib.ptr(qc), d_el.data_ptr(), d_er.data_ptr(), d_hc.data_ptr(),
              _lib.ptr(de), ws.data_ptr(), wsb, s)
    if ev is not None:
        ev[1].record()
    d_hs = torch.zeros_like(hs) if ctx.has_hs else None
    return d_el, d_er, d_hc, d_hs, None, None, None, None, None


def _csc_aggregate(graph: Graph, H, F, w, x, table, out, out_x, stream, ld=0):
    if not graph.has_csc:
        raise RuntimeError("graph has no CSC view (build it with_csc=True)")
    assert out.dtype == table.dtype
    g = graph.desc
    wsb = _lib.load().msha_csc_aggregate_workspace_size(g, H, F)
    ws = None
    if graph._plan["n_multi"] > 0:
        ws = torch.empty(int(wsb), dtype=torch.uint8, device=table.device)
    _lib.call("msha_csc_aggregate", g, H, F, _code(table.dtype), w.data_ptr(), _lib.ptr(x), ld,
              table.data_ptr(), out.data_ptr(), _lib.ptr(out_x), _lib.ptr(ws),
              0 if ws is None else ws.numel(), stream)


def edge_attention(graph: Graph, el, er, hc, hs=None, p: float = 0.0, training: bool = False,
                   slope: float = NEG_SLOPE, seed: int | None = None, ar=None):
    """Fused masked edge-softmax + aggregation.

    el (N,H), er (M,H), hc (M,H,F) [, hs (N,H,F)] ->  u (N,H,F)  [, v (M,H,F)]
    with att = softmax_row(lrelu(el_i + er_j)), u = drop(att) @ hc, v = drop(att).T @ hs.
    Tables (hc, hs, u, v and their gradients) are bf16 when hc or hs is bf16 (fp32
    arithmetic, config C3), else fp32; scores and statistics are always fp32.

    ``ar`` (H, F), optional: the score vector er was computed with, er = hc . ar per
    head (Ablation.py:266-267 scores the aggregated table itself).  Then the u-only
    kernels recompute er_j from the gathered rows instead of gathering er per edge
    (msha_edge_attention_fwd_rs / _bwd_fused_rs); the gradient w.r.t. er is returned
    as before and reaches ar / hc through er's producer.
    """
    _lib.require_cuda(el, er, hc, hs)
    F = hc.shape[-1]
    H = el.shape[1]
    if not _lib.load().msha_edge_attention_supported(H, F):
        raise NotImplementedError(f"edge_attention: (heads={H}, feat={F}) not compiled")
    p = float(p) if training else 0.0
    if seed is None:
        seed = new_seed() if p > 0 else 0
    if ar is not None and tuple(ar.shape) not in ((H, F), (H * F,), (H * F, 1)):
        raise ValueError(f"edge_attention: ar must hold heads x feat = {H} x {F} values")
    return _EdgeAttention.apply(el, er, hc, hs, graph, p, seed, slope, ar)


class _GAL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, a, graph: Graph, p: float, seed: int):
        ctx.h_dtype = h.dtype
        h = _f32c(h)
        ctx.a_shape = None if a is None else (a.shape, a.dtype, a.device)
        out = torch.empty_like(h)
        _lib.call("msha_gal_fwd", graph.desc, h.data_ptr(), p, seed, 0, out.data_ptr(),
                  _stream(h))
        ctx.graph, ctx.p, ctx.seed = graph, p, seed
        ctx.save_for_backward(h)
        return out

    @staticmethod
    def backward(ctx, dout):
        (h,) = ctx.saved_tensors
        dout = _f32c(dout)
        dh = torch.empty_like(h)
        _lib.call("msha_gal_bwd", ctx.graph.desc, h.data_ptr(), dout.data_ptr(), ctx.p, ctx.seed,
                  0, dh.data_ptr(), _stream(h))
        da = None
        if ctx.a_shape is not None:
            shape, dtype, dev = ctx.a_shape
            da = torch.zeros(shape, dtype=dtype, device=dev)
        return dh.to(ctx.h_dtype), da, None, None, None


def gal(graph: Graph, h, p: float = 0.0, training: bool = False, seed: int | None = None,
        zero_grad_of=None):
    """``elu(dropout(mask/deg) * h)`` -- GraphAttentionLayer after its projection.

    ``zero_grad_of``: the layer's score vector ``a``; it cannot change the output
    (the score is constant along a row), so it gets an exact zero gradient, which
    keeps optimizers (Adam weight decay) stepping it as in the reference."""
    _lib.require_cuda(h)
    if h.shape != (graph.n_rows, graph.n_cols):
        raise ValueError(f"GAL: h must be (N, M) = {(graph.n_rows, graph.n_cols)}, "
                         f"got {tuple(h.shape)} (the reference needs adj with out_features "
                         f"columns, GAT.py:22-30)")
    p = float(p) if training else 0.0
    if seed is None:
        seed = new_seed() if p > 0 else 0
    return _GAL.apply(h, zero_grad_of, graph, p, seed)


def dropout_keep_mask(n: int, p: float, seed: int, device, offset: int = 0,
                      flat4: bool = False, word: int | None = None) -> torch.Tensor:
    """The kernels' Philox keep mask of n elements (uint8); flat4: the four-words-per-call
    mask of the flat-table dropout (msha_segments, feature dropout); word: word `word` of
    the block keyed on each element (the Ours intra masks)."""
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    if word is not None:
        _lib.call("msha_dropout_keep_mask_word", seed, offset, n, p, word, keep.data_ptr(),
                  _lib.stream_handle(device))
        return keep
    _lib.call("msha_dropout_keep_mask4" if flat4 else "msha_dropout_keep_mask", seed, offset, n,
              p, keep.data_ptr(), _lib.stream_handle(device))
    return keep


# ------------------------------------------------------------------ projections ---
def _splits_for(rows: int, M: int = 128, N: int = 128) -> int:
    """split-K factor for reductions over `rows`: >= 64 rows per split, <= ~1024
    workgroups in all, and the fp32 slab (splits x M x N) within 16 MB."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    slab_cap = max(1, (16 << 20) // (4 * M * N))
    return max(1, min(rows // 64, slab_cap, max(1, 1024 // tiles)))


def gemm(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor | None = None,
         accumulate: bool = False, splits: int | None = None, out_dtype=None) -> torch.Tensor:
    """C = A @ B (or C += A @ B) on the MFMA GEMM; A and B may be strided views
    (transposes included).  Long reductions use deterministic split-K.  bf16 operands
    (either one) run the bf16 MFMA kernel; C is then out_dtype (default bf16)."""
    M, K = A.shape
    K2, N = B.shape
    assert K == K2
    if splits is None:
        splits = _splits_for(K, M, N) if K >= 4096 else 1
    if A.dtype == BF16 or B.dtype == BF16:
        assert not accumulate and out is None, "bf16 gemm: no accumulate / out"
        return _gemm_bf16(A, B, splits, out_dtype or BF16, -1, None)
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    assert out.stride(1) == 1
    if accumulate and splits == 1:
        splits = 2
    ws = None
    if splits > 1:
        wsb = _lib.load().msha_gemm_workspace_size(M, N, splits)
        ws = torch.empty(int(wsb), dtype=torch.uint8, device=A.device)
    _lib.call("msha_gemm_f32", M, N, K, A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(),
              B.stride(0), B.stride(1), out.data_ptr(), out.stride(0),
              1.0 if accumulate else 0.0, splits, _lib.ptr(ws), 0 if ws is None else ws.numel(),
              _stream(A))
    return out


def _gemm_bf16(A, B, splits, out_dtype, operand, outer):
    """msha_gemm_bf16: bf16 operands (strided views kept), C in out_dtype."""
    A, B = A.to(BF16), B.to(BF16)
    M, K = A.shape
    N = B.shape[1]
    out = torch.empty(M, N, device=A.device, dtype=out_dtype)
    ws = None
    if splits > 1:
        ws = torch.empty(int(_lib.load().msha_gemm_bf16_workspace_size(M, N, splits)),
                         dtype=torch.uint8, device=A.device)
    H = Fd = 0
    d1 = a1 = d2 = a2 = None
    if outer is not None:
        H, Fd, d1, a1, d2, a2 = outer
        a1, a2 = _f32c(a1), _f32c(a2)
    _lib.call("msha_gemm_bf16", M, N, K, A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(),
              B.stride(0), B.stride(1), out.data_ptr(), out.stride(0), _code(out_dtype), splits,
              _lib.ptr(ws), 0 if ws is None else ws.numel(), operand, H, Fd, _lib.ptr(d1),
              _lib.ptr(a1), _lib.ptr(d2), _lib.ptr(a2), _stream(A))
    return out


def gemm_head_outer(A: torch.Tensor, B: torch.Tensor, operand: int, outer,
                    out_dtype=None) -> torch.Tensor:
    """A @ B with operand 0 (A) or 1 (B) read as X + de (x) a [+ de2 (x) a2]
    (outer = (heads, feat, de, a, de2, a2)).  fp32: falls back to materialising the
    sum with msha_add_head_outer only when the operand layout cannot take the fused
    loads.  bf16 operands: the bf16 kernel (C in out_dtype, default bf16)."""
    H, Fd, d1, a1, d2, a2 = outer
    M, K = A.shape
    N = B.shape[1]
    splits = _splits_for(K, M, N) if K >= 4096 else 1
    if A.dtype == BF16 or B.dtype == BF16:
        return _gemm_bf16(A, B, splits, out_dtype or BF16, operand, outer)
    out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    ws = None
    if splits > 1:
        ws = torch.empty(int(_lib.load().msha_gemm_workspace_size(M, N, splits)),
                         dtype=torch.uint8, device=A.device)
    rc = _lib.load().msha_gemm_f32_head_outer(
        M, N, K, A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(), B.stride(0), B.stride(1),
        out.data_ptr(), out.stride(0), 0.0, splits, _lib.ptr(ws), 0 if ws is None else ws.numel(),
        operand, H, Fd, d1.data_ptr(), a1.data_ptr(), _lib.ptr(d2), _lib.ptr(a2), _stream(A))
    if rc == 0:
        return out
    if rc != _lib.MSHA_ERR_UNSUPPORTED:
        _lib.raise_for(rc, "msha_gemm_f32_head_outer")
    X = A if operand == 0 else B
    tot = torch.empty(X.shape, device=X.device, dtype=torch.float32)
    _lib.call("msha_add_head_outer", X.shape[0], H, Fd, _f32c(X).data_ptr(), d1.data_ptr(),
              a1.data_ptr(), _lib.ptr(d2), _lib.ptr(a2), tot.data_ptr(), _stream(X))
    return gemm(tot, B) if operand == 0 else gemm(A, tot)


class _MatMul(torch.autograd.Function):
    """C = A @ B with both products of the backward on the library GEMMs (split-K over
    long reductions, deterministic)."""

    @staticmethod
    def forward(ctx, A, B):
        ctx.save_for_backward(A, B)
        return _mm(A, B)

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        dA = _mm(dC, B.t()).to(A.dtype) if ctx.needs_input_grad[0] else None
        dB = _mm(A.t(), dC).to(B.dtype) if ctx.needs_input_grad[1] else None
        return dA, dB


def _mm(A, B):
    if A.dtype == BF16 or B.dtype == BF16:
        A, B = A.to(BF16), B.to(BF16)
        M, K = A.shape
        N = B.shape[1]
        # the bf16 kernel where it takes both operands as they lie (msha_gemm_bf16_loader:
        # the launch's own layout decision) and C (N % 8 == 0); any other shape or view --
        # a forward's N = 30 recipients, which is its backward's K -- runs fp32 operands
        # on the exact-fp32 kernel, the result rounded to bf16
        if N % 8 == 0 and _lib.fn("msha_gemm_bf16_loader")(
                M, N, K, A.data_ptr(), A.stride(0), A.stride(1), B.data_ptr(), B.stride(0),
                B.stride(1)) >= 0:
            return gemm(A, B)
        return gemm(A.float(), B.float()).to(BF16)
    return gemm(A.float(), B.float())


def matmul(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Differentiable A @ B on the library GEMMs (fp32, or bf16 when an operand is)."""
    _lib.require_cuda(A, B)
    return _MatMul.apply(A, B)


class _ProjectScores(torch.autograd.Function):
    """h = X @ W, el = h . al, er = h . ar (per head) in one MFMA launch.  fp32 X, W:
    the exact-fp32 MFMA kernel; a bf16 X or W: the bf16 kernel (h bf16, el/er fp32)."""

    @staticmethod
    def forward(ctx, X, W, al, ar, heads: int, feat: int):
        ctx.dtypes = (X.dtype, W.dtype, None if al is None else al.dtype,
                      None if ar is None else ar.dtype)
        dt = _table_dtype(X, W)
        X, W = _tc(X, dt), _tc(W, dt)
        al, ar = _f32c(al), _f32c(ar)
        M, K = X.shape
        dev = X.device
        h = torch.empty(M, heads * feat, device=dev, dtype=dt)
        el = torch.empty(M, heads, device=dev, dtype=torch.float32) if al is not None else None
        er = torch.empty(M, heads, device=dev, dtype=torch.float32) if ar is not None else None
        # a small table (the 32 recipients of R15): one single-workgroup launch each way
        ctx.small = dt == torch.float32 and _project_small(M, K, heads, feat)
        fn = ("msha_project_small" if ctx.small else
              "msha_project_scores_bf16" if dt == BF16 else "msha_project_scores")
        _lib.call(fn, M, K, heads, feat, X.data_ptr(), W.data_ptr(), _lib.ptr(al), _lib.ptr(ar),
                  h.data_ptr(), _lib.ptr(el), _lib.ptr(er), _stream(X))
        ctx.heads, ctx.feat = heads, feat
        ctx.save_for_backward(X, W, al, ar, h)
        ctx.proj_tag = None
        # only where the backward would use the slabs (W, al, ar all want gradients): a frozen
        # W would leave the column pass's extra work and its record unused
        if (dt == torch.float32 and al is not None and ar is not None and not ctx.small
                and all(ctx.needs_input_grad[1:4])):
            ctx.proj_tag = h._msha_proj = _ProjTag(X, al, ar)
        outs = [h]
        if el is not None:
            outs.append(el)
        if er is not None:
            outs.append(er)
        return tuple(outs) if len(outs) > 1 else h

    @staticmethod
    def backward(ctx, dh, *dscores):
        X, W, al, ar, h = ctx.saved_tensors
        H, Fd = ctx.heads, ctx.feat
        xdt, wdt, aldt, ardt = ctx.dtypes
        dt = h.dtype
        M = X.shape[0]
        dev = X.device
        s = _stream(X)
        it = iter(dscores)
        d_el = next(it) if al is not None else None
        d_er = next(it) if ar is not None else None
        tag = ctx.proj_tag
        rec, dh_in = (None, None) if tag is None else (tag.take(), dh)
        if ctx.small:
            d_el, d_er = _f32c(d_el), _f32c(d_er)
            dh = None if dh is None else _tc(dh, dt)
            dX = torch.empty_like(X) if ctx.needs_input_grad[0] else None
            dW = torch.empty_like(W) if ctx.needs_input_grad[1] else None
            dal = torch.empty(H, Fd, device=dev) if d_el is not None and ctx.needs_input_grad[2] \
                else None
            dar = torch.empty(H, Fd, device=dev) if d_er is not None and ctx.needs_input_grad[3] \
                else None
            _lib.call("msha_project_small_bwd", M, X.shape[1], H, Fd, X.data_ptr(), W.data_ptr(),
                      _lib.ptr(al), _lib.ptr(ar), h.data_ptr(), _lib.ptr(dh), _lib.ptr(d_el),
                      _lib.ptr(d_er), _lib.ptr(dX), _lib.ptr(dW), _lib.ptr(dal), _lib.ptr(dar), s)
            return (dX, dW, None if dal is None else dal.reshape(al.shape).to(aldt),
                    None if dar is None else dar.reshape(ar.shape).to(ardt), None, None)
        dh = torch.zeros_like(h) if dh is None else _tc(dh, dt)
        terms = [(d, a) for d, a in ((d_el, al), (d_er, ar)) if d is not None]
        dX = dW = dal = dar = None
        kw = {"out_dtype": None}
        if terms:
            # dh + d_el (x) al (+ d_er (x) ar) is folded into the GEMM operand loads
            (d1, a1) = terms[0]
            d2, a2 = terms[1] if len(terms) > 1 else (None, None)
            d1, d2 = _f32c(d1), _f32c(d2)
            outer = (H, Fd, d1, a1, d2, a2)
            if ctx.needs_input_grad[0]:
                kw["out_dtype"] = xdt if dt == BF16 else None
                dX = gemm_head_outer(dh, W.t(), 0, outer, **kw)
            if ctx.needs_input_grad[1]:
                kw["out_dtype"] = wdt if dt == BF16 else None
                if (rec is not None and ctx.needs_input_grad[2] and ctx.needs_input_grad[3]
                        and d_el is not None and d_er is not None
                        and all(_same(t, ident) for t, (_, ident) in
                                zip((dh_in, d_el, d_er), rec[2]))):
                    # the column pass left X^T D' of these very gradients as block slabs
                    # (msha_edge_attention_bwd_fused_wgrad): only the block-order sum is left
                    wg, nb, _ = rec
                    dW = torch.empty(X.shape[1], H * Fd, device=dev, dtype=torch.float32)
                    o1 = torch.empty(H, Fd, device=dev, dtype=torch.float32)
                    o2 = torch.empty(H, Fd, device=dev, dtype=torch.float32)
                    _lib.call("msha_wgrad_reduce", wg.data_ptr(), nb, dW.data_ptr(), dW.stride(0),
                              o1.data_ptr(), o2.data_ptr(), s)
                    WGRAD_FUSED_CALLS["reduce"] += 1
                    dal, dar = _score_grads(d_el, d_er, o1, o2, al, ar, aldt, ardt)
                    return dX, dW, dal, dar, None, None
                if dt == torch.float32 and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]):
                    # dW, dal, dar in one pass over the rows where the shape allows
                    fused = _wgrad_colsum(X, dh, outer, h, W)
                    if fused is not None:
                        dW, o1, o2 = fused
                        dal, dar = _score_grads(d_el, d_er, o1, o2, al, ar, aldt, ardt)
                        return dX, dW, dal, dar, None, None
                dW = gemm_head_outer(X.t(), dh, 1, outer, **kw)
        else:
            if ctx.needs_input_grad[0]:
                dX = gemm(dh, W.t(), out_dtype=xdt if dt == BF16 else None)
            if ctx.needs_input_grad[1]:
                dW = gemm(X.t(), dh, out_dtype=wdt if dt == BF16 else None)
        if terms and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]):
            # dal[h,f] = sum_m d_el[m,h] h[m,h,f] (and dar): one pass over h
            (d1, a1) = terms[0]
            d2 = terms[1][0] if len(terms) > 1 else None
            o1 = torch.empty(H, Fd, device=dev, dtype=torch.float32)
            o2 = torch.empty(H, Fd, device=dev, dtype=torch.float32) if d2 is not None else None
            ws = _workspace(dev, int(_lib.fn("msha_head_colsum_workspace_size")(M, H, Fd)))
            d1, d2 = _f32c(d1), _f32c(d2)  # held until the launch (see bn_lrelu)
            _lib.call("msha_head_colsum", M, H, Fd, _code(dt), d1.data_ptr(),
                      _lib.ptr(d2), h.data_ptr(), o1.data_ptr(), _lib.ptr(o2),
                      ws.data_ptr(), ws.numel(), s)
            dal, dar = _score_grads(d_el, d_er, o1, o2, al, ar, aldt, ardt)
        return dX, dW, dal, dar, None, None


def _score_grads(d_el, d_er, o1, o2, al, ar, aldt, ardt):
    """(dal, dar) from the column sums of the present score terms, in order."""
    outs = [o1] + ([o2] if o2 is not None else [])
    dal = dar = None
    k = 0
    if d_el is not None:
        dal = outs[k].reshape(al.shape).to(aldt)
        k += 1
    if d_er is not None:
        dar = outs[k].reshape(ar.shape).to(ardt)
    return dal, dar


def _wgrad_colsum(X, dh, outer, h, W=None):
    """dW = X^T (dh + d1 (x) a1 [+ d2 (x) a2]) and the column sums of d1 (x) h, d2 (x) h
    (msha_gemm_f32_head_outer_colsum: one pass over the rows), or None where the fused
    kernel does not cover the shape (the caller runs the two ops).  With W (h = X @ W, the
    projection's own output) the sums come as (d^T X) W from the rows the weight gradient
    already reads (msha_gemm_f32_head_outer_colsum_w: h is not read) where that kernel
    covers the shape."""
    H, Fd, d1, a1, d2, a2 = outer
    M, K = X.shape
    N = dh.shape[1]
    if M < 4096 or not (dh.is_contiguous() and h.is_contiguous() and h.shape == dh.shape):
        return None
    splits = _splits_for(M, K, N)
    dev = X.device
    dW = torch.empty(K, N, device=dev, dtype=torch.float32)
    # the GEMM's and the colsum's scratch as two aligned parts of the shared workspace
    wsb = (int(_lib.fn("msha_gemm_workspace_size")(K, N, splits)) + 255) // 256 * 256
    cwsb = int(_lib.fn("msha_head_outer_colsum_workspace_size")(N))
    buf = _workspace(dev, wsb + cwsb)
    o1 = torch.empty(H, Fd, device=dev, dtype=torch.float32)
    o2 = torch.empty(H, Fd, device=dev, dtype=torch.float32) if d2 is not None else None
    A = X.t()
    if W is not None and W.dtype == torch.float32 and W.shape == (K, N) and W.stride(1) == 1:
        rc = _lib.fn("msha_gemm_f32_head_outer_colsum_w")(
            K, N, M, A.data_ptr(), A.stride(0), A.stride(1), dh.data_ptr(), dh.stride(0),
            dh.stride(1), dW.data_ptr(), dW.stride(0), splits, buf.data_ptr(), wsb, H, Fd,
            d1.data_ptr(), a1.data_ptr(), _lib.ptr(d2), _lib.ptr(a2), W.data_ptr(), W.stride(0),
            o1.data_ptr(), _lib.ptr(o2), buf.data_ptr() + wsb, cwsb, _stream(X))
        if rc == 0:
            return dW, o1, o2
        if rc != _lib.MSHA_ERR_UNSUPPORTED:
            _lib.raise_for(rc, "msha_gemm_f32_head_outer_colsum_w")
    rc = _lib.fn("msha_gemm_f32_head_outer_colsum")(
        K, N, M, A.data_ptr(), A.stride(0), A.stride(1), dh.data_ptr(), dh.stride(0),
        dh.stride(1), dW.data_ptr(), dW.stride(0), splits, buf.data_ptr(), wsb, H, Fd,
        d1.data_ptr(), a1.data_ptr(), _lib.ptr(d2), _lib.ptr(a2), h.data_ptr(), o1.data_ptr(),
        _lib.ptr(o2), buf.data_ptr() + wsb, cwsb, _stream(X))
    if rc == _lib.MSHA_ERR_UNSUPPORTED:
        return None
    if rc != 0:
        _lib.raise_for(rc, "msha_gemm_f32_head_outer_colsum")
    return dW, o1, o2


@functools.lru_cache(maxsize=256)
def _project_small(M, K, heads, feat) -> bool:
    return bool(_lib.fn("msha_project_small_supported")(M, K, heads, feat))


@functools.lru_cache(maxsize=256)
def _row_order(M, K, heads, feat, code) -> bool:
    return bool(_lib.fn("msha_project_scores_row_order")(M, K, heads, feat, code))


def project_scores(X, W, al=None, ar=None, heads: int = 1, feat: int | None = None):
    """``h = X @ W`` on the MFMA GEMM, with optional fused per-head score halves
    ``el = h . al``, ``er = h . ar`` (al/ar: (heads, feat)).  Returns h or
    (h, el[, er])."""
    _lib.require_cuda(X, W)
    feat = W.shape[1] // heads if feat is None else feat
    if al is not None:
        al = al.reshape(heads, feat)
    if ar is not None:
        ar = ar.reshape(heads, feat)
    out = _ProjectScores.apply(X, W, al, ar, heads, feat)
    if ar is not None:
        # er computed from the stored h in the order the row-score edge kernels recompute
        # it (msha_project_scores_row_order): edge_attention(..., ar=) then reads this er
        # where it needs er_j per column instead of recomputing it (the same bits)
        M, K = X.shape
        out[-1]._msha_row_order = _row_order(M, K, heads, feat, _code(_table_dtype(X, W)))
    return out


# ----------------------------------------------------------------- GCN SpMM ---
class _SpMM(torch.autograd.Function):
    """out = A^T @ table (transpose) or A @ table, A = the graph with edge values
    ``vals``: msha_csc_aggregate over the CSC view or the CSR-as-CSC row view."""

    @staticmethod
    def forward(ctx, table, vals, graph: Graph, transpose: bool):
        ctx.graph, ctx.transpose = graph, transpose
        ctx.save_for_backward(vals)
        return _spmm(graph, vals, table, transpose)

    @staticmethod
    def backward(ctx, dout):
        (vals,) = ctx.saved_tensors
        return _spmm(ctx.graph, vals, dout, not ctx.transpose), None, None, None


def _spmm(graph: Graph, vals, table, transpose):
    view = graph if transpose else graph.row_view()
    dt = _table_dtype(table)
    table = _tc(table, dt)
    D = table.shape[1]
    if table.shape[0] != view.n_rows:
        raise ValueError(f"spmm: table has {table.shape[0]} rows, expected {view.n_rows}")
    out = torch.empty(view.n_cols, D, device=table.device, dtype=dt)
    _csc_aggregate(view, 1, D, _f32c(vals), None, table, out, None, _stream(table))
    return out


def spmm(graph: Graph, vals: torch.Tensor, table: torch.Tensor, transpose: bool = True):
    """GCN propagation (model.py:37): ``A^T @ table`` (transpose) or ``A @ table`` with
    A's values ``vals`` on the graph's CSR edges (Graph.values); deterministic, fp32 or
    bf16 tables; feature width in {8, 16, 32, 64, 128}."""
    _lib.require_cuda(table, vals)
    if not _lib.load().msha_edge_attention_supported(1, table.shape[1]):
        raise NotImplementedError(f"spmm: width {table.shape[1]} not compiled")
    return _SpMM.apply(table, vals, graph, transpose)


# ------------------------------------------ GraphSAGE baseline (SGAE.py:41-56) ---
SAGE_WIDTHS = (16, 32, 64)  # in, M = hidden and out of msha_sage_fwd (msha_sage_supported)


def _sage_fwd(tb, src, graph, vals, W1, b1, W2, b2):
    B, out = src.numel(), W2.shape[0]
    logp = torch.empty(B, out, dtype=torch.float32, device=tb.device)
    _lib.call("msha_sage_fwd", graph.desc, B, src.data_ptr(), tb.shape[1], out, tb.data_ptr(),
              tb.stride(0), vals.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
              b2.data_ptr(), logp.data_ptr(), _stream(tb))
    return logp


class _Sage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, W1, b1, W2, b2, src, graph, vals):
        tb = table.detach()
        if tb.stride(1) != 1:
            tb = tb.contiguous()
        W1, b1, W2, b2 = (t.detach().contiguous() for t in (W1, b1, W2, b2))
        logp = _sage_fwd(tb, src, graph, vals, W1, b1, W2, b2)
        ctx.graph = graph
        # the registered table itself: the (src, src) plan's list has min(n, 2B) entries
        ctx.leaf = _row_leaf(table, min(tb.shape[0], 2 * src.numel()))
        ctx.save_for_backward(tb, W1, b1, W2, b2, src, vals, logp)
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        tb, W1, b1, W2, b2, src, vals, logp = ctx.saved_tensors
        g = ctx.graph
        n, in_f = tb.shape
        B, out = logp.shape
        dev = tb.device
        need_t, need_w = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:5])
        dl = dlogp.detach().to(torch.float32).contiguous()
        dS = dW1 = db1 = dW2 = db2 = None
        if need_w:
            dW1, db1, dW2, db2 = (torch.empty_like(t) for t in (W1, b1, W2, b2))
        head = (g.desc, B, src.data_ptr(), in_f, out, tb.data_ptr(), tb.stride(0),
                vals.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                logp.data_ptr(), dl.data_ptr())
        wgrads = (_lib.ptr(dW1), _lib.ptr(db1), _lib.ptr(dW2), _lib.ptr(db2))
        if need_t and ctx.leaf is not None:
            # a fuse_row_grad table: the batch's rows and their gradient go to its optimizer
            # (the call itself lists the rows of its (src, src) plan); no (n, in) buffer
            ws = _workspace(dev, _lib.fn("msha_sage_rows_workspace_size")(B, n, in_f, g.n_cols,
                                                                         out))
            _stash_rows(ctx.leaf, min(n, 2 * B), lambda *rows_vals: _lib.call(
                "msha_sage_bwd_rows", *head, *wgrads, *rows_vals, ws.data_ptr(), ws.numel(),
                _stream(tb)))
        else:
            if need_t:
                dS = torch.empty(n, in_f, dtype=torch.float32, device=dev)
            ws = _workspace(dev, _lib.fn("msha_sage_workspace_size")(B, n, in_f, g.n_cols, out))
            _lib.call("msha_sage_bwd", *head, _lib.ptr(dS), *wgrads, ws.data_ptr(), ws.numel(),
                      _stream(tb))
        need = ctx.needs_input_grad
        return (dS, dW1 if need[1] else None, db1 if need[2] else None,
                dW2 if need[3] else None, db2 if need[4] else None, None, None, None)


def sage_forward(table, src, graph, vals, W1, b1, W2, b2, check=True):
    """The GraphSAGE baseline of SGAE.py:41-56 on the sparse rows of the adjacency:

        x = table[src];  z1 = relu(x W1^T + b1);  y = adj[src] * z1
        logp = log_softmax(relu(y W2^T + b2), dim=1)                     (B, out)

    with ``adj`` given as its ``Graph`` (``graph_of(adj)``) and the fp32 values of its CSR
    edges (``graph.values(adj)``).  ``y`` is zero off the edges of row ``src_b``, so both
    Linears run over that row's edges alone and no dense ``adj[src]`` is read.  Only entries
    with ``adj > 0`` are edges: negative adjacency values are not supported.  ``table``
    (n, in), ``W1`` (M, in), ``b1`` (M,), ``W2`` (out, M), ``b2`` (out,) float32 with in, M
    and out each in ``SAGE_WIDTHS``; ``graph`` over (n, M) (SGAE.py:54 multiplies elementwise:
    hidden == M); ``src`` int64 (B,), B >= 0.

    ``check`` (default) applies torch's ``table[src]`` rule first (``check_pair_indices``:
    IndexError outside [-n, n), negative indices wrapped; one stream sync).  With
    ``check=False`` the caller vouches for indices in [0, n) -- as inside a captured HIP
    graph, where nothing may be read back; the kernels still bound every index and give a
    stray entry a NaN row and no gradient.

    Gradients go to ``table``, ``W1``, ``b1``, ``W2`` and ``b2`` for any upstream gradient.
    The forward keeps only its output; the backward recomputes the entry.  No float atomics:
    the weight gradients are block partials added in a fixed order, the table gradient adds the
    entries of a row in batch order (exact zeros for rows outside the batch), so every
    result is bitwise reproducible.  Nothing is read back with ``check=False``.  When
    ``table`` is itself a leaf registered with ``optim.Adam.fuse_row_grad``, its gradient is
    formed on the batch's distinct sources only (``RowGrad``, the dense gradient's rows bit
    for bit; the backward call lists them) and handed to that optimizer; ``table.grad`` stays
    None."""
    for name, t in (("table", table), ("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2),
                    ("vals", vals)):
        if t.dtype != torch.float32:
            raise TypeError(f"sage_forward: {name} must be float32, got {t.dtype}")
    if not isinstance(graph, Graph):
        raise TypeError("sage_forward takes the adjacency's Graph and its edge values "
                        "(graph_of(adj), graph.values(adj))")
    if src.dtype != torch.int64 or src.dim() != 1:
        raise ValueError(f"sage_forward: src must be a 1-D int64 tensor, got {src.dtype} "
                         f"{tuple(src.shape)}")
    if table.dim() != 2 or W1.dim() != 2 or W2.dim() != 2:
        raise ValueError(f"sage_forward: table {tuple(table.shape)}, W1 {tuple(W1.shape)} and "
                         f"W2 {tuple(W2.shape)} must be 2-D")
    if graph.n_rows != table.shape[0]:
        raise ValueError(f"sage_forward: the graph has {graph.n_rows} rows, the table "
                         f"{table.shape[0]}")
    if not (W1.shape[0] == graph.n_cols == W2.shape[1]):
        raise ValueError(f"sage_forward: hidden = {W1.shape[0]} (W1), {W2.shape[1]} (W2) and "
                         f"the adjacency's {graph.n_cols} columns must be equal: SGAE.py:54 "
                         f"multiplies adj[source_index] and the hidden layer elementwise")
    in_f, M, out = table.shape[1], graph.n_cols, W2.shape[0]
    if not all(w in SAGE_WIDTHS for w in (in_f, M, out)):
        raise ValueError(f"sage_forward: widths in = {in_f}, hidden = {M}, out = {out} are not "
                         f"supported: each must be one of {SAGE_WIDTHS}")
    if W1.shape[1] != in_f or b1.shape != (M,) or b2.shape != (out,):
        raise ValueError(f"sage_forward: W1 {tuple(W1.shape)}, b1 {tuple(b1.shape)}, b2 "
                         f"{tuple(b2.shape)} do not fit in = {in_f}, hidden = {M}, out = {out}")
    if vals.shape != (graph.n_edges,) or vals.requires_grad:
        raise ValueError(f"sage_forward: vals must be the {graph.n_edges} edge values of the "
                         f"graph, without gradient (graph.values(adj))")
    if not graph.distinct_cols:
        raise ValueError("sage_forward: the graph's rows must have distinct columns")
    _lib.require_cuda(table, src, vals, W1, b1, W2, b2)
    src = src.contiguous()
    if check and src.numel():
        src, _ = check_pair_indices(src, src, table.shape[0])
    vals = vals.contiguous()
    if src.numel():  # (the backward lists the batch's rows itself: too late for the read)
        _replay_catch_up(table, None, lambda: pair_plan(src, src, table.shape[0]))
    if torch.is_grad_enabled() and any(t.requires_grad for t in (table, W1, b1, W2, b2)):
        return _Sage.apply(table, W1, b1, W2, b2, src, graph, vals)
    tb = table.detach()
    if tb.stride(1) != 1:
        tb = tb.contiguous()
    return _sage_fwd(tb, src, graph, vals, *(t.detach().contiguous() for t in (W1, b1, W2, b2)))


# --------------------------------------------------- BatchNorm + LeakyReLU ---
class _BnLRelu(torch.autograd.Function):
    """lrelu(batch_norm(x)) with training batch statistics (Ablation.py:273-274)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, slope, momentum):
        dt = _table_dtype(x)
        x = _tc(x, dt)
        R, C = x.shape
        dev = x.device
        w32, b32 = _f32c(weight), _f32c(bias)
        rm = rv = None
        if running_mean is not None:
            rm, rv = _f32c(running_mean), _f32c(running_var)
        mean = torch.empty(C, device=dev, dtype=torch.float32)
        invstd = torch.empty(C, device=dev, dtype=torch.float32)
        y = torch.empty_like(x)
        wsb = int(_lib.load().msha_bn_workspace_size(R, C))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.call("msha_bn_lrelu_fwd", R, C, _code(dt), x.data_ptr(), _lib.ptr(w32),
                  _lib.ptr(b32), eps, slope, 1, momentum, _lib.ptr(rm), _lib.ptr(rv),
                  mean.data_ptr(), invstd.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(),
                  _stream(x))
        if rm is not None and rm.data_ptr() != running_mean.data_ptr():
            running_mean.copy_(rm)  # non-fp32 / strided buffers: write the update back
            running_var.copy_(rv)
        ctx.slope = slope
        ctx.pdtypes = (None if weight is None else weight.dtype, None if bias is None else bias.dtype)
        ctx.save_for_backward(x, w32, b32, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32, b32, mean, invstd = ctx.saved_tensors
        R, C = x.shape
        dev = x.device
        dy = _tc(dy, x.dtype)
        dx = torch.empty_like(x)
        dw = torch.empty(C, device=dev, dtype=torch.float32) if w32 is not None else None
        db = torch.empty(C, device=dev, dtype=torch.float32) if b32 is not None else None
        wsb = int(_lib.load().msha_bn_workspace_size(R, C))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.call("msha_bn_lrelu_bwd", R, C, _code(x.dtype), x.data_ptr(), dy.data_ptr(),
                  _lib.ptr(w32), _lib.ptr(b32), mean.data_ptr(), invstd.data_ptr(), ctx.slope,
                  dx.data_ptr(), _lib.ptr(dw), _lib.ptr(db), ws.data_ptr(), ws.numel(),
                  _stream(x))
        wdt, bdt = ctx.pdtypes
        return (dx, None if dw is None else dw.to(wdt), None if db is None else db.to(bdt),
                None, None, None, None, None)


def bn_lrelu(x: torch.Tensor, bn: torch.nn.BatchNorm1d, slope: float,
             count: bool = True) -> torch.Tensor:
    """``lrelu(bn(x), slope)`` for a (rows, C) table on the fused kernels: batch
    statistics and the running-statistics update as torch.nn.BatchNorm1d in training
    mode (momentum set; num_batches_tracked advanced on the device -- by the caller
    when ``count`` is False, e.g. one foreach add for all heads), running
    statistics in eval mode."""
    _lib.require_cuda(x)
    if x.dim() != 2 or bn.momentum is None:
        # cumulative-average momentum needs the host-side batch count: torch's path
        return torch.nn.functional.leaky_relu(bn(x), slope)
    use_batch = bn.training or not bn.track_running_stats
    if not use_batch:
        if torch.is_grad_enabled() and (x.requires_grad or bn.weight.requires_grad):
            return torch.nn.functional.leaky_relu(bn(x), slope)  # eval with autograd
        dt = _table_dtype(x)
        xc = _tc(x, dt)
        R, C = xc.shape
        y = torch.empty_like(xc)
        # fp32 views/copies held in locals until the launch: a temporary freed after
        # data_ptr() can be handed to the next copy by the caching allocator (bf16 models:
        # weight and bias copies would share one block)
        rm, rv = _f32c(bn.running_mean), _f32c(bn.running_var)
        w32, b32 = _f32c(bn.weight), _f32c(bn.bias)
        _lib.call("msha_bn_lrelu_fwd", R, C, _code(dt), xc.data_ptr(), _lib.ptr(w32),
                  _lib.ptr(b32), bn.eps, slope, 0, 0.0, rm.data_ptr(), rv.data_ptr(),
                  None, None, y.data_ptr(), None, 0, _stream(xc))
        return y
    track = bn.training and bn.track_running_stats
    if track and count:
        bn.num_batches_tracked.add_(1)
    return _BnLRelu.apply(x, bn.weight, bn.bias, bn.running_mean if track else None,
                          bn.running_var if track else None, bn.eps, slope,
                          float(bn.momentum))


# ------------------------------------------------------------------ link scoring ---
ACT_BIAS, ACT_RELU, ACT_DROPOUT, ACT_SIGMOID = 1, 2, 4, 8


class _PairInner(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_i, x_j):
        x_i, x_j = _f32c(x_i), _f32c(x_j)
        B, Fd = x_i.shape
        out = torch.empty(B, device=x_i.device, dtype=torch.float32)
        _lib.call("msha_pair_inner_fwd", B, Fd, x_i.data_ptr(), Fd, None, x_j.data_ptr(), Fd,
                  None, out.data_ptr(), _stream(x_i))
        ctx.save_for_backward(x_i, x_j, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x_i, x_j, out = ctx.saved_tensors
        B, Fd = x_i.shape
        dxi, dxj = torch.empty_like(x_i), torch.empty_like(x_j)
        _lib.call("msha_pair_inner_bwd", B, Fd, x_i.data_ptr(), Fd, None, x_j.data_ptr(), Fd,
                  None, out.data_ptr(), _f32c(dout).data_ptr(), dxi.data_ptr(), dxj.data_ptr(),
                  _stream(x_i))
        return dxi, dxj


class _PairLayer(torch.autograd.Function):
    """y = [sigmoid](dropout(relu(x @ W^T + b))) with x = x_i * x_j (first layer,
    fused) or x = x_i (deeper layers, x_j None)."""

    @staticmethod
    def forward(ctx, x_i, x_j, W, b, p: float, seed: int, sigmoid: bool):
        x_i, x_j, W, b = _f32c(x_i), _f32c(x_j), _f32c(W), _f32c(b)
        B, K = x_i.shape
        N = W.shape[0]
        act = ACT_BIAS | ACT_RELU | (ACT_DROPOUT if p > 0 else 0) | (ACT_SIGMOID if sigmoid else 0)
        out = torch.empty(B, N, device=x_i.device, dtype=torch.float32)
        _lib.call("msha_pair_linear", B, K, N, x_i.data_ptr(), K, None, _lib.ptr(x_j), K, None,
                  B, B, W.data_ptr(), b.data_ptr(), act, p, seed, 0, out.data_ptr(),
                  _stream(x_i))
        ctx.p, ctx.sigmoid = p, sigmoid
        ctx.has_xj = x_j is not None
        ctx.save_for_backward(x_i, x_j if x_j is not None else x_i.new_empty(0), W, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x_i, x_j, W, out = ctx.saved_tensors
        B, K = x_i.shape
        N = W.shape[0]
        s = _stream(x_i)
        dz = torch.empty_like(out)
        _lib.call("msha_pair_mlp_dz", B * N, out.data_ptr(), _f32c(dout).data_ptr(), ctx.p,
                  1 if ctx.sigmoid else 0, dz.data_ptr(), s)
        if ctx.has_xj:
            x = torch.empty_like(x_i)
            _lib.call("msha_pair_hadamard", B, K, x_i.data_ptr(), K, None, x_j.data_ptr(), K, None,
                      None, x.data_ptr(), None, s)
        else:
            x = x_i
        dW = gemm(dz.t(), x)                      # (N, K) = dz^T x
        one = torch.ones(1, device=x_i.device, dtype=torch.float32)
        db = gemm(one.as_strided((1, B), (0, 0)), dz).view(N)  # column sums of dz
        dx = gemm(dz, W)                          # (B, K)
        if ctx.has_xj:
            dxi, dxj = torch.empty_like(x_i), torch.empty_like(x_j)
            _lib.call("msha_pair_hadamard", B, K, x_i.data_ptr(), K, None, x_j.data_ptr(), K, None,
                      dx.data_ptr(), dxi.data_ptr(), dxj.data_ptr(), s)
            return dxi, dxj, dW, db, None, None, None
        return dx, None, dW, db, None, None, None


class _PairHadamardSigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_i, x_j):
        x_i, x_j = _f32c(x_i), _f32c(x_j)
        B, Fd = x_i.shape
        y = torch.empty_like(x_i)
        _lib.call("msha_pair_hadamard_sigmoid", B, Fd, x_i.data_ptr(), Fd, None, x_j.data_ptr(),
                  Fd, None, None, None, y.data_ptr(), None, _stream(x_i))
        ctx.save_for_backward(x_i, x_j, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x_i, x_j, y = ctx.saved_tensors
        B, Fd = x_i.shape
        dxi, dxj = torch.empty_like(x_i), torch.empty_like(x_j)
        _lib.call("msha_pair_hadamard_sigmoid", B, Fd, x_i.data_ptr(), Fd, None, x_j.data_ptr(),
                  Fd, None, y.data_ptr(), _f32c(dy).data_ptr(), dxi.data_ptr(), dxj.data_ptr(),
                  _stream(x_i))
        return dxi, dxj


def pair_hadamard_sigmoid(x_i, x_j):
    """LinkPredictor with any predictor other than 'mlp' / 'inner' (LLP.py:104-115):
    ``sigmoid(x_i * x_j)``, (B, F)."""
    _lib.require_cuda(x_i, x_j)
    if x_i.shape != x_j.shape or x_i.dim() != 2:
        raise ValueError(f"pair_hadamard_sigmoid: x_i {tuple(x_i.shape)} vs x_j "
                         f"{tuple(x_j.shape)}")
    return _PairHadamardSigmoid.apply(x_i, x_j)


def pair_inner(x_i, x_j):
    """'inner' LinkPredictor head: sigmoid(sum(x_i * x_j, -1))  (LLP.py:112-115)."""
    _lib.require_cuda(x_i, x_j)
    return _PairInner.apply(x_i, x_j)


def pair_layer(x_i, x_j, W, b, p=0.0, training=False, sigmoid=False, seed=None):
    _lib.require_cuda(x_i, x_j, W, b)
    p = float(p) if training else 0.0
    if seed is None:
        seed = new_seed() if p > 0 else 0
    return _PairLayer.apply(x_i, x_j, W, b, p, seed, sigmoid)


class _LinearBias(torch.autograd.Function):
    """y = x @ W^T + b as one fused launch (msha_pair_linear, act = bias): the student
    MLP's last layer (LLP.py:78), whose dz is dout itself."""

    @staticmethod
    def forward(ctx, x, W, b):
        x, W, b = _f32c(x), _f32c(W), _f32c(b)
        B, K = x.shape
        N = W.shape[0]
        out = torch.empty(B, N, device=x.device, dtype=torch.float32)
        _lib.call("msha_pair_linear", B, K, N, x.data_ptr(), K, None, None, K, None, B, B,
                  W.data_ptr(), b.data_ptr(), ACT_BIAS, 0.0, 0, 0, out.data_ptr(), _stream(x))
        ctx.save_for_backward(x, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, W = ctx.saved_tensors
        B = x.shape[0]
        dz = _f32c(dout)
        dW = gemm(dz.t(), x)                      # (N, K) = dz^T x
        one = torch.ones(1, device=x.device, dtype=torch.float32)
        db = gemm(one.as_strided((1, B), (0, 0)), dz).view(-1)  # column sums of dz
        dx = gemm(dz, W) if ctx.needs_input_grad[0] else None
        return dx, dW, db


def linear_bias(x, W, b):
    """``F.linear(x, W, b)`` on (B, K) float32 rows as one fused MFMA launch, with the
    backward on the library's GEMM (``MLP``'s last layer)."""
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1] or b.shape != (W.shape[0],):
        raise ValueError(f"linear_bias: x {tuple(x.shape)}, W {tuple(W.shape)}, b "
                         f"{tuple(b.shape)}")
    _lib.require_cuda(x, W, b)
    return _LinearBias.apply(x, W, b)


def check_pair_indices(src, dst, rows: int, rows2: int | None = None):
    """torch's ``h[idx]`` index rule for a fused pair gather (LLP.py:233): an index
    outside [-rows, rows) raises IndexError; negative ones inside are wrapped to
    rows + idx.  One device pass (``msha_pair_index_check``) and one flag read (a
    stream sync).  Returns the (possibly wrapped) int64 index tensors."""
    rows2 = rows if rows2 is None else rows2
    src = src.to(torch.int64).contiguous()
    dst = dst.to(torch.int64).contiguous()
    if src.numel() != dst.numel():
        raise ValueError(f"pair indices differ in length: {src.numel()} vs {dst.numel()}")
    flags = torch.zeros(2, dtype=torch.int32, device=src.device)
    _lib.call("msha_pair_index_check", src.numel(), src.data_ptr(), int(rows), dst.data_ptr(),
              int(rows2), flags.data_ptr(), _stream(src))
    oob, neg = flags.tolist()
    if oob:
        for idx, n in ((src, rows), (dst, rows2)):
            bad = idx[(idx >= n) | (idx < -n)]
            if bad.numel():
                raise IndexError(f"index {int(bad[0])} is out of bounds for dimension 0 "
                                 f"with size {n}")
    if neg:
        src = torch.where(src < 0, src + rows, src)
        dst = torch.where(dst < 0, dst + rows2, dst)
    return src, dst


def score_pairs(h, src, dst, mode="inner", W=None, b=None, out=None, out_dtype=None,
                check=True):
    """Fused caller gather + predictor (LLP.py:233 + LLP.py:104-115), inference:
    ``predictor(h[src], h[dst])`` without materialising the gathered rows.
    'inner' -> (P,), 'mlp' (one used Linear W (hidden, F), b) -> (P, hidden).
    A bf16 ``h`` runs the bf16 kernels (bf16 MFMA for 'mlp'; fp32 scores, or bf16
    'mlp' scores with ``out_dtype=torch.bfloat16``, as a bf16 LinkPredictor returns).
    ``check`` (default) applies torch's ``h[idx]`` rule first (``check_pair_indices``:
    IndexError outside [-n, n), negative indices wrapped; one stream sync).  With
    ``check=False`` the caller vouches for indices in [0, n) (a pipelined scorer whose
    batch was checked once); the 'inner' kernel still bounds every row and scores a
    stray pair NaN, the fp32 'mlp' gather reads zeros for it."""
    _lib.require_cuda(h, src, dst)
    dt = _table_dtype(h)
    h = _tc(h, dt)
    bf = dt == BF16
    if check:
        src, dst = check_pair_indices(src, dst, h.shape[0])
    src = src.to(torch.int64).contiguous()
    dst = dst.to(torch.int64).contiguous()
    P, Fd = src.numel(), h.shape[1]
    s = _stream(h)
    if mode == "inner":
        out = torch.empty(P, device=h.device, dtype=torch.float32) if out is None else out
        _lib.call("msha_pair_inner_fwd_ex", P, Fd, _code(dt), h.data_ptr(),
                  h.stride(0), src.data_ptr(), h.shape[0], h.data_ptr(), h.stride(0),
                  dst.data_ptr(), h.shape[0], None, out.data_ptr(), s)
        return out
    W, b = _tc(W, dt), _f32c(b)
    N = W.shape[0]
    if bf and (out_dtype == BF16 or (out is not None and out.dtype == BF16)):
        out = torch.empty(P, N, device=h.device, dtype=BF16) if out is None else out
        _lib.call("msha_pair_linear_bf16_ex", P, Fd, N, h.data_ptr(), h.stride(0),
                  src.data_ptr(), h.data_ptr(), h.stride(0), dst.data_ptr(), W.data_ptr(),
                  b.data_ptr(), ACT_BIAS | ACT_RELU | ACT_SIGMOID, 0.0, 0, 0, 1,
                  out.data_ptr(), s)
        return out
    out = torch.empty(P, N, device=h.device, dtype=torch.float32) if out is None else out
    rows = (h.shape[0], h.shape[0]) if not bf else ()  # the fp32 entry takes the row counts
    _lib.call("msha_pair_linear_bf16" if bf else "msha_pair_linear", P, Fd, N, h.data_ptr(),
              h.stride(0), src.data_ptr(), h.data_ptr(), h.stride(0), dst.data_ptr(), *rows,
              W.data_ptr(), b.data_ptr(), ACT_BIAS | ACT_RELU | ACT_SIGMOID, 0.0, 0, 0,
              out.data_ptr(), s)
    return out


# ------------------------------------------------------- top-K link retrieval ---
TOPK_MAX_K = 128


def exclude_from_pairs(q_pos, cols, n_q: int):
    """The ``exclude`` argument of ``topk_inner`` from unsorted (query position, column)
    pair lists: ``(rowptr, col)`` int32, CSR over the ``n_q`` query positions, columns
    ascending within a row, duplicates dropped.  torch sorts on the lists' device (the
    number of distinct pairs is read back: one sync)."""
    q_pos = q_pos.to(torch.int64).reshape(-1)
    cols = cols.to(torch.int64).reshape(-1)
    if q_pos.numel() != cols.numel():
        raise ValueError(f"pair lists differ in length: {q_pos.numel()} vs {cols.numel()}")
    key = torch.unique((q_pos << 31) | cols)  # sorted: by position, then by column
    counts = torch.bincount(key >> 31, minlength=int(n_q))
    if counts.numel() != int(n_q):
        raise IndexError(f"a query position is outside [0, {int(n_q)})")
    rowptr = torch.zeros(int(n_q) + 1, dtype=torch.int64, device=key.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr.to(torch.int32), (key & 0x7FFFFFFF).to(torch.int32)


def _topk_k(k) -> int:
    k = int(k)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {TOPK_MAX_K}], got {k}")
    return k


def _inner_tables(name, q, table, others=(), k=None):
    """The table pair of ``topk_inner`` / ``rank_inner``: ``(q, table, Fd, code)`` after
    their shared checks (``k``: ``topk_inner``'s, checked at its place among them), detached
    and in a layout the kernels read -- unit stride along a row, 16-byte aligned rows --
    or else copied contiguous."""
    if q.dtype != table.dtype:
        raise TypeError(f"q and table must share a dtype, got {q.dtype} and {table.dtype}")
    if q.dtype not in (torch.float32, BF16):
        raise TypeError(f"{name} takes float32 or bfloat16 tables")
    if q.dim() != 2 or table.dim() != 2 or q.shape[1] != table.shape[1]:
        raise ValueError(f"q and table must be 2-D with one feature width, got "
                         f"{tuple(q.shape)} and {tuple(table.shape)}")
    Fd = q.shape[1]
    code = _code(q.dtype)
    shape = (Fd, code) if k is None else (Fd, _topk_k(k), code)
    _lib.require_cuda(q, table, *others)
    if not _lib.fn(f"msha_{name}_supported")(*shape):
        raise ValueError(f"{name}: feature width {Fd} must be a multiple of 16 in [16, 256]")
    esz = q.element_size()

    def aligned(t):
        return (t.stride(1) == 1 and (t.stride(0) * esz) % 16 == 0 and t.stride(0) >= Fd
                and t.data_ptr() % 16 == 0)

    q, table = q.detach(), table.detach()
    return (q if aligned(q) else q.contiguous(),
            table if aligned(table) else table.contiguous(), Fd, code)


def _inner_exclude(exclude, B):
    """``exclude`` of ``topk_inner`` / ``rank_inner`` as ``(rowptr, col)`` for the library,
    ``(None, None)`` without exclusions."""
    if exclude is None:
        return None, None
    rp, cp = exclude
    _lib.require_cuda(rp, cp)
    if rp.dtype != torch.int32 or cp.dtype != torch.int32 or rp.numel() != B + 1:
        raise ValueError("exclude must be (rowptr, col) int32 tensors with B + 1 row "
                         "pointers (exclude_from_pairs)")
    if cp.numel() == 0:  # a NULL column list would read as "no exclusion half given"
        return None, None
    return rp.contiguous(), cp.contiguous()


def topk_inner(q, table, k, rows=None, exclude=None, sigmoid=True, col_offset=0, splits=None,
               check=True):
    """For each query the ``k`` rows of ``table`` with the highest inner product, without
    the (B, n) score matrix: ``(values, indices)``, (B, k) float32 / int64, each row best
    first.  Query b is ``q[rows[b]]`` (``rows`` None: ``q[b]``); ``q`` may be ``table``.
    ``q`` and ``table`` share dtype (float32: exact-f32 MFMA; bfloat16: bf16 MFMA, fp32
    accumulation) and feature width (a multiple of 16 up to 256).

    Order: logit descending, then index ascending (unique; +inf first, NaN below -inf).
    ``values`` are the probabilities 1 / (1 + exp(-logit)), or the logits with
    ``sigmoid=False``; the ranking is by the logit either way.  ``indices`` are
    ``row + col_offset``; slots past the available candidates hold -inf (0.0 under
    ``sigmoid``) and -1.  ``exclude``: ``(rowptr, col)`` int32 tensors
    (``exclude_from_pairs``), candidates never returned for query position b.
    ``splits``: column splits (None: the library's default); the result does not depend
    on it.

    ``check`` (default) applies torch's ``q[rows]`` rule first (``check_pair_indices``:
    IndexError outside [-n, n), negatives wrapped; one stream sync).  With ``check=False``
    the caller vouches for ``rows`` in [0, n): no host sync happens (the call can be
    captured into a HIP graph), and the kernel still bounds every row -- a stray one comes
    back as filler.  Inference only: the outputs are detached."""
    q, table, Fd, code = _inner_tables("topk_inner", q, table, (rows,), k)
    k = int(k)
    dev = q.device
    if rows is not None:
        if check:
            rows, _ = check_pair_indices(rows, rows, q.shape[0])
        rows = rows.to(torch.int64).contiguous()
        B = rows.numel()
    else:
        B = q.shape[0]
    rp, cp = _inner_exclude(exclude, B)
    n = table.shape[0]
    splits = 0 if splits is None else int(splits)
    vals = torch.empty(B, k, dtype=torch.float32, device=dev)
    idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    need = _lib.fn("msha_topk_inner_workspace_size")(B, n, k, splits)
    ws = _workspace(dev, need)
    _lib.call("msha_topk_inner", B, Fd, code, q.data_ptr(), q.stride(0), _lib.ptr(rows),
              q.shape[0], table.data_ptr() if n else None, table.stride(0), n, int(col_offset),
              _lib.ptr(rp), _lib.ptr(cp), k, 1 if sigmoid else 0, splits, vals.data_ptr(),
              idx.data_ptr(), None, ws.data_ptr(), ws.numel(), _stream(q))
    return vals, idx


def topk_merge(vals, idx=None, k=1, sigmoid=False):
    """Top ``k`` of each row of candidate lists under ``topk_inner``'s order: ``vals``
    (rows, lists, len) or (rows, n) float32, ``idx`` int64 of the same shape (entries < 0
    are ignored) or None (the position in the row).  Returns (rows, k) values and indices,
    filler -inf (0.0 under ``sigmoid``) / -1.  ``sigmoid`` maps the selected values (lists
    of logits) to probabilities; the order is by the values given.  The cross-rank merge
    of ``sharding.topk_sharded`` and the selection behind ``metrics.hits_at_k``; rows of
    any length (cut into chunks and merged hierarchically)."""
    k = _topk_k(k)
    _lib.require_cuda(vals, idx)
    if vals.dim() not in (2, 3):
        raise ValueError("vals must be (rows, lists, len) or (rows, n)")
    if idx is not None and idx.shape != vals.shape:
        raise ValueError("idx must have the shape of vals")
    rows = vals.shape[0]
    lists, ln = (vals.shape[1], vals.shape[2]) if vals.dim() == 3 else (1, vals.shape[1])
    v = vals.detach().to(torch.float32).contiguous()
    i = idx.to(torch.int64).contiguous() if idx is not None else None
    dev = v.device
    out_v = torch.empty(rows, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(rows, k, dtype=torch.int64, device=dev)
    need = _lib.fn("msha_topk_merge_workspace_size")(rows, lists, ln, k)
    ws = _workspace(dev, need)
    _lib.call("msha_topk_merge", rows, lists, ln, k, v.data_ptr() if v.numel() else None,
              _lib.ptr(i) if i is not None and i.numel() else None, 1 if sigmoid else 0,
              out_v.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), _stream(v))
    return out_v, out_i


# ----------------------------------------------------- select over ragged segments ---
class Ragged:
    """Ragged lists on the device: list s is ``idx[ptr[s]:ptr[s + 1]]`` (int32 both).
    ``segment_ties`` also leaves the segment maxima in ``max_val`` and the list lengths in
    ``count``.  ``idx`` is sized for the worst case; only ``idx[:ptr[-1]]`` is meaningful."""

    __slots__ = ("ptr", "idx", "max_val", "count")

    def __init__(self, ptr, idx, max_val=None, count=None):
        self.ptr, self.idx, self.max_val, self.count = ptr, idx, max_val, count

    def __iter__(self):  # ptr, idx = ragged
        return iter((self.ptr, self.idx))

    def lists(self):
        """The lists as numpy arrays on the host (one copy of ptr and idx: a sync)."""
        ptr = self.ptr.cpu().numpy()
        idx = self.idx[: int(ptr[-1])].cpu().numpy()
        return [idx[ptr[s]:ptr[s + 1]] for s in range(len(ptr) - 1)]


def _segment_args(name, ptr, vals, ids, eid, col, chunk):
    """The shared arguments of ``segment_ties`` / ``segment_topk`` for the library."""
    for t, what in ((ptr, "ptr"), (ids, "ids"), (eid, "eid")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
            raise TypeError(f"{name}: {what} must be a contiguous 1-D int32 tensor")
    if ptr.numel() < 1:
        raise ValueError(f"{name}: ptr needs n_seg + 1 entries")
    if vals.dtype != torch.float32 or vals.dim() not in (1, 2):
        raise TypeError(f"{name}: vals must be float32, (n,) or (n, H) with col=")
    vals = vals.detach()
    if vals.dim() == 2:
        if col is None or not 0 <= int(col) < vals.shape[1]:
            raise ValueError(f"{name}: a 2-D vals needs col in [0, {vals.shape[1]})")
        if vals.shape[0] > 1 and (vals.stride(1) != 1 or vals.stride(0) < vals.shape[1]):
            vals = vals.contiguous()
        ld, off = (vals.stride(0) if vals.shape[0] > 1 else vals.shape[1]), int(col)
    else:
        if col is not None:
            raise ValueError(f"{name}: col goes with a 2-D vals")
        if vals.numel() > 1 and vals.stride(0) < 1:
            vals = vals.contiguous()
        ld, off = (vals.stride(0) if vals.numel() > 1 else 1), 0
    n_vals = vals.shape[0]
    n_slots = eid.numel() if eid is not None else (ids.numel() if ids is not None else n_vals)
    if ids is not None and ids.numel() != n_slots:
        raise ValueError(f"{name}: ids and eid must have one entry per slot")
    if eid is None and n_vals < n_slots:
        raise ValueError(f"{name}: vals needs one row per slot")
    chunk = 0 if chunk is None else int(chunk)
    if chunk != 0 and not 64 <= chunk <= 4096:
        raise ValueError(f"{name}: chunk must be in [64, 4096], got {chunk}")
    _lib.require_cuda(ptr, vals, ids, eid)
    return vals, n_vals, ld, off, n_slots, chunk


def segment_ties(ptr, vals, ids=None, eid=None, col=None, rtol: float = 0.0, chunk=None):
    """For each segment ``[ptr[s], ptr[s + 1])`` of slots the maximum and the slots that
    attain it (Explainer.py:25-30 over a CSR row or a CSC column, without the dense
    matrix): a ``Ragged`` whose list s holds the ids of the slots with
    ``value >= max - rtol * |max|`` in slot order (``rtol=0`` or a non-finite maximum:
    equal to the maximum under ``topk_inner``'s order: -0.0 == +0.0, all NaNs equal and
    below -inf), with ``max_val`` (-inf for an empty segment) and ``count``.

    A slot's value is ``vals[e]`` (``vals`` 1-D, any stride: a head of the attention
    export as ``attd[:, h]``) or ``vals[e, col]``, with ``e = eid[t]`` (``eid`` None: the
    slot itself); its id is ``ids[t]`` (None: the position in its segment).  ``ptr``,
    ``ids``, ``eid``: int32.  ``chunk``: slots per wave of a long segment (None: the
    library's choice); the result does not depend on it.  Inference only; no host sync (the lists are sized for
    the worst case), so the call can be captured into a HIP graph."""
    vals, n_vals, ld, off, n_slots, chunk = _segment_args("segment_ties", ptr, vals, ids, eid,
                                                          col, chunk)
    rtol = float(rtol)
    if not 0.0 <= rtol < 1.0:
        raise ValueError(f"segment_ties: rtol must be in [0, 1), got {rtol}")
    n_seg = ptr.numel() - 1
    dev = ptr.device
    max_val = torch.empty(n_seg, dtype=torch.float32, device=dev)
    count = torch.empty(n_seg, dtype=torch.int32, device=dev)
    tie_ptr = torch.zeros(n_seg + 1, dtype=torch.int32, device=dev)
    tie_idx = torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev)
    ws = _workspace(dev, _lib.fn("msha_segment_select_workspace_size")(n_seg, n_slots, 0, chunk))
    _lib.call("msha_segment_ties", n_seg, n_slots, ptr.data_ptr(),
              vals.data_ptr() if n_vals else None, n_vals, ld, off, _lib.ptr(eid), _lib.ptr(ids),
              rtol, chunk, max_val.data_ptr(), count.data_ptr(), tie_ptr.data_ptr(),
              tie_idx.data_ptr(), ws.data_ptr(), ws.numel(), _stream(ptr))
    return Ragged(tie_ptr, tie_idx, max_val, count)


def segment_topk(ptr, vals, k, ids=None, eid=None, col=None, chunk=None):
    """The ``k`` best slots of each segment under ``topk_inner``'s order (value
    descending, then id ascending; Explainer.py:31-34): ``(values, indices)``,
    (n_seg, k) float32 / int64, best first, -inf / -1 past a segment's length.
    1 <= k <= 128 (the 200 of the reference's commented-out variant is out of range).
    Arguments, ``chunk`` and capture as ``segment_ties``."""
    k = _topk_k(k)
    vals, n_vals, ld, off, n_slots, chunk = _segment_args("segment_topk", ptr, vals, ids, eid,
                                                          col, chunk)
    n_seg = ptr.numel() - 1
    dev = ptr.device
    out_v = torch.empty(n_seg, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(n_seg, k, dtype=torch.int64, device=dev)
    ws = _workspace(dev, _lib.fn("msha_segment_select_workspace_size")(n_seg, n_slots, k, chunk))
    _lib.call("msha_segment_topk", n_seg, n_slots, ptr.data_ptr(),
              vals.data_ptr() if n_vals else None, n_vals, ld, off, _lib.ptr(eid), _lib.ptr(ids),
              k, chunk, out_v.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
              _stream(ptr))
    return out_v, out_i


# ------------------------------------------------------------ filtered link ranks ---
def rank_inner(q, table, target, rows=None, exclude=None, col_offset=0, target_logit=None,
               splits=None, check=True):
    """The filtered rank counts of each query's target among the rows of ``table``, without
    the (B, n) score matrix: ``(greater, equal, logit)``, int64, int64 and float32, (B,)
    each.  Query b is ``q[rows[b]]`` (``rows`` None: ``q[b]``), its target the row
    ``target[b] - col_offset`` of ``table``; ``greater[b]`` / ``equal[b]`` count the other,
    non-excluded candidates whose logit is above / equal to the target's ``logit[b]`` --
    the logits and the order of ``topk_inner(..., sigmoid=False)``, bit for bit (NaN below
    -inf, -0.0 == +0.0), so rank = 1 + greater + {0, equal / 2, equal}
    (``metrics.rank_metrics``).  Dtypes, alignment, ``rows``, ``exclude`` and ``splits`` as
    ``topk_inner``; the result does not depend on ``splits``.

    ``target_logit`` (float32, (B,)): rank against these logits instead (a shard of a larger
    table: ``col_offset`` is the shard's first global row and the target's owner computed
    the logit); a target outside the shard is then allowed and every non-excluded row is
    counted.

    ``check`` (default) applies torch's index rule to ``rows`` and, without
    ``target_logit``, to ``target`` against the table's rows (IndexError outside [-n, n),
    negatives wrapped; one stream sync).  With ``check=False`` no host sync happens (the
    call can be captured into a HIP graph); a stray ``rows[b]`` or a target outside the
    table gives -1 / -1 (and a NaN logit) for that row only.  Inference only: the outputs
    are detached."""
    q, table, Fd, code = _inner_tables("rank_inner", q, table, (rows, target, target_logit))
    B = rows.numel() if rows is not None else q.shape[0]
    if target.dim() != 1 or target.numel() != B or target.dtype != torch.int64:
        raise ValueError(f"target must be an int64 vector with one entry per query ({B})")
    if target_logit is not None and (target_logit.dtype != torch.float32
                                     or target_logit.dim() != 1 or target_logit.numel() != B):
        raise ValueError(f"target_logit must be a float32 vector with one entry per query ({B})")
    dev = q.device
    n = table.shape[0]
    col_offset = int(col_offset)
    if check and B:
        if rows is not None:
            rows, _ = check_pair_indices(rows, rows, q.shape[0])
        if target_logit is None:
            local, _ = check_pair_indices(target - col_offset if col_offset else target,
                                          target, n, 1 << 62)
            target = local + col_offset if col_offset else local
    if rows is not None:
        rows = rows.to(torch.int64).contiguous()
    target = target.contiguous()
    if target_logit is not None:
        target_logit = target_logit.detach().contiguous()
    rp, cp = _inner_exclude(exclude, B)
    splits = 0 if splits is None else int(splits)
    greater = torch.empty(B, dtype=torch.int64, device=dev)
    equal = torch.empty(B, dtype=torch.int64, device=dev)
    logit = torch.empty(B, dtype=torch.float32, device=dev)
    need = _lib.fn("msha_rank_inner_workspace_size")(B, n, splits)
    ws = _workspace(dev, need)
    _lib.call("msha_rank_inner", B, Fd, code, q.data_ptr(), q.stride(0), _lib.ptr(rows),
              q.shape[0], table.data_ptr() if n else None, table.stride(0), n, col_offset,
              target.data_ptr(), _lib.ptr(target_logit), _lib.ptr(rp), _lib.ptr(cp), splits,
              greater.data_ptr(), equal.data_ptr(), logit.data_ptr(), None, ws.data_ptr(),
              ws.numel(), _stream(q))
    return greater, equal, logit


# ----------------------------------------------------- link-prediction training ---
def _pair_lists(src, dst, what):
    if src.dtype != torch.int64 or dst.dtype != torch.int64:
        raise TypeError(f"{what}: src and dst must be int64 index tensors")
    if src.dim() != 1 or dst.dim() != 1 or src.numel() != dst.numel():
        raise ValueError(f"{what}: src and dst must be 1-D and of one length, got "
                         f"{tuple(src.shape)} and {tuple(dst.shape)}")
    if 2 * src.numel() >= 2 ** 31:
        raise ValueError(f"{what}: 2 * P must be below 2^31, got P = {src.numel()}")


class PairPlan:
    """Incidence plan of a pair list over a table of ``n`` rows (``pair_plan``): ``rowptr``
    int32 (n + 1) and ``ent`` int32 (2P), row r's endpoint ids in ascending order
    (e < P: the src end of pair e, e >= P: the dst end of pair e - P; padding pairs in no
    row, ``ent`` past ``rowptr[n]`` is -1), plus the backward's chunk table.  Valid for as
    long as the pair list is unchanged."""

    def __init__(self, n, n_pairs, rowptr, ent, chunk_tab):
        self.n, self.n_pairs = int(n), int(n_pairs)
        self.rowptr, self.ent, self.chunk_tab = rowptr, ent, chunk_tab


def pair_plan(src, dst, n: int) -> PairPlan:
    """The ``PairPlan`` of the pairs (src[p], dst[p]) over ``n`` table rows
    (``msha_pair_plan``): a stable device radix sort of the 2P endpoints by row.  A pure
    function of its arguments; nothing is read back, so the call can be captured."""
    _pair_lists(src, dst, "pair_plan")
    n = int(n)
    if not 1 <= n < 2 ** 31 - 1:
        raise ValueError(f"pair_plan: n must be in [1, 2^31 - 1), got {n}")
    _lib.require_cuda(src, dst)
    if src.device != dst.device:
        raise ValueError("pair_plan: src and dst must be on one device")
    src, dst = src.contiguous(), dst.contiguous()
    P, dev = src.numel(), src.device
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ent = torch.empty(2 * P, dtype=torch.int32, device=dev)
    slots = _lib.fn("msha_pair_plan_chunk_slots")(P)
    tab = torch.empty(2 * slots, dtype=torch.int32, device=dev)
    ws = _workspace(dev, _lib.fn("msha_pair_plan_workspace_size")(P))
    _lib.call("msha_pair_plan", P, n, src.data_ptr() if P else None,
              dst.data_ptr() if P else None, rowptr.data_ptr(), ent.data_ptr() if P else None,
              tab.data_ptr(), ws.data_ptr(), ws.numel(), _stream(src))
    return PairPlan(n, P, rowptr, ent, tab)


def plan_rows(plan: PairPlan):
    """The touched-row list of ``plan`` (``msha_plan_rows``): ``(rows, n_rows)`` with ``rows``
    int32 of capacity ``min(n, 2P)``, the ascending ids of the table rows that have an
    endpoint, -1 past the count, and ``n_rows`` a device int32 scalar.  Padding pairs touch
    no row.  A pure function of the plan: integer work, nothing read back (capturable); it is
    kept on the plan and lives as long as the plan does."""
    if not isinstance(plan, PairPlan) or plan.rowptr is None:
        raise ValueError("plan_rows: plan must be a PairPlan (pair_plan / context_plan)")
    got = getattr(plan, "_rows", None)
    if got is not None:
        return got
    _lib.require_cuda(plan.rowptr)
    n, P, dev = plan.n, plan.n_pairs, plan.rowptr.device
    rows = torch.empty(min(n, 2 * P), dtype=torch.int32, device=dev)
    n_rows = torch.empty((), dtype=torch.int32, device=dev)
    ws = _workspace(dev, _lib.fn("msha_plan_rows_workspace_size")(n))
    _lib.call("msha_plan_rows", n, P, plan.rowptr.data_ptr(),
              rows.data_ptr() if rows.numel() else None, n_rows.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream(plan.rowptr))
    plan._rows = (rows, n_rows)
    return plan._rows


class RowGrad:
    """The gradient of an (n, F) table on the rows a batch touches: ``values[i]`` (fp32) is
    the gradient of row ``rows[i]`` for ``i < n_rows`` (``plan_rows``: ``rows`` ascending,
    -1 past the count, ``n_rows`` a device scalar) and zero past it; every other row's
    gradient is zero.  ``shape`` is the table's.  ``optim.Adam`` steps a table registered
    with ``fuse_row_grad`` from it."""

    def __init__(self, rows, n_rows, values, shape):
        self.rows, self.n_rows, self.values, self.shape = rows, n_rows, values, tuple(shape)

    def to_dense(self):
        """The (n, F) fp32 gradient (debugging): a scatter into zeros, nothing read back."""
        n, Fd = self.shape
        out = torch.zeros(n + 1, Fd, dtype=self.values.dtype, device=self.values.device)
        idx = self.rows.to(torch.int64)
        out[torch.where(idx >= 0, idx, torch.full_like(idx, n))] = self.values  # -1: row n
        return out[:n]


def _row_leaf(h, plan):
    """``h`` itself when it is a leaf table registered with ``optim.Adam.fuse_row_grad`` that
    needs a gradient (its backward then forms a ``RowGrad``), else None.  ``plan``: the
    PairPlan whose touched rows the gradient has, or the capacity of a row list that the
    backward's own launches build (``_stash_rows``); None or 0: no row path."""
    if not plan or not (h.requires_grad and h.is_leaf and h.is_contiguous()):
        return None
    from .optim import row_optimizer_of

    return h if row_optimizer_of(h) is not None else None


def _stash_rows(leaf, plan, launch):
    """Backward of a registered leaf: ``launch(rows, n_rows, cap, vals)`` fills the compact
    gradient, which goes to the leaf's optimizer in place of ``.grad``.  ``plan``: a PairPlan
    (the list is its ``plan_rows``), or an int, the capacity of a list that ``launch`` itself
    writes into ``rows`` and ``n_rows``."""
    from .optim import row_optimizer_of

    opt = row_optimizer_of(leaf)
    if opt is None:
        raise RuntimeError("msha: the optimizer of a fuse_row_grad table is gone before its "
                           "backward")
    if isinstance(plan, PairPlan):
        rows, n_rows = plan_rows(plan)
    else:
        rows = torch.empty(int(plan), dtype=torch.int32, device=leaf.device)
        n_rows = torch.empty((), dtype=torch.int32, device=leaf.device)
    vals = torch.empty(rows.numel(), leaf.shape[1], dtype=torch.float32, device=leaf.device)
    opt.stash_row_grad(leaf, RowGrad(rows, n_rows, vals, leaf.shape))  # raises past its limit
    launch(rows.data_ptr(), n_rows.data_ptr(), rows.numel(), vals.data_ptr())


def _replay_catch_up(h, plan, make_plan):
    """Before a loss reads the table ``h``: when ``h`` is registered with
    ``optim.Adam.fuse_row_grad(replay=True)``, the rows the loss is about to read are
    brought up to the present step (``Adam.catch_up``: one launch, nothing read back), in
    grad mode or not.  The rows are those of ``plan``, or of ``make_plan()``, built here.
    Returns the plan (``plan`` unchanged for any other ``h``)."""
    if not getattr(h, "_msha_row_replay", False):
        return plan
    from .optim import row_optimizer_of

    opt = row_optimizer_of(h)
    if opt is None:
        return plan
    if plan is None:
        plan = make_plan()
    opt.catch_up(h, plan)
    return plan


def row_grad_union(grads):
    """The sum of 2 to 4 ``RowGrad``s of one table as one ``RowGrad`` (``msha_row_grad_union``):
    ``rows`` the ascending union (capacity ``min(n, sum of the capacities)``), ``values[i]`` the
    rows' values added left to right in fp32, +0.0 where a list does not hold the row -- what
    accumulating the dense fp32 gradients in that order gives, bit for bit.  Nothing is read
    back (capturable)."""
    grads = list(grads)
    if not 2 <= len(grads) <= _lib.MAX_ROW_LISTS:
        raise ValueError(f"row_grad_union: takes 2 to {_lib.MAX_ROW_LISTS} row gradients, got "
                         f"{len(grads)}")
    shape = grads[0].shape
    if any(g.shape != shape for g in grads):
        raise ValueError("row_grad_union: the row gradients are not of one table")
    n, Fd = shape
    dev = grads[0].values.device
    _lib.require_cuda(*(g.values for g in grads))
    lists = (_lib.MshaRowList * len(grads))()
    for d, g in zip(lists, grads):
        d.rows, d.n_rows = g.rows.data_ptr(), g.n_rows.data_ptr()
        d.cap, d.vals = g.rows.numel(), g.values.data_ptr()
    cap = min(n, sum(g.rows.numel() for g in grads))
    rows = torch.empty(cap, dtype=torch.int32, device=dev)
    n_rows = torch.empty((), dtype=torch.int32, device=dev)
    vals = torch.empty(cap, Fd, dtype=torch.float32, device=dev)
    ws = _workspace(dev, _lib.fn("msha_row_grad_union_workspace_size")(n))
    _lib.call("msha_row_grad_union", n, Fd, len(grads), ctypes.byref(lists), rows.data_ptr(),
              n_rows.data_ptr(), cap, vals.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.stream_handle(dev))
    return RowGrad(rows, n_rows, vals, shape)


def sample_negatives(graph, src, k: int = 1, n_cand: int | None = None, seed: int | None = None,
                     offset: int = 0, col_offset: int = 0):
    """``k`` non-edges per positive: ``(src_rep, dst_neg)``, int64 of length P * k, the pair
    (src[p], d) at p * k + j with d drawn exactly uniformly from the columns [0, n_cand)
    (default: the graph's) that are not neighbours of src[p] (``msha_negative_sample``: no
    rejection loop, one Philox draw and a binary search per pair).  ``graph``: a ``Graph``
    or ``(rowptr, col[, rowflag])`` int32 CSR tensors with columns ascending within a row; a
    virtual full row counts as having no edges.  d is -1 for a row without non-edges and
    for a ``src`` outside the CSR's rows; ``col_offset`` is added to d.  Draws follow
    (``seed``, ``offset``) and the installed replay counter (``set_rng_counter``): a captured
    graph draws fresh negatives on every replay."""
    if isinstance(graph, Graph):
        rowptr, col, rowflag, cols = graph.rowptr, graph.col, graph.rowflag, graph.n_cols
    else:
        rowptr, col = graph[0], graph[1]
        rowflag = graph[2] if len(graph) > 2 else None
        cols = None
    if n_cand is None:
        if cols is None:
            raise ValueError("sample_negatives: n_cand is needed with a bare CSR")
        n_cand = cols
    n_cand, k = int(n_cand), int(k)
    if k < 1:
        raise ValueError(f"sample_negatives: k must be at least 1, got {k}")
    if not 0 <= n_cand < 2 ** 31:
        raise ValueError(f"sample_negatives: n_cand must be in [0, 2^31), got {n_cand}")
    if src.dtype != torch.int64 or src.dim() != 1:
        raise TypeError("sample_negatives: src must be a 1-D int64 tensor")
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.numel() < 1:
        raise TypeError("sample_negatives: the CSR is (rowptr, col) int32 tensors")
    if rowflag is not None and (rowflag.dtype not in (torch.uint8, torch.bool)
                                or rowflag.numel() != rowptr.numel() - 1):
        raise TypeError("sample_negatives: rowflag is one uint8 per CSR row")
    _lib.require_cuda(src, rowptr, col, rowflag)
    src, rowptr, col = src.contiguous(), rowptr.contiguous(), col.contiguous()
    if rowflag is not None:
        rowflag = rowflag.contiguous()
    if seed is None:
        seed = new_seed()
    P, dev = src.numel(), src.device
    src_rep = torch.empty(P * k, dtype=torch.int64, device=dev)
    dst_neg = torch.empty(P * k, dtype=torch.int64, device=dev)
    _lib.call("msha_negative_sample", P, k, src.data_ptr() if P else None, rowptr.numel() - 1,
              n_cand, col.numel(), rowptr.data_ptr(), col.data_ptr() if col.numel() else None,
              _lib.ptr(rowflag), int(col_offset), int(seed), int(offset), src_rep.data_ptr(),
              dst_neg.data_ptr(), _stream(src))
    return src_rep, dst_neg


# The front shared by the table losses (link_bce_loss, link_mlp_loss, link_distill_loss,
# link_match_loss).  `name` is the loss's name in the message.
def _rows16(t):
    """``t`` itself when the kernels can read it in place (unit column stride, 16-byte row
    pitch and base), else a contiguous copy."""
    esz = t.element_size()
    ok = t.stride(1) == 1 and (t.stride(0) * esz) % 16 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def _check_table_dtype(name, t, what="table"):
    if t.dtype not in (torch.float32, BF16):
        raise TypeError(f"{name} takes a float32 or bfloat16 {what}, got {t.dtype}")


def _check_table_shape(name, t, arg="h", form="(n, F)", rows=False):
    if t.dim() != 2 or (rows and t.shape[0] < 1):
        raise ValueError(f"{name}: {arg} must be {form}, got {tuple(t.shape)}")


def _check_table_width(name, *tables):
    for t in tables:
        if t is not None and not _lib.fn("msha_link_bce_supported")(t.shape[1], _code(t.dtype)):
            raise ValueError(f"{name}: feature width {t.shape[1]} of a {t.dtype} table is not "
                             f"supported (a power of two, 16 bytes to 64 lanes x 16 bytes)")


def _check_plan(name, plan, n, P, context=False):
    """``plan`` is None or the PairPlan of a list of P pairs over n rows (``context``: one that
    carries its flat src, a ``context_plan``)."""
    if plan is None:
        return
    ok = isinstance(plan, PairPlan) and plan.n == n and plan.n_pairs == P
    if context and not (ok and getattr(plan, "src", None) is not None):
        raise ValueError(f"{name}: plan is not a context_plan of this context and table")
    if not ok:
        raise ValueError(f"{name}: plan is not a PairPlan of this pair list and table")


def _check_same_device(name, h, *tensors):
    for t in tensors:
        if t is not None and t.device != h.device:
            raise ValueError(f"{name}: every tensor must be on the table's device")


def _table_grad(dH, dt):
    """The fp32 sum ``dH`` as the gradient of a table of dtype ``dt``."""
    return dH if dt == torch.float32 else dH.to(dt)


def _pair_grad_backward(ctx, gloss, hh, dense, rows, pair_args):
    """The backward of a loss whose table gradient is a pair-list sum under ``ctx.plan``
    (pair_grad.h): entry point ``dense`` for an (n, F) gradient, ``rows`` for the touched rows
    of a ``fuse_row_grad`` leaf.  ``pair_args``: the pair list's and the factor's pointers, the
    arguments between ``n`` and ``gloss``."""
    n, Fd = hh.shape
    plan, dev = ctx.plan, hh.device
    P = plan.n_pairs
    g = gloss.detach().to(torch.float32).reshape(1).contiguous()
    ws = _workspace(dev, _lib.fn(dense + "_workspace_size")(P, Fd))
    args = (P, Fd, _code(ctx.dt), hh.data_ptr(), hh.stride(0), n, *pair_args, g.data_ptr(),
            plan.rowptr.data_ptr(), plan.ent.data_ptr(), plan.chunk_tab.data_ptr())
    tail = (ws.data_ptr(), ws.numel(), _stream(hh))
    others = (None,) * (len(ctx.needs_input_grad) - 1)
    if ctx.leaf is not None and ctx.needs_input_grad[0]:
        # a fuse_row_grad table: the touched rows' gradient goes to its optimizer, no
        # (n, F) buffer is formed and .grad stays None
        _stash_rows(ctx.leaf, plan, lambda *rows_vals: _lib.call(rows, *args, *rows_vals, *tail))
        return (None,) + others
    dH = torch.empty(n, Fd, dtype=torch.float32, device=dev)
    _lib.call(dense, *args, dH.data_ptr(), *tail)
    return (_table_grad(dH, ctx.dt),) + others


class _LinkBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, src, dst, target, weight, plan):
        dt = h.dtype
        hh = _rows16(h.detach())
        n, Fd = hh.shape
        P, dev, s = src.numel(), hh.device, _stream(hh)
        z = torch.empty(P, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        npad = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(dev, _lib.fn("msha_link_bce_fwd_workspace_size")(P))
        _lib.call("msha_link_bce_fwd", P, Fd, _code(dt), hh.data_ptr(), hh.stride(0), n,
                  src.data_ptr(), dst.data_ptr(), target.data_ptr(), _lib.ptr(weight),
                  z.data_ptr(), loss.data_ptr(), npad.data_ptr(), ws.data_ptr(), ws.numel(), s)
        ctx.plan, ctx.dt = plan, dt
        ctx.leaf = _row_leaf(h, plan)  # the registered table itself (its optimizer updates it)
        ctx.save_for_backward(hh, src, dst, target, weight, z)
        ctx.mark_non_differentiable(z, npad)
        return loss, z, npad

    @staticmethod
    def backward(ctx, gloss, _gz=None, _gpad=None):
        hh, src, dst, target, weight, z = ctx.saved_tensors
        return _pair_grad_backward(
            ctx, gloss, hh, "msha_link_bce_bwd", "msha_link_bce_bwd_rows",
            (src.data_ptr(), dst.data_ptr(), target.data_ptr(), _lib.ptr(weight), z.data_ptr()))


def link_bce_loss(h, src, dst, target, weight=None, plan=None, return_logits=False):
    """Binary cross-entropy of the inner-product link logits, fused with the caller's gather
    and with a deterministic table gradient:

        F.binary_cross_entropy_with_logits((h[src] * h[dst]).sum(-1), target, weight,
                                           reduction="sum")

    and, with ``weight=None``, the mean.  ``h`` (n, F) float32 or bfloat16 (F a power of two
    spanning 16 bytes to 64 lanes x 16 bytes of a row); ``src`` / ``dst`` int64 (P,);
    ``target`` (P,) in [0, 1], soft targets allowed; ``weight`` (P,) or None.  A pair with an
    index outside [0, n) is padding: it adds nothing (``return_logits`` shows NaN for it).
    Returns the fp32 scalar loss, or ``(loss, logits)`` with ``return_logits``.

    The gradient goes to ``h`` only (a bf16 ``h`` receives it cast from the fp32 sum).  It is
    summed per table row in the order of ``plan`` (``pair_plan(src, dst, n)``, built here
    when None; reuse it for as long as the pair list is unchanged) with no float atomics:
    bitwise reproducible.  Nothing (P, F)-sized is materialised and nothing is read back, so
    plan + loss + backward can be captured into one HIP graph."""
    _check_table_dtype("link_bce_loss", h)
    _check_table_shape("link_bce_loss", h)
    _pair_lists(src, dst, "link_bce_loss")
    P = src.numel()
    if P < 1 or h.shape[0] < 1:
        raise ValueError("link_bce_loss: needs at least one pair and one table row")
    if not target.is_floating_point() or target.shape != (P,):
        raise ValueError(f"link_bce_loss: target must be a float tensor of shape ({P},), got "
                         f"{target.dtype} {tuple(target.shape)}")
    if weight is not None and (not weight.is_floating_point() or weight.shape != (P,)):
        raise ValueError(f"link_bce_loss: weight must be a float tensor of shape ({P},), got "
                         f"{weight.dtype} {tuple(weight.shape)}")
    _check_plan("link_bce_loss", plan, h.shape[0], P)
    _check_table_width("link_bce_loss", h)
    _check_same_device("link_bce_loss", h, src, dst, target, weight)
    _lib.require_cuda(h)
    target = target.detach().to(torch.float32).contiguous()
    weight = weight.detach().to(torch.float32).contiguous() if weight is not None else None
    src, dst = src.contiguous(), dst.contiguous()
    plan = _replay_catch_up(h, plan, lambda: pair_plan(src, dst, h.shape[0]))
    if plan is None and h.requires_grad and torch.is_grad_enabled():
        plan = pair_plan(src, dst, h.shape[0])  # only a backward reads it
    loss, z, _ = _LinkBCE.apply(h, src, dst, target, weight, plan)
    return (loss, z) if return_logits else loss


class _LinkMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b, src, dst, label, teacher, w_label, w_mse, p, seed, plan):
        dt = h.dtype
        hh = _rows16(h.detach())
        n, Fd = hh.shape
        N = W.shape[0]
        Wk = _tc(W.detach(), dt)  # the kernel's weight: bf16 for a bf16 table (score_pairs)
        bk = _f32c(b.detach())
        P, dev = src.numel(), hh.device
        out = torch.empty(P, N, dtype=torch.float32, device=dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)  # written by the kernel: no copy
        pv = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(dev, _lib.fn("msha_link_mlp_loss_fwd_workspace_size")(P))
        _lib.call("msha_link_mlp_loss_fwd", P, Fd, N, _code(dt), hh.data_ptr(), hh.stride(0), n,
                  src.data_ptr(), dst.data_ptr(), _lib.ptr(label), Wk.data_ptr(), bk.data_ptr(),
                  _lib.ptr(teacher), w_label, w_mse, p, seed, 0, out.data_ptr(),
                  terms.data_ptr(), loss.data_ptr(), pv.data_ptr(), ws.data_ptr(), ws.numel(),
                  _stream(hh))
        ctx.plan, ctx.dt, ctx.cfg = plan, dt, (w_label, w_mse, p)
        ctx.wdt, ctx.bdt = W.dtype, b.dtype
        ctx.leaf = _row_leaf(h, plan)  # the registered table itself (its optimizer updates it)
        ctx.save_for_backward(hh, Wk, src, dst, label, teacher, out, pv)
        ctx.mark_non_differentiable(out, terms, pv)
        return loss, out, terms, pv

    @staticmethod
    def backward(ctx, gloss, _go=None, _gt=None, _gp=None):
        hh, Wk, src, dst, label, teacher, out, pv = ctx.saved_tensors
        n, Fd = hh.shape
        P, N = out.shape
        dev, plan = hh.device, ctx.plan
        w_label, w_mse, p = ctx.cfg
        need_h, need_w = ctx.needs_input_grad[0], (ctx.needs_input_grad[1]
                                                   or ctx.needs_input_grad[2])
        g = gloss.detach().to(torch.float32).reshape(1).contiguous()
        dz = torch.empty(P, N, dtype=torch.float32, device=dev)
        dx = dH = dW = db = W32 = None
        if need_h:
            if plan is None:
                raise RuntimeError("link_mlp_loss: the gradient to h needs a PairPlan (h did not "
                                   "require grad when the loss was taken)")
            dx = torch.empty(P, Fd, dtype=torch.float32, device=dev)  # the one (P, F) buffer
            W32 = _f32c(Wk)
        if need_w:
            dW = torch.empty(N, Fd, dtype=torch.float32, device=dev)
            db = torch.empty(N, dtype=torch.float32, device=dev)
        ws = _workspace(dev, _lib.fn("msha_link_mlp_bwd_workspace_size")(P, Fd, N))
        args = (P, Fd, N, _code(ctx.dt), hh.data_ptr(), hh.stride(0), n, src.data_ptr(),
                dst.data_ptr(), _lib.ptr(label), _lib.ptr(W32), _lib.ptr(teacher),
                out.data_ptr(), pv.data_ptr(), w_label, w_mse, p, g.data_ptr(),
                _lib.ptr(plan.rowptr if need_h else None), _lib.ptr(plan.ent if need_h else None),
                _lib.ptr(plan.chunk_tab if need_h else None), dz.data_ptr(), _lib.ptr(dx),
                _lib.ptr(dW), _lib.ptr(db))
        tail = (ws.data_ptr(), ws.numel(), _stream(hh))
        if need_h and ctx.leaf is not None:
            # a fuse_row_grad table: the touched rows' gradient goes to its optimizer, no
            # (n, F) buffer is formed and .grad stays None
            _stash_rows(ctx.leaf, plan, lambda *rows_vals: _lib.call(
                "msha_link_mlp_bwd_rows", *args, *rows_vals, *tail))
        else:
            if need_h:
                dH = torch.empty(n, Fd, dtype=torch.float32, device=dev)
            _lib.call("msha_link_mlp_bwd", *args, _lib.ptr(dH), *tail)
            if need_h:
                dH = _table_grad(dH, ctx.dt)
        if need_w:
            dW = dW if ctx.wdt == torch.float32 else dW.to(ctx.wdt)
            db = db if ctx.bdt == torch.float32 else db.to(ctx.bdt)
        return (dH, dW if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None) + (None,) * 9


def link_mlp_loss(h, src, dst, W, b, *, label=None, teacher_out=None, w_label=1.0, w_mse=0.0,
                  p=0.0, training=False, seed=None, plan=None, return_output=False):
    """LLP's training objective for the 'mlp' link predictor with one used Linear
    (LLP.py:233, :235, :238), fused with the caller's gather:

        out  = torch.sigmoid(F.dropout(F.relu(F.linear(h[src] * h[dst], W, b)), p, training))
        loss = w_label * F.nll_loss(out, label) + w_mse * F.mse_loss(out, teacher_out)

    ``h`` (n, F) float32 or bfloat16, ``W`` (N, F), ``b`` (N,), F and N powers of two in
    [16, 128]; ``src`` / ``dst`` int64 (P,); ``label`` int64 (P,), default ``dst`` itself as
    LLP.py:235 uses it; ``teacher_out`` (P, N), detached, or None (no MSE term).  A pair whose
    ``src`` or ``dst`` lies outside [0, n) or whose label lies outside [0, N) is padding: it
    adds nothing to any term or gradient and is not counted in the means (``out`` shows NaN
    for it); with no valid pair the loss and every gradient are zero.  A bf16 ``h`` runs the
    bf16 MFMA forward with ``W`` cast to bf16, as ``score_pairs`` does.  Dropout follows
    ``msha_pair_linear``'s Philox stream (``dropout_keep_mask(P * N, p, seed)``).

    Returns the fp32 scalar, or ``(loss, out, terms)`` with ``return_output``: ``out`` (P, N)
    fp32 and ``terms`` = (loss, nll term, mse term), both without gradient.

    Gradients go to ``h``, ``W`` and ``b`` in their own dtypes.  The only (P, F)-sized array
    ever made is ``dx = dz @ W``; the weight gradient gathers ``h[src] * h[dst]`` in its MFMA
    loader, and the table gradient is summed per row in the order of ``plan``
    (``pair_plan(src, dst, n)``, built here when None and ``h`` needs a gradient; reuse it
    for as long as the pair list is unchanged).  No float atomics: bitwise reproducible.
    Nothing is read back, so plan + loss + backward can be captured into one HIP graph.
    When ``h`` is itself a leaf registered with ``optim.Adam.fuse_row_grad``, its gradient is
    formed on the plan's touched rows only (``RowGrad``, the dense gradient's rows bit for bit)
    and handed to that optimizer; ``h.grad`` stays None."""
    _check_table_dtype("link_mlp_loss", h)
    _check_table_shape("link_mlp_loss", h)
    _pair_lists(src, dst, "link_mlp_loss")
    P, Fd = src.numel(), h.shape[1]
    if P < 1 or h.shape[0] < 1:
        raise ValueError("link_mlp_loss: needs at least one pair and one table row")
    if not W.is_floating_point() or W.dim() != 2 or W.shape[1] != Fd:
        raise ValueError(f"link_mlp_loss: W must be a float (N, {Fd}) weight, got {W.dtype} "
                         f"{tuple(W.shape)}")
    N = W.shape[0]
    if not b.is_floating_point() or b.shape != (N,):
        raise ValueError(f"link_mlp_loss: b must be a float tensor of shape ({N},), got "
                         f"{b.dtype} {tuple(b.shape)}")
    if label is not None and (label.dtype != torch.int64 or label.shape != (P,)):
        raise ValueError(f"link_mlp_loss: label must be an int64 tensor of shape ({P},), got "
                         f"{label.dtype} {tuple(label.shape)}")
    if teacher_out is not None and (not teacher_out.is_floating_point()
                                    or teacher_out.shape != (P, N)):
        raise ValueError(f"link_mlp_loss: teacher_out must be a float tensor of shape "
                         f"({P}, {N}), got {teacher_out.dtype} {tuple(teacher_out.shape)}")
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"link_mlp_loss: p must be in [0, 1), got {p}")
    _check_plan("link_mlp_loss", plan, h.shape[0], P)
    if not _lib.fn("msha_link_mlp_supported")(Fd, N, _code(h.dtype)):
        raise ValueError(f"link_mlp_loss: widths F = {Fd}, N = {N} of a {h.dtype} table are not "
                         f"supported (powers of two in [16, 128])")
    _check_same_device("link_mlp_loss", h, src, dst, W, b, label, teacher_out)
    _lib.require_cuda(h)
    src, dst = src.contiguous(), dst.contiguous()
    label = label.contiguous() if label is not None else None
    if teacher_out is not None:
        teacher_out = teacher_out.detach().to(torch.float32).contiguous()
    if seed is None:
        seed = new_seed() if p > 0 else 0
    plan = _replay_catch_up(h, plan, lambda: pair_plan(src, dst, h.shape[0]))
    if plan is None and h.requires_grad and torch.is_grad_enabled():
        plan = pair_plan(src, dst, h.shape[0])  # only a backward reads it
    loss, out, terms, _ = _LinkMLP.apply(h, W, b, src, dst, label, teacher_out, float(w_label),
                                         float(w_mse), p, int(seed), plan)
    return (loss, out, terms) if return_output else loss


# ------------------------------------------------- link-prediction distillation ---
MAX_CONTEXT = 64  # context slots per anchor (one lane each)


def sample_context(graph, anchors, walks: int, hops: int, n_rand: int = 0,
                   n_nodes: int | None = None, seed: int | None = None, offset: int = 0):
    """The context nodes LLP distils over: int64 ``(A, K)``, ``K = walks * hops + n_rand``
    (1 <= K <= 64).  Walk ``w`` starts at ``anchors[a]`` and takes ``hops`` uniform steps
    along the CSR (``--ps_method nb``: hops = 1, ``rw``: hops > 1); slot ``w * hops + s``
    holds the node after step ``s``, and -1 from the first step out of a node without edges
    on (outside the CSR's rows, an empty row, a virtual full row).  The last ``n_rand`` slots
    are uniform over ``[0, n_nodes)`` (default: the graph's columns; needed with a bare CSR),
    -1 for an anchor outside the CSR's rows.  ``graph``: a ``Graph`` or ``(rowptr, col[,
    rowflag])`` int32 CSR tensors.  Duplicates and the anchor itself may appear, as in LLP.
    One Philox word per slot under (``seed``, ``offset``) and the installed replay counter
    (``set_rng_counter``): a captured graph draws a fresh context on every replay; nothing is
    read back (``msha_context_sample``)."""
    if isinstance(graph, Graph):
        rowptr, col, rowflag, cols = graph.rowptr, graph.col, graph.rowflag, graph.n_cols
    else:
        rowptr, col = graph[0], graph[1]
        rowflag = graph[2] if len(graph) > 2 else None
        cols = None
    walks, hops, n_rand = int(walks), int(hops), int(n_rand)
    if walks < 0 or hops < 0 or n_rand < 0:
        raise ValueError("sample_context: walks, hops and n_rand must not be negative")
    K = walks * hops + n_rand
    if not 1 <= K <= MAX_CONTEXT:
        raise ValueError(f"sample_context: K = walks * hops + n_rand must be in [1, "
                         f"{MAX_CONTEXT}], got {K}")
    if n_nodes is None:
        if cols is None and n_rand > 0:
            raise ValueError("sample_context: n_nodes is needed with a bare CSR")
        n_nodes = cols if cols is not None else 1
    n_nodes = int(n_nodes)
    if n_rand > 0 and not 1 <= n_nodes < 2 ** 31:
        raise ValueError(f"sample_context: n_nodes must be in [1, 2^31), got {n_nodes}")
    if anchors.dtype != torch.int64 or anchors.dim() != 1:
        raise TypeError("sample_context: anchors must be a 1-D int64 tensor")
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.numel() < 1:
        raise TypeError("sample_context: the CSR is (rowptr, col) int32 tensors")
    if rowflag is not None and (rowflag.dtype not in (torch.uint8, torch.bool)
                                or rowflag.numel() != rowptr.numel() - 1):
        raise TypeError("sample_context: rowflag is one uint8 per CSR row")
    _lib.require_cuda(anchors, rowptr, col, rowflag)
    anchors, rowptr, col = anchors.contiguous(), rowptr.contiguous(), col.contiguous()
    if rowflag is not None:
        rowflag = rowflag.contiguous()
    if seed is None:
        seed = new_seed()
    A, dev = anchors.numel(), anchors.device
    ctx = torch.empty(A, K, dtype=torch.int64, device=dev)
    _lib.call("msha_context_sample", A, walks, hops, n_rand, anchors.data_ptr() if A else None,
              rowptr.numel() - 1, n_nodes, col.numel(), rowptr.data_ptr(),
              col.data_ptr() if col.numel() else None, _lib.ptr(rowflag), int(seed), int(offset),
              ctx.data_ptr() if A else None, _stream(anchors))
    return ctx


def _context_lists(anchors, context, what):
    if anchors.dtype != torch.int64 or context.dtype != torch.int64:
        raise TypeError(f"{what}: anchors and context must be int64 index tensors")
    if anchors.dim() != 1 or context.dim() != 2 or context.shape[0] != anchors.numel():
        raise ValueError(f"{what}: anchors must be (A,) and context (A, K), got "
                         f"{tuple(anchors.shape)} and {tuple(context.shape)}")
    if 2 * context.numel() >= 2 ** 31:
        raise ValueError(f"{what}: 2 * A * K must be below 2^31, got A * K = {context.numel()}")


def context_plan(anchors, context, n: int) -> PairPlan:
    """The ``PairPlan`` of the flat pairs ``(anchors[p // K], context.flat[p])`` over ``n``
    table rows (``pair_plan``); it carries the flat ``src`` it built.  Valid for as long as
    ``(anchors, context)`` is unchanged."""
    _context_lists(anchors, context, "context_plan")
    if anchors.device != context.device:
        raise ValueError("context_plan: anchors and context must be on one device")
    A, K = context.shape
    src = anchors.reshape(A, 1).expand(A, K).reshape(-1)  # a copy: (A K,)
    plan = pair_plan(src, context.reshape(-1), n)
    plan.src = src
    return plan


class _LinkDistill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, anchors, context, tl, th, margin, tau, w_rank, w_dist, w_prob, plan):
        dt = h.dtype
        hh = _rows16(h.detach())
        n, Fd = hh.shape
        A, K = context.shape
        dev, s = hh.device, _stream(hh)
        if th is not None:
            th = _rows16(th)
            t_args = (th.data_ptr(), th.shape[1], _code(th.dtype), th.stride(0), th.shape[0])
        else:
            t_args = (None, 0, 0, 0, 0)
        logits = torch.empty(A, K, dtype=torch.float32, device=dev)
        g = torch.empty(A, K, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        npad = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(dev, _lib.fn("msha_link_distill_fwd_workspace_size")(A))
        _lib.call("msha_link_distill_fwd", A, K, Fd, _code(dt), hh.data_ptr(), hh.stride(0), n,
                  anchors.data_ptr(), context.data_ptr(), _lib.ptr(tl), *t_args, margin, tau,
                  w_rank, w_dist, w_prob, logits.data_ptr(), g.data_ptr(), loss.data_ptr(),
                  terms.data_ptr(), npad.data_ptr(), ws.data_ptr(), ws.numel(), s)
        ctx.plan, ctx.dt = plan, dt
        ctx.leaf = _row_leaf(h, plan)  # the registered table itself (its optimizer updates it)
        ctx.save_for_backward(hh, context, g)
        ctx.mark_non_differentiable(terms, logits, npad)
        return loss, terms, logits, npad

    @staticmethod
    def backward(ctx, gloss, _gt=None, _gz=None, _gpad=None):
        hh, context, g = ctx.saved_tensors
        return _pair_grad_backward(
            ctx, gloss, hh, "msha_pair_grad_bwd", "msha_pair_grad_bwd_rows",
            (ctx.plan.src.data_ptr(), context.data_ptr(), g.data_ptr()))


def link_distill_loss(h, anchors, context, *, teacher_logits=None, teacher_table=None,
                      margin: float = 0.1, tau: float = 1.0, w_rank: float = 1.0,
                      w_dist: float = 1.0, w_prob: float = 0.0, plan=None, return_terms=False,
                      return_logits=False):
    """LLP's teacher-matching loss of the inner-product student logits
    ``y[a, k] = <h[anchors[a]], h[context[a, k]]>`` against teacher logits ``t[a, k]``
    (``teacher_logits`` (A, K), or the same inner product on ``teacher_table`` (n_t, F_t);
    exactly one of the two; never differentiated), fused with the gather:

        L_R = sum_{i<j} F.margin_ranking_loss(y_i, y_j, r_ij, margin, "sum"),
              r_ij = sign(t_i - t_j) where |t_i - t_j| > margin, else 0       (rank-based)
        L_D = F.kl_div(log_softmax(y / tau), softmax(t / tau), "sum")        (distribution)
        L_P = sum (sigmoid(y) - sigmoid(t))^2                 (LLP.py:238's KD_p MSE, summed)
        loss = (w_rank L_R + w_dist L_D + w_prob L_P) / A

    ``h`` (n, F) float32 or bfloat16 under ``link_bce_loss``'s width rule; ``anchors`` int64
    (A,); ``context`` int64 (A, K), 2 <= K <= 64 (``sample_context``).  A slot whose anchor or
    context index is outside the table(s) is padding: it enters no term and shows NaN in the
    logits.  Returns the fp32 scalar loss, then ``terms`` (3,) = (L_R, L_D, L_P) / A with
    ``return_terms`` and the (A, K) logits with ``return_logits``.

    The gradient goes to ``h`` only, summed per table row in the order of ``plan``
    (``context_plan(anchors, context, n)``, built here when None and a gradient is needed)
    with no float atomics: bitwise reproducible, nothing (A, K, F)-sized is materialised and
    nothing is read back, so sample + plan + loss + backward capture into one HIP graph."""
    _check_table_dtype("link_distill_loss", h)
    _check_table_shape("link_distill_loss", h)
    _context_lists(anchors, context, "link_distill_loss")
    A, K = context.shape
    if A < 1 or h.shape[0] < 1:
        raise ValueError("link_distill_loss: needs at least one anchor and one table row")
    if not 2 <= K <= MAX_CONTEXT:
        raise ValueError(f"link_distill_loss: K must be in [2, {MAX_CONTEXT}], got {K}")
    if (teacher_logits is None) == (teacher_table is None):
        raise ValueError("link_distill_loss: give exactly one of teacher_logits and "
                         "teacher_table")
    if teacher_logits is not None and (not teacher_logits.is_floating_point()
                                       or teacher_logits.shape != (A, K)):
        raise ValueError(f"link_distill_loss: teacher_logits must be a float tensor of shape "
                         f"({A}, {K}), got {teacher_logits.dtype} {tuple(teacher_logits.shape)}")
    if teacher_table is not None:
        _check_table_dtype("link_distill_loss", teacher_table, "teacher table")
        _check_table_shape("link_distill_loss", teacher_table, "teacher_table", "(n_t, F_t)",
                           rows=True)
    margin, tau = float(margin), float(tau)
    if not tau > 0.0:
        raise ValueError(f"link_distill_loss: tau must be positive, got {tau}")
    if not margin >= 0.0:
        raise ValueError(f"link_distill_loss: margin must not be negative, got {margin}")
    _check_plan("link_distill_loss", plan, h.shape[0], A * K, context=True)
    _check_table_width("link_distill_loss", h, teacher_table)
    _check_same_device("link_distill_loss", h, anchors, context, teacher_logits, teacher_table)
    _lib.require_cuda(h)
    anchors, context = anchors.contiguous(), context.contiguous()
    tl = (teacher_logits.detach().to(torch.float32).contiguous()
          if teacher_logits is not None else None)
    th = teacher_table.detach() if teacher_table is not None else None
    plan = _replay_catch_up(h, plan, lambda: context_plan(anchors, context, h.shape[0]))
    if plan is None and h.requires_grad and torch.is_grad_enabled():
        plan = context_plan(anchors, context, h.shape[0])  # only a backward reads it
    loss, terms, logits, _ = _LinkDistill.apply(h, anchors, context, tl, th, margin, tau,
                                                float(w_rank), float(w_dist), float(w_prob), plan)
    out = (loss,) + ((terms,) if return_terms else ()) + ((logits,) if return_logits else ())
    return out if len(out) > 1 else loss


# ------------------------------------------------------ representation matching ---
class _LinkMatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, rows, th):
        dt = h.dtype
        hh, th = _rows16(h.detach()), _rows16(th)
        n, Fd = hh.shape
        P = rows.numel() if rows is not None else n
        dev, s = hh.device, _stream(hh)
        coef = torch.empty(n, 2, dtype=torch.float32, device=dev)
        cos_rows = torch.empty(n, dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        npad = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(dev, _lib.fn("msha_link_match_fwd_workspace_size")(P, n))
        _lib.call("msha_link_match_fwd", P, Fd, _code(dt), hh.data_ptr(), hh.stride(0), n,
                  _code(th.dtype), th.data_ptr(), th.stride(0), th.shape[0], _lib.ptr(rows),
                  coef.data_ptr(), cos_rows.data_ptr(), count.data_ptr(), loss.data_ptr(),
                  npad.data_ptr(), ws.data_ptr(), ws.numel(), s)
        ctx.dt = dt
        # the registered table itself: the rows that occur are listed from count in the
        # backward (rows=None names every row: dense)
        ctx.leaf = _row_leaf(h, min(n, P) if rows is not None else None)
        ctx.entries = P
        ctx.save_for_backward(hh, th, coef, count)
        ctx.mark_non_differentiable(cos_rows, count, npad)
        return loss, cos_rows, count, npad

    @staticmethod
    def backward(ctx, gloss, _gc=None, _gn=None, _gp=None):
        hh, th, coef, count = ctx.saved_tensors
        n, Fd = hh.shape
        g = gloss.detach().to(torch.float32).reshape(1).contiguous()
        args = (Fd, _code(ctx.dt), hh.data_ptr(), hh.stride(0), n, _code(th.dtype),
                th.data_ptr(), th.stride(0), th.shape[0], coef.data_ptr(), g.data_ptr())
        if ctx.leaf is not None and ctx.needs_input_grad[0]:
            # a fuse_row_grad table: the rows that occur and their gradient go to its optimizer
            P, s = ctx.entries, _stream(hh)
            ws = _workspace(hh.device, _lib.fn("msha_plan_rows_workspace_size")(n))

            def launch(rows, n_rows, cap, vals):
                _lib.call("msha_link_match_rows", P, n, count.data_ptr(), rows, n_rows,
                          ws.data_ptr(), ws.numel(), s)
                _lib.call("msha_link_match_bwd_rows", P, *args, rows, n_rows, cap, vals, s)

            _stash_rows(ctx.leaf, min(n, P), launch)
            return None, None, None
        dH = torch.empty(n, Fd, dtype=torch.float32, device=hh.device)
        _lib.call("msha_link_match_bwd", *args, dH.data_ptr(), _stream(hh))
        return _table_grad(dH, ctx.dt), None, None


def link_match_loss(h, rows, teacher_table, *, return_rows=False):
    """LLP's representation-matching term (LLP.py:34-35, :237), fused with the caller's two
    gathers and with a deterministic table gradient:

        1 - F.cosine_similarity(h[rows], teacher_table[rows].detach(), dim=-1).mean()

    ``h`` (n, F) and ``teacher_table`` (n_t, F): float32 or bfloat16 each, independently,
    under ``link_bce_loss``'s width rule; ``rows`` int64 (P,).  An entry outside
    [0, min(n, n_t)) is padding: it enters nothing and the mean is over the others (none:
    loss 0).  ``rows=None``: row b of ``h`` against row b of ``teacher_table`` (equal row
    counts), the reference's ``KD_cosine(s, t)`` on tensors already gathered.  Returns the
    fp32 scalar loss, or ``(loss, cos_rows, count)`` with ``return_rows``: the cosine of
    every table row (NaN where the row does not occur) and its int32 occurrence count.

    The gradient goes to ``h`` only (a bf16 ``h`` receives it cast from the fp32 row); the
    teacher is never differentiated.  Every occurrence of a row adds the same cosine and the
    same gradient row, so the work is an integer histogram of ``rows`` and one pass over the
    table rows that occur: loss, counts and gradient are a function of the *multiset* of
    ``rows`` (and the tables) alone -- bitwise reproducible and unchanged by any permutation
    of ``rows`` -- with no float atomics, nothing (P, F)-sized and nothing read back, so
    loss + backward can be captured into one HIP graph.  When ``h`` is itself a leaf
    registered with ``optim.Adam.fuse_row_grad`` and ``rows`` is given, its gradient is formed
    on the rows that occur only (``RowGrad``: the ascending rows with a count, at most
    min(n, P)) and handed to that optimizer; ``h.grad`` stays None."""
    t = teacher_table
    _check_table_dtype("link_match_loss", h)
    _check_table_dtype("link_match_loss", t, "teacher table")
    _check_table_shape("link_match_loss", h, rows=True)
    _check_table_shape("link_match_loss", t, "teacher_table", "(n_t, F)", rows=True)
    if t.shape[1] != h.shape[1]:
        raise ValueError(f"link_match_loss: student and teacher must have one width, got "
                         f"{h.shape[1]} and {t.shape[1]}")
    if rows is not None:
        if rows.dtype != torch.int64:
            raise TypeError("link_match_loss: rows must be an int64 index tensor")
        if rows.dim() != 1 or not 1 <= rows.numel() < 2 ** 31:
            raise ValueError(f"link_match_loss: rows must be 1-D with 1 <= P < 2^31, got "
                             f"{tuple(rows.shape)}")
    elif t.shape[0] != h.shape[0]:
        raise ValueError(f"link_match_loss: rows=None needs equal row counts, got "
                         f"{h.shape[0]} and {t.shape[0]}")
    _check_table_width("link_match_loss", h, t)
    _check_same_device("link_match_loss", h, rows, t)
    _lib.require_cuda(h)
    rows = rows.contiguous() if rows is not None else None
    if rows is not None:
        # (the backward lists the rows from its histogram: too late for the read; the
        # (rows, rows) plan gives the distinct rows now)
        _replay_catch_up(h, None, lambda: pair_plan(rows, rows, h.shape[0]))
    else:
        _replay_catch_up(h, None, lambda: None)  # every row is read: the flush
    loss, cos_rows, count, _ = _LinkMatch.apply(h, rows, t.detach())
    return (loss, cos_rows, count) if return_rows else loss


# --------------------------------------------------------- full MSHA layer (Ours) ---
class _OursAttention(torch.autograd.Function):
    """Inter attention (u, v) exactly as edge_attention computes it, plus the batch intra
    attention added to u, in one of two intra modes.
    Joint (Ours.py:54-101; msha_ours_intra_fwd / _bwd): city and province under one
    normaliser with the inter attention; its backward has a term into every inter row
    (row_coef) and the score vectors a3s / a4s.
    ``split`` (Ablation.py:165-202, OursLayer2; msha_ours_split_fwd / _bwd): city and
    province each under its own softmax.  The intra weights are 1 / group size, so the
    backward has no term into el / er / lse and a3s / a4s get exact zeros (their reference
    gradient is rounding noise around 0); no attention export."""

    @staticmethod
    def forward(ctx, el, er, h1, h2, a3s, a4s, graph: Graph, groups, src, p: float, seed: int,
                slope: float, split: bool):
        n, H = el.shape
        m, _, Fd = h1.shape
        dt = _table_dtype(h1, h2)
        el, er, h1, h2 = _f32c(el), _f32c(er), _tc(h1, dt), _tc(h2, dt)
        src = src.to(torch.int64).contiguous()
        B = src.numel()
        dev = el.device
        s = _stream(el)
        if split:  # the score vectors are not read: only what their zero gradients look like
            ctx.a_meta = (a3s.shape, a3s.dtype, a4s.shape, a4s.dtype)
            scores = ()
        else:
            scores = (_f32c(a3s), _f32c(a4s))
        bstat = torch.empty(max(B, 1), H, 8, device=dev, dtype=torch.float32)
        u = torch.empty(n, H, Fd, device=dev, dtype=dt)
        head = (graph.desc, groups.desc, B, src.data_ptr(), H, Fd, _code(dt), h2.data_ptr())

        def intra(it):
            if split:
                _lib.call("msha_ours_split_fwd", *head, it.u.data_ptr(), p, seed, 0,
                          bstat.data_ptr(), u.data_ptr(), s)
            else:
                _lib.call("msha_ours_intra_fwd", *head, scores[0].data_ptr(),
                          scores[1].data_ptr(), el.data_ptr(), er.data_ptr(), it.lse.data_ptr(),
                          it.u.data_ptr(), slope, p, seed, 0, bstat.data_ptr(), u.data_ptr(), s)

        # (bipartite: u, v and the joint mode's attention export in one pass)
        it = _inter_fwd(graph, el, er, h1, h2, slope, p, seed, export_attd=not split,
                        keep_u_lo=any(ctx.needs_input_grad[:4]), intra=intra)
        ctx.bip, ctx.split = it.bip, split
        ctx.graph, ctx.groups, ctx.p, ctx.seed, ctx.slope = graph, groups, p, seed, slope
        # the bipartite backward recomputes from (el, er, lse); the row form also reads the
        # inter aggregate
        empty = el.new_empty(0)
        ctx.save_for_backward(el, er, h1, h2, it.lse, bstat, src, empty if it.bip else it.u,
                              it.u_lo if it.u_lo is not None else empty, *scores)
        # post-dropout inter attention and batch statistics: outputs for record mode
        attd = None if split else it.attd
        ctx.mark_non_differentiable(*((bstat,) if split else (attd, bstat)))
        ctx.set_materialize_grads(False)  # no zero-filled gradients for attd / bstat
        return u, it.v, attd, bstat

    @staticmethod
    def backward(ctx, dU, dV, _attd=None, _bstat=None):
        el, er, h1, h2, lse, bstat, src, u_inter, u_lo, *scores = ctx.saved_tensors
        u_lo = u_lo if u_lo.numel() else None
        graph, groups, split = ctx.graph, ctx.groups, ctx.split
        n, H = el.shape
        m, _, Fd = h1.shape
        B = src.numel()
        dev = el.device
        s = _stream(el)
        dt = h1.dtype
        dU = torch.zeros(n, H, Fd, device=dev, dtype=dt) if dU is None else _tc(dU, dt)
        dV = torch.zeros(m, H, Fd, device=dev, dtype=dt) if dV is None else _tc(dV, dt)
        G = torch.empty(max(B, 1), 2, H * Fd, device=dev, dtype=torch.float32)
        size_fn = "msha_ours_split_workspace_size" if split else "msha_ours_workspace_size"
        ws = _workspace(dev, _memo(groups, (size_fn, B, H, Fd), lambda: int(
            _lib.fn(size_fn)(groups.desc, B, H, Fd))))
        head = (graph.desc, groups.desc, B, src.data_ptr(), H, Fd, _code(dt))
        # stage 0 (zeroes what it accumulates into), the inter row pass, stage 1
        if split:
            row_coef = None
            das = torch.empty(2, H, Fd, device=dev, dtype=torch.float32)
            head += (bstat.data_ptr(),)
            tail = (ctx.p, ctx.seed, 0, G.data_ptr())
            _lib.call("msha_ours_split_bwd", *head, dU.data_ptr(), 0, *tail, das[0].data_ptr(),
                      das[1].data_ptr(), None, ws.data_ptr(), ws.numel(), s)
            sh3, dt3, sh4, dt4 = ctx.a_meta  # (das is final: the zeros stage 0 wrote)
            da3s, da4s = das[0].view(sh3).to(dt3), das[1].view(sh4).to(dt4)

            def intra(d_hs):
                _lib.call("msha_ours_split_bwd", *head, None, 1, *tail, None, None,
                          d_hs.data_ptr(), None, 0, s)
        else:
            bgrad = torch.empty(max(B, 1), H, 4, device=dev, dtype=torch.float32)
            row_coef = torch.empty(n, H, device=dev, dtype=torch.float32)
            da3s = torch.empty(H, Fd, device=dev, dtype=torch.float32)
            da4s = torch.empty(H, Fd, device=dev, dtype=torch.float32)
            head += (h2.data_ptr(), scores[0].data_ptr(), scores[1].data_ptr(), bstat.data_ptr(),
                     dU.data_ptr())
            tail = (ctx.slope, ctx.p, ctx.seed, 0, G.data_ptr(), bgrad.data_ptr())
            _lib.call("msha_ours_intra_bwd", *head, 0, *tail, row_coef.data_ptr(),
                      da3s.data_ptr(), da4s.data_ptr(), None, ws.data_ptr(), ws.numel(), s)

            def intra(d_hs):
                _lib.call("msha_ours_intra_bwd", *head, 1, *tail, None, None, None,
                          d_hs.data_ptr(), None, 0, s)
        d_el, d_er, d_hc, d_hs = _inter_bwd(graph, ctx.bip, el, er, h1, lse, u_inter, u_lo, dU, h2,
                                            dV, row_coef, ctx.slope, ctx.p, ctx.seed, intra=intra)
        return d_el, d_er, d_hc, d_hs, da3s, da4s, None, None, None, None, None, None, None


def _ours_apply(name, split, graph, groups, src, el, er, h1, h2, a3s, a4s, p, training, slope,
                seed):
    _lib.require_cuda(el, er, h1, h2, a3s, a4s, src)
    H, Fd = el.shape[1], h1.shape[-1]
    if not _lib.load().msha_edge_attention_supported(H, Fd):
        raise NotImplementedError(f"{name}: (heads={H}, feat={Fd}) not compiled")
    if H * Fd > 512:
        raise NotImplementedError(f"{name}: heads*feat must be <= 512")
    p = float(p) if training else 0.0
    if seed is None:
        seed = new_seed() if p > 0 else 0
    return _OursAttention.apply(el, er, h1, h2, a3s, a4s, graph, groups, src, p, seed, slope, split)


def ours_attention(graph: Graph, groups, src, el, er, h1, h2, a3s, a4s, p: float = 0.0,
                   training: bool = False, slope: float = NEG_SLOPE, seed: int | None = None,
                   return_aux: bool = False):
    """Full MSHA attention core (Ours.py:54-101): returns (u, v), u = inter + intra;
    with return_aux also (attd (E, H) post-dropout inter attention, bstat (B, H, 8))."""
    u, v, attd, bstat = _ours_apply("ours_attention", False, graph, groups, src, el, er, h1, h2,
                                    a3s, a4s, p, training, slope, seed)
    return (u, v, attd, bstat) if return_aux else (u, v)


def ours_split_attention(graph: Graph, groups, src, el, er, h1, h2, a3s, a4s, p: float = 0.0,
                         training: bool = False, slope: float = NEG_SLOPE,
                         seed: int | None = None, return_aux: bool = False):
    """OursLayer2's attention core (Ablation.py:165-202): ``ours_attention`` with city and
    province attention each under its own softmax instead of the joint normaliser.  Returns
    (u, v); with return_aux also bstat (B, H, 8) (the intra weights 1 / group size in slots
    5 / 6).  a3s / a4s cannot change the output and get exact zero gradients; the dropout
    draws are ``ours_attention``'s (same Philox keys)."""
    u, v, _, bstat = _ours_apply("ours_split_attention", True, graph, groups, src, el, er, h1, h2,
                                 a3s, a4s, p, training, slope, seed)
    return (u, v, bstat) if return_aux else (u, v)


# ------------------------------------------------------------------ model head ---
HEAD_TAPS = None  # tests: a list here collects each model-head forward's inputs and statistics
def head_supported(graph: Graph, heads: int, feat: int) -> bool:
    return bool(_lib.load().msha_head_supported(graph.n_cols, heads, feat))


_HP_CACHE: dict = {}


def _head_params(H, F, eps, momentum, slope, ptrs, dyn=None):
    """msha_head_params from pointer lists: the ``ptrs`` part is built once per distinct
    set of pointers (the parameters and buffers stay put across steps) and copied; the
    ``dyn`` part (this call's gradient outputs) is written into the copy."""
    key = (H, F, eps, momentum, slope, tuple((k, None if v is None else tuple(v))
                                            for k, v in ptrs.items()))
    base = _HP_CACHE.get(key)
    if base is None:
        if len(_HP_CACHE) > 64:
            _HP_CACHE.clear()
        base = _lib.MshaHeadParams()
        base.heads, base.feat, base.eps, base.momentum, base.slope = H, F, eps, momentum, slope
        for name, lst in ptrs.items():
            arr = getattr(base, name)
            for h in range(len(lst) if lst is not None else H):
                arr[h] = lst[h] if lst is not None else None
        _HP_CACHE[key] = base
    hp = _lib.MshaHeadParams.from_buffer_copy(base)
    for name, lst in (dyn or {}).items():
        arr = getattr(hp, name)
        for h, v in enumerate(lst):
            arr[h] = v
    return hp


# the loss backward flags its gradient's nonzero rows for the model head's backward
# (msha_nll_rows_bwd_flags -> msha_head_bwd_flagged: one launch fewer per step);
# MSHA_NLL_FLAGS=0 keeps the head's own row scan (A/B).  HEAD_BWD_FLAGGED counts the head
# backwards that took the flags (tests).
NLL_FLAGS = os.environ.get("MSHA_NLL_FLAGS", "1") != "0"
HEAD_BWD_FLAGGED = [0]


class _ModelHead(torch.autograd.Function):
    """msha_head_fwd / msha_head_bwd: the heads' BatchNorm + LeakyReLU epilogues,
    elu(u_out @ v_out.T), cat, dropout, out_att (GraphAttentionLayer), elu, log_softmax
    (Ablation.py:273-277 + :298-301; Ours.py:100-109 + :163-167).  ``params``: the heads'
    bn2 (u side) weights, bn2 biases, bn1 (v side) weights, bn1 biases, then out_att.a."""

    @staticmethod
    def forward(ctx, u, v, W, graph: Graph, bns, training, eps, momentum, slope, px, sx, pa,
                sa, *params):
        N, H, F = u.shape
        M = graph.n_cols
        dt = _table_dtype(u, v)
        u, v = _tc(u, dt), _tc(v, dt)
        a_out = params[4 * H]
        dev = u.device
        s = _stream(u)
        # fp32 views of W, the BatchNorm affine parameters and running statistics: the
        # tensors themselves when fp32, else fp32 copies made in ONE cast launch (and the
        # updated running statistics cast back in one launch after the head)
        cast_in, cast_out = [], []

        def f32_of(t):
            if t.dtype == torch.float32 and t.is_contiguous():
                return t
            c = torch.empty(t.shape, device=t.device, dtype=torch.float32)
            cast_in.append((t.contiguous(), c))
            return c

        W32 = f32_of(W)
        p32 = [f32_of(p) for p in params[:4 * H]]  # held until the launches (see bn_lrelu)
        run = {}
        for side, k in (("u", 0), ("v", 1)):
            rm, rv = [], []
            for bu_bv in bns:
                bn = bu_bv[k]
                if training and bn.track_running_stats and bn.running_mean is not None:
                    for buf, lst in ((bn.running_mean, rm), (bn.running_var, rv)):
                        b32 = f32_of(buf)
                        if b32 is not buf:
                            cast_out.append((b32, buf))
                        lst.append(b32)
                elif not training:
                    rm.append(f32_of(bn.running_mean))
                    rv.append(f32_of(bn.running_var))
                else:
                    rm.append(None)
                    rv.append(None)
            run[side] = (rm, rv)
        _cast_many(cast_in, s)
        ptr = lambda lst: [_lib.ptr(t) for t in lst]  # noqa: E731
        hp = _head_params(H, F, eps, momentum, slope, {
            "u_weight": ptr(p32[0:H]), "u_bias": ptr(p32[H:2 * H]),
            "u_running_mean": ptr(run["u"][0]), "u_running_var": ptr(run["u"][1]),
            "v_weight": ptr(p32[2 * H:3 * H]), "v_bias": ptr(p32[3 * H:4 * H]),
            "v_running_mean": ptr(run["v"][0]), "v_running_var": ptr(run["v"][1]),
            # the kernel advances the BatchNorms' step counters (nn.BatchNorm1d's +1)
            "num_batches_tracked": [
                _lib.ptr(bn.num_batches_tracked)
                if training and bn.track_running_stats and bn.num_batches_tracked is not None
                and bn.num_batches_tracked.is_cuda else None
                for pair in bns for bn in pair]})
        stats = torch.empty(4 * H * F + H * F * M, device=dev, dtype=torch.float32)
        out = torch.empty(N, M, device=dev, dtype=dt)
        g = graph.desc
        ws = _workspace(dev, _memo(graph, ("head_ws", H, F), lambda: int(
            _lib.fn("msha_head_workspace_size")(g, H, F))) if training else 0)
        _lib.call("msha_head_fwd", g, C_byref(hp), _code(dt), u.data_ptr(), v.data_ptr(),
                  W32.data_ptr(), int(training), px, sx, pa, sa, stats.data_ptr(),
                  out.data_ptr(), ws.data_ptr(), ws.numel(), s)
        if HEAD_TAPS is not None:  # tests: the statistics that decide the LeakyReLU branches
            HEAD_TAPS.append({"u": u.detach().clone(), "v": v.detach().clone(),
                              "stats": stats.detach().clone(),
                              "params": [p.detach().clone() for p in p32]})
        _cast_many(cast_out, s)  # non-fp32 running buffers: write the update back
        ctx.graph, ctx.hpar = graph, (H, F, eps, momentum, slope)
        ctx.drop = (px, sx, pa, sa)
        ctx.pdtypes = [p.dtype for p in params[:4 * H]]
        ctx.wdtype = W.dtype
        ctx.a_meta = (a_out.shape, a_out.dtype, a_out.device)
        ctx.save_for_backward(u, v, W32, stats, *p32)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, v, W32, stats, *p32 = ctx.saved_tensors
        H, F, eps, momentum, slope = ctx.hpar
        px, sx, pa, sa = ctx.drop
        graph = ctx.graph
        dev = u.device
        dt = u.dtype
        dout = _tc(dout, dt)
        flags = getattr(dout, "_msha_rowflags", None)  # from _NllRows.backward, if dout is its d
        if flags is not None and (flags[1] != dout.shape[0] or not dout.is_contiguous()):
            flags = None
        du = torch.empty_like(u)
        dv = torch.empty_like(v)
        dW = torch.empty_like(W32)
        dp = torch.empty(4, H, F, device=dev, dtype=torch.float32)
        ptr = lambda lst: [_lib.ptr(t) for t in lst]  # noqa: E731
        base = dp.data_ptr()
        step = 4 * F  # dp (4, H, F): gradient k of head h at base + 4 (k H + h) F
        hp = _head_params(H, F, eps, momentum, slope, {
            "u_weight": ptr(p32[0:H]), "u_bias": ptr(p32[H:2 * H]),
            "v_weight": ptr(p32[2 * H:3 * H]), "v_bias": ptr(p32[3 * H:4 * H]),
            "u_running_mean": None, "u_running_var": None, "v_running_mean": None,
            "v_running_var": None}, dyn={
            name: [base + step * (k * H + h) for h in range(H)]
            for k, name in enumerate(("du_weight", "du_bias", "dv_weight", "dv_bias"))})
        g = graph.desc
        ws = _workspace(dev, _memo(graph, ("head_ws", H, F), lambda: int(
            _lib.fn("msha_head_workspace_size")(g, H, F))))
        shape, adt, adev = ctx.a_meta
        da = torch.empty(shape, dtype=torch.float32, device=adev)  # zeroed by the reduce
        if flags is not None:
            fl, n = flags
            nw = (n + 63) // 64
            HEAD_BWD_FLAGGED[0] += 1
            _lib.call("msha_head_bwd_flagged", g, C_byref(hp), _code(dt), u.data_ptr(),
                      v.data_ptr(), W32.data_ptr(), px, sx, pa, sa, stats.data_ptr(),
                      dout.data_ptr(), fl.data_ptr() + 8 * nw, fl.data_ptr(), du.data_ptr(),
                      dv.data_ptr(), dW.data_ptr(), da.data_ptr(), da.numel(), ws.data_ptr(),
                      ws.numel(), _stream(u))
        else:
            _lib.call("msha_head_bwd", g, C_byref(hp), _code(dt), u.data_ptr(), v.data_ptr(),
                      W32.data_ptr(), px, sx, pa, sa, stats.data_ptr(), dout.data_ptr(),
                      du.data_ptr(), dv.data_ptr(), dW.data_ptr(), da.data_ptr(), da.numel(),
                      ws.data_ptr(), ws.numel(), _stream(u))
        # gradients in the parameters' dtypes: one cast launch for every non-fp32 one
        casts = []

        def as_dtype(g, dtype):
            if g.dtype == dtype:
                return g
            c = torch.empty(g.shape, device=g.device, dtype=dtype)
            casts.append((g, c))
            return c

        grads = [as_dtype(dp[k, h], ctx.pdtypes[k * H + h]) for k in range(4) for h in range(H)]
        dW, da = as_dtype(dW, ctx.wdtype), as_dtype(da, adt)
        _cast_many(casts, _stream(u))
        return (du, dv, dW, None, None, None, None, None, None, None, None, None,
                None, *grads, da)


def C_byref(x):
    import ctypes

    return ctypes.byref(x)


def model_head(graph: Graph, u, v, bns, out_W, out_a, p: float = 0.0, training: bool = False,
               slope: float = 0.2):
    """log_softmax(elu(out_att(dropout(cat_h elu(lrelu(bn2_h(u_h)) @ lrelu(bn1_h(v_h)).T)))))
    for the (N, H, F) / (M, H, F) attention aggregates u, v; ``bns``: per head (bn2, bn1)
    BatchNorm1d modules (u side, v side).  Training: batch statistics (running
    statistics and num_batches_tracked advanced as nn.BatchNorm1d), dropout p on x and on
    the out_att attention; eval: running statistics."""
    _lib.require_cuda(u, v, out_W)
    N, H, F = u.shape
    bn0 = bns[0][0]
    params = ([b[0].weight for b in bns] + [b[0].bias for b in bns] + [b[1].weight for b in bns]
              + [b[1].bias for b in bns] + [out_a])
    if not training:
        # msha_head_bwd differentiates the training-mode BatchNorm (batch statistics);
        # eval normalises with the running statistics, whose backward it does not have
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                           for t in (u, v, out_W, *params)):
            raise NotImplementedError(
                "model_head: gradients through eval-mode BatchNorm (running statistics) are "
                "not implemented; call it under torch.no_grad() or use the unfused tail")
        if any(bn.running_mean is None or bn.running_var is None for pair in bns for bn in pair):
            raise ValueError("model_head: eval needs running statistics "
                             "(BatchNorm1d(track_running_stats=True))")
    px = pa = float(p) if training else 0.0
    sx = new_seed() if px > 0 else 0
    sa = new_seed() if pa > 0 else 0
    return _ModelHead.apply(u, v, out_W, graph, bns, bool(training), float(bn0.eps),
                            float(bn0.momentum), float(slope), px, sx, pa, sa, *params)


# ------------------------------------------------- parameter packing / feature dropout ---
_SEG_FMT = struct.Struct("<QQQqqqqqf4xQQii")  # struct msha_segment (checked at import)
assert _SEG_FMT.size == ctypes.sizeof(_lib.MshaSegment)


def _segments(segs, stream):
    """msha_segments launches: segs = [(a, dst, rows, cols, lda, ldd, b, ldb, p, seed
    [, a_dtype, dst_dtype])] (pointers as ints, a / b may be None; dtypes as torch dtypes,
    fp32 when omitted), MSHA_MAX_SEGMENTS per launch.  The records are packed bytes
    (one struct.pack_into each) viewed as the ctypes array."""
    for lo in range(0, len(segs), _lib.MAX_SEGMENTS):
        part = segs[lo:lo + _lib.MAX_SEGMENTS]
        buf = bytearray(_SEG_FMT.size * len(part))
        for k, sg in enumerate(part):
            a, dst, rows, cols, lda, ldd, b, ldb, p, seed = sg[:10]
            adt, ddt = (sg[10], sg[11]) if len(sg) > 10 else (torch.float32, torch.float32)
            _SEG_FMT.pack_into(buf, k * _SEG_FMT.size, a or 0, b or 0, dst, rows, cols, lda,
                               ldb, ldd, p, seed, 0, 1 if adt == BF16 else 0,
                               1 if ddt == BF16 else 0)
        arr = (_lib.MshaSegment * len(part)).from_buffer(buf)
        _lib.call("msha_segments", len(part), C_byref(arr), stream)


def _cast_segs(pairs):
    """Segments writing dst = src (cast to dst's dtype) for contiguous same-numel pairs."""
    return [(a.data_ptr(), d.data_ptr(), 1, a.numel(), a.numel(), a.numel(), None, 0, 0.0, 0,
             a.dtype, d.dtype) for a, d in pairs if a.numel() > 0]


def _cast_many(pairs, stream):
    """Every (src, dst) pair of contiguous same-numel tensors copied with a dtype cast in
    one launch (the bf16 models' small parameters, gradients and BatchNorm buffers: one
    launch where ``.to(dtype)`` issued one per tensor)."""
    segs = _cast_segs(pairs)
    if segs:
        _segments(segs, stream)


def _fd_fwd(S, R, p, s_seed, r_seed):
    """Segments + outputs of dropout(S), dropout(R) (one Philox mask each)."""
    S, R = S.contiguous(), R.contiguous()
    So, Ro = torch.empty_like(S), torch.empty_like(R)
    segs = [(S.data_ptr(), So.data_ptr(), S.shape[0], S.shape[1], S.shape[1], S.shape[1],
             None, 0, p, s_seed, S.dtype, S.dtype),
            (R.data_ptr(), Ro.data_ptr(), R.shape[0], R.shape[1], R.shape[1], R.shape[1],
             None, 0, p, r_seed, R.dtype, R.dtype)]
    return segs, So, Ro


def _fd_bwd(leaves, grads, p, seeds, needs):
    """Segments + gradients of the two feature dropouts (the masks regenerated).  A leaf
    registered with ``optim.Adam.fuse_dropout_grad`` gets no gradient: its optimizer step
    reads the output gradient and the mask seed instead."""
    from .optim import fused_optimizer_of

    segs, outs = [], []
    for k, (d, seed) in enumerate(zip(grads, seeds)):
        leaf = leaves[k]
        opt = fused_optimizer_of(leaf) if d is not None else None
        if opt is not None and needs[k]:
            opt.stash_dropout_grad(leaf, d, p, seed)
            d = None
        if d is None:
            outs.append(None)
            continue
        d = d.contiguous()
        g = torch.empty_like(d)
        segs.append((d.data_ptr(), g.data_ptr(), d.shape[0], d.shape[1], d.shape[1],
                     d.shape[1], None, 0, p, seed, d.dtype, d.dtype))
        outs.append(g)
    return segs, outs


class _FeatureDropout(torch.autograd.Function):
    """dropout(Sfeatures), dropout(Rfeatures) (Ablation.py:296-297, Ours.py:161-162) in one
    launch; the backward regenerates both Philox masks in one launch.  A table registered
    with ``optim.Adam.fuse_dropout_grad`` gets no gradient: the backward hands the
    dropout's output gradient and mask seed to that optimizer, whose step reads them."""

    @staticmethod
    def forward(ctx, S, R, p, s_seed, r_seed):
        ctx.params = (S, R)  # the leaves themselves (a fused optimizer updates them)
        segs, So, Ro = _fd_fwd(S, R, p, s_seed, r_seed)
        _segments(segs, _stream(S))
        ctx.p, ctx.seeds = p, (s_seed, r_seed)
        return So, Ro

    @staticmethod
    def backward(ctx, dSo, dRo):
        segs, outs = _fd_bwd(ctx.params, (dSo, dRo), ctx.p, ctx.seeds, ctx.needs_input_grad)
        if segs:
            _segments(segs, _stream(outs[0] if outs[0] is not None else outs[1]))
        return outs[0], outs[1], None, None, None


def feature_dropout(S, R, p: float, training: bool):
    """(dropout(S, p), dropout(R, p)) for the models' two feature tables: one launch each
    way for fp32 / bf16 tables (Philox masks, seeds from torch's CPU generator; bf16
    outputs rounded once from the fp32 product), F.dropout otherwise."""
    if not training or p <= 0:
        return S, R
    if not _fd_ok(S, R):
        return (torch.nn.functional.dropout(S, p, training=True),
                torch.nn.functional.dropout(R, p, training=True))
    _lib.require_cuda(S, R)
    return _FeatureDropout.apply(S, R, float(p), new_seed(), new_seed())


def _fd_ok(S, R):
    ok = (torch.float32, BF16)
    return S.dtype in ok and R.dtype in ok and S.dim() == 2 and R.dim() == 2


def _ph_fwd(H, intra, params):
    """Segments + outputs of the head packing: W1 / W2 (K, H*F) in the parameters' dtype,
    a_r / a_l (H, F) fp32 [, a3s, a4s = a3[:F] + a3[F:], a4[:F] + a4[F:]]."""
    W1s, W2s, As = params[:H], params[H:2 * H], params[2 * H:3 * H]
    K, Fd = W1s[0].shape
    dev = W1s[0].device
    pdt = W1s[0].dtype
    es = W1s[0].element_size()
    W1 = torch.empty(K, H * Fd, device=dev, dtype=pdt)
    W2 = torch.empty(K, H * Fd, device=dev, dtype=pdt)
    ar = torch.empty(H, Fd, device=dev)
    al = torch.empty(H, Fd, device=dev)
    outs = [W1, W2, ar, al]
    f32 = torch.float32
    segs = []
    w1p, w2p, arp, alp = W1.data_ptr(), W2.data_ptr(), ar.data_ptr(), al.data_ptr()
    for h in range(H):
        segs.append((W1s[h].data_ptr(), w1p + es * h * Fd, K, Fd, Fd, H * Fd, None, 0, 0.0, 0,
                     pdt, pdt))
        segs.append((W2s[h].data_ptr(), w2p + es * h * Fd, K, Fd, Fd, H * Fd, None, 0, 0.0, 0,
                     pdt, pdt))
        pa = As[h].data_ptr()
        segs.append((pa, arp + 4 * h * Fd, 1, Fd, Fd, Fd, None, 0, 0.0, 0, pdt, f32))
        segs.append((pa + es * Fd, alp + 4 * h * Fd, 1, Fd, Fd, Fd, None, 0, 0.0, 0, pdt, f32))
    if intra:
        a3s = torch.empty(H, Fd, device=dev)
        a4s = torch.empty(H, Fd, device=dev)
        outs += [a3s, a4s]
        for h in range(H):
            for src, dst in ((params[3 * H + h], a3s), (params[4 * H + h], a4s)):
                pa = src.data_ptr()
                segs.append((pa, dst.data_ptr() + 4 * h * Fd, 1, Fd, Fd, Fd, pa + es * Fd, Fd,
                             0.0, 0, pdt, f32))
    return segs, outs, (H, intra, K, Fd, pdt)


def _ph_bwd(meta, dW1, dW2, dar, dal, da3s=None, da4s=None):
    """Segments + per-head parameter gradients of the head packing (cast to the
    parameters' dtype); a missing packed gradient writes zeros."""
    H, intra, K, Fd, pdt = meta
    some = next(t for t in (dW1, dW2, dar, dal, da3s, da4s) if t is not None)
    dev = some.device
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    dW1, dW2, dar, dal, da3s, da4s = map(c, (dW1, dW2, dar, dal, da3s, da4s))
    # a missing gradient writes zeros (NULL a); its dtype code is then irrelevant
    dty = lambda t: pdt if t is None else t.dtype  # noqa: E731
    ptr = lambda t, off=0: None if t is None else t.data_ptr() + off * t.element_size()  # noqa: E731
    gW1 = [torch.empty(K, Fd, device=dev, dtype=pdt) for _ in range(H)]
    gW2 = [torch.empty(K, Fd, device=dev, dtype=pdt) for _ in range(H)]
    gA = [torch.empty(2 * Fd, 1, device=dev, dtype=pdt) for _ in range(H)]
    ge = gA[0].element_size()
    segs = []
    for h in range(H):
        o = h * Fd
        segs.append((ptr(dW1, o), gW1[h].data_ptr(), K, Fd, H * Fd, Fd, None, 0, 0.0, 0,
                     dty(dW1), pdt))
        segs.append((ptr(dW2, o), gW2[h].data_ptr(), K, Fd, H * Fd, Fd, None, 0, 0.0, 0,
                     dty(dW2), pdt))
        segs.append((ptr(dar, o), gA[h].data_ptr(), 1, Fd, Fd, Fd, None, 0, 0.0, 0,
                     dty(dar), pdt))
        segs.append((ptr(dal, o), gA[h].data_ptr() + ge * Fd, 1, Fd, Fd, Fd, None, 0, 0.0, 0,
                     dty(dal), pdt))
    g3 = g4 = []
    if intra:
        g3 = [torch.empty(2 * Fd, 1, device=dev, dtype=pdt) for _ in range(H)]
        g4 = [torch.empty(2 * Fd, 1, device=dev, dtype=pdt) for _ in range(H)]
        for h in range(H):
            o = h * Fd
            for d, g in ((da3s, g3[h]), (da4s, g4[h])):  # sum backward: both halves
                segs.append((ptr(d, o), g.data_ptr(), 1, Fd, Fd, Fd, None, 0, 0.0, 0,
                             dty(d), pdt))
                segs.append((ptr(d, o), g.data_ptr() + ge * Fd, 1, Fd, Fd, Fd, None, 0, 0.0,
                             0, dty(d), pdt))
    return segs, [*gW1, *gW2, *gA, *g3, *g4], dev


class _PackHeads(torch.autograd.Function):
    """The heads' parameters as the fused launches read them (Ablation.py:262-267,
    Ours.py:58-75): W1 / W2 concatenated along features (K, H*F) in the parameters'
    dtype, the score vector halves a[:F] (recipient side) / a[F:] (source side) as fp32
    (H, F), and for the full MSHA layer a3[:F] + a3[F:], a4[:F] + a4[F:] -- one launch;
    the backward scatters the packed gradients to every head's parameters (cast to their
    dtype) in one launch.  fp32 or bf16 parameters (the scores are fp32 either way)."""

    @staticmethod
    def forward(ctx, H, intra, *params):
        segs, outs, ctx.meta = _ph_fwd(H, intra, params)
        _segments(segs, _stream(outs[0]))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        segs, gs, dev = _ph_bwd(ctx.meta, *grads)
        _segments(segs, _lib.stream_handle(dev))
        return (None, None, *gs)


def _pack_params(heads, intra):
    names = ["W1", "W2", "a"] + (["a3", "a4"] if intra else [])
    return [getattr(h, n) for n in names for h in heads]


def _ph_ok(H, params):
    pdt = params[0].dtype
    return H <= 4 and pdt in (torch.float32, BF16) and all(
        p.dtype == pdt and p.is_contiguous() and p.is_cuda for p in params)


def pack_heads(heads, intra: bool):
    """(W1 (K, H*F), W2, a_r (H, F), a_l (H, F)[, a3s, a4s]) of the heads' parameters, or
    None when the one-launch packing does not apply (mixed or non-fp32/bf16 dtypes,
    non-contiguous parameters, more than 4 heads)."""
    H = len(heads)
    params = _pack_params(heads, intra)
    if not _ph_ok(H, params):
        return None
    return _PackHeads.apply(H, intra, *params)


class _Prologue(torch.autograd.Function):
    """feature_dropout + pack_heads as ONE launch each way (and one autograd node): the
    models' step starts with both (Ablation.py:296-297 + :262-267, Ours.py:161-162 +
    :58-75) and their segments fit one msha_segments batch."""

    @staticmethod
    def forward(ctx, p, s_seed, r_seed, H, intra, S, R, *params):
        ctx.leaves = (S, R)
        fsegs, So, Ro = _fd_fwd(S, R, p, s_seed, r_seed)
        psegs, outs, ctx.meta = _ph_fwd(H, intra, params)
        _segments(fsegs + psegs, _stream(So))
        ctx.p, ctx.seeds = p, (s_seed, r_seed)
        return (So, Ro, *outs)

    @staticmethod
    def backward(ctx, dSo, dRo, *dpacked):
        fsegs, fouts = _fd_bwd(ctx.leaves, (dSo, dRo), ctx.p, ctx.seeds,
                               ctx.needs_input_grad[5:7])
        if any(d is not None for d in dpacked):
            psegs, gs, dev = _ph_bwd(ctx.meta, *dpacked)
        else:
            psegs, gs = [], [None] * (len(ctx.needs_input_grad) - 7)
        if fsegs or psegs:
            dev = next(t for t in (*fouts, *gs) if t is not None).device
            _segments(fsegs + psegs, _lib.stream_handle(dev))
        return (None, None, None, None, None, fouts[0], fouts[1], *gs)


def model_prologue(S, R, p: float, training: bool, heads, intra: bool):
    """(dropout(S), dropout(R), packed heads) -- feature_dropout and pack_heads in one
    launch each way when both apply (training with dropout, packable heads); otherwise
    the two separately (packed None where pack_heads does not apply)."""
    H = len(heads)
    params = _pack_params(heads, intra)
    if training and p > 0 and _fd_ok(S, R) and _ph_ok(H, params):
        _lib.require_cuda(S, R)
        outs = _Prologue.apply(float(p), new_seed(), new_seed(), H, intra, S, R, *params)
        return outs[0], outs[1], tuple(outs[2:])
    s_in, r_in = feature_dropout(S, R, p, training)
    return s_in, r_in, pack_heads(heads, intra)


# ------------------------------------------------------------- loss on gathered rows ---
class _NllRows(torch.autograd.Function):
    """F.nll_loss(logp[rows], cols) (mean) and its backward, one launch each
    (msha_nll_rows_fwd / _bwd): replaces the row gather, nll forward/backward, the zero
    fill of the (N, M) gradient and the index backward of train.py:227-229."""

    @staticmethod
    def forward(ctx, logp, rows, cols):
        dt = _table_dtype(logp)
        logp = _tc(logp, dt)
        rows = rows.to(torch.int64).contiguous()
        cols = cols.to(torch.int64).contiguous()
        loss = torch.empty((), device=logp.device, dtype=torch.float32)
        _lib.call("msha_nll_rows_fwd", logp.shape[0], logp.shape[1], rows.numel(),
                  rows.data_ptr(), cols.data_ptr(), _code(dt), logp.data_ptr(), logp.stride(0),
                  loss.data_ptr(), _stream(logp))
        ctx.save_for_backward(rows, cols)
        ctx.shape, ctx.dt = tuple(logp.shape), dt
        return loss

    @staticmethod
    def backward(ctx, gloss):
        rows, cols = ctx.saved_tensors
        N, M = ctx.shape
        g = _f32c(gloss.reshape(1))
        d = torch.empty(N, M, device=rows.device, dtype=ctx.dt)
        if NLL_FLAGS:
            # the rows of d with a nonzero, flagged here for the model head's backward (its
            # consumer in every model): msha_head_bwd_flagged then skips its own row scan
            nw = (N + 63) // 64
            fl = torch.empty(8 * nw + N, device=rows.device, dtype=torch.uint8)
            _lib.call("msha_nll_rows_bwd_flags", N, M, rows.numel(), rows.data_ptr(),
                      cols.data_ptr(), g.data_ptr(), _code(ctx.dt), d.data_ptr(), M,
                      fl.data_ptr() + 8 * nw, fl.data_ptr(), _stream(d))
            d._msha_rowflags = (fl, N)
        else:
            _lib.call("msha_nll_rows_bwd", N, M, rows.numel(), rows.data_ptr(), cols.data_ptr(),
                      g.data_ptr(), _code(ctx.dt), d.data_ptr(), M, _stream(d))
        return d, None, None


def nll_loss_rows(logp, rows, cols):
    """``F.nll_loss(logp[rows].float(), cols)`` (mean reduction) for the (N, M) log-probs
    of a model head, train.py:227-229's loss, as one launch forward and one backward."""
    _lib.require_cuda(logp, rows, cols)
    if logp.dim() != 2 or rows.shape != cols.shape:
        raise ValueError("nll_loss_rows: logp (N, M), rows and cols of the same length")
    return _NllRows.apply(logp, rows, cols)
