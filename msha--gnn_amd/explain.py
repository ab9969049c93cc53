"""The attention explanation of the reference's ``Explainer.py`` on the device.

The reference fills dense dumps first (``Record()``, train.py:284-291: 613 forwards of 64
sources at the 2015 graph into an (N, M) and two (N, N) matrices) and then walks their rows
on the host (``argwhere(row == max(row))``, Explainer.py:25-30).  Here the record stays
sparse -- the per-edge inter attention the forward exports anyway, one city and one
province scalar per source, and the group member lists -- and the explanation is a select
over the CSR rows and the CSC columns of the per-edge values
(``functional.segment_ties`` / ``segment_topk``) plus a lookup in ``Groups``:

    rec = attention_record(model, inter_adj, city_adj, province_adj)
    ex = rec.explain()                    # tie sets; explain(k=100): the K best
    dicts = find_top_k(rec, source_names, recipient_names)

Differences from the dense walk, all at values that are exactly zero:
  * a recipient without any edge gets an empty list (in the dense column every source
    ties at 0; ``empty_as_all=True`` reproduces that);
  * top-K lists hold stored edges / group members only and are filled with -1 past them
    (the dense argsort would go on with zero entries in index order);
  * a source whose city / province scalar underflowed to 0 is marked in ``all_tied``: its
    dense row is all zero and every index ties.
"""
from __future__ import annotations

import numpy as np
import torch

from . import functional as MF
from . import layers
from .graph import Graph

# Relative width of the tie band: a slot ties with its segment's maximum when
# value >= max - DEFAULT_RTOL * |max|.  The reference's attention of a degree-1 source is
# exactly 1.0; the forward kernels form it as exp2(fma(x, log2e, -l2)), which could land an
# ulp off.  Measured on the MI355X over the degree-1 rows of the 2015 graph, under each of
# the six forward kernels that export the attention (bip3 / bip2 / bip and the three of
# msha_edge_attention_fwd, each forced at that graph and identified from a trace; fp32 and
# bf16 tables, scores up to 110): the worst |att - 1| is 0, every such row is exactly 1.0
# (scripts/explain_rtol.py).
# The rule -- the next power of two at or above 4x the worst value -- is therefore applied
# to the resolution of that measurement, one ulp below 1.0 (2^-24): a band of four ulps,
# far under the smallest relative gap between a best and a second-best value in the
# reference's own dump (9.37e-5) and under the 2e-5 bound the band must respect.
DEFAULT_RTOL = 2.0 ** -22


class GroupAttention:
    """City or province explanation: source i's list is the sorted member list of its
    group (the intra attention row is constant on the group, Ours.py:71-75), cut to the
    first ``k`` with ``k``; where ``all_tied[i]`` (the scalar underflowed to 0) the dense
    row is all zero and the list is every index."""

    def __init__(self, gid, ptr, members, all_tied, k=None):
        self.gid, self.ptr, self.members, self.all_tied, self.k = gid, ptr, members, all_tied, k

    def lists(self):
        gid, ptr = self.gid.cpu().numpy(), self.ptr.cpu().numpy()
        mem, tied = self.members.cpu().numpy(), self.all_tied.cpu().numpy()
        n = len(gid)
        everyone = np.arange(n, dtype=mem.dtype)
        out = []
        for i in range(n):
            row = everyone if tied[i] else mem[ptr[gid[i]]:ptr[gid[i] + 1]]
            out.append(row if self.k is None else row[: self.k])
        return out


class Explanation:
    """``inter_s`` (per source, its recipients), ``inter_r`` (per recipient, its sources):
    ``functional.Ragged`` tie sets, or (values, indices) with ``k``; ``city`` /
    ``province``: ``GroupAttention``.  ``lists()`` brings the four to the host."""

    def __init__(self, inter_s, inter_r, city, province, k, n_rows, empty_as_all):
        self.inter_s, self.inter_r, self.city, self.province = inter_s, inter_r, city, province
        self.k, self._n_rows, self._empty_as_all = k, n_rows, empty_as_all

    def _inter(self, sel, empty_len):
        if self.k is None:
            rows = sel.lists()
            if empty_len is not None:
                rows = [r if len(r) else np.arange(empty_len, dtype=r.dtype) for r in rows]
            return rows
        idx = sel[1].cpu().numpy()
        return [r[r >= 0] for r in idx]

    def lists(self):
        """{'inter_s', 'inter_r', 'city', 'province'}: lists of index arrays (one sync)."""
        return {"inter_s": self._inter(self.inter_s, None),
                "inter_r": self._inter(self.inter_r,
                                       self._n_rows if self._empty_as_all else None),
                "city": self.city.lists(), "province": self.province.lists()}


class AttentionRecord:
    """The sparse attention record: ``graph`` (CSR + CSC), ``attd`` (E, H) the per-edge
    inter attention in CSR order and ``att`` the chosen head's column of it (a view),
    ``c3`` / ``c4`` (N) the city / province attention of each source, ``groups``."""

    def __init__(self, graph: Graph, attd, head, c3, c4, groups):
        self.graph, self.attd, self.head, self.c3, self.c4, self.groups = (graph, attd, head,
                                                                          c3, c4, groups)
        self.att = attd[: graph.n_edges, head]

    def explain(self, k=None, rtol: float = DEFAULT_RTOL, empty_as_all: bool = False,
                chunk=None) -> Explanation:
        """Tie sets (``k`` None: the slots within ``rtol`` of their segment's maximum) or
        the ``k`` best of every source's recipients and every recipient's sources, and the
        group lists.  No host sync."""
        g = self.graph
        if not g.has_csc:
            raise ValueError("explain needs the graph's CSC view")
        if k is None:
            inter_s = MF.segment_ties(g.rowptr, self.att, ids=g.col, rtol=rtol, chunk=chunk)
            inter_r = MF.segment_ties(g.colptr, self.att, ids=g.csc_row, eid=g.csc_eid,
                                      rtol=rtol, chunk=chunk)
        else:
            inter_s = MF.segment_topk(g.rowptr, self.att, k, ids=g.col, chunk=chunk)
            inter_r = MF.segment_topk(g.colptr, self.att, k, ids=g.csc_row, eid=g.csc_eid,
                                      chunk=chunk)
        (g3, p3, m3), (g4, p4, m4) = self.groups._keep
        city = GroupAttention(g3, p3, m3, self.c3 == 0, k)
        province = GroupAttention(g4, p4, m4, self.c4 == 0, k)
        return Explanation(inter_s, inter_r, city, province, k, g.n_rows, empty_as_all)


def attention_record(model_or_layers, inter_adj, city_adj, province_adj, head: int = -1,
                     batch=None, s_input=None, r_input=None) -> AttentionRecord:
    """The eval-mode forward (no dropout, no gradient) of an ``Ours`` model, or of an
    ``OursLayer`` / a list of them on ``s_input`` / ``r_input``, over ALL sources, kept as
    the sparse record; no dense (N, M) or (N, N) tensor is built.  ``head``: which head's
    attention to keep (-1: the last, what the reference's dump is left with, Ours.py:92-96).
    ``batch``: sources per intra pass (None: all at once); each pass repeats the inter
    attention, whose first export is kept, and ``c3`` / ``c4`` do not depend on it."""
    if isinstance(model_or_layers, layers.Ours):
        heads = list(model_or_layers.attentions)
        s_input, r_input = model_or_layers.Sfeatures, model_or_layers.Rfeatures
    else:
        heads = ([model_or_layers] if isinstance(model_or_layers, layers.OursLayer)
                 else list(model_or_layers))
        if s_input is None or r_input is None:
            raise ValueError("attention_record: layers need s_input and r_input")
    H = len(heads)
    if not -H <= head < H:
        raise IndexError(f"head {head} of {H}")
    head %= H
    graph = layers._graph(inter_adj)
    n = graph.n_rows
    step = n if batch is None else int(batch)
    if step < 1:
        raise ValueError("batch must be positive")
    dev = s_input.device
    c3 = torch.empty(n, dtype=torch.float32, device=dev)
    c4 = torch.empty(n, dtype=torch.float32, device=dev)
    attd = groups = None
    with torch.no_grad():
        s_in, r_in = s_input.detach(), r_input.detach()
        packed = MF.pack_heads(heads, intra=True)
        for b0 in range(0, n, step):
            src = torch.arange(b0, min(n, b0 + step), device=dev)
            _, _, a, bstat, groups, _ = layers._attention_aux(heads, s_in, r_in, graph, city_adj,
                                                              province_adj, src, False, packed)
            if attd is None:
                attd = a
            c3[b0:b0 + step] = bstat[: src.numel(), head, 5]
            c4[b0:b0 + step] = bstat[: src.numel(), head, 6]
    return AttentionRecord(graph, attd, head, c3, c4, groups)


def find_top_k(record: AttentionRecord, source_names=None, recipient_names=None, k=None,
               rtol: float = DEFAULT_RTOL, empty_as_all: bool = False):
    """The four dicts of Explainer.py:39-74 -- ``InterAttS`` (source -> recipients),
    ``InterAttR`` (recipient -> sources), ``CityAtt`` and ``ProvinceAtt`` (source ->
    sources) -- keyed by index, with entries as indices or, given ``source_names`` /
    ``recipient_names`` (index -> name: a sequence or a dict, string keys as in the
    reference's json accepted), as names."""
    ls = record.explain(k=k, rtol=rtol, empty_as_all=empty_as_all).lists()

    def name(names, j):
        if names is None:
            return int(j)
        if isinstance(names, dict):
            return names[int(j)] if int(j) in names else names[str(int(j))]
        return names[int(j)]

    def table(rows, names):
        return {i: [name(names, j) for j in row] for i, row in enumerate(rows)}

    return {"InterAttS": table(ls["inter_s"], recipient_names),
            "InterAttR": table(ls["inter_r"], source_names),
            "CityAtt": table(ls["city"], source_names),
            "ProvinceAtt": table(ls["province"], source_names)}
