"""The attention explanation on the device against the present way, on one box (DESIGN §4,
"Attention explanation"):

    python scripts/explain_ab.py [out.json]        (default profiles/explain_ab/explain_ab.json)

Whole explanation at the 2015 graph (39,179 x 32, 91,283 edges; two heads of 16 -> 8):

- ``new``    ``explain.attention_record`` + ``explain()``: one eval forward over all sources,
             two segment selects, the group lists by reference;
- ``dense``  the ``Record()`` loop of train.py:284-291 at batch 64 through the dense record
             path (613 forwards, each scattering the (N, M) attention and 64 rows of the two
             (N, N) matrices), then ``A == A.max(1, keepdim=True)`` + ``nonzero`` in torch on
             (N, M), (M, N) and the two (N, N).

The two take turns for 7 rounds, every measurement a child process of its own under its
own time limit (wall time between two device syncs, and the peak of torch's allocator); the
median round is quoted.  Nothing more is started after a child that was killed.

Select alone, at the 2015 graph and at the 1M x 32 ``synthetic_csr`` shape, rows and
columns, tie sets and K = 100, against torch on the dense (N, M): one child per shape, the
candidates alternating inside it as in ``rank_ab.py`` (7 rounds, HIP-event time per call).
The fraction of the 8 TB/s HBM peak is by the byte model: values, ``eid``, ids and
pointers read once, plus the outputs written.  At the 2015 graph the values are the strided
view ``attd[:, -1]`` of the two-head export (4 of every 8 bytes), as ``record.explain()``
passes them; the byte model counts the 4.  The columns are also timed at ``chunk=4096``,
the default that was rejected (``rejected_chunk_4096``).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROUNDS, K, BATCH = 7, 100, 64
HBM_PEAK = 8e12
LIMIT_S = {"new": 120, "dense": 300, "select_r15": 300, "select_1m": 300}


def _r15(dev):
    import msha_loader

    msha = msha_loader.load()
    from msha_gnn_amd import layers
    from msha_gnn_amd.data import GroupAdjacency

    z = np.load(os.path.join(ROOT, "tests", "golden", "r15_graph.npz"))
    yz = np.load(os.path.join(ROOT, "tests", "golden", "years.npz"))
    n, m = int(z["n"]), int(z["m"])
    g = msha.Graph.from_csr(z["rowptr"].astype(np.int64), z["col"].astype(np.int64), m, dev)
    torch.manual_seed(3)
    heads = [layers.OursLayer(16, 8, 0.0).to(dev).eval() for _ in range(2)]
    S, R = torch.rand(n, 16, device=dev), torch.rand(m, 16, device=dev)
    city = GroupAdjacency(torch.as_tensor(yz["2015.city"], device=dev))
    prov = GroupAdjacency(torch.as_tensor(yz["2015.prov"], device=dev))
    return g, heads, S, R, city, prov


def _dense_ties(A):
    return (A == A.max(1, keepdim=True).values).nonzero()


def whole(which):
    """One measurement of the whole explanation: {seconds, peak_bytes, lists}."""
    from msha_gnn_amd import explain, layers

    dev = torch.device("cuda:0")
    g, heads, S, R, city, prov = _r15(dev)
    n, m = g.n_rows, g.n_cols

    def new():
        ex = explain.attention_record(heads, g, city, prov, s_input=S, r_input=R).explain()
        return int(ex.inter_s.ptr[-1]) + int(ex.inter_r.ptr[-1])

    def dense():
        C3, C4 = torch.zeros(n, n, device=dev), torch.zeros(n, n, device=dev)
        with torch.no_grad():
            for b0 in range(0, n, BATCH):  # Record(), train.py:284-291
                src = torch.arange(b0, min(n, b0 + BATCH), device=dev)
                layers.fused_ours_layer(heads, S, R, g, city, prov, src, False, True, None, C3,
                                        C4)
        A = layers.record_state.Coeff12new
        found = [_dense_ties(A), _dense_ties(A.t().contiguous()), _dense_ties(C3),
                 _dense_ties(C4)]
        return int(found[0].shape[0]) + int(found[1].shape[0])

    fn = new if which == "new" else dense
    new()  # warm-up for either: the library's first calls (module load, workspaces)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    count = fn()
    torch.cuda.synchronize()
    return {"seconds": time.perf_counter() - t0, "inter_ties": count,
            "peak_bytes": int(torch.cuda.max_memory_allocated())}


def select(shape):
    """Select alone: rows / columns x ties / K = 100 against torch on the dense (N, M)."""
    import msha_loader

    msha = msha_loader.load()
    from rank_ab import alternate, stats

    from msha_gnn_amd import explain
    from msha_gnn_amd import functional as MF

    dev = torch.device("cuda:0")
    if shape == "select_r15":
        g, heads, S, R, city, prov = _r15(dev)
        # the strided view attd[:, -1] (ld = 2) that record.explain() itself passes
        att = explain.attention_record(heads, g, city, prov, s_input=S, r_input=R).att
    else:
        import bench

        rowptr, col, n, m = bench.bip_graph()
        g = msha.Graph.from_csr(rowptr, col, m, dev)
        att = None
    n, m, E = g.n_rows, g.n_cols, g.n_edges
    rows = torch.repeat_interleave(torch.arange(n, device=dev), g.deg().long())
    if att is None:  # random weights normalised per row: a degree-1 source has exactly 1.0
        att = torch.rand(E, device=dev)
        att = att / torch.zeros(n, device=dev).index_add_(0, rows, att)[rows]
    A = torch.zeros(n, m, device=dev)
    A[rows, g.col.long()] = att
    At = A.t().contiguous()
    rtol = explain.DEFAULT_RTOL
    fns = {
        "rows_ties": lambda: MF.segment_ties(g.rowptr, att, ids=g.col, rtol=rtol),
        "cols_ties": lambda: MF.segment_ties(g.colptr, att, ids=g.csc_row, eid=g.csc_eid,
                                             rtol=rtol),
        "rows_topk": lambda: MF.segment_topk(g.rowptr, att, K, ids=g.col),
        "cols_topk": lambda: MF.segment_topk(g.colptr, att, K, ids=g.csc_row, eid=g.csc_eid),
        # the rejected default: one wave per 4,096 slots of a column
        "cols_ties_chunk4096": lambda: MF.segment_ties(g.colptr, att, ids=g.csc_row,
                                                       eid=g.csc_eid, rtol=rtol, chunk=4096),
        "cols_topk_chunk4096": lambda: MF.segment_topk(g.colptr, att, K, ids=g.csc_row,
                                                       eid=g.csc_eid, chunk=4096),
        "torch_rows_ties": lambda: _dense_ties(A),
        "torch_cols_ties": lambda: _dense_ties(At),
        "torch_rows_topk": lambda: torch.topk(A, min(K, m), dim=1),
        "torch_cols_topk": lambda: torch.topk(At, min(K, n), dim=1),
    }
    t = alternate(fns)
    ties_r = int(fns["rows_ties"]().ptr[-1])
    ties_c = int(fns["cols_ties"]().ptr[-1])
    read = {"rows": 4 * E + 4 * E + 4 * (n + 1), "cols": 4 * E + 4 * E + 4 * E + 4 * (m + 1)}
    wrote = {"rows_ties": 12 * n + 4 * ties_r, "cols_ties": 12 * m + 4 * ties_c,
             "rows_topk": 12 * n * K, "cols_topk": 12 * m * K}
    out = {"shape": [n, m, E], "tied_slots": {"rows": ties_r, "cols": ties_c},
           "values_stride": int(att.stride(0)),
           "rejected_chunk_4096": {"cols_ties": stats(t["cols_ties_chunk4096"]),
                                   "cols_topk": stats(t["cols_topk_chunk4096"])}}
    for name in ("rows_ties", "cols_ties", "rows_topk", "cols_topk"):
        by = read[name[:4]] + wrote[name]
        med = float(np.median(t[name]))
        out[name] = dict(stats(t[name]), model_bytes=by,
                         fraction_of_hbm_peak=round(by / (med * 1e-6) / HBM_PEAK, 5),
                         torch_dense=stats(t["torch_" + name]),
                         ratio_torch_over_select=round(
                             float(np.median(t["torch_" + name])) / med, 2))
    return out


def child(case, limit):
    """Run one case in a process of its own; None (and the reason) if it did not finish."""
    print(f"[explain_ab] {case}", file=sys.stderr, flush=True)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case],
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, "time limit"
    if r.returncode != 0:
        return None, f"exit {r.returncode}: {r.stderr[-400:]}"
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def main(out_path):
    res = {"rounds": ROUNDS, "batch": BATCH, "k": K, "whole_r15": {"new": [], "dense": []}}
    stop = None
    for _ in range(ROUNDS):
        for case in ("new", "dense"):
            got, why = child(case, LIMIT_S[case])
            if got is None:
                stop = f"{case}: {why}"
                break
            res["whole_r15"][case].append(got)
        if stop:
            break
    for case in ("select_r15", "select_1m"):
        if stop:
            break
        got, why = child(case, LIMIT_S[case])
        if got is None:
            stop = f"{case}: {why}"
        else:
            res[case] = got
    if stop:
        res["stopped"] = stop
    w = res["whole_r15"]
    if w["new"] and w["dense"]:
        med = {k: float(np.median([x["seconds"] for x in v])) for k, v in w.items()}
        res["whole_r15_summary"] = {
            "new_median_s": round(med["new"], 4), "dense_median_s": round(med["dense"], 4),
            "ratio_dense_over_new": round(med["dense"] / med["new"], 1),
            "new_peak_bytes": max(x["peak_bytes"] for x in w["new"]),
            "dense_peak_bytes": max(x["peak_bytes"] for x in w["dense"])}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    return 1 if stop else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        import msha_loader

        msha_loader.load()
        c = sys.argv[2]
        print(json.dumps(whole(c) if c in ("new", "dense") else select(c)), flush=True)
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(
            ROOT, "profiles", "explain_ab", "explain_ab.json")))
