"""The measurement behind ``explain.DEFAULT_RTOL`` ("Attention explanation"):

    python scripts/explain_rtol.py [out.json]     (default profiles/explain_ab/degree1_rows.json)

A source with one edge has inter attention exactly 1.0 in the reference; the forward kernels
form it as ``exp2(fma(x, log2e, -l2))``.  Over the degree-1 rows of the 2015 graph this
prints max |att - 1| and the number of rows that are exactly 1.0 for each of the six
forward kernels that export the per-edge attention, each forced at that graph:

``msha_bip_attention_fwd`` (edge_bip.hip:1069-1092)
- ``bip3_fwd_kernel``  the MFMA kernels of edge_bip3.hip (2 heads of 64; default from 131,072
                       rows up, here through ``msha_bip2_bwd_min_rows(0)``);
- ``bip2_fwd_kernel``  the mask forward of edge_bip2.hip (2 heads of 64; the default here);
- ``bip_fwd_kernel``   the CSR walk of edge_bip.hip: 2 heads of 64 with ``MSHA_BIP2=0``, and
                       the shapes only it covers (1 head of 64, 2 heads of 32);

``msha_edge_attention_fwd`` (``functional.BIP`` off, and every shape the bipartite kernels do
not cover: 1 and 2 heads of 8)
- ``edge_attn_fwd_gl_kernel``   the gather-layout forward (the default for short rows);
- ``edge_attn_fwd_bat_kernel``  the batched-gather forward (``MSHA_FWD_GL=0``);
- ``edge_attn_fwd_kernel``      the plain row walk (``MSHA_FWD_BAT=0``).

Each with fp32 and bf16 tables and the projected scores as they are and scaled by 4 and by
16.  The switches are read by the library, some once per process, so every setting is a
child process of its own under its own time limit.  Which kernel ran is not inferred from
the setting: it is read from a torch.profiler trace of the first forward of every (shape,
table type), and the results are grouped by it.  The script fails if one of the six was
never seen, and starts nothing more after a child that failed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# setting -> (environment, msha_bip2_bwd_min_rows or None, functional.BIP,
#             ((in_features, heads, feat), ...))
_ALL = ((16, 1, 8), (16, 2, 8), (128, 2, 64))
SETTINGS = {
    "bip3": ({}, 0, True, ((128, 2, 64),)),
    "bip2": ({}, None, True, ((128, 2, 64),)),
    "bip": ({"MSHA_BIP2": "0"}, None, True, ((128, 2, 64), (64, 1, 64), (64, 2, 32))),
    "edge_gl": ({}, None, False, _ALL),
    "edge_bat": ({"MSHA_FWD_GL": "0"}, None, False, _ALL),
    "edge_row": ({"MSHA_FWD_BAT": "0"}, None, False, _ALL),
}
# the forward kernels that export attd (none of the names is a substring of another)
KERNELS = ("bip3_fwd_kernel", "bip2_fwd_kernel", "bip_fwd_kernel", "edge_attn_fwd_gl_kernel",
           "edge_attn_fwd_bat_kernel", "edge_attn_fwd_kernel")
LIMIT_S = 240


def _seen(prof):
    """The forward kernels of KERNELS that appear in a profiler trace."""
    return sorted({name for ev in prof.key_averages() for name in KERNELS if name in ev.key})


def setting(which):
    import msha_loader

    msha = msha_loader.load()
    from torch.profiler import ProfilerActivity, profile

    from msha_gnn_amd import _lib, layers
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.data import GroupAdjacency
    from msha_gnn_amd.graph import groups_for

    _, min_rows, bip, shapes = SETTINGS[which]
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "r15_graph.npz"))
    yz = np.load(os.path.join(ROOT, "tests", "golden", "years.npz"))
    n, m = int(z["n"]), int(z["m"])
    g = msha.Graph.from_csr(z["rowptr"].astype(np.int64), z["col"].astype(np.int64), m, dev)
    city = GroupAdjacency(torch.as_tensor(yz["2015.city"], device=dev))
    prov = GroupAdjacency(torch.as_tensor(yz["2015.prov"], device=dev))
    groups = groups_for(city, prov, dev)
    deg = np.diff(z["rowptr"])
    first = torch.as_tensor(z["rowptr"][:-1][deg == 1].astype(np.int64), device=dev)
    src = torch.arange(64, device=dev)
    runs = []
    MF.BIP = bip
    if min_rows is not None:
        _lib.fn("msha_bip2_bwd_min_rows")(min_rows)
    for fin, H, Fd in shapes:
        torch.manual_seed(5)
        heads = [layers.OursLayer(fin, Fd, 0.0).to(dev).eval() for _ in range(H)]
        S, R = torch.rand(n, fin, device=dev), torch.rand(m, fin, device=dev)
        with torch.no_grad():
            W1 = torch.cat([h.W1 for h in heads], dim=1)
            W2 = torch.cat([h.W2 for h in heads], dim=1)
            a_r, a_l = layers._score_halves(heads, "a").unbind(1)
            a3s = layers._score_halves(heads, "a3").sum(1)
            a4s = layers._score_halves(heads, "a4").sum(1)
            h1, er = MF.project_scores(R, W1, ar=a_r, heads=H)
            h2, el = MF.project_scores(S, W2, al=a_l, heads=H)
            for dt in (torch.float32, torch.bfloat16):
                t1, t2 = h1.view(m, H, Fd).to(dt), h2.view(n, H, Fd).to(dt)

                def fwd(scale):
                    return MF.ours_attention(g, groups, src, el * scale, er * scale, t1, t2,
                                             a3s, a4s, return_aux=True)[2]

                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    fwd(1.0)
                    torch.cuda.synchronize()
                seen = _seen(prof)
                for scale in (1.0, 4.0, 16.0):
                    a = fwd(scale)[first].double()
                    runs.append({
                        "setting": which, "kernels_in_trace": seen,
                        "in_features": fin, "heads": H, "feat": Fd, "scale": scale,
                        "tables": str(dt).replace("torch.", ""),
                        "worst_abs_att_minus_1": float((a - 1.0).abs().max()),
                        "exactly_one": int((a == 1.0).sum()), "values": int(a.numel()),
                        "largest_abs_el_plus_er": float((el * scale).abs().max()
                                                        + (er * scale).abs().max())})
    return {"graph": [n, m, int(len(z["col"]))], "degree1_rows": int((deg == 1).sum()),
            "runs": runs}


def main(out_path):
    res = {"settings": {k: {"environment": v[0], "bip2_bwd_min_rows": v[1], "BIP": v[2]}
                        for k, v in SETTINGS.items()}, "by_kernel": {}, "runs": []}
    stop = None
    for which, (env, _, _, _) in SETTINGS.items():
        print(f"[explain_rtol] {which}", file=sys.stderr, flush=True)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", which],
                               capture_output=True, text=True, timeout=LIMIT_S,
                               env=dict(os.environ, **env))
        except subprocess.TimeoutExpired:
            stop = f"{which}: time limit"
            break
        if r.returncode != 0:
            stop = f"{which}: exit {r.returncode}: {r.stderr[-400:]}"
            break
        got = json.loads(r.stdout.strip().splitlines()[-1])
        res["graph"], res["degree1_rows"] = got["graph"], got["degree1_rows"]
        res["runs"] += got["runs"]
    for x in res["runs"]:
        k = res["by_kernel"].setdefault("+".join(x["kernels_in_trace"]) or "none seen", {
            "runs": 0, "worst_abs_att_minus_1": 0.0, "not_exactly_one": 0, "settings": []})
        k["runs"] += 1
        k["worst_abs_att_minus_1"] = max(k["worst_abs_att_minus_1"], x["worst_abs_att_minus_1"])
        k["not_exactly_one"] += x["values"] - x["exactly_one"]
        if x["setting"] not in k["settings"]:
            k["settings"].append(x["setting"])
    res["kernels_not_seen"] = [k for k in KERNELS if k not in res["by_kernel"]]
    if stop:
        res["stopped"] = stop
    if res["runs"]:
        res["worst_over_all_runs"] = max(x["worst_abs_att_minus_1"] for x in res["runs"])
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    return 1 if stop or res["kernels_not_seen"] else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--setting":
        print(json.dumps(setting(sys.argv[2])), flush=True)
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(
            ROOT, "profiles", "explain_ab", "degree1_rows.json")))
