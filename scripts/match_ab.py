"""Fused representation-matching loss against the torch composition it replaces, on the same
box ("Representation matching"):

    python scripts/match_ab.py [out.json]      (default: profiles/match_ab/match_ab.json)

A 100k x 128 student table against a teacher table of the same shape (fp32 teacher), the
student fp32 and bf16, with (a) 4M entries uniform over the table, (b) 4M entries in 32
rows, the repository's shape (a batch's source_index repeats a few sources), and (c) 4,096
uniform entries, LLP's batch:

- ``functional.link_match_loss`` forward + backward;
- ``1 - F.cosine_similarity(h[rows], t[rows].detach(), -1).mean()`` forward + backward (two
  (P, F) gathers, the normalise, and ``index_put``'s float-atomic backward).

The two are timed in alternating rounds (median of 7 rounds of HIP-event times per call
after warm-up).  Also the forward alone, the backward alone and the histogram alone
(``msha_link_match_count``) in both distributions, and for the forward the achieved
fraction of the 8 TB/s HBM peak by its byte model: 8 P index bytes, 4 n counts, the rows
that occur times both tables' row bytes, and 8 n coefficient bytes.

Every measurement runs as a child process under its own time limit; the first child that
fails ends the run.  With ``lib/libmsha_gnn_histdirect.so`` present (``build.py --variant
histdirect``: one global integer add per entry, no LDS table) the histogram is timed in
that form too.  Prints one JSON object and writes it out.
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, F, P, HOT, BATCH = 100_000, 128, 4_000_000, 32, 4096
HBM_PEAK = 8.0e12
ROUNDS = 7
STEP_LIMIT_S = 420
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DIST = ("uniform", "hot32", "batch4096")
DIRECT_LIB = os.path.join(ROOT, "msha--gnn_amd", "lib", "libmsha_gnn_histdirect.so")


def alternate_us(fns, rounds=ROUNDS, reps=3):
    """Median over ``rounds`` of the per-call time of each function, the functions taking
    turns inside every round."""
    from gemm_ab import timeit

    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timeit(fn, reps=reps, warm=2))
    return [float(np.median(t)) for t in times]


def entries(dist, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    if dist == "uniform":
        return torch.randint(0, N, (P,), device=dev, generator=g)
    if dist == "hot32":
        return torch.randint(0, HOT, (P,), device=dev, generator=g)
    return torch.randint(0, N, (BATCH,), device=dev, generator=g)


def step_case(name, dist):
    import torch.nn.functional as TF

    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    dt = DT[name]
    h = ((torch.rand(N, F, device=dev, generator=g) - 0.5) * 0.35).to(dt).requires_grad_(True)
    t = (torch.rand(N, F, device=dev, generator=g) - 0.5) * 2.0
    rows = entries(dist, dev)
    Pn = rows.numel()

    def fused():
        h.grad = None
        MF.link_match_loss(h, rows, t).backward()

    def baseline():
        h.grad = None
        (1 - TF.cosine_similarity(h[rows].float(), t[rows].detach(), dim=-1).mean()).backward()

    def fwd_only():
        with torch.no_grad():
            return MF.link_match_loss(h, rows, t)

    hd = h.detach()
    coef = torch.empty(N, 2, dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    npad = torch.empty(1, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    dH = torch.empty(N, F, dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.load().msha_link_match_fwd_workspace_size(Pn, N), dtype=torch.uint8,
                     device=dev)
    s = _lib.stream_handle(dev)
    _lib.call("msha_link_match_fwd", Pn, F, MF._code(dt), hd.data_ptr(), hd.stride(0), N, 0,
              t.data_ptr(), t.stride(0), N, rows.data_ptr(), coef.data_ptr(), None,
              count.data_ptr(), loss.data_ptr(), npad.data_ptr(), ws.data_ptr(), ws.numel(), s)
    touched = int((count > 0).sum())

    def bwd_only():
        _lib.call("msha_link_match_bwd", F, MF._code(dt), hd.data_ptr(), hd.stride(0), N, 0,
                  t.data_ptr(), t.stride(0), N, coef.data_ptr(), one.data_ptr(), dH.data_ptr(), s)

    def hist_only():
        _lib.call("msha_link_match_count", Pn, N, N, rows.data_ptr(), count.data_ptr(),
                  npad.data_ptr(), s)

    # same answer first (torch sums in another order: values differ by rounding)
    fused()
    g_f = h.grad.float().clone()
    l_f = float(fwd_only())
    baseline()
    g_b = h.grad.float()
    scale, diff = float(g_b.abs().max()), float((g_f - g_b).abs().max())
    l_b = float(1 - TF.cosine_similarity(hd[rows].float(), t[rows], dim=-1).mean())
    fused()
    again = bool(torch.equal(h.grad.float(), g_f))
    t_f, t_b = alternate_us([fused, baseline])
    t_fw, t_bw, t_h = alternate_us([fwd_only, bwd_only, hist_only], reps=5)
    esz = 4 if dt == torch.float32 else 2
    fwd_bytes = 8 * Pn + 4 * N + touched * F * (esz + 4) + 8 * N
    return {"entries": Pn, "rows_that_occur": touched,
            "link_match_fwd_bwd_us": round(t_f, 1), "torch_fwd_bwd_us": round(t_b, 1),
            "ratio_torch_over_fused": round(t_b / t_f, 3),
            "fwd_us": round(t_fw, 1), "bwd_us": round(t_bw, 1), "hist_us": round(t_h, 1),
            "row_pass_us": round(t_fw - t_h, 1), "fwd_model_bytes": fwd_bytes,
            "fwd_fraction_of_hbm_peak": round(fwd_bytes / (t_fw * 1e-6) / HBM_PEAK, 4),
            "fused_gradient_bitwise_repeatable": again, "loss_fused": l_f, "loss_torch": l_b,
            "max_abs_gradient_difference": diff, "max_abs_gradient": scale}


def step_hist():
    """The histogram alone in the loaded library's form, both distributions."""
    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib

    dev = torch.device("cuda:0")
    count = torch.empty(N, dtype=torch.int32, device=dev)
    npad = torch.empty(1, dtype=torch.int32, device=dev)
    s = _lib.stream_handle(dev)
    out = {}
    for dist in ("uniform", "hot32"):
        rows = entries(dist, dev)

        def hist():
            _lib.call("msha_link_match_count", rows.numel(), N, N, rows.data_ptr(),
                      count.data_ptr(), npad.data_ptr(), s)

        hist()
        exact = bool(torch.equal(count.long(), torch.bincount(rows, minlength=N)))
        (t_h,) = alternate_us([hist], reps=5)
        out[dist] = {"hist_us": round(t_h, 1), "equals_bincount": exact}
    return out


def child(step, env=None):
    """One measurement in a process of its own under a time limit: its last output line."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
           "--step", step]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"match_ab: step {step} ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(out_path):
    res = {"table": [N, F], "teacher": "fp32", "entries": P, "hot_rows": HOT, "batch": BATCH,
           "rounds": ROUNDS, "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for name in DT:
        for dist in DIST:
            res["cases"][f"{name}_{dist}"] = child(f"{name}:{dist}")
            print(f"{name}_{dist}", json.dumps(res["cases"][f"{name}_{dist}"]), flush=True)
    res["histogram_lds_table"] = child("hist")
    if os.path.exists(DIRECT_LIB):
        res["histogram_direct_adds"] = child("hist", dict(os.environ, MSHA_GNN_LIB=DIRECT_LIB))
    res["device"] = child("device")["device"]
    res["not_slower_in_every_case"] = all(c["ratio_torch_over_fused"] >= 1.0
                                          for c in res["cases"].values())
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step = sys.argv[2]
        if step == "hist":
            out = step_hist()
        elif step == "device":
            out = {"device": torch.cuda.get_device_name(0)}
        else:
            out = step_case(*step.split(":"))
        print(json.dumps(out), flush=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1
             else os.path.join(ROOT, "profiles", "match_ab", "match_ab.json"))
