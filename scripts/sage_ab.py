"""``functional.sage_forward`` (the GraphSAGE baseline of SGAE.py:41-56 on sparse adjacency
rows) against the torch composition it replaces, on the same box ("GraphSAGE
baseline"):

    python scripts/sage_ab.py [out.json]   (default: profiles/sage_ab/sage_ab.json)

(a) ``r15_b512``: the shipped 2015 graph at SGAE.py's defaults, 32 / 32 / 32 and a batch of
512; (b) ``bip1m_b65536``: a synthetic 1M x 32 adjacency with the 2015 degree law
(bench.bip_graph) at a batch of 65,536.  Adjacency values are edge counts of 1 normalised by
``normalize_adjacency_matrix``; sources uniform over the rows; upstream gradient of
``F.nll_loss``.

- ``sage_forward`` forward + backward (gradients to the table and the four parameters);
- ``log_softmax(relu(linear2(adj[src] * relu(linear1(table[src])))))`` forward + backward in
  torch (a dense ``adj[src]`` gather, two dense products, ``index_put``'s backward).

The two are timed in alternating rounds (median of 7 rounds of HIP-event times per call after
warm-up; the spread of the rounds is reported).  Also, through the ABI: the forward launch;
the backward with no gradient asked for (the row pass alone), with the weight gradients, with
the table gradient, and whole; and the incidence plan on its own -- the weight-gradient and
table-pass times are differences of those.  Each with the achieved fraction of the 8 TB/s HBM
peak by its byte model.

Every configuration runs as a child process under its own time limit; the first child that
fails ends the run.  Prints one JSON object and writes it out.
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

SHAPES = {"r15_b512": 512, "bip1m_b65536": 65536}
WIDTHS = (32, 32, 32)
HBM_PEAK = 8.0e12
ROUNDS = 7
STEP_LIMIT_S = 420
RESOLUTION_US = 5.0


def rounds_us(fns, rounds=ROUNDS, reps=5):
    """Per function: (median, min, max) over ``rounds`` of the per-call time, the functions
    taking turns inside every round."""
    from gemm_ab import timeit

    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timeit(fn, reps=reps, warm=2))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def step_case(shape):
    import torch.nn.functional as TF

    import bench
    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import graph_of, normalize_adjacency_matrix

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    B = SHAPES[shape]
    in_f, M, out = WIDTHS
    rowptr, col, n, m = bench.r15_graph() if shape.startswith("r15") else bench.bip_graph()
    assert m == M
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    counts = torch.zeros(n, m, device=dev)
    counts[torch.as_tensor(rows, device=dev), torch.as_tensor(col, device=dev)] = 1.0
    counts[:m, :m] += torch.eye(m, device=dev)  # no empty column
    adj = normalize_adjacency_matrix(counts)
    del counts
    g, _ = graph_of(adj)
    vals = g.values(adj)
    table = torch.rand(n, in_f, device=dev, generator=gen).requires_grad_(True)
    l1, l2 = torch.nn.Linear(in_f, M).to(dev), torch.nn.Linear(M, out).to(dev)
    leaves = (table, l1.weight, l1.bias, l2.weight, l2.bias)
    src = torch.randint(0, n, (B,), device=dev, generator=gen)
    target = torch.randint(0, out, (B,), device=dev, generator=gen)
    edges = int((g.deg().long()[src] * (g.rowflag[src] == 0)).sum())

    def clear():
        for x in leaves:
            x.grad = None

    def fused():
        clear()
        TF.nll_loss(MF.sage_forward(table, src, g, vals, *leaves[1:], check=False),
                    target).backward()

    def baseline():
        clear()
        x = torch.relu(l1(table[src]))
        x = torch.relu(l2(torch.mul(adj[src], x)))
        TF.nll_loss(TF.log_softmax(x, dim=1), target).backward()

    # the launches through the ABI
    lib, s = _lib.load(), _lib.stream_handle(dev)
    td = table.detach()
    W1, b1, W2, b2 = (t.detach().contiguous() for t in leaves[1:])
    logp = torch.empty(B, out, device=dev)
    dlogp = torch.zeros(B, out, device=dev)
    dlogp[torch.arange(B, device=dev), target] = -1.0 / B
    dS = torch.empty(n, in_f, device=dev)
    dW1, db1, dW2, db2 = (torch.empty_like(t) for t in (W1, b1, W2, b2))
    ws = torch.empty(lib.msha_sage_workspace_size(B, n, in_f, M, out), dtype=torch.uint8,
                     device=dev)

    def fwd_call():
        _lib.call("msha_sage_fwd", g.desc, B, src.data_ptr(), in_f, out, td.data_ptr(),
                  td.stride(0), vals.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                  b2.data_ptr(), logp.data_ptr(), s)

    def bwd_call(with_w, with_t):
        p = lambda t, on: t.data_ptr() if on else None  # noqa: E731

        def run():
            _lib.call("msha_sage_bwd", g.desc, B, src.data_ptr(), in_f, out, td.data_ptr(),
                      td.stride(0), vals.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                      W2.data_ptr(), b2.data_ptr(), logp.data_ptr(), dlogp.data_ptr(),
                      p(dS, with_t), p(dW1, with_w), p(db1, with_w), p(dW2, with_w),
                      p(db2, with_w), ws.data_ptr(), ws.numel(), s)
        return run

    # same answer first (torch sums in another order: values differ by rounding)
    fused()
    g_f = [x.grad.clone() for x in leaves]
    baseline()
    g_b = [x.grad.clone() for x in leaves]
    fused()
    again = all(bool(torch.equal(x.grad, y)) for x, y in zip(leaves, g_f))
    (t_f, f_lo, f_hi), (t_b, b_lo, b_hi) = rounds_us([fused, baseline], reps=3)
    fwd_call()
    (t_fw, _, _), (t_rows, _, _), (t_w, _, _), (t_t, _, _), (t_all, _, _), (t_plan, _, _) = \
        rounds_us([fwd_call, bwd_call(False, False), bwd_call(True, False),
                   bwd_call(False, True), bwd_call(True, True),
                   lambda: MF.pair_plan(src, src, n)])
    nblk = min(-(-B // 16), 512)  # sage.hip: rounds of 16 entries, at most 512 blocks
    plen = M * in_f + M + out * M + out
    params = 4 * plen
    model = {
        "fwd": B * (8 + 4 * in_f + 9 + 4 * out) + 8 * edges + params,
        "bwd_rows": B * (8 + 8 * in_f + 9 + 12 * out) + 16 * edges + params,
        "wgrad": B * (8 + 4 * in_f + 9 + 4 * out) + 12 * edges + 4 * plen * (2 * nblk + 1),
        "table": n * (4 + 4 * in_f) + B * (8 + 4 * in_f),
    }
    times = {"fwd": t_fw, "bwd_rows": t_rows, "wgrad": t_w - t_rows,
             "table": t_t - t_rows - t_plan}
    res = {"rows": n, "batch": B, "widths": list(WIDTHS), "batch_edges": edges,
           "sage_fwd_bwd_us": round(t_f, 1), "sage_fwd_bwd_min_max_us": [round(f_lo, 1),
                                                                       round(f_hi, 1)],
           "torch_fwd_bwd_us": round(t_b, 1), "torch_fwd_bwd_min_max_us": [round(b_lo, 1),
                                                                         round(b_hi, 1)],
           "ratio_torch_over_sage": round(t_b / t_f, 3),
           "fwd_call_us": round(t_fw, 1), "bwd_call_us": round(t_all, 1),
           "plan_build_us": round(t_plan, 1),
           "sage_gradients_bitwise_repeatable": again}
    for k in model:
        res[f"{k}_us"] = round(times[k], 1)
        res[f"{k}_model_bytes"] = model[k]
        # (a difference of medians under RESOLUTION_US is noise: no fraction is quoted)
        res[f"{k}_fraction_of_hbm_peak"] = (round(model[k] / (times[k] * 1e-6) / HBM_PEAK, 4)
                                            if times[k] >= RESOLUTION_US else None)
    for nm, a, c in zip(("dS", "dW1", "db1", "dW2", "db2"), g_f, g_b):
        res[f"max_abs_{nm}"] = float(c.abs().max())
        res[f"max_abs_{nm}_difference"] = float((a - c).abs().max())
    return res


def child(step):
    """One configuration in a process of its own under a time limit: its last output line."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
           "--step", step]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"sage_ab: step {step} ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(out_path):
    res = {"shapes": SHAPES, "rounds": ROUNDS, "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for shape in SHAPES:
        res["cases"][shape] = child(shape)
        print(shape, json.dumps(res["cases"][shape]), flush=True)
    res["device"] = child("device")["device"]
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step = sys.argv[2]
        out = ({"device": torch.cuda.get_device_name(0)} if step == "device"
               else step_case(step))
        print(json.dumps(out), flush=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1
             else os.path.join(ROOT, "profiles", "sage_ab", "sage_ab.json"))
