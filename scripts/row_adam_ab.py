"""Row-sparse table training against the dense whole-table update of the same build and
against torch's sparse-embedding path, on the same box ("Row-sparse table
training"):

    python scripts/row_adam_ab.py [out.json]  (default: profiles/row_adam_ab/row_adam_ab.json)

Each configuration times a FULL training step -- incidence plan, fused BCE loss, backward,
optimizer step -- of an (n, F) embedding table on P random pairs, three ways:

(a) ``registered``: the table registered with ``optim.Adam.fuse_row_grad``: touched-row list,
    compact gradient, lazy Adam over the touched rows;
(b) ``dense``: the same build without the registration: (n, F) gradient, whole-table Adam;
(c) ``torch``: ``F.embedding(..., sparse=True)`` gathers, the inner product,
    ``binary_cross_entropy_with_logits``, ``torch.optim.SparseAdam``.

Shapes (fp32 and bf16 tables): 100k x 128 with P = 4,096 and P = 65,536; 2M x 128 with
P = 65,536; 1M x 32 with P = 65,536; 100k x 128 with P = 4M (every row touched: nothing to
save, (a) may lose).  The three paths take turns inside every round (7 rounds of 3 steps after
2 warm-up steps, HIP events); every round's time is kept, so "every round of (a) is faster
than every round of (b)" can be read off.

After the eager figures are written, paths (a) and (b) are each captured into one HIP graph
(plan + loss + backward + step) and the replays timed the same way (``graphed_*``; 10 replays
a round): the same kernels without the host's work between the launches, in child processes
of their own.

Also the three new launches alone, through the ABI, with the achieved fraction of the 8 TB/s
HBM peak by these byte models (R touched rows, cap = min(n, 2P), esz the table's element
size):

    plan_rows       16 n + 4 cap                      tile scan of the flags, compact
    bwd_rows        2 P (20 + esz F) + 4 F cap + 12 R  endpoint scalars + gathered rows, vals
    adam_rows_step  R (4 F + 6 esz F + 4)              vals read; p, m, v read and written

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

SHAPES = {"100k_x128_p4096": (100_000, 128, 4096),
          "100k_x128_p65536": (100_000, 128, 65_536),
          "2m_x128_p65536": (2_000_000, 128, 65_536),
          "1m_x32_p65536": (1_000_000, 32, 65_536),
          "100k_x128_p4m": (100_000, 128, 4_000_000)}
CONDITION = "2m_x128_p65536"  # every round of (a) faster than every round of (b)
HBM_PEAK = 8.0e12
ROUNDS = 7
STEP_LIMIT_S = 300
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def alternate_rounds_us(fns, rounds=ROUNDS, reps=3):
    """Per-call time of each function in each round, the functions taking turns inside
    every round: a list of ``rounds`` times per function."""
    from gemm_ab import timeit

    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(float(timeit(fn, reps=reps, warm=2)))
    return times


def graph_case(name, shape):
    """Paths (a) and (b) each captured into one HIP graph (plan + loss + backward + step) and
    replayed: the same kernels without the host's work between the launches."""
    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    n, F, P = SHAPES[shape]
    h0 = ((torch.rand(n, F, device=dev, generator=g) - 0.5) * 0.6).to(DT[name])
    src = torch.randint(0, n, (P,), device=dev, generator=g)
    dst = torch.randint(0, n, (P,), device=dev, generator=g)
    y = (torch.rand(P, device=dev, generator=g) < 0.5).float()
    # a captured graph holds the addresses of its table, moments and step count, not
    # references: both models stay alive for as long as either graph is replayed
    replays, alive = [], []
    for register in (True, False):
        p = h0.clone().requires_grad_(True)
        opt = Adam([p], lr=1e-3)
        if register:
            opt.fuse_row_grad(p)

        def step(p=p, opt=opt):
            opt.zero_grad(set_to_none=True)
            MF.link_bce_loss(p, src, dst, y, plan=MF.pair_plan(src, dst, n)).backward()
            opt.step()

        step()
        step()  # warm-up outside the capture: the moments and the workspaces exist
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        replays.append(gr.replay)
        alive.append((p, opt, step, gr))
    rounds = alternate_rounds_us(replays, reps=10)
    torch.cuda.synchronize()
    del alive
    res = {}
    for nm, t in zip(("registered", "dense"), rounds):
        res[f"graphed_{nm}_step_us_rounds"] = [round(x, 1) for x in t]
        res[f"graphed_{nm}_step_us"] = round(float(np.median(t)), 1)
    res["graphed_ratio_dense_over_registered"] = round(
        res["graphed_dense_step_us"] / res["graphed_registered_step_us"], 3)
    res["graphed_every_registered_round_faster_than_every_dense_round"] = bool(
        max(rounds[0]) < min(rounds[1]))
    return res


def step_case(name, shape):
    import torch.nn.functional as TF

    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    dt = DT[name]
    n, F, P = SHAPES[shape]
    h0 = ((torch.rand(n, F, device=dev, generator=g) - 0.5) * 0.6).to(dt)
    src = torch.randint(0, n, (P,), device=dev, generator=g)
    dst = torch.randint(0, n, (P,), device=dev, generator=g)
    y = (torch.rand(P, device=dev, generator=g) < 0.5).float()

    def msha_step(register):
        p = h0.clone().requires_grad_(True)
        opt = Adam([p], lr=1e-3)
        if register:
            opt.fuse_row_grad(p)

        def step():
            opt.zero_grad(set_to_none=True)
            MF.link_bce_loss(p, src, dst, y, plan=MF.pair_plan(src, dst, n)).backward()
            opt.step()
        return p, opt, step

    pa, oa, step_a = msha_step(True)
    pb, ob, step_b = msha_step(False)
    fns, names = [step_a, step_b], ["registered", "dense"]
    res = {"rows": n, "feat": F, "pairs": P}
    try:  # torch's sparse path (a bf16 sparse gradient may not be supported: recorded then)
        pc = h0.clone().requires_grad_(True)
        oc = torch.optim.SparseAdam([pc], lr=1e-3)

        def step_c():
            oc.zero_grad(set_to_none=True)
            z = (TF.embedding(src, pc, sparse=True) * TF.embedding(dst, pc, sparse=True)).sum(-1)
            TF.binary_cross_entropy_with_logits(z.float(), y).backward()
            oc.step()

        step_c()
        torch.cuda.synchronize()
        fns.append(step_c)
        names.append("torch")
    except Exception as e:  # noqa: BLE001 - the reason goes into the result
        res["torch_unavailable"] = f"{type(e).__name__}: {e}"[:300]

    # same answer first: one step each from the same table
    step_a()
    step_b()
    plan = MF.pair_plan(src, dst, n)
    rows, n_rows = MF.plan_rows(plan)
    R = int(n_rows)
    idx = rows[:R].long()
    res["touched_rows"] = R
    res["touched_rows_bitwise_equal_after_one_step"] = bool(
        torch.equal(pa.detach()[idx].float(), pb.detach()[idx].float()))
    rounds = alternate_rounds_us(fns)
    for nm, t in zip(names, rounds):
        res[f"{nm}_step_us_rounds"] = [round(x, 1) for x in t]
        res[f"{nm}_step_us"] = round(float(np.median(t)), 1)
    res["ratio_dense_over_registered"] = round(res["dense_step_us"] / res["registered_step_us"], 3)
    if "torch_step_us" in res:
        res["ratio_torch_over_registered"] = round(
            res["torch_step_us"] / res["registered_step_us"], 3)
    res["every_registered_round_faster_than_every_dense_round"] = bool(
        max(rounds[0]) < min(rounds[1]))

    # the three new launches alone, through the ABI
    lib, s = _lib.load(), _lib.stream_handle(dev)
    hd = pa.detach()
    code, esz, cap = MF._code(dt), hd.element_size(), rows.numel()
    with torch.no_grad():
        _, z = MF.link_bce_loss(hd, src, dst, y, return_logits=True)
    one = torch.ones(1, device=dev)
    rows2, n_rows2 = torch.empty_like(rows), torch.empty_like(n_rows)
    vals = torch.empty(cap, F, dtype=torch.float32, device=dev)
    ws_r = torch.empty(lib.msha_plan_rows_workspace_size(n), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(lib.msha_link_bce_bwd_workspace_size(P, F), dtype=torch.uint8, device=dev)
    st = oa.state[pa]

    def plan_rows_call():
        _lib.call("msha_plan_rows", n, P, plan.rowptr.data_ptr(), rows2.data_ptr(),
                  n_rows2.data_ptr(), ws_r.data_ptr(), ws_r.numel(), s)

    def bwd_rows_call():
        _lib.call("msha_link_bce_bwd_rows", P, F, code, hd.data_ptr(), hd.stride(0), n,
                  src.data_ptr(), dst.data_ptr(), y.data_ptr(), None, z.data_ptr(),
                  one.data_ptr(), plan.rowptr.data_ptr(), plan.ent.data_ptr(),
                  plan.chunk_tab.data_ptr(), rows.data_ptr(), n_rows.data_ptr(), cap,
                  vals.data_ptr(), ws_b.data_ptr(), ws_b.numel(), s)

    def adam_rows_call():
        _lib.call("msha_adam_rows_step", n, F, code, hd.data_ptr(), st["exp_avg"].data_ptr(),
                  st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), rows.data_ptr(),
                  n_rows.data_ptr(), cap, vals.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, s)

    model = {"plan_rows": 16 * n + 4 * cap,
             "bwd_rows": 2 * P * (20 + esz * F) + 4 * F * cap + 12 * R,
             "adam_rows_step": R * (4 * F + 6 * esz * F + 4)}
    alone = alternate_rounds_us([plan_rows_call, bwd_rows_call, adam_rows_call], reps=10)
    for k, t in zip(model, alone):
        us = float(np.median(t))
        res[f"{k}_us"] = round(us, 1)
        res[f"{k}_model_bytes"] = model[k]
        res[f"{k}_fraction_of_hbm_peak"] = round(model[k] / (us * 1e-6) / HBM_PEAK, 4)
    return res


def child(step):
    """One configuration in a process of its own under a time limit: its last output line."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
           "--step", step]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"row_adam_ab: step {step} ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(out_path):
    res = {"shapes": {k: list(v) for k, v in SHAPES.items()}, "rounds": ROUNDS,
           "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for shape in SHAPES:
        for name in DT:
            key = f"{name}_{shape}"
            res["cases"][key] = child(f"{name}:{shape}")
            print(key, json.dumps(res["cases"][key]), flush=True)
    res["device"] = child("device")["device"]
    res["condition_shape"] = CONDITION
    res["condition_met"] = all(
        res["cases"][f"{name}_{CONDITION}"]["every_registered_round_faster_than_every_dense_round"]
        for name in DT)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    def write():
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    write()  # the eager figures stand whatever becomes of the graph legs
    for shape in SHAPES:
        for name in DT:
            key = f"{name}_{shape}"
            res["cases"][key].update(child(f"graph:{name}:{shape}"))
            print("graph", key, json.dumps({k: v for k, v in res["cases"][key].items()
                                            if k.startswith("graphed_")}), flush=True)
            write()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step = sys.argv[2]
        if step == "device":
            out = {"device": torch.cuda.get_device_name(0)}
        elif step.startswith("graph:"):
            out = graph_case(*step.split(":")[1:])
        else:
            out = step_case(*step.split(":"))
        print(json.dumps(out), flush=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1
             else os.path.join(ROOT, "profiles", "row_adam_ab", "row_adam_ab.json"))
