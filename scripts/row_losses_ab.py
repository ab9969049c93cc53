"""Row-sparse table training through sage_forward, link_mlp_loss and the combined LLP
objective, against the dense whole-table update of the same build and against torch's
sparse-embedding path, on the same box ("Row-sparse table training"):

    python scripts/row_losses_ab.py [out.json]
                                    (default: profiles/row_losses_ab/row_losses_ab.json)

scripts/row_adam_ab.py's method: each leg times a FULL training step of the table -- loss,
backward, optimizer step; the Linear weights are inputs, not trained -- three ways that take
turns inside every round (7 rounds of 3 steps after 2 warm-up steps, HIP events; every round's
time is kept), one child process per leg:

(a) ``registered``: the table registered with ``optim.Adam.fuse_row_grad`` (``accumulate=True``
    for the combined objective): compact row gradient(s), their union, lazy Adam;
(b) ``dense``: the same build without the registration: (n, F) gradient, whole-table Adam;
(c) ``torch``: ``F.embedding(..., sparse=True)`` gathers, the same loss in torch ops,
    ``torch.optim.SparseAdam``.

Legs:

    sage:r15_b512       sage_forward + nll at the shipped 2015 graph (39,179 x 32), B = 512
    sage:bip1m_b65536   the same at a synthetic 1M x 32 adjacency, B = 65,536
    mlp:<shape>         link_mlp_loss (label + MSE terms), N = 128
    llp:<shape>         link_mlp_loss + 0.1 link_match_loss(rows = src)   (LLP.py:237-238)

with <shape> in 100k x 128 and 2M x 128, P = 4,096 and 65,536 (fp32 tables).  After the eager
figures are written, (a) and (b) are each captured into one HIP graph and the replays timed the
same way (``graphed_*``; 10 replays a round).  Every leg runs under its own time limit; the
first child that fails ends the run.  Prints one JSON object and writes it out.
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

from row_adam_ab import ROUNDS, alternate_rounds_us  # noqa: E402

PAIR_SHAPES = {"100k_x128_p4096": (100_000, 128, 4096),
               "100k_x128_p65536": (100_000, 128, 65_536),
               "2m_x128_p4096": (2_000_000, 128, 4096),
               "2m_x128_p65536": (2_000_000, 128, 65_536)}
SAGE_SHAPES = {"r15_b512": 512, "bip1m_b65536": 65_536}
HIDDEN = 128
STEP_LIMIT_S = 300
LEGS = ([f"sage:{s}" for s in SAGE_SHAPES] + [f"mlp:{s}" for s in PAIR_SHAPES]
        + [f"llp:{s}" for s in PAIR_SHAPES])


def _sage_leg(shape, dev, gen):
    """(make_step(register), torch_step, info) of a sage leg."""
    import torch.nn.functional as TF

    import bench
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import graph_of, normalize_adjacency_matrix
    from msha_gnn_amd.optim import Adam

    B = SAGE_SHAPES[shape]
    rowptr, col, n, m = bench.r15_graph() if shape.startswith("r15") else bench.bip_graph()
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    counts = torch.zeros(n, m, device=dev)
    counts[torch.as_tensor(rows, device=dev), torch.as_tensor(col, device=dev)] = 1.0
    counts[:m, :m] += torch.eye(m, device=dev)  # no empty column
    adj = normalize_adjacency_matrix(counts)
    del counts
    g, _ = graph_of(adj)
    vals = g.values(adj)
    h0 = torch.rand(n, 32, device=dev, generator=gen)
    l1, l2 = torch.nn.Linear(32, m).to(dev), torch.nn.Linear(m, 32).to(dev)
    ws = [t.detach() for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
    src = torch.randint(0, n, (B,), device=dev, generator=gen)
    target = torch.randint(0, 32, (B,), device=dev, generator=gen)

    def make(register):
        p = h0.clone().requires_grad_(True)
        opt = Adam([p], lr=1e-3)
        if register:
            opt.fuse_row_grad(p)

        def step():
            opt.zero_grad(set_to_none=True)
            TF.nll_loss(MF.sage_forward(p, src, g, vals, *ws, check=False), target).backward()
            opt.step()
        return p, opt, step

    pc = h0.clone().requires_grad_(True)
    oc = torch.optim.SparseAdam([pc], lr=1e-3)

    def torch_step():
        oc.zero_grad(set_to_none=True)
        x = torch.relu(TF.linear(TF.embedding(src, pc, sparse=True), ws[0], ws[1]))
        x = torch.relu(TF.linear(adj[src] * x, ws[2], ws[3]))
        TF.nll_loss(TF.log_softmax(x, dim=1), target).backward()
        oc.step()

    touched = int(torch.unique(src).numel())
    return make, torch_step, {"rows": n, "feat": 32, "batch": B, "touched_rows": touched}


def _pair_leg(kind, shape, dev, gen):
    """(make_step(register), torch_step, info) of a link_mlp_loss / LLP-objective leg."""
    import torch.nn.functional as TF

    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.optim import Adam

    n, F, P = PAIR_SHAPES[shape]
    N = HIDDEN
    h0 = (torch.rand(n, F, device=dev, generator=gen) - 0.5) * 0.6
    T = (torch.rand(n, F, device=dev, generator=gen) - 0.5) * 0.6 if kind == "llp" else None
    W = torch.randn(N, F, device=dev, generator=gen) / F ** 0.5
    b = torch.zeros(N, device=dev)
    src = torch.randint(0, n, (P,), device=dev, generator=gen)
    dst = torch.randint(0, n, (P,), device=dev, generator=gen)
    label = torch.randint(0, N, (P,), device=dev, generator=gen)
    teacher = torch.rand(P, N, device=dev, generator=gen)

    def make(register):
        p = h0.clone().requires_grad_(True)
        opt = Adam([p], lr=1e-3)
        if register:
            opt.fuse_row_grad(p, accumulate=kind == "llp")

        def step():
            opt.zero_grad(set_to_none=True)
            loss = MF.link_mlp_loss(p, src, dst, W, b, label=label, teacher_out=teacher,
                                    w_mse=0.5, plan=MF.pair_plan(src, dst, n))
            if kind == "llp":
                loss = loss + 0.1 * MF.link_match_loss(p, src, T)
            loss.backward()
            opt.step()
        return p, opt, step

    pc = h0.clone().requires_grad_(True)
    oc = torch.optim.SparseAdam([pc], lr=1e-3)

    def torch_step():
        oc.zero_grad(set_to_none=True)
        hs = TF.embedding(src, pc, sparse=True)
        out = torch.sigmoid(torch.relu(TF.linear(hs * TF.embedding(dst, pc, sparse=True), W, b)))
        loss = TF.nll_loss(out, label) + 0.5 * TF.mse_loss(out, teacher)
        if kind == "llp":
            loss = loss + 0.1 * (1 - TF.cosine_similarity(hs, T[src], dim=-1).mean())
        loss.backward()
        oc.step()

    touched = int(torch.unique(torch.cat([src, dst])).numel())
    return make, torch_step, {"rows": n, "feat": F, "pairs": P, "hidden": N,
                              "touched_rows": touched}


def _leg(leg, dev, gen):
    kind, shape = leg.split(":")
    return _sage_leg(shape, dev, gen) if kind == "sage" else _pair_leg(kind, shape, dev, gen)


def step_case(leg):
    import msha_loader

    msha_loader.load()
    dev = torch.device("cuda:0")
    make, torch_step, res = _leg(leg, dev, torch.Generator(device=dev).manual_seed(0))
    pa, oa, step_a = make(True)
    pb, ob, step_b = make(False)
    fns, names = [step_a, step_b], ["registered", "dense"]
    try:  # torch's sparse path (recorded when it does not run)
        torch_step()
        torch.cuda.synchronize()
        fns.append(torch_step)
        names.append("torch")
    except Exception as e:  # noqa: BLE001 - the reason goes into the result
        res["torch_unavailable"] = f"{type(e).__name__}: {e}"[:300]
    # same answer first: one step each from the same table; the registered table has no .grad
    step_a()
    step_b()
    moved = (ob.state[pb]["exp_avg"] != 0).any(1)  # the rows with a gradient
    res["registered_has_no_dense_grad"] = pa.grad is None
    res["touched_rows_bitwise_equal_after_one_step"] = bool(
        torch.equal(pa.detach()[moved], pb.detach()[moved]))
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
    return res


def graph_case(leg):
    """Paths (a) and (b) each captured into one HIP graph and replayed."""
    import msha_loader

    msha_loader.load()
    dev = torch.device("cuda:0")
    make, _, _ = _leg(leg, dev, torch.Generator(device=dev).manual_seed(0))
    # a captured graph holds addresses, not references: everything stays alive to the end
    replays, alive = [], []
    for register in (True, False):
        p, opt, step = make(register)
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


def child(step):
    """One leg in a process of its own under a time limit: its last output line."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
           "--step", step]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"row_losses_ab: step {step} ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(out_path):
    res = {"pair_shapes": {k: list(v) for k, v in PAIR_SHAPES.items()},
           "sage_batches": SAGE_SHAPES, "hidden": HIDDEN, "rounds": ROUNDS, "cases": {}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    def write():
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)

    for leg in LEGS:
        res["cases"][leg] = child("eager=" + leg)
        print(leg, json.dumps(res["cases"][leg]), flush=True)
        write()
    res["device"] = child("device")["device"]
    write()  # the eager figures stand whatever becomes of the graph legs
    for leg in LEGS:
        res["cases"][leg].update(child("graph=" + leg))
        print("graph", leg, json.dumps({k: v for k, v in res["cases"][leg].items()
                                        if k.startswith("graphed_")}), flush=True)
        write()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step = sys.argv[2]
        if step == "device":
            out = {"device": torch.cuda.get_device_name(0)}
        elif step.startswith("graph="):
            out = graph_case(step.split("=", 1)[1])
        else:
            out = step_case(step.split("=", 1)[1])
        print(json.dumps(out), flush=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1
             else os.path.join(ROOT, "profiles", "row_losses_ab", "row_losses_ab.json"))
