"""Row-sparse Adam that replays missed steps (``fuse_row_grad(replay=True)``) against the
dense whole-table step of the same build, on the same box ("Replaying missed
steps"):

    python scripts/row_replay_ab.py [out.json]  (default: profiles/row_replay_ab/row_replay_ab.json)

Each configuration times a FULL training step (plan, loss, backward, optimizer step) of an
(n, F) table.  Unlike scripts/row_adam_ab.py the batch changes every step -- 16 random
batches taken in turn -- because a fixed batch names the same rows every step and no row
would ever fall behind: here a row is named about once per 16 steps and replays ~15 missed
steps when it is.

Legs at ``weight_decay = 5e-4`` (the reference's configuration):
(a) ``replay``: the table registered with ``fuse_row_grad(replay=True)``;
(b) ``dense``: the same build without the registration (what the parent commit runs).
Legs at ``weight_decay = 0``: ``replay0`` against ``frozen``, the default registration
(frozen moments for unnamed rows): what the dense trajectory costs over that one.

Shapes: 2M x 128 with P = 65,536 and 100k x 128 with P = 4,096 (``link_bce_loss``, fp32 and
bf16); 1M x 32 with B = 65,536 and the 2015 graph's 39,179 x 32 with B = 512
(``sage_forward``, fp32, hidden = out = 32).  The legs take turns inside every round (7
rounds of 16 steps after a warm-up cycle, HIP events); every round's time is kept.

Also recorded: the catch-up launch alone on a batch's rows (``catch_up_us``, the rows ~15
steps behind; the table is re-aged by a cycle of steps before every timing), the extra
``(idx, idx)`` plan of ``sage_forward`` / ``link_match_loss`` (``idx_plan_us``: pair_plan +
plan_rows), and a whole-table flush after 100 steps (``flush_after_100_us``, median of 3).

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

# name: (loss, n, F, entries per batch)
SHAPES = {"2m_x128_p65536": ("bce", 2_000_000, 128, 65_536),
          "1m_x32_b65536": ("sage", 1_000_000, 32, 65_536),
          "100k_x128_p4096": ("bce", 100_000, 128, 4096),
          "39179_x32_b512": ("sage", 39_179, 32, 512)}
CONDITION = "2m_x128_p65536"  # every round of (a) faster than every round of (b)
CYCLE = 16
ROUNDS = 7
STEP_LIMIT_S = 420
WD = 5e-4
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def step_case(name, shape):
    import msha_loader

    msha_loader.load()
    from gemm_ab import timeit
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import graph_of
    from msha_gnn_amd.optim import Adam

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    dt = DT[name]
    loss_name, n, F, P = SHAPES[shape]
    h0 = ((torch.rand(n, F, device=dev, generator=g) - 0.5) * 0.6).to(dt)
    idx = [torch.randint(0, n, (2, P), device=dev, generator=g) for _ in range(CYCLE)]
    y = (torch.rand(P, device=dev, generator=g) < 0.5).float()
    if loss_name == "sage":
        M = 32
        adj = torch.rand(n, M, device=dev, generator=g) * (
            torch.rand(n, M, device=dev, generator=g) < 0.25)
        graph, _ = graph_of(adj)
        vals = graph.values(adj)
        target = torch.randint(0, M, (P,), device=dev, generator=g)
        lin = [((torch.rand(s, device=dev, generator=g) - 0.5) * 0.4)
               for s in ((M, F), (M,), (M, M), (M,))]

    def make(mode, wd):
        p = h0.clone().requires_grad_(True)
        extra = [t.clone().requires_grad_(True) for t in lin] if loss_name == "sage" else []
        opt = Adam([p] + extra, lr=1e-3, weight_decay=wd)
        if mode != "dense":
            opt.fuse_row_grad(p, replay=mode == "replay")
        k = [0]

        def step():
            src, dst = idx[k[0] % CYCLE]
            k[0] += 1
            opt.zero_grad(set_to_none=True)
            if loss_name == "bce":
                loss = MF.link_bce_loss(p, src, dst, y, plan=MF.pair_plan(src, dst, n))
            else:
                loss = torch.nn.functional.nll_loss(
                    MF.sage_forward(p, src, graph, vals, *extra, check=False), target)
            loss.backward()
            opt.step()

        def cycle():
            for _ in range(CYCLE):
                step()
        return p, opt, step, cycle

    res = {"loss": loss_name, "rows": n, "feat": F, "entries": P, "cycle": CYCLE}
    legs = {"replay": make("replay", WD), "dense": make("dense", WD),
            "replay0": make("replay", 0.0), "frozen": make("frozen", 0.0)}
    # same answer first: one cycle each, then the flushed replay table against the dense one
    for leg in legs.values():
        leg[3]()
    pa, oa = legs["replay"][:2]
    res["stale_rows_after_a_cycle"] = int(oa.stale_rows(pa))
    oa.catch_up(pa)
    res["bitwise_equal_to_dense_after_flush"] = bool(torch.equal(
        pa.detach().view(torch.int16 if dt == torch.bfloat16 else torch.int32),
        legs["dense"][0].detach().view(torch.int16 if dt == torch.bfloat16 else torch.int32)))
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, leg in legs.items():
            times[k].append(float(timeit(leg[3], reps=1, warm=0)) / CYCLE)
    for k, t in times.items():
        res[f"{k}_step_us_rounds"] = [round(x, 1) for x in t]
        res[f"{k}_step_us"] = round(float(np.median(t)), 1)
    res["ratio_dense_over_replay"] = round(res["dense_step_us"] / res["replay_step_us"], 3)
    res["ratio_replay0_over_frozen"] = round(res["replay0_step_us"] / res["frozen_step_us"], 3)
    res["every_replay_round_faster_than_every_dense_round"] = bool(
        max(times["replay"]) < min(times["dense"]))

    # the catch-up launch alone: the next batch's rows, about a cycle behind
    p, opt, step, cycle = legs["replay"]
    src, dst = idx[0]
    plan = MF.pair_plan(src, dst, n) if loss_name == "bce" else MF.pair_plan(src, src, n)
    MF.plan_rows(plan)
    ts = []
    for _ in range(ROUNDS):  # (whole cycles so far: batch 0 is next, its rows a cycle old)
        ts.append(float(timeit(lambda: opt.catch_up(p, plan), reps=1, warm=0)))
        cycle()
    res["catch_up_us"] = round(float(np.median(ts)), 1)
    res["catch_up_rows"] = int(MF.plan_rows(plan)[1])
    # the extra (idx, idx) plan of sage_forward / link_match_loss
    one = idx[0][0]
    res["idx_plan_us"] = round(float(timeit(
        lambda: MF.plan_rows(MF.pair_plan(one, one, n)), reps=10)), 1)
    # a whole-table flush after 100 steps
    ts = []
    for _ in range(3):
        opt.catch_up(p)
        for _ in range(100):
            step()
        res["stale_rows_after_100_steps"] = int(opt.stale_rows(p))
        ts.append(float(timeit(lambda: opt.catch_up(p), reps=1, warm=0)))
    res["flush_after_100_us"] = round(float(np.median(ts)), 1)
    # ... and of a table no step has named for 100 steps (every row replays 100 steps; the
    # record is set back by hand, so the table's values mean nothing after this: timing only)
    st = opt.state[p]
    st["row_step"].copy_((st["step"] - 100).clamp_(min=0).to(torch.int32).expand(n))
    res["flush_all_rows_100_steps_us"] = round(float(timeit(
        lambda: opt.catch_up(p), reps=1, warm=0)), 1)
    res["element_steps_per_s_all_rows"] = round(
        n * F * 100 / (res["flush_all_rows_100_steps_us"] * 1e-6), -6)
    return res


def child(step):
    """One configuration in a process of its own under a time limit: its last output line."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
           "--step", step]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"row_replay_ab: step {step} ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(out_path):
    res = {"shapes": {k: list(v) for k, v in SHAPES.items()}, "rounds": ROUNDS,
           "weight_decay": WD, "cases": {}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for shape, (loss_name, *_rest) in SHAPES.items():
        for name in DT:
            if loss_name == "sage" and name != "fp32":
                continue  # sage_forward takes fp32 tables
            key = f"{name}_{shape}"
            res["cases"][key] = child(f"{name}:{shape}")
            print(key, json.dumps(res["cases"][key]), flush=True)
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)
    res["device"] = child("device")["device"]
    res["condition_shape"] = CONDITION
    res["condition_met"] = all(
        res["cases"][f"{name}_{CONDITION}"]["every_replay_round_faster_than_every_dense_round"]
        for name in DT)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step = sys.argv[2]
        if step == "device":
            out = {"device": torch.cuda.get_device_name(0)}
        else:
            out = step_case(*step.split(":"))
        print(json.dumps(out), flush=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1
             else os.path.join(ROOT, "profiles", "row_replay_ab", "row_replay_ab.json"))
