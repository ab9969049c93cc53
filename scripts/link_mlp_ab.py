"""The fused 'mlp' link-predictor loss against the torch composition it replaces, on the same
box ("Link-prediction training of the 'mlp' predictor"):

    python scripts/link_mlp_ab.py [out.json]   (default: profiles/link_mlp_ab/link_mlp_ab.json)

(a) 4M pairs over a 100k x 128 table, N = 128, both ends uniform; (b) the same with dst in 32
rows, the repository's shape; (c) LLP's own batch: 4,096 pairs over a 100k x 32 table, N = 32.
fp32 and bf16 tables; labels uniform over the N classes; a teacher output of the same shape.

- ``functional.link_mlp_loss`` forward + backward (gradients to h, W and b), plan reused;
- ``out = sigmoid(relu(F.linear(h[src] * h[dst], W, b)))``, ``10 nll_loss + 100 mse_loss``
  forward + backward in torch (two (P, F) gathers, their product, ``index_put``'s float
  atomics).

The two are timed in alternating rounds (median of 7 rounds of HIP-event times per call after
warm-up).  Also, through the ABI: the forward call and its MFMA launch alone (their difference
is the index pass + loss pass + finish); the backward with only dz, with dz + weight
gradient, and whole, and ``dx = dz W`` alone -- the weight-gradient and table-gradient times
are differences of those (``table_grad_round_us``: the table-gradient difference of each
round, to show how far that column repeats).  Each with the achieved fraction of the 8 TB/s
HBM peak by its byte model.  The plan build is timed on its own.

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

N_ROWS, HOT = 100_000, 32
SHAPES = {"uniform": (4_000_000, 128, 128), "dst32": (4_000_000, 128, 128),
          "batch4096": (4096, 32, 32)}
HBM_PEAK = 8.0e12
ROUNDS = 7
STEP_LIMIT_S = 420
W_LABEL, W_MSE = 10.0, 100.0
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def alternate_us(fns, rounds=ROUNDS, reps=3, keep=None):
    """Median over ``rounds`` of the per-call time of each function, the functions taking
    turns inside every round.  ``keep``: a list that receives the rounds' own times, one list
    per function."""
    from gemm_ab import timeit

    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timeit(fn, reps=reps, warm=2))
    if keep is not None:
        keep.extend(times)
    return [float(np.median(t)) for t in times]


def step_case(name, dist):
    import torch.nn.functional as TF

    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    dt = DT[name]
    P, F, N = SHAPES[dist]
    n = N_ROWS
    h = ((torch.rand(n, F, device=dev, generator=g) - 0.5) * 1.5).to(dt).requires_grad_(True)
    W = ((torch.rand(N, F, device=dev, generator=g) - 0.5) * (3.0 / F ** 0.5)).requires_grad_(True)
    b = ((torch.rand(N, device=dev, generator=g) - 0.5) * 0.2).requires_grad_(True)
    src = torch.randint(0, n, (P,), device=dev, generator=g)
    dst = torch.randint(0, HOT if dist == "dst32" else n, (P,), device=dev, generator=g)
    lab = torch.randint(0, N, (P,), device=dev, generator=g)
    t_out = torch.rand(P, N, device=dev, generator=g)
    plan = MF.pair_plan(src, dst, n)
    leaves = (h, W, b)

    def clear():
        for x in leaves:
            x.grad = None

    def fused():
        clear()
        MF.link_mlp_loss(h, src, dst, W, b, label=lab, teacher_out=t_out, w_label=W_LABEL,
                         w_mse=W_MSE, plan=plan).backward()

    def baseline():
        clear()
        out = torch.sigmoid(torch.relu(TF.linear(h[src] * h[dst], W.to(dt), b.to(dt)))).float()
        (W_LABEL * TF.nll_loss(out, lab) + W_MSE * TF.mse_loss(out, t_out)).backward()

    # the kernels through the ABI
    lib, s = _lib.load(), _lib.stream_handle(dev)
    hd, Wk, bk = h.detach(), W.detach().to(dt).contiguous(), b.detach()
    W32 = Wk.float().contiguous()
    code = MF._code(dt)
    out = torch.empty(P, N, dtype=torch.float32, device=dev)
    terms = torch.empty(3, dtype=torch.float32, device=dev)
    pv = torch.empty(1, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    dz = torch.empty(P, N, dtype=torch.float32, device=dev)
    dx = torch.empty(P, F, dtype=torch.float32, device=dev)
    dW = torch.empty(N, F, dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev)
    dH = torch.empty(n, F, dtype=torch.float32, device=dev)
    wsf = torch.empty(lib.msha_link_mlp_loss_fwd_workspace_size(P), dtype=torch.uint8, device=dev)
    wsb = torch.empty(lib.msha_link_mlp_bwd_workspace_size(P, F, N), dtype=torch.uint8, device=dev)

    def fwd_call():
        _lib.call("msha_link_mlp_loss_fwd", P, F, N, code, hd.data_ptr(), hd.stride(0), n,
                  src.data_ptr(), dst.data_ptr(), lab.data_ptr(), Wk.data_ptr(), bk.data_ptr(),
                  t_out.data_ptr(), W_LABEL, W_MSE, 0.0, 0, 0, out.data_ptr(), terms.data_ptr(),
                  None, pv.data_ptr(), wsf.data_ptr(), wsf.numel(), s)

    def mfma_only():
        MF.score_pairs(hd, src, dst, "mlp", Wk, bk, out=out, check=False)

    def bwd_call(with_w, with_h):
        def run():
            _lib.call("msha_link_mlp_bwd", P, F, N, code, hd.data_ptr(), hd.stride(0), n,
                      src.data_ptr(), dst.data_ptr(), lab.data_ptr(),
                      W32.data_ptr() if with_h else None, t_out.data_ptr(), out.data_ptr(),
                      pv.data_ptr(), W_LABEL, W_MSE, 0.0, one.data_ptr(),
                      plan.rowptr.data_ptr() if with_h else None,
                      plan.ent.data_ptr() if with_h else None,
                      plan.chunk_tab.data_ptr() if with_h else None, dz.data_ptr(),
                      dx.data_ptr() if with_h else None, dW.data_ptr() if with_w else None,
                      db.data_ptr() if with_w else None, dH.data_ptr() if with_h else None,
                      wsb.data_ptr(), wsb.numel(), s)
        return run

    def dx_only():
        MF.gemm(dz, W32, out=dx)

    # same answer first (torch sums in another order: values differ by rounding)
    fused()
    g_f = [x.grad.float().clone() for x in leaves]
    baseline()
    g_b = [x.grad.float().clone() for x in leaves]
    fused()
    again = all(bool(torch.equal(x.grad.float(), y)) for x, y in zip(leaves, g_f))
    with torch.no_grad():
        l_f = float(MF.link_mlp_loss(h, src, dst, W, b, label=lab, teacher_out=t_out,
                                     w_label=W_LABEL, w_mse=W_MSE))
        o_b = torch.sigmoid(torch.relu(TF.linear(hd[src] * hd[dst], Wk, bk.to(dt)))).float()
        l_b = float(W_LABEL * TF.nll_loss(o_b, lab) + W_MSE * TF.mse_loss(o_b, t_out))
        del o_b
    t_f, t_b = alternate_us([fused, baseline])
    fwd_call()
    t_fw, t_mm = alternate_us([fwd_call, mfma_only], reps=5)
    bwd_rounds = []
    t_dz, t_dzw, t_all, t_dx = alternate_us([bwd_call(False, False), bwd_call(True, False),
                                             bwd_call(True, True), dx_only], reps=5,
                                            keep=bwd_rounds)
    (t_plan,) = alternate_us([lambda: MF.pair_plan(src, dst, n)], reps=5)
    esz = 4 if dt == torch.float32 else 2
    blocks = -(-P // lib.msha_link_mlp_wgrad_rows())
    model = {
        "loss_pass": P * (24 + 16 + 8 * N),                      # index pass + out + teacher
        "dz": P * (24 + 12 * N),
        "wgrad": P * (16 + 4 * N + 2 * esz * F) + 2 * blocks * (N * F + N) * 4,
        "table_grad": 2 * P * (12 + 4 * F + esz * F) + n * (4 + 4 * F),
    }
    times = {"loss_pass": t_fw - t_mm, "dz": t_dz, "wgrad": t_dzw - t_dz,
             "table_grad": t_all - t_dzw - t_dx}
    res = {"pairs": P, "feat": F, "hidden": N,
           "link_mlp_fwd_bwd_us": round(t_f, 1), "torch_fwd_bwd_us": round(t_b, 1),
           "ratio_torch_over_fused": round(t_b / t_f, 3),
           "fwd_call_us": round(t_fw, 1), "fwd_mfma_launch_us": round(t_mm, 1),
           "bwd_call_us": round(t_all, 1), "dx_gemm_us": round(t_dx, 1),
           "plan_build_us": round(t_plan, 1),
           "fused_gradients_bitwise_repeatable": again, "loss_fused": l_f, "loss_torch": l_b,
           # the table-gradient difference round by round: how far the column repeats
           "table_grad_round_us": [round(a - w - x, 1) for _, w, a, x in zip(*bwd_rounds)]}
    for k in model:
        res[f"{k}_us"] = round(times[k], 1)
        res[f"{k}_model_bytes"] = model[k]
        res[f"{k}_fraction_of_hbm_peak"] = (round(model[k] / (times[k] * 1e-6) / HBM_PEAK, 4)
                                            if times[k] > 0 else None)
    for nm, a, c in zip(("dH", "dW", "db"), g_f, g_b):
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
        raise SystemExit(f"link_mlp_ab: step {step} ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(out_path):
    res = {"table_rows": N_ROWS, "hot_rows": HOT, "shapes": {k: list(v) for k, v in SHAPES.items()},
           "w_label": W_LABEL, "w_mse": W_MSE, "rounds": ROUNDS,
           "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for name in DT:
        for dist in SHAPES:
            res["cases"][f"{name}_{dist}"] = child(f"{name}:{dist}")
            print(f"{name}_{dist}", json.dumps(res["cases"][f"{name}_{dist}"]), flush=True)
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
        if step == "device":
            out = {"device": torch.cuda.get_device_name(0)}
        else:
            out = step_case(*step.split(":"))
        print(json.dumps(out), flush=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1
             else os.path.join(ROOT, "profiles", "link_mlp_ab", "link_mlp_ab.json"))
