"""Fused link-prediction distillation loss against the torch composition it replaces, on the
same box in the same process ("Link-prediction distillation"):

    python scripts/distill_ab.py [out.json]      (default: profiles/distill_ab/distill_ab.json)

A = 65,536 anchors x K = 32 context nodes over a 100k x 128 table, fp32 and bf16, teacher
logits given, margin 0.1, tau 1, w_rank = w_dist = 1:

- ``functional.link_distill_loss`` forward + backward with a reused ``context_plan``;
- the torch composition: the (A, K, F) gather, ``einsum`` for the logits,
  ``F.margin_ranking_loss`` over the K (K - 1) / 2 pairs of every anchor, ``F.kl_div`` of the
  two softmaxes, and autograd through ``index_put``'s float-atomic backward.

The two are timed in alternating rounds (median of 7 rounds of HIP-event times per call
after warm-up).  Also the kernels on their own (the forward launch pair, the backward launch
triple, the plan build, the context sampler) and, for the forward and the backward, the
achieved fraction of the 8 TB/s HBM peak by their byte models: A (K + 1) F s gathered plus
A K (8 + 4 + 4 + 4) index and scalar bytes forward; per endpoint 4 + 8 + 8 + s F and per
row 4 + 4 F backward (link_bce_bwd's row).  Prints one JSON object and writes it out.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, F, A, K = 100_000, 128, 65_536, 32
MARGIN, TAU = 0.1, 1.0
HBM_PEAK = 8.0e12
ROUNDS = 7


def alternate_us(fns, rounds=ROUNDS, reps=5):
    """Median over ``rounds`` of the per-call time of each function, the functions taking
    turns inside every round."""
    from gemm_ab import timeit

    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timeit(fn, reps=reps, warm=2))
    return [float(np.median(t)) for t in times]


def main(out_path):
    import torch.nn.functional as TF

    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import Graph

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    table32 = (torch.rand(N, F, device=dev, generator=g) - 0.5) * 0.35
    anchors = torch.randint(0, N, (A,), device=dev, generator=g)
    ctx = torch.randint(0, N, (A, K), device=dev, generator=g)
    tl = torch.randn(A, K, device=dev, generator=g)
    iu, ju = (t.to(dev) for t in torch.triu_indices(K, K, 1))
    d = tl[:, iu] - tl[:, ju]
    r = torch.where(d.abs() > MARGIN, torch.sign(d), torch.zeros_like(d))
    p_teacher = torch.softmax(tl / TAU, 1)
    res = {"table": [N, F], "anchors": A, "context": K, "margin": MARGIN, "tau": TAU,
           "rounds": ROUNDS, "plan_chunk": int(_lib.load().msha_pair_plan_chunk()),
           "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0),
           "cases": {}}
    one = torch.ones((), device=dev)
    P = A * K
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        s = 4 if dt == torch.float32 else 2
        h = table32.to(dt).clone().requires_grad_(True)
        plan = MF.context_plan(anchors, ctx, N)

        def fused():
            h.grad = None
            MF.link_distill_loss(h, anchors, ctx, teacher_logits=tl, margin=MARGIN, tau=TAU,
                                 plan=plan).backward()

        def baseline():
            h.grad = None
            y = torch.einsum("af,akf->ak", h[anchors], h[ctx]).float()
            lr = TF.margin_ranking_loss(y[:, iu], y[:, ju], r, margin=MARGIN, reduction="sum")
            ld = TF.kl_div(torch.log_softmax(y / TAU, 1), p_teacher, reduction="sum")
            ((lr + ld) / A).backward()

        def fwd_only():
            with torch.no_grad():
                return MF.link_distill_loss(h, anchors, ctx, teacher_logits=tl, margin=MARGIN,
                                            tau=TAU)

        hd = h.detach()
        gk = torch.randn(A, K, device=dev, generator=g) / A
        dH = torch.empty(N, F, dtype=torch.float32, device=dev)
        ws = torch.empty(_lib.load().msha_pair_grad_bwd_workspace_size(P, F), dtype=torch.uint8,
                         device=dev)

        def bwd_only():
            _lib.call("msha_pair_grad_bwd", P, F, MF._code(dt), hd.data_ptr(), hd.stride(0), N,
                      plan.src.data_ptr(), ctx.data_ptr(), gk.data_ptr(), one.data_ptr(),
                      plan.rowptr.data_ptr(), plan.ent.data_ptr(), plan.chunk_tab.data_ptr(),
                      dH.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_handle(dev))

        # same answer first (torch sums in another order and takes its hinge decisions from
        # its own logits: values differ by rounding)
        fused()
        g_f = h.grad.float().clone()
        l_f = float(fwd_only())
        baseline()
        g_b = h.grad.float()
        with torch.no_grad():
            y = torch.einsum("af,akf->ak", h[anchors], h[ctx]).float()
            l_b = float((TF.margin_ranking_loss(y[:, iu], y[:, ju], r, margin=MARGIN,
                                                reduction="sum")
                         + TF.kl_div(torch.log_softmax(y / TAU, 1), p_teacher,
                                     reduction="sum")) / A)
            del y
        scale = float(g_b.abs().max())
        diff = float((g_f - g_b).abs().max())
        fused()
        again = bool(torch.equal(h.grad.float(), g_f))
        t_f, t_b = alternate_us([fused, baseline])
        t_fw, t_bw = alternate_us([fwd_only, bwd_only])
        t_plan = alternate_us([lambda: MF.context_plan(anchors, ctx, N)])[0]
        fwd_bytes = A * (K + 1) * F * s + A * K * (8 + 4 + 4 + 4)
        bwd_bytes = 2 * P * (4 + 8 + 8 + s * F) + N * (4 + 4 * F)
        res["cases"][name] = {
            "link_distill_fwd_bwd_us": round(t_f, 1), "torch_fwd_bwd_us": round(t_b, 1),
            "ratio_torch_over_fused": round(t_b / t_f, 3),
            "fwd_us": round(t_fw, 1), "bwd_us": round(t_bw, 1), "plan_build_us": round(t_plan, 1),
            "fwd_model_bytes": fwd_bytes, "bwd_model_bytes": bwd_bytes,
            "fwd_fraction_of_hbm_peak": round(fwd_bytes / (t_fw * 1e-6) / HBM_PEAK, 4),
            "bwd_fraction_of_hbm_peak": round(bwd_bytes / (t_bw * 1e-6) / HBM_PEAK, 4),
            "fused_gradient_bitwise_repeatable": again, "loss_fused": l_f, "loss_torch": l_b,
            "max_abs_gradient_difference": diff, "max_abs_gradient": scale}
        del h, plan, dH, ws, g_f, g_b
    # the sampler: 8 walks of 3 hops plus 8 uniform nodes per anchor on a 100k-node graph
    deg = 8
    rowptr = torch.arange(0, (N + 1) * deg, deg, dtype=torch.int32, device=dev)
    col = torch.randint(0, N, (N * deg,), device=dev, generator=g).to(torch.int32)
    graph = Graph(N, N, rowptr, col)
    t_s = alternate_us([lambda: MF.sample_context(graph, anchors, walks=8, hops=3, n_rand=8,
                                                  seed=1)])[0]
    res["context_sampler"] = {"graph": [N, N], "edges": N * deg, "anchors": A, "walks": 8,
                              "hops": 3, "n_rand": 8, "us": round(t_s, 1)}
    res["not_slower_in_every_case"] = all(c["ratio_torch_over_fused"] >= 1.0
                                          for c in res["cases"].values())
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1
         else os.path.join(ROOT, "profiles", "distill_ab", "distill_ab.json"))
