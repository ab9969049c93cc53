"""Fused link-prediction loss against the torch formulation it replaces, on the same box in
the same process ("Link-prediction training"):

    python scripts/link_loss_ab.py [out.json]

On the link configuration (100k x 128 table, fp32 and bf16, P = 4M pairs), (a) both ends
uniform over the table and (b) dst in [0, 32), the repository's shape:

- ``functional.link_bce_loss`` forward + backward with a reused ``PairPlan``;
- ``F.binary_cross_entropy_with_logits((h[src] * h[dst]).sum(-1), y)`` forward + backward
  (two (P, F) gathers, their products, and ``index_put``'s float-atomic backward).

Also the kernels on their own: the forward launch pair, the backward launch triple, the
plan build, and the negative sampler at k = 1; for the forward and the backward the achieved
fraction of the 8 TB/s HBM peak by their byte models (per pair 16 + 2 s F + 8; per endpoint
4 + 8 + 8 + s F and per row 4 + 4 F; weight = None).  HIP-event times per call after
warm-up (median of 5 batches of 5 calls).  Prints one JSON object; writes it to
``out.json`` if given.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, F, P, HOT = 100_000, 128, 4_000_000, 32
HBM_PEAK = 8.0e12


def median_us(fn, groups=5, reps=5):
    from gemm_ab import timeit

    return float(np.median([timeit(fn, reps=reps, warm=2) for _ in range(groups)]))


def main(out_path=None):
    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.graph import Graph

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    table32 = (torch.rand(N, F, device=dev, generator=g) - 0.5) * 0.35
    y = (torch.rand(P, device=dev, generator=g) < 0.5).to(torch.float32)
    src = torch.randint(0, N, (P,), device=dev, generator=g)
    ends = {"uniform": torch.randint(0, N, (P,), device=dev, generator=g),
            "dst32": torch.randint(0, HOT, (P,), device=dev, generator=g)}
    res = {"table": [N, F], "pairs": P, "plan_chunk": int(_lib.load().msha_pair_plan_chunk()),
           "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0),
           "cases": {}}
    one = torch.ones((), device=dev)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        s = 4 if dt == torch.float32 else 2
        for shape, dst in ends.items():
            h = table32.to(dt).clone().requires_grad_(True)
            plan = MF.pair_plan(src, dst, N)

            def fused():
                h.grad = None
                MF.link_bce_loss(h, src, dst, y, plan=plan).backward()

            def baseline():
                h.grad = None
                logit = (h[src] * h[dst]).sum(-1)
                torch.nn.functional.binary_cross_entropy_with_logits(logit.float(), y).backward()

            def fwd_only():
                with torch.no_grad():
                    return MF.link_bce_loss(h, src, dst, y, return_logits=True)

            loss, z = fwd_only()
            hd = h.detach()
            dH = torch.empty(N, F, dtype=torch.float32, device=dev)
            ws = torch.empty(_lib.load().msha_link_bce_bwd_workspace_size(P, F),
                             dtype=torch.uint8, device=dev)

            def bwd_only():
                _lib.call("msha_link_bce_bwd", P, F, MF._code(dt), hd.data_ptr(), hd.stride(0),
                          N, src.data_ptr(), dst.data_ptr(), y.data_ptr(), None, z.data_ptr(),
                          one.data_ptr(), plan.rowptr.data_ptr(), plan.ent.data_ptr(),
                          plan.chunk_tab.data_ptr(), dH.data_ptr(), ws.data_ptr(), ws.numel(),
                          _lib.stream_handle(dev))

            # same answer first (torch sums in another order: values differ by rounding)
            fused()
            g_f = h.grad.float().clone()
            baseline()
            g_b = h.grad.float()
            scale = float(g_b.abs().max())
            diff = float((g_f - g_b).abs().max())
            fused()
            again = bool(torch.equal(h.grad.float(), g_f))
            t_f, t_b = median_us(fused), median_us(baseline)
            t_fw, t_bw = median_us(fwd_only), median_us(bwd_only)
            t_plan = median_us(lambda: MF.pair_plan(src, dst, N))
            fwd_bytes = P * (16 + 2 * s * F + 8)
            bwd_bytes = 2 * P * (4 + 8 + 8 + s * F) + N * (4 + 4 * F)
            res["cases"][f"{name}_{shape}"] = {
                "link_bce_fwd_bwd_us": round(t_f, 1), "torch_fwd_bwd_us": round(t_b, 1),
                "ratio_torch_over_fused": round(t_b / t_f, 3),
                "fwd_us": round(t_fw, 1), "bwd_us": round(t_bw, 1),
                "plan_build_us": round(t_plan, 1),
                "fwd_model_bytes": fwd_bytes, "bwd_model_bytes": bwd_bytes,
                "fwd_fraction_of_hbm_peak": round(fwd_bytes / (t_fw * 1e-6) / HBM_PEAK, 4),
                "bwd_fraction_of_hbm_peak": round(bwd_bytes / (t_bw * 1e-6) / HBM_PEAK, 4),
                "fused_gradient_bitwise_repeatable": again,
                "max_abs_gradient_difference": diff, "max_abs_gradient": scale}
            del h, plan, dH, ws, g_f, g_b
    # the sampler on the repository's shape: 100k sources x 32 recipients, k = 1
    adj = (torch.rand(N, HOT, device=dev, generator=g) < 0.15).to(torch.float32)
    graph = Graph.from_dense(adj)
    t_s = median_us(lambda: MF.sample_negatives(graph, src, k=1, seed=1))
    res["negative_sampler"] = {"graph": [N, HOT], "edges": graph.n_edges, "positives": P, "k": 1,
                               "us": round(t_s, 1)}
    res["not_slower_in_every_case"] = all(c["ratio_torch_over_fused"] >= 1.0
                                          for c in res["cases"].values())
    print(json.dumps(res), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
