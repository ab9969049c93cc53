"""Fused top-K retrieval against the only path the library offered before it, on the same
box in the same process ("Top-K link retrieval"):

    python scripts/topk_ab.py [out.json]

On the link configuration (100k x 128 table, K = 50, B = 512 and 4,096 queries, fp32 and
bf16):

- ``functional.topk_inner`` (one scoring launch + the split merge, no score matrix);
- ``functional.gemm`` into a (B_chunk, n) fp32 score buffer followed by ``torch.topk``,
  chunked so the buffer stays under 1 GB.

HIP-event times per call after warm-up (median of 5 batches of 10 calls).  For each case
also the achieved fraction of the MFMA peak of the operand type (fp32: 157.3 TFLOP/s on
the exact-f32 forms; bf16: 2,500 TFLOP/s dense) at 2 B n F flops, for the fused path and
for the GEMM alone at the same shape.  Prints one JSON object; writes it to ``out.json``
if given.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, F, K = 100_000, 128, 50
BATCHES = (512, 4096)
PEAK = {"fp32": 157.3e12, "bf16": 2500e12}
BUF_BYTES = 1 << 30


def median_us(fn, groups=5, reps=10):
    from gemm_ab import timeit

    return float(np.median([timeit(fn, reps=reps, warm=2) for _ in range(groups)]))


def main(out_path=None):
    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    table32 = torch.rand(N, F, device=dev, generator=g)
    res = {"table": [N, F], "k": K, "device": torch.cuda.get_device_name(0), "cases": {}}
    chunk = min(max(BATCHES), BUF_BYTES // (4 * N) // 256 * 256)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        table = table32.to(dt)
        tt = table.t()
        for B in BATCHES:
            rows = torch.randint(0, N, (B,), device=dev, generator=g)
            q = table[rows].contiguous()
            buf = torch.empty(min(B, chunk), N, device=dev, dtype=torch.float32)

            def fused():
                return MF.topk_inner(table, table, K, rows=rows, sigmoid=False, check=False)

            def scores(b0, b1):
                if dt == torch.float32:
                    return MF.gemm(q[b0:b1], tt, out=buf[: b1 - b0])
                return MF.gemm(q[b0:b1], tt, out_dtype=torch.float32)

            def gemm_only():
                for b0 in range(0, B, chunk):
                    scores(b0, min(B, b0 + chunk))

            def baseline():
                out = []
                for b0 in range(0, B, chunk):
                    out.append(torch.topk(scores(b0, min(B, b0 + chunk)), K, dim=1))
                return out

            # same answer first (the GEMM sums over f in another order: values differ by rounding)
            v, i = fused()
            bv = torch.cat([o[0] for o in baseline()])
            same = bool(torch.equal(v, bv)) if dt == torch.float32 else None
            close = float((v - bv).abs().max())
            t_f, t_b, t_g = median_us(fused), median_us(baseline), median_us(gemm_only)
            flops = 2.0 * B * N * F
            res["cases"][f"{name}_B{B}"] = {
                "topk_inner_us": round(t_f, 1), "gemm_topk_us": round(t_b, 1),
                "gemm_only_us": round(t_g, 1), "ratio_baseline_over_fused": round(t_b / t_f, 3),
                "splits": int(_lib.load().msha_topk_inner_splits(B, N, F, K, MF._code(dt))),
                "fused_fraction_of_mfma_peak": round(flops / (t_f * 1e-6) / PEAK[name], 4),
                "gemm_fraction_of_mfma_peak": round(flops / (t_g * 1e-6) / PEAK[name], 4),
                "values_equal_baseline": same, "max_abs_value_difference": close,
                "score_buffer_bytes_avoided": 4 * B * N}
    res["not_slower_in_every_case"] = all(c["ratio_baseline_over_fused"] >= 1.0
                                          for c in res["cases"].values())
    print(json.dumps(res), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
