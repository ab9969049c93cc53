"""Filtered link ranks against the only routes the library offered before them, on the same
box in the same process ("Filtered link ranks"):

    python scripts/rank_ab.py [out.json]

On the link configuration (100k x 128 table, B = 512 and 4,096 queries, uniform targets, no
exclusion list, fp32 and bf16):

- ``functional.rank_inner`` (one counting launch + the split sum, no score matrix);
- (a) the route it replaces: ``functional.gemm`` into a (B_chunk, n) fp32 score buffer
  followed by ``(S > S[b, t]).sum(1)`` and ``(S == S[b, t]).sum(1)`` in torch, chunked so
  the buffer stays under 1 GB;
- (b) ``functional.topk_inner`` at K = 128, which answers Hits@K up to 128 and no rank
  beyond it.

The three, and the GEMM alone, are timed in alternating rounds (rank, a, b, gemm, rank, ...),
7 rounds: HIP-event time per call after warm-up over a window of at least 10 calls and
about 0.1 s of device time; the median round is quoted, the lowest and highest are kept
beside it.  For each case also the achieved fraction of the MFMA peak of the operand type
(fp32: 157.3 TFLOP/s on the exact-f32 forms; bf16: 2,500 TFLOP/s dense) at 2 B n F flops --
a whole-call rate, the splits' finishing launch included -- for the counting path, the
top-K path and the GEMM alone at the same shape.  Beside the comparison, ``rank_inner`` is
timed in the same rounds with an exclusion list of 20 and of 200 random candidates per
query (the filtered setting).  Prints one JSON object; writes it to ``out.json`` if given.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, F, K = 100_000, 128, 128
BATCHES = (512, 4096)
PEAK = {"fp32": 157.3e12, "bf16": 2500e12}
BUF_BYTES = 1 << 30
ROUNDS, MIN_REPS, WINDOW_US = 7, 10, 1e5


def alternate(fns):
    """{name: [us per call of each round]}, the functions taking turns within a round."""
    from gemm_ab import timeit

    reps = {k: max(MIN_REPS, int(WINDOW_US / timeit(fn, reps=MIN_REPS, warm=3)))
            for k, fn in fns.items()}
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            out[k].append(timeit(fn, reps=reps[k], warm=2))
    return out


def stats(xs):
    return {"median_us": round(float(np.median(xs)), 1), "min_us": round(float(min(xs)), 1),
            "max_us": round(float(max(xs)), 1)}


def main(out_path=None):
    import msha_loader

    msha_loader.load()
    from msha_gnn_amd import _lib
    from msha_gnn_amd import functional as MF

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    table32 = torch.rand(N, F, device=dev, generator=g)
    res = {"table": [N, F], "topk_k": K, "rounds": ROUNDS, "window_us": WINDOW_US,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    chunk = min(max(BATCHES), BUF_BYTES // (4 * N) // 256 * 256)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        table = table32.to(dt)
        tt = table.t()
        for B in BATCHES:
            rows = torch.randint(0, N, (B,), device=dev, generator=g)
            target = torch.randint(0, N, (B,), device=dev, generator=g)
            q = table[rows].contiguous()
            buf = torch.empty(min(B, chunk), N, device=dev, dtype=torch.float32)

            def ranks():
                return MF.rank_inner(table, table, target, rows=rows, check=False)

            def excluded(per_query):
                qpos = torch.arange(B, device=dev).repeat_interleave(per_query)
                cols = torch.randint(0, N, (B * per_query,), device=dev, generator=g)
                ex = MF.exclude_from_pairs(qpos, cols, B)
                return lambda: MF.rank_inner(table, table, target, rows=rows, exclude=ex,
                                             check=False)

            def scores(b0, b1):
                if dt == torch.float32:
                    return MF.gemm(q[b0:b1], tt, out=buf[: b1 - b0])
                return MF.gemm(q[b0:b1], tt, out_dtype=torch.float32)

            def gemm_only():
                for b0 in range(0, B, chunk):
                    scores(b0, min(B, b0 + chunk))

            def baseline():
                gr, eq = [], []
                for b0 in range(0, B, chunk):
                    b1 = min(B, b0 + chunk)
                    S = scores(b0, b1)
                    zt = S.gather(1, target[b0:b1, None])
                    gr.append((S > zt).sum(1))
                    eq.append((S == zt).sum(1) - 1)  # the target itself
                return torch.cat(gr), torch.cat(eq)

            def topk():
                return MF.topk_inner(table, table, K, rows=rows, sigmoid=False, check=False)

            # the same answer first: the GEMM sums over f in another order, so a count may
            # move by the candidates whose logit is within rounding of the target's
            gr, eq, _ = ranks()
            bg, be = baseline()
            moved = int((gr != bg).sum())
            worst = int((gr - bg).abs().max())
            t = alternate({"rank_inner": ranks, "gemm_compare": baseline, "topk_inner": topk,
                           "gemm_only": gemm_only, "rank_inner_excl20": excluded(20),
                           "rank_inner_excl200": excluded(200)})
            med = {k: float(np.median(v)) for k, v in t.items()}
            flops = 2.0 * B * N * F
            lib = _lib.load()
            res["cases"][f"{name}_B{B}"] = {
                "rank_inner": stats(t["rank_inner"]), "gemm_compare": stats(t["gemm_compare"]),
                "topk_inner_k128": stats(t["topk_inner"]), "gemm_only": stats(t["gemm_only"]),
                "rank_inner_exclude_20_per_query": stats(t["rank_inner_excl20"]),
                "rank_inner_exclude_200_per_query": stats(t["rank_inner_excl200"]),
                "ratio_gemm_compare_over_rank": round(med["gemm_compare"] / med["rank_inner"], 3),
                "ratio_topk_over_rank": round(med["topk_inner"] / med["rank_inner"], 3),
                "splits": int(lib.msha_rank_inner_splits(B, N, F, MF._code(dt))),
                "rank_fraction_of_mfma_peak": round(flops / (med["rank_inner"] * 1e-6) / PEAK[name], 4),
                "topk_fraction_of_mfma_peak": round(flops / (med["topk_inner"] * 1e-6) / PEAK[name], 4),
                "gemm_fraction_of_mfma_peak": round(flops / (med["gemm_only"] * 1e-6) / PEAK[name], 4),
                "rows_whose_greater_differs_from_gemm": moved, "largest_such_difference": worst,
                "score_buffer_bytes_avoided": 4 * B * N}
    res["faster_than_gemm_compare_in_every_case"] = all(
        c["ratio_gemm_compare_over_rank"] > 1.0 for c in res["cases"].values())
    print(json.dumps(res), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
