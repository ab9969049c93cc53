// Filtered link ranks for the inner-product scorer (LLP.py:20 and the MRR / Hits@K protocol
// around it): for query position b with target candidate t_b,
//   greater[b] = #{ j != t_b, j not excluded for b : key(z_bj) > key(z_bt) }
//   equal[b]   = the same set with ==
// z_bj = sum_f Q[q_b, f] * T[j, f], without ever writing the (B, n) score matrix and for
// every K at once (rank = 1 + greater + a share of equal).
//
//   rank_inner    inner_tile.h's streamed tile with a counting epilogue.  A block owns a
//                 tile of 128 query rows, resident as MFMA A operands (wave w: rows
//                 32 w .. +31, all 64 candidates of a tile), and streams its range of
//                 candidates; a logit is one accumulation chain ordered by f alone, through
//                 the one mma_chunk topk_inner_kernel runs, so the logits are the ones it
//                 reports, bit for bit.
//                 Before its range a block stages the rows T[t_b] of its own query tile as
//                 two gathered candidate tiles, runs them through the same path and keeps the
//                 diagonal: the target's logit comes from the same chain, a candidate row
//                 bytewise equal to the target row ties with it exactly.  Each lane then
//                 holds the two thresholds of its 8 rows in registers; per logit the epilogue
//                 is one integer image, two compares and two counter bumps.  With an
//                 exclusion list each row keeps a cursor to its next excluded candidate (the
//                 lists ascend, and so do the tiles); an excluded candidate is counted like
//                 any other and taken out again by the lane that holds it: a cursor step
//                 per list entry, no search in the loop.  bf16: two
//                 blocks share a CU (at most 256 VGPRs), so one block's compares run under
//                 the other's MFMAs; fp32 holds twice the A registers and runs one block a
//                 CU (by instruction count its MFMAs take 8x the compares' cycles at F = 128).
//   rank_finish   sums the column splits' partial counts (uint32, ws) into the int64
//                 outputs, writes -1 / -1 for rows without a rank and raises *err.
//   rank_summary  MRR / mean-rank / Hits@K sums of the counts: integers, and one fp64 sum
//                 in a fixed order (lanes stride, xor tree, waves in order, blocks in order).
//
// Order: order_key.h's rk_image -- topk.hip's order (-0.0 folded onto +0.0, +inf highest,
// every NaN below -inf and all NaNs equal among themselves) in the shifted form that makes the
// NaNs the lowest contiguous range.  Integer compares and integer adds only, ordinary
// vector stores, no atomics: the result does not depend on the order of execution or on the
// split count.
#include "inner_tile.h"
#include "order_key.h"

namespace msha {

using namespace inner;

constexpr int kRkQT = 128;        // query rows per block
constexpr int kRkNC = kCT / 16;   // 16-candidate groups a wave holds: all of a tile

struct RkArgs {
  int64_t n_q, rows_q, ldq, ldt, n_cand, col_offset, per_split;
  const void* Q;
  const int64_t* qi;
  const void* T;
  const int64_t* target;
  const float* tl_in;
  const int32_t* excl_rowptr;
  const int32_t* excl_col;
  int F, splits;
  float* out_logit;
  uint32_t* part;  // (splits, n_q, 2): greater, equal of each split
};

// does query position b have a rank; bits: 1 stray qi, 2 target not local and no logit given
__device__ __forceinline__ int rk_row_fault(const RkArgs& a, int64_t b, int64_t* tloc) {
  const int64_t qrow = a.qi != nullptr ? a.qi[b] : b;
  *tloc = -1;
  if ((uint64_t)qrow >= (uint64_t)a.rows_q) return 1;
  const int64_t t = a.target[b] - a.col_offset;
  if ((uint64_t)t < (uint64_t)a.n_cand) {
    *tloc = t;
    return 0;
  }
  return a.tl_in != nullptr ? 0 : 2;
}

template <typename T, bool EXCL>
__global__ void __launch_bounds__(kThreads, sizeof(T) == 2 ? 2 : 1)
    rank_inner_kernel(RkArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char chunks[2 * kChunk];
  __shared__ int s_tloc[kRkQT];   // the row's target as a local candidate, or -1
  __shared__ int s_live[kRkQT];   // the row has a rank
  __shared__ float s_tz[kRkQT];   // the logit it is ranked against
  __shared__ float s_self[kRkQT]; // the local target's own logit from the chain

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int rb = w * 32;
  const int64_t q0 = (int64_t)blockIdx.x * kRkQT;
  const int split = blockIdx.y;
  const Width wd = width<T>(a.F);

  if (tid < kRkQT) {
    const int64_t b = q0 + tid;
    int64_t tloc = -1;
    int live = 0;
    float z = __builtin_nanf("");
    if (b < a.n_q) {
      live = rk_row_fault(a, b, &tloc) == 0 ? 1 : 0;
      if (!live) tloc = -1;
      if (live && a.tl_in != nullptr) z = a.tl_in[b];
    }
    s_tloc[tid] = (int)tloc;
    s_live[tid] = live;
    s_tz[tid] = z;
    s_self[tid] = 0.f;
  }

  // ---- the query tile: A operands, resident.  Validity is decided from qi[b] alone.
  uint4 areg[2][Geo<T>::NSTEP];
  int qst[2];
  load_queries<T>(areg, qst, a.Q, a.qi, a.rows_q, a.ldq, a.n_q, q0 + rb, wd.fbytes);

  f32x4 acc[2][kRkNC];
  const Range rg = split_range(split, a.per_split, a.n_cand);
  const int64_t j_begin = rg.j_begin, j_end = rg.j_end, ntiles = rg.ntiles;
  const int64_t total = ntiles * wd.nch;
  uint4 stg[4];

  // ---- the targets' own logits: rows T[t_b] of this tile as two gathered candidate tiles;
  // candidate c of gathered tile gt is the target of row 64 gt + c, so the diagonal sits in
  // wave w (gt == w >> 1), group 2 (w & 1) + r, at the lanes with n == 4 g + i
  __syncthreads();
#pragma unroll 1
  for (int gt = 0; gt < kRkQT / kCT; ++gt) {
    zero_acc<kRkNC>(acc);
#pragma unroll
    for (int ch = 0; ch < Geo<T>::NCH; ++ch) {
      if (ch < wd.nch) {
        load_stage<T>(stg, a.T, a.ldt, wd.fbytes,
                      [&](int c) -> int64_t { return s_tloc[gt * kCT + c]; }, a.n_cand, ch);
        store_stage(chunks, stg);
        __syncthreads();
        mma_chunk<T, kRkNC>(acc, areg, chunks, ch, wd.nsteps, 0, n, g);
        __syncthreads();
      }
    }
    if ((w >> 1) == gt) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < kRkNC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c == 2 * (w & 1) + r && n == 4 * g + i) s_self[rb + 16 * r + n] = acc[r][c][i];
    }
  }
  __syncthreads();
  if (tid < kRkQT) {
    if (a.tl_in == nullptr && s_live[tid]) s_tz[tid] = s_self[tid];
    const int64_t b = q0 + tid;
    if (split == 0 && b < a.n_q && a.out_logit != nullptr) a.out_logit[b] = s_tz[tid];
  }
  __syncthreads();

  // ---- per lane: thresholds and counters of its rows rb + 16 r + 4 g + i, k = 4 r + i
  uint32_t lo[8], hi[8], ge[8], gtc[8];
  unsigned livebits = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int row = rb + 16 * (k >> 2) + 4 * g + (k & 3);
    rk_bracket(s_tz[row], &lo[k], &hi[k]);
    if (s_live[row]) livebits |= 1u << k;
    ge[k] = 0u;
    gtc[k] = 0u;
  }

  // exclusion cursors: tiles arrive in ascending order and the lists are ascending, so each
  // row keeps the position and the value of its next excluded candidate (none: INT32_MAX)
  int32_t xpos[8], xnext[8];
  if (EXCL) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      xpos[k] = 0;
      xnext[k] = 0x7fffffff;
      if ((livebits >> k) & 1u) {
        const int64_t b = q0 + rb + 16 * (k >> 2) + 4 * g + (k & 3);
        const int32_t end = a.excl_rowptr[b + 1];
        xpos[k] = lower_bound(a.excl_col, a.excl_rowptr[b], end, j_begin);
        if (xpos[k] < end) xnext[k] = a.excl_col[xpos[k]];
      }
    }
  }

  // the streaming loop (its shape is topk_inner_kernel's: stage to LDS, one barrier, the next
  // stage's loads issued, the chunk's MFMAs under them)
  auto load = [&](int64_t j0, int ch) {
    load_stage<T>(stg, a.T, a.ldt, wd.fbytes, [=](int c) { return j0 + c; }, j_end, ch);
  };
  if (total > 0) load(j_begin, 0);
  int64_t it_no = 0;

  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = j_begin + t * kCT;
    zero_acc<kRkNC>(acc);
#pragma unroll
    for (int ch = 0; ch < Geo<T>::NCH; ++ch) {
      if (ch < wd.nch) {
        unsigned char* img = chunks + (it_no & 1) * kChunk;
        store_stage(img, stg);
        __syncthreads();
        ++it_no;
        if (it_no < total) {
          if (ch + 1 < wd.nch) load(j0, ch + 1);
          else load(j0 + kCT, 0);
        }
        mma_chunk<T, kRkNC>(acc, areg, img, ch, wd.nsteps, 0, n, g);
      }
    }

    // ---- count: C/D layout col = lane & 15 (candidate), row = (lane >> 4) * 4 + reg
    const int left = (int)min((int64_t)kCT, j_end - j0);  // candidates of this tile
    if (left == kCT) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < kRkNC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const uint32_t img = rk_image(acc[r][c][i]);
            ge[4 * r + i] += img >= lo[4 * r + i] ? 1u : 0u;
            gtc[4 * r + i] += img > hi[4 * r + i] ? 1u : 0u;
          }
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < kRkNC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k = 4 * r + i;
            const uint32_t img = rk_image(acc[r][c][i]);
            const bool on = 16 * c + n < left;
            ge[k] += (on && img >= lo[k]) ? 1u : 0u;
            gtc[k] += (on && img > hi[k]) ? 1u : 0u;
          }
    }
    // the row's excluded candidates inside this tile were counted like any other: the lane
    // that holds one takes it out again (a cursor step per list entry, no search)
    if (EXCL) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 4 * r + i;
          while ((int64_t)xnext[k] < j0 + kCT) {
            const int32_t cur = xnext[k];
            const int e = (int)(cur - j0);
            if (e >= 0 && e < left && (e & 15) == n) {
              const int c = e >> 4;
              const float v = c == 0 ? acc[r][0][i] : c == 1 ? acc[r][1][i]
                            : c == 2 ? acc[r][2][i] : acc[r][3][i];
              const uint32_t img = rk_image(v);
              ge[k] -= img >= lo[k] ? 1u : 0u;
              gtc[k] -= img > hi[k] ? 1u : 0u;
            }
            const int32_t end = a.excl_rowptr[q0 + rb + 16 * r + 4 * g + i + 1];
            do {  // the next entry, past duplicates
              ++xpos[k];
              xnext[k] = xpos[k] < end ? a.excl_col[xpos[k]] : 0x7fffffff;
            } while (xnext[k] == cur);
          }
        }
    }
  }

  // ---- per row: the 16 lanes' counts, less the target itself where this split counted it
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      ge[k] += __shfl_xor(ge[k], o);
      gtc[k] += __shfl_xor(gtc[k], o);
    }
  }
  if (n == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int row = rb + 16 * (k >> 2) + 4 * g + (k & 3);
      const int64_t b = q0 + row;
      if (b < a.n_q) {
        uint32_t cge = ge[k], cgt = gtc[k];
        const int tl = s_tloc[row];
        if (((livebits >> k) & 1u) && tl >= j_begin && tl < j_end) {
          bool counted = true;
          if (EXCL) counted = !excluded(a.excl_rowptr, a.excl_col, b, tl);
          if (counted) {
            const uint32_t img = rk_image(s_self[row]);
            cge -= img >= lo[k] ? 1u : 0u;
            cgt -= img > hi[k] ? 1u : 0u;
          }
        }
        uint32_t* out = a.part + ((int64_t)split * a.n_q + b) * 2;
        out[0] = cgt;
        out[1] = cge - cgt;
      }
    }
  }
}

// the splits' partial counts -> int64 outputs; rows without a rank -> -1 / -1 and *err
__global__ void __launch_bounds__(kThreads) rank_finish_kernel(RkArgs a, int64_t* out_greater,
                                                                 int64_t* out_equal,
                                                                 int32_t* err) {
  const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.n_q) return;
  int64_t tloc;
  const int fault = rk_row_fault(a, b, &tloc);
  if (fault != 0) {
    out_greater[b] = -1;
    out_equal[b] = -1;
    if (a.out_logit != nullptr) a.out_logit[b] = __builtin_nanf("");
    if (err != nullptr) atomicOr(err, fault);
    return;
  }
  int64_t gsum = 0, esum = 0;
  for (int s = 0; s < a.splits; ++s) {
    const uint32_t* p = a.part + ((int64_t)s * a.n_q + b) * 2;
    gsum += p[0];
    esum += p[1];
  }
  out_greater[b] = gsum;
  out_equal[b] = esum;
}

// ------------------------------------------------------------- rank_summary ----

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / kWave;
constexpr int kRsMaxK = 8;
constexpr int kRsSlots = 16;         // 64-bit words of a block's partial
constexpr int64_t kRsSpan = 16384;   // rows a block sums, up to kRsMaxBlocks blocks
constexpr int kRsMaxBlocks = 256;

struct RsArgs {
  int64_t n, span;
  const int64_t* greater;
  const int64_t* equal;
  int ties, nk;
  int64_t k2[kRsMaxK];  // 2 k
};

// partial of block x at part[x * kRsSlots + ...]: [0, nk) hits, [8] valid rows, [9] sum of
// 2 rank, [10] the bits of the fp64 sum of 1 / rank
__global__ void __launch_bounds__(kRsThreads) rank_summary_kernel(RsArgs a, int64_t* part) {
  __shared__ int64_t s_i[kRsWaves][kRsMaxK + 2];
  __shared__ double s_rr[kRsWaves];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * a.span, r1 = min(a.n, r0 + a.span);
  int64_t acc[kRsMaxK + 2];
#pragma unroll
  for (int k = 0; k < kRsMaxK + 2; ++k) acc[k] = 0;
  double rr = 0.0;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += kRsThreads) {
    const int64_t gr = a.greater[i], eq = a.equal[i];
    if (gr < 0) continue;
    const int64_t r2 = 2 + 2 * gr + (a.ties == 0 ? 0 : a.ties == 1 ? eq : 2 * eq);
#pragma unroll
    for (int k = 0; k < kRsMaxK; ++k)
      if (k < a.nk && r2 <= a.k2[k]) acc[k] += 1;
    acc[kRsMaxK] += 1;
    acc[kRsMaxK + 1] += r2;
    rr += 2.0 / (double)r2;
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
#pragma unroll
    for (int k = 0; k < kRsMaxK + 2; ++k) acc[k] += __shfl_xor(acc[k], o);
    rr += __shfl_xor(rr, o);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kRsMaxK + 2; ++k) s_i[w][k] = acc[k];
    s_rr[w] = rr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t* out = part + (int64_t)blockIdx.x * kRsSlots;
    double s = 0.0;
    for (int ww = 0; ww < kRsWaves; ++ww) s += s_rr[ww];
    for (int k = 0; k < kRsMaxK + 2; ++k) {
      int64_t v = 0;
      for (int ww = 0; ww < kRsWaves; ++ww) v += s_i[ww][k];
      out[k] = v;
    }
    out[kRsMaxK + 2] = __double_as_longlong(s);
  }
}

// the blocks' partials, in block order
__global__ void __launch_bounds__(kWave) rank_summary_finish_kernel(int nb, int nk,
                                                                    const int64_t* part,
                                                                    int64_t* out_counts,
                                                                    double* out_rr) {
  if (threadIdx.x != 0) return;
  int64_t acc[kRsMaxK + 2];
  for (int k = 0; k < kRsMaxK + 2; ++k) acc[k] = 0;
  double rr = 0.0;
  for (int x = 0; x < nb; ++x) {
    const int64_t* p = part + (int64_t)x * kRsSlots;
    for (int k = 0; k < kRsMaxK + 2; ++k) acc[k] += p[k];
    rr += __longlong_as_double(p[kRsMaxK + 2]);
  }
  for (int k = 0; k < nk; ++k) out_counts[k] = acc[k];
  out_counts[nk] = acc[kRsMaxK];
  out_counts[nk + 1] = acc[kRsMaxK + 1];
  out_rr[0] = rr;
}

// blocks per CU: 2 for bf16 tables, 1 for fp32 (the kernel's launch bounds)
static int rk_default_splits(int64_t n_q, int64_t n_cand, int32_t dtype) {
  if (n_q <= 0 || n_cand <= 0) return 1;
  const int64_t tiles = (n_q + kRkQT - 1) / kRkQT;
  int64_t s = kCUs * (dtype == MSHA_DTYPE_BF16 ? 2 : 1) / tiles;
  s = s < n_cand / 512 ? s : n_cand / 512;  // a split has at least 512 candidates
  return (int)(s < 1 ? 1 : s);
}

static int rs_blocks(int64_t n) {
  const int64_t nb = (n + kRsSpan - 1) / kRsSpan;
  return (int)(nb < 1 ? 1 : nb > kRsMaxBlocks ? kRsMaxBlocks : nb);
}

}  // namespace msha

using namespace msha;

extern "C" int msha_rank_inner_supported(int32_t feat, int32_t dtype) {
  return supported(feat, dtype) ? 1 : 0;
}

extern "C" int msha_rank_inner_splits(int64_t n_q, int64_t n_cand, int32_t feat, int32_t dtype) {
  if (!supported(feat, dtype)) return 1;
  return rk_default_splits(n_q, n_cand, dtype);
}

extern "C" size_t msha_rank_inner_workspace_size(int64_t n_q, int64_t n_cand, int32_t splits) {
  if (n_q < 0 || n_cand < 0) return 0;
  if (splits <= 0) splits = rk_default_splits(n_q, n_cand, MSHA_DTYPE_BF16);  // the larger
  return 256 + align256((size_t)n_q * splits * 2 * sizeof(uint32_t));
}

extern "C" int msha_rank_inner(int64_t n_q, int32_t feat, int32_t dtype, const void* Q,
                               int64_t ldq, const int64_t* qi, int64_t rows_q, const void* T,
                               int64_t ldt, int64_t n_cand, int64_t col_offset,
                               const int64_t* target, const float* target_logit_in,
                               const int32_t* excl_rowptr, const int32_t* excl_col,
                               int32_t splits, int64_t* out_greater, int64_t* out_equal,
                               float* out_logit, int32_t* err, void* ws, size_t ws_bytes,
                               msha_stream_t stream) {
  const int rc = check_tables("rank_inner", dtype, true, feat, n_q, n_cand, rows_q, splits,
                              excl_rowptr, excl_col,
                              target != nullptr && out_greater != nullptr && out_equal != nullptr,
                              Q, ldq, qi, T, ldt);
  if (rc != MSHA_OK || n_q == 0) return rc;
  splits = clamp_splits(splits, rk_default_splits(n_q, n_cand, dtype), n_cand);
  const size_t need = align256((size_t)n_q * splits * 2 * sizeof(uint32_t));
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws % 16) == 0,
                 "rank_inner: workspace too small (msha_rank_inner_workspace_size) or unaligned");
  const int64_t tiles = (n_q + kRkQT - 1) / kRkQT;
  MSHA_ARG_CHECK(tiles < ((int64_t)1 << 31), "rank_inner: too many queries");
  RkArgs a;
  a.n_q = n_q;
  a.rows_q = rows_q;
  a.ldq = ldq;
  a.ldt = ldt;
  a.n_cand = n_cand;
  a.col_offset = col_offset;
  a.per_split = per_split(n_cand, splits);
  a.Q = Q;
  a.qi = qi;
  a.T = T;
  a.target = target;
  a.tl_in = target_logit_in;
  a.excl_rowptr = excl_rowptr;
  a.excl_col = excl_col;
  a.F = feat;
  a.splits = splits;
  a.out_logit = out_logit;
  a.part = reinterpret_cast<uint32_t*>(ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, (unsigned)splits);
  const bool ex = excl_rowptr != nullptr;
  if (dtype == MSHA_DTYPE_BF16) {
    if (ex)
      hipLaunchKernelGGL((rank_inner_kernel<bf16_t, true>), grid, dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL((rank_inner_kernel<bf16_t, false>), grid, dim3(kThreads), 0, s, a);
  } else {
    if (ex)
      hipLaunchKernelGGL((rank_inner_kernel<float, true>), grid, dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL((rank_inner_kernel<float, false>), grid, dim3(kThreads), 0, s, a);
  }
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((n_q + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, a, out_greater, out_equal, err);
  return check_launch("rank_inner");
}

extern "C" size_t msha_rank_summary_workspace_size(int64_t n) {
  if (n < 0) return 0;
  return 256 + align256((size_t)rs_blocks(n) * kRsSlots * sizeof(int64_t));
}

extern "C" int msha_rank_summary(int64_t n, const int64_t* greater, const int64_t* equal,
                                 int32_t ties, const int64_t* ks, int32_t nk,
                                 int64_t* out_counts, double* out_rr, void* ws, size_t ws_bytes,
                                 msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 0, "rank_summary: negative size");
  MSHA_ARG_CHECK(ties >= 0 && ties <= 2,
                 "rank_summary: ties must be 0 (optimistic), 1 (mean) or 2 (pessimistic)");
  MSHA_ARG_CHECK(nk >= 0 && nk <= kRsMaxK && (nk == 0 || ks != nullptr),
                 "rank_summary: at most 8 values of k");
  MSHA_ARG_CHECK(out_counts != nullptr && out_rr != nullptr &&
                     (n == 0 || (greater != nullptr && equal != nullptr)),
                 "rank_summary: null pointer");
  const int nb = rs_blocks(n);
  const size_t need = align256((size_t)nb * kRsSlots * sizeof(int64_t));
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws % 16) == 0,
                 "rank_summary: workspace too small (msha_rank_summary_workspace_size) or "
                 "unaligned");
  RsArgs a;
  a.n = n;
  a.span = (n + nb - 1) / nb;
  a.greater = greater;
  a.equal = equal;
  a.ties = ties;
  a.nk = nk;
  for (int k = 0; k < kRsMaxK; ++k) {
    a.k2[k] = 0;
    if (k < nk) {
      MSHA_ARG_CHECK(ks[k] >= 1 && ks[k] < ((int64_t)1 << 61), "rank_summary: k must be >= 1");
      a.k2[k] = 2 * ks[k];
    }
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t* part = reinterpret_cast<int64_t*>(ws);
  hipLaunchKernelGGL(rank_summary_kernel, dim3(nb), dim3(kRsThreads), 0, s, a, part);
  hipLaunchKernelGGL(rank_summary_finish_kernel, dim3(1), dim3(kWave), 0, s, nb, (int)nk, part,
                     out_counts, out_rr);
  return check_launch("rank_summary");
}
