// The GraphSAGE baseline of the paper's comparison table (SGAE.py:41-56) on the rows of a
// sparse adjacency, forward and backward, with no dense (B, M) operand, no matrix pipe and no
// float atomics:
//
//   x  = Sfeatures[source_index]                    (B, in)
//   z1 = relu(x W1^T + b1)                          (B, M)
//   y  = adj[source_index] * z1                     (B, M)   hidden == M
//   z2 = relu(y W2^T + b2)                          (B, out)
//   logp = log_softmax(z2, dim=1)
//
// y[b, j] is zero wherever adj[src_b, j] is, so both Linears collapse onto the CSR row of
// src_b: for each edge (src_b, j) with value a, y_j = a relu(x_b . W1[j, :] + b1[j]) and
// p2 += y_j W2[:, j].  Only edges with adj > 0 are in the Graph: negative adjacency entries
// are not supported (the reference's normalised adjacency has none).
//
//   sage_fwd        one launch.  W1, b1, W2^T, b2 staged once per block in LDS; 16 lanes per
//                   batch entry gather the table row, walk the CSR row, keep p2 in registers,
//                   apply ReLU and the row's log-sum-exp and write logp.  Nothing is saved.
//   sage_bwd        rows     the entry recomputed (same arithmetic: the same ReLU branches),
//                            dr = (dlogp - exp(logp) sum dlogp) [p2 > 0], then per edge
//                            dy_j = W2[:, j] . dr, dz1_j = a dy_j [p1_j > 0], dx_b += dz1_j
//                            W1[j, :]; dr (B, out), the edges' (dz1_j, y_j) and dx (B, in)
//                            go to the workspace.
//                   wgrad    blocks own runs of batch entries; wave w of a block owns the
//                            columns j = w (mod 4) of the block's LDS accumulators and walks
//                            the run's edges in batch order, so each accumulator has one
//                            writer and one order; a block's sums are a partial.
//                   finish   the partials added in a fixed order (16 interleaved runs in
//                            block order, then the 16 sums in order).
//                   table    dSfeatures[r] = sum of dx_b over the entries b with src_b = r in
//                            batch order, under the incidence plan of the pair list (src,
//                            src) (msha_pair_plan: row r holds each of its entries b and
//                            b + B, ascending; the ends >= B are skipped), every row written
//                            (zeros outside the batch).
//
// An entry whose source lies outside [0, n) is padding: its logp row is NaN and it adds to no
// gradient.  A virtual (empty) row is skipped through rowflag: y = 0, logp =
// log_softmax(relu(b2)), dx = 0.  Every index is range-checked before a load goes through it.
#include <type_traits>

#include "common.h"
#include "pair_grad.h"

namespace msha {

constexpr int kSgThreads = 256;
constexpr int kSgWaves = kSgThreads / kWave;
constexpr int kSgGroup = 16;                    // lanes per batch entry
constexpr int kSgTile = kSgThreads / kSgGroup;  // entries per block round
constexpr int kSgMaxW = 64;                     // widest in / M / out
constexpr int kSgPer = kSgMaxW / kSgGroup;      // elements of a row per lane, at most
constexpr int kSgFwdBlocks = 1024;              // forward / row-pass grid cap
constexpr int kSgWgBlocks = 512;                // weight-gradient partials, at most (2 a CU)

struct SgArgs {
  int64_t B, n, ld, n_edges;
  int in, M, out;
  const float* table;
  const int64_t* src;
  const int32_t* rowptr;
  const int32_t* col;
  const uint8_t* rowflag;
  const float* vals;
  const float *W1, *b1, *W2, *b2;
};

// a batch entry as its 16 lanes hold it: lane q has elements q, q + 16, .. of the table row
// (slot k < width / 16 of a lane: the widths are multiples of 16, so the test is wave-uniform)
struct SgEntry {
  bool ok;      // the source is inside the table
  int e0, deg;  // its CSR row (deg 0: virtual, empty or not a row of this graph)
  float x[kSgPer];
};

// W1 as it is, W2 transposed ([j][o]: a lane group reads consecutive words either way)
__device__ __forceinline__ void sg_stage_params(const SgArgs& a, float* sW1, float* sW2t,
                                                float* sb1, float* sb2) {
  for (int t = threadIdx.x; t < a.M * a.in; t += kSgThreads) sW1[t] = a.W1[t];
  for (int t = threadIdx.x; t < a.out * a.M; t += kSgThreads) {
    const int o = t / a.M, j = t - o * a.M;
    sW2t[j * a.out + o] = a.W2[t];
  }
  if ((int)threadIdx.x < a.M) sb1[threadIdx.x] = a.b1[threadIdx.x];
  if ((int)threadIdx.x < a.out) sb2[threadIdx.x] = a.b2[threadIdx.x];
}

__device__ __forceinline__ SgEntry sg_entry(const SgArgs& a, int64_t b, int64_t bend, int q) {
  SgEntry en;
  en.ok = false;
  en.e0 = en.deg = 0;
#pragma unroll
  for (int k = 0; k < kSgPer; ++k) en.x[k] = 0.f;
  if (b < bend) {
    const int64_t s = a.src[b];
    if ((uint64_t)s < (uint64_t)a.n) {
      en.ok = true;
#pragma unroll
      for (int k = 0; k < kSgPer; ++k)
        if (k < a.in / kSgGroup) en.x[k] = a.table[s * a.ld + q + kSgGroup * k];
      if (a.rowflag == nullptr || a.rowflag[s] == 0) {
        const int e0 = a.rowptr[s], e1 = a.rowptr[s + 1];
        if (e0 >= 0 && e1 >= e0 && (int64_t)e1 <= a.n_edges && e1 - e0 <= a.M) {
          en.e0 = e0;
          en.deg = e1 - e0;
        }
      }
    }
  }
  return en;
}

// edge k of the entry: column 0 with value 0 past the row's end or for a stray column
__device__ __forceinline__ void sg_edge(const SgArgs& a, const SgEntry& en, int k, int& j,
                                        float& av) {
  j = 0;
  av = 0.f;
  if (k < en.deg) {
    const int c = a.col[en.e0 + k];
    if ((unsigned)c < (unsigned)a.M) {
      j = c;
      av = a.vals[en.e0 + k];
    }
  }
}

// its column alone (k < deg)
__device__ __forceinline__ int sg_col(const SgArgs& a, const SgEntry& en, int k) {
  const int c = a.col[en.e0 + k];
  return (unsigned)c < (unsigned)a.M ? c : 0;
}

__device__ __forceinline__ float sg_group_max(float v) {
#pragma unroll
  for (int o = 1; o < kSgGroup; o <<= 1) v = fmaxf(v, xor_shfl(v, o));
  return v;
}

// the largest degree among the wave's four entries: the edge loops run to it in every lane,
// so the lane-group sums inside them are taken with the whole wave active
__device__ __forceinline__ int sg_wave_max(int d) {
  d = max(d, __shfl_xor(d, 16));
  d = max(d, __shfl_xor(d, 32));
  return d;
}

// p1_j = x . W1[j, :] + b1[j]: the lane's elements in order, the 16 lanes by an xor tree
__device__ __forceinline__ float sg_p1(const SgArgs& a, const SgEntry& en, const float* sW1,
                                       const float* sb1, int j, int q) {
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < kSgPer; ++k)
    if (k < a.in / kSgGroup) d = fmaf(en.x[k], sW1[j * a.in + q + kSgGroup * k], d);
  return group_sum<kSgGroup>(d) + sb1[j];
}

// p2 = sum over the row's edges in CSR order of y_j W2[:, j], then + b2; lane q holds
// outputs q, q + 16, ..
__device__ __forceinline__ void sg_forward(const SgArgs& a, const SgEntry& en, int maxdeg,
                                           const float* sW1, const float* sW2t,
                                           const float* sb1, const float* sb2, int q,
                                           float (&p2)[kSgPer]) {
#pragma unroll
  for (int k = 0; k < kSgPer; ++k) p2[k] = 0.f;
  for (int k = 0; k < maxdeg; ++k) {
    int j;
    float av;
    sg_edge(a, en, k, j, av);
    const float y = av * fmaxf(sg_p1(a, en, sW1, sb1, j, q), 0.f);
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk)
      if (kk < a.out / kSgGroup)
        p2[kk] = fmaf(y, sW2t[j * a.out + q + kSgGroup * kk], p2[kk]);
  }
#pragma unroll
  for (int kk = 0; kk < kSgPer; ++kk)
    if (kk < a.out / kSgGroup) p2[kk] += sb2[q + kSgGroup * kk];
}

__global__ void __launch_bounds__(kSgThreads) sage_fwd_kernel(SgArgs a, float* __restrict__ logp) {
  __shared__ float sW1[kSgMaxW * kSgMaxW], sW2t[kSgMaxW * kSgMaxW], sb1[kSgMaxW], sb2[kSgMaxW];
  sg_stage_params(a, sW1, sW2t, sb1, sb2);
  __syncthreads();
  const int g = threadIdx.x / kSgGroup, q = threadIdx.x % kSgGroup;
  for (int64_t base = (int64_t)blockIdx.x * kSgTile; base < a.B;
       base += (int64_t)gridDim.x * kSgTile) {
    const int64_t b = base + g;
    const SgEntry en = sg_entry(a, b, a.B, q);
    const int maxdeg = sg_wave_max(en.deg);
    float p2[kSgPer];
    sg_forward(a, en, maxdeg, sW1, sW2t, sb1, sb2, q, p2);
    // log_softmax of relu(p2): the row's maximum is >= 0, which the unused slots hold
    float r[kSgPer], m = 0.f;
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk) {
      r[kk] = kk < a.out / kSgGroup ? fmaxf(p2[kk], 0.f) : 0.f;
      m = fmaxf(m, r[kk]);
    }
    m = sg_group_max(m);
    float s = 0.f;
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk)
      if (kk < a.out / kSgGroup) s += expf(r[kk] - m);
    const float lse = m + logf(group_sum<kSgGroup>(s));
    if (b < a.B) {
#pragma unroll
      for (int kk = 0; kk < kSgPer; ++kk)
        if (kk < a.out / kSgGroup)
          logp[b * a.out + q + kSgGroup * kk] = en.ok ? r[kk] - lse : __builtin_nanf("");
    }
  }
}

// The backward's row pass.  dr (B, out); ez / ey (B, M): slot k of row b is edge k of the
// entry's CSR row (dz1_j and y_j), slots past the degree unwritten; dx (B, in), nullable.
__global__ void __launch_bounds__(kSgThreads) sage_bwd_rows_kernel(
    SgArgs a, const float* __restrict__ logp, const float* __restrict__ dlogp,
    float* __restrict__ dr_out, float* __restrict__ ez, float* __restrict__ ey,
    float* __restrict__ dx) {
  __shared__ float sW1[kSgMaxW * kSgMaxW], sW2t[kSgMaxW * kSgMaxW], sb1[kSgMaxW], sb2[kSgMaxW];
  sg_stage_params(a, sW1, sW2t, sb1, sb2);
  __syncthreads();
  const int g = threadIdx.x / kSgGroup, q = threadIdx.x % kSgGroup;
  for (int64_t base = (int64_t)blockIdx.x * kSgTile; base < a.B;
       base += (int64_t)gridDim.x * kSgTile) {
    const int64_t b = base + g;
    const SgEntry en = sg_entry(a, b, a.B, q);
    const int maxdeg = sg_wave_max(en.deg);
    float p2[kSgPer];
    sg_forward(a, en, maxdeg, sW1, sW2t, sb1, sb2, q, p2);
    float gv[kSgPer], lp[kSgPer], gs = 0.f;
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk) {
      const bool on = en.ok && kk < a.out / kSgGroup;
      gv[kk] = on ? dlogp[b * a.out + q + kSgGroup * kk] : 0.f;
      lp[kk] = on ? logp[b * a.out + q + kSgGroup * kk] : 0.f;
      gs += gv[kk];
    }
    gs = group_sum<kSgGroup>(gs);
    float dr[kSgPer];
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk) {
      const bool on = en.ok && kk < a.out / kSgGroup && p2[kk] > 0.f;
      dr[kk] = on ? gv[kk] - expf(lp[kk]) * gs : 0.f;
    }
    if (b < a.B) {
#pragma unroll
      for (int kk = 0; kk < kSgPer; ++kk)
        if (kk < a.out / kSgGroup) dr_out[b * a.out + q + kSgGroup * kk] = dr[kk];
    }
    float dxa[kSgPer];
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk) dxa[kk] = 0.f;
    for (int k = 0; k < maxdeg; ++k) {
      int j;
      float av;
      sg_edge(a, en, k, j, av);
      const float p1 = sg_p1(a, en, sW1, sb1, j, q);
      float dy = 0.f;
#pragma unroll
      for (int kk = 0; kk < kSgPer; ++kk)
        if (kk < a.out / kSgGroup)
          dy = fmaf(sW2t[j * a.out + q + kSgGroup * kk], dr[kk], dy);
      dy = group_sum<kSgGroup>(dy);
      const float dz1 = p1 > 0.f ? av * dy : 0.f;
      if (q == 0 && k < en.deg) {
        ez[b * a.M + k] = dz1;
        ey[b * a.M + k] = av * fmaxf(p1, 0.f);
      }
#pragma unroll
      for (int kk = 0; kk < kSgPer; ++kk)
        if (kk < a.in / kSgGroup)
          dxa[kk] = fmaf(dz1, sW1[j * a.in + q + kSgGroup * kk], dxa[kk]);
    }
    if (dx != nullptr && b < a.B) {
#pragma unroll
      for (int kk = 0; kk < kSgPer; ++kk)
        if (kk < a.in / kSgGroup) dx[b * a.in + q + kSgGroup * kk] = dxa[kk];
    }
  }
}

// Block k owns the batch entries [k per, (k + 1) per) and one partial of
// dW1 (M in) | db1 (M) | dW2 (out M) | db2 (out).  A round stages 16 entries (x, dr and the
// edges' column, dz1 and y) in LDS; wave w then walks the round's edges in batch order and
// adds those of the columns j = w (mod 4) into the block's accumulators: dW1[j, :] +=
// dz1_j x, db1[j] += dz1_j, dW2[:, j] += y_j dr (db2 += dr by wave 0, once an entry).  An
// accumulator is written by one wave in one order: no atomics, and the partial is a function
// of the inputs and per alone.
__global__ void __launch_bounds__(kSgThreads) sage_wgrad_kernel(
    SgArgs a, int64_t per, const float* __restrict__ dr, const float* __restrict__ ez,
    const float* __restrict__ ey, float* __restrict__ part) {
  // acc[j] = dW1[j, :] | dW2[:, j] | db1[j] and tu[i] = x_i | dr_i | 1, one pitch: an edge is
  // acc[j][l] += (dz1 or y) tu[i][l] over l
  constexpr int kPitch = 2 * kSgMaxW + 1;
  __shared__ float acc[kSgMaxW * kPitch], ab2[kSgMaxW];
  __shared__ float tu[kSgTile][kPitch], tdz[kSgTile][kSgMaxW], ty[kSgTile][kSgMaxW];
  __shared__ int tj[kSgTile][kSgMaxW], tdeg[kSgTile];
  const int g = threadIdx.x / kSgGroup, q = threadIdx.x % kSgGroup;
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int in = a.in, M = a.M, out = a.out, P = in + out + 1;
  for (int t = threadIdx.x; t < M * P; t += kSgThreads) acc[t] = 0.f;
  if ((int)threadIdx.x < kSgMaxW) ab2[threadIdx.x] = 0.f;
  if ((int)threadIdx.x < kSgTile) tu[threadIdx.x][in + out] = 1.f;
  const int64_t b0 = (int64_t)blockIdx.x * per;
  const int nrun = (int)(min(a.B, b0 + per) - b0);  // (<= 0: an empty block of B = 0)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int r0 = 0; r0 < nrun; r0 += kSgTile) {
    __syncthreads();  // (the fills above / the previous round's walk)
    const int64_t b = b0 + r0 + g;
    const SgEntry en = sg_entry(a, r0 + g < nrun ? b : a.B, a.B, q);
#pragma unroll
    for (int kk = 0; kk < kSgPer; ++kk) {
      const int e = q + kSgGroup * kk;
      if (kk < in / kSgGroup) tu[g][e] = en.x[kk];
      if (kk < out / kSgGroup) tu[g][in + e] = en.ok ? dr[b * out + e] : 0.f;
    }
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int k = q; k < en.deg; k += kSgGroup) {
      tj[g][k] = sg_col(a, en, k);
      tdz[g][k] = ez[b * M + k];
      ty[g][k] = ey[b * M + k];
    }
    if (q == 0) tdeg[g] = en.deg;
    __syncthreads();
    const int cnt = min(kSgTile, nrun - r0);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = 0; i < cnt; ++i) {
      if (w == 0 && lane < out) ab2[lane] += tu[i][in + lane];
      // (the same word in every lane: kept scalar, so the walk's branches are wave-uniform)
      const int deg = __builtin_amdgcn_readfirstlane(tdeg[i]);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
      for (int k = 0; k < deg; ++k) {
        const int j = __builtin_amdgcn_readfirstlane(tj[i][k]);
        if ((j & (kSgWaves - 1)) != w) continue;
        const float dz = tdz[i][k], y = ty[i][k];
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int l = lane; l < P; l += kWave) {
          const float c = l >= in && l < in + out ? y : dz;
          acc[j * P + l] = fmaf(c, tu[i][l], acc[j * P + l]);
        }
      }
    }
  }
  __syncthreads();
  // wave w writes the rows j = w, w + 4, .. of acc to their places in the partial
  float* o = part + (int64_t)blockIdx.x * (M * in + M + out * M + out);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int j = w; j < M; j += kSgWaves) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int l = lane; l < P; l += kWave) {
      const float v = acc[j * P + l];
      if (l < in)
        o[j * in + l] = v;
      else if (l < in + out)
        o[M * in + M + (l - in) * M + j] = v;
      else
        o[M * in + j] = v;
    }
  }
  if ((int)threadIdx.x < out) o[M * in + M + out * M + threadIdx.x] = ab2[threadIdx.x];
}

// The blocks' partials in a fixed order: a block of the finish takes 16 elements; thread
// (q, e) adds the partials q, q + 16, .. of element e in order (16 consecutive words a load),
// then the 16 sums of an element are added in q order: a function of nblk alone.
__global__ void __launch_bounds__(kSgThreads) sage_wfinish_kernel(
    int64_t nblk, int len, int o1, int o2, int o3, const float* __restrict__ part,
    float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
    float* __restrict__ db2) {
  __shared__ float red[kSgTile][kSgGroup];
  const int q = threadIdx.x / kSgGroup, e = threadIdx.x % kSgGroup;
  const int j = (int)blockIdx.x * kSgGroup + e;
  float s = 0.f;
  if (j < len) {
#pragma unroll 4  // the loads of 4 partials in flight; the adds stay in order
    for (int64_t b = q; b < nblk; b += kSgTile) s += part[b * len + j];
  }
  red[q][e] = s;
  __syncthreads();
  if (q != 0 || j >= len) return;
  s = red[0][e];
#pragma unroll
  for (int k = 1; k < kSgTile; ++k) s += red[k][e];
  if (j < o1)
    dW1[j] = s;
  else if (j < o2)
    db1[j - o1] = s;
  else if (j < o3)
    dW2[j - o2] = s;
  else
    db2[j - o3] = s;
}

// dS[r] = the dx rows of r's batch entries in batch order, a float4 a thread.  The plan is
// that of the pair list (src, src): row r's range holds each entry b of r and b + B; the
// second ends are skipped.  Every row is written.  R (pair_grad.h): every table row to dS[r]
// (PgAllRows), or entry i of the plan's touched-row list to vals[i] (PgListRows: the loop runs
// to the list's capacity; an entry past the device count or outside the table is exact zeros).
template <typename R>
__global__ void __launch_bounds__(kSgThreads) sage_table_kernel(
    int64_t B, int64_t n, int in, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ ent, const float* __restrict__ dx, float* __restrict__ dS,
    R rows) {
  const int LPR = in / 4;
  const int64_t cnt = rows.count(n), total = rows.extent(n) * LPR;
  for (int64_t t = (int64_t)blockIdx.x * kSgThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kSgThreads) {
    const int64_t i = t / LPR;
    const int c = 4 * (int)(t % LPR);
    const int64_t r = rows.row(i, cnt);
    int64_t b = 0, e = 0;
    if ((uint64_t)r < (uint64_t)n) b = rowptr[r], e = rowptr[r + 1];
    if (b < 0 || e < b || e > 2 * B) b = e = 0;  // (not a plan of this list)
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t k = b; k < e; ++k) {
      const int64_t p = ent[k];
      if ((uint64_t)p < (uint64_t)B) {
        const float4 v = *reinterpret_cast<const float4*>(dx + p * in + c);
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
      }
    }
    *reinterpret_cast<float4*>(dS + i * in + c) = s;
  }
}

static bool sg_width(int32_t w) { return w == 16 || w == 32 || w == 64; }

static size_t sg_align(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr int64_t kSgMaxBatch = ((int64_t)1 << 30) - 1;  // msha_pair_plan's 2 B < 2^31

// weight-gradient blocks and their run of entries: a function of B alone
static int64_t sg_wg_blocks(int64_t B) {
  const int64_t tiles = B > 0 ? (B + kSgTile - 1) / kSgTile : 1;
  return tiles < kSgWgBlocks ? tiles : kSgWgBlocks;
}
static int64_t sg_wg_per(int64_t B) {
  const int64_t nblk = sg_wg_blocks(B);
  const int64_t per = ((B > 0 ? B : 1) + nblk - 1) / nblk;
  return (per + kSgTile - 1) / kSgTile * kSgTile;
}
static int sg_len(int32_t in, int32_t M, int32_t out) { return M * in + M + out * M + out; }

struct SgLayout {
  size_t dr, ez, ey, dx, part, prow, pent, ptab, pws, total;  // msha_sage_workspace_size
  size_t rws, rows_total;  // + msha_plan_rows' workspace: msha_sage_rows_workspace_size
};
static SgLayout sg_layout(int64_t B, int64_t n, int32_t in, int32_t M, int32_t out) {
  SgLayout L;
  size_t off = 0;
  L.dr = off;
  off += sg_align((size_t)B * out * 4);
  L.ez = off;
  off += sg_align((size_t)B * M * 4);
  L.ey = off;
  off += sg_align((size_t)B * M * 4);
  L.dx = off;
  off += sg_align((size_t)B * in * 4);
  L.part = off;
  off += sg_align((size_t)sg_wg_blocks(B) * sg_len(in, M, out) * 4);
  L.prow = off;
  off += sg_align((size_t)(n + 1) * 4);
  L.pent = off;
  off += sg_align((size_t)2 * B * 4 + 16);
  L.ptab = off;
  off += sg_align((size_t)2 * msha_pair_plan_chunk_slots(B) * 4 + 16);
  L.pws = off;
  off += sg_align(msha_pair_plan_workspace_size(B) + 16);
  L.total = off;
  L.rws = off;
  L.rows_total = off + sg_align(msha_plan_rows_workspace_size(n));
  return L;
}

static int sg_check(const char* name, const msha_graph* g, int64_t B, const int64_t* src,
                    int32_t in, int32_t out, const float* table, int64_t ld, const float* vals,
                    const float* W1, const float* b1, const float* W2, const float* b2) {
  const std::string nm(name);
  if (g == nullptr || g->rowptr == nullptr || g->n_rows < 1 || g->n_cols < 1 || g->n_edges < 0 ||
      (g->n_edges > 0 && (g->col == nullptr || vals == nullptr)))
    return fail(MSHA_ERR_ARG, nm + ": graph CSR or edge values missing");
  if (g->n_cols > kSgMaxW || !sg_width(in) || !sg_width((int32_t)g->n_cols) || !sg_width(out))
    return fail(MSHA_ERR_ARG, nm + ": unsupported widths: in, M = hidden and out must each be "
                                   "16, 32 or 64 (msha_sage_supported)");
  if (B < 0 || B > kSgMaxBatch || g->n_rows >= ((int64_t)1 << 31) - 1 ||
      g->n_edges >= ((int64_t)1 << 31))
    return fail(MSHA_ERR_ARG, nm + ": bad sizes (0 <= B < 2^30, rows and edges below 2^31)");
  if ((B > 0 && src == nullptr) || !table || !W1 || !b1 || !W2 || !b2)
    return fail(MSHA_ERR_ARG, nm + ": null pointer");
  if (ld < in) return fail(MSHA_ERR_ARG, nm + ": the table's row pitch is below its width");
  return MSHA_OK;
}

static SgArgs sg_args(const msha_graph* g, int64_t B, const int64_t* src, int32_t in, int32_t out,
                      const float* table, int64_t ld, const float* vals, const float* W1,
                      const float* b1, const float* W2, const float* b2) {
  SgArgs a;
  a.B = B; a.n = g->n_rows; a.ld = ld; a.n_edges = g->n_edges;
  a.in = in; a.M = (int)g->n_cols; a.out = out;
  a.table = table; a.src = src;
  a.rowptr = g->rowptr; a.col = g->col; a.rowflag = g->rowflag; a.vals = vals;
  a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2;
  return a;
}

}  // namespace msha

using namespace msha;

extern "C" int msha_sage_supported(int32_t in, int32_t M, int32_t out) {
  return sg_width(in) && sg_width(M) && sg_width(out) ? 1 : 0;
}

extern "C" size_t msha_sage_workspace_size(int64_t B, int64_t n, int32_t in, int32_t M,
                                           int32_t out) {
  if (B < 0 || B > kSgMaxBatch || n < 1 || !msha_sage_supported(in, M, out)) return 0;
  return sg_layout(B, n, in, M, out).total;
}

extern "C" int msha_sage_fwd(const msha_graph* g, int64_t B, const int64_t* src, int32_t in,
                             int32_t out, const float* table, int64_t ld, const float* vals,
                             const float* W1, const float* b1, const float* W2, const float* b2,
                             float* logp, msha_stream_t stream) {
  const int rc = sg_check("sage_fwd", g, B, src, in, out, table, ld, vals, W1, b1, W2, b2);
  if (rc != MSHA_OK) return rc;
  if (B == 0) return MSHA_OK;
  MSHA_ARG_CHECK(logp != nullptr, "sage_fwd: null pointer");
  const SgArgs a = sg_args(g, B, src, in, out, table, ld, vals, W1, b1, W2, b2);
  hipLaunchKernelGGL(sage_fwd_kernel, dim3(grid_for(B, kSgTile, kSgFwdBlocks)), dim3(kSgThreads),
                     0, (hipStream_t)stream, a, logp);
  return check_launch("sage_fwd");
}

namespace msha {

// where the table gradient goes: dS (n, in), every row; or the touched-row list of the batch
// (rows, n_rows: written by the call) and its (cap, in) vals
struct SgDense {
  using Policy = PgAllRows;
  static constexpr const char* kOutS = "dS";
  Policy policy() const { return {}; }
};
struct SgList {
  using Policy = PgListRows;
  static constexpr const char* kOutS = "vals";
  int32_t *list, *count_out;
  int64_t cap;
  Policy policy() const { return {list, count_out, cap}; }
};

// msha_sage_bwd (R = SgDense, dS = the (n, in) gradient, nullable) and msha_sage_bwd_rows (R =
// SgList, dS = vals): one row pass, one weight gradient, one (src, src) plan
template <typename R>
static int sg_bwd_run(const char* name, const msha_graph* g, int64_t B, const int64_t* src,
                      int32_t in, int32_t out, const float* table, int64_t ld, const float* vals,
                      const float* W1, const float* b1, const float* W2, const float* b2,
                      const float* logp, const float* dlogp, float* dS, float* dW1, float* db1,
                      float* dW2, float* db2, void* ws, size_t ws_bytes, msha_stream_t stream,
                      R rows) {
  constexpr bool kList = std::is_same<R, SgList>::value;
  const std::string nm(name);
  const int rc = sg_check(name, g, B, src, in, out, table, ld, vals, W1, b1, W2, b2);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(B == 0 || (logp && dlogp), nm + ": null pointer");
  MSHA_ARG_CHECK((dW1 != nullptr) == (db1 != nullptr) && (dW1 != nullptr) == (dW2 != nullptr) &&
                     (dW1 != nullptr) == (db2 != nullptr),
                 nm + ": dW1, db1, dW2 and db2 come together or not at all");
  MSHA_ARG_CHECK(((uintptr_t)dS % 16) == 0, nm + ": " + R::kOutS + " must be 16-byte aligned");
  const int M = (int)g->n_cols;
  const SgLayout L = sg_layout(B, g->n_rows, in, M, out);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= (kList ? L.rows_total : L.total) &&
                     ((uintptr_t)ws % 16) == 0,
                 nm + ": workspace too small or unaligned (" +
                     (kList ? "msha_sage_rows_workspace_size" : "msha_sage_workspace_size") + ")");
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  float* dr = (float*)(w + L.dr);
  float* ez = (float*)(w + L.ez);
  float* ey = (float*)(w + L.ey);
  float* dx = (float*)(w + L.dx);
  const SgArgs a = sg_args(g, B, src, in, out, table, ld, vals, W1, b1, W2, b2);
  if (B > 0)
    hipLaunchKernelGGL(sage_bwd_rows_kernel, dim3(grid_for(B, kSgTile, kSgFwdBlocks)),
                       dim3(kSgThreads), 0, s, a, logp, dlogp, dr, ez, ey,
                       dS != nullptr ? dx : nullptr);
  if (dW1 != nullptr) {
    float* part = (float*)(w + L.part);
    const int64_t nblk = sg_wg_blocks(B);
    const int len = sg_len(in, M, out);
    hipLaunchKernelGGL(sage_wgrad_kernel, dim3((unsigned)nblk), dim3(kSgThreads), 0, s, a,
                       sg_wg_per(B), dr, ez, ey, part);
    hipLaunchKernelGGL(sage_wfinish_kernel, dim3(grid_for(len, kSgGroup)), dim3(kSgThreads), 0,
                       s, nblk, len, M * in, M * in + M, M * in + M + out * M, part, dW1, db1, dW2,
                       db2);
  }
  if (dS != nullptr || kList) {  // (a list of capacity 0 still gets its count)
    int32_t* prow = (int32_t*)(w + L.prow);
    int32_t* pent = (int32_t*)(w + L.pent);
    int32_t* ptab = (int32_t*)(w + L.ptab);
    const int prc = msha_pair_plan(B, g->n_rows, src, src, prow, pent, ptab, w + L.pws,
                                   L.total - L.pws, stream);
    if (prc != MSHA_OK) return prc;
    if constexpr (kList) {  // the touched rows of that plan: the distinct valid sources
      const int lrc = msha_plan_rows(g->n_rows, B, prow, rows.list, rows.count_out, w + L.rws,
                                     L.rows_total - L.rws, stream);
      if (lrc != MSHA_OK) return lrc;
    }
    if (dS != nullptr)
      hipLaunchKernelGGL((sage_table_kernel<typename R::Policy>),
                         dim3(grid_for(rows.policy().grid_rows(g->n_rows) * (in / 4), kSgThreads,
                                       1 << 16)),
                         dim3(kSgThreads), 0, s, B, g->n_rows, (int)in, prow, pent, dx, dS,
                         rows.policy());
  }
  return check_launch(name);
}

}  // namespace msha

extern "C" int msha_sage_bwd(const msha_graph* g, int64_t B, const int64_t* src, int32_t in,
                             int32_t out, const float* table, int64_t ld, const float* vals,
                             const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* logp, const float* dlogp, float* dS, float* dW1,
                             float* db1, float* dW2, float* db2, void* ws, size_t ws_bytes,
                             msha_stream_t stream) {
  return sg_bwd_run("sage_bwd", g, B, src, in, out, table, ld, vals, W1, b1, W2, b2, logp, dlogp,
                    dS, dW1, db1, dW2, db2, ws, ws_bytes, stream, SgDense{});
}

extern "C" size_t msha_sage_rows_workspace_size(int64_t B, int64_t n, int32_t in, int32_t M,
                                                int32_t out) {
  if (msha_sage_workspace_size(B, n, in, M, out) == 0 || n >= ((int64_t)1 << 31) - 1) return 0;
  return sg_layout(B, n, in, M, out).rows_total;
}

extern "C" int msha_sage_bwd_rows(const msha_graph* g, int64_t B, const int64_t* src, int32_t in,
                                  int32_t out, const float* table, int64_t ld, const float* vals,
                                  const float* W1, const float* b1, const float* W2,
                                  const float* b2, const float* logp, const float* dlogp,
                                  float* dW1, float* db1, float* dW2, float* db2, int32_t* rows,
                                  int32_t* n_rows, int64_t cap, float* row_vals, void* ws,
                                  size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(g != nullptr, "sage_bwd_rows: graph CSR or edge values missing");
  MSHA_ARG_CHECK(n_rows && (cap == 0 || (rows && row_vals)), "sage_bwd_rows: null pointer");
  MSHA_ARG_CHECK(B >= 0 && cap == pg_rows_cap(g->n_rows, B),
                 "sage_bwd_rows: cap must be min(n, 2 * B) (the (src, src) plan's list)");
  return sg_bwd_run("sage_bwd_rows", g, B, src, in, out, table, ld, vals, W1, b1, W2, b2, logp,
                    dlogp, row_vals, dW1, db1, dW2, db2, ws, ws_bytes, stream,
                    SgList{rows, n_rows, cap});
}
