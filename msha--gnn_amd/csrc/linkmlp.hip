// Link-prediction training for the 'mlp' predictor with one used Linear (LLP.py:233-238:
// output = predictor(h[src], h[dst]); nll_loss(output, label) and mse_loss(output, t_out)),
// with no gathered (P, F) operand anywhere and no float atomics:
//
//   x_p   = h[src_p] * h[dst_p]
//   out_p = sigmoid(dropout(relu(W x_p + b)))                       (P, N), msha_pair_linear
//   loss  = w_label * (-(1/Pv) sum_p out_p[label_p])
//         + w_mse   * ((1/(Pv N)) sum_p sum_j (out_pj - t_pj)^2)
//
//   link_mlp_loss_fwd  the gathered MFMA launch of msha_pair_linear(_bf16) on index lists
//                      with the padding pairs redirected to row 0, then ONE pass over out,
//                      t, label, src, dst: the valid-pair count Pv, the two sums by per-block
//                      partials in a fixed order, the NaN rows of padding pairs; one block
//                      adds the partials in order and writes {loss, L_lab, L_mse}, Pv, and
//                      the loss once more into a scalar of its own (the autograd output: no
//                      copy node in a captured graph).
//   link_mlp_bwd       dz (one pass, msha_pair_mlp_dz's rule from the stored out);
//                      dW = dz^T (h[src] * h[dst]) on v_mfma_f32_16x16x4_f32 with the A
//                      operand gathered and multiplied in the loader, db from the same pass,
//                      both by per-row-block partials added in block order;
//                      dx = dz W on msha_gemm_f32; dH by pair_grad.h's vector-factor pass.
//
// A pair is padding when src or dst lies outside [0, n) or its label outside [0, N): it is
// in no sum, not in Pv, its dz row is zero and its out row is NaN.  Every table read is
// bounds-checked on the index it uses.
#include "common.h"
#include "pair_grad.h"

namespace msha {

constexpr int kLmThreads = 256;
constexpr int kLmWaves = kLmThreads / kWave;
constexpr int kLmTile = 256;      // pairs per loss block (fixes the loss order)
constexpr int kLmFin = 1024;      // threads of the ordered finish
constexpr int kLmWgRows = 2048;   // pairs per weight-gradient block (msha_link_mlp_wgrad_rows)
constexpr int kLmKC = 32;         // pairs per staged chunk of the weight gradient
constexpr int kLmMaxW = 128;      // widest feat / hidden
constexpr int kLmPitch = kLmMaxW + 16;  // LDS row pitch (floats): 4 k-rows 16 banks apart
constexpr int kLmStage = kLmKC * kLmMaxW / 4 / kLmThreads;  // float4 pieces per thread, at most

// the label of pair p (dst itself without a label list) and whether the pair is real
__device__ __forceinline__ bool lm_pair(int64_t p, int64_t n, int N,
                                        const int64_t* __restrict__ src,
                                        const int64_t* __restrict__ dst,
                                        const int64_t* __restrict__ label, int64_t& lab) {
  const int64_t s = src[p], d = dst[p];
  lab = label != nullptr ? label[p] : d;
  return (uint64_t)s < (uint64_t)n && (uint64_t)d < (uint64_t)n && (uint64_t)lab < (uint64_t)N;
}

// the pair lists the gathered forward reads: a padding pair reads row 0 (its out row is
// overwritten with NaN by the loss pass), so no index leaves the table
__global__ void __launch_bounds__(kLmThreads) lm_index_kernel(
    int64_t P, int64_t n, int N, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const int64_t* __restrict__ label, int64_t* __restrict__ gi, int64_t* __restrict__ gj) {
  for (int64_t p = (int64_t)blockIdx.x * kLmThreads + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * kLmThreads) {
    int64_t lab;
    const bool ok = lm_pair(p, n, N, src, dst, label, lab);
    gi[p] = ok ? src[p] : 0;
    gj[p] = ok ? dst[p] : 0;
  }
}

// One block per tile of kLmTile pairs; N / 4 lanes a row, a float4 each.  Lane group g of
// wave w takes rows w RPW + g, + 4 RPW, ... of the tile in order; the groups' sums meet in an
// xor tree, the waves' in wave order: the order is a function of P and N alone.
__global__ void __launch_bounds__(kLmThreads) lm_loss_kernel(
    int64_t P, int64_t n, int N, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const int64_t* __restrict__ label, const float* __restrict__ teacher, float* __restrict__ out,
    float* __restrict__ part, int32_t* __restrict__ cntpart) {
  __shared__ float wl[kLmWaves], wm[kLmWaves];
  __shared__ int wc[kLmWaves];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int LPR = N / 4, RPW = kWave / LPR;
  const int slot = lane / LPR, q = lane % LPR;
  const int64_t base = (int64_t)blockIdx.x * kLmTile;
  const int count = (int)min((int64_t)kLmTile, P - base);
  float alab = 0.f, amse = 0.f;
  int cnt = 0;
  const float nanv = __builtin_nanf("");
  for (int i = wv * RPW + slot; i < count; i += kLmWaves * RPW) {
    const int64_t p = base + i;
    int64_t lab;
    const bool ok = lm_pair(p, n, N, src, dst, label, lab);
    float* o = out + p * N + 4 * q;
    if (!ok) {
      *reinterpret_cast<float4*>(o) = make_float4(nanv, nanv, nanv, nanv);
      continue;
    }
    if (teacher != nullptr) {
      const float4 v = *reinterpret_cast<const float4*>(o);
      const float4 t = *reinterpret_cast<const float4*>(teacher + p * N + 4 * q);
      const float d0 = v.x - t.x, d1 = v.y - t.y, d2 = v.z - t.z, d3 = v.w - t.w;
      amse += fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, d3 * d3)));
    }
    if (q == 0) {
      alab += out[p * N + lab];
      ++cnt;
    }
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    alab += __shfl_xor(alab, o);
    amse += __shfl_xor(amse, o);
    cnt += __shfl_xor(cnt, o);
  }
  if (lane == 0) {
    wl[wv] = alab;
    wm[wv] = amse;
    wc[wv] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    int c = 0;
    for (int k = 0; k < kLmWaves; ++k) {
      a += wl[k];
      b += wm[k];
      c += wc[k];
    }
    part[2 * (int64_t)blockIdx.x] = a;
    part[2 * (int64_t)blockIdx.x + 1] = b;
    cntpart[blockIdx.x] = c;
  }
}

// the blocks' partials in a fixed order: thread t strides them, xor tree, waves ascending;
// terms = {loss, L_lab, L_mse}, all 0 without a valid pair
__global__ void __launch_bounds__(kLmFin) lm_loss_final_kernel(
    int64_t nb, int N, const float* __restrict__ part, const int32_t* __restrict__ cntpart,
    float w_label, float w_mse, float* __restrict__ terms, float* __restrict__ loss,
    int32_t* __restrict__ n_valid) {
  __shared__ float wl[kLmFin / kWave], wm[kLmFin / kWave];
  __shared__ int wc[kLmFin / kWave];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  float a = 0.f, b = 0.f;
  int c = 0;
  for (int64_t i = threadIdx.x; i < nb; i += kLmFin) {
    a += part[2 * i];
    b += part[2 * i + 1];
    c += cntpart[i];
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
    c += __shfl_xor(c, o);
  }
  if (lane == 0) {
    wl[wv] = a;
    wm[wv] = b;
    wc[wv] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sa = 0.f, sb = 0.f;
    int pv = 0;
    for (int k = 0; k < kLmFin / kWave; ++k) {
      sa += wl[k];
      sb += wm[k];
      pv += wc[k];
    }
    float llab = 0.f, lmse = 0.f;
    if (pv > 0) {
      llab = -sa / (float)pv;
      lmse = sb / ((float)pv * (float)N);
    }
    const float total = w_label * llab + w_mse * lmse;
    terms[0] = total;
    if (loss != nullptr) loss[0] = total;  // the differentiable scalar: its own tensor
    terms[1] = llab;
    terms[2] = lmse;
    n_valid[0] = pv;
  }
}

// dz = g * out (1 - out) / (1 - p) where out > 0.5 (kept and ReLU-active), else 0, with
// g_pj = gloss (-w_label / Pv [j == label_p] + 2 w_mse (out_pj - t_pj) / (Pv N)); a float4 a
// thread, rows of padding pairs zero
__global__ void __launch_bounds__(kLmThreads) lm_dz_kernel(
    int64_t P, int64_t n, int N, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const int64_t* __restrict__ label, const float* __restrict__ teacher,
    const float* __restrict__ out, const int32_t* __restrict__ n_valid, float w_label,
    float w_mse, float scale, const float* __restrict__ gloss, float* __restrict__ dz) {
  const int LPR = N / 4;
  const int64_t total = P * LPR;
  const int pv = n_valid[0];
  const float gl = gloss[0];
  const float cl = pv > 0 ? -gl * w_label / (float)pv : 0.f;
  const float cm = pv > 0 ? 2.f * gl * w_mse / ((float)pv * (float)N) : 0.f;
  for (int64_t t = (int64_t)blockIdx.x * kLmThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kLmThreads) {
    const int64_t p = t / LPR;
    const int c = 4 * (int)(t % LPR);
    int64_t lab;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lm_pair(p, n, N, src, dst, label, lab)) {
      const float4 v = *reinterpret_cast<const float4*>(out + p * N + c);
      float4 tv = v;  // no teacher: out - t = 0
      if (teacher != nullptr) tv = *reinterpret_cast<const float4*>(teacher + p * N + c);
      const float o[4] = {v.x, v.y, v.z, v.w};
      const float tt[4] = {tv.x, tv.y, tv.z, tv.w};
      float d[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float g = fmaf(cm, o[i] - tt[i], (int64_t)(c + i) == lab ? cl : 0.f);
        d[i] = o[i] > 0.5f ? g * o[i] * (1.f - o[i]) * scale : 0.f;
      }
      r = make_float4(d[0], d[1], d[2], d[3]);
    }
    *reinterpret_cast<float4*>(dz + p * N + c) = r;
  }
}

// ---- the gathered weight gradient ----
// 4 elements of a table row as loaded (converted at the LDS store, so the loads of the next
// chunk stay in flight under the MFMAs of this one)
template <typename T> struct LmRaw;
template <> struct LmRaw<float> { typedef float4 type; };
template <> struct LmRaw<bf16_t> { typedef uint2 type; };

__device__ __forceinline__ float4 lm_prod(float4 a, float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 lm_prod(uint2 a, uint2 b) {
  return make_float4(__uint_as_float(a.x << 16) * __uint_as_float(b.x << 16),
                     __uint_as_float(a.x & 0xffff0000u) * __uint_as_float(b.x & 0xffff0000u),
                     __uint_as_float(a.y << 16) * __uint_as_float(b.y << 16),
                     __uint_as_float(a.y & 0xffff0000u) * __uint_as_float(b.y & 0xffff0000u));
}

template <typename T>
struct LmStage {
  float4 dz[kLmStage];
  typename LmRaw<T>::type xa[kLmStage], xb[kLmStage];
  uint32_t ok;  // bit it: the x piece is of a pair inside the table
};

// chunk [p0, p0 + kLmKC) of the block's rows [.., r1): piece idx = it * 256 + tid is row
// idx / (W / 4), columns 4 (idx % (W / 4)).. of the (kLmKC, W) image (W = N for dz, F for x)
template <typename T>
__device__ __forceinline__ void lm_stage_load(LmStage<T>& st, int64_t p0, int64_t r1, int64_t n,
                                              int64_t ld, int F, int N, const T* __restrict__ h,
                                              const int64_t* __restrict__ src,
                                              const int64_t* __restrict__ dst,
                                              const float* __restrict__ dz, int tid) {
  typedef typename LmRaw<T>::type raw_t;
  uint32_t ok = 0u;
#pragma unroll
  for (int it = 0; it < kLmStage; ++it) {
    const int idx = it * kLmThreads + tid;
    {
      const int row = idx / (N / 4), c = 4 * (idx % (N / 4));
      const int64_t p = p0 + row;
      st.dz[it] = row < kLmKC && p < r1 ? *reinterpret_cast<const float4*>(dz + p * N + c)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    {
      const int row = idx / (F / 4), c = 4 * (idx % (F / 4));
      const int64_t p = p0 + row;
      int64_t s = 0, d = 0;
      bool v = row < kLmKC && p < r1;
      if (v) {
        s = src[p];
        d = dst[p];
        v = (uint64_t)s < (uint64_t)n && (uint64_t)d < (uint64_t)n;
      }
      if (!v) s = d = 0;  // row 0 of the table: inside it, dropped at the store
      st.xa[it] = *reinterpret_cast<const raw_t*>(h + s * ld + c);
      st.xb[it] = *reinterpret_cast<const raw_t*>(h + d * ld + c);
      ok |= (v ? 1u : 0u) << it;
    }
  }
  st.ok = ok;
}

template <typename T>
__device__ __forceinline__ void lm_stage_store(const LmStage<T>& st, int F, int N, float* dzs,
                                               float* xs, float4& dbacc, int tid) {
#pragma unroll
  for (int it = 0; it < kLmStage; ++it) {
    const int idx = it * kLmThreads + tid;
    {
      const int row = idx / (N / 4), c = 4 * (idx % (N / 4));
      if (row < kLmKC) {
        *reinterpret_cast<float4*>(dzs + row * kLmPitch + c) = st.dz[it];
        dbacc = make_float4(dbacc.x + st.dz[it].x, dbacc.y + st.dz[it].y, dbacc.z + st.dz[it].z,
                            dbacc.w + st.dz[it].w);
      }
    }
    {
      const int row = idx / (F / 4), c = 4 * (idx % (F / 4));
      if (row < kLmKC) {
        const float4 x = (st.ok >> it) & 1u ? lm_prod(st.xa[it], st.xb[it])
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(xs + row * kLmPitch + c) = x;
      }
    }
  }
}

// Block b owns pairs [b R, (b + 1) R) and the whole (N, F) output: the (N / 16)(F / 16)
// MFMA tiles go to the 4 waves in runs of TPW (tile t = w TPW + i is rows 16 (t / (F / 16)),
// columns 16 (t % (F / 16))).  dW_b[nn, f] = sum_p dz[p, nn] x[p, f]: A = dz^T, B = x, both
// read from their [pair][column] LDS images a k-row of 16 lanes at a time (pitch 144: the 4
// k-rows of a step lie 16 banks apart).  part_b = dW_b (N F) | db_b (N).
// FTC: F / 16 at compile time (0: run time).  With it a wave's tile coordinates are constants
// beside w, so the 2 A and 8 B fragments its 16 tiles share at 128 x 128 are each read once a
// step; the tiles, their k order and so the result's bits are the same either way.
template <typename T, int TPW, int FTC = 0>
__global__ void __launch_bounds__(kLmThreads, 2) lm_wgrad_kernel(
    int64_t P, int64_t n, int64_t ld, int F, int N, const T* __restrict__ h,
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const float* __restrict__ dz, float* __restrict__ part) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float smem[2 * kLmKC * kLmPitch];
  float* dzs = smem;
  float* xs = smem + kLmKC * kLmPitch;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int FT = FTC > 0 ? FTC : F / 16, ntiles = (N / 16) * FT;
  const int64_t r0 = (int64_t)blockIdx.x * kLmWgRows;
  const int64_t r1 = min(P, r0 + kLmWgRows);
  f32x4 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 dbacc = make_float4(0.f, 0.f, 0.f, 0.f);
  LmStage<T> st;
  lm_stage_load(st, r0, r1, n, ld, F, N, h, src, dst, dz, tid);
  for (int64_t p0 = r0; p0 < r1; p0 += kLmKC) {
    __syncthreads();
    lm_stage_store(st, F, N, dzs, xs, dbacc, tid);
    __syncthreads();
    if (p0 + kLmKC < r1) lm_stage_load(st, p0 + kLmKC, r1, n, ld, F, N, h, src, dst, dz, tid);
#pragma unroll 2  // (fully unrolled, the LDS reads of all 8 steps are hoisted: 260 VGPRs)
    for (int ks = 0; ks < kLmKC / 4; ++ks) {
      const int kr = (4 * ks + (lane >> 4)) * kLmPitch + (lane & 15);
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int t = w * TPW + i;
        if (FTC > 0 || t < ntiles) {  // (an FTC instance runs with every tile in use)
          const float a = dzs[kr + 16 * (t / FT)];
          const float b = xs[kr + 16 * (t % FT)];
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
        }
      }
    }
  }
  // C layout: row 4 (lane >> 4) + reg, column lane & 15
  float* o = part + (int64_t)blockIdx.x * ((int64_t)N * F + N);
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = w * TPW + i;
    if (t < ntiles) {
      const int row = 16 * (t / FT) + 4 * (lane >> 4), col = 16 * (t % FT) + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(int64_t)(row + r) * F + col] = acc[i][r];
    }
  }
  // db: thread tid summed columns 4 (tid % (N / 4)).. of its rows; the 256 / (N / 4) threads
  // of a column group are added in thread order
  __syncthreads();
  const int LPR = N / 4;
  *reinterpret_cast<float4*>(smem + (tid / LPR) * N + 4 * (tid % LPR)) = dbacc;
  __syncthreads();
  if (tid < N) {
    float s = 0.f;
    for (int g = 0; g < kLmThreads / LPR; ++g) s += smem[g * N + tid];
    o[(int64_t)N * F + tid] = s;
  }
}

// the row blocks' partials added in block order, an element a thread
__global__ void __launch_bounds__(kLmThreads) lm_wfinish_kernel(
    int64_t nblk, int64_t len, int64_t nf, const float* __restrict__ part, float* __restrict__ dW,
    float* __restrict__ db) {
  const int64_t j = (int64_t)blockIdx.x * kLmThreads + threadIdx.x;
  if (j >= len) return;
  float s = part[j];
#pragma unroll 8  // the loads of 8 partials in flight; the adds stay in block order
  for (int64_t b = 1; b < nblk; ++b) s += part[b * len + j];
  if (j < nf)
    dW[j] = s;
  else
    db[j - nf] = s;
}

static bool lm_pow2(int32_t x) { return x > 0 && (x & (x - 1)) == 0; }

// feat and hidden powers of two in [16, 128] (whole 16 x 16 MFMA tiles, a float4 lane
// layout of the (P, hidden) rows); feat also under msha_link_bce_supported
static bool lm_shape_ok(int32_t feat, int32_t hidden, int32_t dtype) {
  return pg_width_ok(feat, dtype) && lm_pow2(feat) && lm_pow2(hidden) && feat >= 16 &&
         feat <= kLmMaxW && hidden >= 16 && hidden <= kLmMaxW;
}

static int64_t lm_loss_blocks(int64_t P) { return P > 0 ? (P + kLmTile - 1) / kLmTile : 1; }
static int64_t lm_wg_blocks(int64_t P) { return P > 0 ? (P + kLmWgRows - 1) / kLmWgRows : 1; }

struct LmFwdLayout {
  size_t gi, gj, part, cnt, total;
};
static LmFwdLayout lm_fwd_layout(int64_t P) {
  LmFwdLayout L;
  size_t off = 0;
  L.gi = off;
  off += pg_align((size_t)P * 8);
  L.gj = off;
  off += pg_align((size_t)P * 8);
  L.part = off;
  off += pg_align((size_t)lm_loss_blocks(P) * 8);
  L.cnt = off;
  off += pg_align((size_t)lm_loss_blocks(P) * 4);
  L.total = off;
  return L;
}

struct LmBwdLayout {
  size_t wpart, pgpart, total;
};
static LmBwdLayout lm_bwd_layout(int64_t P, int32_t feat, int32_t hidden) {
  LmBwdLayout L;
  size_t off = 0;
  L.wpart = off;
  off += pg_align((size_t)lm_wg_blocks(P) * ((size_t)hidden * feat + hidden) * 4);
  L.pgpart = off;
  off += pg_workspace_bytes(P, feat);
  L.total = off;
  return L;
}

static int lm_check(const char* name, int64_t n_pairs, int32_t feat, int32_t hidden,
                    int32_t dtype, const void* h, int64_t ld, int64_t n) {
  const int rc = pg_table_check(name, n_pairs, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  if (!lm_shape_ok(feat, hidden, dtype))
    return fail(MSHA_ERR_ARG, std::string(name) + ": unsupported shape: feat and hidden must be "
                                                  "powers of two in [16, 128] "
                                                  "(msha_link_mlp_supported)");
  return MSHA_OK;
}

template <typename T>
static void lm_wgrad_launch(int64_t P, int64_t n, int64_t ld, int F, int N, const T* h,
                            const int64_t* src, const int64_t* dst, const float* dz, float* part,
                            hipStream_t s) {
  const int ntiles = (N / 16) * (F / 16);
  const dim3 grid((unsigned)lm_wg_blocks(P)), blk(kLmThreads);
  if (N == 128 && F == 128)
    hipLaunchKernelGGL((lm_wgrad_kernel<T, 16, 8>), grid, blk, 0, s, P, n, ld, F, N, h, src, dst,
                       dz, part);
  else if (ntiles <= 4)
    hipLaunchKernelGGL((lm_wgrad_kernel<T, 1>), grid, blk, 0, s, P, n, ld, F, N, h, src, dst, dz,
                       part);
  else if (ntiles <= 16)
    hipLaunchKernelGGL((lm_wgrad_kernel<T, 4>), grid, blk, 0, s, P, n, ld, F, N, h, src, dst, dz,
                       part);
  else
    hipLaunchKernelGGL((lm_wgrad_kernel<T, 16>), grid, blk, 0, s, P, n, ld, F, N, h, src, dst, dz,
                       part);
}

}  // namespace msha

using namespace msha;

extern "C" int msha_link_mlp_supported(int32_t feat, int32_t hidden, int32_t dtype) {
  return lm_shape_ok(feat, hidden, dtype) ? 1 : 0;
}

extern "C" int32_t msha_link_mlp_wgrad_rows(void) { return kLmWgRows; }

extern "C" size_t msha_link_mlp_loss_fwd_workspace_size(int64_t n_pairs) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs) return 0;
  return lm_fwd_layout(n_pairs).total;
}

extern "C" size_t msha_link_mlp_bwd_workspace_size(int64_t n_pairs, int32_t feat,
                                                   int32_t hidden) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs || feat < 1 || hidden < 1) return 0;
  return lm_bwd_layout(n_pairs, feat, hidden).total;
}

extern "C" int msha_link_mlp_loss_fwd(int64_t n_pairs, int32_t feat, int32_t hidden,
                                      int32_t dtype, const void* h, int64_t ld, int64_t n,
                                      const int64_t* src, const int64_t* dst,
                                      const int64_t* label, const void* W, const float* bias,
                                      const float* teacher_out, float w_label, float w_mse,
                                      float drop_p, uint64_t seed, uint64_t offset, float* out,
                                      float* terms, float* loss, int32_t* n_valid, void* ws,
                                      size_t ws_bytes, msha_stream_t stream) {
  const int rc = lm_check("link_mlp_loss_fwd", n_pairs, feat, hidden, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(src && dst && W && bias && out && terms && n_valid,
                 "link_mlp_loss_fwd: null pointer");
  MSHA_ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, "link_mlp_loss_fwd: drop_p must be in [0, 1)");
  MSHA_ARG_CHECK(((uintptr_t)out % 16) == 0 && ((uintptr_t)W % 16) == 0 &&
                     (teacher_out == nullptr || ((uintptr_t)teacher_out % 16) == 0),
                 "link_mlp_loss_fwd: W, out and teacher_out must be 16-byte aligned");
  const LmFwdLayout L = lm_fwd_layout(n_pairs);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= L.total && ((uintptr_t)ws % 16) == 0,
                 "link_mlp_loss_fwd: workspace too small or unaligned "
                 "(msha_link_mlp_loss_fwd_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  int64_t* gi = (int64_t*)(w + L.gi);
  int64_t* gj = (int64_t*)(w + L.gj);
  float* part = (float*)(w + L.part);
  int32_t* cnt = (int32_t*)(w + L.cnt);
  hipLaunchKernelGGL(lm_index_kernel, dim3(grid_for(n_pairs, kLmThreads, 1 << 16)),
                     dim3(kLmThreads), 0, s, n_pairs, n, (int)hidden, src, dst, label, gi, gj);
  const int32_t act = 1 | 2 | (drop_p > 0.f ? 4 : 0) | 8;  // bias | relu | [dropout] | sigmoid
  int prc;
  if (dtype == MSHA_DTYPE_BF16)
    prc = msha_pair_linear_bf16(n_pairs, feat, hidden, h, ld, gi, h, ld, gj, W, bias, act, drop_p,
                                seed, offset, out, stream);
  else
    prc = msha_pair_linear(n_pairs, feat, hidden, (const float*)h, ld, gi, (const float*)h, ld,
                           gj, n, n, (const float*)W, bias, act, drop_p, seed, offset, out,
                           stream);
  if (prc != MSHA_OK) return prc;
  const int64_t nb = lm_loss_blocks(n_pairs);
  hipLaunchKernelGGL(lm_loss_kernel, dim3((unsigned)nb), dim3(kLmThreads), 0, s, n_pairs, n,
                     (int)hidden, src, dst, label, teacher_out, out, part, cnt);
  hipLaunchKernelGGL(lm_loss_final_kernel, dim3(1), dim3(kLmFin), 0, s, nb, (int)hidden, part,
                     cnt, w_label, w_mse, terms, loss, n_valid);
  return check_launch("link_mlp_loss_fwd");
}

namespace msha {

// msha_link_mlp_bwd and msha_link_mlp_bwd_rows: out = dH (n, F) with PgAllRows, the (cap, F)
// vals of the touched-row list with PgListRows; everything before the table gradient is shared
template <typename R>
static int lm_bwd_run(const char* name, int64_t n_pairs, int32_t feat, int32_t hidden,
                      int32_t dtype, const void* h, int64_t ld, int64_t n, const int64_t* src,
                      const int64_t* dst, const int64_t* label, const float* W32,
                      const float* teacher_out, const float* out, const int32_t* n_valid,
                      float w_label, float w_mse, float drop_p, const float* gloss,
                      const int32_t* plan_rowptr, const int32_t* plan_ent,
                      const int32_t* plan_chunk_tab, float* dz, float* dx, float* dW, float* db,
                      float* dH, void* ws, size_t ws_bytes, msha_stream_t stream, R rows) {
  const std::string nm(name);
  const int rc = lm_check(name, n_pairs, feat, hidden, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(src && dst && out && n_valid && gloss && dz, nm + ": null pointer");
  MSHA_ARG_CHECK((dW == nullptr) == (db == nullptr),
                 nm + ": dW and db come together or not at all");
  MSHA_ARG_CHECK(dH == nullptr || (W32 && dx && plan_rowptr && plan_ent && plan_chunk_tab),
                 nm + ": " + R::kOut + " needs W, dx and the plan");
  MSHA_ARG_CHECK(drop_p >= 0.f && drop_p < 1.f, nm + ": drop_p must be in [0, 1)");
  MSHA_ARG_CHECK(((uintptr_t)out % 16) == 0 && ((uintptr_t)dz % 16) == 0 &&
                     ((uintptr_t)dx % 16) == 0 && ((uintptr_t)dH % 16) == 0 &&
                     (teacher_out == nullptr || ((uintptr_t)teacher_out % 16) == 0),
                 nm + ": out, teacher_out, dz, dx and " + R::kOut + " must be 16-byte aligned");
  const LmBwdLayout L = lm_bwd_layout(n_pairs, feat, hidden);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= L.total && ((uintptr_t)ws % 16) == 0,
                 nm + ": workspace too small or unaligned (msha_link_mlp_bwd_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  const int F = feat, N = hidden;
  const float scale = (float)(1.0 / (1.0 - (double)drop_p));
  hipLaunchKernelGGL(lm_dz_kernel, dim3(grid_for(n_pairs * (N / 4), kLmThreads, 1 << 18)),
                     dim3(kLmThreads), 0, s, n_pairs, n, N, src, dst, label, teacher_out, out,
                     n_valid, w_label, w_mse, scale, gloss, dz);
  if (dW != nullptr) {
    float* wpart = (float*)(w + L.wpart);
    if (dtype == MSHA_DTYPE_BF16)
      lm_wgrad_launch(n_pairs, n, ld, F, N, (const bf16_t*)h, src, dst, dz, wpart, s);
    else
      lm_wgrad_launch(n_pairs, n, ld, F, N, (const float*)h, src, dst, dz, wpart, s);
    const int64_t len = (int64_t)N * F + N;
    hipLaunchKernelGGL(lm_wfinish_kernel, dim3(grid_for(len, kLmThreads)), dim3(kLmThreads), 0, s,
                       lm_wg_blocks(n_pairs), len, (int64_t)N * F, wpart, dW, db);
  }
  if (dH != nullptr) {
    // dx = dz W: (P, N) x (N, F), W an nn.Linear weight (N x F) row-major
    const int grc = msha_gemm_f32(n_pairs, F, N, dz, N, 1, W32, F, 1, dx, F, 0.f, 1, nullptr, 0,
                                  stream);
    if (grc != MSHA_OK) return grc;
    // dH from dx under the plan (pair_grad.h); dx carries gloss already (lm_dz_kernel)
    return pg_run(name, "msha_link_mlp_bwd_workspace_size", n_pairs, feat, dtype, h, ld, n, src,
                  dst, plan_rowptr, plan_ent, plan_chunk_tab, PgDx{dx}, nullptr, dH, w + L.pgpart,
                  L.total - L.pgpart, stream, rows);
  }
  return check_launch(name);
}

}  // namespace msha

extern "C" int msha_link_mlp_bwd(int64_t n_pairs, int32_t feat, int32_t hidden, int32_t dtype,
                                 const void* h, int64_t ld, int64_t n, const int64_t* src,
                                 const int64_t* dst, const int64_t* label, const float* W32,
                                 const float* teacher_out, const float* out,
                                 const int32_t* n_valid, float w_label, float w_mse, float drop_p,
                                 const float* gloss, const int32_t* plan_rowptr,
                                 const int32_t* plan_ent, const int32_t* plan_chunk_tab,
                                 float* dz, float* dx, float* dW, float* db, float* dH, void* ws,
                                 size_t ws_bytes, msha_stream_t stream) {
  return lm_bwd_run("link_mlp_bwd", n_pairs, feat, hidden, dtype, h, ld, n, src, dst, label, W32,
                    teacher_out, out, n_valid, w_label, w_mse, drop_p, gloss, plan_rowptr,
                    plan_ent, plan_chunk_tab, dz, dx, dW, db, dH, ws, ws_bytes, stream,
                    PgAllRows{});
}

extern "C" int msha_link_mlp_bwd_rows(int64_t n_pairs, int32_t feat, int32_t hidden,
                                      int32_t dtype, const void* h, int64_t ld, int64_t n,
                                      const int64_t* src, const int64_t* dst,
                                      const int64_t* label, const float* W32,
                                      const float* teacher_out, const float* out,
                                      const int32_t* n_valid, float w_label, float w_mse,
                                      float drop_p, const float* gloss,
                                      const int32_t* plan_rowptr, const int32_t* plan_ent,
                                      const int32_t* plan_chunk_tab, float* dz, float* dx,
                                      float* dW, float* db, const int32_t* rows,
                                      const int32_t* n_rows, int64_t cap, float* vals, void* ws,
                                      size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(rows && n_rows && vals, "link_mlp_bwd_rows: null pointer");
  MSHA_ARG_CHECK(cap == pg_rows_cap(n, n_pairs),
                 "link_mlp_bwd_rows: cap must be min(n, 2 * n_pairs) (msha_plan_rows)");
  return lm_bwd_run("link_mlp_bwd_rows", n_pairs, feat, hidden, dtype, h, ld, n, src, dst, label,
                    W32, teacher_out, out, n_valid, w_label, w_mse, drop_p, gloss, plan_rowptr,
                    plan_ent, plan_chunk_tab, dz, dx, dW, db, vals, ws, ws_bytes, stream,
                    PgListRows{rows, n_rows, cap});
}
