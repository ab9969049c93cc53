// Link-prediction training for the 'inner' scorer (LLP.py:112-115 under a BCE loss):
// sample -> score -> loss -> table gradient, with no (P, F) array anywhere and no float
// atomics.
//
//   negative_sample  for positive p and j < k: the pair (src[p], d), d uniform over the
//                    candidates that are not neighbours of src[p] in a CSR.  No rejection:
//                    r = mulhi32(philox, cnt) picks the r-th non-edge column, found by a
//                    binary search for the smallest t with col[t] - t > r; d = r + t.
//   pair_plan        the inverted index of a pair list: the 2P endpoints (e < P: the src end
//                    of pair e, e >= P: the dst end of pair e - P) sorted by table row with a
//                    stable LSD radix sort (8-bit digits, per-block histograms, one scan of
//                    the (digit, block) table, ranked scatter -- msha_rank_auc's passes with
//                    a 4-byte payload), then rowptr by binary search and a chunk table.
//   link_bce_fwd     z = <h[src], h[dst]>, loss = sum w (max(z,0) - z y + log1p(exp(-|z|))):
//                    a block owns a fixed tile of pairs, its partial is summed in a fixed
//                    order, and one block adds the partials in order.
//   link_bce_bwd     dH[r] = sum over row r's endpoints, in plan order, of g h[other], with
//                    g = gloss w (sigmoid(z) - y) formed on the fly.  One wave per row; rows
//                    longer than a chunk go through chunk partials added in chunk order.
//
// Chunks of a long row [b, e) start at b, b + C, b + 2C, ...  Two chunk starts of long rows
// that are not a row's first lie more than C apart, so window m = [mC, (m+1)C) of `ent`
// holds at most one of them: the chunk table and the partials are addressed by window,
// 2 * ceil(2P / C) slots (even: the chunk that starts inside the window, odd: the first
// chunk of the long row that starts inside it).  A static bound; nothing is read back.
#include "common.h"
#include "pair_grad.h"

namespace msha {

typedef unsigned long long u64;

constexpr int kLlThreads = 256;
constexpr int kLlWaves = kLlThreads / kWave;
constexpr int kPlTile = kLlThreads * 16;  // keys per block and radix pass
constexpr int kPlChunk = kPgChunk;        // endpoints per backward chunk (pair_grad.h)
constexpr int kFwdTile = 1024;            // pairs per forward block (fixes the loss order)
constexpr int kFinThreads = 1024;

// ------------------------------------------------------------- negative_sample ----

__global__ void __launch_bounds__(kLlThreads) ll_negative_kernel(
    int64_t total, int k, const int64_t* __restrict__ src, int64_t n_rows, int32_t n_cand,
    int64_t n_edges, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ rowflag, int64_t col_offset, Dropout dp,
    int64_t* __restrict__ src_rep, int64_t* __restrict__ dst_neg) {
  const uint64_t off = dropout_offset(dp, dp.offset);
  for (int64_t t = (int64_t)blockIdx.x * kLlThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kLlThreads) {
    const int64_t s = src[t / k];
    int64_t d = -1;
    if ((uint64_t)s < (uint64_t)n_rows) {  // decided before any load through s
      const int64_t beg = rowptr[s];
      int64_t deg = (int64_t)rowptr[s + 1] - beg;
      const bool csr_ok = beg >= 0 && deg >= 0 && beg + deg <= n_edges;
      if (rowflag != nullptr && rowflag[s] != 0) deg = 0;  // a virtual full row: no edges
      const int64_t cnt = (int64_t)n_cand - deg;
      if (csr_ok && cnt > 0) {
        const int64_t r = mulhi32(philox_x(dp.seed, off, (uint64_t)t), (uint32_t)cnt);
        int lo = 0, hi = (int)deg;  // smallest t in [0, deg] with col[t] - t > r
        for (int it = 0; it < 32 && lo < hi; ++it) {
          const int mid = lo + ((hi - lo) >> 1);
          if ((int64_t)col[beg + mid] - mid > r)
            hi = mid;
          else
            lo = mid + 1;
        }
        const int64_t c = r + lo;
        if (c < n_cand) d = c + col_offset;  // (always, on ascending in-range columns)
      }
    }
    src_rep[t] = s;
    dst_neg[t] = d;
  }
}

// ------------------------------------------------------------------- pair_plan ----

// key of endpoint e = its table row, n for an endpoint of a padding pair; payload = e
__global__ void __launch_bounds__(kLlThreads) pl_keys_kernel(
    int64_t P, uint32_t n, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    uint32_t* __restrict__ keys, uint32_t* __restrict__ pay) {
  for (int64_t e = (int64_t)blockIdx.x * kLlThreads + threadIdx.x; e < 2 * P;
       e += (int64_t)gridDim.x * kLlThreads) {
    const int64_t p = e < P ? e : e - P;
    const int64_t s = src[p], d = dst[p];
    const bool ok = (uint64_t)s < (uint64_t)n && (uint64_t)d < (uint64_t)n;
    keys[e] = ok ? (uint32_t)(e < P ? s : d) : n;
    pay[e] = (uint32_t)e;
  }
}

// hist[digit * nb + block] = the block's count of the digit in its tile
__global__ void __launch_bounds__(kLlThreads) pl_hist_kernel(int64_t n,
                                                            const uint32_t* __restrict__ keys,
                                                            int shift,
                                                            uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const int t = threadIdx.x;
  const int64_t nb = gridDim.x, i0 = (int64_t)blockIdx.x * kPlTile;
  const int count = (int)min((int64_t)kPlTile, n - i0);
  h[t] = 0u;
  __syncthreads();
  for (int j = t; j < count; j += kLlThreads) atomicAdd(&h[(keys[i0 + j] >> shift) & 255u], 1u);
  __syncthreads();
  hist[(int64_t)t * nb + blockIdx.x] = h[t];
}

// one wave per digit row: exclusive scan of its nb block counts in place, total to tot[digit]
__global__ void __launch_bounds__(kLlThreads) pl_scan_kernel(int64_t nb,
                                                            uint32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ tot) {
  const int lane = lane_id();
  const int d = blockIdx.x * kLlWaves + (threadIdx.x >> 6);
  uint32_t* hd = hist + (int64_t)d * nb;
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kWave) {
    const int64_t b = b0 + lane;
    const uint32_t v = b < nb ? hd[b] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (b < nb) hd[b] = carry + inc - v;
    carry += __shfl(inc, kWave - 1);
  }
  if (lane == 0) tot[d] = carry;
}

// exclusive scan of 256 LDS words in place (thread t owns a[t])
__device__ __forceinline__ void pl_excl_scan256(uint32_t* a, uint32_t* wt) {
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const uint32_t v = a[t];
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == kWave - 1) wt[w] = inc;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (int ww = 0; ww < kLlWaves; ++ww)
    if (ww < w) before += wt[ww];
  a[t] = before + inc - v;
  __syncthreads();
}

// The stable scatter of one tile: element e goes to (first position of its digit) + (the
// block's offset in the digit) + (elements of the tile before e with its digit) -- a rank,
// never a grabbed slot, so the output is a function of the keys alone.
__global__ void __launch_bounds__(kLlThreads) pl_scatter_kernel(
    int64_t n, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sp,
    uint32_t* __restrict__ dk, uint32_t* __restrict__ dp, int shift,
    const uint32_t* __restrict__ hist, const uint32_t* __restrict__ tot) {
  __shared__ uint32_t base[256], wc[kLlWaves][256], wt[kLlWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const int64_t nb = gridDim.x, i0 = (int64_t)blockIdx.x * kPlTile;
  const int count = (int)min((int64_t)kPlTile, n - i0);
  base[t] = tot[t];
#pragma unroll
  for (int ww = 0; ww < kLlWaves; ++ww) wc[ww][t] = 0u;
  __syncthreads();
  pl_excl_scan256(base, wt);
  base[t] += hist[(int64_t)t * nb + blockIdx.x];
  __syncthreads();
  const u64 lt = (1ull << lane) - 1ull;
  for (int j0 = 0; j0 < count; j0 += kLlThreads) {
    const int j = j0 + t;
    const bool valid = j < count;
    const uint32_t key = valid ? sk[i0 + j] : 0u;
    const uint32_t pv = valid ? sp[i0 + j] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    u64 m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const u64 bb = __ballot(on);
      m &= on ? bb : ~bb;
    }
    const uint32_t rank = (uint32_t)__popcll(m & lt);
    if (valid && rank == 0) wc[w][d] = (uint32_t)__popcll(m);
    __syncthreads();
    if (valid) {
      uint32_t pos = base[d] + rank;
      for (int ww = 0; ww < w; ++ww) pos += wc[ww][d];
      if ((int64_t)pos < n) {
        dk[pos] = key;
        dp[pos] = pv;
      }
    }
    __syncthreads();
    {
      uint32_t s = 0;
#pragma unroll
      for (int ww = 0; ww < kLlWaves; ++ww) {
        s += wc[ww][t];
        wc[ww][t] = 0u;
      }
      base[t] += s;
    }
    __syncthreads();
  }
}

// rowptr[r] = the first sorted position whose key is >= r (r in [0, n]: rowptr[n] = the
// number of endpoints of real pairs); ent = the payloads, -1 past rowptr[n]
__global__ void __launch_bounds__(kLlThreads) pl_rows_kernel(
    int64_t E, int64_t n, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pay,
    int32_t* __restrict__ rowptr, int32_t* __restrict__ ent) {
  const int64_t t0 = (int64_t)blockIdx.x * kLlThreads + threadIdx.x;
  const int64_t nt = (int64_t)gridDim.x * kLlThreads;
  for (int64_t r = t0; r <= n; r += nt) {
    int64_t lo = 0, hi = E;
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if ((int64_t)keys[mid] < r)
        lo = mid + 1;
      else
        hi = mid;
    }
    rowptr[r] = (int32_t)lo;
  }
  for (int64_t i = t0; i < E; i += nt)
    ent[i] = (int64_t)keys[i] >= n ? -1 : (int32_t)pay[i];
}

// tab[2m] = the long row with a chunk (not its first) starting in window m, tab[2m + 1] =
// that chunk's first position; -1 / -1 when there is none
__global__ void __launch_bounds__(kLlThreads) pl_chunks_kernel(int64_t nwin, int64_t n,
                                                              const int32_t* __restrict__ rowptr,
                                                              int32_t* __restrict__ tab) {
  for (int64_t m = (int64_t)blockIdx.x * kLlThreads + threadIdx.x; m < nwin;
       m += (int64_t)gridDim.x * kLlThreads) {
    const int64_t pos = m * kPlChunk;
    int32_t row = -1, start = -1;
    if (pos < (int64_t)rowptr[n]) {
      int64_t lo = 0, hi = n;  // rowptr[lo] <= pos < rowptr[hi]
      for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)rowptr[mid] <= pos)
          lo = mid;
        else
          hi = mid;
      }
      const int64_t b = rowptr[lo], e = rowptr[lo + 1];
      if (e - b > kPlChunk) {
        const int64_t q = b + (pos - b + kPlChunk - 1) / kPlChunk * kPlChunk;
        if (q > b && q < e) {
          row = (int32_t)lo;
          start = (int32_t)q;
        }
      }
    }
    tab[2 * m] = row;
    tab[2 * m + 1] = start;
  }
}

// ---------------------------------------------------------------- link_bce_fwd ----

template <typename T>
__global__ void __launch_bounds__(kLlThreads) lb_fwd_kernel(
    int64_t P, int F, const T* __restrict__ h, int64_t ld, int64_t n,
    const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const float* __restrict__ y, const float* __restrict__ w, float winv, float* __restrict__ z,
    float* __restrict__ part, int32_t* __restrict__ padpart) {
  __shared__ float zs[kFwdTile];
  __shared__ uint8_t fl[kFwdTile];
  __shared__ float wsum[kLlWaves];
  __shared__ int wpad[kLlWaves];
  constexpr int V = Pk<T>::V;
  constexpr int UNROLL = 4;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int QP = F / V;    // lanes per pair
  const int PPW = 64 / QP;  // pairs per wave-instruction
  const int slot = lane / QP, q = lane % QP;
  const int64_t base = (int64_t)blockIdx.x * kFwdTile;
  const int count = (int)min((int64_t)kFwdTile, P - base);
  for (int i0 = wv * PPW * UNROLL; i0 < count; i0 += kLlWaves * PPW * UNROLL) {
    float acc[UNROLL];
    bool pad[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int i = i0 + u * PPW + slot;
      acc[u] = 0.f;
      pad[u] = false;
      if (i < count) {
        const int64_t a = src[base + i], b = dst[base + i];
        if ((uint64_t)a < (uint64_t)n && (uint64_t)b < (uint64_t)n)
          acc[u] = pk_dot(pk_load(h + a * ld + V * q), pk_load(h + b * ld + V * q));
        else
          pad[u] = true;
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float v = acc[u];
      for (int o = 1; o < QP; o <<= 1) v += __shfl_xor(v, o);
      const int i = i0 + u * PPW + slot;
      if (q == 0 && i < count) {
        const float zv = pad[u] ? __builtin_nanf("") : v;
        z[base + i] = zv;
        zs[i] = zv;
        fl[i] = pad[u] ? 1 : 0;
      }
    }
  }
  __syncthreads();
  // the tile's loss with every lane busy: thread t takes pairs t, t + 256, ... in order
  float acc = 0.f;
  int np = 0;
  for (int i = threadIdx.x; i < count; i += kLlThreads) {
    if (fl[i]) {
      ++np;
      continue;
    }
    const float zv = zs[i];
    const float ww = w != nullptr ? w[base + i] : winv;
    const float l = fmaf(-zv, y[base + i], fmaxf(zv, 0.f)) + log1pf(expf(-fabsf(zv)));
    acc = fmaf(ww, l, acc);
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    acc += __shfl_xor(acc, o);
    np += __shfl_xor(np, o);
  }
  if (lane == 0) {
    wsum[wv] = acc;
    wpad[wv] = np;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    int c = 0;
    for (int k = 0; k < kLlWaves; ++k) {
      s += wsum[k];
      c += wpad[k];
    }
    part[blockIdx.x] = s;
    padpart[blockIdx.x] = c;
  }
}

// the blocks' partials in a fixed order: thread t strides them, xor tree, waves ascending
__global__ void __launch_bounds__(kFinThreads) lb_loss_final_kernel(
    int64_t nb, const float* __restrict__ part, const int32_t* __restrict__ padpart,
    float* __restrict__ loss, int32_t* __restrict__ npad) {
  __shared__ float ws[kFinThreads / kWave];
  __shared__ int wp[kFinThreads / kWave];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  float s = 0.f;
  int c = 0;
  for (int64_t b = threadIdx.x; b < nb; b += kFinThreads) {
    s += part[b];
    c += padpart[b];
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    s += __shfl_xor(s, o);
    c += __shfl_xor(c, o);
  }
  if (lane == 0) {
    ws[wv] = s;
    wp[wv] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    int k = 0;
    for (int i = 0; i < kFinThreads / kWave; ++i) {
      t += ws[i];
      k += wp[i];
    }
    loss[0] = t;
    npad[0] = k;
  }
}

// ---------------------------------------------------------------- link_bce_bwd ----

// g = gloss w (sigmoid(z) - y) as (1 - y) sigmoid(z) - y sigmoid(-z), in fp64: neither a
// saturated sigmoid nor a soft target near it cancels
__device__ __forceinline__ float lb_grad(float z, float y, float w, float gl) {
  const double zd = (double)z;
  const double e = exp(-fabs(zd));
  const double inv = 1.0 / (1.0 + e);
  const double sp = zd >= 0.0 ? inv : e * inv;
  const double sn = zd >= 0.0 ? e * inv : inv;
  return (float)((double)gl * (double)w * ((1.0 - (double)y) * sp - (double)y * sn));
}

// where link_bce_bwd's per-pair factor comes from (pair_grad.h): recomputed from the stored
// logit, the target and the weight
struct LbBceG {
  const float *z, *y, *w;
  float winv;
  bool ok() const { return z != nullptr && y != nullptr; }
  __device__ __forceinline__ float at(int64_t p, float gl) const {
    return lb_grad(z[p], y[p], w != nullptr ? w[p] : winv, gl);
  }
};

struct PlLayout {
  int64_t nb;
  size_t keys[2], pay[2], hist, tot, total;
};

static PlLayout pl_layout(int64_t P) {
  PlLayout L;
  const int64_t E = 2 * P;
  L.nb = E > 0 ? (E + kPlTile - 1) / kPlTile : 1;
  size_t off = 0;
  for (int i = 0; i < 2; ++i) {
    L.keys[i] = off;
    off += pg_align((size_t)E * 4);
  }
  for (int i = 0; i < 2; ++i) {
    L.pay[i] = off;
    off += pg_align((size_t)E * 4);
  }
  L.hist = off;
  off += pg_align((size_t)256 * L.nb * 4);
  L.tot = off;
  off += pg_align((size_t)256 * 4);
  L.total = off;
  return L;
}

static int64_t fwd_blocks(int64_t P) { return P > 0 ? (P + kFwdTile - 1) / kFwdTile : 1; }

}  // namespace msha

using namespace msha;

extern "C" int msha_negative_sample(int64_t n_pos, int32_t k, const int64_t* src, int64_t n_rows,
                                    int64_t n_cand, int64_t n_edges, const int32_t* rowptr,
                                    const int32_t* col, const uint8_t* rowflag,
                                    int64_t col_offset, uint64_t seed, uint64_t offset,
                                    int64_t* src_rep, int64_t* dst_neg, msha_stream_t stream) {
  MSHA_ARG_CHECK(n_pos >= 0 && k >= 1 && n_rows >= 0 && n_edges >= 0,
                 "negative_sample: bad sizes (n_pos >= 0, k >= 1)");
  MSHA_ARG_CHECK(n_cand >= 0 && n_cand < ((int64_t)1 << 31) && n_edges < ((int64_t)1 << 31),
                 "negative_sample: n_cand and n_edges must be below 2^31");
  MSHA_ARG_CHECK(n_pos * (int64_t)k < ((int64_t)1 << 40), "negative_sample: too many draws");
  if (n_pos == 0) return MSHA_OK;
  MSHA_ARG_CHECK(src && rowptr && src_rep && dst_neg && (col != nullptr || n_edges == 0),
                 "negative_sample: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Dropout dp = make_dropout(0.f, seed, offset, s);
  const int64_t total = n_pos * k;
  hipLaunchKernelGGL(ll_negative_kernel, dim3(grid_for(total, kLlThreads, 1 << 16)),
                     dim3(kLlThreads), 0, s, total, (int)k, src, n_rows, (int32_t)n_cand, n_edges,
                     rowptr, col, rowflag, col_offset, dp, src_rep, dst_neg);
  return check_launch("negative_sample");
}

extern "C" int32_t msha_pair_plan_chunk(void) { return kPlChunk; }

extern "C" int64_t msha_pair_plan_chunk_slots(int64_t n_pairs) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs) return 0;
  return pg_windows(n_pairs);
}

extern "C" size_t msha_pair_plan_workspace_size(int64_t n_pairs) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs) return 0;
  return pl_layout(n_pairs).total;
}

extern "C" int msha_pair_plan(int64_t n_pairs, int64_t n, const int64_t* src, const int64_t* dst,
                              int32_t* rowptr, int32_t* ent, int32_t* chunk_tab, void* ws,
                              size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(n_pairs >= 0 && n >= 1, "pair_plan: bad sizes (n_pairs >= 0, n >= 1)");
  MSHA_ARG_CHECK(n_pairs <= kPgMaxPairs, "pair_plan: 2 * n_pairs must be below 2^31");
  MSHA_ARG_CHECK(n < ((int64_t)1 << 31) - 1, "pair_plan: n must be below 2^31 - 1");
  MSHA_ARG_CHECK(rowptr && chunk_tab && (n_pairs == 0 || (src && dst && ent)),
                 "pair_plan: null pointer");
  const PlLayout L = pl_layout(n_pairs);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= L.total && ((uintptr_t)ws % 16) == 0,
                 "pair_plan: workspace too small or unaligned (msha_pair_plan_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t E = 2 * n_pairs;
  char* w = (char*)ws;
  uint32_t* keys[2] = {(uint32_t*)(w + L.keys[0]), (uint32_t*)(w + L.keys[1])};
  uint32_t* pay[2] = {(uint32_t*)(w + L.pay[0]), (uint32_t*)(w + L.pay[1])};
  uint32_t* hist = (uint32_t*)(w + L.hist);
  uint32_t* tot = (uint32_t*)(w + L.tot);
  const dim3 blk(kLlThreads);
  int cur = 0;
  if (E > 0) {
    hipLaunchKernelGGL(pl_keys_kernel, dim3(grid_for(E, kLlThreads, 1 << 16)), blk, 0, s, n_pairs,
                       (uint32_t)n, src, dst, keys[0], pay[0]);
    int bits = 0;  // of the largest key, n (the padding endpoints)
    while (((int64_t)1 << bits) <= n) ++bits;
    for (int shift = 0; shift < bits; shift += 8) {
      const int a = cur, b = cur ^ 1;
      hipLaunchKernelGGL(pl_hist_kernel, dim3((unsigned)L.nb), blk, 0, s, E, keys[a], shift, hist);
      hipLaunchKernelGGL(pl_scan_kernel, dim3(256 / kLlWaves), blk, 0, s, L.nb, hist, tot);
      hipLaunchKernelGGL(pl_scatter_kernel, dim3((unsigned)L.nb), blk, 0, s, E, keys[a], pay[a],
                         keys[b], pay[b], shift, hist, tot);
      cur = b;
    }
  }
  hipLaunchKernelGGL(pl_rows_kernel, dim3(grid_for(E > n ? E : n + 1, kLlThreads, 1 << 16)), blk, 0,
                     s, E, n, keys[cur], pay[cur], rowptr, ent);
  const int64_t nwin = pg_windows(n_pairs);
  hipLaunchKernelGGL(pl_chunks_kernel, dim3(grid_for(nwin, kLlThreads, 1 << 16)), blk, 0, s, nwin,
                     n, rowptr, chunk_tab);
  return check_launch("pair_plan");
}

extern "C" int msha_link_bce_supported(int32_t feat, int32_t dtype) {
  return pg_width_ok(feat, dtype) ? 1 : 0;
}

extern "C" size_t msha_link_bce_fwd_workspace_size(int64_t n_pairs) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs) return 0;
  return 2 * pg_align((size_t)fwd_blocks(n_pairs) * 4);
}

extern "C" size_t msha_link_bce_bwd_workspace_size(int64_t n_pairs, int32_t feat) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs || feat < 1) return 0;
  return pg_workspace_bytes(n_pairs, feat);
}

extern "C" int msha_link_bce_fwd(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                 int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                                 const float* target, const float* weight, float* z, float* loss,
                                 int32_t* n_pad, void* ws, size_t ws_bytes,
                                 msha_stream_t stream) {
  const int rc = pg_table_check("link_bce_fwd", n_pairs, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(src && dst && target && z && loss && n_pad, "link_bce_fwd: null pointer");
  const int64_t nb = fwd_blocks(n_pairs);
  const size_t half = pg_align((size_t)nb * 4);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= 2 * half && ((uintptr_t)ws % 16) == 0,
                 "link_bce_fwd: workspace too small or unaligned "
                 "(msha_link_bce_fwd_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  int32_t* padpart = (int32_t*)((char*)ws + half);
  const float winv = (float)(1.0 / (double)n_pairs);
  if (dtype == MSHA_DTYPE_BF16)
    hipLaunchKernelGGL(lb_fwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(kLlThreads), 0, s, n_pairs,
                       (int)feat, (const bf16_t*)h, ld, n, src, dst, target, weight, winv, z, part,
                       padpart);
  else
    hipLaunchKernelGGL(lb_fwd_kernel<float>, dim3((unsigned)nb), dim3(kLlThreads), 0, s, n_pairs,
                       (int)feat, (const float*)h, ld, n, src, dst, target, weight, winv, z, part,
                       padpart);
  hipLaunchKernelGGL(lb_loss_final_kernel, dim3(1), dim3(kFinThreads), 0, s, nb, part, padpart,
                     loss, n_pad);
  return check_launch("link_bce_fwd");
}

static LbBceG lb_factor(int64_t n_pairs, const float* z, const float* target,
                        const float* weight) {
  return {z, target, weight, (float)(1.0 / (double)n_pairs)};
}

extern "C" int msha_link_bce_bwd(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                 int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                                 const float* target, const float* weight, const float* z,
                                 const float* gloss, const int32_t* plan_rowptr,
                                 const int32_t* plan_ent, const int32_t* plan_chunk_tab, float* dH,
                                 void* ws, size_t ws_bytes, msha_stream_t stream) {
  const int rc = pg_table_check("link_bce_bwd", n_pairs, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  return pg_run("link_bce_bwd", "msha_link_bce_bwd_workspace_size", n_pairs, feat, dtype, h, ld,
                n, src, dst, plan_rowptr, plan_ent, plan_chunk_tab,
                lb_factor(n_pairs, z, target, weight), gloss, dH, ws, ws_bytes, stream,
                PgAllRows{});
}

extern "C" int msha_link_bce_bwd_rows(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                      int64_t ld, int64_t n, const int64_t* src,
                                      const int64_t* dst, const float* target,
                                      const float* weight, const float* z, const float* gloss,
                                      const int32_t* plan_rowptr, const int32_t* plan_ent,
                                      const int32_t* plan_chunk_tab, const int32_t* rows,
                                      const int32_t* n_rows, int64_t cap, float* vals, void* ws,
                                      size_t ws_bytes, msha_stream_t stream) {
  const int rc = pg_table_check("link_bce_bwd_rows", n_pairs, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(rows && n_rows, "link_bce_bwd_rows: null pointer");
  MSHA_ARG_CHECK(cap == pg_rows_cap(n, n_pairs),
                 "link_bce_bwd_rows: cap must be min(n, 2 * n_pairs) (msha_plan_rows)");
  return pg_run("link_bce_bwd_rows", "msha_link_bce_bwd_workspace_size", n_pairs, feat, dtype, h,
                ld, n, src, dst, plan_rowptr, plan_ent, plan_chunk_tab,
                lb_factor(n_pairs, z, target, weight), gloss, vals, ws, ws_bytes, stream,
                PgListRows{rows, n_rows, cap});
}
