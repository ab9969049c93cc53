// Device-side evaluation (train.py:239-282, model.py:66-92): what test() does with a
// .cpu().item() per value and sklearn on the host, as launches on the score table.
//
//   eval_rows   one launch per test batch: gather output[source_index] (fp32 or bf16,
//               widened exactly), append the rows to an (n, C) fp32 store, nll[b] =
//               -row[y], pred[b] = lowest index of the row maximum, conf[y, pred] += 1.
//   eval_loss   the printed loss from nll: mean over chunks of the chunk's mean, every
//               sum in a fixed order (lanes stride a chunk, xor tree, chunks ascending
//               per wave, waves ascending) -- no float atomics.
//   rank_auc    per column of the store: P, Nn and the tie-aware rank statistic
//               U2 = sum over groups of equal score of pos_g (2 neg_below_g + neg_g),
//               so AUC = U2 / (2 P Nn) on the host in fp64.  Integers only on the device:
//               the result does not depend on the order of execution.
//
// rank_auc sorts each column's keys (order_key.h's ra_key of the fp32 score: order-preserving,
// -0.0 folded onto +0.0; the positive bit rides as a one-byte payload) with a stable LSD
// radix sort, 8-bit digits, 4 passes.  A column of at most kRaTile keys is sorted in the
// LDS of one block (one launch for all columns).  Longer columns take, per pass, per-block
// digit histograms, one scan of the (column, digit, block) table and a ranked scatter,
// batched over the columns in grid.y.  The statistic then comes from one scan over the
// sorted order: with the exclusive prefix counts (neg, pos) at a group's start s and the
// inclusive counts at its end e, the group adds (pos_e - pos_s) * (neg_s + neg_e).
#include "common.h"
#include "order_key.h"

namespace msha {

typedef unsigned long long u64;

constexpr int kEvThreads = 256;
constexpr int kEvWaves = kEvThreads / kWave;
constexpr int kRaItems = 16;
constexpr int kRaTile = kEvThreads * kRaItems;  // keys per block and pass; the LDS cut

// ---------------------------------------------------------------- eval_rows ----

// (v1, i1) ahead of (v2, i2) in "row maximum, lowest index": a NaN is the maximum (as
// torch.max and numpy.argmax have it), equal values go to the lower index; i < 0: no entry
__device__ __forceinline__ bool ev_wins(float v1, int i1, float v2, int i2) {
  if (i1 < 0) return false;
  if (i2 < 0) return true;
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 != n2) return n1;
  if (!n1 && v1 != v2) return v1 > v2;
  return i1 < i2;
}

__device__ __forceinline__ bool ev_nonfinite(uint32_t bits) {
  return (bits & 0x7f800000u) == 0x7f800000u;
}

// One wave per row.  Validity is decided from src[b] and labels[b] alone, before any load
// through them: a bad row reads nothing of the table.
template <typename T>
__global__ void __launch_bounds__(kEvThreads) eval_rows_kernel(
    int64_t N, int C, int64_t B, const T* __restrict__ table, int64_t ld,
    const int64_t* __restrict__ src, const int64_t* __restrict__ labels,
    float* __restrict__ store, int64_t* __restrict__ labels_out, float* __restrict__ nll,
    int64_t* __restrict__ pred, u64* __restrict__ conf, u64* __restrict__ counters) {
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * kEvThreads + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * kEvThreads) >> 6;
  for (int64_t b = wave; b < B; b += nwaves) {
    int64_t i = src != nullptr ? src[b] : b;
    const int64_t y = labels[b];
    if (i < 0 && i >= -N) i += N;  // torch's wrap of output[source_index]
    float* out = store + b * C;
    if (!(i >= 0 && i < N && y >= 0 && y < C)) {
      for (int c = lane; c < C; c += kWave) out[c] = 0.f;
      if (lane == 0) {
        nll[b] = 0.f;
        pred[b] = -1;
        labels_out[b] = -1;
        atomicAdd(counters + 1, 1ull);
      }
      continue;
    }
    const T* row = table + i * ld;
    float best = 0.f, vy = 0.f;
    int bi = -1, nf = 0;
    for (int c = lane; c < C; c += kWave) {
      const float v = to_f32(row[c]);
      out[c] = v;
      nf += ev_nonfinite(__float_as_uint(v)) ? 1 : 0;
      if (c == (int)y) vy = v;
      if (ev_wins(v, c, best, bi)) {
        best = v;
        bi = c;
      }
    }
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      nf += __shfl_xor(nf, o);
      if (ev_wins(ov, oi, best, bi)) {
        best = ov;
        bi = oi;
      }
    }
    vy = __shfl(vy, (int)(y & (kWave - 1)));
    if (lane == 0) {
      nll[b] = -vy;
      pred[b] = bi;
      labels_out[b] = y;
      atomicAdd(conf + y * C + bi, 1ull);
      if (nf != 0) atomicAdd(counters, (u64)nf);
    }
  }
}

// ---------------------------------------------------------------- eval_loss ----

constexpr int kLossWaves = 16;

__global__ void __launch_bounds__(kLossWaves* kWave) eval_loss_kernel(
    int64_t n, int64_t chunk, const float* __restrict__ nll, float* __restrict__ loss) {
  __shared__ float part[kLossWaves];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int64_t nchunks = (n + chunk - 1) / chunk;
  float acc = 0.f;
  for (int64_t c = w; c < nchunks; c += kLossWaves) {
    const int64_t r0 = c * chunk, r1 = min(n, r0 + chunk);
    float s = 0.f;
    for (int64_t i = r0 + lane; i < r1; i += kWave) s += nll[i];
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) s += __shfl_xor(s, o);
    acc += s / (float)(r1 - r0);
  }
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < kLossWaves; ++k) s += part[k];
    loss[0] = s / (float)nchunks;
  }
}

// ----------------------------------------------------------------- rank_auc ----

__device__ __forceinline__ uint8_t ra_pos(int64_t label, const int32_t* cls, int k, int binary) {
  if (binary) return label != 0 ? 1 : 0;
  return label == (int64_t)(cls != nullptr ? cls[k] : k) ? 1 : 0;
}

// (neg, pos) counts of at most 256 elements in one word, and as a 64-bit pair (n < 2^31)
__device__ __forceinline__ u64 ra_unpack(uint32_t x) {
  return ((u64)(x >> 16) << 32) | (u64)(x & 0xffffu);
}

// One stable pass over `count` keys at sk / sp (a block's tile, in order): element e goes
// to base[digit] + (elements of the tile before e with its digit).  base (LDS, 256 words)
// holds each digit's first position on entry and is consumed; wc: kEvWaves x 256 LDS
// words, zero on entry and on exit.  Positions at or past `limit` are not written.
__device__ __forceinline__ void ra_scatter_tile(const uint32_t* sk, const uint8_t* sp,
                                                uint32_t* dk, uint8_t* dp, int count, int shift,
                                                uint32_t limit, uint32_t* base,
                                                uint32_t (*wc)[256]) {
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const u64 lt = (1ull << lane) - 1ull;
  for (int j0 = 0; j0 < count; j0 += kEvThreads) {
    const int j = j0 + t;
    const bool valid = j < count;
    const uint32_t key = valid ? sk[j] : 0u;
    const uint8_t pay = valid ? sp[j] : (uint8_t)0;
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
      if (pos < limit) {
        dk[pos] = key;
        dp[pos] = pay;
      }
    }
    __syncthreads();
    {
      uint32_t s = 0;
#pragma unroll
      for (int ww = 0; ww < kEvWaves; ++ww) {
        s += wc[ww][t];
        wc[ww][t] = 0u;
      }
      base[t] += s;
    }
    __syncthreads();
  }
}

// exclusive scan of 256 words in LDS, in place (thread t owns a[t]); returns the total
__device__ __forceinline__ uint32_t ra_excl_scan256(uint32_t* a, uint32_t* wt) {
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
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int ww = 0; ww < kEvWaves; ++ww) {
    if (ww < w) before += wt[ww];
    total += wt[ww];
  }
  a[t] = before + inc - v;
  __syncthreads();
  return total;
}

struct RaCarry {
  u64 sum;    // (neg << 32 | pos) of every element before the current one
  u64 start;  // the same counts at the start of the group that is open
  bool any;   // a group started since the carry was set
};

// The scan over sorted elements [i0, i0 + count) of a column of n (keys / pay: the whole
// column).  Returns this thread's share of U2 for the groups that END in the range and
// leaves the carries for the next range; nf: the thread's count of non-finite scores.
// ex: 256 LDS words, wt / wm: kEvWaves LDS words each.
__device__ __forceinline__ u64 ra_u2_range(const uint32_t* keys, const uint8_t* pay, int64_t i0,
                                           int count, int64_t n, RaCarry& cy, uint32_t& nf,
                                           uint32_t* ex, uint32_t* wt, uint32_t* wm) {
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  u64 acc = 0;
  for (int j0 = 0; j0 < count; j0 += kEvThreads) {
    const int j = j0 + t;
    const bool valid = j < count;
    const int64_t i = i0 + j;
    const uint32_t key = valid ? keys[i] : 0u;
    const bool isstart = valid && (i == 0 || keys[i - 1] != key);
    const bool isend = valid && (i == n - 1 || keys[i + 1] != key);
    const uint32_t v = valid ? (pay[i] ? 1u : 0x10000u) : 0u;
    nf += valid && ev_nonfinite(ra_bits(key)) ? 1u : 0u;
    uint32_t inc = v, smax = isstart ? (uint32_t)(t + 1) : 0u;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o);
      const uint32_t s = __shfl_up(smax, o);
      if (lane >= o) {
        inc += u;
        smax = max(smax, s);
      }
    }
    if (lane == kWave - 1) {
      wt[w] = inc;
      wm[w] = smax;
    }
    __syncthreads();
    uint32_t tot = 0, last = 0;
#pragma unroll
    for (int ww = 0; ww < kEvWaves; ++ww) {
      if (ww < w) {
        inc += wt[ww];
        smax = max(smax, wm[ww]);
      }
      tot += wt[ww];
      last = max(last, wm[ww]);
    }
    ex[t] = inc - v;
    __syncthreads();
    if (isend) {
      const u64 endp = cy.sum + ra_unpack(inc);
      const u64 startp = smax > 0 ? cy.sum + ra_unpack(ex[smax - 1]) : cy.start;
      const u64 posg = (endp & 0xffffffffull) - (startp & 0xffffffffull);
      acc += posg * ((startp >> 32) + (endp >> 32));
    }
    if (last > 0) {
      cy.start = cy.sum + ra_unpack(ex[last - 1]);
      cy.any = true;
    }
    cy.sum += ra_unpack(tot);
    __syncthreads();
  }
  return acc;
}

// block sum of a 64-bit and a 32-bit integer (LDS integer atomics: exact in any order)
__device__ __forceinline__ void ra_block_sum(u64 a, uint32_t b, u64* sa, uint32_t* sb) {
  if (threadIdx.x == 0) {
    *sa = 0ull;
    *sb = 0u;
  }
  __syncthreads();
  if (a != 0ull) atomicAdd(sa, a);
  if (b != 0u) atomicAdd(sb, b);
  __syncthreads();
}

// columns of at most kRaTile keys: block k sorts column k in LDS and scans it
__global__ void __launch_bounds__(kEvThreads) ra_lds_kernel(
    int n, const float* __restrict__ scores, int64_t ld, const int64_t* __restrict__ labels,
    const int32_t* __restrict__ cls, int binary, int64_t* __restrict__ out) {
  __shared__ uint32_t kA[kRaTile], kB[kRaTile];
  __shared__ uint8_t pA[kRaTile], pB[kRaTile];
  __shared__ uint32_t h[256], wc[kEvWaves][256], ex[256], wt[kEvWaves], wm[kEvWaves];
  __shared__ u64 s_u2;
  __shared__ uint32_t s_nf;
  const int t = threadIdx.x, k = blockIdx.x;
  for (int j = t; j < n; j += kEvThreads) {
    kA[j] = ra_key(__float_as_uint(scores[(int64_t)j * ld + k]));
    pA[j] = ra_pos(labels[j], cls, k, binary);
  }
#pragma unroll
  for (int ww = 0; ww < kEvWaves; ++ww) wc[ww][t] = 0u;
  uint32_t* sk = kA;
  uint32_t* dk = kB;
  uint8_t* sp = pA;
  uint8_t* dp = pB;
  for (int shift = 0; shift < 32; shift += 8) {
    h[t] = 0u;
    __syncthreads();  // (the fill / the previous pass's writes)
    for (int j = t; j < n; j += kEvThreads) atomicAdd(&h[(sk[j] >> shift) & 255u], 1u);
    __syncthreads();
    ra_excl_scan256(h, wt);
    ra_scatter_tile(sk, sp, dk, dp, n, shift, (uint32_t)n, h, wc);
    uint32_t* tk = sk; sk = dk; dk = tk;
    uint8_t* tp = sp; sp = dp; dp = tp;
  }
  RaCarry cy = {0ull, 0ull, false};
  uint32_t nf = 0;
  const u64 acc = ra_u2_range(sk, sp, 0, n, n, cy, nf, ex, wt, wm);
  ra_block_sum(acc, nf, &s_u2, &s_nf);
  if (t == 0) {
    out[4 * k + 0] = (int64_t)(cy.sum & 0xffffffffull);
    out[4 * k + 1] = (int64_t)(cy.sum >> 32);
    out[4 * k + 2] = (int64_t)s_u2;
    out[4 * k + 3] = (int64_t)s_nf;
  }
}

// (n, C) scores -> column-major keys and positive bits, through a 64 x 64 LDS transpose
__global__ void __launch_bounds__(kEvThreads) ra_keys_kernel(
    int64_t n, int C, const float* __restrict__ scores, int64_t ld,
    const int64_t* __restrict__ labels, const int32_t* __restrict__ cls, int binary,
    uint32_t* __restrict__ keys, uint8_t* __restrict__ pay) {
  __shared__ uint32_t tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  for (int r = ty; r < 64; r += kEvWaves) {
    if (r0 + r < n && c0 + tx < C)
      tile[r][tx] = __float_as_uint(scores[(r0 + r) * ld + c0 + tx]);
  }
  __syncthreads();
  const int64_t row = r0 + tx;
  if (row < n) {
    const int64_t y = labels[row];
    for (int c = ty; c < 64 && c0 + c < C; c += kEvWaves) {
      const int k = c0 + c;
      keys[(int64_t)k * n + row] = ra_key(tile[tx][c]);
      pay[(int64_t)k * n + row] = ra_pos(y, cls, k, binary);
    }
  }
}

// the same for a few columns (C < kRaNarrow): a thread per row, coalesced column writes
// (the 64-column tile above runs one lane in 64 at C = 1: 160 us at 4M rows)
constexpr int kRaNarrow = 32;
__global__ void __launch_bounds__(kEvThreads) ra_keys_narrow_kernel(
    int64_t n, int C, const float* __restrict__ scores, int64_t ld,
    const int64_t* __restrict__ labels, const int32_t* __restrict__ cls, int binary,
    uint32_t* __restrict__ keys, uint8_t* __restrict__ pay) {
  for (int64_t row = (int64_t)blockIdx.x * kEvThreads + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * kEvThreads) {
    const int64_t y = labels[row];
    for (int k = 0; k < C; ++k) {
      keys[(int64_t)k * n + row] = ra_key(__float_as_uint(scores[row * ld + k]));
      pay[(int64_t)k * n + row] = ra_pos(y, cls, k, binary);
    }
  }
}

// hist[(k * 256 + digit) * nb + block] = the block's count of the digit in its tile
__global__ void __launch_bounds__(kEvThreads) ra_hist_kernel(
    int64_t n, const uint32_t* __restrict__ keys, int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const int t = threadIdx.x, k = blockIdx.y;
  const int64_t nb = gridDim.x, i0 = (int64_t)blockIdx.x * kRaTile;
  const int count = (int)min((int64_t)kRaTile, n - i0);
  const uint32_t* sk = keys + (int64_t)k * n + i0;
  h[t] = 0u;
  __syncthreads();
  for (int j = t; j < count; j += kEvThreads) atomicAdd(&h[(sk[j] >> shift) & 255u], 1u);
  __syncthreads();
  hist[((int64_t)k * 256 + t) * nb + blockIdx.x] = h[t];
}

// the (digit, block) table of column k: one wave per digit row scans its nb block counts
// in place (exclusive, 64 coalesced entries a step) and leaves the digit's total in
// tot[k * 256 + digit]; the scatter adds the scan over the 256 totals.  (One block a
// column walking the rows serially took 409 us a pass at 4M keys, 3/4 of the whole call.)
__global__ void __launch_bounds__(kEvThreads) ra_scan_kernel(int64_t nb,
                                                             uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ tot) {
  const int lane = lane_id();
  const int d = blockIdx.x * kEvWaves + (threadIdx.x >> 6), k = blockIdx.y;
  uint32_t* hd = hist + ((int64_t)k * 256 + d) * nb;
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
  if (lane == 0) tot[k * 256 + d] = carry;
}

__global__ void __launch_bounds__(kEvThreads) ra_scatter_kernel(
    int64_t n, const uint32_t* __restrict__ sk, const uint8_t* __restrict__ sp,
    uint32_t* __restrict__ dk, uint8_t* __restrict__ dp, int shift,
    const uint32_t* __restrict__ hist, const uint32_t* __restrict__ tot) {
  __shared__ uint32_t base[256], wc[kEvWaves][256], wt[kEvWaves];
  const int t = threadIdx.x, k = blockIdx.y;
  const int64_t nb = gridDim.x, i0 = (int64_t)blockIdx.x * kRaTile;
  const int count = (int)min((int64_t)kRaTile, n - i0);
  base[t] = tot[k * 256 + t];
#pragma unroll
  for (int ww = 0; ww < kEvWaves; ++ww) wc[ww][t] = 0u;
  __syncthreads();
  ra_excl_scan256(base, wt);  // the digit's first position in the column
  base[t] += hist[((int64_t)k * 256 + t) * nb + blockIdx.x];
  __syncthreads();
  const int64_t col = (int64_t)k * n;
  ra_scatter_tile(sk + col + i0, sp + col + i0, dk + col, dp + col, count, shift, (uint32_t)n,
                  base, wc);
}

// per-tile summary of the sorted column: sums[(k * nb + tile) * 4 + {0: counts, 1: counts
// at the last group start inside the tile, 2: a group starts in the tile, 3: non-finite}]
__global__ void __launch_bounds__(kEvThreads) ra_tile_sums_kernel(
    int64_t n, const uint32_t* __restrict__ keys, const uint8_t* __restrict__ pay,
    u64* __restrict__ sums) {
  __shared__ uint32_t ex[256], wt[kEvWaves], wm[kEvWaves];
  __shared__ u64 s_u2;
  __shared__ uint32_t s_nf;
  const int k = blockIdx.y;
  const int64_t nb = gridDim.x, i0 = (int64_t)blockIdx.x * kRaTile;
  const int count = (int)min((int64_t)kRaTile, n - i0);
  const int64_t col = (int64_t)k * n;
  RaCarry cy = {0ull, 0ull, false};
  uint32_t nf = 0;
  ra_u2_range(keys + col, pay + col, i0, count, n, cy, nf, ex, wt, wm);
  ra_block_sum(0ull, nf, &s_u2, &s_nf);
  if (threadIdx.x == 0) {
    u64* s = sums + ((int64_t)k * nb + blockIdx.x) * 4;
    s[0] = cy.sum;
    s[1] = cy.start;
    s[2] = cy.any ? 1ull : 0ull;
    s[3] = (u64)s_nf;
  }
}

// one block per column: the tiles' summaries -> each tile's carries (in place: [0] counts
// before the tile, [1] counts at the start of the group open at the tile's first element),
// and out[k] = {P, Nn, 0, non-finite}.  Thread t walks a run of tiles; the 256 runs are
// combined in order by one thread.
__global__ void __launch_bounds__(kEvThreads) ra_carry_kernel(int64_t nb, u64* __restrict__ sums,
                                                              int64_t* __restrict__ out) {
  __shared__ u64 rsum[256], rstart[256];
  __shared__ uint32_t rany[256];
  __shared__ u64 s_u2;
  __shared__ uint32_t s_nf;
  const int t = threadIdx.x, k = blockIdx.x;
  const int64_t per = (nb + kEvThreads - 1) / kEvThreads;
  const int64_t b0 = min(nb, (int64_t)t * per), b1 = min(nb, b0 + per);
  u64* s = sums + (int64_t)k * nb * 4;
  u64 sum = 0, start = 0;
  uint32_t any = 0, nf = 0;
  for (int64_t b = b0; b < b1; ++b) {
    if (s[4 * b + 2] != 0ull) {
      start = sum + s[4 * b + 1];
      any = 1;
    }
    sum += s[4 * b];
    nf += (uint32_t)s[4 * b + 3];
  }
  rsum[t] = sum;
  rstart[t] = start;
  rany[t] = any;
  ra_block_sum(0ull, nf, &s_u2, &s_nf);  // (its barriers also publish the run summaries)
  if (t == 0) {
    u64 csum = 0, cstart = 0;
    for (int r = 0; r < kEvThreads; ++r) {
      const u64 rs = rsum[r], rst = rstart[r];
      const uint32_t ra = rany[r];
      rsum[r] = csum;
      rstart[r] = cstart;
      if (ra) cstart = csum + rst;
      csum += rs;
    }
    out[4 * k + 0] = (int64_t)(csum & 0xffffffffull);
    out[4 * k + 1] = (int64_t)(csum >> 32);
    out[4 * k + 2] = 0;
    out[4 * k + 3] = (int64_t)s_nf;
  }
  __syncthreads();
  sum = rsum[t];
  start = rstart[t];
  for (int64_t b = b0; b < b1; ++b) {
    const u64 ts = s[4 * b], tst = s[4 * b + 1];
    const bool ta = s[4 * b + 2] != 0ull;
    s[4 * b] = sum;
    s[4 * b + 1] = start;
    if (ta) start = sum + tst;
    sum += ts;
  }
}

__global__ void __launch_bounds__(kEvThreads) ra_u2_kernel(
    int64_t n, const uint32_t* __restrict__ keys, const uint8_t* __restrict__ pay,
    const u64* __restrict__ sums, int64_t* __restrict__ out) {
  __shared__ uint32_t ex[256], wt[kEvWaves], wm[kEvWaves];
  __shared__ u64 s_u2;
  __shared__ uint32_t s_nf;
  const int k = blockIdx.y;
  const int64_t nb = gridDim.x, i0 = (int64_t)blockIdx.x * kRaTile;
  const int count = (int)min((int64_t)kRaTile, n - i0);
  const int64_t col = (int64_t)k * n;
  const u64* s = sums + ((int64_t)k * nb + blockIdx.x) * 4;
  RaCarry cy = {s[0], s[1], false};
  uint32_t nf = 0;
  const u64 acc = ra_u2_range(keys + col, pay + col, i0, count, n, cy, nf, ex, wt, wm);
  ra_block_sum(acc, 0u, &s_u2, &s_nf);
  if (threadIdx.x == 0 && s_u2 != 0ull) atomicAdd((u64*)(out + 4 * k + 2), s_u2);
}

static size_t ra_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct RaLayout {
  int64_t nb;
  size_t keys[2], pay[2], hist, tot, sums, total;
};

static RaLayout ra_layout(int64_t n, int64_t C) {
  RaLayout L;
  L.nb = (n + kRaTile - 1) / kRaTile;
  size_t off = 0;
  for (int i = 0; i < 2; ++i) {
    L.keys[i] = off;
    off += ra_align((size_t)n * C * 4);
  }
  for (int i = 0; i < 2; ++i) {
    L.pay[i] = off;
    off += ra_align((size_t)n * C);
  }
  L.hist = off;
  off += ra_align((size_t)C * 256 * L.nb * 4);
  L.tot = off;
  off += ra_align((size_t)C * 256 * 4);
  L.sums = off;
  off += ra_align((size_t)C * L.nb * 4 * 8);
  L.total = off;
  return L;
}

}  // namespace msha

using namespace msha;

extern "C" int msha_eval_rows(int64_t N, int32_t C, int64_t B, int32_t dtype, const void* table,
                              int64_t ld, const int64_t* src, const int64_t* labels,
                              int64_t row_offset, float* store, int64_t* labels_out, float* nll,
                              int64_t* pred, int64_t* conf, int64_t* counters,
                              msha_stream_t stream) {
  MSHA_ARG_CHECK(N > 0 && C >= 1 && C <= 1024 && B >= 0 && ld >= C && row_offset >= 0,
                 "eval_rows: bad sizes (1 <= C <= 1024, ld >= C)");
  MSHA_ARG_CHECK(dtype == MSHA_DTYPE_F32 || dtype == MSHA_DTYPE_BF16, "eval_rows: bad dtype");
  MSHA_ARG_CHECK(table && labels && store && labels_out && nll && pred && conf && counters,
                 "eval_rows: null pointer");
  if (B == 0) return MSHA_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(grid_for(B, kEvWaves, 1 << 16));
  float* st = store + row_offset * C;
  if (dtype == MSHA_DTYPE_BF16)
    hipLaunchKernelGGL(eval_rows_kernel<bf16_t>, grid, dim3(kEvThreads), 0, s, N, (int)C, B,
                       (const bf16_t*)table, ld, src, labels, st, labels_out + row_offset,
                       nll + row_offset, pred + row_offset, (u64*)conf, (u64*)counters);
  else
    hipLaunchKernelGGL(eval_rows_kernel<float>, grid, dim3(kEvThreads), 0, s, N, (int)C, B,
                       (const float*)table, ld, src, labels, st, labels_out + row_offset,
                       nll + row_offset, pred + row_offset, (u64*)conf, (u64*)counters);
  return check_launch("eval_rows");
}

extern "C" int msha_eval_loss(int64_t n, int64_t chunk, const float* nll, float* loss,
                              msha_stream_t stream) {
  MSHA_ARG_CHECK(n > 0 && chunk > 0 && nll && loss, "eval_loss: bad arguments");
  hipLaunchKernelGGL(eval_loss_kernel, dim3(1), dim3(kLossWaves * kWave), 0, (hipStream_t)stream,
                     n, chunk, nll, loss);
  return check_launch("eval_loss");
}

extern "C" int64_t msha_rank_auc_block_keys(void) { return kRaTile; }

extern "C" size_t msha_rank_auc_workspace_size(int64_t n, int32_t C) {
  if (n <= kRaTile || C < 1) return 0;
  return ra_layout(n, C).total;
}

extern "C" int msha_rank_auc(int64_t n, int32_t C, const float* scores, int64_t ld,
                             const int64_t* labels, const int32_t* cls, int32_t binary,
                             int64_t* out, void* ws, size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 1 && n < ((int64_t)1 << 31) && C >= 1 && C <= 65535 && ld >= C,
                 "rank_auc: bad sizes (1 <= n < 2^31, 1 <= C <= 65535, ld >= C)");
  MSHA_ARG_CHECK(scores && labels && out, "rank_auc: null pointer");
  MSHA_ARG_CHECK(!binary || (C == 1 && cls == nullptr),
                 "rank_auc: binary mode takes one column and no class map");
  hipStream_t s = (hipStream_t)stream;
  if (n <= kRaTile) {
    hipLaunchKernelGGL(ra_lds_kernel, dim3(C), dim3(kEvThreads), 0, s, (int)n, scores, ld, labels,
                       cls, (int)binary, out);
    return check_launch("rank_auc");
  }
  const RaLayout L = ra_layout(n, C);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= L.total && ((uintptr_t)ws % 16) == 0,
                 "rank_auc: workspace too small or unaligned (msha_rank_auc_workspace_size)");
  char* w = (char*)ws;
  uint32_t* keys[2] = {(uint32_t*)(w + L.keys[0]), (uint32_t*)(w + L.keys[1])};
  uint8_t* pay[2] = {(uint8_t*)(w + L.pay[0]), (uint8_t*)(w + L.pay[1])};
  uint32_t* hist = (uint32_t*)(w + L.hist);
  uint32_t* tot = (uint32_t*)(w + L.tot);
  u64* sums = (u64*)(w + L.sums);
  const dim3 blk(kEvThreads), tiles((unsigned)L.nb, (unsigned)C);
  if (C < kRaNarrow)
    hipLaunchKernelGGL(ra_keys_narrow_kernel, dim3(grid_for(n, kEvThreads, 1 << 16)), blk, 0, s, n,
                       (int)C, scores, ld, labels, cls, (int)binary, keys[0], pay[0]);
  else
    hipLaunchKernelGGL(ra_keys_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((C + 63) / 64)),
                       blk, 0, s, n, (int)C, scores, ld, labels, cls, (int)binary, keys[0],
                       pay[0]);
  for (int p = 0; p < 4; ++p) {
    const int a = p & 1, b = a ^ 1;
    hipLaunchKernelGGL(ra_hist_kernel, tiles, blk, 0, s, n, keys[a], 8 * p, hist);
    hipLaunchKernelGGL(ra_scan_kernel, dim3(256 / kEvWaves, (unsigned)C), blk, 0, s, L.nb, hist,
                       tot);
    hipLaunchKernelGGL(ra_scatter_kernel, tiles, blk, 0, s, n, keys[a], pay[a], keys[b], pay[b],
                       8 * p, hist, tot);
  }
  hipLaunchKernelGGL(ra_tile_sums_kernel, tiles, blk, 0, s, n, keys[0], pay[0], sums);
  hipLaunchKernelGGL(ra_carry_kernel, dim3(C), blk, 0, s, L.nb, sums, out);
  hipLaunchKernelGGL(ra_u2_kernel, tiles, blk, 0, s, n, keys[0], pay[0], sums, out);
  return check_launch("rank_auc");
}
