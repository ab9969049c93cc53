// LLP's representation-matching term (LLP.py:34-35, :237):
//
//   loss = 1 - mean_p cos(h[rows[p]], T[rows[p]]),   T never differentiated
//
// Student and teacher are indexed by the same node id, so every occurrence of row r adds
// the same cosine and the same gradient row: with c_r the occurrences of r and P_v the
// valid entries,
//
//   loss  = 1 - (1 / P_v) sum_r c_r cos_r
//   dH[r] = -(gloss / P_v) c_r (T[r] / (ns_r nt_r) - cos_r h[r] / (ns_r |h[r]|))
//
// ns = max(|h[r]|, eps), nt = max(|T[r]|, eps), eps = 1e-8: torch's cosine_similarity, which
// clamps each norm on its own, in place and outside autograd, so the backward still sees
// d|h| / dh = h / |h| of the unclamped norm (0 for a zero row).  Above eps that is
// cos_r h[r] / ns_r^2.  So the term is an
// integer histogram of the list and one pass over the table rows that occur: no (P, F)
// gather, no plan, no sort, no float atomics.  The result is a function of the multiset of
// indices.
//
//   link_match_fwd   zero count -> histogram (exact integer atomics) -> row pass: coef (n, 2),
//                    cos_rows, the loss by link_bce_fwd's discipline (a block owns a fixed
//                    tile of rows, its partial is summed in a fixed order, one block adds the
//                    partials in order).
//   link_match_bwd   dH[r] = -gloss (coef[r, 0] T[r] - coef[r, 1] h[r]), one streaming pass.
#include "common.h"
#include "pair_grad.h"
#include "row_list.h"

// the histogram's form: 1 = equal indices aggregated in an LDS table per block, flushed
// with one global add per distinct row; 0 = one global add per entry (A/B)
#ifndef MATCH_HIST_LDS
#define MATCH_HIST_LDS 1
#endif

namespace msha {

constexpr int kMtThreads = 256;
constexpr int kMtWaves = kMtThreads / kWave;
constexpr int kMtHistTile = 2048;   // entries per block and table fill
constexpr int kMtSlots = 4096;      // LDS table slots (load factor <= 1/2)
constexpr int kMtSlotBits = 12;
constexpr int kMtProbes = 8;        // then the entry goes to global memory directly
constexpr int kMtRowTile = 1024;    // table rows per row-pass block (fixes the loss order)
constexpr int kMtFinThreads = 1024;
constexpr double kMtEps = 1e-8;

// ------------------------------------------------------------------- histogram ----

__global__ void __launch_bounds__(kMtThreads) mt_zero_kernel(int64_t n, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ npad) {
  for (int64_t i = (int64_t)blockIdx.x * kMtThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kMtThreads)
    count[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) npad[0] = 0;
}

__device__ __forceinline__ void mt_global_add(int32_t* p, int32_t v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the block's padding entries to npad[0]: one integer add per block
__device__ __forceinline__ void mt_flush_pad(int np, int32_t* __restrict__ npad) {
  __shared__ int wpad[kMtWaves];
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) np += __shfl_xor(np, o);
  if (lane_id() == 0) wpad[threadIdx.x >> 6] = np;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int k = 0; k < kMtWaves; ++k) c += wpad[k];
    if (c != 0) mt_global_add(npad, c);
  }
}

// count[r] += occurrences of r among the valid entries (r in [0, m)); the others are padding,
// decided before anything is addressed through the entry.  Tiles of kMtHistTile entries go
// through an open-addressing LDS table (key = row, linear probing, at most kMtProbes steps):
// a tile's equal indices meet in one slot and leave as one global add.
__global__ void __launch_bounds__(kMtThreads) mt_hist_lds_kernel(
    int64_t P, int64_t m, const int64_t* __restrict__ rows, int32_t* __restrict__ count,
    int32_t* __restrict__ npad) {
  __shared__ int32_t key[kMtSlots];
  __shared__ int32_t cnt[kMtSlots];
  const int t = threadIdx.x;
  const int64_t ntiles = (P + kMtHistTile - 1) / kMtHistTile;
  int np = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    for (int i = t; i < kMtSlots; i += kMtThreads) {
      key[i] = -1;
      cnt[i] = 0;
    }
    __syncthreads();
    const int64_t base = tile * kMtHistTile;
    const int n_ent = (int)min((int64_t)kMtHistTile, P - base);
    for (int j = t; j < n_ent; j += kMtThreads) {
      const int64_t r64 = rows[base + j];
      if ((uint64_t)r64 >= (uint64_t)m) {
        ++np;
        continue;
      }
      const int32_t r = (int32_t)r64;
      uint32_t s = ((uint32_t)r * 2654435761u) >> (32 - kMtSlotBits);
      bool done = false;
      for (int probe = 0; probe < kMtProbes; ++probe) {
        const int32_t old = atomicCAS(&key[s], -1, r);
        if (old == -1 || old == r) {
          __hip_atomic_fetch_add(&cnt[s], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          done = true;
          break;
        }
        s = (s + 1) & (kMtSlots - 1);
      }
      if (!done) mt_global_add(count + r, 1);
    }
    __syncthreads();
    for (int i = t; i < kMtSlots; i += kMtThreads) {
      const int32_t r = key[i];
      if (r >= 0 && (int64_t)r < m) mt_global_add(count + r, cnt[i]);
    }
    __syncthreads();
  }
  mt_flush_pad(np, npad);
}

// the form without the table: one global add per valid entry
__global__ void __launch_bounds__(kMtThreads) mt_hist_direct_kernel(
    int64_t P, int64_t m, const int64_t* __restrict__ rows, int32_t* __restrict__ count,
    int32_t* __restrict__ npad) {
  int np = 0;
  for (int64_t p = (int64_t)blockIdx.x * kMtThreads + threadIdx.x; p < P;
       p += (int64_t)gridDim.x * kMtThreads) {
    const int64_t r = rows[p];
    if ((uint64_t)r < (uint64_t)m)
      mt_global_add(count + r, 1);
    else
      ++np;
  }
  mt_flush_pad(np, npad);
}

// -------------------------------------------------------------------- row pass ----

// V consecutive elements of a table row as fp32: 16 bytes of fp32 or bf16 (Pk's loads), or
// 8 bytes of a bf16 row where the other table is fp32 and maps the lanes
template <int V, typename T>
struct MtRow;
template <>
struct MtRow<4, float> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const Pk<float> x = pk_load(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = x.v[i];
  }
};
template <>
struct MtRow<8, bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const Pk<bf16_t> x = pk_load(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x.v[i];
  }
};
template <>
struct MtRow<4, bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const uint2 x = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(x.x << 16);
    v[1] = __uint_as_float(x.x & 0xffff0000u);
    v[2] = __uint_as_float(x.y << 16);
    v[3] = __uint_as_float(x.y & 0xffff0000u);
  }
};

// elements per lane: 16 bytes of the wider element type
template <typename TH, typename TT>
struct MtGeo {
  static constexpr int V = 16 / (int)(sizeof(TH) > sizeof(TT) ? sizeof(TH) : sizeof(TT));
};

struct MtArgs {
  int64_t n, n_t, ld, t_ld;
  int F;
  int64_t P;
  int64_t ident;           // count == nullptr: rows [0, ident) occur once (rows == NULL)
  const int32_t* count;    // (n,) or nullptr
  const int32_t* npad;     // device padding count, nullptr with ident
  float* coef;             // (n, 2)
  float* cos_rows;         // (n,) or nullptr
  int32_t* count_out;      // (n,) or nullptr: the identity counts written out
  double* part;            // one per block
};

// Block b owns table rows [b kMtRowTile, (b + 1) kMtRowTile).  QP = F / V lanes a row,
// 64 / QP rows per wave-instruction; the three dot products of a row in fp32 lanes and an
// xor tree over its QP lanes, the per-row scalars in fp64 on lane q == 0.
template <typename TH, typename TT>
__global__ void __launch_bounds__(kMtThreads) mt_rows_kernel(MtArgs a, const TH* __restrict__ h,
                                                            const TT* __restrict__ T) {
  __shared__ double term[kMtRowTile];
  __shared__ double wsum[kMtWaves];
  constexpr int V = MtGeo<TH, TT>::V;
  constexpr int UNROLL = 4;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int QP = a.F / V, RPW = kWave / QP;
  const int slot = lane / QP, q = lane % QP;
  const int64_t base = (int64_t)blockIdx.x * kMtRowTile;
  const int n_rows = (int)min((int64_t)kMtRowTile, a.n - base);
  const int64_t m = a.n < a.n_t ? a.n : a.n_t;
  const int64_t pv = a.npad != nullptr ? a.P - (int64_t)a.npad[0] : a.ident;
  const double inv_pv = pv > 0 ? 1.0 / (double)pv : 0.0;
  for (int i0 = wv * RPW * UNROLL; i0 < n_rows; i0 += kMtWaves * RPW * UNROLL) {
    float dot[UNROLL], ss[UNROLL], tt[UNROLL];
    int c[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int i = i0 + u * RPW + slot;
      dot[u] = ss[u] = tt[u] = 0.f;
      c[u] = 0;
      if (i < n_rows) {
        const int64_t r = base + i;
        int cr = a.count != nullptr ? a.count[r] : (r < a.ident ? 1 : 0);
        if (r >= m || cr < 0) cr = 0;  // (a row outside the teacher occurs in no valid entry)
        c[u] = cr;
        if (cr > 0) {
          float hv[V], tv[V];
          MtRow<V, TH>::load(h + r * a.ld + V * q, hv);
          MtRow<V, TT>::load(T + r * a.t_ld + V * q, tv);
          float d = hv[V - 1] * tv[V - 1], s = hv[V - 1] * hv[V - 1], w = tv[V - 1] * tv[V - 1];
#pragma unroll
          for (int k = V - 2; k >= 0; --k) {
            d = fmaf(hv[k], tv[k], d);
            s = fmaf(hv[k], hv[k], s);
            w = fmaf(tv[k], tv[k], w);
          }
          dot[u] = d;
          ss[u] = s;
          tt[u] = w;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float d = dot[u], s = ss[u], w = tt[u];
      for (int o = 1; o < QP; o <<= 1) {
        d += __shfl_xor(d, o);
        s += __shfl_xor(s, o);
        w += __shfl_xor(w, o);
      }
      const int i = i0 + u * RPW + slot;
      if (q == 0 && i < n_rows) {
        const int64_t r = base + i;
        float c0 = 0.f, c1 = 0.f, cs = __builtin_nanf("");
        double tr = 0.0;
        if (c[u] > 0) {
          const double raw = sqrt((double)s);  // the unclamped student norm
          const double ns = fmax(raw, kMtEps), nt = fmax(sqrt((double)w), kMtEps);
          const double cosv = (double)d / (ns * nt);
          const double cw = (double)c[u] * inv_pv;
          c0 = (float)(cw / (ns * nt));
          c1 = raw > 0.0 ? (float)(cw * cosv / (ns * raw)) : 0.f;
          cs = (float)cosv;
          tr = (double)c[u] * cosv;
        }
        *reinterpret_cast<float2*>(a.coef + 2 * r) = make_float2(c0, c1);
        if (a.cos_rows != nullptr) a.cos_rows[r] = cs;
        if (a.count_out != nullptr) a.count_out[r] = c[u];
        term[i] = tr;
      }
    }
  }
  __syncthreads();
  // the tile's sum with every lane busy: thread t takes rows t, t + 256, ... in order
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_rows; i += kMtThreads) acc += term[i];
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) wsum[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < kMtWaves; ++k) s += wsum[k];
    a.part[blockIdx.x] = s;
  }
}

// the blocks' partials in a fixed order: thread t strides them, xor tree, waves ascending
__global__ void __launch_bounds__(kMtFinThreads) mt_final_kernel(
    int64_t nb, const double* __restrict__ part, int64_t P, int64_t ident,
    float* __restrict__ loss, int32_t* __restrict__ npad, bool ident_mode) {
  __shared__ double ws[kMtFinThreads / kWave];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kMtFinThreads) s += part[b];
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) s += __shfl_xor(s, o);
  if (lane == 0) ws[wv] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < kMtFinThreads / kWave; ++i) t += ws[i];
    if (ident_mode) npad[0] = (int32_t)(P - ident);
    const int64_t pv = ident_mode ? ident : P - (int64_t)npad[0];
    loss[0] = pv > 0 ? (float)(1.0 - t / (double)pv) : 0.f;
  }
}

// -------------------------------------------------------------------- backward ----

// dH[r] = -gloss (coef[r, 0] T[r] - coef[r, 1] h[r]); a row whose coefficients are both zero
// (absent, or outside the teacher) is written as zeros and reads neither table.  R (pair_grad.h):
// every table row to dH[r] (PgAllRows), or entry i of the list of the rows that occur
// (msha_link_match_rows) to vals[i] (PgListRows; zeros past the device count).
template <typename TH, typename TT, typename R>
__global__ void __launch_bounds__(kMtThreads) mt_bwd_kernel(
    int64_t n, int64_t n_t, int F, const TH* __restrict__ h, int64_t ld, const TT* __restrict__ T,
    int64_t t_ld, const float* __restrict__ coef, const float* __restrict__ gloss,
    float* __restrict__ dH, R rows) {
  constexpr int V = MtGeo<TH, TT>::V;
  constexpr int UNROLL = 4;
  const int lane = lane_id();
  const int QP = F / V, RPW = kWave / QP;
  const int slot = lane / QP, q = lane % QP;
  const float gl = -gloss[0];
  const int64_t m = n < n_t ? n : n_t;
  const int64_t wave = ((int64_t)blockIdx.x * kMtThreads + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * kMtThreads) >> 6;
  const int64_t cnt = rows.count(n), ext = rows.extent(n);
  for (int64_t i0 = wave * RPW * UNROLL; i0 < ext; i0 += nwaves * RPW * UNROLL) {
    float hv[UNROLL][V], tv[UNROLL][V];
    float2 cf[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t i = i0 + u * RPW + slot;
      const int64_t r = i < ext ? rows.row(i, cnt) : -1;
      cf[u] = make_float2(0.f, 0.f);
      if ((uint64_t)r < (uint64_t)m) cf[u] = *reinterpret_cast<const float2*>(coef + 2 * r);
      const bool on = cf[u].x != 0.f || cf[u].y != 0.f;
      if (on) {
        MtRow<V, TH>::load(h + r * ld + V * q, hv[u]);
        MtRow<V, TT>::load(T + r * t_ld + V * q, tv[u]);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) hv[u][k] = tv[u][k] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t i = i0 + u * RPW + slot;
      if (i >= ext) continue;
      const bool on = cf[u].x != 0.f || cf[u].y != 0.f;
      float* out = dH + i * F + V * q;
#pragma unroll
      for (int k = 0; k < V; k += 4) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) {
          o.x = gl * fmaf(cf[u].x, tv[u][k], -(cf[u].y * hv[u][k]));
          o.y = gl * fmaf(cf[u].x, tv[u][k + 1], -(cf[u].y * hv[u][k + 1]));
          o.z = gl * fmaf(cf[u].x, tv[u][k + 2], -(cf[u].y * hv[u][k + 2]));
          o.w = gl * fmaf(cf[u].x, tv[u][k + 3], -(cf[u].y * hv[u][k + 3]));
        }
        *reinterpret_cast<float4*>(out + k) = o;
      }
    }
  }
}

// ------------------------------------------------------------------------ host ----

constexpr int64_t kMtMaxEntries = ((int64_t)1 << 31) - 1;  // P < 2^31
constexpr int64_t kMtMaxRows = ((int64_t)1 << 31) - 1;     // row ids are int32 table keys

static int64_t mt_row_blocks(int64_t n) { return (n + kMtRowTile - 1) / kMtRowTile; }

struct MtLayout {
  size_t count, part, total;
};

static MtLayout mt_layout(int64_t n) {
  MtLayout L;
  L.count = 0;
  L.part = pg_align((size_t)n * 4);
  L.total = L.part + pg_align((size_t)mt_row_blocks(n) * 8);
  return L;
}

// the table checks shared by the forward and the backward: pg_table_check on each table
// (the student's carries the entry-count message), then the pair's own rules
static int mt_tables_check(const char* name, int32_t feat, int32_t h_dtype, const void* h,
                           int64_t ld, int64_t n, int32_t t_dtype, const void* T, int64_t t_ld,
                           int64_t n_t) {
  int rc = pg_table_check(name, 1, feat, h_dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  rc = pg_table_check(name, 1, feat, t_dtype, T, t_ld, n_t);
  if (rc != MSHA_OK) return rc;
  if (n > kMtMaxRows || n_t > kMtMaxRows)
    return fail(MSHA_ERR_ARG, std::string(name) + ": n and n_t must be below 2^31");
  return MSHA_OK;
}

template <typename TH, typename TT>
static void mt_rows_launch(const MtArgs& a, const void* h, const void* T, int64_t nb,
                           hipStream_t s) {
  hipLaunchKernelGGL((mt_rows_kernel<TH, TT>), dim3((unsigned)nb), dim3(kMtThreads), 0, s, a,
                     (const TH*)h, (const TT*)T);
}

template <typename TH, typename TT, typename R>
static void mt_bwd_launch(int64_t n, int64_t n_t, int F, const void* h, int64_t ld, const void* T,
                          int64_t t_ld, const float* coef, const float* gloss, float* dH,
                          hipStream_t s, R rows) {
  constexpr int V = MtGeo<TH, TT>::V;
  const int rows_per_block = kMtWaves * (kWave / (F / V)) * 4;
  hipLaunchKernelGGL((mt_bwd_kernel<TH, TT, R>),
                     dim3(grid_for(rows.grid_rows(n), rows_per_block, 1 << 16)), dim3(kMtThreads),
                     0, s, n, n_t, F, (const TH*)h, ld, (const TT*)T, t_ld, coef, gloss, dH, rows);
}

// the rows that occur: count[r] > 0 (the forward's histogram, or its identity counts)
struct MtCountFlag {
  const int32_t* count;
  __device__ __forceinline__ int operator()(int64_t r) const { return count[r] > 0 ? 1 : 0; }
};

// FN<student type, teacher type>(...) for the four dtype pairs
#define MT_DISPATCH(FN, HD, TD, ...)                           \
  do {                                                         \
    if ((HD) == MSHA_DTYPE_BF16 && (TD) == MSHA_DTYPE_BF16)    \
      FN<bf16_t, bf16_t>(__VA_ARGS__);                         \
    else if ((HD) == MSHA_DTYPE_BF16)                          \
      FN<bf16_t, float>(__VA_ARGS__);                          \
    else if ((TD) == MSHA_DTYPE_BF16)                          \
      FN<float, bf16_t>(__VA_ARGS__);                          \
    else                                                       \
      FN<float, float>(__VA_ARGS__);                           \
  } while (0)

// zero, then the histogram in the form chosen at compile time
static void mt_count_launch(int64_t P, int64_t n, int64_t m, const int64_t* rows, int32_t* cnt,
                            int32_t* n_pad, hipStream_t s) {
  hipLaunchKernelGGL(mt_zero_kernel, dim3(grid_for(n, kMtThreads, 1 << 14)), dim3(kMtThreads), 0,
                     s, n, cnt, n_pad);
#if MATCH_HIST_LDS
  const int64_t ntiles = (P + kMtHistTile - 1) / kMtHistTile;
  hipLaunchKernelGGL(mt_hist_lds_kernel, dim3(grid_for(ntiles, 1, 1 << 14)), dim3(kMtThreads), 0,
                     s, P, m, rows, cnt, n_pad);
#else
  hipLaunchKernelGGL(mt_hist_direct_kernel, dim3(grid_for(P, kMtThreads, 1 << 14)),
                     dim3(kMtThreads), 0, s, P, m, rows, cnt, n_pad);
#endif
}

}  // namespace msha

using namespace msha;

extern "C" size_t msha_link_match_fwd_workspace_size(int64_t n_entries, int64_t n) {
  if (n_entries < 1 || n_entries > kMtMaxEntries || n < 1 || n > kMtMaxRows) return 0;
  return mt_layout(n).total;
}

extern "C" int msha_link_match_count(int64_t n_entries, int64_t n, int64_t n_valid,
                                     const int64_t* rows, int32_t* count, int32_t* n_pad,
                                     msha_stream_t stream) {
  MSHA_ARG_CHECK(n_entries >= 1 && n_entries <= kMtMaxEntries,
                 "link_match_count: bad sizes (1 <= n_entries < 2^31)");
  MSHA_ARG_CHECK(n >= 1 && n <= kMtMaxRows && n_valid >= 0 && n_valid <= n,
                 "link_match_count: bad sizes (1 <= n < 2^31, 0 <= n_valid <= n)");
  MSHA_ARG_CHECK(rows && count && n_pad, "link_match_count: null pointer");
  mt_count_launch(n_entries, n, n_valid, rows, count, n_pad, (hipStream_t)stream);
  return check_launch("link_match_count");
}

extern "C" int msha_link_match_fwd(int64_t n_entries, int32_t feat, int32_t h_dtype,
                                   const void* h, int64_t ld, int64_t n, int32_t t_dtype,
                                   const void* teacher, int64_t t_ld, int64_t n_t,
                                   const int64_t* rows, float* coef, float* cos_rows,
                                   int32_t* count, float* loss, int32_t* n_pad, void* ws,
                                   size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(n_entries >= 1 && n_entries <= kMtMaxEntries,
                 "link_match_fwd: bad sizes (1 <= n_entries < 2^31)");
  const int rc = mt_tables_check("link_match_fwd", feat, h_dtype, h, ld, n, t_dtype, teacher,
                                 t_ld, n_t);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(coef && loss && n_pad, "link_match_fwd: null pointer");
  MSHA_ARG_CHECK(((uintptr_t)coef % 8) == 0, "link_match_fwd: coef must be 8-byte aligned");
  const MtLayout L = mt_layout(n);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= L.total && ((uintptr_t)ws % 16) == 0,
                 "link_match_fwd: workspace too small or unaligned "
                 "(msha_link_match_fwd_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t m = n < n_t ? n : n_t;
  const bool ident = rows == nullptr;
  int32_t* cnt = count != nullptr ? count : (int32_t*)((char*)ws + L.count);
  double* part = (double*)((char*)ws + L.part);
  if (!ident) mt_count_launch(n_entries, n, m, rows, cnt, n_pad, s);
  const int64_t nb = mt_row_blocks(n);
  MtArgs a;
  a.n = n; a.n_t = n_t; a.ld = ld; a.t_ld = t_ld;
  a.F = (int)feat;
  a.P = n_entries;
  a.ident = ident ? (n_entries < m ? n_entries : m) : 0;
  a.count = ident ? nullptr : cnt;
  a.npad = ident ? nullptr : n_pad;
  a.coef = coef;
  a.cos_rows = cos_rows;
  a.count_out = ident ? count : nullptr;
  a.part = part;
  MT_DISPATCH(mt_rows_launch, h_dtype, t_dtype, a, h, teacher, nb, s);
  hipLaunchKernelGGL(mt_final_kernel, dim3(1), dim3(kMtFinThreads), 0, s, nb, part, n_entries,
                     a.ident, loss, n_pad, ident);
  return check_launch("link_match_fwd");
}

extern "C" int msha_link_match_bwd(int32_t feat, int32_t h_dtype, const void* h, int64_t ld,
                                   int64_t n, int32_t t_dtype, const void* teacher, int64_t t_ld,
                                   int64_t n_t, const float* coef, const float* gloss, float* dH,
                                   msha_stream_t stream) {
  const int rc = mt_tables_check("link_match_bwd", feat, h_dtype, h, ld, n, t_dtype, teacher,
                                 t_ld, n_t);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(coef && gloss && dH, "link_match_bwd: null pointer");
  MSHA_ARG_CHECK(((uintptr_t)coef % 8) == 0, "link_match_bwd: coef must be 8-byte aligned");
  MSHA_ARG_CHECK(((uintptr_t)dH % 16) == 0, "link_match_bwd: dH must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  MT_DISPATCH(mt_bwd_launch, h_dtype, t_dtype, n, n_t, (int)feat, h, ld, teacher, t_ld, coef,
              gloss, dH, s, PgAllRows{});
  return check_launch("link_match_bwd");
}

extern "C" int msha_link_match_rows(int64_t n_entries, int64_t n, const int32_t* count,
                                    int32_t* rows, int32_t* n_rows, void* ws, size_t ws_bytes,
                                    msha_stream_t stream) {
  MSHA_ARG_CHECK(n_entries >= 1 && n_entries <= kMtMaxEntries,
                 "link_match_rows: bad sizes (1 <= n_entries < 2^31)");
  MSHA_ARG_CHECK(n >= 1 && n < kMtMaxRows, "link_match_rows: bad sizes (1 <= n < 2^31 - 1)");
  MSHA_ARG_CHECK(count && rows && n_rows, "link_match_rows: null pointer");
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= rl_layout(n).total && ((uintptr_t)ws % 16) == 0,
                 "link_match_rows: workspace too small or unaligned "
                 "(msha_plan_rows_workspace_size)");
  const int64_t cap = n < n_entries ? n : n_entries;
  rl_build(n, cap, MtCountFlag{count}, rows, n_rows, ws, (hipStream_t)stream);
  return check_launch("link_match_rows");
}

extern "C" int msha_link_match_bwd_rows(int64_t n_entries, int32_t feat, int32_t h_dtype,
                                        const void* h, int64_t ld, int64_t n, int32_t t_dtype,
                                        const void* teacher, int64_t t_ld, int64_t n_t,
                                        const float* coef, const float* gloss,
                                        const int32_t* rows, const int32_t* n_rows, int64_t cap,
                                        float* vals, msha_stream_t stream) {
  MSHA_ARG_CHECK(n_entries >= 1 && n_entries <= kMtMaxEntries,
                 "link_match_bwd_rows: bad sizes (1 <= n_entries < 2^31)");
  const int rc = mt_tables_check("link_match_bwd_rows", feat, h_dtype, h, ld, n, t_dtype, teacher,
                                 t_ld, n_t);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(coef && gloss && rows && n_rows && vals, "link_match_bwd_rows: null pointer");
  MSHA_ARG_CHECK(cap == (n < n_entries ? n : n_entries),
                 "link_match_bwd_rows: cap must be min(n, n_entries) (msha_link_match_rows)");
  MSHA_ARG_CHECK(((uintptr_t)coef % 8) == 0, "link_match_bwd_rows: coef must be 8-byte aligned");
  MSHA_ARG_CHECK(((uintptr_t)vals % 16) == 0, "link_match_bwd_rows: vals must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  MT_DISPATCH(mt_bwd_launch, h_dtype, t_dtype, n, n_t, (int)feat, h, ld, teacher, t_ld, coef,
              gloss, vals, s, PgListRows{rows, n_rows, cap});
  return check_launch("link_match_bwd_rows");
}
