// The table gradient of a pair list under its incidence plan (msha_pair_plan), shared by
// link_bce_bwd (linkloss.hip: g recomputed from the stored logit), pair_grad_bwd (distill.hip:
// g loaded) and link_mlp_bwd (linkmlp.hip: the fp32 row dx[p]):
//
//   dH[r] = sum over row r's endpoints e, in plan order, of factor(p(e)) h[other(e)]
//
// One wave per table row; rows longer than a chunk go through chunk partials added in chunk
// order (the chunk table's layout: linkloss.hip).  No float atomics: the result is a function
// of the plan alone.  One kernel family and one host driver (pg_run) serve every factor:
// G is where a pair's factor comes from, and PgFactor<G> is what the kernels need to know of
// it.  A scalar factor is any G with G::at(p, gloss) -> float; PgDx is the row factor.
#pragma once

#include "common.h"

namespace msha {

constexpr int kPgThreads = 256;
constexpr int kPgWaves = kPgThreads / kWave;
constexpr int kPgChunk = 512;  // endpoints per backward chunk (msha_pair_plan_chunk)

template <typename T, typename G>
struct PgArgs {
  int64_t P, n, ld;
  int F;
  const T* h;
  const int64_t *src, *dst;
  G g;
  const float* gloss;  // null where PgFactor<G>::kGloss is false
  const int32_t *rowptr, *ent, *tab;
  float* part;  // (2 nwin, F) chunk partials
  float* dH;
};

// the Pk<T>::V fp32 elements from p (16 or 32 bytes)
template <typename T>
__device__ __forceinline__ Pk<T> pk_load_f32(const float* p) {
  Pk<T> r;
#pragma unroll
  for (int i = 0; i < Pk<T>::V; i += 4) {
    const float4 x = *reinterpret_cast<const float4*>(p + i);
    r.v[i] = x.x; r.v[i + 1] = x.y; r.v[i + 2] = x.z; r.v[i + 3] = x.w;
  }
  return r;
}

// What pg_sum_range needs of a factor.  The lane that decodes an endpoint keeps a Lane for it
// (none(): a rejected endpoint); the endpoint's lane group receives that Lane by shuffle and
// turns it into its Piece of the factor.  in: the slot lies inside the range.
//
// Scalar factor (any G with at() and ok()): the Lane is g itself, 0 for a rejected endpoint;
// every in-range slot loads its row of h (a rejected one reads row 0 and multiplies by 0).
template <typename G>
struct PgFactor {
  using Lane = float;
  template <typename T>
  using Piece = float;
  static constexpr bool kGloss = true;  // at() takes the loss gradient: gloss[0] is read
  static bool ok(const G& g, const float* gloss) { return g.ok() && gloss != nullptr; }
  static __device__ __forceinline__ Lane none() { return 0.f; }
  static __device__ __forceinline__ Lane lane(const G& g, int64_t p, float gl) {
    return g.at(p, gl);
  }
  static __device__ __forceinline__ bool live(Lane, bool in) { return in; }
  template <typename T>
  static __device__ __forceinline__ float piece(const G&, Lane s, bool in, int, int) {
    return in ? s : 0.f;
  }
};

// Row factor: the fp32 row dx[p] (pitch F), which already carries the loss gradient, so gloss
// is null and never read.  The Lane is the pair index, -1 for a rejected endpoint, whose group
// loads neither dx nor h; the group's lanes load their 16 or 32 bytes of dx[p] themselves.
struct PgDx {
  const float* dx;  // (P, F)
};
template <>
struct PgFactor<PgDx> {
  using Lane = int64_t;
  template <typename T>
  using Piece = Pk<T>;
  static constexpr bool kGloss = false;
  static bool ok(const PgDx& g, const float*) { return g.dx != nullptr; }
  static __device__ __forceinline__ Lane none() { return -1; }
  static __device__ __forceinline__ Lane lane(const PgDx&, int64_t p, float) { return p; }
  static __device__ __forceinline__ bool live(Lane s, bool in) { return in && s >= 0; }
  template <typename T>
  static __device__ __forceinline__ Pk<T> piece(const PgDx& g, Lane s, bool in, int F, int q) {
    return live(s, in) ? pk_load_f32<T>(g.dx + s * F + Pk<T>::V * q) : pk_zero<T>();
  }
};

// acc += factor piece * row piece: a scalar against the row, or element by element
template <typename T>
__device__ __forceinline__ Pk<T> pg_fma(float f, const Pk<T>& row, Pk<T> acc) {
  return pk_fma(f, row, acc);
}
template <typename T>
__device__ __forceinline__ Pk<T> pg_fma(const Pk<T>& f, const Pk<T>& row, Pk<T> acc) {
#pragma unroll
  for (int i = 0; i < Pk<T>::V; ++i) acc.v[i] = fmaf(f.v[i], row.v[i], acc.v[i]);
  return acc;
}

// Which rows a launch sums and where row i of its loop is written: every table row, row r
// to dH[r] (PgAllRows), or the touched-row list of the plan (msha_plan_rows), row rows[i] to
// vals[i] (PgListRows; the loop runs to the list's capacity, and an entry past the device
// count, or one outside the table, is an empty row: zeros).  The sums themselves are shared.
struct PgAllRows {
  static constexpr const char* kOut = "dH";
  __device__ __forceinline__ int64_t extent(int64_t n) const { return n; }
  __device__ __forceinline__ int64_t count(int64_t n) const { return n; }
  __device__ __forceinline__ int64_t row(int64_t i, int64_t) const { return i; }
  int64_t grid_rows(int64_t n) const { return n; }
};
struct PgListRows {
  static constexpr const char* kOut = "vals";
  const int32_t *rows, *n_rows;
  int64_t cap;
  __device__ __forceinline__ int64_t extent(int64_t) const { return cap; }
  __device__ __forceinline__ int64_t count(int64_t) const {
    const int64_t c = n_rows[0];
    return c < 0 ? 0 : c > cap ? cap : c;
  }
  __device__ __forceinline__ int64_t row(int64_t i, int64_t cnt) const {
    return i < cnt ? (int64_t)rows[i] : -1;
  }
  int64_t grid_rows(int64_t) const { return cap; }
};

// sum over the endpoints ent[beg, end) of factor h[other], one wave: 64 endpoints are decoded
// a lane each, then their rows are gathered 64 / QP at a time (QP lanes x 16 bytes a row); the
// loads of UNROLL endpoints are issued before the first fma.  Endpoint i of the range goes to
// lane group i % (64 / QP); the groups are added by an xor tree at the end: the order is a
// function of the range and F alone.  All lanes of a column hold the sum on return.
template <typename T, typename G>
__device__ __forceinline__ Pk<T> pg_sum_range(const PgArgs<T, G>& a, int beg, int end) {
  using Fa = PgFactor<G>;
  constexpr int V = Pk<T>::V;
  constexpr int UNROLL = 4;
  const int lane = lane_id();
  const int QP = a.F / V, EPW = kWave / QP;
  const int slot = lane / QP, q = lane % QP;
  float gl = 0.f;
  if constexpr (Fa::kGloss) gl = a.gloss[0];
  Pk<T> acc = pk_zero<T>();
  for (int base = beg; base < end; base += kWave) {
    const int pos = base + lane;
    typename Fa::Lane g = Fa::none();
    int64_t other = 0;
    if (pos < end) {
      const int64_t e = a.ent[pos];
      if ((uint64_t)e < (uint64_t)(2 * a.P)) {
        const int64_t p = e < a.P ? e : e - a.P;
        const int64_t o = e < a.P ? a.dst[p] : a.src[p];
        if ((uint64_t)o < (uint64_t)a.n) {  // (a plan of another pair list: no stray read)
          other = o;
          g = Fa::lane(a.g, p, gl);
        }
      }
    }
    const int cnt = min(kWave, end - base);
    for (int j0 = 0; j0 < cnt; j0 += EPW * UNROLL) {
      typename Fa::template Piece<T> fac[UNROLL];
      Pk<T> row[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int j = j0 + u * EPW + slot;
        const typename Fa::Lane gv = __shfl(g, j & (kWave - 1));
        const int64_t ov = __shfl(other, j & (kWave - 1));
        fac[u] = Fa::template piece<T>(a.g, gv, j < cnt, a.F, q);
        row[u] = Fa::live(gv, j < cnt) ? pk_load(a.h + ov * a.ld + V * q) : pk_zero<T>();
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) acc = pg_fma(fac[u], row[u], acc);
    }
  }
  for (int o = QP; o < kWave; o <<= 1) acc = pk_xor_add(acc, o);
  return acc;
}

template <typename T>
__device__ __forceinline__ void pg_store(float* out, const Pk<T>& acc, int q) {
  constexpr int V = Pk<T>::V;
#pragma unroll
  for (int i = 0; i < V; i += 4)
    *reinterpret_cast<float4*>(out + V * q + i) =
        make_float4(acc.v[i], acc.v[i + 1], acc.v[i + 2], acc.v[i + 3]);
}

// one wave per table row: its first min(deg, C) endpoints; a row of at most C endpoints is
// complete (zeros for none), a longer one leaves its first chunk's partial
template <typename T, typename G, typename R>
__global__ void __launch_bounds__(kPgThreads) pg_rows_kernel(PgArgs<T, G> a, R rows) {
  constexpr int V = Pk<T>::V;
  const int lane = lane_id();
  const int QP = a.F / V;
  const int64_t wave = ((int64_t)blockIdx.x * kPgThreads + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * kPgThreads) >> 6;
  const int64_t cnt = rows.count(a.n), ext = rows.extent(a.n);
  for (int64_t i = wave; i < ext; i += nwaves) {
    const int64_t r = rows.row(i, cnt);
    int b = 0, e = 0;
    if ((uint64_t)r < (uint64_t)a.n) b = a.rowptr[r], e = a.rowptr[r + 1];
    if (b < 0 || e < b || (int64_t)e > 2 * a.P) b = e = 0;  // (not a plan of this list)
    const bool lng = e - b > kPgChunk;
    const Pk<T> acc = pg_sum_range(a, b, lng ? b + kPgChunk : e);
    float* out = lng ? a.part + (int64_t)(2 * (b / kPgChunk) + 1) * a.F : a.dH + i * a.F;
    if (lane < QP) pg_store(out, acc, lane);
  }
}

// one wave per window: the chunk of a long row that starts in it (not the row's first)
template <typename T, typename G>
__global__ void __launch_bounds__(kPgThreads) pg_chunks_kernel(PgArgs<T, G> a, int64_t nwin) {
  constexpr int V = Pk<T>::V;
  const int lane = lane_id();
  const int QP = a.F / V;
  const int64_t wave = ((int64_t)blockIdx.x * kPgThreads + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * kPgThreads) >> 6;
  for (int64_t m = wave; m < nwin; m += nwaves) {
    const int64_t r = a.tab[2 * m];
    const int b = a.tab[2 * m + 1];
    if ((uint64_t)r >= (uint64_t)a.n || b < 0 || b / kPgChunk != m) continue;
    const int e = min(b + kPgChunk, a.rowptr[r + 1]);
    if ((int64_t)e > 2 * a.P) continue;  // (not a plan of this list)
    const Pk<T> acc = pg_sum_range(a, b, e);
    if (lane < QP) pg_store(a.part + 2 * m * a.F, acc, lane);
  }
}

// long rows: the chunk partials added in chunk order (one wave per row, a float4 per lane)
template <typename R>
static __global__ void __launch_bounds__(kPgThreads) pg_finish_kernel(
    int64_t P, int64_t n, int F, const int32_t* __restrict__ rowptr,
    const float* __restrict__ part, float* __restrict__ dH, R rows) {
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * kPgThreads + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * kPgThreads) >> 6;
  const int64_t cnt = rows.count(n);
  for (int64_t i = wave; i < cnt; i += nwaves) {
    const int64_t r = rows.row(i, cnt);
    if ((uint64_t)r >= (uint64_t)n) continue;
    const int b = rowptr[r], e = rowptr[r + 1];
    if (b < 0 || (int64_t)e > 2 * P || e - b <= kPgChunk) continue;
    for (int f = 4 * lane; f < F; f += 4 * kWave) {
      float4 s = *reinterpret_cast<const float4*>(part + (int64_t)(2 * (b / kPgChunk) + 1) * F + f);
#pragma unroll 8  // the loads of 8 partials in flight; the adds stay in chunk order
      for (int64_t qp = (int64_t)b + kPgChunk; qp < e; qp += kPgChunk) {
        const float4 v = *reinterpret_cast<const float4*>(part + 2 * (qp / kPgChunk) * F + f);
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
      }
      *reinterpret_cast<float4*>(dH + i * F + f) = s;
    }
  }
}

static inline size_t pg_align(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int64_t pg_windows(int64_t P) {
  return P > 0 ? (2 * P + kPgChunk - 1) / kPgChunk : 1;
}
constexpr int64_t kPgMaxPairs = ((int64_t)1 << 30) - 1;  // 2P < 2^31

// feat a power of two spanning 16 bytes to 64 lanes x 16 bytes of an fp32 or bf16 row
static inline bool pg_width_ok(int32_t feat, int32_t dtype) {
  if (dtype != MSHA_DTYPE_F32 && dtype != MSHA_DTYPE_BF16) return false;
  const int v = dtype == MSHA_DTYPE_BF16 ? 8 : 4;
  return feat >= v && feat <= 64 * v && (feat & (feat - 1)) == 0;
}

static inline int pg_table_check(const char* name, int64_t n_pairs, int32_t feat, int32_t dtype,
                                 const void* h, int64_t ld, int64_t n) {
  const std::string nm(name);
  if (n_pairs < 1 || n < 1) return fail(MSHA_ERR_ARG, nm + ": bad sizes (n_pairs >= 1, n >= 1)");
  if (n_pairs > kPgMaxPairs) return fail(MSHA_ERR_ARG, nm + ": 2 * n_pairs must be below 2^31");
  if (!pg_width_ok(feat, dtype))
    return fail(MSHA_ERR_ARG, nm + ": unsupported width: feat must be a power of two in [16 B, "
                                   "64 lanes x 16 B] of an fp32 or bf16 table "
                                   "(msha_link_bce_supported)");
  const int v = dtype == MSHA_DTYPE_BF16 ? 8 : 4;
  if (h == nullptr) return fail(MSHA_ERR_ARG, nm + ": null pointer");
  if (ld < feat || ld % v != 0 || ((uintptr_t)h % 16) != 0)
    return fail(MSHA_ERR_ARG, nm + ": the table must be 16-byte aligned with a 16-byte row pitch");
  return MSHA_OK;
}

// a.dH: (n, F) with PgAllRows, the (cap, F) vals of the list with PgListRows
template <typename T, typename G, typename R = PgAllRows>
static void pg_launch(const PgArgs<T, G>& a, int64_t nwin, hipStream_t s, R rows = R{}) {
  const int64_t ext = rows.grid_rows(a.n);
  hipLaunchKernelGGL((pg_rows_kernel<T, G, R>), dim3(grid_for(ext, kPgWaves, 1 << 20)),
                     dim3(kPgThreads), 0, s, a, rows);
  hipLaunchKernelGGL((pg_chunks_kernel<T, G>), dim3(grid_for(nwin, kPgWaves, 1 << 20)),
                     dim3(kPgThreads), 0, s, a, nwin);
  hipLaunchKernelGGL((pg_finish_kernel<R>), dim3(grid_for(ext, kPgWaves, 1 << 16)),
                     dim3(kPgThreads), 0, s, a.P, a.n, a.F, a.rowptr, a.part, a.dH, rows);
}

// the list's capacity (msha_plan_rows): no plan names more rows than it has endpoints
static inline int64_t pg_rows_cap(int64_t n, int64_t P) { return n < 2 * P ? n : 2 * P; }

// the chunk partials of a launch: (2 nwin, feat) fp32
static inline size_t pg_workspace_bytes(int64_t P, int32_t feat) {
  return pg_align((size_t)2 * pg_windows(P) * feat * 4);
}

// The host driver of every entry point, after its pg_table_check: the dense gradient (R =
// PgAllRows, out = dH) and the touched-row one (R = PgListRows, out = vals) of factor g.  One
// argument check, one launch sequence.  ws_size_name: the entry point's workspace-size
// function, for the message.
template <typename G, typename R>
static int pg_run(const char* name, const char* ws_size_name, int64_t n_pairs, int32_t feat,
                  int32_t dtype, const void* h, int64_t ld, int64_t n, const int64_t* src,
                  const int64_t* dst, const int32_t* plan_rowptr, const int32_t* plan_ent,
                  const int32_t* plan_chunk_tab, const G& g, const float* gloss, float* out,
                  void* ws, size_t ws_bytes, msha_stream_t stream, R rows) {
  const std::string nm(name);
  MSHA_ARG_CHECK(src && dst && PgFactor<G>::ok(g, gloss) && plan_rowptr && plan_ent &&
                     plan_chunk_tab && out,
                 nm + ": null pointer");
  MSHA_ARG_CHECK(((uintptr_t)out % 16) == 0,
                 nm + ": " + R::kOut + " must be 16-byte aligned");
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= pg_workspace_bytes(n_pairs, feat) &&
                     ((uintptr_t)ws % 16) == 0,
                 nm + ": workspace too small or unaligned (" + ws_size_name + ")");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nwin = pg_windows(n_pairs);
  if (dtype == MSHA_DTYPE_BF16) {
    const PgArgs<bf16_t, G> a = {n_pairs, n, ld, (int)feat, (const bf16_t*)h, src, dst, g, gloss,
                                 plan_rowptr, plan_ent, plan_chunk_tab, (float*)ws, out};
    pg_launch(a, nwin, s, rows);
  } else {
    const PgArgs<float, G> a = {n_pairs, n, ld, (int)feat, (const float*)h, src, dst, g, gloss,
                                plan_rowptr, plan_ent, plan_chunk_tab, (float*)ws, out};
    pg_launch(a, nwin, s, rows);
  }
  return check_launch(name);
}

}  // namespace msha
