// The touched-row list of an incidence plan (include/msha_gnn.h msha_plan_rows): the ascending
// ids of the table rows that have an endpoint, for the row-sparse table gradient
// (msha_link_bce_bwd_rows / msha_pair_grad_bwd_rows, pair_grad.h's PgListRows) and the lazy
// Adam over them (msha_adam_rows_step, optim.hip).
//
// flag -> exclusive scan -> compact in row_list.h's three launches: the flags are formed from
// rowptr inside the tile scan and again inside the compaction (never stored).  Integer work
// only, no atomics, nothing read back.  A row whose rowptr pair is not a plan's (negative,
// decreasing, past 2P) is empty, as pg_rows_kernel reads it.
//
// And the sum of several such row gradients of one table over the union of their lists
// (msha_row_grad_union), for a table that several losses share in one step.
#include "row_list.h"

namespace msha {

struct PrFlag {
  const int32_t* rowptr;
  int64_t P;
  __device__ __forceinline__ int operator()(int64_t r) const {
    const int b = rowptr[r], e = rowptr[r + 1];
    return b >= 0 && e > b && (int64_t)e <= 2 * P ? 1 : 0;
  }
};

// ---- the union of up to kRuMax touched-row lists of one table (msha_row_grad_union): the
// lists' rows are marked in an n-int array (plain stores of 1), the marks go through the same
// scan and compaction, and every output row looks itself up in each sorted list.
constexpr int kRuMax = 4;

struct RuLists {
  int k;
  const int32_t* rows[kRuMax];
  const int32_t* n_rows[kRuMax];
  int64_t cap[kRuMax];
  const float* vals[kRuMax];
};

struct RuFlag {
  const int32_t* mark;
  __device__ __forceinline__ int operator()(int64_t r) const { return mark[r] != 0 ? 1 : 0; }
};

__device__ __forceinline__ int64_t ru_count(const int32_t* n_rows, int64_t cap) {
  const int64_t c = n_rows[0];
  return c < 0 ? 0 : c > cap ? cap : c;
}

static __global__ void __launch_bounds__(kRlThreads) ru_zero_kernel(int64_t n,
                                                                    int32_t* __restrict__ mark) {
  for (int64_t r = (int64_t)blockIdx.x * kRlThreads + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * kRlThreads)
    mark[r] = 0;
}

static __global__ void __launch_bounds__(kRlThreads) ru_mark_kernel(int64_t n, RuLists L,
                                                                    int32_t* __restrict__ mark) {
  const int64_t tid = (int64_t)blockIdx.x * kRlThreads + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * kRlThreads;
#pragma unroll
  for (int j = 0; j < kRuMax; ++j) {
    if (j >= L.k) break;
    const int64_t cnt = ru_count(L.n_rows[j], L.cap[j]);
    for (int64_t i = tid; i < cnt; i += nthr) {
      const int64_t r = L.rows[j][i];
      if ((uint64_t)r < (uint64_t)n) mark[r] = 1;
    }
  }
}

// vals[i] = x_1 + .. + x_k left to right, x_j the row's value in list j (binary search over
// the list's ascending ids) or +0.0; a float4 per thread, zeros past the count
static __global__ void __launch_bounds__(kRlThreads) ru_sum_kernel(
    int64_t n, int F, RuLists L, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ n_rows, int64_t cap, float* __restrict__ vals) {
  const int LPR = F / 4;
  const int64_t total = cap * LPR;
  const int64_t cnt = ru_count(n_rows, cap);
  for (int64_t t = (int64_t)blockIdx.x * kRlThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kRlThreads) {
    const int64_t i = t / LPR;
    const int c = 4 * (int)(t % LPR);
    const int64_t r = i < cnt ? (int64_t)rows[i] : -1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((uint64_t)r < (uint64_t)n) {
#pragma unroll
      for (int j = 0; j < kRuMax; ++j) {
        if (j >= L.k) break;
        int64_t lo = 0, hi = ru_count(L.n_rows[j], L.cap[j]);
        while (lo < hi) {  // the first entry >= r
          const int64_t mid = (lo + hi) >> 1;
          if ((int64_t)L.rows[j][mid] < r) lo = mid + 1; else hi = mid;
        }
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lo < ru_count(L.n_rows[j], L.cap[j]) && (int64_t)L.rows[j][lo] == r)
          x = *reinterpret_cast<const float4*>(L.vals[j] + lo * F + c);
        s = j == 0 ? x : make_float4(s.x + x.x, s.y + x.y, s.z + x.z, s.w + x.w);
      }
    }
    *reinterpret_cast<float4*>(vals + i * F + c) = s;
  }
}

static size_t ru_mark_bytes(int64_t n) { return rl_align((size_t)n * 4); }

}  // namespace msha

using namespace msha;

extern "C" size_t msha_plan_rows_workspace_size(int64_t n) {
  if (n < 1 || n >= ((int64_t)1 << 31) - 1) return 0;
  return rl_layout(n).total;
}

extern "C" int msha_plan_rows(int64_t n, int64_t n_pairs, const int32_t* rowptr, int32_t* rows,
                              int32_t* n_rows, void* ws, size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 1 && n_pairs >= 0, "plan_rows: bad sizes (n >= 1, n_pairs >= 0)");
  MSHA_ARG_CHECK(n_pairs < ((int64_t)1 << 30), "plan_rows: 2 * n_pairs must be below 2^31");
  MSHA_ARG_CHECK(n < ((int64_t)1 << 31) - 1, "plan_rows: n must be below 2^31 - 1");
  const int64_t cap = n < 2 * n_pairs ? n : 2 * n_pairs;
  MSHA_ARG_CHECK(rowptr && n_rows && (rows || cap == 0), "plan_rows: null pointer");
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= rl_layout(n).total && ((uintptr_t)ws % 16) == 0,
                 "plan_rows: workspace too small or unaligned (msha_plan_rows_workspace_size)");
  rl_build(n, cap, PrFlag{rowptr, n_pairs}, rows, n_rows, ws, (hipStream_t)stream);
  return check_launch("plan_rows");
}

extern "C" size_t msha_row_grad_union_workspace_size(int64_t n) {
  if (n < 1 || n >= ((int64_t)1 << 31) - 1) return 0;
  return ru_mark_bytes(n) + rl_layout(n).total;
}

extern "C" int msha_row_grad_union(int64_t n, int32_t feat, int32_t k, const msha_row_list* lists,
                                   int32_t* rows, int32_t* n_rows, int64_t cap, float* vals,
                                   void* ws, size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 1 && n < ((int64_t)1 << 31) - 1,
                 "row_grad_union: bad sizes (1 <= n < 2^31 - 1)");
  MSHA_ARG_CHECK(k >= 1 && k <= kRuMax, "row_grad_union: k must be in [1, 4]");
  MSHA_ARG_CHECK(feat >= 4 && feat % 4 == 0 && feat <= 65536,
                 "row_grad_union: feat must be a multiple of 4 (16-byte pieces of an fp32 row)");
  MSHA_ARG_CHECK(lists && rows && n_rows && vals, "row_grad_union: null pointer");
  RuLists L{};
  L.k = k;
  int64_t sum = 0;
  for (int j = 0; j < k; ++j) {
    const msha_row_list& l = lists[j];
    MSHA_ARG_CHECK(l.rows && l.n_rows && l.vals, "row_grad_union: null pointer in a list");
    MSHA_ARG_CHECK(l.cap >= 1 && l.cap <= n, "row_grad_union: a list's cap must be in [1, n]");
    MSHA_ARG_CHECK(((uintptr_t)l.vals % 16) == 0,
                   "row_grad_union: every vals must be 16-byte aligned");
    L.rows[j] = l.rows, L.n_rows[j] = l.n_rows, L.cap[j] = l.cap, L.vals[j] = l.vals;
    sum += l.cap;
  }
  MSHA_ARG_CHECK(cap == (n < sum ? n : sum),
                 "row_grad_union: cap must be min(n, the sum of the lists' caps)");
  MSHA_ARG_CHECK(((uintptr_t)vals % 16) == 0, "row_grad_union: vals must be 16-byte aligned");
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= ru_mark_bytes(n) + rl_layout(n).total &&
                     ((uintptr_t)ws % 16) == 0,
                 "row_grad_union: workspace too small or unaligned "
                 "(msha_row_grad_union_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  int32_t* mark = (int32_t*)ws;
  int64_t longest = 0;
  for (int j = 0; j < k; ++j) longest = L.cap[j] > longest ? L.cap[j] : longest;
  hipLaunchKernelGGL(ru_zero_kernel, dim3(grid_for(n, kRlThreads, 1 << 16)), dim3(kRlThreads), 0,
                     s, n, mark);
  hipLaunchKernelGGL(ru_mark_kernel, dim3(grid_for(longest, kRlThreads, 1 << 16)),
                     dim3(kRlThreads), 0, s, n, L, mark);
  rl_build(n, cap, RuFlag{mark}, rows, n_rows, (char*)ws + ru_mark_bytes(n), s);
  hipLaunchKernelGGL(ru_sum_kernel, dim3(grid_for(cap * (feat / 4), kRlThreads, 1 << 16)),
                     dim3(kRlThreads), 0, s, n, (int)feat, L, rows, n_rows, cap, vals);
  return check_launch("row_grad_union");
}
