// The touched-row list of an incidence plan (include/msha_gnn.h msha_plan_rows): the ascending
// ids of the table rows that have an endpoint, for the row-sparse table gradient
// (msha_link_bce_bwd_rows / msha_pair_grad_bwd_rows, pair_grad.h's PgListRows) and the lazy
// Adam over them (msha_adam_rows_step, optim.hip).
//
// flag -> exclusive scan -> compact with int_scan.h's pieces, in three launches: the flags
// are formed from rowptr inside the tile scan and again inside the compaction (never
// stored), and the compaction adds the tile offsets itself.  Integer work only, no atomics,
// nothing read back.  A row whose rowptr pair is not a plan's (negative, decreasing, past 2P)
// is empty, as pg_rows_kernel reads it.
#include "int_scan.h"

namespace msha {

constexpr int kPrThreads = 256;

static inline size_t pr_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct PrLayout {
  size_t off, sums, total;
};
static PrLayout pr_layout(int64_t n) {
  PrLayout L;
  L.off = 0;
  L.sums = L.off + pr_align((size_t)(n + 1) * 4);
  L.total = L.sums + pr_align(scan_ws_ints(n) * 4);
  return L;
}

__device__ __forceinline__ int pr_flag(const int32_t* __restrict__ rowptr, int64_t r, int64_t P) {
  const int b = rowptr[r], e = rowptr[r + 1];
  return b >= 0 && e > b && (int64_t)e <= 2 * P ? 1 : 0;
}

// scan_tiles_kernel over the flags: off[r] = the flagged rows before r in r's tile
static __global__ void __launch_bounds__(kScanThreads) pr_tiles_kernel(
    int64_t n, int64_t P, const int32_t* __restrict__ rowptr, int32_t* __restrict__ off,
    int32_t* __restrict__ tile_sums) {
  __shared__ int sh[kScanThreads / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = base + k < n ? pr_flag(rowptr, base + k, P) : 0;
    s += v[k];
  }
  int total;
  int run = block_exclusive_scan(s, sh, total);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k < n) off[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// rows[sums[tile of r] + off[r]] = r for the flagged rows, -1 from the count to cap, the
// count to n_rows.  A rowptr that is no plan can flag more than cap rows: the list and the
// count stop at cap.  (sums: the tiles' exclusive offsets, off[n]: the total --
// scan_sums_kernel.)
static __global__ void __launch_bounds__(kPrThreads) pr_compact_kernel(
    int64_t n, int64_t P, int64_t cap, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ off, const int32_t* __restrict__ sums,
    int32_t* __restrict__ rows, int32_t* __restrict__ n_rows) {
  const int64_t tid = (int64_t)blockIdx.x * kPrThreads + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * kPrThreads;
  const int64_t total = off[n];
  const int64_t cnt = total < cap ? total : cap;
  for (int64_t r = tid; r < n; r += nthr) {
    if (!pr_flag(rowptr, r, P)) continue;
    const int64_t o = (int64_t)sums[r / kScanTile] + off[r];
    if (o < cap) rows[o] = (int32_t)r;
  }
  for (int64_t i = cnt + tid; i < cap; i += nthr) rows[i] = -1;
  if (tid == 0) n_rows[0] = (int32_t)cnt;
}

}  // namespace msha

using namespace msha;

extern "C" size_t msha_plan_rows_workspace_size(int64_t n) {
  if (n < 1 || n >= ((int64_t)1 << 31) - 1) return 0;
  return pr_layout(n).total;
}

extern "C" int msha_plan_rows(int64_t n, int64_t n_pairs, const int32_t* rowptr, int32_t* rows,
                              int32_t* n_rows, void* ws, size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 1 && n_pairs >= 0, "plan_rows: bad sizes (n >= 1, n_pairs >= 0)");
  MSHA_ARG_CHECK(n_pairs < ((int64_t)1 << 30), "plan_rows: 2 * n_pairs must be below 2^31");
  MSHA_ARG_CHECK(n < ((int64_t)1 << 31) - 1, "plan_rows: n must be below 2^31 - 1");
  const int64_t cap = n < 2 * n_pairs ? n : 2 * n_pairs;
  MSHA_ARG_CHECK(rowptr && n_rows && (rows || cap == 0), "plan_rows: null pointer");
  const PrLayout L = pr_layout(n);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= L.total && ((uintptr_t)ws % 16) == 0,
                 "plan_rows: workspace too small or unaligned (msha_plan_rows_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  int32_t* off = (int32_t*)(w + L.off);
  int32_t* sums = (int32_t*)(w + L.sums);
  const int64_t ntiles = (n + kScanTile - 1) / kScanTile;  // >= 1
  hipLaunchKernelGGL(pr_tiles_kernel, dim3((unsigned)ntiles), dim3(kScanThreads), 0, s, n, n_pairs,
                     rowptr, off, sums);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, s, sums, ntiles, off, n);
  hipLaunchKernelGGL(pr_compact_kernel, dim3(grid_for(n, kPrThreads, 1 << 16)), dim3(kPrThreads),
                     0, s, n, n_pairs, cap, rowptr, off, sums, rows, n_rows);
  return check_launch("plan_rows");
}
