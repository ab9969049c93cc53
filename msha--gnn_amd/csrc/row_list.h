// The ascending list of the flagged rows of a table: flag -> exclusive scan -> compact with
// int_scan.h's pieces, in three launches.  The flag is a functor over the row id (a plan's
// rowptr pair in rowgrad.hip, an occurrence count in match.hip, a marked int in the union of
// several lists): it is evaluated inside the tile scan and again inside the compaction, never
// stored, and the compaction adds the tile offsets itself.  Integer work only, no atomics,
// nothing read back.
#pragma once

#include "int_scan.h"

namespace msha {

constexpr int kRlThreads = 256;

static inline size_t rl_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct RlLayout {
  size_t off, sums, total;
};
static inline RlLayout rl_layout(int64_t n) {
  RlLayout L;
  L.off = 0;
  L.sums = L.off + rl_align((size_t)(n + 1) * 4);
  L.total = L.sums + rl_align(scan_ws_ints(n) * 4);
  return L;
}

// scan_tiles_kernel over the flags: off[r] = the flagged rows before r in r's tile
template <typename Fl>
__global__ void __launch_bounds__(kScanThreads) rl_tiles_kernel(int64_t n, Fl flag,
                                                                int32_t* __restrict__ off,
                                                                int32_t* __restrict__ tile_sums) {
  __shared__ int sh[kScanThreads / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = base + k < n ? flag(base + k) : 0;
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
// count to n_rows.  Flags that name more than cap rows: the list and the count stop at cap.
// (sums: the tiles' exclusive offsets, off[n]: the total -- scan_sums_kernel.)
template <typename Fl>
__global__ void __launch_bounds__(kRlThreads) rl_compact_kernel(
    int64_t n, int64_t cap, Fl flag, const int32_t* __restrict__ off,
    const int32_t* __restrict__ sums, int32_t* __restrict__ rows, int32_t* __restrict__ n_rows) {
  const int64_t tid = (int64_t)blockIdx.x * kRlThreads + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * kRlThreads;
  const int64_t total = off[n];
  const int64_t cnt = total < cap ? total : cap;
  for (int64_t r = tid; r < n; r += nthr) {
    if (!flag(r)) continue;
    const int64_t o = (int64_t)sums[r / kScanTile] + off[r];
    if (o < cap) rows[o] = (int32_t)r;
  }
  for (int64_t i = cnt + tid; i < cap; i += nthr) rows[i] = -1;
  if (tid == 0) n_rows[0] = (int32_t)cnt;
}

// the three launches; ws: rl_layout(n).total bytes, 16-byte aligned; rows may be NULL when
// cap is 0
template <typename Fl>
static void rl_build(int64_t n, int64_t cap, Fl flag, int32_t* rows, int32_t* n_rows, void* ws,
                     hipStream_t s) {
  const RlLayout L = rl_layout(n);
  int32_t* off = (int32_t*)((char*)ws + L.off);
  int32_t* sums = (int32_t*)((char*)ws + L.sums);
  const int64_t ntiles = (n + kScanTile - 1) / kScanTile;  // >= 1
  hipLaunchKernelGGL((rl_tiles_kernel<Fl>), dim3((unsigned)ntiles), dim3(kScanThreads), 0, s, n,
                     flag, off, sums);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, s, sums, ntiles, off, n);
  hipLaunchKernelGGL((rl_compact_kernel<Fl>), dim3(grid_for(n, kRlThreads, 1 << 16)),
                     dim3(kRlThreads), 0, s, n, cap, flag, off, sums, rows, n_rows);
}

}  // namespace msha
