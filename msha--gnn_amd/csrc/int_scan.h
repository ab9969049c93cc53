// Exclusive scan of int32 counts into an (n + 1)-long offset array (graph.hip's CSR / CSC
// pointers, explain.hip's chunk and tie pointers): tiles of kScanTile counts scanned by one
// block each, the tile sums by one block, then added back.  Integer adds only.
#pragma once

#include <algorithm>

#include "common.h"

namespace msha {

constexpr int kScanItems = 4;
constexpr int kScanThreads = 1024;
constexpr int kScanTile = kScanItems * kScanThreads;

__device__ __forceinline__ int block_exclusive_scan(int v, int* sh, int& total) {
  // sh: kScanThreads/64 ints
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  if (w == 0) {
    int s = lane < (kScanThreads / 64) ? sh[lane] : 0;
    int si = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(si, o);
      if (lane >= o) si += t;
    }
    if (lane < (kScanThreads / 64)) sh[lane] = si - s;
    if (lane == (kScanThreads / 64) - 1) sh[kScanThreads / 64] = si;
  }
  __syncthreads();
  const int res = sh[w] + incl - v;
  total = sh[kScanThreads / 64];
  __syncthreads();
  return res;
}

static __global__ void __launch_bounds__(kScanThreads) scan_tiles_kernel(
    const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ out,
    int32_t* __restrict__ tile_sums) {
  __shared__ int sh[kScanThreads / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int v[kScanItems];
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = base + k < n ? in[base + k] : 0;
    s += v[k];
  }
  int total;
  int run = block_exclusive_scan(s, sh, total);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// single block: exclusive scan of the tile sums (any count, chunked with a carry);
// writes the grand total to out[n]
static __global__ void __launch_bounds__(kScanThreads) scan_sums_kernel(
    int32_t* __restrict__ sums, int64_t ntiles, int32_t* __restrict__ out, int64_t n) {
  __shared__ int sh[kScanThreads / 64 + 1];
  int carry = 0;
  for (int64_t c = 0; c < ntiles; c += kScanThreads) {
    const int64_t k = c + threadIdx.x;
    const int v = k < ntiles ? sums[k] : 0;
    int total;
    const int ex = block_exclusive_scan(v, sh, total);
    if (k < ntiles) sums[k] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

static __global__ void __launch_bounds__(256) scan_add_kernel(int32_t* __restrict__ out,
                                                              int64_t n,
                                                              const int32_t* __restrict__ sums) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x)
    out[k] += sums[k / kScanTile];
}

static size_t scan_ws_ints(int64_t n) { return (size_t)((n + kScanTile - 1) / kScanTile) + 1; }

// out (n + 1) = exclusive scan of in (n); in and out must not overlap.  ws: scan_ws_ints(n)
static void exclusive_scan(const int32_t* in, int64_t n, int32_t* out, int32_t* ws,
                           hipStream_t s) {
  const int64_t ntiles = std::max<int64_t>(1, (n + kScanTile - 1) / kScanTile);
  hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)ntiles), dim3(kScanThreads), 0, s, in, n,
                     out, ws);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, s, ws, ntiles, out, n);
  hipLaunchKernelGGL(scan_add_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, out, n, ws);
}

}  // namespace msha
