// The wave selection network of the top-K kernels (topk.hip, explain.hip): a bitonic
// network over 64-bit keys ((image << 32) | ~index, order_key.h's tk_key; 0 is "no
// candidate") held in registers as element r * 64 + lane, and the store of a selected key.
// Integer compares only: what it selects does not depend on the order of execution.
#pragma once

#include "common.h"
#include "order_key.h"

namespace msha {

typedef unsigned long long u64;

constexpr int kTkMaxK = 128;
constexpr int kTkMergeChunk = 4096;  // elements one wave selects from

__device__ __forceinline__ void tk_emit(u64 key, int sigmoid, int64_t col_offset, float* val,
                                        int64_t* idx) {
  if (key == 0ull) {
    *val = sigmoid ? 0.f : -__builtin_inff();
    *idx = -1;
    return;
  }
  float v = tk_value((uint32_t)(key >> 32));
  if (sigmoid) v = 1.f / (1.f + __expf(-v));  // scorer.hip's expression
  *val = v;
  *idx = (int64_t)(uint32_t)~(uint32_t)key + col_offset;
}

// One compare-exchange step (block size k, distance j) of the bitonic network over the
// 64 * EPL keys a wave holds as element r * 64 + lane; blocks with (element & k) == 0 sort
// descending.
template <int EPL>
__device__ __forceinline__ void tk_step(u64 (&a)[EPL], int lane, int k, int j) {
  if (j < 64) {
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const u64 o = __shfl_xor(a[r], j);
      const bool up = (((r << 6) | lane) & k) == 0;
      const bool lower = (lane & j) == 0;
      const u64 mx = a[r] > o ? a[r] : o, mn = a[r] > o ? o : a[r];
      a[r] = (lower == up) ? mx : mn;
    }
  } else {
    const int jr = j >> 6;
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      if ((r & jr) == 0) {
        const bool up = ((r << 6) & k) == 0;  // k >= 128: decided by r alone
        const u64 x = a[r], y = a[r | jr];
        const u64 mx = x > y ? x : y, mn = x > y ? y : x;
        a[r] = up ? mx : mn;
        a[r | jr] = up ? mn : mx;
      }
    }
  }
}

// Bitonic sort, descending.
template <int EPL>
__device__ __forceinline__ void tk_sort(u64 (&a)[EPL], int lane) {
  constexpr int L = 64 * EPL;
#pragma unroll
  for (int k = 2; k <= L; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) tk_step<EPL>(a, lane, k, j);
  }
}

// a[0 .. EPL/2): sorted descending (the best so far); a[EPL/2 .. EPL): new keys in any
// order.  Sorts the new half ascending (the descending network on the complements), which
// makes the whole a bitonic sequence, then runs the network's last stage: all 64 * EPL keys
// descending.
template <int EPL>
__device__ __forceinline__ void tk_merge_top(u64 (&a)[EPL], int lane) {
  constexpr int H = EPL / 2, L = 64 * EPL;
  u64 u[H];
#pragma unroll
  for (int r = 0; r < H; ++r) u[r] = ~a[H + r];
  tk_sort<H>(u, lane);
#pragma unroll
  for (int r = 0; r < H; ++r) a[H + r] = ~u[r];
#pragma unroll
  for (int j = L >> 1; j > 0; j >>= 1) tk_step<EPL>(a, lane, L, j);
}

// element K - 1 of the sorted keys, in every lane
template <int EPL>
__device__ __forceinline__ u64 tk_kth(const u64 (&a)[EPL], int K) {
  u64 t = 0;
#pragma unroll
  for (int r = 0; r < EPL; ++r)
    if (r == ((K - 1) >> 6)) t = a[r];
  return __shfl(t, (K - 1) & 63);
}

}  // namespace msha
