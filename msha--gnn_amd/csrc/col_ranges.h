// Column ranges of the fused column pass + weight gradient (edge_attention.hip,
// bwd_cols_wgrad_kernel) and the decision whether a call takes that kernel: what the launch
// and the host-only route query (msha_edge_attention_bwd_fused_wgrad_route) both ask.
// Plain host C++ over plain arguments: nothing here touches the device, so it also builds
// into a stand-alone host program (scripts/col_ranges_check.cpp).
#pragma once
#include <cstdint>

namespace msha {
namespace colrange {

constexpr int kMaxBlocks = 256;  // what wgrad_reduce_kernel reads in one round trip

// blocks for a graph of n_cols columns: one per CU of the part while columns last
inline int blocks_for(int64_t n_cols) {
  return n_cols <= 0 ? 0 : (int)(n_cols < kMaxBlocks ? n_cols : kMaxBlocks);
}

// cut[0..nb]: block b owns columns [cut[b], cut[b+1]).  Block b starts at the first column
// whose CSC slot offset reaches b / nb of the slots, moved where needed so that the block
// before it and every block after it keep at least one column (needs 0 < nb <= n_cols, as
// blocks_for gives: every range is non-empty).  Where neither end of a range was moved its
// slot count is within one column's degree of n_slots / nb.  colptr: n_cols + 1 ascending
// offsets.
template <typename I>
inline void cut(const I* colptr, int64_t n_cols, int nb, int32_t* out) {
  const int64_t base = (int64_t)colptr[0], total = (int64_t)colptr[n_cols] - base;
  int64_t j = 0;
  out[0] = 0;
  for (int b = 1; b < nb; ++b) {
    // ceil(b * total / nb) without overflow for total < 2^31 * 2^8
    const int64_t target = base + (total * b + nb - 1) / nb;
    // first column whose offset reaches the target, in [previous cut + 1, n_cols - (nb - b)]:
    // one column stays for the block before and for each of the nb - b blocks that follow
    // (nb <= n_cols: the window is never empty)
    int64_t lo = j + 1, hi = n_cols - (nb - b);
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)colptr[mid] >= target) hi = mid; else lo = mid + 1;
    }
    j = lo;
    out[b] = (int32_t)j;
  }
  out[nb] = (int32_t)n_cols;
}

// the fused kernels' scope: fp32 tables of 128 floats a row (8 x 16: the head-per-lane column
// pass; 4 x 32, 2 x 64, 1 x 128: the quad-per-lane one), a 128-wide projection input, whole
// columns (no multi-chunk column), row terms from the forward (d_el is written before the column pass), the er
// table (not the a_r recompute), every table addressable by 32-bit byte offsets.
// Returns the block count, 0 = the caller keeps its two launches.
inline int route(bool enabled, int64_t n_rows, int64_t n_cols, int64_t n_edges, int64_t n_multi,
                 int heads, int feat, bool fp32, int64_t K, int64_t ldx, bool rowterms,
                 bool er_table, bool cols_buf, int rec_stride, uintptr_t X, uintptr_t al,
                 uintptr_t ar) {
  const int64_t lim = 1ll << 31;
  const bool shape = (heads == 8 && feat == 16) || (heads == 4 && feat == 32) ||
                     (heads == 2 && feat == 64) || (heads == 1 && feat == 128);
  if (!enabled || !fp32 || !shape || K != 128 || ldx < K || ldx % 4) return 0;
  if (n_multi != 0 || !rowterms || !er_table || !cols_buf || n_rows != n_cols) return 0;
  if (((X | al | ar) & 15) != 0) return 0;
  if (n_rows * (int64_t)heads * feat * 4 >= lim || n_edges * 4 * (int64_t)heads >= lim ||
      n_rows * 4 * (int64_t)rec_stride >= lim || n_cols * ldx * 4 >= lim)
    return 0;
  return blocks_for(n_cols);
}

}  // namespace colrange
}  // namespace msha
