// The bipartite attention's host side, shared by edge_bip.hip (the entry points and the CSR
// walk), edge_bip2.hip (mask kernels) and edge_bip3.hip (MFMA kernels): the route
// (bip_route.h) picks a family, the family's launcher below picks the template instance
// and submits the block-partial reduce (bip_reduce.h).
#pragma once

#include <type_traits>

#include "bip_reduce.h"
#include "bip_route.h"

namespace msha {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for run-time bools: one
// spelling of "every combination of these template flags is an instance"
template <class F>
inline void with_bools(F&& f) {
  f();
}
template <class F, class... Bs>
inline void with_bools(F&& f, bool b, Bs... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <bool BF16>
using bip_table_t = std::conditional_t<BF16, bf16_t, float>;

// The arguments of msha_bip_attention_fwd / _bwd as the launchers take them; part / nb: the
// block-partial workspace and the block count it was sized for (the CU count)
struct BipFwd {
  const msha_graph* g;
  int dtype;
  const float *el, *er;
  const void *hc, *hs;
  float slope;
  Dropout dp;
  void *u, *u_lo;
  float *lse, *attd;
  void* v;
  float* part;
  int nb;
  bool bf16() const { return dtype == MSHA_DTYPE_BF16; }
};
struct BipBwd {
  const msha_graph* g;
  int dtype;
  const float *el, *er;
  const void* hc;
  const float* lse;
  const void *dU, *hs, *dV;
  const float* row_coef;
  float slope;
  Dropout dp;
  float *d_el, *d_er;
  void *d_hc, *d_hs;
  float* part;
  int nb;
  bool bf16() const { return dtype == MSHA_DTYPE_BF16; }
};

// each launches its kernel and submits the reduce (forward: only with hs / v); the caller
// asked bip_route: mask and MFMA serve 2 x 64 graphs with row masks only
void bip2_fwd(const BipFwd& a, hipStream_t s);
void bip2_bwd(const BipBwd& a, hipStream_t s);
void bip3_fwd(const BipFwd& a, hipStream_t s);
void bip3_bwd(const BipBwd& a, hipStream_t s);

}  // namespace msha
