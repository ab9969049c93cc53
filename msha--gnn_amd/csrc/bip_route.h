// Which kernel family serves msha_bip_attention_fwd / _bwd: the one decision that the two
// launches, msha_bip_supported and the host-only query msha_bip_route all ask.  Plain host
// C++ over plain values (sizes, the null-ness of rowmask and u_lo, the knobs as numbers):
// nothing here touches the device or the environment, so it also builds into the
// stand-alone host program scripts/route_check.cpp.  DESIGN §4 has the table.
#pragma once
#include <cstdint>

namespace msha {
namespace bip_route {

constexpr int kNone = 0;  // not covered: the general edge kernels
constexpr int kWalk = 1;  // CSR walk (edge_bip.hip)
constexpr int kMask = 2;  // row masks (edge_bip2.hip)
constexpr int kMfma = 3;  // row masks on the matrix cores (edge_bip3.hip)
constexpr int64_t k2G = 1ll << 31;
constexpr int kMaxMD = 4096;  // floats of one (M, H*F) LDS table: M = 32 at H*F = 128

struct Call {
  int64_t n_rows, n_cols, n_edges;
  bool rowmask;   // msha_graph.rowmask is set
  int heads, feat;
  int esize;      // sizeof the table element: 4 (fp32), 2 (bf16), 0 (any other dtype)
  bool compiled;  // (heads, feat) is in MSHA_FOR_EACH_SHAPE (edge_geo.h)
  float slope;
  bool dropout;   // p > 0
  bool u_lo;      // the forward's caller asks for the bf16 rounding residual
};

// MSHA_BIP2, MSHA_BIP3 (once per process), MSHA_BIP3_BWD32 (per call, -1 = unset), the row
// cut msha_bip2_bwd_min_rows
struct Knobs {
  int64_t bip2, bip3;
  int bwd32;
  int64_t cut;
};

struct Route {
  int fwd, bwd;
};

// msha_bip_supported.  32-bit buffer offsets below the kOOB mask bit: every table < 2 GiB.
// M <= 32 and M * H <= 64: a row's (edge, head) slots fit one 64-lane sub-group and a
// group's kPD rows fit the kColPages column pages.
inline bool covered(const Call& c) {
  if (c.n_rows <= 0 || c.n_cols <= 0 || c.heads <= 0 || c.feat <= 0) return false;
  const int64_t D = (int64_t)c.heads * c.feat;
  if (D % 64 != 0 || D > 256 || 64 % c.heads != 0 || c.feat % (D / 64) != 0) return false;
  if (c.n_cols > 32 || c.n_cols * D > kMaxMD || c.n_cols * c.heads > 64) return false;
  // (counts at or past 2^31 first: the byte products below then stay far inside 64 bits)
  if (c.n_rows >= k2G || c.n_edges >= k2G) return false;
  if (c.n_rows * D * 4 >= k2G || c.n_edges * c.heads * 4 >= k2G) return false;
  if (c.esize != 4 && c.esize != 2) return false;
  return c.compiled;
}

// the mask and MFMA kernels' shape: 2 x 64, one 32-bit column mask per row
inline bool maskable(const Call& c, const Knobs& k) {
  return k.bip2 != 0 && c.heads == 2 && c.feat == 64 && c.rowmask && c.n_cols <= 32 &&
         c.slope >= 0.f && c.slope <= 1.f && c.n_rows * 128 * 4 < k2G && c.n_edges * 8 < k2G;
}

inline Route route(const Call& c, const Knobs& k) {
  if (!covered(c)) return Route{kNone, kNone};
  const bool mask = maskable(c, k), large = c.n_rows >= k.cut, mfma = k.bip3 != 0;
  Route r{kWalk, kWalk};
  // below the cut (the shipped graphs: < 1 tile per wave) the forward is the mask kernel;
  // only the walk writes u_lo
  if (mask && !c.u_lo) r.fwd = large && mfma ? kMfma : kMask;
  // below the cut the backward is the walk.  fp32 MFMA: its dropout variants spill (the
  // keep words), so with dropout the mask kernel runs unless MSHA_BIP3_BWD32 forces it
  if (mask && large) {
    const bool f32_mask = c.esize == 4 && (k.bwd32 == 0 || (k.bwd32 < 0 && c.dropout));
    r.bwd = mfma && !f32_mask ? kMfma : kMask;
  }
  return r;
}

}  // namespace bip_route
}  // namespace msha
