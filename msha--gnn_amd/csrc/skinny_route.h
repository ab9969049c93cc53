// Which calls the resident-W kernels of skinny.hip cover: the one decision that the
// launches and the host-only route queries (msha_*_route, include/msha_gnn.h) both ask.
// Plain host C++ over plain arguments (sizes, strides, addresses as integers, the two
// environment knobs as values): nothing here touches the device, so the predicates also
// build into a stand-alone host program (scripts/route_check.cpp).
#pragma once
#include <cstdint>

namespace msha {
namespace route {

constexpr int kTiled = 0;     // not covered: the caller runs its tiled kernel
constexpr int kResident = 1;  // exact-fp32 / bf16 resident-W kernel
constexpr int kSplit = 2;     // split-bf16 resident-W kernel (fp32 operands)
constexpr int64_t kMinRows = 1024;
constexpr int64_t k2G = 1ll << 31;
// the windowed pair gather's tables end at or below this byte count: the offset of a masked
// row (this value) plus the bytes of a row's last 16-byte slot stays below 2^32
constexpr int64_t kWindowMax = 0xFFFFFE00ll;

inline bool shape_ok(int64_t K, int64_t N) { return (K == 64 || K == 128) && (N == 64 || N == 128); }
inline bool aligned16(uintptr_t a, uintptr_t b, uintptr_t c, uintptr_t d = 0) {
  return ((a | b | c | d) & 15) == 0;
}

// proj_kernel<T, K, N, FE, SPLIT>: `code`, and the instance's FE (0 = no score vector)
struct Proj {
  int code;
  int64_t K, N;
  int fe;
};
// esize: sizeof(T), 4 (fp32) or 2 (bf16); score: al or ar given; split_min: the fp32
// cut-over to the split-bf16 form (MSHA_PROJ_SPLIT_MIN_ROWS)
inline Proj project(bool enabled, int64_t split_min, int64_t M, int64_t K, int heads, int feat,
                    int esize, uintptr_t X, uintptr_t W, uintptr_t h, bool score) {
  const int64_t N = (int64_t)heads * feat;
  const Proj no{kTiled, K, N, 0};
  // (M K esize < 2^31, as a quotient: K esize divides 2^31 for every covered K, any M is safe)
  if (!enabled || !shape_ok(K, N) || M < kMinRows || M >= k2G / (K * esize)) return no;
  if (!aligned16(X, W, h)) return no;
  const int minfe = 16 / esize;
  if (score && (feat < minfe || N % feat != 0)) return no;
  // FE in {0, 16, 32, 64, N}
  const int fe = score ? feat : 0;
  if (fe != 0 && fe != 16 && fe != 32 && fe != 64 && fe != N) return no;
  const bool split = esize == 4 && M >= split_min;
  return Proj{split ? kSplit : kResident, K, N, fe};
}

// pair_kernel (kResident) / pair_x3_kernel (kSplit, the windowed form): ba / bb are the
// byte extents of the two tables that the windowed kernel's buffer descriptors take
struct Pair {
  int code;
  uint32_t ba, bb;
};
inline Pair pair_linear(bool enabled, int64_t P, int64_t K, int64_t N, uintptr_t G, int64_t ldg,
                        bool has_gi, uintptr_t G2, int64_t ldg2, bool has_gj, int64_t g_rows,
                        int64_t g2_rows, uintptr_t W, uintptr_t out) {
  const Pair no{kTiled, 0, 0};
  if (!enabled || P < kMinRows || P >= k2G || !has_gi || !has_gj) return no;
  if (G2 == 0) { G2 = G; ldg2 = ldg; g2_rows = g_rows; }
  if (ldg % 4 || ldg2 % 4 || !aligned16(G, G2, out, W)) return no;
  if (!shape_ok(K, N)) return no;
  // table bytes up to the last row's K columns (the kernel reads no further); a table
  // past the window limit (or of unknown rows) is no window
  auto span = [&](int64_t rows, int64_t ld) -> int64_t {
    if (rows <= 0 || ld < 0) return -1;
    if (ld > 0 && rows - 1 > (kWindowMax / 4) / ld) return kWindowMax + 1;
    return ((rows - 1) * ld + K) * 4;
  };
  const int64_t ba = span(g_rows, ldg), bb = span(g2_rows, ldg2);
  const bool window = ba > 0 && bb > 0 && ba <= kWindowMax && bb <= kWindowMax && P * N * 4 < k2G;
  if (!window) return Pair{kResident, 0, 0};
  return Pair{kSplit, (uint32_t)ba, (uint32_t)bb};
}

// pair_bf16_kernel
inline int pair_linear_bf16(bool enabled, int64_t P, int64_t K, int64_t N, uintptr_t G, int64_t ldg,
                            bool has_gi, uintptr_t G2, int64_t ldg2, bool has_gj, uintptr_t W,
                            uintptr_t out) {
  if (!enabled || P < kMinRows || P >= k2G || !has_gi || !has_gj) return kTiled;
  if (G2 == 0) { G2 = G; ldg2 = ldg; }
  if (ldg % 8 || ldg2 % 8 || !aligned16(G, G2, W, out)) return kTiled;
  return shape_ok(K, N) ? kResident : kTiled;
}

// dx_kernel<K, N>: dX (M x N) = (Dh + d1 (x) a1 [+ d2 (x) a2]) W^T, Dh (M x K), K = hH hF
inline int dx(bool enabled, int64_t M, int64_t N, int64_t K, uintptr_t Dh, uintptr_t W, uintptr_t C,
              int hH, int hF, bool has_term) {
  if (!enabled || !shape_ok(K, N) || M < kMinRows) return kTiled;
  if (hF < 16 || K % hF != 0 || (int64_t)hH * hF != K || !has_term) return kTiled;
  // M K 4 and M hH 4 below 2^31 (quotients: K and hH are powers of two here)
  if (M >= k2G / (K * 4) || M >= k2G / ((int64_t)hH * 4)) return kTiled;
  if (!aligned16(Dh, C, W)) return kTiled;
  return kResident;
}

}  // namespace route
}  // namespace msha
