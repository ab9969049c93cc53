// Stand-alone host check of the route predicates -- the resident-W kernels'
// (csrc/skinny_route.h) and the bipartite attention's (csrc/bip_route.h) -- for a sanitizer
// build: plain C++, no device, no library.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined scripts/route_check.cpp -o route_check
//   ./route_check            (or any host compiler: clang++ -fsanitize=address,undefined ...)
//
// Walks every instance of the dispatch tables and the boundary shapes (1,023 / 1,024 rows,
// byte counts at 2^31, the 4 GiB window, g_rows = 0, a null G2, offset bases, odd pitches)
// and compares the codes with the documented rule; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>

#include "../msha--gnn_amd/csrc/bip_route.h"
#include "../msha--gnn_amd/csrc/skinny_route.h"

using namespace msha::route;
namespace br = msha::bip_route;

static int g_bad = 0, g_n = 0;
static void expect(int got, int want, const char* what, long long a = 0, long long b = 0,
                   long long c = 0) {
  ++g_n;
  if (got != want) {
    ++g_bad;
    std::printf("MISMATCH %s(%lld, %lld, %lld): got %d, want %d\n", what, a, b, c, got, want);
  }
}

// The bipartite attention's route (csrc/bip_route.h) against the rule as DESIGN §4 states
// it, written out here a second time in the order of the table: every knob combination,
// cut - 1 and cut, u_lo, a null rowmask, slopes outside [0, 1], the 2^31 byte limits and
// the shapes the mask kernels do not serve.  Returns how many calls reached each kind.
static void check_bip(int (&seen)[2][4]) {
  struct Shape {
    int heads, feat;
    int64_t m;
    bool covered;  // by the walk's shape rule
  };
  const Shape shapes[] = {{2, 64, 32, true},  {2, 64, 20, true},  {2, 64, 33, false}, {8, 16, 8, true},
                          {8, 16, 9, false},  {1, 64, 17, true},  {2, 128, 16, true}, {2, 128, 17, false},
                          {4, 32, 16, true},  {4, 64, 16, true},  {4, 64, 17, false}, {2, 16, 8, false},
                          {16, 8, 4, false},  {1, 192, 8, false}, {0, 64, 8, false},  {2, 0, 8, false}};
  const int64_t cut = 256;
  for (const Shape& sh : shapes)
    for (int esize : {4, 2, 0})
      for (int64_t bip2 : {1, 0})
        for (int64_t bip3 : {1, 0})
          for (int bwd32 : {-1, 0, 1})
            for (int64_t rows : {cut - 1, cut})
              for (int flags = 0; flags < 8; ++flags)
                for (float slope : {0.2f, 0.f, 1.f, -0.1f, 1.5f}) {
                  const bool u_lo = flags & 1, rowmask = !(flags & 2), drop = flags & 4;
                  const bool compiled = sh.heads >= 1 && sh.heads <= 8 && sh.feat >= 8 && sh.feat <= 128;
                  const br::Call c{rows, sh.m, rows * 2, rowmask, sh.heads, sh.feat, esize, compiled,
                                   slope, drop, u_lo};
                  const br::Route r = br::route(c, br::Knobs{bip2, bip3, bwd32, cut});
                  int fwd = br::kNone, bwd = br::kNone;
                  if (sh.covered && esize != 0) {
                    const bool maskable = bip2 != 0 && sh.heads == 2 && sh.feat == 64 && rowmask &&
                                          slope >= 0.f && slope <= 1.f;
                    if (u_lo || !maskable) fwd = br::kWalk;
                    else if (rows >= cut && bip3 != 0) fwd = br::kMfma;
                    else fwd = br::kMask;
                    if (!maskable || rows < cut) bwd = br::kWalk;
                    else if (bip3 != 0 && (esize == 2 || bwd32 == 1 || (bwd32 < 0 && !drop))) bwd = br::kMfma;
                    else bwd = br::kMask;
                  }
                  expect(r.fwd, fwd, "bip fwd", sh.heads, sh.feat, flags);
                  expect(r.bwd, bwd, "bip bwd", sh.heads, sh.feat, flags);
                  ++seen[0][r.fwd];
                  ++seen[1][r.bwd];
                }
  // the byte limits: n_rows H F 4 and n_edges H 4 (covered); n_edges 8 (maskable; at 2 x 64
  // the same bound as the covered one, so it never decides alone)
  const br::Knobs k{1, 1, -1, 131072};
  auto at = [&](int64_t rows, int64_t edges, int heads, int feat, int64_t m) {
    return br::route(br::Call{rows, m, edges, true, heads, feat, 4, true, 0.2f, false, false}, k);
  };
  const int64_t r128 = br::k2G / (128 * 4), r256 = br::k2G / (256 * 4);
  expect(at(r128 - 1, 8, 2, 64, 32).fwd, br::kMfma, "bip rows below 2^31 bytes", r128 - 1);
  expect(at(r128 - 1, 8, 2, 64, 32).bwd, br::kMfma, "bip rows below 2^31 bytes, bwd", r128 - 1);
  expect(at(r128, 8, 2, 64, 32).fwd, br::kNone, "bip rows at 2^31 bytes", r128);
  expect(at(r256 - 1, 8, 4, 64, 16).fwd, br::kWalk, "bip 4 x 64 rows below 2^31 bytes", r256 - 1);
  expect(at(r256, 8, 4, 64, 16).bwd, br::kNone, "bip 4 x 64 rows at 2^31 bytes", r256);
  expect(at(1000, br::k2G / 8 - 1, 2, 64, 32).fwd, br::kMask, "bip edges below 2^31 bytes");
  expect(at(1000, br::k2G / 8, 2, 64, 32).fwd, br::kNone, "bip edges at 2^31 bytes");
  expect(at(1000, br::k2G / 32, 8, 16, 8).fwd, br::kNone, "bip 8 heads edges at 2^31 bytes");
  expect(at(1000, br::k2G / 32 - 1, 8, 16, 8).fwd, br::kWalk, "bip 8 heads edges below 2^31 bytes");
  expect(at(INT64_MAX / 2, 8, 2, 64, 32).fwd, br::kNone, "bip huge rows");
  expect(at(1000, INT64_MAX / 2, 2, 64, 32).bwd, br::kNone, "bip huge edges");
  expect(at(0, 0, 2, 64, 32).fwd, br::kNone, "bip no rows");
  expect(at(1000, 8, 2, 64, 0).fwd, br::kNone, "bip no columns");
  // (heads, feat) outside the compiled set, whatever else holds
  expect(br::route(br::Call{1000, 32, 2000, true, 2, 64, 4, false, 0.2f, false, false}, k).fwd, br::kNone,
         "bip not compiled");
  // MSHA_BIP3_BWD32 above 1 forces the MFMA backward like 1 does
  expect(br::route(br::Call{1000, 32, 2000, true, 2, 64, 4, true, 0.2f, true, false}, br::Knobs{1, 1, 2, 0}).bwd,
         br::kMfma, "bip bwd32 = 2");
}

int main() {
  int bip_seen[2][4] = {};
  check_bip(bip_seen);
  const uintptr_t base = (uintptr_t)1 << 30;
  const int64_t split_min = 65536;
  const int64_t ks[2] = {128, 64};
  const int64_t sizes[] = {1023, 1024, 1045, 32789, 65535, 65536, 65549};
  int reached = 0;
  for (int64_t K : ks)
    for (int64_t N : ks)
      for (int fe : {0, 16, 32, 64, 128}) {
        if (fe > N) continue;
        const int feat = fe ? fe : 16, heads = (int)(N / feat);
        for (int esize : {4, 2}) {
          for (int64_t M : sizes) {
            const Proj r = project(true, split_min, M, K, heads, feat, esize, base, base, base, fe != 0);
            const int want = M < 1024 ? kTiled : esize == 4 && M >= split_min ? kSplit : kResident;
            expect(r.code, want, "project", M, K, N);
            if (r.code) expect(r.fe, fe, "project.fe", M, K, N);
            reached += r.code != 0;
          }
          // M K esize at 2^31
          const int64_t lim = k2G / (K * esize);
          expect(project(true, split_min, lim - 1, K, heads, feat, esize, base, base, base, fe != 0).code != 0, 1,
                 "project below 2^31", lim - 1, K, N);
          expect(project(true, split_min, lim, K, heads, feat, esize, base, base, base, fe != 0).code, kTiled,
                 "project at 2^31", lim, K, N);
          expect(project(false, split_min, 2048, K, heads, feat, esize, base, base, base, fe != 0).code, kTiled,
                 "project disabled", 2048, K, N);
          for (int which = 0; which < 3; ++which)
            expect(project(true, split_min, 2048, K, heads, feat, esize, base + (which == 0 ? 4 : 0),
                           base + (which == 1 ? 4 : 0), base + (which == 2 ? 4 : 0), fe != 0).code,
                   kTiled, "project misaligned", which, K, N);
        }
      }
  expect(project(true, split_min, 2048, 128, 16, 8, 4, base, base, base, true).code, kTiled, "fp32 feat 8");
  expect(project(true, split_min, 2048, 128, 16, 8, 2, base, base, base, true).code, kTiled, "bf16 feat 8");
  expect(project(true, split_min, 2048, 128, 32, 4, 2, base, base, base, true).code, kTiled, "bf16 feat 4");
  expect(project(true, split_min, 2048, 128, 16, 8, 4, base, base, base, false).code, kResident, "no score");
  expect(project(true, split_min, 2048, 96, 8, 16, 4, base, base, base, true).code, kTiled, "K 96");
  expect(project(true, split_min, 2048, 128, 6, 16, 4, base, base, base, true).code, kTiled, "N 96");
  expect(project(true, split_min, INT64_MAX / 1024, 128, 8, 16, 4, base, base, base, true).code, kTiled, "huge M");

  for (int64_t K : ks)
    for (int64_t N : ks) {
      const uintptr_t G2 = base + (1u << 20);
      for (int64_t P : {(int64_t)1023, (int64_t)1024, (int64_t)1045, (int64_t)4099}) {
        const int live = P >= 1024;
        expect(pair_linear(true, P, K, N, base, K + 4, true, G2, K + 8, true, 37, 53, base, base).code,
               live ? kSplit : kTiled, "pair window", P, K, N);
        expect(pair_linear(true, P, K, N, base, K + 4, true, G2, K + 8, true, 0, 0, base, base).code,
               live ? kResident : kTiled, "pair g_rows 0", P, K, N);
        expect(pair_linear(true, P, K, N, base, K + 4, true, G2, K + 8, true, 37, 0, base, base).code,
               live ? kResident : kTiled, "pair g2_rows 0", P, K, N);
        expect(pair_linear(true, P, K, N, base, K + 4, true, 0, 0, true, 37, 0, base, base).code,
               live ? kSplit : kTiled, "pair null G2", P, K, N);
        expect(pair_linear(true, P, K, N, base, K + 4, true, 0, 0, true, 0, 53, base, base).code,
               live ? kResident : kTiled, "pair null G2, g_rows 0", P, K, N);
        expect(pair_linear_bf16(true, P, K, N, base, K + 8, true, G2, K + 16, true, base, base),
               live ? kResident : kTiled, "pair bf16", P, K, N);
        expect(pair_linear_bf16(true, P, K, N, base, K + 8, true, 0, 0, true, base, base),
               live ? kResident : kTiled, "pair bf16 null G2", P, K, N);
      }
      const Pair w = pair_linear(true, 1024, K, N, base, K + 4, true, G2, K + 8, true, 37, 53, base, base);
      expect((int)(w.ba == (36 * (K + 4) + K) * 4), 1, "pair ba", K, N);
      expect((int)(w.bb == (52 * (K + 8) + K) * 4), 1, "pair bb", K, N);
      // the window limit (4 GiB less 512 bytes) and the output's 2^31 bytes
      const int64_t rows = kWindowMax / (4 * K);
      expect(pair_linear(true, 1024, K, N, base, K, true, G2, K, true, rows, 53, base, base).code, kSplit,
             "pair table at the window limit", rows, K, N);
      expect(pair_linear(true, 1024, K, N, base, K, true, G2, K, true, rows + 1, 53, base, base).code, kResident,
             "pair table past the window limit", rows + 1, K, N);
      expect(pair_linear(true, 1024, K, N, base, K, true, G2, K, true, 53, INT64_MAX / 4, base, base).code,
             kResident, "pair huge g2_rows", K, N);
      expect(pair_linear(true, k2G / (4 * N) - 1, K, N, base, K, true, G2, K, true, 37, 53, base, base).code,
             kSplit, "pair output below 2^31", K, N);
      expect(pair_linear(true, k2G / (4 * N), K, N, base, K, true, G2, K, true, 37, 53, base, base).code,
             kResident, "pair output at 2^31", K, N);
      expect(pair_linear(true, k2G - 1, K, N, base, K, true, G2, K, true, 37, 53, base, base).code, kResident,
             "pair P below 2^31", K, N);
      expect(pair_linear(true, k2G, K, N, base, K, true, G2, K, true, 37, 53, base, base).code, kTiled,
             "pair P at 2^31", K, N);
      expect(pair_linear(true, 2048, K, N, base + 4, K, true, G2, K, true, 37, 53, base, base).code, kTiled,
             "pair G + 4", K, N);
      expect(pair_linear(true, 2048, K, N, base, K + 2, true, G2, K, true, 37, 53, base, base).code, kTiled,
             "pair ldg % 4", K, N);
      expect(pair_linear(true, 2048, K, N, base, K, false, G2, K, true, 37, 53, base, base).code, kTiled,
             "pair no gi", K, N);
      expect(pair_linear(false, 2048, K, N, base, K, true, G2, K, true, 37, 53, base, base).code, kTiled,
             "pair disabled", K, N);
      expect(pair_linear_bf16(true, 2048, K, N, base, K + 4, true, G2, K, true, base, base), kTiled,
             "pair bf16 ldg % 8", K, N);
      // dx: K = hH hF, N the input width
      for (int hF : {8, 16, 32, 64, 128}) {
        const bool ok = hF >= 16 && K % hF == 0;
        const int hH = ok ? (int)(K / hF) : 1;
        for (int64_t M : {(int64_t)1023, (int64_t)1024, (int64_t)32789})
          expect(dx(true, M, N, K, base, base, base, hH, hF, true), ok && M >= 1024 ? kResident : kTiled,
                 "dx", M, K, hF);
      }
      expect(dx(true, k2G / (4 * K) - 1, N, K, base, base, base, (int)(K / 16), 16, true), kResident,
             "dx below 2^31", K, N);
      expect(dx(true, k2G / (4 * K), N, K, base, base, base, (int)(K / 16), 16, true), kTiled, "dx at 2^31", K, N);
      expect(dx(true, 2048, N, K, base, base, base, (int)(K / 16), 16, false), kTiled, "dx no term", K, N);
      expect(dx(true, 2048, N, K, base, base, base + 4, (int)(K / 16), 16, true), kTiled, "dx C + 4", K, N);
    }
  for (int d = 0; d < 2; ++d) {
    std::printf("bip %s: %d none, %d walk, %d mask, %d mfma\n", d ? "bwd" : "fwd", bip_seen[d][0],
                bip_seen[d][1], bip_seen[d][2], bip_seen[d][3]);
    for (int kind = 0; kind < 4; ++kind) expect(bip_seen[d][kind] > 0, 1, "bip kind reached", d, kind);
  }
  std::printf("route_check: %d checks, %d mismatches, %d covered projection calls\n", g_n, g_bad, reached);
  return g_bad != 0;
}
