// Stand-alone host check of the resident-W route predicates (csrc/skinny_route.h) for a
// sanitizer build: plain C++, no device, no library.
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

#include "../msha--gnn_amd/csrc/skinny_route.h"

using namespace msha::route;

static int g_bad = 0, g_n = 0;
static void expect(int got, int want, const char* what, long long a = 0, long long b = 0,
                   long long c = 0) {
  ++g_n;
  if (got != want) {
    ++g_bad;
    std::printf("MISMATCH %s(%lld, %lld, %lld): got %d, want %d\n", what, a, b, c, got, want);
  }
}

int main() {
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
  std::printf("route_check: %d checks, %d mismatches, %d covered projection calls\n", g_n, g_bad, reached);
  return g_bad != 0;
}
