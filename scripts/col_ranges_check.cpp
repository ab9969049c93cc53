// Stand-alone host check of the column-range cut and the route predicate of the column pass
// that carries the weight gradient (csrc/col_ranges.h) for a sanitizer build: plain C++, no
// device, no library.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined scripts/col_ranges_check.cpp -o col_ranges_check
//   ./col_ranges_check       (or any host compiler: clang++ -fsanitize=address,undefined ...)
//
// Cuts exactly sized heap copies of colptr (so a read or write past either array is caught)
// for degree patterns with empty columns, one huge column, all-empty graphs, nb = 1 and
// nb = n_cols, and checks: cut[0] = 0, cut[nb] = n_cols, strictly ascending (every range
// non-empty: nb <= n_cols), and -- where no range had to be moved to keep its neighbours
// non-empty -- a slot count within one column's degree of n_slots / nb.  Exits non-zero on
// a mismatch.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../msha--gnn_amd/csrc/col_ranges.h"

using namespace msha::colrange;

static int g_bad = 0, g_n = 0;
static void expect(bool ok, const char* what, long long a, long long b, long long c) {
  ++g_n;
  if (!ok) {
    ++g_bad;
    std::printf("MISMATCH %s (pattern %lld, n_cols %lld, nb %lld)\n", what, a, b, c);
  }
}

template <typename I>
static void check(int pattern, const std::vector<int64_t>& deg, int nb) {
  const int64_t n = (int64_t)deg.size();
  I* colptr = new I[n + 1];
  colptr[0] = 0;
  int64_t maxdeg = 0;
  for (int64_t j = 0; j < n; ++j) {
    colptr[j + 1] = (I)(colptr[j] + deg[j]);
    if (deg[j] > maxdeg) maxdeg = deg[j];
  }
  int32_t* cut_ = new int32_t[nb + 1];
  cut(colptr, n, nb, cut_);
  const int64_t total = colptr[n];
  expect(cut_[0] == 0 && cut_[nb] == n, "ends", pattern, n, nb);
  bool asc = true, even = true;
  for (int b = 0; b < nb; ++b) {
    if (cut_[b + 1] <= cut_[b]) asc = false;
    // a range that starts where the rule puts it (first column reaching b / nb of the slots)
    // and ends where the rule puts the next one holds within one degree of total / nb slots
    const int64_t lo_t = (total * b + nb - 1) / nb, hi_t = (total * (b + 1) + nb - 1) / nb;
    const bool lo_ruled = b == 0 || ((int64_t)colptr[cut_[b]] >= lo_t &&
                                     (int64_t)colptr[cut_[b] - 1] < lo_t);
    const bool hi_ruled = b + 1 == nb || ((int64_t)colptr[cut_[b + 1]] >= hi_t &&
                                          (int64_t)colptr[cut_[b + 1] - 1] < hi_t);
    if (lo_ruled && hi_ruled && asc) {
      const int64_t slots = (int64_t)colptr[cut_[b + 1]] - (int64_t)colptr[cut_[b]];
      const int64_t d = slots * nb - total;  // nb * (slots - total / nb)
      if (d > (maxdeg + 1) * nb || -d > (maxdeg + 1) * nb) even = false;
    }
  }
  expect(asc, "ascending / non-empty", pattern, n, nb);
  expect(even, "slot balance", pattern, n, nb);
  delete[] cut_;
  delete[] colptr;
}

int main() {
  const int64_t sizes[] = {1, 2, 15, 16, 17, 255, 256, 257, 1045, 4099};
  for (int64_t n : sizes)
    for (int pattern = 0; pattern < 6; ++pattern) {
      std::vector<int64_t> deg((size_t)n);
      for (int64_t j = 0; j < n; ++j) {
        const int64_t cyc[6] = {0, 1, 8, 9, 17, 40};
        deg[(size_t)j] = pattern == 0   ? 0
                         : pattern == 1 ? 3
                         : pattern == 2 ? cyc[j % 6]
                         : pattern == 3 ? (j == n / 2 ? 100000 : 1)
                         : pattern == 4 ? (j < n / 2 ? 0 : 7)
                                        : (j * 2654435761u >> 7) % 41;
      }
      const int full = blocks_for(n);
      const int nbs[4] = {1, full, full > 3 ? full / 3 : 1, full > 1 ? full - 1 : 1};
      for (int nb : nbs) {
        check<int64_t>(pattern, deg, nb);
        check<int32_t>(pattern, deg, nb);
      }
    }
  // the route's scope
  const uintptr_t a = 1u << 20;
  auto r = [&](int64_t rows, int64_t cols, int64_t edges, int64_t multi, int h, int f, bool fp32,
               int64_t K, int64_t ldx, bool rt, bool ert, bool bufs, uintptr_t X) {
    return route(true, rows, cols, edges, multi, h, f, fp32, K, ldx, rt, ert, bufs, 32, X, a, a);
  };
  expect(r(100000, 100000, 2000000, 0, 8, 16, true, 128, 128, true, true, true, a) == 256, "C4", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 128, true, true, true, a) == 100, "small", 0, 0, 0);
  expect(route(false, 100, 100, 500, 0, 8, 16, true, 128, 128, true, true, true, 32, a, a, a) == 0, "knob", 0, 0, 0);
  expect(r(100, 101, 500, 0, 8, 16, true, 128, 128, true, true, true, a) == 0, "bipartite", 0, 0, 0);
  expect(r(100, 100, 500, 1, 8, 16, true, 128, 128, true, true, true, a) == 0, "multi", 0, 0, 0);
  expect(r(100, 100, 500, 0, 2, 64, true, 128, 128, true, true, true, a) == 100, "2x64", 0, 0, 0);
  expect(r(100, 100, 500, 0, 4, 32, true, 128, 128, true, true, true, a) == 100, "4x32", 0, 0, 0);
  expect(r(100, 100, 500, 0, 1, 128, true, 128, 128, true, true, true, a) == 100, "1x128", 0, 0, 0);
  expect(r(100, 100, 500, 0, 2, 32, true, 128, 128, true, true, true, a) == 0, "2x32", 0, 0, 0);
  expect(r(100, 100, 500, 0, 16, 8, true, 128, 128, true, true, true, a) == 0, "16x8", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, false, 128, 128, true, true, true, a) == 0, "bf16", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 64, 64, true, true, true, a) == 0, "K", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 130, true, true, true, a) == 0, "pitch", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 132, true, true, true, a) == 100, "pitch 132", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 128, false, true, true, a) == 0, "row terms", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 128, true, false, true, a) == 0, "a_r", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 128, true, true, false, a) == 0, "no buffers", 0, 0, 0);
  expect(r(100, 100, 500, 0, 8, 16, true, 128, 128, true, true, true, a + 8) == 0, "alignment", 0, 0, 0);
  expect(r(1ll << 22, 1ll << 22, 500, 0, 8, 16, true, 128, 128, true, true, true, a) == 0, "2 GiB table", 0, 0, 0);
  expect(r(100, 100, 1ll << 26, 0, 8, 16, true, 128, 128, true, true, true, a) == 0, "2 GiB edges", 0, 0, 0);
  std::printf("col_ranges_check: %d checks, %d mismatches\n", g_n, g_bad);
  return g_bad != 0;
}
