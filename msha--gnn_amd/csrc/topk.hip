// Top-K link retrieval for the inner-product scorer (LLP.py:20 Hits@K, Explainer.py:31-34):
// for each query row, the K candidates of a table with the highest logit
// sum_f Q[q, f] * T[j, f], without ever writing the (B, n) score matrix.
//
//   topk_inner   inner_tile.h's streamed tile (query rows resident as MFMA A operands, the
//                candidates through a double-buffered LDS image; a logit is one accumulation
//                chain whose order is fixed by f alone, so it does not depend on the tile,
//                the block or the column split that computed it) with a selecting epilogue.
//                After a tile's MFMAs each lane compares its logits with the row's K-th best
//                key (LDS); survivors are appended to the row's buffer through an LDS
//                counter.  When a buffer fills, every row with half a buffer or more is
//                merged by its wave (the buffer sorted, then one bitonic merge stage with
//                the sorted list, 64-bit keys in registers) and its threshold raised.
//   topk_merge   top K of rows x n candidates given as values (+ indices) or as keys: one
//                wave per (row, chunk) keeps K best while the chunk streams past; long rows
//                are cut into chunks and the selections merged again (host loop).
//
// Order: (logit descending, index ascending), as ONE integer compare of the key
// (image << 32) | ~index, where image is order_key.h's tk_image: -0.0 folded onto +0.0 and
// every NaN sent to 1 (below -inf, above "none").
// Key 0 is "no candidate".  Integer compares only: the result is unique and does not
// depend on the order of execution.  No float atomics.
#include "inner_tile.h"
#include "tk_select.h"

namespace msha {

using namespace inner;
struct TkArgs {
  int64_t n_q, rows_q, ldq, ldt, n_cand, col_offset, per_split;
  const void* Q;
  const int64_t* qi;
  const void* T;
  const int32_t* excl_rowptr;
  const int32_t* excl_col;
  int F, K, sigmoid, splits;
  float* out_val;
  int64_t* out_idx;
  int32_t* err;
  u64* part;
};

// KP: list length (64 for K <= 64, else 128).  Query tile QT = 64 rows (KP 64) or 32 rows
// (KP 128); candidate tile 64.  Waves: QT 64 -> wave (w >> 1, w & 1) holds rows
// 32 (w >> 1) .. +31 and candidates 32 (w & 1) .. +31 of the tile; QT 32 -> every wave
// holds all 32 rows and candidates 16 w .. +15.  Per row in LDS: KP sorted keys + KP buffer.
template <typename T, int KP>
__global__ void __launch_bounds__(kThreads) topk_inner_kernel(TkArgs a) {
  constexpr int QT = KP <= 64 ? 64 : 32;
  constexpr int L = 2 * KP, CAP = KP, EPL = L / 64;
  constexpr int NC = QT == 64 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) unsigned char chunks[2 * kChunk];
  __shared__ u64 lists[QT * L];
  __shared__ u64 thr[QT];
  __shared__ int cnt[QT];
  __shared__ int state[QT];  // 0: past n_q, 1: live, 2: stray index (filler row)
  __shared__ int flag[3];    // the block-wide OR of a filter round, rotating

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int rb = QT == 64 ? (w >> 1) * 32 : 0;
  const int cb = QT == 64 ? (w & 1) * 32 : w * 16;
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int split = blockIdx.y;
  const Width wd = width<T>(a.F);

  for (int i = tid; i < QT * L; i += kThreads) lists[i] = 0ull;
  if (tid < QT) cnt[tid] = 0;
  if (tid < 3) flag[tid] = 0;
  int round = 0;

  // merge row's buffer into its sorted list (one wave), raise its threshold
  auto merge_row = [&](int row, u64 (&v)[EPL]) {
    const int m = min(cnt[row], CAP);
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const int e = r * 64 + lane;
      v[r] = e < KP + m ? lists[row * L + e] : 0ull;
    }
    tk_merge_top<EPL>(v, lane);
#pragma unroll
    for (int r = 0; r < EPL / 2; ++r) lists[row * L + r * 64 + lane] = v[r];
    const u64 kth = tk_kth<EPL>(v, a.K);
    if (lane == 0) {
      thr[row] = kth;
      cnt[row] = 0;
    }
  };

  // ---- the query tile: A operands, resident.  Validity is decided from qi[b] alone.
  uint4 areg[2][Geo<T>::NSTEP];
  int qst[2];
  load_queries<T>(areg, qst, a.Q, a.qi, a.rows_q, a.ldq, a.n_q, q0 + rb, wd.fbytes);
  if (g == 0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = rb + 16 * r + n;
      state[row] = qst[r];
      thr[row] = qst[r] == 1 ? 0ull : ~0ull;
      if (qst[r] == 2 && a.err != nullptr) atomicOr(a.err, 1);
    }
  }

  const Range rg = split_range(split, a.per_split, a.n_cand);
  const int64_t j_begin = rg.j_begin, j_end = rg.j_end, ntiles = rg.ntiles;
  const int64_t total = ntiles * wd.nch;

  // the streaming loop (its shape is rank_inner_kernel's: stage to LDS, one barrier, the next
  // stage's loads issued, the chunk's MFMAs under them)
  uint4 stg[4];
  auto load = [&](int64_t j0, int ch) {
    load_stage<T>(stg, a.T, a.ldt, wd.fbytes, [=](int c) { return j0 + c; }, j_end, ch);
  };
  if (total > 0) load(j_begin, 0);
  int64_t it_no = 0;

  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = j_begin + t * kCT;
    f32x4 acc[2][NC];
    zero_acc<NC>(acc);

#pragma unroll
    for (int ch = 0; ch < Geo<T>::NCH; ++ch) {
      if (ch < wd.nch) {
        unsigned char* img = chunks + (it_no & 1) * kChunk;
        store_stage(img, stg);
        __syncthreads();
        ++it_no;
        if (it_no < total) {
          if (ch + 1 < wd.nch) load(j0, ch + 1);
          else load(j0 + kCT, 0);
        }
        mma_chunk<T, NC>(acc, areg, img, ch, wd.nsteps, cb, n, g);
      }
    }

    // ---- filter: C/D layout col = lane & 15 (candidate), row = (lane >> 4) * 4 + reg
    unsigned pend = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rb + 16 * r + 4 * g + i;
          const int64_t j = j0 + cb + 16 * c + n;
          const u64 key = tk_key(acc[r][c][i], (uint32_t)j);
          if (j < j_end && key > thr[row]) pend |= 1u << ((r * NC + c) * 4 + i);
        }
    if (a.excl_rowptr != nullptr && pend != 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned bit = 1u << ((r * NC + c) * 4 + i);
            if (pend & bit) {
              const int64_t b = q0 + rb + 16 * r + 4 * g + i;
              const int32_t j = (int32_t)(j0 + cb + 16 * c + n);
              if (excluded(a.excl_rowptr, a.excl_col, b, j)) pend &= ~bit;
            }
          }
    }
    while (true) {
      int bits = 0;  // 1: an append found its row's buffer full; 2: a buffer filled up
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned bit = 1u << ((r * NC + c) * 4 + i);
            if (pend & bit) {
              const int row = rb + 16 * r + 4 * g + i;
              const int slot = atomicAdd(&cnt[row], 1);
              if (slot < CAP) {
                lists[row * L + KP + slot] =
                    tk_key(acc[r][c][i], (uint32_t)(j0 + cb + 16 * c + n));
                pend &= ~bit;
              }
              if (slot >= CAP - 1) bits |= 2;
            }
          }
      if (pend) bits |= 1;
      // the block's OR in one barrier: flag[round % 3]; the flag of the round before is
      // cleared for the round after next
      {
        const int wb = (__ballot(bits & 1) ? 1 : 0) | (__ballot(bits & 2) ? 2 : 0);
        if (lane == 0 && wb) atomicOr(&flag[round % 3], wb);
      }
      __syncthreads();
      const int any = flag[round % 3];
      if (tid == 0) flag[(round + 2) % 3] = 0;
      ++round;
      if (any & 2) {
        // every row with half a buffer or more merges now: merges are rare events that
        // stall the block, so each one takes all that is worth it.  Wave w owns the rows
        // with row % 4 == w (only it resets their counters, so its view of them is stable).
        const int c = lane < QT ? cnt[lane] : 0;
        u64 mask = __ballot(c >= CAP / 2) & (0x1111111111111111ull << w);
        while (mask) {
          const int row = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          u64 v[EPL];
          merge_row(row, v);
        }
      }
      if (!(any & 1)) break;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned bit = 1u << ((r * NC + c) * 4 + i);
            if (pend & bit) {
              const int row = rb + 16 * r + 4 * g + i;
              if (!(tk_key(acc[r][c][i], (uint32_t)(j0 + cb + 16 * c + n)) > thr[row]))
                pend &= ~bit;
            }
          }
    }
  }

  // ---- final merge of each row and the stores (ordinary vector stores)
  __syncthreads();
  for (int row = w; row < QT; row += kThreads / kWave) {
    const int st = state[row];
    if (st == 0) continue;
    const int64_t b = q0 + row;
    u64 v[EPL];
    if (st == 1) {
      merge_row(row, v);
    } else {
#pragma unroll
      for (int r = 0; r < EPL; ++r) v[r] = 0ull;
    }
#pragma unroll
    for (int r = 0; r < EPL / 2; ++r) {
      const int e = r * 64 + lane;
      if (e < a.K) {
        if (a.splits > 1) {
          a.part[(b * a.splits + split) * a.K + e] = v[r];
        } else {
          tk_emit(v[r], a.sigmoid, a.col_offset, a.out_val + b * a.K + e, a.out_idx + b * a.K + e);
        }
      }
    }
  }
}

struct TkMergeArgs {
  int64_t rows, n_in, chunk, nc;
  const u64* keys;      // keys of earlier selections, or NULL:
  const float* vals;    //   values and
  const int64_t* idx;   //   indices (NULL: the position in the row; < 0: no candidate)
  u64* out_keys;        // (rows, nc, K) selections, or NULL:
  float* out_val;       //   (rows, K) results (nc == 1)
  int64_t* out_idx;
  int K, sigmoid;
  int64_t col_offset;
};

// One wave per (row, chunk): registers hold KP best (sorted) + the next KP elements; a
// batch with nothing above the K-th best so far is skipped without sorting.
template <int KP>
__global__ void __launch_bounds__(kThreads) topk_merge_kernel(TkMergeArgs m) {
  constexpr int EPL = 2 * KP / 64, H = EPL / 2;
  const int lane = lane_id();
  const int64_t gw = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
  if (gw >= m.rows * m.nc) return;
  const int64_t row = gw / m.nc, c = gw % m.nc;
  const int64_t e0 = c * m.chunk, e1 = min(m.n_in, e0 + m.chunk);
  u64 v[EPL];
#pragma unroll
  for (int r = 0; r < EPL; ++r) v[r] = 0ull;
  u64 kth = 0ull;
  for (int64_t base = e0; base < e1; base += KP) {
    bool any = false;
#pragma unroll
    for (int r = 0; r < H; ++r) {
      const int64_t e = base + r * 64 + lane;
      u64 key = 0ull;
      if (e < e1) {
        const int64_t at = row * m.n_in + e;
        if (m.keys != nullptr) {
          key = m.keys[at];
        } else {
          const int64_t id = m.idx != nullptr ? m.idx[at] : e;
          if (id >= 0) key = tk_key(m.vals[at], (uint32_t)id);
        }
      }
      v[H + r] = key;
      any |= key > kth;
    }
    if (__ballot(any) == 0ull) continue;
    tk_merge_top<EPL>(v, lane);
    kth = tk_kth<EPL>(v, m.K);
  }
#pragma unroll
  for (int r = 0; r < H; ++r) {
    const int e = r * 64 + lane;
    if (e < m.K) {
      if (m.out_keys != nullptr) {
        m.out_keys[(row * m.nc + c) * m.K + e] = v[r];
      } else {
        tk_emit(v[r], m.sigmoid, m.col_offset, m.out_val + row * m.K + e, m.out_idx + row * m.K + e);
      }
    }
  }
}

// scratch of the hierarchical selection over rows x n_in elements: two key buffers
static size_t tk_merge_ws(int64_t rows, int64_t n_in, int k) {
  if (n_in <= kTkMergeChunk) return 0;
  const int64_t n1 = (n_in + kTkMergeChunk - 1) / kTkMergeChunk;
  size_t bytes = align256((size_t)rows * n1 * k * sizeof(u64));
  if (n1 * k > kTkMergeChunk) {
    const int64_t n2 = (n1 * k + kTkMergeChunk - 1) / kTkMergeChunk;
    bytes += align256((size_t)rows * n2 * k * sizeof(u64));
  }
  return bytes;
}

static void tk_merge_launch(const TkMergeArgs& m, hipStream_t s) {
  const int64_t waves = m.rows * m.nc;
  const dim3 grid((unsigned)((waves + 3) / 4));
  if (m.K <= 64)
    hipLaunchKernelGGL(topk_merge_kernel<64>, grid, dim3(kThreads), 0, s, m);
  else
    hipLaunchKernelGGL(topk_merge_kernel<128>, grid, dim3(kThreads), 0, s, m);
}

// Top K of rows x n_in elements (keys, or vals + idx) into out_val / out_idx: chunks of
// kTkMergeChunk are selected by one wave each, and the selections merged, until one wave
// per row finishes.  ws: tk_merge_ws bytes.
static void tk_merge_run(int64_t rows, int64_t n_in, int k, const u64* keys, const float* vals,
                         const int64_t* idx, int sigmoid, int64_t col_offset, float* out_val,
                         int64_t* out_idx, void* ws, hipStream_t s) {
  TkMergeArgs m;
  m.rows = rows;
  m.keys = keys;
  m.vals = vals;
  m.idx = idx;
  m.K = k;
  m.sigmoid = sigmoid;
  m.col_offset = col_offset;
  unsigned char* wb = reinterpret_cast<unsigned char*>(ws);
  u64* buf[2] = {nullptr, nullptr};
  if (n_in > kTkMergeChunk) {
    const int64_t n1 = (n_in + kTkMergeChunk - 1) / kTkMergeChunk;
    buf[0] = reinterpret_cast<u64*>(wb);
    buf[1] = reinterpret_cast<u64*>(wb + align256((size_t)rows * n1 * k * sizeof(u64)));
  }
  int flip = 0;
  while (n_in > kTkMergeChunk) {
    m.n_in = n_in;
    m.chunk = kTkMergeChunk;
    m.nc = (n_in + kTkMergeChunk - 1) / kTkMergeChunk;
    m.out_keys = buf[flip];
    m.out_val = nullptr;
    m.out_idx = nullptr;
    tk_merge_launch(m, s);
    m.keys = buf[flip];
    m.vals = nullptr;
    m.idx = nullptr;
    n_in = m.nc * k;
    flip ^= 1;
  }
  m.n_in = n_in;
  m.chunk = n_in > 0 ? n_in : 1;
  m.nc = 1;
  m.out_keys = nullptr;
  m.out_val = out_val;
  m.out_idx = out_idx;
  tk_merge_launch(m, s);
}

static bool tk_supported(int32_t feat, int32_t k, int32_t dtype) {
  return supported(feat, dtype) && k >= 1 && k <= kTkMaxK;
}

static int tk_default_splits(int64_t n_q, int64_t n_cand, int32_t k) {
  if (n_q <= 0 || n_cand <= 0) return 1;
  const int qt = k <= 64 ? 64 : 32;
  const int64_t tiles = (n_q + qt - 1) / qt;
  int64_t s = kCUs / tiles;               // one block per CU
  s = s < n_cand / 512 ? s : n_cand / 512;  // a split has at least 512 candidates
  return (int)(s < 1 ? 1 : s);
}

}  // namespace msha

using namespace msha;

extern "C" int msha_topk_inner_supported(int32_t feat, int32_t k, int32_t dtype) {
  return tk_supported(feat, k, dtype) ? 1 : 0;
}

extern "C" int msha_topk_inner_splits(int64_t n_q, int64_t n_cand, int32_t feat, int32_t k,
                                      int32_t dtype) {
  if (!tk_supported(feat, k, dtype)) return 1;
  return tk_default_splits(n_q, n_cand, k);
}

extern "C" size_t msha_topk_inner_workspace_size(int64_t n_q, int64_t n_cand, int32_t k,
                                                 int32_t splits) {
  if (n_q < 0 || n_cand < 0 || k < 1 || k > kTkMaxK) return 0;
  if (splits <= 0) splits = tk_default_splits(n_q, n_cand, k);
  size_t bytes = 256;
  if (splits > 1)
    bytes += align256((size_t)n_q * splits * k * sizeof(u64)) +
             tk_merge_ws(n_q, (int64_t)splits * k, k);
  return bytes;
}

extern "C" int msha_topk_inner(int64_t n_q, int32_t feat, int32_t dtype, const void* Q,
                               int64_t ldq, const int64_t* qi, int64_t rows_q, const void* T,
                               int64_t ldt, int64_t n_cand, int64_t col_offset,
                               const int32_t* excl_rowptr, const int32_t* excl_col, int32_t k,
                               int32_t sigmoid, int32_t splits, float* out_val, int64_t* out_idx,
                               int32_t* err, void* ws, size_t ws_bytes, msha_stream_t stream) {
  const int rc = check_tables("topk_inner", dtype, k >= 1 && k <= kTkMaxK, feat, n_q, n_cand,
                              rows_q, splits, excl_rowptr, excl_col,
                              out_val != nullptr && out_idx != nullptr, Q, ldq, qi, T, ldt);
  if (rc != MSHA_OK || n_q == 0) return rc;
  splits = clamp_splits(splits, tk_default_splits(n_q, n_cand, k), n_cand);
  const size_t part_bytes = splits > 1 ? align256((size_t)n_q * splits * k * sizeof(u64)) : 0;
  const size_t need = splits > 1 ? part_bytes + tk_merge_ws(n_q, (int64_t)splits * k, k) : 0;
  MSHA_ARG_CHECK(need == 0 || (ws != nullptr && ws_bytes >= need && ((uintptr_t)ws % 16) == 0),
                 "topk_inner: workspace too small (msha_topk_inner_workspace_size) or unaligned");
  const int qt = k <= 64 ? 64 : 32;
  const int64_t tiles = (n_q + qt - 1) / qt;
  MSHA_ARG_CHECK(tiles < ((int64_t)1 << 31), "topk_inner: too many queries");
  TkArgs a;
  a.n_q = n_q;
  a.rows_q = rows_q;
  a.ldq = ldq;
  a.ldt = ldt;
  a.n_cand = n_cand;
  a.col_offset = col_offset;
  a.per_split = per_split(n_cand, splits);
  a.Q = Q;
  a.qi = qi;
  a.T = T;
  a.excl_rowptr = excl_rowptr;
  a.excl_col = excl_col;
  a.F = feat;
  a.K = k;
  a.sigmoid = sigmoid;
  a.splits = splits;
  a.out_val = out_val;
  a.out_idx = out_idx;
  a.err = err;
  a.part = reinterpret_cast<u64*>(ws);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)tiles, (unsigned)splits);
  if (dtype == MSHA_DTYPE_BF16) {
    if (k <= 64)
      hipLaunchKernelGGL((topk_inner_kernel<bf16_t, 64>), grid, dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL((topk_inner_kernel<bf16_t, 128>), grid, dim3(kThreads), 0, s, a);
  } else {
    if (k <= 64)
      hipLaunchKernelGGL((topk_inner_kernel<float, 64>), grid, dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL((topk_inner_kernel<float, 128>), grid, dim3(kThreads), 0, s, a);
  }
  if (splits > 1)
    tk_merge_run(n_q, (int64_t)splits * k, k, a.part, nullptr, nullptr, sigmoid, col_offset,
                 out_val, out_idx, reinterpret_cast<unsigned char*>(ws) + part_bytes, s);
  return check_launch("topk_inner");
}

extern "C" size_t msha_topk_merge_workspace_size(int64_t rows, int64_t lists, int64_t len,
                                                 int32_t k) {
  if (rows < 0 || lists < 0 || len < 0 || k < 1 || k > kTkMaxK) return 0;
  return 256 + tk_merge_ws(rows, lists * len, k);
}

extern "C" int msha_topk_merge(int64_t rows, int64_t lists, int64_t len, int32_t k,
                               const float* vals, const int64_t* idx, int32_t sigmoid,
                               float* out_val, int64_t* out_idx, void* ws, size_t ws_bytes,
                               msha_stream_t stream) {
  MSHA_ARG_CHECK(k >= 1 && k <= kTkMaxK, "topk_merge: k must be in [1, 128]");
  MSHA_ARG_CHECK(rows >= 0 && lists >= 0 && len >= 0, "topk_merge: negative size");
  if (rows == 0) return MSHA_OK;
  MSHA_ARG_CHECK(lists == 0 || len == 0 || lists < ((int64_t)0xffffffff) / len,
                 "topk_merge: lists * len must stay below 2^32 - 1");
  const int64_t n_in = lists * len;
  MSHA_ARG_CHECK(out_val != nullptr && out_idx != nullptr && (vals != nullptr || n_in == 0),
                 "topk_merge: null pointer");
  MSHA_ARG_CHECK((rows + 3) / 4 * ((n_in + kTkMergeChunk - 1) / kTkMergeChunk + 1) <
                     ((int64_t)1 << 31),
                 "topk_merge: too many rows");
  const size_t need = tk_merge_ws(rows, n_in, k);
  MSHA_ARG_CHECK(need == 0 || (ws != nullptr && ws_bytes >= need && ((uintptr_t)ws % 16) == 0),
                 "topk_merge: workspace too small (msha_topk_merge_workspace_size) or unaligned");
  tk_merge_run(rows, n_in, k, nullptr, vals, idx, sigmoid, 0, out_val, out_idx, ws,
               (hipStream_t)stream);
  return check_launch("topk_merge");
}
