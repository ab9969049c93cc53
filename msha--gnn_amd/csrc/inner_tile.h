// The streamed inner-product tile of topk.hip and rank.hip, in one place: a block keeps a
// tile of query rows resident as MFMA A operands in registers and streams its range of
// candidate rows through a double-buffered LDS image in 256-byte row chunks.  fp32 tables
// run the exact-f32 v_mfma_f32_16x16x4_f32, bf16 tables v_mfma_f32_16x16x32_bf16.
//
// The numerical contract: a logit z = sum_f Q[q, f] * T[j, f] is ONE accumulation chain,
// 64-byte steps of the row ascending and, in fp32, the four k-slices of a step ascending
// (mma_chunk).  The chain is fixed by f alone -- not by the tile, the wave, the block, the
// column split or the kernel -- so rank_inner's logits are topk_inner's, bit for bit, and a
// candidate row bytewise equal to a target row ties with it exactly.  Both kernels reach
// the MFMAs only through this header.
//
// Shared: the geometry, the query operands, the stage (load with a caller's row map, store),
// the MFMA step, the split range, the exclusion search and the host-side argument rules.
// The double-buffered loop that strings them together (store, barrier, next loads, MFMAs,
// epilogue) is written out in each kernel: hoisted into one template with the epilogue as a
// callable it computed the same bits, but the register allocator then moved the accumulators
// between VGPRs and AGPRs inside the loop (rank_inner fp32 +9..12 %, topk_inner +2..7 % on
// MI355X; profiles/inner_tile_ab).
#pragma once

#include "common.h"

namespace msha {
namespace inner {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kCT = 64;            // candidates per tile
constexpr int kChunkBytes = 256;   // bytes of a row staged at once: four 64-byte MFMA steps
constexpr int kPitch = 272;        // LDS pitch of a row chunk (16 B of padding)
constexpr int kChunk = kCT * kPitch;
constexpr int kCUs = 256;

template <typename T>
struct Geo {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int NSTEP = 256 * (int)sizeof(T) / 64;  // 64-byte steps of a 256-feature row
  static constexpr int NCH = NSTEP / 4;                    // 256-byte chunks of it
};

// a call's feature width in the tile's units
struct Width {
  int fbytes, nsteps, nch;
};
template <typename T>
__device__ __forceinline__ Width width(int F) {
  Width w;
  w.fbytes = F * (int)sizeof(T);
  w.nsteps = (w.fbytes + 63) / 64;
  w.nch = (w.nsteps + 3) / 4;
  return w;
}

// the candidates [j_begin, j_end) of a column split, in ntiles tiles
struct Range {
  int64_t j_begin, j_end, ntiles;
};
__device__ __forceinline__ Range split_range(int split, int64_t per_split, int64_t n_cand) {
  Range r;
  r.j_begin = (int64_t)split * per_split;
  r.j_end = min(n_cand, r.j_begin + per_split);
  r.ntiles = r.j_end > r.j_begin ? (r.j_end - r.j_begin + kCT - 1) / kCT : 0;
  return r;
}

// The A operands of a wave's 2 x 16 query positions b0 + 16 r + (lane & 15): query b is row
// qi[b] of Q (qi NULL: row b).  st[r]: 0 past n_q, 1 live, 2 stray index; only a live row
// is read, the others are zero rows.
template <typename T>
__device__ __forceinline__ void load_queries(uint4 (&areg)[2][Geo<T>::NSTEP], int (&st)[2],
                                             const void* Q, const int64_t* qi, int64_t rows_q,
                                             int64_t ldq, int64_t n_q, int64_t b0, int fbytes) {
  const unsigned char* Qb = reinterpret_cast<const unsigned char*>(Q);
  const int n = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int64_t b = b0 + 16 * r + n;
    int64_t qrow = -1;
    st[r] = 0;
    if (b < n_q) {
      qrow = qi != nullptr ? qi[b] : b;
      st[r] = 1;
      if ((uint64_t)qrow >= (uint64_t)rows_q) {
        qrow = -1;
        st[r] = 2;
      }
    }
#pragma unroll
    for (int s = 0; s < Geo<T>::NSTEP; ++s) {
      const int off = s * 64 + 16 * g;
      areg[r][s] = (qrow >= 0 && off < fbytes)
                       ? *reinterpret_cast<const uint4*>(Qb + qrow * ldq * (int64_t)sizeof(T) + off)
                       : make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// Stage chunk ch of a candidate tile: 64 rows x 256 bytes, 4 pieces of 16 bytes per thread.
// row_of(c) is the table row of the tile's candidate c; a row outside [0, row_end) is a zero
// row (one unsigned compare: a streamed tile's rows past its split's end, a gathered tile's
// -1 for "none").
template <typename T, typename RowOf>
__device__ __forceinline__ void load_stage(uint4 (&stg)[4], const void* Tp, int64_t ldt,
                                           int fbytes, RowOf row_of, int64_t row_end, int ch) {
  const unsigned char* Tb = reinterpret_cast<const unsigned char*>(Tp);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int p = threadIdx.x + kThreads * it;
    const int64_t j = row_of(p >> 4);
    const int off = ch * kChunkBytes + (p & 15) * 16;
    stg[it] = ((uint64_t)j < (uint64_t)row_end && off < fbytes)
                  ? *reinterpret_cast<const uint4*>(Tb + j * ldt * (int64_t)sizeof(T) + off)
                  : make_uint4(0u, 0u, 0u, 0u);
  }
}
__device__ __forceinline__ void store_stage(unsigned char* img, const uint4 (&stg)[4]) {
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int p = threadIdx.x + kThreads * it;
    *reinterpret_cast<uint4*>(img + (p >> 4) * kPitch + (p & 15) * 16) = stg[it];
  }
}

// The MFMAs of staged chunk ch: acc[r][c] += rows 16 r .. +15 of the wave's queries x
// candidates cb + 16 c .. +15 of the image (n = lane & 15, g = lane >> 4; C/D layout:
// col = n the candidate, row = 4 g + reg).  Steps ascending, fp32 k-slices ascending: the
// chain order of the header comment.
template <typename T, int NC>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[2][NC],
                                          const uint4 (&areg)[2][Geo<T>::NSTEP],
                                          const unsigned char* img, int ch, int nsteps, int cb,
                                          int n, int g) {
#pragma unroll
  for (int sl = 0; sl < 4; ++sl) {
    const int s = ch * 4 + sl;
    if (s < nsteps) {
      uint4 breg[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        breg[c] = *reinterpret_cast<const uint4*>(img + (cb + 16 * c + n) * kPitch + sl * 64 +
                                                  16 * g);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (Geo<T>::BF) {
            acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, areg[r][s]), __builtin_bit_cast(bf16x8, breg[c]),
                acc[r][c], 0, 0, 0);
          } else {
            const uint32_t av[4] = {areg[r][s].x, areg[r][s].y, areg[r][s].z, areg[r][s].w};
            const uint32_t bv[4] = {breg[c].x, breg[c].y, breg[c].z, breg[c].w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
              acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  __uint_as_float(av[i]), __uint_as_float(bv[i]), acc[r][c], 0, 0, 0);
          }
        }
    }
  }
}

template <int NC>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[2][NC]) {
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// first position in [lo, hi) of the ascending col whose entry is >= key (hi: none)
__device__ __forceinline__ int32_t lower_bound(const int32_t* col, int32_t lo, int32_t hi,
                                               int64_t key) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)col[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// is candidate j in the ascending exclusion row of query position b
__device__ __forceinline__ bool excluded(const int32_t* rowptr, const int32_t* col, int64_t b,
                                         int32_t j) {
  const int32_t end = rowptr[b + 1];
  const int32_t at = lower_bound(col, rowptr[b], end, j);
  return at < end && col[at] == j;
}

// ---------------------------------------------------------------------- host ----

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline bool supported(int32_t feat, int32_t dtype) {
  return feat >= 16 && feat <= 256 && feat % 16 == 0 &&
         (dtype == MSHA_DTYPE_F32 || dtype == MSHA_DTYPE_BF16);
}

// a call's split count: the entry point's default for 0, at most one split per tile
inline int32_t clamp_splits(int32_t splits, int32_t default_splits, int64_t n_cand) {
  if (splits == 0) splits = default_splits;
  const int64_t max_splits = n_cand > 0 ? (n_cand + kCT - 1) / kCT : 1;
  return splits > max_splits ? (int32_t)max_splits : splits;
}

// candidates per split: whole tiles
inline int64_t per_split(int64_t n_cand, int32_t splits) {
  const int64_t per = (n_cand + splits - 1) / splits;
  return (per + kCT - 1) / kCT * kCT;
}

// What msha_topk_inner and msha_rank_inner ask of their common arguments, in one order and
// with one set of texts behind the entry point's name.  k_ok and own_ptrs are the entry
// point's own conditions, checked at their place in that order.  n_q == 0 is MSHA_OK
// before any pointer is looked at: the caller returns then, too.
inline int check_tables(const char* name, int32_t dtype, bool k_ok, int32_t feat, int64_t n_q,
                        int64_t n_cand, int64_t rows_q, int32_t splits,
                        const int32_t* excl_rowptr, const int32_t* excl_col, bool own_ptrs,
                        const void* Q, int64_t ldq, const int64_t* qi, const void* T,
                        int64_t ldt) {
#define MSHA_INNER_CHECK(cond, text) \
  MSHA_ARG_CHECK(cond, std::string(name) + ": " + (text))
  MSHA_INNER_CHECK(dtype == MSHA_DTYPE_F32 || dtype == MSHA_DTYPE_BF16,
                   "dtype must be MSHA_DTYPE_F32 or MSHA_DTYPE_BF16");
  MSHA_INNER_CHECK(k_ok, "k must be in [1, 128]");
  MSHA_INNER_CHECK(feat >= 16 && feat <= 256 && feat % 16 == 0,
                   "feat must be a multiple of 16 in [16, 256]");
  MSHA_INNER_CHECK(n_q >= 0 && n_cand >= 0 && n_cand < (int64_t)0x7fffffff && rows_q >= 0,
                   "sizes must be non-negative, n_cand below 2^31 - 1");
  MSHA_INNER_CHECK(splits >= 0 && splits <= 65535, "splits must be in [0, 65535]");
  MSHA_INNER_CHECK((excl_rowptr == nullptr) == (excl_col == nullptr),
                   "excl_rowptr and excl_col go together");
  if (n_q == 0) return MSHA_OK;
  MSHA_INNER_CHECK(Q != nullptr && own_ptrs, "null pointer");
  MSHA_INNER_CHECK(T != nullptr || n_cand == 0, "null table");
  MSHA_INNER_CHECK(qi != nullptr || rows_q >= n_q, "rows_q below n_q without qi");
  const int64_t esz = dtype == MSHA_DTYPE_BF16 ? 2 : 4;
  MSHA_INNER_CHECK((ldq * esz) % 16 == 0 && (ldt * esz) % 16 == 0 && ldq >= feat &&
                       (ldt >= feat || n_cand == 0) && ((uintptr_t)Q % 16) == 0 &&
                       ((uintptr_t)T % 16) == 0,
                   "tables must be 16-byte aligned with a 16-byte row pitch >= feat");
#undef MSHA_INNER_CHECK
  return MSHA_OK;
}

}  // namespace inner
}  // namespace msha
