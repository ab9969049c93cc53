// Select over ragged segments (Explainer.py:25-34): for every segment [ptr[s], ptr[s + 1])
// of a per-slot value array, either the maximum and the slots that attain it (within a
// relative band), or the K best slots -- the attention explanation over the CSR rows and
// the CSC columns of the per-edge attention, without a dense (N, M) matrix.
//
//   slot value  x_t  = vals[(eid ? eid[t] : t) * ld + off]      (fp32; one head of attd)
//   slot id     id_t = ids ? ids[t] : t - ptr[s]                (col / csc_row)
//
// Order: topk.hip's -- (value descending, id ascending) through order_key.h's tk_image /
// tk_key: -0.0 folded onto +0.0, every NaN below -inf and all NaNs equal.  Integer compares
// and integer adds only, ordinary stores, no atomics: the results are unique and do not
// depend on the grid or on the chunk length.
//
// Two regimes, chosen per segment on the device from its length (no host sync):
//   short  len <= W: a group of W lanes per segment (W a power of two in [4, 64] picked by
//          the host from the mean length), 64 / W segments per wave instruction; maximum,
//          count and bitonic sort by xor shuffles inside the group.
//   long   len > W: cut into chunks of at most `chunk` (<= 4096) slots, one wave per
//          (segment, chunk).  The chunk list is a scan of the per-segment chunk counts
//          (sx_plan_kernel + int_scan.h); a wave finds its segment by binary search in it
//          (once a call, then kept per chunk), so the work is proportional to the slots.
//          Partial maxima / counts / K-lists go through the workspace and are combined in
//          chunk order by the wave of the segment's first chunk: each is read once.
//
// Tie mode is count -> scan -> emit: a slot's output position is tie_ptr[s] + the counts of
// the segment's earlier chunks + the prefix popcount of the wave's ballot, so tie_idx is in
// slot order.  Top-K reuses tk_select.h's wave network (tk_merge_top / tk_kth).
#include "int_scan.h"
#include "tk_select.h"

namespace msha {

constexpr int kSxThreads = 256;
constexpr int kSxWaves = kSxThreads / kWave;

struct SxArgs {
  int64_t n_seg, n_slots, n_vals, ld, off, max_chunks;
  const int32_t* ptr;
  const float* vals;
  const int32_t* eid;
  const int32_t* ids;
  int W, chunk, K;
  float rtol;
  int32_t* nchunk;     // (n_seg) chunks of each segment, 0 for a short one
  int32_t* cptr;       // (n_seg + 1) its exclusive scan
  int32_t* chunk_seg;  // (max_chunks) a chunk's segment
  uint32_t* part_max;  // (max_chunks) image of a chunk's maximum
  uint32_t* seg_img;   // (n_seg) image of a long segment's maximum
  int32_t* part_cnt;   // (max_chunks) a chunk's ties, then the ties of the segment's earlier chunks
  u64* part_keys;      // (max_chunks, K) a chunk's K best
  float* max_val;
  int32_t* n_tie;
  int32_t* tie_ptr;
  int32_t* tie_idx;
  float* out_val;
  int64_t* out_idx;
};

struct SxSeg {
  int64_t p0, p1;
};

// the segment's slot range, forced into [0, n_slots] and non-negative length
__device__ __forceinline__ SxSeg sx_seg(const SxArgs& a, int64_t s) {
  SxSeg g;
  const int64_t p0 = a.ptr[s], p1 = a.ptr[s + 1];
  g.p0 = min(max(p0, (int64_t)0), a.n_slots);
  g.p1 = min(max(p1, g.p0), a.n_slots);
  return g;
}

// a slot whose eid points outside vals reads as NaN (ranks last)
__device__ __forceinline__ float sx_val(const SxArgs& a, int64_t t) {
  const int64_t e = a.eid != nullptr ? (int64_t)a.eid[t] : t;
  if (e < 0 || e >= a.n_vals) return __builtin_nanf("");
  return a.vals[e * a.ld + a.off];
}
__device__ __forceinline__ int32_t sx_id(const SxArgs& a, int64_t t, int64_t p0) {
  return a.ids != nullptr ? a.ids[t] : (int32_t)(t - p0);
}

// image of the tie threshold of a segment whose maximum has image m: the maximum itself
// with rtol = 0 or a non-finite maximum, else max - rtol * |max| in fp32 (two roundings)
__device__ __forceinline__ uint32_t sx_thr(uint32_t m, float rtol) {
  if (m <= 1u || rtol == 0.f) return m;
  const float v = tk_value(m);
  if (!(fabsf(v) < __builtin_inff())) return m;
  return tk_image(__fsub_rn(v, __fmul_rn(rtol, fabsf(v))));
}
__device__ __forceinline__ float sx_maxval(uint32_t m) {
  if (m == 0u) return -__builtin_inff();
  if (m == 1u) return __uint_as_float(0x7fc00000u);
  return tk_value(m);
}

__device__ __forceinline__ uint32_t sx_wave_max(uint32_t m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)m, o);
    m = m > t ? m : t;
  }
  return m;
}
__device__ __forceinline__ int sx_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the long regime's chunks: as many as the plan counted (max_chunks is their upper bound)
__device__ __forceinline__ int64_t sx_chunks(const SxArgs& a) {
  return min((int64_t)a.cptr[a.n_seg], a.max_chunks);
}

// chunk c < sx_chunks of the long regime: its segment, its place j among the segment's nc
// chunks.  FIND: by binary search in the chunk list, and kept in chunk_seg (the first chunk
// kernel of a call); else read back from there
template <bool FIND>
__device__ __forceinline__ void sx_chunk(const SxArgs& a, int64_t c, int64_t* s, int* j, int* nc) {
  int64_t lo = 0;
  if (FIND) {
    int64_t hi = a.n_seg;  // cptr[lo] <= c < cptr[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.cptr[mid] <= c) lo = mid;
      else hi = mid;
    }
    if (lane_id() == 0) a.chunk_seg[c] = (int32_t)lo;
  } else {
    lo = min(max((int64_t)a.chunk_seg[c], (int64_t)0), a.n_seg - 1);
  }
  *s = lo;
  *j = (int)(c - a.cptr[lo]);
  *nc = a.cptr[lo + 1] - a.cptr[lo];
}

// the waves of a chunk kernel stride over the chunks: the grid is capped (sx_chunk_grid) and
// a wave past the counted chunks leaves at once
__device__ __forceinline__ int64_t sx_wave_id() {
  return (int64_t)blockIdx.x * kSxWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
__device__ __forceinline__ int64_t sx_wave_stride() { return (int64_t)gridDim.x * kSxWaves; }

__global__ void __launch_bounds__(kSxThreads) sx_plan_kernel(SxArgs a) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.n_seg;
       s += (int64_t)gridDim.x * blockDim.x) {
    const SxSeg g = sx_seg(a, s);
    const int64_t len = g.p1 - g.p0;
    a.nchunk[s] = len > a.W ? (int32_t)((len + a.chunk - 1) / a.chunk) : 0;
  }
}

// the lane group of a short segment: gl the lane in the group, len < 0 "not mine"
struct SxGroup {
  int64_t s, p0;
  int gl, len;
};
__device__ __forceinline__ SxGroup sx_group(const SxArgs& a) {
  SxGroup q;
  const int64_t gt = (int64_t)blockIdx.x * kSxThreads + threadIdx.x;
  q.s = gt / a.W;
  q.gl = (int)(threadIdx.x & (a.W - 1));
  q.p0 = 0;
  q.len = -1;
  if (q.s < a.n_seg) {
    const SxSeg g = sx_seg(a, q.s);
    q.p0 = g.p0;
    if (g.p1 - g.p0 <= a.W) q.len = (int)(g.p1 - g.p0);
  }
  return q;
}

// ---- tie mode, short segments.  EMIT = false: max_val and n_tie; true: tie_idx
template <bool EMIT>
__global__ void __launch_bounds__(kSxThreads) sx_short_ties_kernel(SxArgs a) {
  const SxGroup q = sx_group(a);
  const int W = a.W, lane = lane_id();
  const bool live = q.gl < q.len;
  const uint32_t img = live ? tk_image(sx_val(a, q.p0 + q.gl)) : 0u;
  uint32_t m = img;
  for (int o = 1; o < W; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)m, o);
    m = m > t ? m : t;
  }
  const bool tie = live && img >= sx_thr(m, a.rtol);
  const u64 b = __ballot(tie);
  const u64 gm = W == 64 ? b : (b >> (lane & ~(W - 1))) & ((1ull << W) - 1ull);
  if (!EMIT) {
    if (q.gl == 0 && q.len >= 0) {
      a.max_val[q.s] = sx_maxval(m);
      a.n_tie[q.s] = __popcll(gm);
    }
  } else if (tie) {
    const int64_t pos = (int64_t)a.tie_ptr[q.s] + __popcll(gm & ((1ull << q.gl) - 1ull));
    if (pos >= 0 && pos < a.n_slots) a.tie_idx[pos] = sx_id(a, q.p0 + q.gl, q.p0);
  }
}

// ---- tie mode, long segments: the image of each chunk's maximum
__global__ void __launch_bounds__(kSxThreads) sx_long_max_kernel(SxArgs a) {
  const int lane = lane_id();
  const int64_t n_chunks = sx_chunks(a);
  for (int64_t c = sx_wave_id(); c < n_chunks; c += sx_wave_stride()) {
    int64_t s;
    int j, nc;
    sx_chunk<true>(a, c, &s, &j, &nc);
    const SxSeg g = sx_seg(a, s);
    const int64_t b0 = g.p0 + (int64_t)j * a.chunk, b1 = min(g.p1, b0 + a.chunk);
    uint32_t m = 0u;
    for (int64_t t = b0 + lane; t < b1; t += kWave) {
      const uint32_t i = tk_image(sx_val(a, t));
      m = m > i ? m : i;
    }
    m = sx_wave_max(m);
    if (lane == 0) a.part_max[c] = m;
  }
}

// a long segment's maximum from its chunks', by the wave of its first chunk: every chunk's
// maximum is read once
__global__ void __launch_bounds__(kSxThreads) sx_seg_max_kernel(SxArgs a) {
  const int lane = lane_id();
  const int64_t n_chunks = sx_chunks(a);
  for (int64_t c = sx_wave_id(); c < n_chunks; c += sx_wave_stride()) {
    int64_t s;
    int j, nc;
    sx_chunk<false>(a, c, &s, &j, &nc);
    if (j != 0) continue;
    uint32_t m = 0u;
    for (int i = lane; i < nc && c + i < n_chunks; i += kWave) {
      const uint32_t t = a.part_max[c + i];
      m = m > t ? m : t;
    }
    m = sx_wave_max(m);
    if (lane == 0) {
      a.seg_img[s] = m;
      a.max_val[s] = sx_maxval(m);
    }
  }
}

// a chunk's ties against its segment's threshold: counted (EMIT = false) or written at
// tie_ptr[s] + the ties of the segment's earlier chunks (sx_finish_ties_kernel's prefix)
template <bool EMIT>
__global__ void __launch_bounds__(kSxThreads) sx_long_ties_kernel(SxArgs a) {
  const int lane = lane_id();
  const u64 below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int64_t n_chunks = sx_chunks(a);
  for (int64_t c = sx_wave_id(); c < n_chunks; c += sx_wave_stride()) {
    int64_t s;
    int j, nc;
    sx_chunk<false>(a, c, &s, &j, &nc);
    const SxSeg g = sx_seg(a, s);
    const uint32_t thr = sx_thr(a.seg_img[s], a.rtol);
    const int64_t base = EMIT ? (int64_t)a.tie_ptr[s] + a.part_cnt[c] : 0;
    const int64_t b0 = g.p0 + (int64_t)j * a.chunk, b1 = min(g.p1, b0 + a.chunk);
    int cnt = 0;
    for (int64_t t0 = b0; t0 < b1; t0 += kWave) {
      const int64_t t = t0 + lane;
      const bool tie = t < b1 && tk_image(sx_val(a, t)) >= thr;
      const u64 b = __ballot(tie);
      if (EMIT && tie) {
        const int64_t pos = base + cnt + __popcll(b & below);
        if (pos >= 0 && pos < a.n_slots) a.tie_idx[pos] = sx_id(a, t, g.p0);
      }
      cnt += __popcll(b);
    }
    if (!EMIT && lane == 0) a.part_cnt[c] = cnt;
  }
}

// n_tie of the long segments, and each chunk's count replaced by the ties of the segment's
// earlier chunks: the wave of a segment's first chunk scans the counts, 64 chunks a step
__global__ void __launch_bounds__(kSxThreads) sx_finish_ties_kernel(SxArgs a) {
  const int lane = lane_id();
  const int64_t n_chunks = sx_chunks(a);
  for (int64_t c = sx_wave_id(); c < n_chunks; c += sx_wave_stride()) {
    int64_t s;
    int j, nc;
    sx_chunk<false>(a, c, &s, &j, &nc);
    if (j != 0) continue;
    int run = 0;
    for (int i0 = 0; i0 < nc; i0 += kWave) {
      const bool mine = i0 + lane < nc && c + i0 + lane < n_chunks;
      const int t = mine ? a.part_cnt[c + i0 + lane] : 0;
      int incl = t;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
      }
      if (mine) a.part_cnt[c + i0 + lane] = run + incl - t;
      run += __shfl(incl, kWave - 1);
    }
    if (lane == 0) a.n_tie[s] = run;
  }
}

// ---- top-K, short segments: the group sorts its (at most W) keys
__global__ void __launch_bounds__(kSxThreads) sx_short_topk_kernel(SxArgs a) {
  const SxGroup q = sx_group(a);
  const int W = a.W;
  u64 key = 0ull;
  if (q.gl < q.len)
    key = tk_key(sx_val(a, q.p0 + q.gl), (uint32_t)sx_id(a, q.p0 + q.gl, q.p0));
  for (int k = 2; k <= W; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const u64 o = __shfl_xor(key, j);
      const bool up = (q.gl & k) == 0, lower = (q.gl & j) == 0;
      const u64 mx = key > o ? key : o, mn = key > o ? o : key;
      key = (lower == up) ? mx : mn;
    }
  if (q.len < 0) return;
  for (int e = q.gl; e < a.K; e += W)
    tk_emit(e == q.gl ? key : 0ull, 0, 0, a.out_val + q.s * a.K + e, a.out_idx + q.s * a.K + e);
}

// ---- top-K, long segments.  stage 0: one wave per (segment, chunk) keeps the K best of its
// slots -- a single-chunk segment is finished here, else the list goes to part_keys.
// stage 1: the wave of a several-chunk segment's first chunk selects from the segment's
// lists, in order.
// KP: list length (64 for K <= 64, else 128); the loop is topk.hip's topk_merge_kernel's.
template <int KP>
__global__ void __launch_bounds__(kSxThreads) sx_long_topk_kernel(SxArgs a, int stage) {
  constexpr int EPL = 2 * KP / 64, H = EPL / 2;
  const int lane = lane_id();
  const int64_t n_chunks = sx_chunks(a);
  for (int64_t c = sx_wave_id(); c < n_chunks; c += sx_wave_stride()) {
    int64_t s, e0, e1, p0 = 0;
    int j, nc;
    if (stage == 0) sx_chunk<true>(a, c, &s, &j, &nc);
    else sx_chunk<false>(a, c, &s, &j, &nc);
    if (stage == 0) {
      const SxSeg g = sx_seg(a, s);
      p0 = g.p0;
      e0 = g.p0 + (int64_t)j * a.chunk;
      e1 = min(g.p1, e0 + a.chunk);
    } else {
      if (j != 0 || nc < 2) continue;
      e0 = c * a.K;
      e1 = min(c + nc, a.max_chunks) * a.K;
    }
    const bool last = stage != 0 || nc == 1;
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
        if (e < e1)
          key = stage == 0 ? tk_key(sx_val(a, e), (uint32_t)sx_id(a, e, p0)) : a.part_keys[e];
        v[H + r] = key;
        any |= key > kth;
      }
      if (__ballot(any) == 0ull) continue;
      tk_merge_top<EPL>(v, lane);
      kth = tk_kth<EPL>(v, a.K);
    }
#pragma unroll
    for (int r = 0; r < H; ++r) {
      const int e = r * 64 + lane;
      if (e < a.K) {
        if (last) tk_emit(v[r], 0, 0, a.out_val + s * a.K + e, a.out_idx + s * a.K + e);
        else a.part_keys[c * a.K + e] = v[r];
      }
    }
  }
}

// ---- host side
static size_t sx_align(size_t x) { return (x + 255) & ~(size_t)255; }

// lane-group width of the short regime: the power of two in [4, 64] at or above twice the
// mean segment length
static int sx_width(int64_t n_seg, int64_t n_slots) {
  const int64_t twice = n_seg > 0 ? (2 * n_slots + n_seg - 1) / n_seg : 0;
  int w = 4;
  while (w < 64 && w < twice) w <<= 1;
  return w;
}

// an upper bound of the long regime's chunks: a long segment has more than W slots and
// ceil(len / chunk) <= len / chunk + 1 chunks
static int64_t sx_max_chunks(int64_t n_seg, int64_t n_slots, int w, int chunk) {
  const int64_t longs = std::min(n_seg, n_slots / (w + 1));
  return n_slots / chunk + longs + 1;
}

struct SxLayout {
  size_t nchunk, cptr, scan, chunk_seg, part_max, seg_img, part_cnt, part_keys, bytes;
};
static SxLayout sx_layout(int64_t n_seg, int64_t max_chunks, int k) {
  SxLayout l;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += sx_align(bytes);
    return here;
  };
  l.nchunk = take((size_t)(n_seg + 1) * sizeof(int32_t));
  l.cptr = take((size_t)(n_seg + 1) * sizeof(int32_t));
  l.scan = take(scan_ws_ints(n_seg) * sizeof(int32_t));
  l.chunk_seg = take((size_t)max_chunks * sizeof(int32_t));
  l.part_max = take((size_t)max_chunks * sizeof(uint32_t));
  l.seg_img = take((size_t)(n_seg + 1) * sizeof(uint32_t));
  l.part_cnt = take((size_t)max_chunks * sizeof(int32_t));
  l.part_keys = take((size_t)max_chunks * (size_t)k * sizeof(u64));
  l.bytes = at;
  return l;
}

// slots per wave of a long segment when the caller leaves it open.  Tie mode: 256 -- a wave
// walks its chunk three times (maximum, count, emit) in dependent 64-slot steps, so short
// chunks on many waves beat long ones.  Top-K: the power of two in [256, 4096] at or above
// sqrt(mean length x k), which balances a chunk's stream against the merge of a segment's
// chunk lists (len / chunk lists of k keys, one wave).
static int sx_chunk_of(int32_t chunk, int64_t n_seg, int64_t n_slots, int k) {
  if (chunk != 0) return chunk;
  if (k == 0) return 256;
  const double mean = n_seg > 0 ? (double)n_slots / (double)n_seg : 0.0;
  int c = 256;
  while (c < kTkMergeChunk && (double)c * (double)c < mean * k) c <<= 1;
  return c;
}

// the shared argument checks and the chunk plan (sx_plan_kernel + scan)
static int sx_prepare(const char* what, SxArgs& a, int64_t n_seg, int64_t n_slots,
                      const int32_t* ptr, const float* vals, int64_t n_vals, int64_t ld,
                      int64_t off, const int32_t* eid, const int32_t* ids, int32_t k,
                      int32_t chunk, void* ws, size_t ws_bytes, SxLayout* lay) {
  const std::string w(what);
  MSHA_ARG_CHECK(n_seg >= 0 && n_slots >= 0 && n_vals >= 0, w + ": negative size");
  MSHA_ARG_CHECK(n_seg < ((int64_t)1 << 31) - 1 && n_slots < ((int64_t)1 << 31) - 1,
                 w + ": n_seg and n_slots must stay below 2^31 - 1");
  MSHA_ARG_CHECK(chunk == 0 || (chunk >= 64 && chunk <= kTkMergeChunk),
                 w + ": chunk must be 0 (default) or in [64, 4096]");
  MSHA_ARG_CHECK(ptr != nullptr, w + ": null ptr");
  MSHA_ARG_CHECK(vals != nullptr || n_slots == 0, w + ": null vals");
  MSHA_ARG_CHECK(ld >= 1 && off >= 0 && off < ld, w + ": need 0 <= off < ld");
  MSHA_ARG_CHECK(eid != nullptr || n_vals >= n_slots,
                 w + ": without eid, vals needs a row per slot");
  a.n_seg = n_seg;
  a.n_slots = n_slots;
  a.n_vals = n_vals;
  a.ld = ld;
  a.off = off;
  a.ptr = ptr;
  a.vals = vals;
  a.eid = eid;
  a.ids = ids;
  a.W = sx_width(n_seg, n_slots);
  a.chunk = sx_chunk_of(chunk, n_seg, n_slots, k);
  a.K = k;
  a.max_chunks = sx_max_chunks(n_seg, n_slots, a.W, a.chunk);
  *lay = sx_layout(n_seg, a.max_chunks, k);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= lay->bytes && ((uintptr_t)ws % 16) == 0,
                 w + ": workspace too small (msha_segment_select_workspace_size) or unaligned");
  MSHA_ARG_CHECK((n_seg * a.W + kSxThreads - 1) / kSxThreads < ((int64_t)1 << 31),
                 w + ": too many segments");
  unsigned char* b = reinterpret_cast<unsigned char*>(ws);
  a.nchunk = reinterpret_cast<int32_t*>(b + lay->nchunk);
  a.cptr = reinterpret_cast<int32_t*>(b + lay->cptr);
  a.chunk_seg = reinterpret_cast<int32_t*>(b + lay->chunk_seg);
  a.part_max = reinterpret_cast<uint32_t*>(b + lay->part_max);
  a.seg_img = reinterpret_cast<uint32_t*>(b + lay->seg_img);
  a.part_cnt = reinterpret_cast<int32_t*>(b + lay->part_cnt);
  a.part_keys = reinterpret_cast<u64*>(b + lay->part_keys);
  return MSHA_OK;
}

static dim3 sx_seg_grid(int64_t n_seg) { return dim3((unsigned)grid_for(n_seg, kSxThreads, 8192)); }
static dim3 sx_group_grid(const SxArgs& a) {
  return dim3((unsigned)((a.n_seg * a.W + kSxThreads - 1) / kSxThreads));
}
// one wave per chunk up to kSxChunkBlocks blocks (twice what the device holds at once);
// beyond that the waves stride
constexpr int kSxChunkBlocks = 4096;
static dim3 sx_chunk_grid(const SxArgs& a) {
  return dim3((unsigned)grid_for(a.max_chunks, kSxWaves, kSxChunkBlocks));
}

}  // namespace msha

using namespace msha;

extern "C" size_t msha_segment_select_workspace_size(int64_t n_seg, int64_t n_slots, int32_t k,
                                                     int32_t chunk) {
  if (n_seg < 0 || n_slots < 0 || k < 0 || k > kTkMaxK) return 0;
  if (chunk != 0 && (chunk < 64 || chunk > kTkMergeChunk)) return 0;
  const int w = sx_width(n_seg, n_slots);
  return 256 + sx_layout(n_seg, sx_max_chunks(n_seg, n_slots, w, sx_chunk_of(chunk, n_seg, n_slots, k)), k)
                   .bytes;
}

extern "C" int msha_segment_ties(int64_t n_seg, int64_t n_slots, const int32_t* ptr,
                                 const float* vals, int64_t n_vals, int64_t ld, int64_t off,
                                 const int32_t* eid, const int32_t* ids, float rtol,
                                 int32_t chunk, float* max_val, int32_t* n_tie, int32_t* tie_ptr,
                                 int32_t* tie_idx, void* ws, size_t ws_bytes,
                                 msha_stream_t stream) {
  MSHA_ARG_CHECK(rtol >= 0.f && rtol < 1.f, "segment_ties: rtol must be in [0, 1)");
  MSHA_ARG_CHECK(max_val != nullptr && n_tie != nullptr && tie_ptr != nullptr &&
                     (tie_idx != nullptr || n_slots == 0),
                 "segment_ties: null output pointer");
  SxArgs a = {};
  SxLayout lay;
  const int rc = sx_prepare("segment_ties", a, n_seg, n_slots, ptr, vals, n_vals, ld, off, eid,
                            ids, 0, chunk, ws, ws_bytes, &lay);
  if (rc != MSHA_OK || n_seg == 0) return rc;
  a.rtol = rtol;
  a.max_val = max_val;
  a.n_tie = n_tie;
  a.tie_ptr = tie_ptr;
  a.tie_idx = tie_idx;
  int32_t* scan = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(ws) + lay.scan);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kSxThreads);
  hipLaunchKernelGGL(sx_plan_kernel, sx_seg_grid(n_seg), blk, 0, s, a);
  exclusive_scan(a.nchunk, n_seg, a.cptr, scan, s);
  hipLaunchKernelGGL(sx_short_ties_kernel<false>, sx_group_grid(a), blk, 0, s, a);
  hipLaunchKernelGGL(sx_long_max_kernel, sx_chunk_grid(a), blk, 0, s, a);
  hipLaunchKernelGGL(sx_seg_max_kernel, sx_chunk_grid(a), blk, 0, s, a);
  hipLaunchKernelGGL(sx_long_ties_kernel<false>, sx_chunk_grid(a), blk, 0, s, a);
  hipLaunchKernelGGL(sx_finish_ties_kernel, sx_chunk_grid(a), blk, 0, s, a);
  exclusive_scan(n_tie, n_seg, tie_ptr, scan, s);
  if (n_slots > 0) {
    hipLaunchKernelGGL(sx_short_ties_kernel<true>, sx_group_grid(a), blk, 0, s, a);
    hipLaunchKernelGGL(sx_long_ties_kernel<true>, sx_chunk_grid(a), blk, 0, s, a);
  }
  return check_launch("segment_ties");
}

extern "C" int msha_segment_topk(int64_t n_seg, int64_t n_slots, const int32_t* ptr,
                                 const float* vals, int64_t n_vals, int64_t ld, int64_t off,
                                 const int32_t* eid, const int32_t* ids, int32_t k, int32_t chunk,
                                 float* out_val, int64_t* out_idx, void* ws, size_t ws_bytes,
                                 msha_stream_t stream) {
  MSHA_ARG_CHECK(k >= 1 && k <= kTkMaxK, "segment_topk: k must be in [1, 128]");
  MSHA_ARG_CHECK(out_val != nullptr && out_idx != nullptr, "segment_topk: null output pointer");
  SxArgs a = {};
  SxLayout lay;
  const int rc = sx_prepare("segment_topk", a, n_seg, n_slots, ptr, vals, n_vals, ld, off, eid,
                            ids, k, chunk, ws, ws_bytes, &lay);
  if (rc != MSHA_OK || n_seg == 0) return rc;
  a.out_val = out_val;
  a.out_idx = out_idx;
  int32_t* scan = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(ws) + lay.scan);
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kSxThreads);
  hipLaunchKernelGGL(sx_plan_kernel, sx_seg_grid(n_seg), blk, 0, s, a);
  exclusive_scan(a.nchunk, n_seg, a.cptr, scan, s);
  hipLaunchKernelGGL(sx_short_topk_kernel, sx_group_grid(a), blk, 0, s, a);
  if (k <= 64) {
    hipLaunchKernelGGL(sx_long_topk_kernel<64>, sx_chunk_grid(a), blk, 0, s, a, 0);
    hipLaunchKernelGGL(sx_long_topk_kernel<64>, sx_chunk_grid(a), blk, 0, s, a, 1);
  } else {
    hipLaunchKernelGGL(sx_long_topk_kernel<128>, sx_chunk_grid(a), blk, 0, s, a, 0);
    hipLaunchKernelGGL(sx_long_topk_kernel<128>, sx_chunk_grid(a), blk, 0, s, a, 1);
  }
  return check_launch("segment_topk");
}
