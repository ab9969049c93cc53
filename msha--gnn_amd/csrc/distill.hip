// Link-prediction distillation for the 'inner' scorer (LLP.py:231-238: a teacher-matching
// term beside the label loss): context sample -> plan -> fused loss -> table gradient, with
// no (A, K, F) array anywhere and no float atomics.
//
//   context_sample    K = walks * hops + n_rand context nodes per anchor: random-walk
//                     neighbours (one Philox word and one CSR load a step, -1 from a dead end
//                     on) and uniform nodes.  No rejection loop, nothing read back.
//   link_distill_fwd  a wave takes 64 / W anchors at a time (W = the power of two >= K, at
//                     least 8).  The anchor's row piece stays in registers; the context rows
//                     are gathered 64 / QP per wave-instruction, several in flight, and
//                     reduced by link_bce_fwd's own chain (pk_dot of the 16-byte pieces, xor
//                     tree over the row's lanes), so y is bitwise its z.  The logits cross a
//                     wave-private LDS row so that lane gi W + k holds (y_k, t_k) of the gi-th
//                     anchor; the softmax sums are xor trees over the W lanes (fp64: one
//                     rounding in g and in the terms) and the K-step pair loop reads slot j
//                     of the lane's own anchor.  A block owns a fixed tile of anchors; its
//                     partials are summed in a fixed order and one block adds the tiles'
//                     partials in order.
//   pair_grad_bwd     pair_grad.h with g loaded: link_bce_bwd's kernels, shared.
#include "common.h"
#include "pair_grad.h"

namespace msha {

typedef unsigned long long u64;

constexpr int kDsThreads = 256;
constexpr int kDsWaves = kDsThreads / kWave;
constexpr int kDsTile = 64;  // anchors per forward block (fixes the loss order)
constexpr int kDsFinThreads = 1024;
constexpr int kDsMaxK = 64;

// ------------------------------------------------------------- context_sample ----

// one thread per (anchor, walk) and per (anchor, random slot): U = walks + n_rand units
__global__ void __launch_bounds__(kDsThreads) ds_context_kernel(
    int64_t total, int U, int walks, int hops, int K, const int64_t* __restrict__ anchors,
    int64_t n_rows, uint32_t n_nodes, int64_t n_edges, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const uint8_t* __restrict__ rowflag, Dropout dp,
    int64_t* __restrict__ ctx) {
  const uint64_t off = dropout_offset(dp, dp.offset);
  for (int64_t t = (int64_t)blockIdx.x * kDsThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kDsThreads) {
    const int64_t a = t / U;
    const int u = (int)(t % U);
    const int64_t v0 = anchors[a];
    if (u < walks) {
      int64_t v = v0;
      for (int s = 0; s < hops; ++s) {
        const int slot = u * hops + s;
        int64_t nxt = -1;
        if ((uint64_t)v < (uint64_t)n_rows) {  // decided before any load through v
          const int64_t beg = rowptr[v];
          const int64_t deg = (int64_t)rowptr[v + 1] - beg;
          bool ok = beg >= 0 && deg > 0 && beg + deg <= n_edges;
          if (rowflag != nullptr && rowflag[v] != 0) ok = false;  // a virtual full row: no edges
          if (ok) {
            const uint32_t word = philox_x(dp.seed, off, (uint64_t)(a * K + slot));
            nxt = col[beg + mulhi32(word, (uint32_t)deg)];
            if (nxt < 0) nxt = -1;
          }
        }
        ctx[a * K + slot] = nxt;
        v = nxt;  // -1: outside every CSR, so the rest of the walk is -1
      }
    } else {
      const int slot = walks * hops + (u - walks);
      int64_t d = -1;
      if ((uint64_t)v0 < (uint64_t)n_rows)
        d = mulhi32(philox_x(dp.seed, off, (uint64_t)(a * K + slot)), n_nodes);
      ctx[a * K + slot] = d;
    }
  }
}

// ----------------------------------------------------------- link_distill_fwd ----

struct DsArgs {
  int64_t A, n, ld, n_t, t_ld;
  int K, F, Ft;
  const void *h, *th;  // th: the teacher table, or nullptr with teacher logits
  const int64_t *anchors, *ctx;
  const float* tl;
  float margin, tau, w_rank, w_dist, w_prob;
  float *logits, *g;
  double* part;  // (tiles, 4): L_R, L_D, L_P and the padding count
};

// <tab[a], tab[c_k]> of one anchor's valid slots into out[k] (an LDS row of this wave): lane
// l0 + k holds c_k; vm: the anchor's valid slots, bit k (a is inside the table when vm != 0)
template <typename T>
__device__ __forceinline__ void ds_dots(const T* __restrict__ tab, int64_t ld, int F, int64_t a,
                                        int64_t c, int l0, u64 vm, int K, float* out) {
  constexpr int V = Pk<T>::V;
  constexpr int UNROLL = 4;
  const int lane = lane_id();
  const int QP = F / V;     // lanes per row
  const int PPW = 64 / QP;  // rows per wave-instruction
  const int slot = lane / QP, q = lane % QP;
  if (vm == 0) return;
  const Pk<T> ha = pk_load(tab + a * ld + V * q);
  for (int k0 = 0; k0 < K; k0 += PPW * UNROLL) {
    float acc[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int k = k0 + u * PPW + slot;
      const int64_t ck = __shfl(c, (l0 + k) & (kWave - 1));
      const bool ok = k < K && ((vm >> (k & (kWave - 1))) & 1ull) != 0;
      // no branch around the load (the four stay in flight together): a padding slot reads
      // the anchor's own row, which is inside the table, and its product is dropped
      const float dot = pk_dot(ha, pk_load(tab + (ok ? ck : a) * ld + V * q));
      acc[u] = ok ? dot : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float v = acc[u];
      for (int o = 1; o < QP; o <<= 1) v += __shfl_xor(v, o);
      const int k = k0 + u * PPW + slot;
      if (q == 0 && k < K) out[k] = v;
    }
  }
}

// sigmoid(z) and sigmoid(-z) without cancellation at either end (fp64, as lb_grad)
__device__ __forceinline__ void ds_sigmoids(double z, double& sp, double& sn) {
  const double e = exp(-fabs(z));
  const double inv = 1.0 / (1.0 + e);
  sp = z >= 0.0 ? inv : e * inv;
  sn = z >= 0.0 ? e * inv : inv;
}

__device__ __forceinline__ double ds_wave_sum(double v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
// over an aligned group of W consecutive lanes (W a power of two)
__device__ __forceinline__ double ds_group_sum(double v, int W) {
  for (int o = 1; o < W; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float ds_group_max(float v, int W) {
  for (int o = 1; o < W; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// A wave takes G = 64 / W anchors at a time, W = the power of two >= K (at least 8): lane
// gi W + k holds slot k of the step's gi-th anchor, so the softmax block and the pair loop
// below run on K of every W lanes instead of K of 64.  The gather is per anchor, 64 / QP rows
// per instruction whatever K is.  The smooth terms are evaluated in fp64 from the fp32 logits:
// their sums and their part of g carry one fp32 rounding, at the store.
template <typename T, typename TT>
__global__ void __launch_bounds__(kDsThreads) ds_fwd_kernel(DsArgs a) {
  __shared__ float ys[kDsWaves][kWave];
  __shared__ float ts[kDsWaves][kWave];
  __shared__ double wsum[kDsWaves][3];
  __shared__ int wpad[kDsWaves];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int K = a.K;
  int W = 8;
  while (W < K) W <<= 1;
  const int G = kWave / W, gi = lane / W, kl = lane % W, l0 = gi * W;
  const u64 wmask = W == kWave ? ~0ull : (1ull << W) - 1ull;
  const int64_t base = (int64_t)blockIdx.x * kDsTile;
  const int count = (int)min((int64_t)kDsTile, a.A - base);
  const double inv_a = 1.0 / (double)a.A, inv_tau = 1.0 / (double)a.tau;
  const double wd = (double)a.w_dist * inv_tau, wp2 = 2.0 * (double)a.w_prob;
  double accR = 0.0, accD = 0.0, accP = 0.0;
  int npad = 0;
  // step s of the tile holds anchors s G .. s G + G - 1; the next step's indices and teacher
  // logits are loaded one step ahead
  int64_t an = -1, c = -1;
  float tl = 0.f;
  {
    const int i = wv * G + gi;
    if (i < count) {
      an = a.anchors[base + i];
      if (kl < K) {
        c = a.ctx[(base + i) * K + kl];
        if (a.tl != nullptr) tl = a.tl[(base + i) * K + kl];
      }
    }
  }
  for (int s = wv; s * G < count; s += kDsWaves) {
    const int i = s * G + gi;  // this lane's anchor of the tile
    const bool live = i < count && kl < K;
    const int64_t ai = base + i;
    int64_t an_next = -1, c_next = -1;
    float tl_next = 0.f;
    {
      const int i1 = (s + kDsWaves) * G + gi;
      if (i1 < count) {
        an_next = a.anchors[base + i1];
        if (kl < K) {
          c_next = a.ctx[(base + i1) * K + kl];
          if (a.tl != nullptr) tl_next = a.tl[(base + i1) * K + kl];
        }
      }
    }
    bool v = live && (uint64_t)an < (uint64_t)a.n && (uint64_t)c < (uint64_t)a.n;
    if (a.th != nullptr) v = v && (uint64_t)an < (uint64_t)a.n_t && (uint64_t)c < (uint64_t)a.n_t;
    const u64 vmask = __ballot(v);
    npad += (int)__popcll(__ballot(live && !v));
    for (int g = 0; g < G; ++g) {  // wave-uniform: one anchor's rows at a time
      const int64_t ag = __shfl(an, g * W);
      const u64 vm = (vmask >> (g * W)) & wmask;
      ds_dots<T>((const T*)a.h, a.ld, a.F, ag, c, g * W, vm, K, ys[wv] + g * W);
      if (a.th != nullptr)
        ds_dots<TT>((const TT*)a.th, a.t_ld, a.Ft, ag, c, g * W, vm, K, ts[wv] + g * W);
    }
    __builtin_amdgcn_wave_barrier();
    float y = ys[wv][lane];
    float t = a.th != nullptr ? ts[wv][lane] : tl;
    __builtin_amdgcn_wave_barrier();
    float gk = 0.f;
    if (vmask != 0) {
      if (!v) y = 0.f, t = 0.f;
      const double yd = (double)y, td = (double)t;
      // distribution term: p = softmax(t / tau), q = softmax(y / tau).  The shift is the
      // fp32 maximum of the anchor's logits (any common shift gives the same softmax; tau > 0).
      // A group without a valid slot computes on infinities; every use below is under v.
      const float ninf = -__builtin_inff();
      const double my = (double)ds_group_max(v ? y : ninf, W) * inv_tau;
      const double mt = (double)ds_group_max(v ? t : ninf, W) * inv_tau;
      const double ay = yd * inv_tau - my, at = td * inv_tau - mt;  // <= 0 on valid slots
      const double ey = v ? exp(ay) : 0.0, et = v ? exp(at) : 0.0;
      const double sy = ds_group_sum(ey, W), st = ds_group_sum(et, W);
      const double p = et * (1.0 / st), qs = ey * (1.0 / sy);
      // log p - log q = (at - log st) - (ay - log sy)
      const double ld = v ? p * ((at - ay) - log(st / sy)) : 0.0;
      // probability term: d = sigmoid(y) - sigmoid(t) from the small sides
      double spy, sny, spt, snt;
      ds_sigmoids(yd, spy, sny);
      ds_sigmoids(td, spt, snt);
      const double d = (yd >= 0.0 && td >= 0.0) ? snt - sny : spy - spt;
      const double lp = v ? d * d : 0.0;
      // rank term: lane (gi, k) against slot j of its own anchor.  With dt = t_k - t_j and dy
      // = y_k - y_j the pair's hinge argument margin - r dy is the same from either end, and
      // so is the count's sign: c_k -= r wherever the pair is active.  Each decision is one
      // fp32 subtraction and one compare (r dy is exact).
      int cnt = 0;
      float lr = 0.f;
      for (int j = 0; j < K; ++j) {
        const float yj = __shfl(y, l0 + j), tj = __shfl(t, l0 + j);
        const bool vj = ((vmask >> (l0 + j)) & 1ull) != 0;
        const float dt = t - tj;
        const float dy = y - yj;
        const float r = fabsf(dt) > a.margin ? (dt > 0.f ? 1.f : -1.f) : 0.f;
        const float arg = a.margin - r * dy;
        const bool on = v && vj && j != kl;
        if (on && r != 0.f && arg > 0.f) cnt -= (int)r;
        if (on && kl < j) lr += fmaxf(arg, 0.f);
      }
      if (v) {
        gk = (float)(((double)a.w_rank * (double)cnt + wd * (qs - p) + wp2 * d * (spy * sny)) *
                     inv_a);
        // per lane over the wave's steps in order; the lanes are added once, after the loop
        accR += (double)lr;
        accD += ld;
        accP += lp;
      }
    }
    if (live) {
      a.logits[ai * K + kl] = v ? y : __builtin_nanf("");
      a.g[ai * K + kl] = gk;
    }
    an = an_next;
    c = c_next;
    tl = tl_next;
  }
  accR = ds_wave_sum(accR);
  accD = ds_wave_sum(accD);
  accP = ds_wave_sum(accP);
  if (lane == 0) {
    wsum[wv][0] = accR;
    wsum[wv][1] = accD;
    wsum[wv][2] = accP;
    wpad[wv] = npad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int np = 0;
    for (int k = 0; k < kDsWaves; ++k) {
      s0 += wsum[k][0];
      s1 += wsum[k][1];
      s2 += wsum[k][2];
      np += wpad[k];
    }
    double* out = a.part + 4 * (int64_t)blockIdx.x;
    out[0] = s0;
    out[1] = s1;
    out[2] = s2;
    out[3] = (double)np;
  }
}

// the tiles' partials in a fixed order: thread t strides them, xor tree, waves ascending
__global__ void __launch_bounds__(kDsFinThreads) ds_final_kernel(
    int64_t nb, const double* __restrict__ part, double invA, float w_rank, float w_dist,
    float w_prob, float* __restrict__ loss, float* __restrict__ terms,
    int32_t* __restrict__ npad) {
  __shared__ double ws[kDsFinThreads / kWave][4];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, c = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kDsFinThreads) {
    s0 += part[4 * b];
    s1 += part[4 * b + 1];
    s2 += part[4 * b + 2];
    c += part[4 * b + 3];
  }
  s0 = ds_wave_sum(s0);
  s1 = ds_wave_sum(s1);
  s2 = ds_wave_sum(s2);
  c = ds_wave_sum(c);
  if (lane == 0) {
    ws[wv][0] = s0;
    ws[wv][1] = s1;
    ws[wv][2] = s2;
    ws[wv][3] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, k = 0.0;
    for (int i = 0; i < kDsFinThreads / kWave; ++i) {
      t0 += ws[i][0];
      t1 += ws[i][1];
      t2 += ws[i][2];
      k += ws[i][3];
    }
    t0 *= invA;
    t1 *= invA;
    t2 *= invA;
    terms[0] = (float)t0;
    terms[1] = (float)t1;
    terms[2] = (float)t2;
    loss[0] = (float)((double)w_rank * t0 + (double)w_dist * t1 + (double)w_prob * t2);
    npad[0] = (int32_t)k;
  }
}

// ------------------------------------------------------------- pair_grad_bwd ----

// the per-pair factor, loaded
struct DsLoadG {
  const float* g;
  bool ok() const { return g != nullptr; }
  __device__ __forceinline__ float at(int64_t p, float gl) const { return gl * g[p]; }
};

static int64_t ds_tiles(int64_t A) { return A > 0 ? (A + kDsTile - 1) / kDsTile : 1; }

template <typename T>
static void ds_fwd_launch(const DsArgs& a, int32_t t_dtype, hipStream_t s) {
  const dim3 grid((unsigned)ds_tiles(a.A)), blk(kDsThreads);
  if (a.th != nullptr && t_dtype == MSHA_DTYPE_BF16)
    hipLaunchKernelGGL((ds_fwd_kernel<T, bf16_t>), grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL((ds_fwd_kernel<T, float>), grid, blk, 0, s, a);
}

}  // namespace msha

using namespace msha;

extern "C" int msha_context_sample(int64_t n_anchors, int32_t walks, int32_t hops, int32_t n_rand,
                                   const int64_t* anchors, int64_t n_rows, int64_t n_nodes,
                                   int64_t n_edges, const int32_t* rowptr, const int32_t* col,
                                   const uint8_t* rowflag, uint64_t seed, uint64_t offset,
                                   int64_t* context, msha_stream_t stream) {
  MSHA_ARG_CHECK(n_anchors >= 0 && walks >= 0 && hops >= 0 && n_rand >= 0 && n_rows >= 0 &&
                     n_edges >= 0,
                 "context_sample: bad sizes (n_anchors, walks, hops, n_rand >= 0)");
  const int64_t K = (int64_t)walks * hops + n_rand;
  MSHA_ARG_CHECK(K >= 1 && K <= kDsMaxK,
                 "context_sample: K = walks * hops + n_rand must be in [1, 64]");
  MSHA_ARG_CHECK(n_rand == 0 || (n_nodes >= 1 && n_nodes < ((int64_t)1 << 31)),
                 "context_sample: n_nodes must be in [1, 2^31) with random slots");
  MSHA_ARG_CHECK(n_edges < ((int64_t)1 << 31), "context_sample: n_edges must be below 2^31");
  MSHA_ARG_CHECK(n_anchors * K < ((int64_t)1 << 40), "context_sample: too many draws");
  if (n_anchors == 0) return MSHA_OK;
  MSHA_ARG_CHECK(anchors && context && (walks * hops == 0 || (rowptr && (col || n_edges == 0))),
                 "context_sample: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Dropout dp = make_dropout(0.f, seed, offset, s);
  const int w = hops > 0 ? walks : 0;  // (walks of no step fill no slot)
  const int U = w + n_rand;
  const int64_t total = n_anchors * U;
  hipLaunchKernelGGL(ds_context_kernel, dim3(grid_for(total, kDsThreads, 1 << 16)),
                     dim3(kDsThreads), 0, s, total, U, w, (int)hops, (int)K, anchors, n_rows,
                     (uint32_t)n_nodes, n_edges, rowptr, col, rowflag, dp, context);
  return check_launch("context_sample");
}

extern "C" size_t msha_link_distill_fwd_workspace_size(int64_t n_anchors) {
  if (n_anchors < 0 || n_anchors > kPgMaxPairs) return 0;
  return pg_align((size_t)ds_tiles(n_anchors) * 32);
}

extern "C" int msha_link_distill_fwd(int64_t n_anchors, int32_t k, int32_t feat, int32_t dtype,
                                     const void* h, int64_t ld, int64_t n, const int64_t* anchors,
                                     const int64_t* context, const float* teacher_logits,
                                     const void* teacher, int32_t t_feat, int32_t t_dtype,
                                     int64_t t_ld, int64_t n_t, float margin, float tau,
                                     float w_rank, float w_dist, float w_prob, float* logits,
                                     float* g, float* loss, float* terms, int32_t* n_pad, void* ws,
                                     size_t ws_bytes, msha_stream_t stream) {
  MSHA_ARG_CHECK(k >= 2 && k <= kDsMaxK, "link_distill_fwd: K must be in [2, 64]");
  MSHA_ARG_CHECK(n_anchors >= 1 && n_anchors <= kPgMaxPairs / k,
                 "link_distill_fwd: bad sizes (n_anchors >= 1, n_anchors * K below 2^30)");
  int rc = pg_table_check("link_distill_fwd", n_anchors * k, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK((teacher_logits != nullptr) != (teacher != nullptr),
                 "link_distill_fwd: exactly one of teacher_logits and the teacher table");
  if (teacher != nullptr) {
    rc = pg_table_check("link_distill_fwd (teacher table)", n_anchors * k, t_feat, t_dtype,
                        teacher, t_ld, n_t);
    if (rc != MSHA_OK) return rc;
  }
  MSHA_ARG_CHECK(tau > 0.f && margin >= 0.f, "link_distill_fwd: tau > 0 and margin >= 0");
  MSHA_ARG_CHECK(anchors && context && logits && g && loss && terms && n_pad,
                 "link_distill_fwd: null pointer");
  const int64_t nb = ds_tiles(n_anchors);
  MSHA_ARG_CHECK(ws != nullptr && ws_bytes >= pg_align((size_t)nb * 32) &&
                     ((uintptr_t)ws % 16) == 0,
                 "link_distill_fwd: workspace too small or unaligned "
                 "(msha_link_distill_fwd_workspace_size)");
  hipStream_t s = (hipStream_t)stream;
  DsArgs a;
  a.A = n_anchors, a.n = n, a.ld = ld, a.n_t = n_t, a.t_ld = t_ld;
  a.K = k, a.F = feat, a.Ft = t_feat;
  a.h = h, a.th = teacher;
  a.anchors = anchors, a.ctx = context, a.tl = teacher_logits;
  a.margin = margin, a.tau = tau, a.w_rank = w_rank, a.w_dist = w_dist, a.w_prob = w_prob;
  a.logits = logits, a.g = g, a.part = (double*)ws;
  if (dtype == MSHA_DTYPE_BF16)
    ds_fwd_launch<bf16_t>(a, t_dtype, s);
  else
    ds_fwd_launch<float>(a, t_dtype, s);
  hipLaunchKernelGGL(ds_final_kernel, dim3(1), dim3(kDsFinThreads), 0, s, nb, (const double*)ws,
                     1.0 / (double)n_anchors, w_rank, w_dist, w_prob, loss, terms, n_pad);
  return check_launch("link_distill_fwd");
}

extern "C" size_t msha_pair_grad_bwd_workspace_size(int64_t n_pairs, int32_t feat) {
  if (n_pairs < 0 || n_pairs > kPgMaxPairs || feat < 1) return 0;
  return pg_workspace_bytes(n_pairs, feat);
}

extern "C" int msha_pair_grad_bwd(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                  int64_t ld, int64_t n, const int64_t* src, const int64_t* dst,
                                  const float* g, const float* gloss, const int32_t* plan_rowptr,
                                  const int32_t* plan_ent, const int32_t* plan_chunk_tab, float* dH,
                                  void* ws, size_t ws_bytes, msha_stream_t stream) {
  const int rc = pg_table_check("pair_grad_bwd", n_pairs, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  return pg_run("pair_grad_bwd", "msha_pair_grad_bwd_workspace_size", n_pairs, feat, dtype, h, ld,
                n, src, dst, plan_rowptr, plan_ent, plan_chunk_tab, DsLoadG{g}, gloss, dH, ws,
                ws_bytes, stream, PgAllRows{});
}

extern "C" int msha_pair_grad_bwd_rows(int64_t n_pairs, int32_t feat, int32_t dtype, const void* h,
                                       int64_t ld, int64_t n, const int64_t* src,
                                       const int64_t* dst, const float* g, const float* gloss,
                                       const int32_t* plan_rowptr, const int32_t* plan_ent,
                                       const int32_t* plan_chunk_tab, const int32_t* rows,
                                       const int32_t* n_rows, int64_t cap, float* vals, void* ws,
                                       size_t ws_bytes, msha_stream_t stream) {
  const int rc = pg_table_check("pair_grad_bwd_rows", n_pairs, feat, dtype, h, ld, n);
  if (rc != MSHA_OK) return rc;
  MSHA_ARG_CHECK(rows && n_rows, "pair_grad_bwd_rows: null pointer");
  MSHA_ARG_CHECK(cap == pg_rows_cap(n, n_pairs),
                 "pair_grad_bwd_rows: cap must be min(n, 2 * n_pairs) (msha_plan_rows)");
  return pg_run("pair_grad_bwd_rows", "msha_pair_grad_bwd_workspace_size", n_pairs, feat, dtype,
                h, ld, n, src, dst, plan_rowptr, plan_ent, plan_chunk_tab, DsLoadG{g}, gloss, vals,
                ws, ws_bytes, stream, PgListRows{rows, n_rows, cap});
}
