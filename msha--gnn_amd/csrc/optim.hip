// The optimizer step of train.py's loop (train.py:207 optim.Adam(lr 1e-3, weight_decay
// 5e-4); :232 optimizer.step()) as one launch over every parameter (include/msha_gnn.h
// msha_adam_step).  torch's fused multi-tensor Adam read each gradient the backward had
// written; here the feature dropout's backward (the only producer of Sfeatures' gradient,
// Ablation.py:296 / Ours.py:161) can be fused into the gradient read instead: the 5M-float
// gradient is never written or re-read.
//
// One thread owns 4 consecutive elements (16-B fp32 / 8-B bf16 pieces of every operand);
// each tensor gets its own range of blocks of a 1-D grid.  Arithmetic follows torch.optim.Adam's
// single-tensor step (grad + wd * p, lerp of the first moment, addcmul of the second,
// addcdiv with step_size = lr / bias_correction1), fp32 per element with the bias
// corrections in double from the step count, as torch computes them on the host.
#include "common.h"
#include "pair_grad.h"  // pg_width_ok: the row widths of the link losses

namespace msha {

constexpr int kAdamLeaves = 64;  // completion-ticket leaves (see adam_kernel's end)
constexpr int kAdamLine = 64;    // uint32 words per ticket counter: one 256-B line each

struct AdamBatch {
  msha_adam_tensor t[MSHA_MAX_ADAM];
  double lr, b1, b2, eps, wd;  // torch's Python-float hyperparameters
  int n;
  int first[MSHA_MAX_ADAM + 1];  // blocks [first[i], first[i+1]) update tensor i (1-D grid)
  uint32_t* ticket;     // completion ticket: top counter, then the leaves (workspace, zero between launches)
  const uint64_t* ctr;  // device replay counter (dropout offsets)
};

__device__ __forceinline__ float4 ad_ld4(const void* p, int dt, int64_t q) {
  if (dt == MSHA_DTYPE_BF16) {
    const uint2 w = reinterpret_cast<const uint2*>(p)[q];
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u),
                       __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u));
  }
  return reinterpret_cast<const float4*>(p)[q];
}
__device__ __forceinline__ void ad_st4(void* p, int dt, int64_t q, float4 v) {
  if (dt == MSHA_DTYPE_BF16)
    reinterpret_cast<uint2*>(p)[q] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
  else
    reinterpret_cast<float4*>(p)[q] = v;
}
__device__ __forceinline__ float ad_ld(const void* p, int dt, int64_t i) {
  return dt == MSHA_DTYPE_BF16 ? (float)reinterpret_cast<const bf16_t*>(p)[i]
                               : reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ void ad_st(void* p, int dt, int64_t i, float v) {
  if (dt == MSHA_DTYPE_BF16)
    reinterpret_cast<bf16_t*>(p)[i] = (bf16_t)v;
  else
    reinterpret_cast<float*>(p)[i] = v;
}

struct AdamScalars {
  float b1c, b2c, wd, step_size, bc2_sqrt, eps;  // b1c = 1 - beta1, b2c = 1 - beta2
  float b2;
};

// one element: returns the new (param, m, v)
__device__ __forceinline__ void adam_elem(const AdamScalars& a, float g, float& p, float& m,
                                          float& v) {
  g = fmaf(a.wd, p, g);                  // grad.add(param, alpha=wd)
  m = fmaf(a.b1c, g - m, m);             // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf(a.b2c, g * g, v * a.b2);      // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p - a.step_size * (m / denom);     // param.addcdiv_(exp_avg, denom, -step_size)
}

// bias corrections of step t (exact integer t) in double, as torch computes them on the
// host: beta ** t by squaring (<= 2 log2 t double multiplies, a few ulps)
__device__ __forceinline__ float2 adam_scalars(double lr, double b1, double b2, float t) {
  double p1 = 1.0, p2 = 1.0, s1 = b1, s2 = b2;
  for (uint32_t e = (uint32_t)t; e != 0; e >>= 1) {
    if (e & 1u) {
      p1 *= s1;
      p2 *= s2;
    }
    s1 *= s1;
    s2 *= s2;
  }
  return make_float2((float)(lr / (1.0 - p1)), (float)sqrt(1.0 - p2));
}
__device__ __forceinline__ float2 adam_scalars(const AdamBatch& b, float t) {
  return adam_scalars(b.lr, b.b1, b.b2, t);
}

// One launch (round 5 ran a one-block launch ahead of the update for the scalars: one more
// graph node, ~4 us).  Every thread reads its tensor's step count t - 1 and derives step t's
// scalars itself (as torch's capturable Adam adds 1 first); the last block to finish -- a
// completion ticket in the workspace, zero between launches -- advances every step count.
// The ticket is a relaxed atomic with no fence: each block's step read was consumed by its
// whole update before the block takes its ticket, and nothing else is published through
// it (a device-scope fence per block writes back L2: that form measured 102 us vs 25).
__global__ void __launch_bounds__(256) adam_kernel(AdamBatch b) {
  // the tensor of this block: first[ti] <= blockIdx.x < first[ti + 1] (binary search over
  // the <= 64 boundaries; every block works -- a 2-D grid sized by the largest tensor left
  // ~2k idle blocks per small tensor)
  const int bid = blockIdx.x;
  int lo = 0, hi = b.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b.first[mid] <= bid) lo = mid; else hi = mid;
  }
  const int ti = lo;
  const msha_adam_tensor& T = b.t[ti];
  const int dt = T.dtype;
  const float2 sc = adam_scalars(b, *T.step + 1.f);
  AdamScalars a;  // the scalars torch hands its fp32 kernels
  a.b1c = (float)(1.0 - b.b1);
  a.b2c = (float)(1.0 - b.b2);
  a.b2 = (float)b.b2;
  a.wd = (float)b.wd;
  a.eps = (float)b.eps;
  a.step_size = sc.x;
  a.bc2_sqrt = sc.y;
  Dropout d{};
  d.active = T.drop_p > 0.f;
  uint64_t off = 0;
  if (d.active) {
    d.seed = T.drop_seed;
    d.offset = T.drop_offset;
    d.ctr = b.ctr;
    const double th = (double)T.drop_p * 4294967296.0;
    d.threshold = T.drop_p >= 1.f ? 0xFFFFFFFFu : (uint32_t)(th > 4294967295.0 ? 4294967295.0 : th);
    d.scale = T.drop_p < 1.f ? (float)(1.0 / (1.0 - (double)T.drop_p)) : 0.f;
    off = dropout_offset(d, d.offset);
  }
  const int64_t nthr = (int64_t)(b.first[ti + 1] - b.first[ti]) * blockDim.x;
  const int64_t tid = (int64_t)(bid - b.first[ti]) * blockDim.x + threadIdx.x;
  const int64_t nq = T.n / 4;
  for (int64_t q = tid; q < nq; q += nthr) {
    float4 g = ad_ld4(T.grad, dt, q), p = ad_ld4(T.param, dt, q);
    float4 m = ad_ld4(T.exp_avg, dt, q), v = ad_ld4(T.exp_avg_sq, dt, q);
    if (d.active) {  // the fused dropout backward: msha_segments' flat mask of element 4q + k
      const uint4 w = philox4(d.seed, off, (uint64_t)q);
      g = make_float4(g.x * (w.x >= d.threshold ? d.scale : 0.f),
                      g.y * (w.y >= d.threshold ? d.scale : 0.f),
                      g.z * (w.z >= d.threshold ? d.scale : 0.f),
                      g.w * (w.w >= d.threshold ? d.scale : 0.f));
    }
    adam_elem(a, g.x, p.x, m.x, v.x);
    adam_elem(a, g.y, p.y, m.y, v.y);
    adam_elem(a, g.z, p.z, m.z, v.z);
    adam_elem(a, g.w, p.w, m.w, v.w);
    ad_st4(T.param, dt, q, p);
    ad_st4(T.exp_avg, dt, q, m);
    ad_st4(T.exp_avg_sq, dt, q, v);
  }
  for (int64_t e = 4 * nq + tid; e < T.n; e += nthr) {  // the < 4 tail elements
    float g = ad_ld(T.grad, dt, e), p = ad_ld(T.param, dt, e);
    float m = ad_ld(T.exp_avg, dt, e), v = ad_ld(T.exp_avg_sq, dt, e);
    if (d.active) {
      const uint4 w = philox4(d.seed, off, (uint64_t)e >> 2);
      const uint32_t x = (e & 3) == 0 ? w.x : (e & 3) == 1 ? w.y : (e & 3) == 2 ? w.z : w.w;
      g *= x >= d.threshold ? d.scale : 0.f;
    }
    adam_elem(a, g, p, m, v);
    ad_st(T.param, dt, e, p);
    ad_st(T.exp_avg, dt, e, m);
    ad_st(T.exp_avg_sq, dt, e, v);
  }
  // two-level completion ticket: 64 leaf counters (a 256-B line each) and one top
  // counter -- same-address atomics serialise at the memory side, so 2048 blocks on one
  // counter added ~18 us; here no counter sees more than 64
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t leaf = blockIdx.x & (kAdamLeaves - 1);
    const uint32_t in_leaf = (gridDim.x - leaf + kAdamLeaves - 1) / kAdamLeaves;
    const uint32_t leaves = min(gridDim.x, (uint32_t)kAdamLeaves);
    uint32_t* lc = b.ticket + (1 + leaf) * kAdamLine;
    int last = 0;
    if (__hip_atomic_fetch_add(lc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_leaf - 1) {
      *lc = 0u;  // every block of this leaf has counted
      last = __hip_atomic_fetch_add(b.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             leaves - 1;
    }
    s_last = last;
  }
  __syncthreads();
  if (s_last) {
    const bool own = (int)threadIdx.x < b.n;
    const float t = own ? *b.t[threadIdx.x].step + 1.f : 0.f;
    __syncthreads();  // every count read before any is written (tensors may share one)
    if (own) *b.t[threadIdx.x].step = t;
    if (threadIdx.x == 0) *b.ticket = 0u;
  }
}

// ---- lazy Adam over the touched rows of a table (msha_adam_rows_step): the update above at
// weight_decay 0, for the rows of a list (msha_plan_rows) only, the gradient of list entry i
// in the fp32 row vals[i] (msha_link_bce_bwd_rows).  A lane group of F * esz / 16 lanes owns a
// row, 16 bytes of every operand per lane; rows outside the list are neither read nor
// written.  One step count for the whole table: every lane group reads it, and a trailing
// one-thread launch advances it (stream order: after every read).
struct AdamRows {
  void *param, *exp_avg, *exp_avg_sq;
  float* step;
  const int32_t *rows, *n_rows;
  const float* vals;
  int64_t n, cap;
  int F, dt;
  double lr, b1, b2, eps;
};

// the gradient a bf16 table's dense path sees: the fp32 sum rounded once to bf16
__device__ __forceinline__ float ad_round(int dt, float x) {
  return dt == MSHA_DTYPE_BF16 ? (float)(bf16_t)x : x;
}

// 8 bf16 elements, one 16-byte piece (ad_ld4 / ad_st4 twice over, in one memory operation)
__device__ __forceinline__ void ad_ld8(const void* p, int64_t q, float (&x)[8]) {
  const uint4 w = reinterpret_cast<const uint4*>(p)[q];
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x[2 * k] = __uint_as_float(u[k] << 16);
    x[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
  }
}
__device__ __forceinline__ void ad_st8(void* p, int64_t q, const float (&x)[8]) {
  reinterpret_cast<uint4*>(p)[q] = make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]),
                                              pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7]));
}

__global__ void __launch_bounds__(256) adam_rows_kernel(AdamRows b) {
  const int dt = b.dt;
  const int np = dt == MSHA_DTYPE_BF16 ? 2 : 1;  // 4-element pieces in a lane's 16 bytes
  const int F4 = b.F / 4, G = F4 / np;           // G: lanes per row, a power of two <= 64
  const int64_t c = b.n_rows[0];
  const int64_t cnt = c < 0 ? 0 : c > b.cap ? b.cap : c;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
  const int q = (int)(tid % G);
  if (tid / G >= cnt) return;
  const float2 sc = adam_scalars(b.lr, b.b1, b.b2, *b.step + 1.f);
  AdamScalars a;
  a.b1c = (float)(1.0 - b.b1);
  a.b2c = (float)(1.0 - b.b2);
  a.b2 = (float)b.b2;
  a.wd = 0.f;
  a.eps = (float)b.eps;
  a.step_size = sc.x;
  a.bc2_sqrt = sc.y;
  const float4* vals = reinterpret_cast<const float4*>(b.vals);
  for (int64_t i = tid / G; i < cnt; i += ngroups) {
    const int64_t r = b.rows[i];
    if ((uint64_t)r >= (uint64_t)b.n) continue;  // (not a list of this table: no stray access)
    if (dt == MSHA_DTYPE_BF16) {  // 8 elements: one 16-byte piece of p, m, v, two of vals
      const int64_t qt = r * G + q;
      const float4 g0 = vals[i * F4 + 2 * q], g1 = vals[i * F4 + 2 * q + 1];
      float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      float p[8], m[8], v[8];
      ad_ld8(b.param, qt, p);
      ad_ld8(b.exp_avg, qt, m);
      ad_ld8(b.exp_avg_sq, qt, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) adam_elem(a, ad_round(dt, g[k]), p[k], m[k], v[k]);
      ad_st8(b.param, qt, p);
      ad_st8(b.exp_avg, qt, m);
      ad_st8(b.exp_avg_sq, qt, v);
    } else {
      const int64_t qt = r * F4 + q;
      const float4 g = vals[i * F4 + q];
      float4 p = ad_ld4(b.param, dt, qt);
      float4 m = ad_ld4(b.exp_avg, dt, qt), v = ad_ld4(b.exp_avg_sq, dt, qt);
      adam_elem(a, g.x, p.x, m.x, v.x);
      adam_elem(a, g.y, p.y, m.y, v.y);
      adam_elem(a, g.z, p.z, m.z, v.z);
      adam_elem(a, g.w, p.w, m.w, v.w);
      ad_st4(b.param, dt, qt, p);
      ad_st4(b.exp_avg, dt, qt, m);
      ad_st4(b.exp_avg_sq, dt, qt, v);
    }
  }
}

__global__ void adam_rows_tick_kernel(float* step) { *step = *step + 1.f; }

// ---- lazy Adam that replays the steps a row missed (msha_adam_rows_replay): the dense
// update, weight decay included, at the cost of the rows a batch names.  Adam is elementwise:
// a row that no batch named for k steps has, under the dense optimizer, taken k updates with
// gradient +0.0 (plus wd * p).  row_step[r] records the step after which row r's p, m, v in
// memory are valid; a lane group that names r reads the row once, applies adam_elem with
// g = +0.0 for every missed step t with step t's own scalars (adam_scalars(t): the bits the
// dense kernel derived at step t), then the current step's gradient if there is one, and
// writes the row once.  bf16 rows pass through bf16 after every replayed step, as the dense
// kernel's store and reload do.
//
// The scalars of a step cost more than a lane's 4 or 8 element updates (a double power by
// squaring, a divide, a square root), so a block shares them: per pass it finds the span of
// steps its rows miss (a min / max over the block through shuffles and LDS, no atomics) and
// walks it in windows of 256 steps, thread k filling step w0 + k's scalars, every lane group
// reading the ones it needs.  All loop bounds around a barrier are block-uniform.
struct AdamReplay {
  void *param, *exp_avg, *exp_avg_sq;
  float* step;
  int32_t* row_step;
  const int32_t *rows, *n_rows;
  const float* vals;
  int64_t n, cap;
  int F, max_steps;
  double lr, b1, b2, eps, wd;
};

constexpr int kReplayWindow = 256;  // steps whose scalars a block holds at a time (= block size)

template <bool BF>
__device__ __forceinline__ void rp_ld(const void* p, int64_t q, float (&x)[BF ? 8 : 4]) {
  if constexpr (BF) {
    ad_ld8(p, q, x);
  } else {
    const float4 w = reinterpret_cast<const float4*>(p)[q];
    x[0] = w.x, x[1] = w.y, x[2] = w.z, x[3] = w.w;
  }
}
template <bool BF>
__device__ __forceinline__ void rp_st(void* p, int64_t q, const float (&x)[BF ? 8 : 4]) {
  if constexpr (BF)
    ad_st8(p, q, x);
  else
    reinterpret_cast<float4*>(p)[q] = make_float4(x[0], x[1], x[2], x[3]);
}
// what a bf16 store and reload leave of a lane's 8 values
__device__ __forceinline__ void rp_through_bf16(float (&x)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t u = pack_bf16x2(x[2 * k], x[2 * k + 1]);
    x[2 * k] = __uint_as_float(u << 16);
    x[2 * k + 1] = __uint_as_float(u & 0xffff0000u);
  }
}

template <bool BF>
__global__ void __launch_bounds__(256) adam_replay_kernel(AdamReplay b) {
  constexpr int V = BF ? 8 : 4;  // elements in a lane's 16 bytes
  constexpr int dt = BF ? MSHA_DTYPE_BF16 : MSHA_DTYPE_F32;
  __shared__ float2 s_win[kReplayWindow];
  __shared__ int s_lo[4], s_hi[4];
  const int G = b.F / V;      // lanes per row, a power of two <= 64: a group lies in one wave
  const int rpb = 256 / G;    // rows of a block per pass
  int64_t cnt = b.n;
  if (b.rows != nullptr) {
    const int64_t c = b.n_rows[0];
    cnt = c < 0 ? 0 : c > b.cap ? b.cap : c;
  }
  int64_t base = (int64_t)blockIdx.x * rpb;
  if (base >= cnt) return;  // (the whole block)
  const int T = (int)*b.step;  // completed steps
  const int lg = (int)threadIdx.x / G, q = (int)threadIdx.x % G;
  AdamScalars a;
  a.b1c = (float)(1.0 - b.b1);
  a.b2c = (float)(1.0 - b.b2);
  a.b2 = (float)b.b2;
  a.wd = (float)b.wd;
  a.eps = (float)b.eps;
  float2 sc_next = make_float2(0.f, 0.f);  // step T + 1's, for the gradient
  if (b.vals != nullptr) sc_next = adam_scalars(b.lr, b.b1, b.b2, (float)T + 1.f);
  // a zero-gradient step leaves an element with m = v = +0 as it is when nothing decays it
  const bool rest_ok = a.wd == 0.f && a.eps > 0.f;
  const float4* vals = reinterpret_cast<const float4*>(b.vals);
  const int64_t stride = (int64_t)gridDim.x * rpb;
  for (; base < cnt; base += stride) {
    const int64_t i = base + lg;
    int64_t r = -1;
    if (i < cnt) {
      r = b.rows != nullptr ? (int64_t)b.rows[i] : i;
      if ((uint64_t)r >= (uint64_t)b.n) r = -1;  // (not a list of this table: no stray access)
    }
    int rs = 0, end = 0;
    bool take = false;
    if (r >= 0) {
      rs = b.row_step[r];  // every lane of the group, before lane 0 writes it below
      const int64_t e = (int64_t)rs + b.max_steps;
      end = e < (int64_t)T ? (int)e : T;
      if (end < rs) end = rs;
      take = b.vals != nullptr && end >= T;
    }
    const bool gap = r >= 0 && end > rs;
    const int64_t qt = r * G + q;
    float p[V], m[V], v[V];
    bool replay = false;
    if (gap || take) {
      rp_ld<BF>(b.param, qt, p);
      rp_ld<BF>(b.exp_avg, qt, m);
      rp_ld<BF>(b.exp_avg_sq, qt, v);
      replay = gap;
      if (gap && rest_ok) {
        bool rest = true;
#pragma unroll
        for (int k = 0; k < V; ++k)
          rest = rest && __float_as_uint(m[k]) == 0u && __float_as_uint(v[k]) == 0u &&
                 fabsf(p[k]) < __builtin_inff();
        replay = !rest;
      }
    }
    // the block's span of missed steps
    int lo = replay ? rs + 1 : 0x7fffffff, hi = replay ? end : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o));
      hi = max(hi, __shfl_xor(hi, o));
    }
    __syncthreads();  // the last pass has read s_lo / s_hi
    if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
    __syncthreads();
    const int blo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
    const int bhi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    for (int w0 = blo; w0 <= bhi; w0 += kReplayWindow) {
      __syncthreads();  // the last window has been read
      if (w0 + (int)threadIdx.x <= bhi)
        s_win[threadIdx.x] = adam_scalars(b.lr, b.b1, b.b2, (float)(w0 + (int)threadIdx.x));
      __syncthreads();
      if (replay) {
        const int t1 = min(end, w0 + kReplayWindow - 1);
        for (int t = max(rs + 1, w0); t <= t1; ++t) {
          const float2 sc = s_win[t - w0];
          a.step_size = sc.x;
          a.bc2_sqrt = sc.y;
#pragma unroll
          for (int k = 0; k < V; ++k) adam_elem(a, 0.f, p[k], m[k], v[k]);
          if constexpr (BF) {
            rp_through_bf16(p);
            rp_through_bf16(m);
            rp_through_bf16(v);
          }
        }
      }
    }
    if (take) {  // the row stands at step T: step T + 1 with its gradient row
      a.step_size = sc_next.x;
      a.bc2_sqrt = sc_next.y;
      float g[V];
#pragma unroll
      for (int j = 0; j < V / 4; ++j) {
        const float4 w = vals[(i * b.F + q * V) / 4 + j];
        g[4 * j] = w.x, g[4 * j + 1] = w.y, g[4 * j + 2] = w.z, g[4 * j + 3] = w.w;
      }
#pragma unroll
      for (int k = 0; k < V; ++k) adam_elem(a, ad_round(dt, g[k]), p[k], m[k], v[k]);
    }
    if (replay || take) {
      rp_st<BF>(b.param, qt, p);
      rp_st<BF>(b.exp_avg, qt, m);
      rp_st<BF>(b.exp_avg_sq, qt, v);
    }
    if ((gap || take) && q == 0) b.row_step[r] = take ? T + 1 : end;
  }
}

}  // namespace msha

using namespace msha;

extern "C" int msha_adam_step(int32_t n, const msha_adam_tensor* tensors, double lr,
                              double beta1, double beta2, double eps, double weight_decay,
                              void* ws, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 0 && n <= MSHA_MAX_ADAM && (n == 0 || tensors != nullptr),
                 "adam_step: 0..MSHA_MAX_ADAM tensors");
  MSHA_ARG_CHECK(ws != nullptr, "adam_step: needs the msha_adam_workspace_size() workspace");
  MSHA_ARG_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                 "adam_step: bad hyperparameters");
  if (n == 0) return MSHA_OK;
  AdamBatch b{};
  int nblocks = 0;
  for (int i = 0; i < n; ++i) {
    const msha_adam_tensor& t = tensors[i];
    MSHA_ARG_CHECK(t.param && t.grad && t.exp_avg && t.exp_avg_sq && t.step && t.n >= 0,
                   "adam_step: null pointer / bad size");
    MSHA_ARG_CHECK(t.dtype == MSHA_DTYPE_F32 || t.dtype == MSHA_DTYPE_BF16,
                   "adam_step: dtype must be MSHA_DTYPE_F32 or MSHA_DTYPE_BF16");
    MSHA_ARG_CHECK(t.drop_p >= 0.f && t.drop_p <= 1.f, "adam_step: drop_p must be in [0, 1]");
    const uintptr_t am = t.dtype == MSHA_DTYPE_BF16 ? 7 : 15;
    MSHA_ARG_CHECK((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg |
                     (uintptr_t)t.exp_avg_sq) & am) == 0,
                   "adam_step: operands must be aligned to 4 elements");
    b.t[i] = t;
    b.first[i] = nblocks;
    nblocks += grid_for(t.n, 256 * 4, 2048);  // 4 elements per thread, grid-stride past 2048
  }
  b.first[n] = nblocks;
  b.lr = lr;
  b.b1 = beta1;
  b.b2 = beta2;
  b.eps = eps;
  b.wd = weight_decay;
  b.n = n;
  hipStream_t s = (hipStream_t)stream;
  b.ctr = rng_counter(s);
  b.ticket = (uint32_t*)ws;
  hipLaunchKernelGGL(adam_kernel, dim3(nblocks), dim3(256), 0, s, b);
  return check_launch("adam_step");
}

extern "C" int msha_adam_rows_step(int64_t n, int32_t feat, int32_t dtype, void* param,
                                   void* exp_avg, void* exp_avg_sq, float* step,
                                   const int32_t* rows, const int32_t* n_rows, int64_t cap,
                                   const float* vals, double lr, double beta1, double beta2,
                                   double eps, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 1 && n < ((int64_t)1 << 31) - 1,
                 "adam_rows_step: bad sizes (1 <= n < 2^31 - 1)");
  MSHA_ARG_CHECK(pg_width_ok(feat, dtype),
                 "adam_rows_step: unsupported width: feat must be a power of two in [16 B, "
                 "64 lanes x 16 B] of an fp32 or bf16 table (msha_link_bce_supported)");
  MSHA_ARG_CHECK(cap >= 1 && cap <= n, "adam_rows_step: cap must be in [1, n] (msha_plan_rows)");
  MSHA_ARG_CHECK(param && exp_avg && exp_avg_sq && step && rows && n_rows && vals,
                 "adam_rows_step: null pointer");
  MSHA_ARG_CHECK((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
                   (uintptr_t)vals) & 15) == 0,
                 "adam_rows_step: the table, its moments and vals must be 16-byte aligned");
  MSHA_ARG_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
                 "adam_rows_step: bad hyperparameters");
  AdamRows b{};
  b.param = param, b.exp_avg = exp_avg, b.exp_avg_sq = exp_avg_sq, b.step = step;
  b.rows = rows, b.n_rows = n_rows, b.vals = vals;
  b.n = n, b.cap = cap, b.F = feat, b.dt = dtype;
  b.lr = lr, b.b1 = beta1, b.b2 = beta2, b.eps = eps;
  const int lanes = feat * (dtype == MSHA_DTYPE_BF16 ? 2 : 4) / 16;  // per row
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_rows_kernel, dim3(grid_for(cap, 256 / lanes, 1 << 20)), dim3(256), 0,
                     s, b);
  hipLaunchKernelGGL(adam_rows_tick_kernel, dim3(1), dim3(1), 0, s, step);
  return check_launch("adam_rows_step");
}

extern "C" int msha_adam_rows_replay(int64_t n, int32_t feat, int32_t dtype, void* param,
                                     void* exp_avg, void* exp_avg_sq, float* step,
                                     int32_t* row_step, const int32_t* rows,
                                     const int32_t* n_rows, int64_t cap, const float* vals,
                                     int32_t max_steps, double lr, double beta1, double beta2,
                                     double eps, double weight_decay, msha_stream_t stream) {
  MSHA_ARG_CHECK(n >= 1 && n < ((int64_t)1 << 31) - 1,
                 "adam_rows_replay: bad sizes (1 <= n < 2^31 - 1)");
  MSHA_ARG_CHECK(pg_width_ok(feat, dtype),
                 "adam_rows_replay: unsupported width: feat must be a power of two in [16 B, "
                 "64 lanes x 16 B] of an fp32 or bf16 table (msha_link_bce_supported)");
  MSHA_ARG_CHECK(cap >= 1 && cap <= n,
                 "adam_rows_replay: cap must be in [1, n] (msha_plan_rows)");
  MSHA_ARG_CHECK(param && exp_avg && exp_avg_sq && step && row_step && (!rows || n_rows),
                 "adam_rows_replay: null pointer");
  MSHA_ARG_CHECK(rows != nullptr || cap == n,
                 "adam_rows_replay: rows == NULL names every row: cap must be n");
  MSHA_ARG_CHECK(max_steps >= 1, "adam_rows_replay: max_steps must be at least 1");
  MSHA_ARG_CHECK((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
                   (uintptr_t)vals) & 15) == 0,
                 "adam_rows_replay: the table, its moments and vals must be 16-byte aligned");
  MSHA_ARG_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 &&
                     weight_decay >= 0.0,
                 "adam_rows_replay: bad hyperparameters (betas in [0, 1), eps >= 0, "
                 "weight_decay >= 0)");
  AdamReplay b{};
  b.param = param, b.exp_avg = exp_avg, b.exp_avg_sq = exp_avg_sq, b.step = step;
  b.row_step = row_step, b.rows = rows, b.n_rows = n_rows, b.vals = vals;
  b.n = n, b.cap = cap, b.F = feat, b.max_steps = max_steps;
  b.lr = lr, b.b1 = beta1, b.b2 = beta2, b.eps = eps, b.wd = weight_decay;
  const int lanes = feat * (dtype == MSHA_DTYPE_BF16 ? 2 : 4) / 16;  // per row
  const dim3 grid(grid_for(cap, 256 / lanes, 1 << 20));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MSHA_DTYPE_BF16)
    hipLaunchKernelGGL(adam_replay_kernel<true>, grid, dim3(256), 0, s, b);
  else
    hipLaunchKernelGGL(adam_replay_kernel<false>, grid, dim3(256), 0, s, b);
  if (vals != nullptr) hipLaunchKernelGGL(adam_rows_tick_kernel, dim3(1), dim3(1), 0, s, step);
  return check_launch("adam_rows_replay");
}

extern "C" size_t msha_adam_workspace_size(void) {
  return sizeof(uint32_t) * kAdamLine * (1 + kAdamLeaves);
}
