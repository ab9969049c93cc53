// Order-preserving uint32 images of an fp32 value: integer compares that order floats.
//
//   ra_key    the base image (eval.hip's rank AUC): the fp32 bits with -0.0 folded onto
//             +0.0, negatives inverted, the sign bit flipped.  Unsigned order == float
//             order on everything but NaN; NaNs land at both ends by their sign.
//   tk_image  ra_key with every NaN sent to 1 first (topk.hip): below -inf (0x007fffff),
//             above 0 ("no candidate"), all NaNs equal.
//   rk_image  the same order as tk_image, without its two branches (rank.hip): no fold and
//             no NaN test, but the unfolded base image + 0x007fffff (mod 2^32), written as
//             m + 0x807fffff with m the fp32 bits, the low 31 inverted under a set sign.
//             The rotation makes the NaNs the lowest contiguous range and leaves -0.0 one
//             below +0.0.
//             rk_bracket turns a target's logit into the closed range of images that tie
//             with it (the NaN range, the two zeros, or one image), so "above" and "equal"
//             are two compares per logit and give tk_image's answers.
#pragma once

#include "common.h"

namespace msha {

__device__ __forceinline__ uint32_t ra_key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0u;  // -0.0 == +0.0 (denormals stay distinct)
  return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u;
}
__device__ __forceinline__ uint32_t ra_bits(uint32_t key) {
  return (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
}

__device__ __forceinline__ uint32_t tk_image(float v) {
  const uint32_t b = __float_as_uint(v);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 1u;
  return ra_key(b);
}
__device__ __forceinline__ float tk_value(uint32_t img) { return __uint_as_float(ra_bits(img)); }
// (logit descending, index ascending) as one integer compare; 0 is "no candidate"
__device__ __forceinline__ unsigned long long tk_key(float v, uint32_t idx) {
  return ((unsigned long long)tk_image(v) << 32) | (unsigned long long)(uint32_t)~idx;
}

constexpr uint32_t kRkNaNTop = 0x00fffffdu;    // every NaN's image is at or below this
constexpr uint32_t kRkNegZero = 0x807ffffeu;   // image of -0.0; +0.0 is one above

__device__ __forceinline__ uint32_t rk_image(float v) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t flip = (uint32_t)((int32_t)b >> 31) >> 1;
  return (b ^ flip) + 0x807fffffu;
}
// [lo, hi]: the images that tie with a target of logit z
__device__ __forceinline__ void rk_bracket(float z, uint32_t* lo, uint32_t* hi) {
  const uint32_t w = rk_image(z);
  if (w <= kRkNaNTop) {
    *lo = 0u;
    *hi = kRkNaNTop;
  } else if (w == kRkNegZero || w == kRkNegZero + 1u) {
    *lo = kRkNegZero;
    *hi = kRkNegZero + 1u;
  } else {
    *lo = w;
    *hi = w;
  }
}

}  // namespace msha
