// Index functions of F.interpolate (bilinear, align_corners=False; nearest) and nn.AdaptiveAvgPool2d, shared by the resize /
// pooling kernels (resize.hip) and the fused pyramid-pooling branches (ppm.hip): one statement of which source a destination
// reads, with which weight, and which pixels a pooling bin covers.
#pragma once
#include "vkas_common.h"

namespace {

// source coordinate of F.interpolate(bilinear, align_corners=False): src = max((dst+0.5)*in/out-0.5, 0)
__device__ __forceinline__ void bilinear_src(int dst, float scale, int n_in, int& i0, int& i1, float& w1) {
  float src = ((float)dst + 0.5f) * scale - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  w1 = src - (float)i0;
}
// a * (1 - w) + b * w with the contraction spelled out: one rounded product, one fused multiply-add.  Left to the compiler,
// the generic and the x2 forward contracted these sums differently (mul + fma for some outputs, mul + mul + add for others)
// and about a sixth of their fp32 outputs differed in the last bit (the 16-bit types rounded it away; the backwards agreed);
// written this way both round the same products in the same places (tests/test_gpu_resize.py compares them).
__device__ __forceinline__ float lerp2(float a, float b, float w) { return fmaf(b, w, __fmul_rn(a, 1.f - w)); }
// nearest: src = min((int)floorf(dst * scale), in-1) with the float32 scale = (float)in / out, as F.interpolate evaluates it
// (one rounded division, one rounded product: where dst * in / out is an integer the product may fall just below it, and
// the integer form floor(dst * in / out) would then pick the next source index)
__device__ __forceinline__ int nearest_src(int dst, int n_in, int n_out) {
  const float scale = __fdiv_rn((float)n_in, (float)n_out);
  const int s = (int)floorf(__fmul_rn((float)dst, scale));
  return s < n_in - 1 ? s : n_in - 1;
}

// weight with which destination index `dst` reads source index `src_i` along one axis (0 if it does not)
__device__ __forceinline__ float axis_weight(int dst, float scale, int n_in, int n_out, int src_i, int mode) {
  if (mode == 0) {
    int i0, i1;
    float w1;
    bilinear_src(dst, scale, n_in, i0, i1, w1);
    return (i0 == src_i ? 1.f - w1 : 0.f) + (i1 == src_i ? w1 : 0.f);
  }
  return nearest_src(dst, n_in, n_out) == src_i ? 1.f : 0.f;
}

// destination range [lo, hi] along one axis that reads source index i (tight; empty if lo > hi)
__device__ __forceinline__ void dst_range(int i, int n_in, int n_out, float scale, int mode, int& lo, int& hi) {
  const float r = (float)n_out / (float)n_in;
  if (mode == 0) {
    lo = (int)floorf(((float)i - 1.f) * r) - 2;
    hi = (int)ceilf(((float)i + 1.5f) * r) + 2;
  } else {
    lo = (int)floorf((float)i * r) - 2;
    hi = (int)ceilf(((float)i + 1.f) * r) + 2;
  }
  if (i == n_in - 1) hi = n_out - 1;  // the last source index also collects every clamped destination
  if (lo < 0) lo = 0;
  if (hi > n_out - 1) hi = n_out - 1;
  while (lo <= hi && axis_weight(lo, scale, n_in, n_out, i, mode) == 0.f) ++lo;
  while (hi >= lo && axis_weight(hi, scale, n_in, n_out, i, mode) == 0.f) --hi;
}

// bin i of AdaptiveAvgPool: [floor(i*n/s), ceil((i+1)*n/s))
__device__ __forceinline__ void pool_bin(int i, int n, int s, int& lo, int& hi) {
  lo = (i * n) / s;
  hi = ((i + 1) * n + s - 1) / s;
}

}  // namespace
