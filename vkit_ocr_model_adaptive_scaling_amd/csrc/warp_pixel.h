// The affine warp row and its pixel rule (inferencing/packing.py, "affine warps"), shared by the kernels that cut slanted
// rectangles out of an image: the warp kernels of respack.hip (regions into a page) and strips.hip (text lines into strips).
#pragma once
#include "vkas_common.h"

constexpr int SIDE_MAX = 8192;
constexpr int DIM_MAX = 32768;                              // source / page sides: pixel counts stay below 2^30

// 12 int64 (dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, 0), an affine warp (inferencing/orient.py builds the rows):
// destination pixel (i, j) of the rectangle reads the source at Y = ay + i*myy + j*myx, X = ax + i*mxy + j*mxx in Q16, an
// integer coordinate being a pixel centre.
constexpr int WARP_WORDS = 12;
constexpr long long WARP_M_MAX = 1LL << 22, WARP_A_MAX = 1LL << 40;

struct WarpRow {
  long long dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n;
  static __device__ __forceinline__ WarpRow load(const long long* __restrict__ table, int i) {
    const long long* t = table + (long)i * WARP_WORDS;
    return WarpRow{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10]};
  }
  // needs no source: within these bounds no intermediate leaves 64 bits (|Y| < 2^40 + 2^36) and a tap outside the source
  // reads 0, so no table content makes a kernel read outside the source
  __device__ __forceinline__ bool ok() const {
    const auto m_ok = [](long long m) { return m >= -WARP_M_MAX && m <= WARP_M_MAX; };
    return dh >= 1 && dw >= 1 && dh <= SIDE_MAX && dw <= SIDE_MAX && dy >= 0 && dx >= 0 && dy <= DIM_MAX && dx <= DIM_MAX &&
           ay > -WARP_A_MAX && ay < WARP_A_MAX && ax > -WARP_A_MAX && ax < WARP_A_MAX && m_ok(myy) && m_ok(myx) &&
           m_ok(mxy) && m_ok(mxx) && log2n >= 0 && log2n <= 3;
  }
};

__device__ __forceinline__ bool side_ok(long long v) { return v >= 1 && v <= DIM_MAX; }

// two-tap bilinear in x on source row k (zero outside the source): sum over the taps of weight * pixel, below 2^24
__device__ __forceinline__ void warp_row_taps(const unsigned char* __restrict__ src, int Hs, int Ws, long long k,
                                              long long kx, unsigned fx, unsigned in[3]) {
  in[0] = in[1] = in[2] = 0u;
  if (k < 0 || k >= Hs) return;
  const unsigned char* row = src + (long)k * Ws * 3;
  if (kx >= 0 && kx < Ws) {
    const unsigned char* px = row + kx * 3;
    const unsigned w = 65536u - fx;
    in[0] += w * px[0]; in[1] += w * px[1]; in[2] += w * px[2];
  }
  if (fx != 0u && kx + 1 >= 0 && kx + 1 < Ws) {
    const unsigned char* px = row + (kx + 1) * 3;
    in[0] += fx * px[0]; in[1] += fx * px[1]; in[2] += fx * px[2];
  }
}

__device__ __forceinline__ void warp_pixel(const unsigned char* __restrict__ src, int Hs, int Ws, const WarpRow& p, int i,
                                           int j, unsigned out[3]) {
  const long long Y = p.ay + i * p.myy + j * p.myx, X = p.ax + i * p.mxy + j * p.mxx;
  const int ln = (int)p.log2n, n = 1 << ln;
  unsigned long long acc[3] = {0ull, 0ull, 0ull};
  for (int a = 0; a < n; ++a) {
    for (int b = 0; b < n; ++b) {
      const long long ka = 2 * a + 1 - n, kb = 2 * b + 1 - n;
      const long long Ys = Y + ((ka * p.myy + kb * p.myx) >> (1 + ln));  // arithmetic shifts: floors
      const long long Xs = X + ((ka * p.mxy + kb * p.mxx) >> (1 + ln));
      const long long ky = Ys >> 16, kx = Xs >> 16;
      const unsigned fy = (unsigned)(Ys & 65535), fx = (unsigned)(Xs & 65535);
      unsigned r0[3], r1[3] = {0u, 0u, 0u};
      warp_row_taps(src, Hs, Ws, ky, kx, fx, r0);
      if (fy != 0u) warp_row_taps(src, Hs, Ws, ky + 1, kx, fx, r1);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += (unsigned long long)(65536u - fy) * r0[c] + (unsigned long long)fy * r1[c];
    }
  }
  const int shift = 32 + 2 * ln;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (unsigned)((acc[c] + (1ull << (shift - 1))) >> shift);
}
