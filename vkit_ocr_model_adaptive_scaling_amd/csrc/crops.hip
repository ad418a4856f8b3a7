// Training crops from annotated pages (dataset/crops.py holds the rule and the host oracle crop_host): one affine map per
// output image - scale, a small rotation, a translation - sampled by the integer rule of the inference warps (respack.hip's
// warp_pixel, inferencing/packing.py::warp_host), then a photometric jitter in float32.  rows (B, 16) int64: source, ay, ax,
// myy, myx, mxy, mxx (Q16), log2n, three gain and three bias words and the noise amplitude (float32 bits in the low 32), the
// 64-bit noise key.  The pages lie in ONE byte arena with the (S, 4) int64 source table (byte offset, Hs, Ws, 0) of the
// multi pack.  One launch, driven from the output:
//
//   * a 256-thread workgroup owns a 16 x 64 tile of one output image, a thread four adjacent cells of a row (labels.hip's
//     tile shape: a wave stores 4 rows x 256 bytes per channel plane);
//   * the image's 16 words and its source entry are read at wave-uniform addresses (scalar loads);
//   * a cell is n x n bilinear sub-samples with 64-bit accumulators and one rounding shift, a tap outside the page weighing 0;
//     the page bytes are gathered directly and without a branch (see DESIGN.md 4m for the LDS staging that was not built);
//     a cell none of whose taps can reach the page is zero without the loop;
//   * t = gain*v, t += bias, t += amp*r, clamp to [0, 255]: every product and sum rounded (cr_mul / cr_add below, compiled
//     without contraction); r = float(u >> 40) * 2^-23 - 1 from a splitmix64 finaliser of the element's index and the key;
//   * one 16-byte store per channel plane when W % 4 == 0 and the output is 16-byte aligned, plain stores otherwise.
// No atomics, no allocation, no synchronisation; every output element is written exactly once, so the call is capture-safe
// and bit-identical from run to run.  An image whose row cannot be trusted - source outside [0, S), a source entry that
// does not fit the arena or has a side outside [1, 8192], a coefficient outside the warp bounds - is written as zeros; log2n is
// clamped to [0, 3]; taps are bounded by that source's Hs, Ws: no table content makes the kernel touch memory outside its
// buffers.  The blurred crops (vkas_crop_warp_blur_f32, two launches) are described above their kernels below.
#include "vkas_common.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_TILE_H = 16, CR_TILE_W = 64, CR_QUAD = 4;
constexpr int CR_WORDS = 16;
constexpr int CR_SIDE_MAX = 8192;
constexpr long long CR_M_MAX = 1LL << 22, CR_A_MAX = 1LL << 40;
constexpr unsigned long long CR_GOLD = 0x9E3779B97F4A7C15ull, CR_C1 = 0xBF58476D1CE4E5B9ull, CR_C2 = 0x94D049BB133111EBull;

// one rounding per operation, as numpy float32 does (see labels.hip on why plain * and + are not enough)
#pragma clang fp contract(off)
__device__ __forceinline__ float cr_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float cr_add(float a, float b) { return a + b; }
#pragma clang fp contract(fast)

__device__ __forceinline__ unsigned long long cr_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * CR_C1;
  z = (z ^ (z >> 27)) * CR_C2;
  return z ^ (z >> 31);
}

struct CropMap {
  long long ay, ax, myy, myx, mxy, mxx;
  int ln;
};

__device__ __forceinline__ int cr_clamp(long long k, int hi) { return (int)(k < 0 ? 0 : (k > hi ? hi : k)); }

// The arithmetic of respack.hip's warp_pixel for destination pixel (i, j) with N = 2^LN sub-samples per axis, without a
// branch: the four taps of a sub-sample are read at indices clamped into the page and a tap outside it gets weight 0 (the
// form of the host's _warp_samples).  The sums are integers, so this is the same value; and the twelve byte loads of a
// sub-sample - and those of the unrolled ones beside it - are in flight together instead of one wait per tap.
template <int LN>
__device__ __forceinline__ void cr_pixel(const unsigned char* __restrict__ src, int Hs, int Ws, const CropMap& p, int i, int j,
                                         unsigned out[3]) {
  constexpr int n = 1 << LN, unrolled = n < 4 ? n : 4;
  const long long Y = p.ay + i * p.myy + j * p.myx, X = p.ax + i * p.mxy + j * p.mxx;
  unsigned long long acc[3] = {0ull, 0ull, 0ull};
#pragma unroll 1
  for (int a = 0; a < n; ++a) {
#pragma unroll unrolled
    for (int b = 0; b < n; ++b) {
      const long long ka = 2 * a + 1 - n, kb = 2 * b + 1 - n;
      const long long Ys = Y + ((ka * p.myy + kb * p.myx) >> (1 + LN));  // arithmetic shifts: floors
      const long long Xs = X + ((ka * p.mxy + kb * p.mxx) >> (1 + LN));
      const long long ky = Ys >> 16, kx = Xs >> 16;
      const unsigned fy = (unsigned)(Ys & 65535), fx = (unsigned)(Xs & 65535);
      const unsigned wy0 = (ky >= 0 && ky < Hs) ? 65536u - fy : 0u, wy1 = (ky + 1 >= 0 && ky + 1 < Hs) ? fy : 0u;
      const unsigned wx0 = (kx >= 0 && kx < Ws) ? 65536u - fx : 0u, wx1 = (kx + 1 >= 0 && kx + 1 < Ws) ? fx : 0u;
      const long r0 = (long)cr_clamp(ky, Hs - 1) * Ws, r1 = (long)cr_clamp(ky + 1, Hs - 1) * Ws;
      const int c0 = cr_clamp(kx, Ws - 1), c1 = cr_clamp(kx + 1, Ws - 1);
      const unsigned char *p00 = src + (r0 + c0) * 3, *p01 = src + (r0 + c1) * 3;
      const unsigned char *p10 = src + (r1 + c0) * 3, *p11 = src + (r1 + c1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned in0 = wx0 * p00[c] + wx1 * p01[c], in1 = wx0 * p10[c] + wx1 * p11[c];  // below 2^24
        acc[c] += (unsigned long long)wy0 * in0 + (unsigned long long)wy1 * in1;
      }
    }
  }
  constexpr int shift = 32 + 2 * LN;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (unsigned)((acc[c] + (1ull << (shift - 1))) >> shift);
}

// How far (Q16) a sub-sample of a cell lies from the cell's own coordinate on one axis, at most: its offset is the floor of
// t / 2^(1 + ln) with |t| <= (n - 1) * (|my| + |mx|).
__device__ __forceinline__ long long cr_reach(long long my, long long mx, int ln) {
  const long long n1 = (1 << ln) - 1;
  return ((n1 * ((my < 0 ? -my : my) + (mx < 0 ? -mx : mx))) >> (1 + ln)) + 1;
}

// false: every tap (rows k, k + 1 and columns kx, kx + 1 of every sub-sample) of cell (i, j) lies outside the page, so its
// geometric value is 0 without the loop and its loads - the zero padding around a page
__device__ __forceinline__ bool cr_reaches(const CropMap& p, long long ry, long long rx, int Hs, int Ws, int i, int j) {
  const long long Y = p.ay + i * p.myy + j * p.myx, X = p.ax + i * p.mxy + j * p.mxx;
  return ((Y + ry) >> 16) >= -1 && ((Y - ry) >> 16) < Hs && ((X + rx) >> 16) >= -1 && ((X - rx) >> 16) < Ws;
}

__global__ __launch_bounds__(CR_THREADS) void crop_warp_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                               const long long* __restrict__ sources, int S,
                                                               const long long* __restrict__ rows, float* __restrict__ out,
                                                               int H, int W, int vec) {
  const int tid = threadIdx.x, b = blockIdx.z;
  const int y = blockIdx.y * CR_TILE_H + tid / (CR_TILE_W / CR_QUAD);
  const int x = blockIdx.x * CR_TILE_W + (tid % (CR_TILE_W / CR_QUAD)) * CR_QUAD;
  if (y >= H || x >= W) return;

  const long long* t = rows + (long)b * CR_WORDS;  // wave-uniform
  const long long s = t[0];
  CropMap p{t[1], t[2], t[3], t[4], t[5], t[6], 0};
  const long long ln = t[7];
  p.ln = (int)(ln < 0 ? 0 : (ln > 3 ? 3 : ln));
  const auto m_ok = [](long long m) { return m >= -CR_M_MAX && m <= CR_M_MAX; };
  bool ok = s >= 0 && s < S && p.ay > -CR_A_MAX && p.ay < CR_A_MAX && p.ax > -CR_A_MAX && p.ax < CR_A_MAX && m_ok(p.myy) &&
            m_ok(p.myx) && m_ok(p.mxy) && m_ok(p.mxx);
  const unsigned char* src = arena;
  int Hs = 0, Ws = 0;
  if (ok) {
    const long long* e = sources + s * 4;
    const long long off = e[0], hs = e[1], ws = e[2];
    ok = hs >= 1 && hs <= CR_SIDE_MAX && ws >= 1 && ws <= CR_SIDE_MAX && off >= 0 && off <= arena_bytes &&
         3 * hs * ws <= arena_bytes - off;
    if (ok) {
      src = arena + off;
      Hs = (int)hs; Ws = (int)ws;
    }
  }

  float v[3][CR_QUAD];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < CR_QUAD; ++q) v[c][q] = 0.f;
  if (ok) {
    float gain[3], bias[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      gain[c] = __int_as_float((int)(unsigned)t[8 + c]);
      bias[c] = __int_as_float((int)(unsigned)t[11 + c]);
    }
    const float amp = __int_as_float((int)(unsigned)t[14]);
    const unsigned long long key = (unsigned long long)t[15];
    const long long ry = cr_reach(p.myy, p.myx, p.ln), rx = cr_reach(p.mxy, p.mxx, p.ln);
#pragma unroll
    for (int q = 0; q < CR_QUAD; ++q) {
      if (x + q >= W) continue;
      unsigned g[3] = {0u, 0u, 0u};
      if (cr_reaches(p, ry, rx, Hs, Ws, y, x + q)) {
        switch (p.ln) {  // wave-uniform
          case 0: cr_pixel<0>(src, Hs, Ws, p, y, x + q, g); break;
          case 1: cr_pixel<1>(src, Hs, Ws, p, y, x + q, g); break;
          case 2: cr_pixel<2>(src, Hs, Ws, p, y, x + q, g); break;
          default: cr_pixel<3>(src, Hs, Ws, p, y, x + q, g); break;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned long long idx = ((unsigned long long)c * H + y) * W + (x + q);
        const unsigned long long u = cr_mix((idx + 1ull) * CR_GOLD + key);
        const float r = cr_add(cr_mul((float)(unsigned)(u >> 40), 0x1p-23f), -1.0f);
        float tv = cr_mul(gain[c], (float)g[c]);
        tv = cr_add(tv, bias[c]);
        tv = cr_add(tv, cr_mul(amp, r));
        v[c][q] = tv > 0.f ? (tv < 255.f ? tv : 255.f) : 0.f;  // -0 and NaN give +0
      }
    }
  }

#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* o = out + (((long)b * 3 + c) * H + y) * W + x;
    if (vec) {  // W % 4 == 0 and a 16-byte aligned output: x + 3 < W and every quad starts on 16 bytes
      f32x4 quad = {v[c][0], v[c][1], v[c][2], v[c][3]};
      *reinterpret_cast<f32x4*>(o) = quad;
    } else {
#pragma unroll
      for (int q = 0; q < CR_QUAD; ++q)
        if (x + q < W) o[q] = v[c][q];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Blurred crops (dataset/blur.py holds the rule and the host oracle crop_blur_host): a (B, 226) int32 blur-row table - the
// radius R in [0, 7], then 15 x 15 weights that sum to 65536 - turns the geometric value into
// acc = sum over a, b in [-R, R] of w[7 + a][7 + b] * v(y + a, x + b) before the jitter, v continuing the row's map outside the
// crop.  Two launches on one stream:
//
//   1. crop_geo_kernel: cr_pixel at cell (wy - Rm, wx - Rm), Rm = radius_max, into uint8 planes (B, 3, H + 2 Rm, pitch) of the
//      caller's work buffer, pitch a multiple of 16 - each geometric value is computed ONCE: the n x n gather is the expensive
//      part, and a fused kernel would redo it 2.3 x for a 16 x 64 tile with a halo of 7.  The tile shape of crop_warp_kernel;
//      a thread stores its four cells of a plane as one dword, a wave 4 rows x 256 bytes.  Cells outside the sample's own halo
//      (its R may be below Rm) are stored as 0 without the gather.  The bounds of a row hold over the halo: for i, j in
//      [-7, 8192 + 7) |Y| < 2^40 + 2 * 8199 * 2^22 < 2^40 + 2^36 + 2^26, no intermediate leaves 64 bits.
//   2. crop_blur_kernel: the tile shape, the jitter and the store path of crop_warp_kernel.  The workgroup validates its blur
//      row (range, square, the sum by a reduction); R is wave-uniform (blockIdx.z) and selects one of eight bodies, so that the
//      window of a thread lives in registers.  The (16 + 2R) x (64 + 2R) window of each plane is staged through LDS as the
//      aligned dwords of the work rows that hold it (the window starts s = 0..3 bytes into the first, s wave-uniform); an LDS
//      row is 48 dwords, so that the two rows of a 32-lane half read disjoint banks (16 + 32k apart).  Per window row a
//      thread reads its 1 + ceil((4 + 2R) / 4) dwords once, shifts them by s, and slides its four cells over the 4 + 2R bytes:
//      an LDS byte is read once per row, not once per tap.  The weights of the row are read at wave-uniform addresses; a
//      product is 24-bit (w <= 2^16, v <= 255, the sum below 2^24): one full-rate 24-bit multiply-add per tap, cell and plane.
//
// No atomics, no allocation, no synchronisation; every output element is written exactly once; capture-safe and bit-identical
// from run to run.  The trust rules of crop_warp_kernel apply unchanged, and an image whose blur row is invalid - R outside
// [0, radius_max], a weight outside [0, 65536], a non-zero weight outside the square, a sum other than 65536 - is zeros.
constexpr int BL_WORDS = 226, BL_SIDE = 15, BL_RMAX = 7, BL_ONE = 65536;
constexpr int BL_LDS_PITCH = 48;                     // dwords per LDS row: 16 mod 32, at least 16 + ceil(17 / 4) = 21
constexpr int BL_LDS_ROWS = CR_TILE_H + 2 * BL_RMAX;

// the row of image b as crop_warp_kernel trusts it: false for an image of zeros
__device__ __forceinline__ bool cr_trusted_row(const unsigned char* __restrict__ arena, long long arena_bytes,
                                               const long long* __restrict__ sources, int S, const long long* __restrict__ t,
                                               CropMap& p, const unsigned char*& src, int& Hs, int& Ws) {
  const long long s = t[0];
  p = CropMap{t[1], t[2], t[3], t[4], t[5], t[6], 0};
  const long long ln = t[7];
  p.ln = (int)(ln < 0 ? 0 : (ln > 3 ? 3 : ln));
  const auto m_ok = [](long long m) { return m >= -CR_M_MAX && m <= CR_M_MAX; };
  if (!(s >= 0 && s < S && p.ay > -CR_A_MAX && p.ay < CR_A_MAX && p.ax > -CR_A_MAX && p.ax < CR_A_MAX && m_ok(p.myy) &&
        m_ok(p.myx) && m_ok(p.mxy) && m_ok(p.mxx)))
    return false;
  const long long* e = sources + s * 4;
  const long long off = e[0], hs = e[1], ws = e[2];
  if (!(hs >= 1 && hs <= CR_SIDE_MAX && ws >= 1 && ws <= CR_SIDE_MAX && off >= 0 && off <= arena_bytes &&
        3 * hs * ws <= arena_bytes - off))
    return false;
  src = arena + off;
  Hs = (int)hs; Ws = (int)ws;
  return true;
}

__global__ __launch_bounds__(CR_THREADS) void crop_geo_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                              const long long* __restrict__ sources, int S,
                                                              const long long* __restrict__ rows,
                                                              const int* __restrict__ blur_rows, int Rm,
                                                              unsigned char* __restrict__ work, int H, int W, int pitch) {
  const int tid = threadIdx.x, b = blockIdx.z;
  const int Hw = H + 2 * Rm;
  const int wy = blockIdx.y * CR_TILE_H + tid / (CR_TILE_W / CR_QUAD);
  const int wx = blockIdx.x * CR_TILE_W + (tid % (CR_TILE_W / CR_QUAD)) * CR_QUAD;
  if (wy >= Hw || wx >= pitch) return;  // pitch % 4 == 0: a thread's dword lies inside the row or outside it

  CropMap p;
  const unsigned char* src = arena;
  int Hs = 0, Ws = 0;
  const int R = blur_rows[(long)b * BL_WORDS];  // wave-uniform
  const bool ok = cr_trusted_row(arena, arena_bytes, sources, S, rows + (long)b * CR_WORDS, p, src, Hs, Ws) && R >= 0 && R <= Rm;
  unsigned packed[3] = {0u, 0u, 0u};
  const int i = wy - Rm;
  if (ok && i >= -R && i < H + R) {
    const long long ry = cr_reach(p.myy, p.myx, p.ln), rx = cr_reach(p.mxy, p.mxx, p.ln);
#pragma unroll
    for (int q = 0; q < CR_QUAD; ++q) {
      const int j = wx + q - Rm;
      if (j < -R || j >= W + R || !cr_reaches(p, ry, rx, Hs, Ws, i, j)) continue;
      unsigned g[3];
      switch (p.ln) {  // wave-uniform
        case 0: cr_pixel<0>(src, Hs, Ws, p, i, j, g); break;
        case 1: cr_pixel<1>(src, Hs, Ws, p, i, j, g); break;
        case 2: cr_pixel<2>(src, Hs, Ws, p, i, j, g); break;
        default: cr_pixel<3>(src, Hs, Ws, p, i, j, g); break;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) packed[c] |= g[c] << (8 * q);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)  // work is 16-byte aligned, pitch % 16 == 0, wx % 4 == 0
    *reinterpret_cast<unsigned*>(work + (((long)b * 3 + c) * Hw + wy) * pitch + wx) = packed[c];
}

// acc[c][q] += sum over the (2R + 1)^2 taps for the thread's four cells; win: the thread's first dword of LDS row 0 of plane 0
template <int R>
__device__ __forceinline__ void blur_taps(const unsigned* __restrict__ win, const int* __restrict__ weights, int s,
                                          unsigned acc[3][CR_QUAD]) {
  constexpr int taps = 2 * R + 1, span = CR_QUAD + 2 * R;  // bytes of a row that the four cells see
  constexpr int aligned = (span + 3) / 4, loaded = aligned + 1;
#pragma unroll 1
  for (int a = 0; a < taps; ++a) {
    const int* wrow = weights + (BL_RMAX - R + a) * BL_SIDE + (BL_RMAX - R);  // wave-uniform
    unsigned w[taps];
#pragma unroll
    for (int k = 0; k < taps; ++k) w[k] = (unsigned)wrow[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned* row = win + (c * BL_LDS_ROWS + a) * BL_LDS_PITCH;
      unsigned d[loaded];
#pragma unroll
      for (int k = 0; k < loaded; ++k) d[k] = row[k];
      unsigned v[4 * aligned];
#pragma unroll
      for (int k = 0; k < aligned; ++k) {
        const unsigned u = (unsigned)((((unsigned long long)d[k + 1] << 32) | d[k]) >> (8 * s));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * k + e] = (u >> (8 * e)) & 255u;
      }
#pragma unroll
      for (int q = 0; q < CR_QUAD; ++q)
#pragma unroll
        for (int k = 0; k < taps; ++k) acc[c][q] = __umul24(w[k], v[q + k]) + acc[c][q];
    }
  }
}

__global__ __launch_bounds__(CR_THREADS) void crop_blur_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                               const long long* __restrict__ sources, int S,
                                                               const long long* __restrict__ rows,
                                                               const int* __restrict__ blur_rows, int Rm,
                                                               const unsigned char* __restrict__ work, int pitch,
                                                               float* __restrict__ out, int H, int W, int vec) {
  __shared__ unsigned lds[3 * BL_LDS_ROWS * BL_LDS_PITCH];
  __shared__ unsigned wave_sum[CR_THREADS / 64];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int ty = tid / (CR_TILE_W / CR_QUAD), tx = tid % (CR_TILE_W / CR_QUAD);
  const int y0 = blockIdx.y * CR_TILE_H, x0 = blockIdx.x * CR_TILE_W;
  const int y = y0 + ty, x = x0 + tx * CR_QUAD;
  const int Hw = H + 2 * Rm;

  // the blur row: every weight in range and zero outside the square (one per thread), the sum by a reduction
  const int* bw = blur_rows + (long)b * BL_WORDS;  // wave-uniform
  const int R = bw[0];
  const bool r_ok = R >= 0 && R <= Rm;
  int bad = 0;
  unsigned part = 0u;
  if (tid < BL_SIDE * BL_SIDE) {
    const int w = bw[1 + tid];
    const int da = tid / BL_SIDE - BL_RMAX, db = tid % BL_SIDE - BL_RMAX;
    const bool far = da < -R || da > R || db < -R || db > R;
    bad = w < 0 || w > BL_ONE || (far && w != 0);
    part = (unsigned)w;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) part += __shfl_down(part, off);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = part;
  const int any_bad = __syncthreads_or(bad);  // also orders wave_sum
  const bool blur_ok = r_ok && !any_bad && wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3] == (unsigned)BL_ONE;

  CropMap p;
  const unsigned char* src = arena;
  int Hs = 0, Ws = 0;
  const long long* t = rows + (long)b * CR_WORDS;  // wave-uniform
  const bool ok = cr_trusted_row(arena, arena_bytes, sources, S, t, p, src, Hs, Ws) && blur_ok;  // block-uniform

  float v[3][CR_QUAD];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < CR_QUAD; ++q) v[c][q] = 0.f;
  if (ok) {
    // the window: crop rows y0 - R .., columns x0 - R .., i.e. work rows y0 + Rm - R .. and work columns c0 + s ..
    const int wy0 = y0 + Rm - R, wx0 = x0 + Rm - R;
    const int c0 = wx0 & ~3, s = wx0 & 3;
    const int nrows = CR_TILE_H + 2 * R, ndw = CR_TILE_W / 4 + (3 + 2 * R + 3) / 4;  // at most 30 rows of 21 dwords
    for (int k = tid; k < 3 * nrows * ndw; k += CR_THREADS) {
      const int c = k / (nrows * ndw), rem = k - c * nrows * ndw, r = rem / ndw, d = rem - r * ndw;
      const int wy = wy0 + r, wx = c0 + 4 * d;
      unsigned u = 0u;  // outside the planes: rows and columns that only cells outside the crop would read
      if (wy < Hw && wx < pitch) u = *reinterpret_cast<const unsigned*>(work + (((long)b * 3 + c) * Hw + wy) * pitch + wx);
      lds[(c * BL_LDS_ROWS + r) * BL_LDS_PITCH + d] = u;
    }
    __syncthreads();

    unsigned acc[3][CR_QUAD];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int q = 0; q < CR_QUAD; ++q) acc[c][q] = 0u;
    const unsigned* win = lds + ty * BL_LDS_PITCH + tx;
    switch (R) {  // wave-uniform
      case 0: blur_taps<0>(win, bw + 1, s, acc); break;
      case 1: blur_taps<1>(win, bw + 1, s, acc); break;
      case 2: blur_taps<2>(win, bw + 1, s, acc); break;
      case 3: blur_taps<3>(win, bw + 1, s, acc); break;
      case 4: blur_taps<4>(win, bw + 1, s, acc); break;
      case 5: blur_taps<5>(win, bw + 1, s, acc); break;
      case 6: blur_taps<6>(win, bw + 1, s, acc); break;
      default: blur_taps<7>(win, bw + 1, s, acc); break;
    }

    float gain[3], bias[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      gain[c] = __int_as_float((int)(unsigned)t[8 + c]);
      bias[c] = __int_as_float((int)(unsigned)t[11 + c]);
    }
    const float amp = __int_as_float((int)(unsigned)t[14]);
    const unsigned long long key = (unsigned long long)t[15];
    if (y < H) {
#pragma unroll
      for (int q = 0; q < CR_QUAD; ++q) {
        if (x + q >= W) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const unsigned long long idx = ((unsigned long long)c * H + y) * W + (x + q);
          const unsigned long long u = cr_mix((idx + 1ull) * CR_GOLD + key);
          const float r = cr_add(cr_mul((float)(unsigned)(u >> 40), 0x1p-23f), -1.0f);
          float tv = cr_mul(gain[c], cr_mul((float)acc[c][q], 0x1p-16f));  // acc < 2^24: both exact
          tv = cr_add(tv, bias[c]);
          tv = cr_add(tv, cr_mul(amp, r));
          v[c][q] = tv > 0.f ? (tv < 255.f ? tv : 255.f) : 0.f;  // -0 and NaN give +0
        }
      }
    }
  }

  if (y >= H || x >= W) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* o = out + (((long)b * 3 + c) * H + y) * W + x;
    if (vec) {  // W % 4 == 0 and a 16-byte aligned output: x + 3 < W and every quad starts on 16 bytes
      f32x4 quad = {v[c][0], v[c][1], v[c][2], v[c][3]};
      *reinterpret_cast<f32x4*>(o) = quad;
    } else {
#pragma unroll
      for (int q = 0; q < CR_QUAD; ++q)
        if (x + q < W) o[q] = v[c][q];
    }
  }
}

}  // namespace

extern "C" int vkas_crop_warp_f32(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                  const long long* rows, int B, float* out, int H, int W, void* stream) {
  VKAS_CHECK(B >= 0 && B <= 65535, "%s: bad B=%d (0..65535)", __func__, B);
  VKAS_CHECK(H >= 1 && W >= 1 && H <= CR_SIDE_MAX && W <= CR_SIDE_MAX, "%s: bad crop %d x %d (sides 1..%d)", __func__, H, W,
             CR_SIDE_MAX);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(arena && sources && rows && out, "%s: null pointer", __func__);
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "%s: empty arena (%lld bytes, %d sources)", __func__, arena_bytes, S);
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)rows) & 7u) == 0 && (((uintptr_t)out) & 3u) == 0,
             "%s: the source table and the rows must be 8-byte aligned, out 4-byte aligned", __func__);
  // a plane starts at a multiple of H*W floats: 16-byte aligned whenever W % 4 == 0 and the first one is
  const int vec = (W % 4 == 0) && vkas_aligned16(out);
  const dim3 grid((unsigned)vkas_cdiv(W, CR_TILE_W), (unsigned)vkas_cdiv(H, CR_TILE_H), (unsigned)B);
  crop_warp_kernel<<<grid, CR_THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, rows, out, H, W, vec);
  VKAS_LAUNCH_CHECK("crop_warp_f32");
  return VKAS_OK;
}

extern "C" int vkas_crop_warp_blur_f32(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                       const long long* rows, const int* blur_rows, int B, int radius_max, unsigned char* work,
                                       long long work_bytes, float* out, int H, int W, void* stream) {
  VKAS_CHECK(B >= 0 && B <= 65535, "%s: bad B=%d (0..65535)", __func__, B);
  VKAS_CHECK(H >= 1 && W >= 1 && H <= CR_SIDE_MAX && W <= CR_SIDE_MAX, "%s: bad crop %d x %d (sides 1..%d)", __func__, H, W,
             CR_SIDE_MAX);
  VKAS_CHECK(radius_max >= 0 && radius_max <= BL_RMAX, "%s: bad radius_max=%d (0..%d)", __func__, radius_max, BL_RMAX);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(arena && sources && rows && blur_rows && work && out, "%s: null pointer", __func__);
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "%s: empty arena (%lld bytes, %d sources)", __func__, arena_bytes, S);
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)rows) & 7u) == 0 && (((uintptr_t)blur_rows) & 3u) == 0 &&
                 (((uintptr_t)out) & 3u) == 0 && vkas_aligned16(work),
             "%s: the source table and the rows must be 8-byte aligned, the blur rows and out 4-byte, work 16-byte", __func__);
  const int Hw = H + 2 * radius_max, pitch = (int)vkas_cdiv(W + 2 * radius_max, 16) * 16;
  const long long need = (long long)B * 3 * Hw * pitch;
  VKAS_CHECK(work_bytes >= need, "%s: work holds %lld bytes, %d x 3 x %d x %d planes need %lld", __func__, work_bytes, B, Hw, pitch,
             need);
  const dim3 geo((unsigned)vkas_cdiv(pitch, CR_TILE_W), (unsigned)vkas_cdiv(Hw, CR_TILE_H), (unsigned)B);
  crop_geo_kernel<<<geo, CR_THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, rows, blur_rows, radius_max, work,
                                                               H, W, pitch);
  VKAS_LAUNCH_CHECK("crop_warp_blur_f32 (geometric pass)");
  // a plane starts at a multiple of H*W floats: 16-byte aligned whenever W % 4 == 0 and the first one is
  const int vec = (W % 4 == 0) && vkas_aligned16(out);
  const dim3 grid((unsigned)vkas_cdiv(W, CR_TILE_W), (unsigned)vkas_cdiv(H, CR_TILE_H), (unsigned)B);
  crop_blur_kernel<<<grid, CR_THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, rows, blur_rows, radius_max, work,
                                                                pitch, out, H, W, vec);
  VKAS_LAUNCH_CHECK("crop_warp_blur_f32 (blur pass)");
  return VKAS_OK;
}
