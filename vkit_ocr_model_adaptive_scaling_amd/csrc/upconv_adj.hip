// Backward of a head, z = conv3x3(U x) with U the x2 bilinear upsample (resize2x_fwd_kernel) of the neck feature x, at the
// neck's resolution.  For the incoming dz (B, 2h, 2w, N) the nine maps
//     E_k[s, n] = sum_q U[q, s] * dz[q + (k - 1), n]        k = (ky, kx) in {0,1,2}^2, zero where q + (k - 1) leaves the map
// (q an upsampled pixel that reads source pixel s) turn both gradients into plain matrix products over h*w rows:
//     dx[s, c]     = sum_{k, n} E_k[s, n] * Bt[c][k][n]     Bt = the mode-1 (dgrad, taps rotated) weight image
//     dW[n, c, 8-k] = sum_s E_k[s, n] * x[s, c]
// - a quarter of the products of the dgrad / wgrad convolutions at 2h x 2w.  E is (B, h, w, 9 N), column k * N + n: the K
// order of the mode-1 image.
//
// A thread owns one 8-channel vector of one source pixel (i, j): consecutive lanes walk channels, then j, so a wave's loads
// and its stores are contiguous runs of N elements.  U^T reads destinations 2i-1 .. 2i+2 x 2j-1 .. 2j+2; the nine taps move that
// 4 x 4 window by one pixel each way, so the thread reads the 6 x 6 window 2i-2 .. 2i+3 x 2j-2 .. 2j+3 ONCE (row by row) and
// applies the separable weights: along x into three partial sums per window row, then along y into the nine accumulators
// (108 multiply-adds per channel instead of 144).  Loads are unconditional from clamped addresses; a window pixel outside
// the map (the convolution's zero padding) is zeroed on use, and U's border clamping is in the weights.  fp32 arithmetic, one
// rounding to the storage type.
#include "vkas_common.h"

namespace {

// as in resize.hip: workgroups are dealt round-robin over the 8 XCDs; give every XCD one contiguous run of image rows
__device__ __forceinline__ int xcd_row(unsigned bx, unsigned rows) {
  const unsigned xcd = bx & 7u, slot = bx >> 3;
  const unsigned q8 = rows >> 3, r8 = rows & 7u;
  return (int)((xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot);
}

// weights with which destinations 2i-1, 2i, 2i+1, 2i+2 read source i of n (bilinear x2, align_corners=False, clamped):
// 0.25, 0.75, 0.75, 0.25; destination 0 reads source 0 alone and destination 2n-1 source n-1 alone; outside the map: 0
__device__ __forceinline__ void ut_weights(int i, int n, float* w) {
  w[0] = i == 0 ? 0.f : 0.25f;
  w[1] = i == 0 ? 1.f : 0.75f;
  w[2] = i == n - 1 ? 1.f : 0.75f;
  w[3] = i == n - 1 ? 0.f : 0.25f;
}

// grid.x = B*h source rows, grid.y = chunks of 256 (pixel, vector) pairs of one row
template <typename T>
__global__ __launch_bounds__(256) void upconv_adj_kernel(const T* __restrict__ dz, long lddz, T* __restrict__ E, int h,
                                                         int w, int nvec) {
  const int idx = blockIdx.y * 256 + threadIdx.x;
  const int j = idx / nvec;
  const int v = idx - j * nvec;
  if (j >= w) return;
  const int row = xcd_row(blockIdx.x, gridDim.x);
  const int b = row / h;
  const int i = row - b * h;
  const int H2 = 2 * h, W2 = 2 * w;
  float wy[4], wx[4];
  ut_weights(i, h, wy);
  ut_weights(j, w, wx);
  int xc[6];
  bool xok[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int X = 2 * j - 2 + c;
    xok[c] = X >= 0 && X < W2;
    xc[c] = X < 0 ? 0 : (X >= W2 ? W2 - 1 : X);
  }
  const T* db = dz + (long)b * H2 * W2 * lddz + v * 8;
  float acc[3][3][8];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[ky][kx][k] = 0.f;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int Y = 2 * i - 2 + r;
    const bool yok = Y >= 0 && Y < H2;
    const int yc = Y < 0 ? 0 : (Y >= H2 ? H2 - 1 : Y);
    const T* rowp = db + (long)yc * W2 * lddz;
    Raw8<T> raw[6];  // the row's six requests first, conversions afterwards
#pragma unroll
    for (int c = 0; c < 6; ++c) raw[c].load(rowp + (long)xc[c] * lddz);
    float hs[3][8];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int k = 0; k < 8; ++k) hs[kx][k] = 0.f;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      raw[c].keep_if(yok && xok[c]);
      float t[8];
      raw[c].unpack(t);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int a = c - kx;  // window column c is destination 2j-1+a moved by tap kx
        if (a < 0 || a > 3) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) hs[kx][k] = fmaf(wx[a], t[k], hs[kx][k]);
      }
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int a = r - ky;
      if (a < 0 || a > 3) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[ky][kx][k] = fmaf(wy[a], hs[kx][k], acc[ky][kx][k]);
    }
  }
  const long N = (long)nvec * 8;
  T* dst = E + (((long)b * h + i) * w + j) * (9 * N) + v * 8;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) store8(dst + (ky * 3 + kx) * N, acc[ky][kx]);
}

// gE (9 N, Cp) fp32, row k * N + n [the weight-gradient GEMM of E against x] added onto the packed gradient
// gwp (N, 3, 3, Cp) of the forward taps: gwp[n][8 - k][c] += gE[k * N + n][c]
__global__ __launch_bounds__(256) void upconv_adj_unpack_kernel(const float* __restrict__ gE, float* __restrict__ gwp, int N,
                                                                int Cp4, long total4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const int c4 = (int)(i % Cp4);
    const long r = i / Cp4;
    const int n = (int)(r % N);
    const int k = (int)(r / N);
    const float4 s = reinterpret_cast<const float4*>(gE)[i];
    float4* d = reinterpret_cast<float4*>(gwp) + ((long)n * 9 + (8 - k)) * Cp4 + c4;
    float4 o = *d;
    o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
    *d = o;
  }
}

}  // namespace

extern "C" int vkas_upconv_adj(const void* dz, long lddz, void* E, int B, int h, int w, int N, int dtype, void* stream) {
  VKAS_CHECK(dz && E && vkas_aligned16(dz) && vkas_aligned16(E), "vkas_upconv_adj: null/misaligned tensor");
  VKAS_CHECK(B >= 0 && h > 0 && w > 0, "vkas_upconv_adj: bad spatial dims");
  VKAS_CHECK(N > 0 && N % 8 == 0 && lddz >= N && lddz % 8 == 0, "vkas_upconv_adj: bad channels/stride (N=%d lddz=%ld)", N, lddz);
  VKAS_CHECK(dtype == VKAS_BF16 || dtype == VKAS_F16, "vkas_upconv_adj: 16-bit storage only");
  if (B == 0) return VKAS_OK;
  VKAS_CHECK((long)B * h < (1L << 31) && (long)w * (N / 8) < (1L << 30) && vkas_cdiv((long)w * (N / 8), 256) <= 65535,
             "vkas_upconv_adj: map too large");
  dim3 grid((unsigned)((long)B * h), (unsigned)vkas_cdiv((long)w * (N / 8), 256));
  if (dtype == VKAS_BF16)
    upconv_adj_kernel<bf16_t><<<grid, 256, 0, vkas_stream(stream)>>>((const bf16_t*)dz, lddz, (bf16_t*)E, h, w, N / 8);
  else
    upconv_adj_kernel<f16_t><<<grid, 256, 0, vkas_stream(stream)>>>((const f16_t*)dz, lddz, (f16_t*)E, h, w, N / 8);
  VKAS_LAUNCH_CHECK("upconv_adj");
  return VKAS_OK;
}

extern "C" int vkas_upconv_adj_unpack_wgrad(const float* gE, float* gwp, int N, int Cp, void* stream) {
  VKAS_CHECK(gE && gwp && vkas_aligned16(gE) && vkas_aligned16(gwp), "vkas_upconv_adj_unpack_wgrad: null/misaligned pointer");
  VKAS_CHECK(N > 0 && Cp > 0 && Cp % 8 == 0, "vkas_upconv_adj_unpack_wgrad: bad sizes (N=%d Cp=%d)", N, Cp);
  const long total4 = 9L * N * (Cp / 4);
  long g = vkas_cdiv(total4, 256);
  if (g > 4096) g = 4096;
  upconv_adj_unpack_kernel<<<(unsigned)g, 256, 0, vkas_stream(stream)>>>(gE, gwp, N, Cp / 4, total4);
  VKAS_LAUNCH_CHECK("upconv_adj_unpack_wgrad");
  return VKAS_OK;
}
