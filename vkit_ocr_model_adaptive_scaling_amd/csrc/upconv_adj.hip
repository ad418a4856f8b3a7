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

int vkas_colreduce_finalize(const float* partial, long P, int n, int ldp, float* out, int accumulate, hipStream_t st);

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

// One (source pixel, 8-channel vector) pair: E's nine vectors from the 6 x 6 window of dz.  CS: also add the centre 2 x 2 block
// (upsampled pixels 2i, 2i+1 x 2j, 2j+1: every upsampled pixel is in exactly one pair's centre block) onto the thread's own
// sums cs[k * 256], row-major (in LDS: the kernel has no registers to spare).
template <typename T, bool CS>
__device__ __forceinline__ void upconv_adj_pair(const T* __restrict__ dz, long lddz, T* __restrict__ E, int h, int w, int nvec,
                                                int b, int i, int j, int v, float* cs) {
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
    Raw8<T> raw[6];  // the row's six requests first, conversions afterwards
    if constexpr (CS) {
      // a row base that is the same in every lane plus six 32-bit element offsets that serve all six rows (the host
      // checks that a row of dz stays below 2^31 elements): fewer address registers than six 64-bit pointers per row
      const T* rowb = dz + ((long)b * H2 + yc) * W2 * lddz;
#pragma unroll
      for (int c = 0; c < 6; ++c) raw[c].load(rowb + (unsigned)(xc[c] * (int)lddz + v * 8));
    } else {
      const T* rowp = db + (long)yc * W2 * lddz;
#pragma unroll
      for (int c = 0; c < 6; ++c) raw[c].load(rowp + (long)xc[c] * lddz);
    }
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
      if (CS && (r == 2 || r == 3) && (c == 2 || c == 3)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) cs[k * 256] += t[k];
      }
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
  upconv_adj_pair<T, false>(dz, lddz, E, h, w, nvec, b, row - b * h, j, v, nullptr);
}

// The same E, and the column sums of dz on the way.  grid.x = B*h source rows; workgroup (x, y) takes the chunks y, y +
// gridDim.y, ... of its row, a chunk being ppc = 256 / nvec whole pixels (nvec <= 256), so that a thread keeps its vector v
// and adds its centre blocks onto its own eight sums in LDS (red[k * 256 + thread]), chunk after chunk.  The workgroup's threads of
// one v are then summed in thread order by the first of them: partial[x * gridDim.y + y][v * 8 ..], a fixed order throughout.
template <typename T>
__global__ __launch_bounds__(256, 2) void upconv_adj_colsum_kernel(const T* __restrict__ dz, long lddz, T* __restrict__ E, int h,
                                                                int w, int nvec, float* __restrict__ partial) {
  const int ppc = 256 / nvec;
  const int jl = threadIdx.x / nvec;
  const int v = threadIdx.x - jl * nvec;
  const int row = xcd_row(blockIdx.x, gridDim.x);
  const int b = __builtin_amdgcn_readfirstlane(row / h);  // the same in every lane: row addresses stay in scalar registers
  const int i = row - b * h;
  __shared__ float red[8 * 256];  // [k][thread]
#pragma unroll
  for (int k = 0; k < 8; ++k) red[k * 256 + threadIdx.x] = 0.f;
  if (jl < ppc) {
    for (int j = blockIdx.y * ppc + jl; j < w; j += gridDim.y * ppc)
      upconv_adj_pair<T, true>(dz, lddz, E, h, w, nvec, b, i, j, v, red + threadIdx.x);
  }
  __syncthreads();
  if (jl == 0) {
    float cs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cs[k] = red[k * 256 + v];
    for (int r = 1; r < ppc; ++r)
#pragma unroll
      for (int k = 0; k < 8; ++k) cs[k] += red[k * 256 + r * nvec + v];
    store8(partial + ((long)blockIdx.x * gridDim.y + blockIdx.y) * ((long)nvec * 8) + v * 8, cs);
  }
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

namespace {
// workgroups per source row of the column-sum variant: as many as keep the partial rows near 4096 (B*h = 2048 rows of the
// benchmark's passes: 2), at most one per chunk
static inline long cs_groups(int B, int h, int w, int N) {
  const long chunks = vkas_cdiv(w, 256 / (N / 8));
  long g = 4096 / ((long)B * h);
  g = g < 1 ? 1 : g;
  return g < chunks ? g : chunks;
}
}  // namespace

extern "C" size_t vkas_upconv_adj_colsum_ws_bytes(int B, int h, int w, int N) {
  if (B <= 0 || h <= 0 || w <= 0 || N <= 0 || N % 8 || N > 2048) return 0;
  return (size_t)B * h * cs_groups(B, h, w, N) * N * sizeof(float);
}

// vkas_upconv_adj, and out[n] (+)= the column sums of dz (what vkas_colsum(dz, ...) delivers): per-workgroup partial rows in
// ws, summed by the finalize kernel of vkas_colsum.  Fixed summation order: two launches give the same bits.
extern "C" int vkas_upconv_adj_colsum(const void* dz, long lddz, void* E, int B, int h, int w, int N, float* out, int accumulate,
                                      float* ws, size_t ws_bytes, int dtype, void* stream) {
  VKAS_CHECK(dz && E && out && ws && vkas_aligned16(dz) && vkas_aligned16(E) && vkas_aligned16(ws),
             "vkas_upconv_adj_colsum: null/misaligned pointer");
  VKAS_CHECK(B > 0 && h > 0 && w > 0 && (long)B * h < (1L << 31) && 2L * w * lddz < (1L << 31),
             "vkas_upconv_adj_colsum: bad spatial dims");
  VKAS_CHECK(N > 0 && N % 8 == 0 && N <= 2048 && lddz >= N && lddz % 8 == 0,
             "vkas_upconv_adj_colsum: bad channels/stride (N=%d lddz=%ld)", N, lddz);
  VKAS_CHECK(dtype == VKAS_BF16 || dtype == VKAS_F16, "vkas_upconv_adj_colsum: 16-bit storage only");
  VKAS_CHECK(ws_bytes >= vkas_upconv_adj_colsum_ws_bytes(B, h, w, N), "vkas_upconv_adj_colsum: workspace too small");
  const long G = cs_groups(B, h, w, N);
  dim3 grid((unsigned)((long)B * h), (unsigned)G);
  hipStream_t st = vkas_stream(stream);
  if (dtype == VKAS_BF16)
    upconv_adj_colsum_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dz, lddz, (bf16_t*)E, h, w, N / 8, ws);
  else
    upconv_adj_colsum_kernel<f16_t><<<grid, 256, 0, st>>>((const f16_t*)dz, lddz, (f16_t*)E, h, w, N / 8, ws);
  VKAS_LAUNCH_CHECK("upconv_adj_colsum");
  return vkas_colreduce_finalize(ws, (long)B * h * G, N, N, out, accumulate, st);
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
