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

// One (source pixel, 8-channel vector) pair: E's nine vectors from the 6 x 6 window of dz.
template <typename T>
__device__ __forceinline__ void upconv_adj_pair(const T* __restrict__ dz, long lddz, T* __restrict__ E, int h, int w, int nvec,
                                                int b, int i, int j, int v) {
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
    const T* rowp = db + (long)yc * W2 * lddz;
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
  upconv_adj_pair<T>(dz, lddz, E, h, w, nvec, b, row - b * h, j, v);
}

// ---- the same E by walking down the rows, and the column sums of dz on the way ----
// Source rows i and i + 1 share four of their six window rows, and a window row's partial sums hs depend on the column
// alone.  So a thread keeps its (j, v), walks down the source rows i0 .. i1-1 of one image segment with the partial sums
// of the six window rows in registers (a ring of six slots, two replaced per step), and per source row loads the two new dz
// rows only: 12 loads and two x passes instead of 36 and six.  The y pass is the fmaf chain of upconv_adj_pair over the four
// window rows of each ky in ascending order, from zero: the same bits.

// The x pass of one window row: its six vectors as loaded -> the three horizontal partial sums hs[kx], an fmaf chain over the
// window columns in ascending order, as in upconv_adj_pair; a pixel outside the map enters as zero (by selects: keep_if
// compiles to a branch per vector here, which costs the walk registers).  centre: also add window columns 2 and 3 (upsampled
// pixels 2j, 2j+1) onto cs.
template <typename T>
__device__ __forceinline__ void upconv_adj_x_pass(Raw8<T>* raw, bool yok, const bool* xok, const float* wx, float (*hs)[8],
                                                  bool centre, float* cs) {
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int k = 0; k < 8; ++k) hs[kx][k] = 0.f;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    raw[c].a = (yok && xok[c]) ? raw[c].a : decltype(raw[c].a){};
    float t[8];
    raw[c].unpack(t);
    if (centre && (c == 2 || c == 3)) {
#pragma unroll
      for (int k = 0; k < 8; ++k) cs[k] += t[k];
    }
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int a = c - kx;  // window column c is destination 2j-1+a moved by tap kx
      if (a < 0 || a > 3) continue;
#pragma unroll
      for (int k = 0; k < 8; ++k) hs[kx][k] = fmaf(wx[a], t[k], hs[kx][k]);
    }
  }
}

// the six window columns 2j-2 .. 2j+3 of source column j: inside the map?, and clamped
__device__ __forceinline__ void window_cols(int j, int W2, bool* xok, int* xc) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int X = 2 * j - 2 + c;
    xok[c] = X >= 0 && X < W2;
    xc[c] = X < 0 ? 0 : (X >= W2 ? W2 - 1 : X);
  }
}

// dz row Y (clamped into the map: always readable) at one thread's six window columns: a row base that is the same in every
// lane plus six 32-bit byte offsets (the host checks that a row of dz stays below 2^31 elements)
template <typename T>
__device__ __forceinline__ void upconv_adj_load_row(Raw8<T>* raw, const T* img, long rowstride, int Y, int H2, const unsigned* off) {
  const char* rowb = reinterpret_cast<const char*>(img + (long)(Y < 0 ? 0 : (Y >= H2 ? H2 - 1 : Y)) * rowstride);
#pragma unroll
  for (int c = 0; c < 6; ++c) raw[c].load(reinterpret_cast<const T*>(rowb + off[c]));
}

// two window rows as loaded -> their partial sums hs0, hs1; where sum is set their pixels 2j, 2j+1, added up in registers
// first, go onto the thread's column sums cs[k * 256] in LDS
template <typename T>
__device__ __forceinline__ void upconv_adj_x_pass2(Raw8<T>* raw, bool yok, const bool* xok, const float* wx, float (*hs0)[8],
                                                   float (*hs1)[8], bool sum, float* cs) {
  float rs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) rs[k] = 0.f;
  upconv_adj_x_pass<T>(raw, yok, xok, wx, hs0, sum, rs);
  upconv_adj_x_pass<T>(raw + 6, yok, xok, wx, hs1, sum, rs);
#pragma unroll
  for (int k = 0; k < 8; ++k) cs[k * 256] += rs[k];
}

// One step of the walk, for source row i with the window's rows 0 .. 5 in slots (2 PH + r) % 6 and raw holding rows 4, 5
// (dz rows 2i+2, 2i+3), which go to the column sums here: every dz row is x-passed as a row 4 or 5 by exactly one step of
// exactly one segment (rows 0 and 1 of an image: by the warm-up of its first segment), so every upsampled pixel is added
// once.  The next step's two rows are requested ahead of the y pass, the second of them once ky = 0 is done and window row 0
// is dead (that keeps the kernel inside 256 registers); after a segment's last step they are not used.
template <typename T, int PH>
__device__ __forceinline__ void upconv_adj_step(Raw8<T>* raw, float (*hs)[3][8], const T* img, long rowstride, int h, int i,
                                                const bool* xok, const float* wx, const unsigned* off, T* dst, long N, float* cs) {
  upconv_adj_x_pass2<T>(raw, i + 1 < h, xok, wx, hs[(2 * PH + 4) % 6], hs[(2 * PH + 5) % 6], true, cs);
  upconv_adj_load_row<T>(raw, img, rowstride, 2 * i + 4, 2 * h, off);
  float wy[4];
  ut_weights(i, h, wy);
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      float acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = fmaf(wy[a], hs[(2 * PH + ky + a) % 6][kx][k], acc[k]);
      store8(dst + (ky * 3 + kx) * N, acc);
    }
    if (ky == 0) upconv_adj_load_row<T>(raw + 6, img, rowstride, 2 * i + 5, 2 * h, off);
  }
}

// source rows i0 .. i1-1 of column j, vector v, image b.  The warm-up builds window rows 0 .. 3 of source row i0 without storing.
template <typename T>
__device__ __forceinline__ void upconv_adj_walk(const T* __restrict__ dz, long lddz, T* __restrict__ E, int h, int w, int nvec,
                                                int b, int i0, int i1, int j, int v, float* cs) {
  const int H2 = 2 * h, W2 = 2 * w;
  float wx[4];
  ut_weights(j, w, wx);
  int xc[6];
  bool xok[6];
  window_cols(j, W2, xok, xc);
  unsigned off[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) off[c] = (unsigned)(xc[c] * (int)lddz + v * 8) * (unsigned)sizeof(T);
  const long rowstride = (long)W2 * lddz, N = (long)nvec * 8, dstep = (long)w * 9 * N;
  const T* img = dz + (long)b * H2 * rowstride;
  T* dst = E + (((long)b * h + i0) * w + j) * (9 * N) + v * 8;
  float hs[6][3][8];
  Raw8<T> raw[12];
  upconv_adj_load_row<T>(raw, img, rowstride, 2 * i0 - 2, H2, off);
  upconv_adj_load_row<T>(raw + 6, img, rowstride, 2 * i0 - 1, H2, off);
  upconv_adj_x_pass2<T>(raw, i0 > 0, xok, wx, hs[0], hs[1], false, cs);
  upconv_adj_load_row<T>(raw, img, rowstride, 2 * i0, H2, off);
  upconv_adj_load_row<T>(raw + 6, img, rowstride, 2 * i0 + 1, H2, off);
  upconv_adj_x_pass2<T>(raw, true, xok, wx, hs[2], hs[3], i0 == 0, cs);
  upconv_adj_load_row<T>(raw, img, rowstride, 2 * i0 + 2, H2, off);
  upconv_adj_load_row<T>(raw + 6, img, rowstride, 2 * i0 + 3, H2, off);
  for (int i = i0;;) {  // three steps: every slot index is static
    upconv_adj_step<T, 0>(raw, hs, img, rowstride, h, i, xok, wx, off, dst, N, cs);
    dst += dstep;
    if (++i == i1) break;
    upconv_adj_step<T, 1>(raw, hs, img, rowstride, h, i, xok, wx, off, dst, N, cs);
    dst += dstep;
    if (++i == i1) break;
    upconv_adj_step<T, 2>(raw, hs, img, rowstride, h, i, xok, wx, off, dst, N, cs);
    dst += dstep;
    if (++i == i1) break;
  }
}

// An image is cut into nseg segments of seg_rows source rows (the last one may be shorter), a row of pixels into chunks of
// ppc = 256 / nvec whole pixels (nvec <= 256).  Workgroup (b, s, y), dealt so that every XCD gets one contiguous run of them
// (y fastest: neighbours in a row share window columns), walks segment s of image b for the chunks y, y + G, ...; a thread
// keeps its vector v throughout and adds the dz rows it x-passes onto its own eight sums.  The workgroup's threads of
// one v are then summed in thread order by the first of them into partial[(b * nseg + s) * G + y][v * 8 ..]: a fixed order.
template <typename T>
__global__ __launch_bounds__(256, 2) void upconv_adj_colsum_kernel(const T* __restrict__ dz, long lddz, T* __restrict__ E, int h,
                                                                int w, int nvec, int seg_rows, int nseg, int G,
                                                                float* __restrict__ partial) {
  const int ppc = 256 / nvec;
  const int jl = threadIdx.x / nvec;
  const int v = threadIdx.x - jl * nvec;
  // the same in every lane: row addresses and the walk's bounds stay in scalar registers
  const int work = __builtin_amdgcn_readfirstlane(xcd_row(blockIdx.x, gridDim.x));
  const int bs = __builtin_amdgcn_readfirstlane(work / G);
  const int y = work - bs * G;
  const int b = __builtin_amdgcn_readfirstlane(bs / nseg);
  const int i0 = (bs - b * nseg) * seg_rows;
  const int i1 = i0 + seg_rows < h ? i0 + seg_rows : h;
  __shared__ float red[8 * 256];  // [k][thread]
#pragma unroll
  for (int k = 0; k < 8; ++k) red[k * 256 + threadIdx.x] = 0.f;
  if (jl < ppc) {
    for (int c = y; c * ppc < w; c += G) {  // the chunk is the same in every lane: nothing per lane is carried from walk to walk
      const int j = c * ppc + jl;
      if (j < w) upconv_adj_walk<T>(dz, lddz, E, h, w, nvec, b, i0, i1, j, v, red + threadIdx.x);
    }
  }
  __syncthreads();
  if (jl == 0) {
    float cs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cs[k] = red[k * 256 + v];
    for (int r = 1; r < ppc; ++r)
#pragma unroll
      for (int k = 0; k < 8; ++k) cs[k] += red[k * 256 + r * nvec + v];
    store8(partial + (long)work * ((long)nvec * 8) + v * 8, cs);
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
// partial rows of the column sums per source row: as many as keep them near 4096 in all (B*h = 2048 rows of the benchmark's
// passes: 2), at most one per chunk.  The workspace holds B * h * cs_groups rows; a launch uses B * nseg * G of them.
static inline long cs_chunks(int w, int N) { return vkas_cdiv(w, 256 / (N / 8)); }
static inline long cs_groups(int B, int h, int w, int N) {
  const long chunks = cs_chunks(w, N);
  long g = 4096 / ((long)B * h);
  g = g < 1 ? 1 : g;
  return g < chunks ? g : chunks;
}
// workgroups per (image, segment): one per chunk where the workspace has the rows for it
static inline long cs_seg_groups(int B, int h, int w, int N, long nseg) {
  const long chunks = cs_chunks(w, N), room = (long)h * cs_groups(B, h, w, N) / nseg;
  return room < chunks ? room : chunks;
}
// The segment length of the plain entry.  Two 256-thread workgroups fit a CU (two waves per SIMD), 512 on the MI355X's 256
// CUs, and all workgroups of a launch take about the same time, so a launch runs in ceil(workgroups / 512) rounds of
// (walks per workgroup) * (seg_rows + 2) row steps each - the warm-up of a walk loads and x-passes four rows, two steps'
// worth.  Take the length with the fewest row steps among those that fill every CU twice (if any does); ties: the longer.
static inline int cs_seg_rows(int B, int h, int w, int N) {
  const long chunks = cs_chunks(w, N), slots = 2 * 256;
  long best = h, best_cost = -1;
  bool best_full = false;
  for (long seg = h; seg >= 1; --seg) {
    const long nseg = vkas_cdiv(h, seg);
    if (vkas_cdiv(h, nseg) != seg) continue;  // the same cut with a shorter last segment
    const long G = cs_seg_groups(B, h, w, N, nseg), wgs = (long)B * nseg * G;
    const long cost = vkas_cdiv(wgs, slots) * vkas_cdiv(chunks, G) * (seg + 2);
    const bool full = wgs >= slots;
    if (best_cost < 0 || (full && !best_full) || (full == best_full && cost < best_cost)) {
      best = seg; best_cost = cost; best_full = full;
    }
  }
  return (int)best;
}

static int colsum_seg(const char* who, const void* dz, long lddz, void* E, int B, int h, int w, int N, float* out, int accumulate,
                      float* ws, size_t ws_bytes, int dtype, void* stream, int seg_rows) {
  VKAS_CHECK(dz && E && out && ws && vkas_aligned16(dz) && vkas_aligned16(E) && vkas_aligned16(ws),
             "%s: null/misaligned pointer", who);
  VKAS_CHECK(B > 0 && h > 0 && w > 0 && (long)B * h < (1L << 31) && 2L * w * lddz < (1L << 31), "%s: bad spatial dims", who);
  VKAS_CHECK(N > 0 && N % 8 == 0 && N <= 2048 && lddz >= N && lddz % 8 == 0, "%s: bad channels/stride (N=%d lddz=%ld)", who, N,
             lddz);
  VKAS_CHECK(dtype == VKAS_BF16 || dtype == VKAS_F16, "%s: 16-bit storage only", who);
  VKAS_CHECK(ws_bytes >= vkas_upconv_adj_colsum_ws_bytes(B, h, w, N), "%s: workspace too small", who);
  VKAS_CHECK(seg_rows >= 0, "%s: bad segment length %d", who, seg_rows);
  if (seg_rows == 0) seg_rows = cs_seg_rows(B, h, w, N);
  if (seg_rows > h) seg_rows = h;
  const long nseg = vkas_cdiv(h, seg_rows), G = cs_seg_groups(B, h, w, N, nseg), P = (long)B * nseg * G;
  hipStream_t st = vkas_stream(stream);
  if (dtype == VKAS_BF16)
    upconv_adj_colsum_kernel<bf16_t><<<(unsigned)P, 256, 0, st>>>((const bf16_t*)dz, lddz, (bf16_t*)E, h, w, N / 8, seg_rows,
                                                                  (int)nseg, (int)G, ws);
  else
    upconv_adj_colsum_kernel<f16_t><<<(unsigned)P, 256, 0, st>>>((const f16_t*)dz, lddz, (f16_t*)E, h, w, N / 8, seg_rows,
                                                                 (int)nseg, (int)G, ws);
  VKAS_LAUNCH_CHECK(who);
  return vkas_colreduce_finalize(ws, P, N, N, out, accumulate, st);
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
  return colsum_seg("vkas_upconv_adj_colsum", dz, lddz, E, B, h, w, N, out, accumulate, ws, ws_bytes, dtype, stream, 0);
}

// the same with the segment length given (0: the plain entry's rule; longer than the image: one segment)
extern "C" int vkas_upconv_adj_colsum_seg(const void* dz, long lddz, void* E, int B, int h, int w, int N, float* out,
                                          int accumulate, float* ws, size_t ws_bytes, int dtype, void* stream, int seg_rows) {
  return colsum_seg("vkas_upconv_adj_colsum_seg", dz, lddz, E, B, h, w, N, out, accumulate, ws, ws_bytes, dtype, stream, seg_rows);
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
