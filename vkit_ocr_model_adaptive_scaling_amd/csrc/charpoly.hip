// Character quadrilaterals from the precise maps (inferencing/adaptive_scaling.py:399-465,481-491): the peaks of the char
// probability map (scipy maximum_filter + threshold) and, for each peak, the up-left / up-right / down-right / down-left
// corners built from the offset, angle-distribution and distance maps at that pixel.  The reference downloads every map and
// runs scipy and a Python loop per character; here four launches leave only the peak count and the peak rows on the device.
//
//   cp_rowmax_kernel   rowmax = max of prob over the window [x - s/2, x + s - 1 - s/2] clamped to the row (scipy's
//                      'reflect' border never brings in a value from outside that range, so clamping is exact)
//   cp_flag_kernel     colmax over the same window in y; peak = prob == colmax && !(prob < thr).  Block k owns the flat
//                      pixels [k*1024, (k+1)*1024), so block order is (b, y, x) order: one 64-bit ballot per wave and step
//                      is kept, and the block's peak count.
//   cp_scan_kernel     one block: exclusive scan of the block counts, and the total
//   cp_scatter_kernel  each peak's slot = block offset + the peaks in front of it in its block (ballot popcounts); the
//                      thread writes (b, y, x), prob and the quadrilateral
// No atomics: the output order is np.nonzero's and eager runs equal graph replays bit for bit.  Capacity B*H*W (an
// all-plateau map) means there is no overflow path.
#include "vkas_common.h"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_STEPS = 4;
constexpr int CP_CHUNK = CP_THREADS * CP_STEPS;     // flat pixels per block of the flag / scatter passes
constexpr int CP_WORDS = CP_CHUNK / 64;             // ballot words per block, in flat order
constexpr int CP_SCAN_THREADS = 1024;
constexpr float CP_TWO_PI = 6.28318530717958647692f;  // (float)(2 * pi), as numpy casts the Python float

__device__ __forceinline__ int cp_lo(int c, int size) { return max(0, c - size / 2); }
__device__ __forceinline__ int cp_hi(int c, int size, int n) { return min(n - 1, c + size - 1 - size / 2); }

// numpy's float32 floor-mod (npy_divmodf): fmod, moved into the divisor's sign, +0 for an exact multiple
__device__ __forceinline__ float cp_mod_2pi(float a) {
  float m = fmodf(a, CP_TWO_PI);
  if (m != 0.f) {
    if (m < 0.f) m = __fadd_rn(m, CP_TWO_PI);
  } else {
    m = 0.f;
  }
  return m;
}

__global__ __launch_bounds__(CP_THREADS) void cp_rowmax_kernel(const float* __restrict__ prob, long n, int W, int size,
                                                                float* __restrict__ rowmax) {
  for (long i = (long)blockIdx.x * CP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * CP_THREADS) {
    const int x = (int)(i % W);
    const float* row = prob + (i - x);
    const int hi = cp_hi(x, size, W);
    float m = row[cp_lo(x, size)];
    for (int k = cp_lo(x, size) + 1; k <= hi; ++k) m = fmaxf(m, row[k]);
    rowmax[i] = m;
  }
}

__global__ __launch_bounds__(CP_THREADS) void cp_flag_kernel(const float* __restrict__ prob,
                                                              const float* __restrict__ rowmax, long n, int H, int W,
                                                              int size, float thr, unsigned long long* __restrict__ words,
                                                              int* __restrict__ counts) {
  __shared__ int wave_count[CP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
  for (int s = 0; s < CP_STEPS; ++s) {
    const long i = (long)blockIdx.x * CP_CHUNK + s * CP_THREADS + threadIdx.x;
    bool peak = false;
    if (i < n) {
      const int x = (int)(i % W);
      const long r = i / W;
      const int y = (int)(r % H);
      const float* col = rowmax + (r - y) * W + x;  // column x of page b
      const int hi = cp_hi(y, size, H);
      float m = col[(long)cp_lo(y, size) * W];
      for (int k = cp_lo(y, size) + 1; k <= hi; ++k) m = fmaxf(m, col[(long)k * W]);
      const float p = prob[i];
      peak = p == m && !(p < thr);
    }
    const unsigned long long bits = __ballot(peak);
    if (lane == 0) words[(long)blockIdx.x * CP_WORDS + s * (CP_THREADS / 64) + wave] = bits;
    cnt += __popcll(bits);
  }
  if (lane == 0) wave_count[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < CP_THREADS / 64; ++w) t += wave_count[w];
    counts[blockIdx.x] = t;
  }
}

// one block: offsets[k] = counts[0] + ... + counts[k-1], *total = the sum of all; each thread owns a contiguous run of blocks
__global__ __launch_bounds__(CP_SCAN_THREADS) void cp_scan_kernel(const int* __restrict__ counts, int nblk,
                                                                  int* __restrict__ offsets, int* __restrict__ total) {
  __shared__ int wave_sum[CP_SCAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int seg = (nblk + CP_SCAN_THREADS - 1) / CP_SCAN_THREADS;
  const int lo = min(nblk, t * seg), hi = min(nblk, lo + seg);
  int own = 0;
  for (int k = lo; k < hi; ++k) own += counts[k];
  int v = own;  // inclusive scan over the wave
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  if (lane == 63) wave_sum[wave] = v;
  __syncthreads();
  int run = v - own, all = 0;
  for (int w = 0; w < CP_SCAN_THREADS / 64; ++w) {
    if (w < wave) run += wave_sum[w];
    all += wave_sum[w];
  }
  for (int k = lo; k < hi; ++k) {
    offsets[k] = run;
    run += counts[k];
  }
  if (t == 0) *total = all;
}

__global__ __launch_bounds__(CP_THREADS) void cp_scatter_kernel(const float* __restrict__ prob,
                                                                 const float* __restrict__ offset,
                                                                 const float* __restrict__ angle,
                                                                 const float* __restrict__ dist, long n, int H, int W,
                                                                 float scale_y, float scale_x,
                                                                 const unsigned long long* __restrict__ words,
                                                                 const int* __restrict__ offsets, int* __restrict__ points,
                                                                 float* __restrict__ probs, float* __restrict__ quads) {
  __shared__ unsigned long long w_bits[CP_WORDS];
  __shared__ int w_before[CP_WORDS];
  if (threadIdx.x < CP_WORDS) w_bits[threadIdx.x] = words[(long)blockIdx.x * CP_WORDS + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = offsets[blockIdx.x];
    for (int k = 0; k < CP_WORDS; ++k) {
      w_before[k] = t;
      t += __popcll(w_bits[k]);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = 0; s < CP_STEPS; ++s) {
    const int k = s * (CP_THREADS / 64) + wave;
    const unsigned long long bits = w_bits[k];
    if (!((bits >> lane) & 1ull)) continue;
    const long i = (long)blockIdx.x * CP_CHUNK + s * CP_THREADS + threadIdx.x;  // < n: only pixels < n were flagged
    const long pos = w_before[k] + __popcll(bits & ((1ull << lane) - 1ull));
    const int x = (int)(i % W);
    const long r = i / W;
    const int y = (int)(r % H), b = (int)(r / H);
    points[pos * 3 + 0] = b;
    points[pos * 3 + 1] = y;
    points[pos * 3 + 2] = x;
    probs[pos] = prob[i];
    // :399-465 in float32, products rounded before the sums as numpy does (no contraction into fma)
    const float py = __fmul_rn((float)y, scale_y), px = __fmul_rn((float)x, scale_x);
    const float2 o = *reinterpret_cast<const float2*>(offset + i * 2);
    const float4 a = *reinterpret_cast<const float4*>(angle + i * 4);
    const float4 d = *reinterpret_cast<const float4*>(dist + i * 4);
    float theta = cp_mod_2pi(atan2f(o.x, o.y));
    float c[6];
    const float frac[3] = {a.x, a.y, a.z}, len[3] = {d.y, d.z, d.w};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      theta = cp_mod_2pi(__fadd_rn(theta, __fmul_rn(frac[q], CP_TWO_PI)));
      c[2 * q] = __fadd_rn(py, __fmul_rn(sinf(theta), len[q]));
      c[2 * q + 1] = __fadd_rn(px, __fmul_rn(cosf(theta), len[q]));
    }
    float4* out = reinterpret_cast<float4*>(quads + pos * 8);
    out[0] = make_float4(__fadd_rn(py, o.x), __fadd_rn(px, o.y), c[0], c[1]);
    out[1] = make_float4(c[2], c[3], c[4], c[5]);
  }
}

static size_t cp_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct CpLayout {
  size_t rowmax, words, counts, offsets, bytes;
};

static CpLayout cp_layout(long n) {
  const long nblk = vkas_cdiv(n, CP_CHUNK);
  CpLayout l;
  l.rowmax = 0;
  l.words = cp_align(l.rowmax + (size_t)n * sizeof(float));
  l.counts = cp_align(l.words + (size_t)nblk * CP_WORDS * sizeof(unsigned long long));
  l.offsets = cp_align(l.counts + (size_t)nblk * sizeof(int));
  l.bytes = cp_align(l.offsets + (size_t)nblk * sizeof(int));
  return l;
}

static int cp_check_dims(const char* what, int B, int H, int W, int size) {
  VKAS_CHECK(B >= 0 && H > 0 && W > 0, "%s: bad dims B=%d H=%d W=%d", what, B, H, W);
  VKAS_CHECK((long)B * H * W < (1L << 31), "%s: B*H*W = %ld must stay below 2^31", what, (long)B * H * W);
  VKAS_CHECK(size >= 1, "%s: maximum filter size %d must be >= 1", what, size);
  return VKAS_OK;
}

}  // namespace

extern "C" long vkas_char_polygons_workspace_bytes(int B, int H, int W, int size) {
  if (cp_check_dims("vkas_char_polygons_workspace_bytes", B, H, W, size) != VKAS_OK) return -1;
  return (long)cp_layout((long)B * H * W).bytes;
}

extern "C" int vkas_char_polygons(const float* prob, const float* offset, const float* angle, const float* dist, int B,
                                  int H, int W, int size, float thr, float scale_y, float scale_x, void* workspace,
                                  size_t workspace_bytes, int* count, int* points, float* probs, float* quads,
                                  void* stream) {
  VKAS_CHECK(prob && offset && angle && dist && workspace && count && points && probs && quads,
             "vkas_char_polygons: null pointer");
  const int rc = cp_check_dims("vkas_char_polygons", B, H, W, size);
  if (rc != VKAS_OK) return rc;
  const long n = (long)B * H * W;
  const CpLayout l = cp_layout(n);
  VKAS_CHECK(workspace_bytes >= l.bytes, "vkas_char_polygons: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  VKAS_CHECK(vkas_aligned16(workspace) && vkas_aligned16(angle) && vkas_aligned16(dist) && vkas_aligned16(quads) &&
                 (((uintptr_t)offset) & 7u) == 0,
             "vkas_char_polygons: workspace, angle, dist and quads must be 16-byte aligned, offset 8-byte aligned");
  char* ws = static_cast<char*>(workspace);
  float* rowmax = reinterpret_cast<float*>(ws + l.rowmax);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + l.words);
  int* counts = reinterpret_cast<int*>(ws + l.counts);
  int* offsets = reinterpret_cast<int*>(ws + l.offsets);
  const int nblk = (int)vkas_cdiv(n, CP_CHUNK);
  hipStream_t s = vkas_stream(stream);
  if (n > 0) {
    long g = vkas_cdiv(n, CP_THREADS * 4);
    cp_rowmax_kernel<<<(unsigned)(g > 4096 ? 4096 : g), CP_THREADS, 0, s>>>(prob, n, W, size, rowmax);
    VKAS_LAUNCH_CHECK("char_polygons rowmax");
    cp_flag_kernel<<<nblk, CP_THREADS, 0, s>>>(prob, rowmax, n, H, W, size, thr, words, counts);
    VKAS_LAUNCH_CHECK("char_polygons flag");
  }
  cp_scan_kernel<<<1, CP_SCAN_THREADS, 0, s>>>(counts, nblk, offsets, count);  // B = 0: writes a count of 0
  VKAS_LAUNCH_CHECK("char_polygons scan");
  if (n > 0) {
    cp_scatter_kernel<<<nblk, CP_THREADS, 0, s>>>(prob, offset, angle, dist, n, H, W, scale_y, scale_x, words, offsets,
                                                  points, probs, quads);
    VKAS_LAUNCH_CHECK("char_polygons scatter");
  }
  return VKAS_OK;
}
