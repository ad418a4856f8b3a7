// Orientation of the text regions (inferencing/orient.py states the rule and holds the host oracles): the raw second-order
// moments of every region of a label map, and the extents of every region along a given direction.  Both are exact integer
// reductions keyed by the pixel's label.
//
// A thread reads four adjacent pixels of one row (one 16-byte load when the row allows) and folds equal-label runs in
// registers.  A run that ends inside the thread's quad goes to global memory at once (rare: a region edge); the run that is
// still open at the end of the quad is folded across the wave first - the wave takes the label of its first pending lane,
// every lane holding that label joins one butterfly, lane 0 issues the atomics, repeat until no lane is pending - so a large
// region costs one set of atomics per wave rather than per pixel.  Only integer vector atomics on global memory are used
// (64-bit add, 32-bit min / max): the results do not depend on the order and two calls give the same bytes.
#include <climits>

#include "vkas_common.h"

namespace {

constexpr int THREADS = 256, QUAD = 4;
constexpr int DIM_MAX = 32768;

typedef unsigned long long u64;

struct MomentAcc {
  long long v[6];  // n, sum y, sum x, sum y^2, sum x^2, sum x*y
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0;
  }
  __device__ __forceinline__ void add(long long y, long long x, const int*, long) {
    v[0] += 1; v[1] += y; v[2] += x; v[3] += y * y; v[4] += x * x; v[5] += x * y;
  }
  __device__ __forceinline__ void fold(int offset) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += __shfl_xor(v[k], offset);
  }
  __device__ __forceinline__ void commit(void* out, long row) const {
    u64* o = reinterpret_cast<u64*>(out) + row * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) atomicAdd(o + k, (u64)v[k]);
  }
};

struct ExtentAcc {
  int lo_u, hi_u, lo_v, hi_v;
  __device__ __forceinline__ void clear() { lo_u = lo_v = INT_MAX; hi_u = hi_v = INT_MIN; }
  __device__ __forceinline__ void add(int y, int x, const int* dirs, long row) {
    const int c = dirs[row * 2], s = dirs[row * 2 + 1];
    const int u = c * x + s * y, v = c * y - s * x;
    lo_u = min(lo_u, u); hi_u = max(hi_u, u); lo_v = min(lo_v, v); hi_v = max(hi_v, v);
  }
  __device__ __forceinline__ void fold(int offset) {
    lo_u = min(lo_u, __shfl_xor(lo_u, offset)); hi_u = max(hi_u, __shfl_xor(hi_u, offset));
    lo_v = min(lo_v, __shfl_xor(lo_v, offset)); hi_v = max(hi_v, __shfl_xor(hi_v, offset));
  }
  __device__ __forceinline__ void commit(void* out, long row) const {
    int* o = reinterpret_cast<int*>(out) + row * 4;
    atomicMin(o, lo_u); atomicMax(o + 1, hi_u); atomicMin(o + 2, lo_v); atomicMax(o + 3, hi_v);
  }
};

// labels (B,H,W); one image per blockIdx.y; thread t of the image owns pixels [4t, 4t + 4) of the row-major quads of a row
template <class Acc>
__global__ __launch_bounds__(THREADS) void region_reduce_kernel(const int* __restrict__ labels, int H, int W, int R,
                                                                const int* __restrict__ dirs, void* __restrict__ out,
                                                                int vec_loads) {
  const int b = blockIdx.y;
  const int quads_per_row = (W + QUAD - 1) / QUAD;
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  const long total = (long)H * quads_per_row;
  const long row_base = (long)b * R;  // table row of region 1 of this image
  int lab[QUAD] = {0, 0, 0, 0};
  int y = 0, x0 = 0;
  if (t < total) {
    y = (int)(t / quads_per_row);
    x0 = (int)(t % quads_per_row) * QUAD;
    const int* p = labels + ((long)b * H + y) * W + x0;
    if (vec_loads) {
      const int4 q = *reinterpret_cast<const int4*>(p);
      lab[0] = q.x; lab[1] = q.y; lab[2] = q.z; lab[3] = q.w;
    } else {
#pragma unroll
      for (int q = 0; q < QUAD; ++q)
        if (x0 + q < W) lab[q] = p[q];
    }
  }
  Acc acc;
  acc.clear();
  int cur = 0;  // the label of the open run, 0: none
#pragma unroll
  for (int q = 0; q < QUAD; ++q) {
    const int l = (lab[q] >= 1 && lab[q] <= R) ? lab[q] : 0;
    if (l != cur) {
      if (cur) acc.commit(out, row_base + cur - 1);
      acc.clear();
      cur = l;
    }
    if (l) acc.add(y, x0 + q, dirs, row_base + l - 1);
  }
  // the open runs of the wave, one label at a time (the loop condition is wave-uniform)
  const int lane = threadIdx.x & 63;
  bool pending = cur != 0;
  for (;;) {
    const u64 mask = __ballot(pending);
    if (!mask) break;
    const int leader = __ffsll((long long)mask) - 1;
    const int l = __shfl(cur, leader);
    const bool mine = pending && cur == l;
    Acc part = acc;
    if (!mine) part.clear();
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) part.fold(offset);
    if (lane == 0) part.commit(out, row_base + l - 1);
    if (mine) pending = false;
  }
}

__global__ void extents_init_kernel(int* __restrict__ out, long rows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) *reinterpret_cast<int4*>(out + i * 4) = make_int4(INT_MAX, INT_MIN, INT_MAX, INT_MIN);
}

// the table is cleared by a kernel, like every other table of the inference path: a captured graph then holds kernel nodes only
__global__ void moments_init_kernel(u64* __restrict__ out, long words) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) out[i] = 0ull;
}

int check_dims(const char* who, int B, int H, int W, int R) {
  VKAS_CHECK(B >= 1 && H >= 1 && W >= 1 && R >= 1, "%s: bad dims B %d H %d W %d R %d", who, B, H, W, R);
  VKAS_CHECK(H <= DIM_MAX && W <= DIM_MAX, "%s: map sides must not exceed %d", who, DIM_MAX);
  VKAS_CHECK(B <= 65535, "%s: at most 65535 images", who);
  VKAS_CHECK((long)B * H * W < (1L << 31) && (long)B * R < (1L << 31), "%s: B*H*W and B*R must stay below 2^31", who);
  return VKAS_OK;
}

template <class Acc>
void launch_reduce(const int* labels, int B, int H, int W, int R, const int* dirs, void* out, void* stream) {
  const long quads = (long)H * vkas_cdiv(W, QUAD);
  const int vec_loads = (W % QUAD == 0) && vkas_aligned16(labels);
  const dim3 grid((unsigned)vkas_cdiv(quads, THREADS), (unsigned)B);
  region_reduce_kernel<Acc><<<grid, THREADS, 0, vkas_stream(stream)>>>(labels, H, W, R, dirs, out, vec_loads);
}

}  // namespace

extern "C" int vkas_region_moments(const int* labels, int B, int H, int W, int max_regions, long long* moments,
                                   void* stream) {
  VKAS_CHECK(labels && moments, "vkas_region_moments: null pointer");
  if (const int rc = check_dims("vkas_region_moments", B, H, W, max_regions)) return rc;
  VKAS_CHECK((((uintptr_t)moments) & 7u) == 0, "vkas_region_moments: the table must be 8-byte aligned");
  const long words = (long)B * max_regions * 6;
  moments_init_kernel<<<(unsigned)vkas_cdiv(words, 256), 256, 0, vkas_stream(stream)>>>(reinterpret_cast<u64*>(moments), words);
  VKAS_LAUNCH_CHECK("region_moments init");
  launch_reduce<MomentAcc>(labels, B, H, W, max_regions, nullptr, moments, stream);
  VKAS_LAUNCH_CHECK("region_moments");
  return VKAS_OK;
}

extern "C" int vkas_region_extents(const int* labels, int B, int H, int W, int max_regions, const int* dirs, int* extents,
                                   void* stream) {
  VKAS_CHECK(labels && dirs && extents, "vkas_region_extents: null pointer");
  if (const int rc = check_dims("vkas_region_extents", B, H, W, max_regions)) return rc;
  VKAS_CHECK(vkas_aligned16(extents), "vkas_region_extents: the table must be 16-byte aligned");
  const long rows = (long)B * max_regions;
  extents_init_kernel<<<(unsigned)vkas_cdiv(rows, 256), 256, 0, vkas_stream(stream)>>>(extents, rows);
  VKAS_LAUNCH_CHECK("region_extents init");
  launch_reduce<ExtentAcc>(labels, B, H, W, max_regions, dirs, extents, stream);
  VKAS_LAUNCH_CHECK("region_extents");
  return VKAS_OK;
}
