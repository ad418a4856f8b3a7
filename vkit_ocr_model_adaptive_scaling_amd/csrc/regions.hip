// Text regions of the rough character mask and the median character height of each (the step between the two passes,
// inferencing/adaptive_scaling.py:190-279, restated on pixels): a region is an 8-connected component of mask != 0, regions
// are numbered 1..N by their first pixel in row-major order, and each gets its inclusive box, its area, the number of its
// pixels with height > 0 and the exact fp32 median of those heights.  Ten launches on one stream:
//
//   tr_init_kernel      table rows: boxes to (max, max, -1, -1), areas and valid to 0
//   tr_tile_kernel      one 64 x 16 tile per workgroup: union-find over the tile's pixels in LDS (links to W, NW, N, NE, the
//                       larger root under the smaller by atomicMin), then parent[pixel] = the flat index of its tile root
//   tr_seam_kernel      the same four links where they cross a tile seam or corner, on the global parent array
//   tr_flatten_kernel   labels[pixel] = root (the component's smallest flat index), -1 on background; roots per 1024-pixel chunk
//   tr_scan_kernel      per image: exclusive scan of the chunk counts, count[b] = the true number of components
//   tr_number_kernel    rootnum[root] = 1 + the roots in front of it in its image (chunk offset + ballot popcounts)
//   tr_table_kernel     labels[pixel] = rootnum[root] (0 on background); box / area / valid of regions 1..max_regions by
//                       integer atomics, one set per run of equal labels in a wave (rows of one label are the common case)
//   tr_offsets_kernel   per image: exclusive scan of valid[] = where each region's heights start; cursors to 0
//   tr_gather_kernel    the bit patterns of the valid heights, grouped by region (one atomicAdd per run reserves its slots; the
//                       order inside a region depends on arrival, the median does not)
//   tr_median_kernel    one workgroup per table row: radix select on the bit patterns (positive floats order as unsigned
//                       integers; four 8-bit passes with a 256-bin LDS histogram) for the lower middle element, the upper
//                       one from the counts or one more pass; rows beyond the image's count are zeroed
//
// Integer atomics only: every output is bit-identical from run to run.  Nothing persists between calls - every workspace word
// that is read was written earlier in the same call - and ordering comes from the kernel boundaries alone, so the call can be
// captured into a HIP graph and replayed.
#include "vkas_common.h"

#include <limits.h>

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_TW = 64, TR_TH = 16;               // tile of the LDS labelling pass
constexpr int TR_TILE = TR_TW * TR_TH;
constexpr int TR_CHUNK = 1024;                       // flat pixels per workgroup of the numbering passes
constexpr int TR_STEPS = TR_CHUNK / TR_THREADS;
constexpr int TR_WORDS = TR_CHUNK / 64;
constexpr int TR_SCAN_THREADS = 1024;

__global__ __launch_bounds__(TR_THREADS) void tr_init_kernel(int rows, int* __restrict__ boxes, int* __restrict__ areas,
                                                              int* __restrict__ valid) {
  const int r = blockIdx.x * TR_THREADS + threadIdx.x;
  if (r >= rows) return;
  boxes[r * 4 + 0] = INT_MAX;
  boxes[r * 4 + 1] = INT_MAX;
  boxes[r * 4 + 2] = -1;
  boxes[r * 4 + 3] = -1;
  areas[r] = 0;
  valid[r] = 0;
}

// ---- union-find: a parent is never larger than its child, a root is its own parent; links only ever lower a parent ----------
__device__ __forceinline__ int tr_find_lds(volatile int* lab, int a) {
  int p = lab[a];
  while (p != a) {
    a = p;
    p = lab[a];
  }
  return a;
}

__device__ __forceinline__ void tr_union_lds(int* lab, int a, int b) {
  for (;;) {
    a = tr_find_lds(lab, a);
    b = tr_find_lds(lab, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&lab[a], b);  // a was a root when read: hang it under the smaller root b
    if (old == a) return;
    a = old;  // somebody linked a first: a now hangs under min(old, b), and old and b still have to be joined
  }
}

__device__ __forceinline__ int tr_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int tr_find_global(const int* parent, int a) {
  int p = tr_load(parent + a);
  while (p != a) {
    a = p;
    p = tr_load(parent + a);
  }
  return a;
}

__device__ __forceinline__ void tr_union_global(int* parent, int a, int b) {
  for (;;) {
    a = tr_find_global(parent, a);
    b = tr_find_global(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_tile_kernel(const unsigned char* __restrict__ mask, int H, int W,
                                                              int* __restrict__ parent) {
  __shared__ int lab[TR_TILE];
  const int x0 = blockIdx.x * TR_TW, y0 = blockIdx.y * TR_TH;
  const int base = blockIdx.z * H * W;  // < 2^31: checked by the caller
  for (int p = threadIdx.x; p < TR_TILE; p += TR_THREADS) {
    const int x = x0 + p % TR_TW, y = y0 + p / TR_TW;
    lab[p] = (x < W && y < H && mask[base + y * W + x] != 0) ? p : -1;
  }
  __syncthreads();
  volatile int* vlab = lab;
  for (int p = threadIdx.x; p < TR_TILE; p += TR_THREADS) {
    if (vlab[p] < 0) continue;
    const int tx = p % TR_TW, ty = p / TR_TW;
    if (tx > 0 && vlab[p - 1] >= 0) tr_union_lds(lab, p, p - 1);
    if (ty > 0) {
      if (tx > 0 && vlab[p - TR_TW - 1] >= 0) tr_union_lds(lab, p, p - TR_TW - 1);
      if (vlab[p - TR_TW] >= 0) tr_union_lds(lab, p, p - TR_TW);
      if (tx < TR_TW - 1 && vlab[p - TR_TW + 1] >= 0) tr_union_lds(lab, p, p - TR_TW + 1);
    }
  }
  __syncthreads();
  for (int p = threadIdx.x; p < TR_TILE; p += TR_THREADS) {
    const int x = x0 + p % TR_TW, y = y0 + p / TR_TW;
    if (x >= W || y >= H) continue;
    int g = -1;
    if (vlab[p] >= 0) {
      const int r = tr_find_lds(lab, p);  // the tile root: smallest tile index = smallest flat index of the tile's part
      g = base + (y0 + r / TR_TW) * W + x0 + r % TR_TW;
    }
    parent[base + y * W + x] = g;
  }
}

// one thread per pixel; only pixels in a tile's first row, first column or last column have a W / NW / N / NE neighbour in
// another tile
__global__ __launch_bounds__(TR_THREADS) void tr_seam_kernel(int H, int W, int* parent) {
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= H * W) return;
  const int x = i % W, y = i / W;
  const int tx = x % TR_TW, ty = y % TR_TH;
  if (ty != 0 && tx != 0 && tx != TR_TW - 1) return;
  const int g = blockIdx.y * H * W + i;
  if (parent[g] < 0) return;  // background stays -1 for the whole call
  if (tx == 0 && x > 0 && parent[g - 1] >= 0) tr_union_global(parent, g, g - 1);
  if (y > 0) {
    if ((ty == 0 || tx == 0) && x > 0 && parent[g - W - 1] >= 0) tr_union_global(parent, g, g - W - 1);
    if (ty == 0 && parent[g - W] >= 0) tr_union_global(parent, g, g - W);
    if ((ty == 0 || tx == TR_TW - 1) && x < W - 1 && parent[g - W + 1] >= 0) tr_union_global(parent, g, g - W + 1);
  }
}

// chunk k of image b owns the image's flat pixels [k*1024, (k+1)*1024): chunk order is row-major order
__global__ __launch_bounds__(TR_THREADS) void tr_flatten_kernel(const int* __restrict__ parent, int HW, int nchunk,
                                                                 int* __restrict__ labels, int* __restrict__ chunk_count) {
  __shared__ int wave_count[TR_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int base = blockIdx.y * HW;
  int cnt = 0;
  for (int s = 0; s < TR_STEPS; ++s) {
    const int i = blockIdx.x * TR_CHUNK + s * TR_THREADS + threadIdx.x;
    bool root = false;
    if (i < HW) {
      const int g = base + i;
      int r = parent[g];
      if (r >= 0) {
        int p = parent[r];
        while (p != r) {
          r = p;
          p = parent[r];
        }
      }
      labels[g] = r;
      root = r == g;
    }
    cnt += __popcll(__ballot(root));
  }
  if (lane == 0) wave_count[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < TR_THREADS / 64; ++w) t += wave_count[w];
    chunk_count[blockIdx.y * nchunk + blockIdx.x] = t;
  }
}

// one workgroup: out[k] = in[0] + ... + in[k-1] for k < n, returns the sum of all in every thread; each thread owns a
// contiguous run.  out may be null.
__device__ __forceinline__ int tr_block_exscan(const int* __restrict__ in, int n, int* __restrict__ out) {
  __shared__ int wave_sum[TR_SCAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int seg = (n + TR_SCAN_THREADS - 1) / TR_SCAN_THREADS;
  const int lo = min(n, t * seg), hi = min(n, lo + seg);
  int own = 0;
  for (int k = lo; k < hi; ++k) own += in[k];
  int v = own;  // inclusive scan over the wave
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  if (lane == 63) wave_sum[wave] = v;
  __syncthreads();
  int run = v - own, all = 0;
  for (int w = 0; w < TR_SCAN_THREADS / 64; ++w) {
    if (w < wave) run += wave_sum[w];
    all += wave_sum[w];
  }
  if (out) {
    for (int k = lo; k < hi; ++k) {
      const int c = in[k];
      out[k] = run;
      run += c;
    }
  }
  return all;
}

__global__ __launch_bounds__(TR_SCAN_THREADS) void tr_scan_kernel(const int* __restrict__ chunk_count, int nchunk,
                                                                  int* __restrict__ chunk_offset, int* __restrict__ count) {
  const int b = blockIdx.x;
  const int all = tr_block_exscan(chunk_count + b * nchunk, nchunk, chunk_offset + b * nchunk);
  if (threadIdx.x == 0) count[b] = all;
}

__global__ __launch_bounds__(TR_THREADS) void tr_number_kernel(const int* __restrict__ labels, int HW, int nchunk,
                                                                const int* __restrict__ chunk_offset,
                                                                int* __restrict__ rootnum) {
  __shared__ unsigned long long w_bits[TR_WORDS];
  __shared__ int w_before[TR_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int base = blockIdx.y * HW;
  for (int s = 0; s < TR_STEPS; ++s) {
    const int i = blockIdx.x * TR_CHUNK + s * TR_THREADS + threadIdx.x;  // word s*4 + wave holds flat pixels in order
    const bool root = i < HW && labels[base + i] == base + i;
    const unsigned long long bits = __ballot(root);
    if (lane == 0) w_bits[s * (TR_THREADS / 64) + wave] = bits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = chunk_offset[blockIdx.y * nchunk + blockIdx.x];
    for (int k = 0; k < TR_WORDS; ++k) {
      w_before[k] = t;
      t += __popcll(w_bits[k]);
    }
  }
  __syncthreads();
  for (int s = 0; s < TR_STEPS; ++s) {
    const int k = s * (TR_THREADS / 64) + wave;
    const unsigned long long bits = w_bits[k];
    if (!((bits >> lane) & 1ull)) continue;
    const int i = blockIdx.x * TR_CHUNK + s * TR_THREADS + threadIdx.x;  // < HW: only such pixels were flagged
    rootnum[base + i] = w_before[k] + __popcll(bits & ((1ull << lane) - 1ull)) + 1;
  }
}

// The run of equal labels (within one map row) that this lane belongs to, among the 64 consecutive pixels of its wave:
// [start, end) in lanes, and its lanes as a mask.  Every lane of the wave must call it.
struct TrRun {
  int start, end;
  unsigned long long lanes;
};
__device__ __forceinline__ TrRun tr_run(int label, int x, int lane) {
  const int prev = __shfl_up(label, 1);
  const bool head = lane == 0 || label != prev || x == 0;
  const unsigned long long heads = __ballot(head);  // bit 0 is always set
  const unsigned long long upto = heads & (~0ull >> (63 - lane));
  const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
  TrRun r;
  r.start = 63 - __clzll((long long)upto);
  r.end = above ? __ffsll((unsigned long long)above) - 1 : 64;
  const unsigned long long below_end = r.end == 64 ? ~0ull : (1ull << r.end) - 1ull;
  r.lanes = below_end & ~((1ull << r.start) - 1ull);
  return r;
}

__global__ __launch_bounds__(TR_THREADS) void tr_table_kernel(const float* __restrict__ height, int H, int W, int R,
                                                               const int* __restrict__ rootnum, int* __restrict__ labels,
                                                               int* __restrict__ boxes, int* __restrict__ areas,
                                                               int* __restrict__ valid) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  const int HW = H * W, b = blockIdx.y;
  int label = 0;
  bool has_height = false;
  if (i < HW) {
    const int g = b * HW + i;
    const int r = labels[g];
    label = r >= 0 ? rootnum[r] : 0;
    labels[g] = label;
    has_height = label > 0 && height[g] > 0.f;
  }
  const int x = i % W, y = i / W;
  const TrRun run = tr_run(label, x, lane);
  const unsigned long long vmask = __ballot(has_height);
  if (lane == run.start && label > 0 && label <= R) {
    const int row = b * R + label - 1;
    atomicMin(&boxes[row * 4 + 0], y);
    atomicMin(&boxes[row * 4 + 1], x);
    atomicMax(&boxes[row * 4 + 2], y);
    atomicMax(&boxes[row * 4 + 3], x + (run.end - run.start) - 1);
    atomicAdd(&areas[row], run.end - run.start);
    const int nv = __popcll(vmask & run.lanes);
    if (nv > 0) atomicAdd(&valid[row], nv);
  }
}

__global__ __launch_bounds__(TR_SCAN_THREADS) void tr_offsets_kernel(const int* __restrict__ count, int R,
                                                                     const int* __restrict__ valid,
                                                                     int* __restrict__ seg_offset, int* __restrict__ cursor) {
  const int b = blockIdx.x;
  const int rows = min(count[b], R);
  tr_block_exscan(valid + b * R, rows, seg_offset + b * R);
  for (int r = threadIdx.x; r < rows; r += TR_SCAN_THREADS) cursor[b * R + r] = 0;
}

// the heights of region r of image b go to bits[b*HW + seg_offset[b,r] + 0 .. valid[b,r]): the segments of one image
// partition at most HW slots
__global__ __launch_bounds__(TR_THREADS) void tr_gather_kernel(const float* __restrict__ height, int H, int W, int R,
                                                                const int* __restrict__ labels,
                                                                const int* __restrict__ seg_offset, int* __restrict__ cursor,
                                                                unsigned* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  const int HW = H * W, b = blockIdx.y;
  int label = 0;
  float h = 0.f;
  if (i < HW) {
    label = labels[b * HW + i];
    if (label > R) label = 0;  // no table row: not gathered (any two such neighbours form one run of 0, harmless)
    h = height[b * HW + i];
  }
  const bool has_height = label > 0 && h > 0.f;
  const TrRun run = tr_run(label, i % W, lane);
  const unsigned long long vmask = __ballot(has_height) & run.lanes;
  int first = 0;
  if (lane == run.start && vmask != 0ull) first = atomicAdd(&cursor[b * R + label - 1], __popcll(vmask));
  first = __shfl(first, run.start);
  if (has_height) {
    const int slot = seg_offset[b * R + label - 1] + first + __popcll(vmask & ((1ull << lane) - 1ull));
    bits[b * HW + slot] = __float_as_uint(h);
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_median_kernel(const int* __restrict__ count, int HW, int R,
                                                                const int* __restrict__ seg_offset,
                                                                const unsigned* __restrict__ bits, int* __restrict__ boxes,
                                                                const int* __restrict__ valid, float* __restrict__ medians) {
  __shared__ int hist[256];
  __shared__ unsigned s_prefix, s_next;
  __shared__ int s_rank, s_less, s_equal;
  const int r = blockIdx.x, b = blockIdx.y, row = b * R + r;
  if (r >= min(count[b], R)) {  // no such region in this image: a zero row (areas and valid are zero already)
    if (threadIdx.x < 4) boxes[row * 4 + threadIdx.x] = 0;
    if (threadIdx.x == 0) medians[row] = 0.f;
    return;
  }
  const int n = valid[row];
  if (n == 0) {
    if (threadIdx.x == 0) medians[row] = 0.f;
    return;
  }
  const unsigned* seg = bits + b * HW + seg_offset[row];
  if (threadIdx.x == 0) {
    s_prefix = 0u;
    s_rank = (n - 1) / 2;  // the lower middle element, 0-based, among the elements that match the prefix so far
    s_less = 0;            // elements below every element that matches the prefix
    s_next = 0xFFFFFFFFu;
  }
  unsigned care = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    for (int j = threadIdx.x; j < n; j += TR_THREADS) {
      const unsigned u = seg[j];
      if ((u & care) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int rank = s_rank, bin = 0, c = hist[0];
      while (rank >= c && bin < 255) {  // rank < the number of elements that match the prefix: ends by bin 255
        rank -= c;
        s_less += c;
        c = hist[++bin];
      }
      s_rank = rank;
      s_equal = c;
      s_prefix = prefix | ((unsigned)bin << shift);
    }
    care |= 255u << shift;
    __syncthreads();
  }
  const unsigned lo = s_prefix;  // the element of rank (n-1)/2; s_less elements are smaller, s_equal equal
  unsigned hi = lo;
  if ((n & 1) == 0 && n / 2 >= s_less + s_equal) {  // the upper middle element is the smallest one above lo
    unsigned m = 0xFFFFFFFFu;
    for (int j = threadIdx.x; j < n; j += TR_THREADS) {
      const unsigned u = seg[j];
      if (u > lo) m = min(m, u);
    }
    atomicMin(&s_next, m);
    __syncthreads();
    hi = s_next;
  }
  if (threadIdx.x == 0) {
    const float a = __uint_as_float(lo), c = __uint_as_float(hi);
    medians[row] = (n & 1) ? a : __fmul_rn(__fadd_rn(a, c), 0.5f);
  }
}

static size_t tr_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct TrLayout {
  size_t parent, rootnum, bits, chunk_count, chunk_offset, seg_offset, cursor, bytes;
};

static TrLayout tr_layout(int B, int H, int W, int R) {
  const size_t n = (size_t)B * H * W, nchunk = (size_t)B * vkas_cdiv((long)H * W, TR_CHUNK), rows = (size_t)B * R;
  TrLayout l;
  l.parent = 0;
  l.rootnum = tr_align(l.parent + n * sizeof(int));
  l.bits = tr_align(l.rootnum + n * sizeof(int));
  l.chunk_count = tr_align(l.bits + n * sizeof(unsigned));
  l.chunk_offset = tr_align(l.chunk_count + nchunk * sizeof(int));
  l.seg_offset = tr_align(l.chunk_offset + nchunk * sizeof(int));
  l.cursor = tr_align(l.seg_offset + rows * sizeof(int));
  l.bytes = tr_align(l.cursor + rows * sizeof(int));
  return l;
}

static int tr_check_dims(const char* what, int B, int H, int W, int R) {
  VKAS_CHECK(B >= 1 && H >= 1 && W >= 1, "%s: bad dims B=%d H=%d W=%d", what, B, H, W);
  VKAS_CHECK(R >= 1, "%s: max_regions %d must be >= 1", what, R);
  VKAS_CHECK((long)B * H * W < (1L << 31), "%s: B*H*W = %ld must stay below 2^31", what, (long)B * H * W);
  VKAS_CHECK(B <= 65535 && vkas_cdiv(H, TR_TH) <= 65535 && R <= (1 << 24) && (long)B * R < (1L << 29),
             "%s: B=%d, H=%d or max_regions=%d too large for one launch", what, B, H, R);
  return VKAS_OK;
}

}  // namespace

extern "C" long long vkas_text_regions_workspace_bytes(int B, int H, int W, int max_regions) {
  if (tr_check_dims("vkas_text_regions_workspace_bytes", B, H, W, max_regions) != VKAS_OK) return -1;
  return (long long)tr_layout(B, H, W, max_regions).bytes;
}

extern "C" int vkas_text_regions(const unsigned char* mask, const float* height, int B, int H, int W, int max_regions,
                                 void* workspace, long long workspace_bytes, int* count, int* labels, int* boxes, int* areas,
                                 int* valid, float* medians, void* stream) {
  VKAS_CHECK(mask && height && workspace && count && labels && boxes && areas && valid && medians,
             "vkas_text_regions: null pointer");
  const int rc = tr_check_dims("vkas_text_regions", B, H, W, max_regions);
  if (rc != VKAS_OK) return rc;
  const int R = max_regions;
  const TrLayout l = tr_layout(B, H, W, R);
  VKAS_CHECK(workspace_bytes >= (long long)l.bytes, "vkas_text_regions: workspace of %lld bytes, %zu needed", workspace_bytes,
             l.bytes);
  VKAS_CHECK(vkas_aligned16(workspace), "vkas_text_regions: workspace must be 16-byte aligned");
  char* ws = static_cast<char*>(workspace);
  int* parent = reinterpret_cast<int*>(ws + l.parent);
  int* rootnum = reinterpret_cast<int*>(ws + l.rootnum);
  unsigned* bits = reinterpret_cast<unsigned*>(ws + l.bits);
  int* chunk_count = reinterpret_cast<int*>(ws + l.chunk_count);
  int* chunk_offset = reinterpret_cast<int*>(ws + l.chunk_offset);
  int* seg_offset = reinterpret_cast<int*>(ws + l.seg_offset);
  int* cursor = reinterpret_cast<int*>(ws + l.cursor);
  const int HW = H * W, rows = B * R;
  const int nchunk = (int)vkas_cdiv(HW, TR_CHUNK);
  const dim3 per_pixel((unsigned)vkas_cdiv(HW, TR_THREADS), (unsigned)B);
  hipStream_t s = vkas_stream(stream);
  tr_init_kernel<<<(unsigned)vkas_cdiv(rows, TR_THREADS), TR_THREADS, 0, s>>>(rows, boxes, areas, valid);
  VKAS_LAUNCH_CHECK("text_regions init");
  tr_tile_kernel<<<dim3((unsigned)vkas_cdiv(W, TR_TW), (unsigned)vkas_cdiv(H, TR_TH), (unsigned)B), TR_THREADS, 0, s>>>(
      mask, H, W, parent);
  VKAS_LAUNCH_CHECK("text_regions tile");
  tr_seam_kernel<<<per_pixel, TR_THREADS, 0, s>>>(H, W, parent);
  VKAS_LAUNCH_CHECK("text_regions seam");
  tr_flatten_kernel<<<dim3((unsigned)nchunk, (unsigned)B), TR_THREADS, 0, s>>>(parent, HW, nchunk, labels, chunk_count);
  VKAS_LAUNCH_CHECK("text_regions flatten");
  tr_scan_kernel<<<B, TR_SCAN_THREADS, 0, s>>>(chunk_count, nchunk, chunk_offset, count);
  VKAS_LAUNCH_CHECK("text_regions scan");
  tr_number_kernel<<<dim3((unsigned)nchunk, (unsigned)B), TR_THREADS, 0, s>>>(labels, HW, nchunk, chunk_offset, rootnum);
  VKAS_LAUNCH_CHECK("text_regions number");
  tr_table_kernel<<<per_pixel, TR_THREADS, 0, s>>>(height, H, W, R, rootnum, labels, boxes, areas, valid);
  VKAS_LAUNCH_CHECK("text_regions table");
  tr_offsets_kernel<<<B, TR_SCAN_THREADS, 0, s>>>(count, R, valid, seg_offset, cursor);
  VKAS_LAUNCH_CHECK("text_regions offsets");
  tr_gather_kernel<<<per_pixel, TR_THREADS, 0, s>>>(height, H, W, R, labels, seg_offset, cursor, bits);
  VKAS_LAUNCH_CHECK("text_regions gather");
  tr_median_kernel<<<dim3((unsigned)R, (unsigned)B), TR_THREADS, 0, s>>>(count, HW, R, seg_offset, bits, boxes, valid, medians);
  VKAS_LAUNCH_CHECK("text_regions median");
  return VKAS_OK;
}
