// Training label maps from character quadrilaterals (dataset/labels.py holds the rule and the host oracle; the rule is this
// project's own, restated on pixels, not vkit's polygon fill or warped Gaussian).  rows (B, K, 20) int32: Q4 corners (8), the
// inclusive pixel box (4), float32 centre (2), inverse frame (4), height, valid.  One launch, driven from the output:
//
//   * a 256-thread workgroup owns a 16 x 64 tile of the CROPPED map of one image, a thread four adjacent cells of one row
//     (csrc/respack.hip's tile shape: rows are the contiguous direction, a wave stores 4 rows x 256 bytes per output);
//   * the image's table is walked in chunks of 256 rows, one row per thread: the rows that are valid and whose box - clipped
//     to the tile, whatever it holds - is not empty are appended, whole, to an LDS list at the ballot's prefix count.  A list
//     is bounded by its chunk (256 x 80 B = 20 KB), so there is no overflow path, however many quads overlap;
//   * all threads then run the list with wave-uniform (broadcast) LDS reads and keep a running (a, index, height) per cell;
//     the tie-break a == best && index < best_index is explicit, so the order of the list does not matter;
//   * int64 edge functions at the cell centre (16y + 8, 16x + 8), inclusive; a in float32 in the stated order, every product
//     and sum rounded (lb_mul / lb_add / lb_sub below: no contraction into fma); expf once per cell, at the end.
// No atomics, no allocation, no synchronisation; every output element is written exactly once (zero where no quad
// reaches), so the call is capture-safe and bit-identical from run to run.  Table reads are bounded by the clamped count
// and stores by the output tile: no table content makes the kernel touch memory outside its buffers.
#include "vkas_common.h"

#include <limits.h>

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_TILE_H = 16, LB_TILE_W = 64;  // cells; LB_TILE_W / 4 threads per row
constexpr int LB_CHUNK = LB_THREADS;           // table rows per pass over the list
constexpr int LB_WORDS = 20;                   // int32 per row
constexpr int LB_WAVES = LB_THREADS / 64;

// One rounding per operation, as numpy float32 does.  This toolchain's lb_mul / lb_add are plain `x * y` / `x + y`
// compiled under the default -ffp-contract=fast, and the first build of this kernel had v_pk_fma_f32 in place of the sums
// of products below; instructions emitted under `contract(off)` carry no contract flag and cannot be fused.
#pragma clang fp contract(off)
__device__ __forceinline__ float lb_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float lb_add(float a, float b) { return a + b; }
__device__ __forceinline__ float lb_sub(float a, float b) { return a - b; }
#pragma clang fp contract(fast)

__global__ __launch_bounds__(LB_THREADS) void char_label_maps_kernel(const int* __restrict__ rows,
                                                                      const int* __restrict__ count, int K, int up, int left,
                                                                      int CH, int CW, float k, int vec,
                                                                      int* __restrict__ owner, float* __restrict__ mask,
                                                                      float* __restrict__ height,
                                                                      float* __restrict__ score) {
  __shared__ int4 s_rows[LB_CHUNK * (LB_WORDS / 4)];
  __shared__ int s_count[LB_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  // the tile in crop coordinates, its cells in map coordinates
  const int ty0 = blockIdx.y * LB_TILE_H, tx0 = blockIdx.x * LB_TILE_W;
  const int ty1 = min(ty0 + LB_TILE_H, CH) - 1, tx1 = min(tx0 + LB_TILE_W, CW) - 1;  // inclusive, never empty
  const int y = ty0 + (tid >> 4), x = tx0 + (tid & 15) * 4;                           // crop coordinates of the first cell
  const int Y = y + up, X = x + left;
  const int n = min(max(count[b], 0), K);
  const int4* table = reinterpret_cast<const int4*>(rows + (long)b * K * LB_WORDS);

  float best[4], bh[4];
  int bi[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    best[c] = __builtin_inff();
    bi[c] = INT_MAX;
    bh[c] = 0.f;
  }
  const long py = 16L * Y + 8;

  for (int c0 = 0; c0 < n; c0 += LB_CHUNK) {
    const int r = c0 + tid;
    bool reach = false;
    int4 box = make_int4(0, 0, 0, 0), tail = box;
    if (r < n) {
      box = table[(long)r * 5 + 2];
      tail = table[(long)r * 5 + 4];
      // the box clipped to the tile: what the list keeps, whatever the table holds
      box.x = max(box.x, ty0 + up);
      box.y = max(box.y, tx0 + left);
      box.z = min(box.z, ty1 + up);
      box.w = min(box.w, tx1 + left);
      reach = tail.w != 0 && box.x <= box.z && box.y <= box.w;
    }
    const unsigned long long bits = __ballot(reach);
    if (lane == 0) s_count[wave] = __popcll(bits);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int wv = 0; wv < LB_WAVES; ++wv) {
      const int cnt = s_count[wv];
      if (wv < wave) base += cnt;
      total += cnt;
    }
    if (reach) {
      int4* dst = s_rows + (base + __popcll(bits & ((1ull << lane) - 1ull))) * 5;  // < LB_CHUNK slots: one per thread
      dst[0] = table[(long)r * 5 + 0];
      dst[1] = table[(long)r * 5 + 1];
      dst[2] = box;
      dst[3] = table[(long)r * 5 + 3];
      tail.w = r;  // a listed row is valid: its index takes that word
      dst[4] = tail;
    }
    __syncthreads();
    for (int e = 0; e < total; ++e) {
      const int4 bx = s_rows[e * 5 + 2];
      if (Y < bx.x || Y > bx.z || X + 3 < bx.y || X > bx.w) continue;
      const int4 c01 = s_rows[e * 5 + 0], c23 = s_rows[e * 5 + 1], fr = s_rows[e * 5 + 3], tl = s_rows[e * 5 + 4];
      const long qy[4] = {c01.x, c01.z, c23.x, c23.z}, qx[4] = {c01.y, c01.w, c23.y, c23.w};
      const float cy = __int_as_float(fr.x), cx = __int_as_float(fr.y);
      const float m00 = __int_as_float(fr.z), m01 = __int_as_float(fr.w);
      const float m10 = __int_as_float(tl.x), m11 = __int_as_float(tl.y);
      const float dy = lb_sub(lb_add((float)Y, 0.5f), cy);
      const int idx = tl.w;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int Xc = X + c;
        if (Xc < bx.y || Xc > bx.w) continue;
        const long px = 16L * Xc + 8;
        bool in = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int j1 = (j + 1) & 3;
          in = in && ((qx[j1] - qx[j]) * (py - qy[j]) - (qy[j1] - qy[j]) * (px - qx[j]) >= 0);
        }
        if (!in) continue;
        const float dx = lb_sub(lb_add((float)Xc, 0.5f), cx);
        const float s = lb_add(lb_mul(m00, dy), lb_mul(m01, dx));
        const float t = lb_add(lb_mul(m10, dy), lb_mul(m11, dx));
        const float a = lb_mul(k, lb_add(lb_mul(s, s), lb_mul(t, t)));
        if (a < best[c] || (a == best[c] && idx < bi[c])) {
          best[c] = a;
          bi[c] = idx;
          bh[c] = __int_as_float(tl.z);
        }
      }
    }
    __syncthreads();  // the list and the counts are rewritten by the next chunk
  }

  if (y >= CH || x >= CW) return;
  int o[4];
  float m[4], h[4], s[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bool owned = bi[c] != INT_MAX;
    o[c] = owned ? bi[c] + 1 : 0;
    m[c] = owned ? 1.f : 0.f;
    h[c] = owned ? bh[c] : 0.f;
    s[c] = owned ? expf(-best[c]) : 0.f;
  }
  const long at = ((long)b * CH + y) * CW + x;
  if (vec) {  // CW % 4 == 0 and 16-byte aligned outputs: x + 3 < CW, at % 4 == 0
    if (owner) *reinterpret_cast<int4*>(owner + at) = make_int4(o[0], o[1], o[2], o[3]);
    if (mask) *reinterpret_cast<float4*>(mask + at) = make_float4(m[0], m[1], m[2], m[3]);
    if (height) *reinterpret_cast<float4*>(height + at) = make_float4(h[0], h[1], h[2], h[3]);
    if (score) *reinterpret_cast<float4*>(score + at) = make_float4(s[0], s[1], s[2], s[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (x + c >= CW) break;
      if (owner) owner[at + c] = o[c];
      if (mask) mask[at + c] = m[c];
      if (height) height[at + c] = h[c];
      if (score) score[at + c] = s[c];
    }
  }
}

}  // namespace

extern "C" int vkas_char_label_maps(const int* rows, const int* count, int B, int K, int h, int w, int up, int left, int CH,
                                    int CW, float k, int* owner, float* mask, float* height, float* score, void* stream) {
  VKAS_CHECK(B >= 0 && B <= 65535 && K >= 0, "vkas_char_label_maps: bad B=%d (0..65535) or K=%d (>= 0)", B, K);
  VKAS_CHECK(h > 0 && w > 0, "vkas_char_label_maps: bad map %d x %d", h, w);
  VKAS_CHECK((long)B * h * w < (1L << 31), "vkas_char_label_maps: B*h*w = %ld must stay below 2^31", (long)B * h * w);
  VKAS_CHECK(CH > 0 && CW > 0 && up >= 0 && left >= 0 && (long)up + CH <= h && (long)left + CW <= w,
             "vkas_char_label_maps: crop (up %d, left %d, %d x %d) outside the %d x %d map", up, left, CH, CW, h, w);
  VKAS_CHECK(k > 0.f && k <= 3.0e38f, "vkas_char_label_maps: k = 1 / (2 sigma^2) must be finite and positive");
  VKAS_CHECK(owner || mask || height || score, "vkas_char_label_maps: every output is NULL");
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(count && (rows || K == 0), "vkas_char_label_maps: null table");
  VKAS_CHECK(vkas_aligned16(rows), "vkas_char_label_maps: rows must be 16-byte aligned");
  const int vec = CW % 4 == 0 && vkas_aligned16(owner) && vkas_aligned16(mask) && vkas_aligned16(height) &&
                  vkas_aligned16(score);
  const dim3 grid((unsigned)vkas_cdiv(CW, LB_TILE_W), (unsigned)vkas_cdiv(CH, LB_TILE_H), (unsigned)B);
  VKAS_CHECK(grid.y <= 65535, "vkas_char_label_maps: crop height %d needs more than 65535 tile rows", CH);
  char_label_maps_kernel<<<grid, LB_THREADS, 0, vkas_stream(stream)>>>(rows, count, K, up, left, CH, CW, k, vec, owner, mask,
                                                                       height, score);
  VKAS_LAUNCH_CHECK("char_label_maps");
  return VKAS_OK;
}
