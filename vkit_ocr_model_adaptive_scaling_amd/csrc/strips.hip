// Text lines cut into upright strips of one height (inferencing/strips.py holds the rule and the host oracle
// quad_strips_host): every strip row is an affine warp (warp_pixel.h: the pixel rule of the warp kernels of respack.hip) of
// one image of an arena into its own slot of h x slot_w pixels in one output buffer, all strips of all images in one launch.
//
// The strips are ragged - a slot is 64 to 2048 pixels wide at the defaults -, so the work is a flat list of tiles, and
// tile_start FOLLOWS THE ROWS in the same table: rows[12 * n + r].  The walk, its distrust of the table and the patch of a
// wave are strip_tiles.h's; here are the row's own words and its rule.
#include "strip_tiles.h"

namespace {

// row words 4 .. 10 after src, offset, slot_w, w: ay, ax, myy, myx, mxy, mxx, log2n - one WarpRow for the whole strip
struct QuadRule {
  WarpRow p;
  __device__ __forceinline__ bool along_j(int) const { return llabs(p.mxx) >= llabs(p.myx); }  // per tile
  __device__ __forceinline__ bool row(int, int, WarpRow& q) const { q = p; return true; }      // checked once per tile
  __device__ __forceinline__ int col(int j) const { return j; }
};

__global__ __launch_bounds__(THREADS) void quad_strips_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                              const long long* __restrict__ sources, int S,
                                                              const long long* __restrict__ rows, int n, int h,
                                                              unsigned char* __restrict__ out, long long out_bytes) {
  const long long total = tile_total(rows + (long)n * STRIP_WORDS, n, h);
  for (long long b = blockIdx.x; b < total; b += gridDim.x) {  // every condition up to the barriers is workgroup-uniform
    StripTile t;
    if (!strip_tile(rows, n, h, b, out_bytes, sources, S, arena, arena_bytes, t)) continue;
    const long long* r = rows + (long)t.lo * STRIP_WORDS;
    const QuadRule rule{WarpRow{0, 0, h, t.w, r[4], r[5], r[6], r[7], r[8], r[9], r[10]}};
    strip_patch(t, t.fill && rule.p.ok(), h, rule, out);
  }
}

}  // namespace

extern "C" int vkas_quad_strips_u8(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                   const long long* rows, int n, int h, unsigned char* out, long long out_bytes,
                                   void* stream) {
  VKAS_CHECK(n >= 0, "%s: bad table (n %d)", __func__, n);
  if (int e = strip_check_height(__func__, h)) return e;
  if (int e = strip_check_io(__func__, out_bytes, arena && sources && rows && out, arena_bytes, S)) return e;
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)rows) & 7u) == 0,
             "%s: the source table and the row table must be 8-byte aligned", __func__);
  if (n == 0) return VKAS_OK;  // nothing to write
  quad_strips_kernel<<<strip_grid(n, h, 1), THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, rows, n, h, out,
                                                                               out_bytes);
  VKAS_LAUNCH_CHECK("quad_strips_u8");
  return VKAS_OK;
}
