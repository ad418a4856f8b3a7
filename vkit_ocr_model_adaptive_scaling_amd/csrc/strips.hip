// Text lines cut into upright strips of one height (inferencing/strips.py holds the rule and the host oracle
// quad_strips_host): every strip row is an affine warp (warp_pixel.h: the pixel rule of the warp kernels of respack.hip)
// of one image of an arena into its own slot of h x slot_w pixels in one output buffer, all strips of all images in one
// launch.
//
// The strips are ragged - a slot is 64 to 2048 pixels wide at the defaults -, so the work is a flat list of tiles: row r
// owns the tiles tile_start[r] .. tile_start[r + 1] - 1, TILE_H x TILE_W pixels each, and tile_start (n + 1 int64 words,
// scanned on the host) FOLLOWS THE ROWS in the same table: rows[12 * n + r].  A workgroup walks the tiles b = blockIdx.x,
// blockIdx.x + gridDim.x, ... below tile_start[n] and finds the row of each by binary search (wave-uniform: scalar loads).
// The host cannot read a device table, so it sizes the grid from n and h alone, and the kernel trusts nothing in the
// table: the total is clamped to what n rows of the widest slot need, a search ends on some row 0..n-1 whatever the table
// holds, and the tile's place in the row is checked against the row's own tile count.
//
// A wave owns a compact patch of 16 rows x 16 pixels, the four waves of a workgroup lie side by side.  A line runs in any
// direction: the source footprint of such a patch is about 16 x 16 source pixels times the scale for horizontal and
// vertical text alike, where a patch of one row of 256 pixels would put every lane of a vertical line on a cache line of
// its own.  The patch is computed in four passes of 16 x 4 pixels whose long side follows the source's rows, staged in
// LDS (768 bytes per wave) and written out by rows: a lane stores 4 adjacent pixels, 12 bytes, three aligned dwords where
// the address allows.
#include "vkas_common.h"
#include "warp_pixel.h"

namespace {

constexpr int TILE_H = 16, TILE_W = 64, QUAD = 4, THREADS = 256;  // a wave: 16 rows x (4 lanes x 4 pixels)
constexpr int STRIP_WORDS = 12;                                    // src, offset, slot_w, w, ay, ax, myy, myx, mxy, mxx, log2n, 0
constexpr int STRIP_H_MAX = 256;
constexpr int GRID_MAX = 2048;                                     // 8 workgroups on each of 256 CUs
constexpr long long OUT_BYTES_MAX = 1LL << 40;

__device__ __forceinline__ long long slot_tiles(long long slot_w, int h) {
  return (long long)((h + TILE_H - 1) / TILE_H) * ((slot_w + TILE_W - 1) / TILE_W);
}

__global__ __launch_bounds__(THREADS) void quad_strips_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                              const long long* __restrict__ sources, int S,
                                                              const long long* __restrict__ rows, int n, int h,
                                                              unsigned char* __restrict__ out, long long out_bytes) {
  const long long* __restrict__ tile_start = rows + (long)n * STRIP_WORDS;
  const long long most = (long long)n * slot_tiles(SIDE_MAX, h);
  const long long total = min(max(tile_start[n], 0LL), most);
  // a wave's patch of 16 x 16 pixels, as it goes out: row i, 48 bytes; lane l reads dwords 3*l .. 3*l + 2 (no bank conflict)
  __shared__ unsigned stage[THREADS / 64][TILE_H * 16 * 3 / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* patch = reinterpret_cast<unsigned char*>(stage[wave]);
  for (long long b = blockIdx.x; b < total; b += gridDim.x) {  // every condition up to the barriers is workgroup-uniform
    int lo = 0, hi = n;  // the last row whose tile_start is at or below b, if the table rises
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_start[mid] <= b) lo = mid; else hi = mid;
    }
    const long long* t = rows + (long)lo * STRIP_WORDS;
    const long long src = t[0], offset = t[1], slot_w = t[2], w = t[3];
    // the slot: a row without one is skipped
    if (slot_w < 1 || slot_w > SIDE_MAX || offset < 0 || offset > out_bytes || 3LL * h * slot_w > out_bytes - offset) continue;
    const long long tile = b - tile_start[lo];
    if (tile < 0 || tile >= slot_tiles(slot_w, h)) continue;
    const int tiles_w = (int)((slot_w + TILE_W - 1) / TILE_W);
    const int i0 = (int)(tile / tiles_w) * TILE_H, j0 = (int)(tile % tiles_w) * TILE_W + wave * 16;  // of the wave's patch
    // everything else: a row that fails gets a slot of zeros
    const WarpRow p{0, 0, h, w, t[4], t[5], t[6], t[7], t[8], t[9], t[10]};
    bool fill = w >= 1 && w <= slot_w && p.ok() && src >= 0 && src < S;
    const unsigned char* image = arena;
    int Hs = 0, Ws = 0;
    if (fill) {
      const long long* e = sources + src * 4;
      const long long off = e[0], hs = e[1], ws = e[2];
      fill = side_ok(hs) && side_ok(ws) && off >= 0 && off <= arena_bytes && 3 * hs * ws <= arena_bytes - off;
      image = arena + (fill ? off : 0);
      Hs = (int)hs; Ws = (int)ws;
    }
    // The pixels are computed in four passes of 16 x 4: the 16 lanes that are adjacent in a pass lie along the strip axis
    // that runs along the source's rows (j for horizontal text, i for vertical text), so one load instruction of the wave
    // touches 4 or 5 source rows in either case and not 16 to 20.
    const bool along_j = llabs(p.mxx) >= llabs(p.myx);
    const int fast = lane & 15, slow = lane >> 4;
#pragma unroll
    for (int q = 0; q < QUAD; ++q) {
      const int pi = along_j ? q * 4 + slow : fast, pj = along_j ? fast : q * 4 + slow;
      unsigned v[3] = {0u, 0u, 0u};
      if (fill && i0 + pi < h && j0 + pj < w) warp_pixel(image, Hs, Ws, p, i0 + pi, j0 + pj, v);
      unsigned char* cell = patch + (pi * 16 + pj) * 3;
      cell[0] = (unsigned char)v[0]; cell[1] = (unsigned char)v[1]; cell[2] = (unsigned char)v[2];
    }
    __syncthreads();
    // out: a lane takes 4 adjacent pixels of one row, 12 bytes
    const int i = i0 + (lane >> 2), j = j0 + (lane & 3) * QUAD;
    if (i < h && j < slot_w) {
      const unsigned d0 = stage[wave][3 * lane], d1 = stage[wave][3 * lane + 1], d2 = stage[wave][3 * lane + 2];
      unsigned char* o = out + offset + ((long long)i * slot_w + j) * 3;
      const int cells = (int)min((long long)QUAD, slot_w - j);
      if (cells == QUAD && (((uintptr_t)o) & 3u) == 0) {
        unsigned* d = reinterpret_cast<unsigned*>(o);
        d[0] = d0; d[1] = d1; d[2] = d2;
      } else {
        const unsigned dw[3] = {d0, d1, d2};
#pragma unroll
        for (int k = 0; k < QUAD * 3; ++k)
          if (k < cells * 3) o[k] = (unsigned char)(dw[k >> 2] >> (8 * (k & 3)));
      }
    }
    __syncthreads();  // the patch is free for the next tile
  }
}

}  // namespace

extern "C" int vkas_quad_strips_u8(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                   const long long* rows, int n, int h, unsigned char* out, long long out_bytes,
                                   void* stream) {
  VKAS_CHECK(n >= 0, "%s: bad table (n %d)", __func__, n);
  VKAS_CHECK(h >= 1 && h <= STRIP_H_MAX, "%s: the strip height %d must be in 1..%d", __func__, h, STRIP_H_MAX);
  VKAS_CHECK(out_bytes >= 0 && out_bytes < OUT_BYTES_MAX, "%s: out_bytes %lld must be in [0, 2^40)", __func__, out_bytes);
  VKAS_CHECK(arena && sources && rows && out, "%s: null pointer", __func__);
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "%s: empty arena (%lld bytes, %d sources)", __func__, arena_bytes, S);
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)rows) & 7u) == 0,
             "%s: the source table and the row table must be 8-byte aligned", __func__);
  if (n == 0) return VKAS_OK;  // nothing to write
  const long long most = (long long)n * vkas_cdiv(h, TILE_H) * (SIDE_MAX / TILE_W);
  const unsigned grid = (unsigned)(most < GRID_MAX ? most : GRID_MAX);
  quad_strips_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, rows, n, h, out, out_bytes);
  VKAS_LAUNCH_CHECK("quad_strips_u8");
  return VKAS_OK;
}
