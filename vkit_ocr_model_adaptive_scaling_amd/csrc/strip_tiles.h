// The tile walk of the kernels that cut text lines into strips of one height (strips.hip: upright quads; spines.hip: curved
// lines along their spines), stated once.  Both tables begin alike: n rows of STRIP_WORDS words whose first four are src,
// offset, slot_w, w (the source, the byte offset of the slot of h x slot_w pixels in the output, the columns that hold
// pixels), then tile_start, n + 1 words scanned on the host: row r owns the tiles tile_start[r] .. tile_start[r + 1] - 1,
// TILE_H x TILE_W pixels each.  A workgroup walks the tiles b = blockIdx.x, blockIdx.x + gridDim.x, ... and finds the row of
// each by binary search (wave-uniform: scalar loads).  The host cannot read a device table, so it sizes the grid from n and h
// alone (strip_grid), and the kernels trust nothing in the table:
//   tile_total   tile_start[n] clamped to what n rows of the widest slot need
//   tile_row     ends on some row 0..n-1 whatever the table holds
//   strip_tile   the prologue of a tile.  No slot (slot_w outside 1..SIDE_MAX, a slot that leaves the output, a tile beyond
//                the row's own count): false, the tile is SKIPPED.  Anything else amiss in the four words or the source entry:
//                fill = false, the tile is written as ZEROS.  A kernel reads the rest of its row itself.
//   strip_patch  the body of a tile.  A wave owns a compact patch of 16 rows x 16 pixels, four waves side by side: about
//                16 x 16 source pixels times the scale whichever way the line runs.  It is computed in four passes of 16 x 4
//                pixels whose 16 adjacent lanes lie along the strip axis that follows the source's rows (a load then touches
//                4 or 5 source rows, not 16 to 20), staged in LDS (768 bytes per wave) and, after a barrier, written out by
//                rows: a lane stores 4 adjacent pixels, 12 bytes, three aligned dwords where the address allows.  A second
//                barrier frees the patch.
// A Rule is a struct of __device__ __forceinline__ members, built per tile and resolved at compile time:
//   along_j(wave)     whether the adjacent lanes of the wave's passes run along j (which lanes share a cache line, not a byte)
//   row(wave, pj, p)  the WarpRow of column pj of the wave's patch; false: the column is zeros
//   col(j)            the j that pixel (i, j) of the strip passes to warp_pixel beside its i
// Every condition up to the barriers is workgroup-uniform: the walk, the search, strip_tile's verdicts and what a kernel
// decides between strip_tile and strip_patch depend on b and the tables alone.  Writes are bounded by the slot, reads by the
// source's sides (warp_pixel.h).  The host half (the grid, the argument checks the entry points share) is at the end.
#pragma once
#include "warp_pixel.h"

namespace {

constexpr int TILE_H = 16, TILE_W = 64, QUAD = 4, THREADS = 256;  // a wave: 16 rows x (4 lanes x 4 pixels)
constexpr int STRIP_WORDS = 12, STRIP_H_MAX = 256;                 // the words of a row in either table; the heights
constexpr int GRID_MAX = 2048;                                     // 8 workgroups on each of 256 CUs
constexpr long long OUT_BYTES_MAX = 1LL << 40;

__device__ __forceinline__ long long slot_tiles(long long slot_w, int h) {
  return (long long)((h + TILE_H - 1) / TILE_H) * ((slot_w + TILE_W - 1) / TILE_W);
}
__device__ __forceinline__ long long tile_total(const long long* __restrict__ tile_start, int n, int h) {
  return min(max(tile_start[n], 0LL), (long long)n * slot_tiles(SIDE_MAX, h));
}

// the last row whose tile_start is at or below b, if the table rises; some row 0..n-1 whatever it holds
__device__ __forceinline__ int tile_row(const long long* __restrict__ tile_start, int n, long long b) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

struct StripTile {
  int lo, ti, tj, Hs, Ws;              // the row; the tile's place in the row's grid of tiles; the source's sides
  long long first, offset, slot_w, w;  // tile_start[lo]; row words 1 .. 3
  const unsigned char* image;
  bool fill;                           // false: zeros
};

__device__ __forceinline__ bool strip_tile(const long long* __restrict__ rows, int n, int h, long long b, long long out_bytes,
                                           const long long* __restrict__ sources, int S,
                                           const unsigned char* __restrict__ arena, long long arena_bytes, StripTile& t) {
  const long long* __restrict__ tile_start = rows + (long)n * STRIP_WORDS;
  t.lo = tile_row(tile_start, n, b);
  const long long* r = rows + (long)t.lo * STRIP_WORDS;
  const long long src = r[0];
  t.offset = r[1]; t.slot_w = r[2]; t.w = r[3]; t.first = tile_start[t.lo];
  // the slot: a row without one is skipped
  if (t.slot_w < 1 || t.slot_w > SIDE_MAX || t.offset < 0 || t.offset > out_bytes || 3LL * h * t.slot_w > out_bytes - t.offset)
    return false;
  const long long tile = b - t.first;
  if (tile < 0 || tile >= slot_tiles(t.slot_w, h)) return false;
  const int tiles_w = (int)((t.slot_w + TILE_W - 1) / TILE_W);
  t.ti = (int)(tile / tiles_w); t.tj = (int)(tile % tiles_w);
  // everything else: a row that fails gets a slot of zeros
  t.fill = t.w >= 1 && t.w <= t.slot_w && src >= 0 && src < S;
  t.image = arena; t.Hs = t.Ws = 0;
  if (t.fill) {
    const long long* e = sources + src * 4;
    const long long off = e[0], hs = e[1], ws = e[2];
    t.fill = side_ok(hs) && side_ok(ws) && off >= 0 && off <= arena_bytes && 3 * hs * ws <= arena_bytes - off;
    t.image = arena + (t.fill ? off : 0); t.Hs = (int)hs; t.Ws = (int)ws;
  }
  return true;
}

template <class Rule>
__device__ __forceinline__ void strip_patch(const StripTile& t, bool fill, int h, const Rule& rule, unsigned char* out) {
  // a wave's patch of 16 x 16 pixels, as it goes out: row i, 48 bytes; lane l reads dwords 3*l .. 3*l + 2 (no bank conflict)
  __shared__ unsigned stage[THREADS / 64][TILE_H * 16 * 3 / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fast = lane & 15, slow = lane >> 4;
  unsigned char* patch = reinterpret_cast<unsigned char*>(stage[wave]);
  const int i0 = t.ti * TILE_H, j0 = t.tj * TILE_W + wave * 16;  // of the wave's patch
  const bool along_j = rule.along_j(wave);
#pragma unroll
  for (int q = 0; q < QUAD; ++q) {
    const int pi = along_j ? q * 4 + slow : fast, pj = along_j ? fast : q * 4 + slow;
    unsigned v[3] = {0u, 0u, 0u};
    WarpRow p;
    if (fill && i0 + pi < h && j0 + pj < t.w && rule.row(wave, pj, p))
      warp_pixel(t.image, t.Hs, t.Ws, p, i0 + pi, rule.col(j0 + pj), v);
    unsigned char* cell = patch + (pi * 16 + pj) * 3;
    cell[0] = (unsigned char)v[0]; cell[1] = (unsigned char)v[1]; cell[2] = (unsigned char)v[2];
  }
  __syncthreads();
  // out: a lane takes 4 adjacent pixels of one row, 12 bytes
  const int i = i0 + (lane >> 2), j = j0 + (lane & 3) * QUAD;
  if (i < h && j < t.slot_w) {
    const unsigned dw[3] = {stage[wave][3 * lane], stage[wave][3 * lane + 1], stage[wave][3 * lane + 2]};
    unsigned char* o = out + t.offset + ((long long)i * t.slot_w + j) * 3;
    const int cells = (int)min((long long)QUAD, t.slot_w - j);
    if (cells == QUAD && (((uintptr_t)o) & 3u) == 0) {
      unsigned* d = reinterpret_cast<unsigned*>(o);
      d[0] = dw[0]; d[1] = dw[1]; d[2] = dw[2];
    } else {
#pragma unroll
      for (int k = 0; k < QUAD * 3; ++k)
        if (k < cells * 3) o[k] = (unsigned char)(dw[k >> 2] >> (8 * (k & 3)));
    }
  }
  __syncthreads();  // the patch (and what the kernel staged beside it) is free for the next tile
}

// ---- host ------------------------------------------------------------------------------------------------------------
unsigned strip_grid(int n, int h, int per_block) {  // for the tiles of n rows, per_block tiles to a workgroup at a time
  const long long blocks = vkas_cdiv((long long)n * vkas_cdiv(h, TILE_H) * (SIDE_MAX / TILE_W), per_block);
  return (unsigned)(blocks < GRID_MAX ? blocks : GRID_MAX);
}

// what the strips entry points check alike: the height, and after their tables the output size, their pointers, the arena
int strip_check_height(const char* who, int h) {
  VKAS_CHECK(h >= 1 && h <= STRIP_H_MAX, "%s: the strip height %d must be in 1..%d", who, h, STRIP_H_MAX);
  return VKAS_OK;
}
int strip_check_io(const char* who, long long out_bytes, bool pointers, long long arena_bytes, int S) {
  VKAS_CHECK(out_bytes >= 0 && out_bytes < OUT_BYTES_MAX, "%s: out_bytes %lld must be in [0, 2^40)", who, out_bytes);
  VKAS_CHECK(pointers, "%s: null pointer", who);
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "%s: empty arena (%lld bytes, %d sources)", who, arena_bytes, S);
  return VKAS_OK;
}

}  // namespace
