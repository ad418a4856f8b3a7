// Curved text lines cut into strips along their spines (inferencing/spines.py holds the rule from a line's character quads
// to its knots, the integer rule from knots to columns and the host oracle spine_strips_host).  A strip column is a
// one-pixel-wide affine warp (warp_pixel.h), so the pixel rule is that of strips.hip and respack.hip.
//
// One table: n spine rows of 12 words (src, offset, slot_w, w, knot_start, knots, col_start, log2n, 0, 0, 0, 0), then
// tile_start (n + 1 words, the 16 x 64 tiles of strips.hip), then knots_total knot records of 6 words (q, cy, cx, vy, vx, 0).
// Two launches on one stream:
//   columns  one lane per strip column: a wave takes a tile of the strips kernel's walk, and where that tile lies in the
//            first tile row of its strip the 64 lanes write the records (ay, ax, myy, myx, mxy, mxx) of its 64 columns into
//            the workspace at col_start + j; the segment of a column is found by the search the rule fixes;
//   strips   the tile walk of quad_strips_kernel (strips.hip), COPIED here, not shared: the grid strides over the tiles, the
//            search over tile_start is wave-uniform, a wave owns a patch of 16 x 16 pixels staged in LDS and stores 12 bytes
//            per lane.  The 16 column records of a patch are loaded once per tile by 16 lanes into LDS; whether the lanes
//            that are adjacent in a pass run along j or along i is chosen per wave from the patch's first column.
// Nothing in the table is trusted: see the checks in spine_row_ok and at the head of both tile loops.  A tile of the strips
// kernel reads column records only where the columns kernel, which walks the same table by the same search, has written
// them: it looks up the tile of the first tile row above it and drops its own tile unless that one resolves to the same row.
#include <climits>

#include "vkas_common.h"
#include "warp_pixel.h"

namespace {

constexpr int TILE_H = 16, TILE_W = 64, QUAD = 4, THREADS = 256;  // a wave: 16 rows x (4 lanes x 4 pixels)
constexpr int SPINE_WORDS = 12, KNOT_WORDS = 6, COLUMN_WORDS = 6;
constexpr int SPINE_H_MAX = 256;
constexpr int GRID_MAX = 2048;                                     // 8 workgroups on each of 256 CUs
constexpr long long OUT_BYTES_MAX = 1LL << 40;
constexpr long long KNOT_C_MAX = 1LL << 39, KNOT_V_MAX = 1LL << 30;
constexpr long long NONE = LLONG_MIN;                              // the six words of an invalid column

__device__ __forceinline__ long long slot_tiles(long long slot_w, int h) {
  return (long long)((h + TILE_H - 1) / TILE_H) * ((slot_w + TILE_W - 1) / TILE_W);
}

struct SpineRow {
  long long src, offset, slot_w, w, knot_start, knots, col_start, log2n;
  static __device__ __forceinline__ SpineRow load(const long long* __restrict__ table, int r) {
    const long long* t = table + (long)r * SPINE_WORDS;
    return SpineRow{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]};
  }
  __device__ __forceinline__ bool width_ok() const { return slot_w >= 1 && slot_w <= SIDE_MAX; }
  // the row's knots lie inside the knot table and its columns inside the workspace: checked before either is an index
  __device__ __forceinline__ bool ok(long long knots_total, long long columns_cap) const {
    return w >= 1 && w <= slot_w && log2n >= 0 && log2n <= 3 && knot_start >= 0 && knots >= 2 && knot_start <= knots_total &&
           knots <= knots_total - knot_start && col_start >= 0 && col_start <= columns_cap && w <= columns_cap - col_start;
  }
};

// the last row whose tile_start is at or below b, if the table rises; some row 0..n-1 whatever it holds
__device__ __forceinline__ int tile_row(const long long* __restrict__ tile_start, int n, long long b) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_start[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long fdiv(long long a, long long b) {  // floor(a / b), b > 0
  const long long q = a / b;
  return a % b < 0 ? q - 1 : q;
}
__device__ __forceinline__ long long rdiv(long long x, long long d) { return fdiv(2 * x + d, 2 * d); }

// The integer rule from knots to a column (inferencing/spines.py::spine_columns_host): rec = ay, ax, myy, myx, mxy, mxx, or
// six words of NONE.  k: the row's `knots` records, all inside the table.
__device__ __forceinline__ void spine_column(const long long* __restrict__ k, long long knots, long long j, int h,
                                             long long rec[COLUMN_WORDS]) {
#pragma unroll
  for (int c = 0; c < COLUMN_WORDS; ++c) rec[c] = NONE;
  long long lo = 0, hi = knots;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (k[mid * KNOT_WORDS] <= j) lo = mid; else hi = mid;
  }
  if (lo + 1 >= knots) return;
  const long long* e0 = k + lo * KNOT_WORDS;
  const long long* e1 = e0 + KNOT_WORDS;
  const long long q0 = e0[0], q1 = e1[0];
  // n <= 8192 needs q0 > j - 8192 and q1 <= j + 8192: tested first, so that n itself cannot overflow
  if (!(q0 <= j && j < q1 && q0 > j - SIDE_MAX && q1 <= j + SIDE_MAX)) return;
  const long long n = q1 - q0;
  if (n > SIDE_MAX) return;
  long long c0[4], d[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const long long u = e0[1 + c], v = e1[1 + c], top = c < 2 ? KNOT_C_MAX - 1 : KNOT_V_MAX;
    if (u < -top || u > top || v < -top || v > top) return;
    c0[c] = u; d[c] = v - u;
  }
  const long long a = 2 * (j - q0) + 1;
  const long long Cy = c0[0] + fdiv(d[0] * a, 2 * n), Cx = c0[1] + fdiv(d[1] * a, 2 * n);
  const long long Vy = c0[2] + fdiv(d[2] * a, 2 * n), Vx = c0[3] + fdiv(d[3] * a, 2 * n);
  const long long myy = rdiv(Vy, h), mxy = rdiv(Vx, h), myx = rdiv(d[0], n), mxx = rdiv(d[1], n);
  const long long ay = Cy - fdiv((h - 1) * myy, 2), ax = Cx - fdiv((h - 1) * mxy, 2);
  const WarpRow p{0, 0, h, 1, ay, ax, myy, myx, mxy, mxx, 0};
  if (!p.ok()) return;
  rec[0] = ay; rec[1] = ax; rec[2] = myy; rec[3] = myx; rec[4] = mxy; rec[5] = mxx;
}

__global__ __launch_bounds__(THREADS) void spine_columns_kernel(const long long* __restrict__ rows, int n,
                                                                long long knots_total, int h,
                                                                long long* __restrict__ columns, long long columns_cap) {
  const long long* __restrict__ tile_start = rows + (long)n * SPINE_WORDS;
  const long long* __restrict__ knots = tile_start + n + 1;
  const long long most = (long long)n * slot_tiles(SIDE_MAX, h);
  const long long total = min(max(tile_start[n], 0LL), most);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = THREADS / 64;
  for (long long b = (long long)blockIdx.x * waves + wave; b < total; b += (long long)gridDim.x * waves) {  // wave-uniform
    const int lo = tile_row(tile_start, n, b);
    const SpineRow r = SpineRow::load(rows, lo);
    if (!r.width_ok()) continue;
    const long long tile = b - tile_start[lo];
    if (tile < 0 || tile >= slot_tiles(r.slot_w, h)) continue;
    const int tiles_w = (int)((r.slot_w + TILE_W - 1) / TILE_W);
    if (tile >= tiles_w || !r.ok(knots_total, columns_cap)) continue;  // the first tile row of the strip writes its columns
    const long long j = tile * TILE_W + lane;
    if (j >= r.w) continue;
    long long rec[COLUMN_WORDS];
    spine_column(knots + r.knot_start * KNOT_WORDS, r.knots, j, h, rec);
    long long* o = columns + (r.col_start + j) * COLUMN_WORDS;
#pragma unroll
    for (int c = 0; c < COLUMN_WORDS; ++c) o[c] = rec[c];
  }
}

__global__ __launch_bounds__(THREADS) void spine_strips_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                               const long long* __restrict__ sources, int S,
                                                               const long long* __restrict__ rows, int n,
                                                               long long knots_total, int h,
                                                               const long long* __restrict__ columns, long long columns_cap,
                                                               unsigned char* __restrict__ out, long long out_bytes) {
  const long long* __restrict__ tile_start = rows + (long)n * SPINE_WORDS;
  const long long most = (long long)n * slot_tiles(SIDE_MAX, h);
  const long long total = min(max(tile_start[n], 0LL), most);
  // a wave's patch of 16 x 16 pixels, as it goes out: row i, 48 bytes; lane l reads dwords 3*l .. 3*l + 2 (no bank conflict)
  __shared__ unsigned stage[THREADS / 64][TILE_H * 16 * 3 / 4];
  __shared__ long long cols[THREADS / 64][16][COLUMN_WORDS];  // the records of the patch's 16 columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* patch = reinterpret_cast<unsigned char*>(stage[wave]);
  for (long long b = blockIdx.x; b < total; b += gridDim.x) {  // every condition up to the barriers is workgroup-uniform
    const int lo = tile_row(tile_start, n, b);
    const SpineRow r = SpineRow::load(rows, lo);
    // the slot: a row without one is skipped
    if (!r.width_ok() || r.offset < 0 || r.offset > out_bytes || 3LL * h * r.slot_w > out_bytes - r.offset) continue;
    const long long first = tile_start[lo], tile = b - first;
    if (tile < 0 || tile >= slot_tiles(r.slot_w, h)) continue;
    const int tiles_w = (int)((r.slot_w + TILE_W - 1) / TILE_W);
    const int ti = (int)(tile / tiles_w), tj = (int)(tile % tiles_w);
    const int i0 = ti * TILE_H, j0 = tj * TILE_W + wave * 16;  // of the wave's patch
    // everything else: a row that fails gets a slot of zeros
    bool fill = r.ok(knots_total, columns_cap) && r.src >= 0 && r.src < S;
    const unsigned char* image = arena;
    int Hs = 0, Ws = 0;
    if (fill) {
      const long long* e = sources + r.src * 4;
      const long long off = e[0], hs = e[1], ws = e[2];
      fill = side_ok(hs) && side_ok(ws) && off >= 0 && off <= arena_bytes && 3 * hs * ws <= arena_bytes - off;
      image = arena + (fill ? off : 0);
      Hs = (int)hs; Ws = (int)ws;
    }
    // the columns of this tile were written by the wave that took tile `above` of the first tile row - if the walk of
    // the columns kernel reached it and found this row for it (always, when tile_start is honest)
    if (fill && ti != 0) {
      const long long above = first + tj;
      if (above < 0 || above >= total || tile_row(tile_start, n, above) != lo) continue;
    }
    if (lane < 16) {
      const long long j = j0 + lane;
      const bool have = fill && j < r.w;
      const long long* c = columns + (have ? (r.col_start + j) * COLUMN_WORDS : 0);
#pragma unroll
      for (int k = 0; k < COLUMN_WORDS; ++k) cols[wave][lane][k] = have ? c[k] : NONE;
    }
    __syncthreads();
    // The pixels are computed in four passes of 16 x 4, as in strips.hip: the 16 lanes that are adjacent in a pass lie
    // along the strip axis that runs along the source's rows AT THE PATCH'S FIRST COLUMN (a line that turns inside the
    // patch keeps that choice: it changes which lanes share a cache line, not a byte of the result).
    const long long myx0 = cols[wave][0][3], mxx0 = cols[wave][0][5];
    const bool along_j = myx0 == NONE || llabs(mxx0) >= llabs(myx0);
    const int fast = lane & 15, slow = lane >> 4;
#pragma unroll
    for (int q = 0; q < QUAD; ++q) {
      const int pi = along_j ? q * 4 + slow : fast, pj = along_j ? fast : q * 4 + slow;
      const long long* c = cols[wave][pj];
      const WarpRow p{0, 0, h, 1, c[0], c[1], c[2], c[3], c[4], c[5], r.log2n};
      unsigned v[3] = {0u, 0u, 0u};
      if (fill && i0 + pi < h && j0 + pj < r.w && p.ok()) warp_pixel(image, Hs, Ws, p, i0 + pi, 0, v);
      unsigned char* cell = patch + (pi * 16 + pj) * 3;
      cell[0] = (unsigned char)v[0]; cell[1] = (unsigned char)v[1]; cell[2] = (unsigned char)v[2];
    }
    __syncthreads();
    // out: a lane takes 4 adjacent pixels of one row, 12 bytes
    const int i = i0 + (lane >> 2), j = j0 + (lane & 3) * QUAD;
    if (i < h && j < r.slot_w) {
      const unsigned d0 = stage[wave][3 * lane], d1 = stage[wave][3 * lane + 1], d2 = stage[wave][3 * lane + 2];
      unsigned char* o = out + r.offset + ((long long)i * r.slot_w + j) * 3;
      const int cells = (int)min((long long)QUAD, r.slot_w - j);
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
    __syncthreads();  // the patch and the records are free for the next tile
  }
}

int check_table(const char* who, const long long* table, int n, long long knots_total, int h) {
  VKAS_CHECK(n >= 0 && knots_total >= 0, "%s: bad table (n %d, %lld knots)", who, n, knots_total);
  VKAS_CHECK(h >= 1 && h <= SPINE_H_MAX, "%s: the strip height %d must be in 1..%d", who, h, SPINE_H_MAX);
  VKAS_CHECK(table, "%s: null pointer", who);
  VKAS_CHECK((((uintptr_t)table) & 7u) == 0, "%s: the table must be 8-byte aligned", who);
  return VKAS_OK;
}

void launch_columns(const long long* table, int n, long long knots_total, int h, long long* columns, long long columns_cap,
                    hipStream_t stream) {
  const long long most = (long long)n * vkas_cdiv(h, TILE_H) * (SIDE_MAX / TILE_W);
  const long long blocks = vkas_cdiv(most, THREADS / 64);
  const unsigned grid = (unsigned)(blocks < GRID_MAX ? blocks : GRID_MAX);
  spine_columns_kernel<<<grid, THREADS, 0, stream>>>(table, n, knots_total, h, columns, columns_cap);
}

}  // namespace

extern "C" long long vkas_spine_strips_workspace_bytes(long long columns) {
  return columns < 0 ? -1 : columns * COLUMN_WORDS * (long long)sizeof(long long);
}

extern "C" int vkas_spine_columns(const long long* table, int n, long long knots_total, int h, long long* columns,
                                  long long columns_cap, void* stream) {
  if (int e = check_table(__func__, table, n, knots_total, h)) return e;
  VKAS_CHECK(columns && (((uintptr_t)columns) & 7u) == 0, "%s: columns must be an 8-byte aligned pointer", __func__);
  VKAS_CHECK(columns_cap >= n && columns_cap < (1LL << 40), "%s: room for %lld columns, %d rows need at least one each",
             __func__, columns_cap, n);
  if (n == 0) return VKAS_OK;  // nothing to write
  launch_columns(table, n, knots_total, h, columns, columns_cap, vkas_stream(stream));
  VKAS_LAUNCH_CHECK("spine_columns");
  return VKAS_OK;
}

extern "C" int vkas_spine_strips_u8(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                    const long long* table, int n, long long knots_total, int h, void* ws,
                                    long long ws_bytes, unsigned char* out, long long out_bytes, void* stream) {
  if (int e = check_table(__func__, table, n, knots_total, h)) return e;
  VKAS_CHECK(out_bytes >= 0 && out_bytes < OUT_BYTES_MAX, "%s: out_bytes %lld must be in [0, 2^40)", __func__, out_bytes);
  VKAS_CHECK(arena && sources && ws && out, "%s: null pointer", __func__);
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "%s: empty arena (%lld bytes, %d sources)", __func__, arena_bytes, S);
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0,
             "%s: the source table and the workspace must be 8-byte aligned", __func__);
  VKAS_CHECK(ws_bytes >= vkas_spine_strips_workspace_bytes(n) && ws_bytes < OUT_BYTES_MAX,
             "%s: a workspace of %lld bytes, %d rows need at least one column record (48 bytes) each", __func__, ws_bytes, n);
  if (n == 0) return VKAS_OK;  // nothing to write
  const long long columns_cap = ws_bytes / vkas_spine_strips_workspace_bytes(1);
  long long* columns = static_cast<long long*>(ws);
  launch_columns(table, n, knots_total, h, columns, columns_cap, vkas_stream(stream));
  VKAS_LAUNCH_CHECK("spine_strips_u8 (columns)");
  const long long most = (long long)n * vkas_cdiv(h, TILE_H) * (SIDE_MAX / TILE_W);
  const unsigned grid = (unsigned)(most < GRID_MAX ? most : GRID_MAX);
  spine_strips_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, table, n, knots_total, h,
                                                                 columns, columns_cap, out, out_bytes);
  VKAS_LAUNCH_CHECK("spine_strips_u8");
  return VKAS_OK;
}
