// Curved text lines cut into strips along their spines (inferencing/spines.py holds the rule from a line's character quads
// to its knots, the integer rule from knots to columns and the host oracle spine_strips_host).  A strip column is a
// one-pixel-wide affine warp (warp_pixel.h), so the pixel rule is that of strips.hip and respack.hip.
//
// One table: n spine rows of 12 words (src, offset, slot_w, w, knot_start, knots, col_start, log2n, 0, 0, 0, 0), then
// tile_start (n + 1 words, the tiles of strip_tiles.h), then knots_total knot records of 6 words (q, cy, cx, vy, vx, 0).
// Two launches on one stream:
//   columns  one lane per strip column: a wave takes a tile of the strips kernel's walk, and where that tile lies in the
//            first tile row of its strip the 64 lanes write the records (ay, ax, myy, myx, mxy, mxx) of its 64 columns into
//            the workspace at col_start + j; the segment of a column is found by the search the rule fixes;
//   strips   the walk, the prologue and the patch body of strip_tiles.h; between prologue and body 16 lanes load the 16
//            column records of the wave's patch into LDS - one more barrier -, and the rule reads them there.
// Nothing in the table is trusted: see strip_tiles.h, SpineRow::ok and the head of the columns loop.  A tile of the strips
// kernel reads column records only where the columns kernel, which walks the same table by the same search, has written
// them: it looks up the tile of the first tile row above it and drops its own - skipped, not zero-filled - unless that one
// resolves to the same row.
#include <climits>
#include "strip_tiles.h"

namespace {

constexpr int KNOT_WORDS = 6, COLUMN_WORDS = 6;
constexpr long long KNOT_C_MAX = 1LL << 39, KNOT_V_MAX = 1LL << 30;
constexpr long long NONE = LLONG_MIN;                              // the six words of an invalid column

struct SpineRow {
  long long slot_w, w, knot_start, knots, col_start, log2n;  // row words 2 .. 7
  static __device__ __forceinline__ SpineRow load(const long long* __restrict__ table, int r) {
    const long long* t = table + (long)r * STRIP_WORDS;
    return SpineRow{t[2], t[3], t[4], t[5], t[6], t[7]};
  }
  // the row's knots lie inside the knot table and its columns inside the workspace: checked before either is an index
  __device__ __forceinline__ bool ok(long long knots_total, long long columns_cap) const {
    return w >= 1 && w <= slot_w && log2n >= 0 && log2n <= 3 && knot_start >= 0 && knots >= 2 && knot_start <= knots_total &&
           knots <= knots_total - knot_start && col_start >= 0 && col_start <= columns_cap && w <= columns_cap - col_start;
  }
};

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
  const long long* __restrict__ tile_start = rows + (long)n * STRIP_WORDS;
  const long long* __restrict__ knots = tile_start + n + 1;
  const long long total = tile_total(tile_start, n, h);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = THREADS / 64;
  for (long long b = (long long)blockIdx.x * waves + wave; b < total; b += (long long)gridDim.x * waves) {  // wave-uniform
    const int lo = tile_row(tile_start, n, b);
    const SpineRow r = SpineRow::load(rows, lo);
    if (r.slot_w < 1 || r.slot_w > SIDE_MAX) continue;
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

// the rule of a tile: a WarpRow per column, from the records of the patch's 16 columns as the kernel staged them
struct SpineRule {
  const long long (*cols)[16][COLUMN_WORDS];
  long long h, log2n;
  __device__ __forceinline__ bool along_j(int wave) const {  // per wave, AT THE PATCH'S FIRST COLUMN, wherever the line turns
    const long long myx0 = cols[wave][0][3], mxx0 = cols[wave][0][5];
    return myx0 == NONE || llabs(mxx0) >= llabs(myx0);
  }
  __device__ __forceinline__ bool row(int wave, int pj, WarpRow& p) const {
    const long long* c = cols[wave][pj];
    p = WarpRow{0, 0, h, 1, c[0], c[1], c[2], c[3], c[4], c[5], log2n};
    return p.ok();
  }
  __device__ __forceinline__ int col(int) const { return 0; }  // a column is a strip one pixel wide
};

__global__ __launch_bounds__(THREADS) void spine_strips_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                               const long long* __restrict__ sources, int S,
                                                               const long long* __restrict__ rows, int n,
                                                               long long knots_total, int h,
                                                               const long long* __restrict__ columns, long long columns_cap,
                                                               unsigned char* __restrict__ out, long long out_bytes) {
  const long long* __restrict__ tile_start = rows + (long)n * STRIP_WORDS;
  const long long total = tile_total(tile_start, n, h);
  __shared__ long long cols[THREADS / 64][16][COLUMN_WORDS];  // the records of the patch's 16 columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long b = blockIdx.x; b < total; b += gridDim.x) {  // every condition up to the barriers is workgroup-uniform
    StripTile t;
    if (!strip_tile(rows, n, h, b, out_bytes, sources, S, arena, arena_bytes, t)) continue;
    const SpineRow r = SpineRow::load(rows, t.lo);
    const bool fill = t.fill && r.ok(knots_total, columns_cap);
    // the columns of this tile were written by the wave that took tile `above` of the first tile row - if the walk of
    // the columns kernel reached it and found this row for it (always, when tile_start is honest)
    const long long above = t.first + t.tj;
    if (fill && t.ti != 0 && (above < 0 || above >= total || tile_row(tile_start, n, above) != t.lo)) continue;
    if (lane < 16) {
      const long long j = t.tj * TILE_W + wave * 16 + lane;
      const bool have = fill && j < r.w;
      const long long* c = columns + (have ? (r.col_start + j) * COLUMN_WORDS : 0);
#pragma unroll
      for (int k = 0; k < COLUMN_WORDS; ++k) cols[wave][lane][k] = have ? c[k] : NONE;
    }
    __syncthreads();
    strip_patch(t, fill, h, SpineRule{cols, h, r.log2n}, out);
  }
}

int check_table(const char* who, const long long* table, int n, long long knots_total, int h) {
  VKAS_CHECK(n >= 0 && knots_total >= 0, "%s: bad table (n %d, %lld knots)", who, n, knots_total);
  if (int e = strip_check_height(who, h)) return e;
  VKAS_CHECK(table, "%s: null pointer", who);
  VKAS_CHECK((((uintptr_t)table) & 7u) == 0, "%s: the table must be 8-byte aligned", who);
  return VKAS_OK;
}

void launch_columns(const long long* table, int n, long long knots_total, int h, long long* columns, long long columns_cap,
                    hipStream_t stream) {
  spine_columns_kernel<<<strip_grid(n, h, THREADS / 64), THREADS, 0, stream>>>(table, n, knots_total, h, columns, columns_cap);
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
  if (int e = strip_check_io(__func__, out_bytes, arena && sources && ws && out, arena_bytes, S)) return e;
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)ws) & 7u) == 0,
             "%s: the source table and the workspace must be 8-byte aligned", __func__);
  VKAS_CHECK(ws_bytes >= vkas_spine_strips_workspace_bytes(n) && ws_bytes < OUT_BYTES_MAX,
             "%s: a workspace of %lld bytes, %d rows need at least one column record (48 bytes) each", __func__, ws_bytes, n);
  if (n == 0) return VKAS_OK;  // nothing to write
  const long long columns_cap = ws_bytes / vkas_spine_strips_workspace_bytes(1);
  long long* columns = static_cast<long long*>(ws);
  launch_columns(table, n, knots_total, h, columns, columns_cap, vkas_stream(stream));
  VKAS_LAUNCH_CHECK("spine_strips_u8 (columns)");
  spine_strips_kernel<<<strip_grid(n, h, 1), THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, table, n,
                                                                                knots_total, h, columns, columns_cap, out,
                                                                                out_bytes);
  VKAS_LAUNCH_CHECK("spine_strips_u8");
  return VKAS_OK;
}
