// Crop, rescale and pack the text regions into the page of the precise pass (inferencing/adaptive_scaling.py:190-293 restated
// on pixels; the rule and the host oracles: inferencing/packing.py): a variable-ratio gather / resample of 3-byte pixels from
// one source image into the disjoint rectangles of a packed page, and the int32 region-label page that goes with it.
//
// Both kernels are driven from the output.  A workgroup owns a tile of TILE_H x TILE_W output cells (page pixels / label
// pixels) and first searches the placement table for the rows that reach into its tile: every wave takes 64 rows at a time,
// ballots the hits and appends (row index, hit rectangle clipped to the tile) to its own list in LDS - no atomics, and the
// order is irrelevant because destinations are disjoint, which also bounds a list by the tile's cell count.  Then every
// thread resolves the owner of its four adjacent cells from the lists (wave-uniform LDS reads) and produces them: 12 bytes
// of page (three aligned dword stores when Wp % 4 == 0) or four labels (one 16-byte store when Wq % 4 == 0).  Every output
// byte is written exactly once - zero where no placement reaches - so a call leaves nothing of the buffer's earlier contents.
//
// The source pixels are gathered directly (byte loads through the vector L1): see DESIGN.md for why this first version
// does not stage source rows in LDS.  All arithmetic is integer: inner row sums in 32 bits, the outer sum in 64, one
// rounding division by the product of the axis denominators.
#include "vkas_common.h"

namespace {

constexpr int TILE_H = 16, TILE_W = 64, QUAD = 4;           // cells per tile; cells per thread along x
constexpr int THREADS = TILE_H * TILE_W / QUAD;             // 256
constexpr int WAVES = THREADS / 64;
constexpr int LIST_CAP = TILE_H * TILE_W;                   // disjoint placements: at most one per cell of the tile
constexpr int SIDE_MAX = 8192;
constexpr int DIM_MAX = 32768;                              // source / page sides: pixel counts stay below 2^30

// what a row is checked against: the one source of the single-image kernels; the multi kernels look theirs up per row
struct SourceDims {
  int Hs, Ws;
};

struct Placement {
  int sy, sx, sh, sw, dy, dx, dh, dw;
  static __device__ __forceinline__ Placement load(const int* __restrict__ table, int i);
  __device__ __forceinline__ bool ok(const SourceDims& d) const;
};

__device__ __forceinline__ Placement load_placement(const int* __restrict__ table, int i) {
  const int4 a = *reinterpret_cast<const int4*>(table + (long)i * 8);
  const int4 b = *reinterpret_cast<const int4*>(table + (long)i * 8 + 4);
  return Placement{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// the kernels trust the host's disjointness check, but never a row's bounds: a row that fails here is treated as absent,
// so no table content can make a kernel read outside the source (writes are bounded by the output tile in any case)
__device__ __forceinline__ bool placement_ok(const Placement& p, int Hs, int Ws) {
  return p.sh >= 1 && p.sw >= 1 && p.dh >= 1 && p.dw >= 1 && p.sh <= SIDE_MAX && p.sw <= SIDE_MAX && p.dh <= SIDE_MAX &&
         p.dw <= SIDE_MAX && p.sy >= 0 && p.sx >= 0 && p.sy <= Hs - p.sh && p.sx <= Ws - p.sw && p.dy >= 0 && p.dx >= 0 &&
         p.dy <= DIM_MAX && p.dx <= DIM_MAX;
}

// cells [lo, hi) of one axis whose centres c*f + f/2 lie in the page interval [d0, d0 + dlen); f == 1: the pixels themselves
__device__ __forceinline__ void cell_range(int d0, int dlen, int f, int& lo, int& hi) {
  const int a = 2 * d0 - f, b = 2 * (d0 + dlen) - f;
  lo = a <= 0 ? 0 : (a + 2 * f - 1) / (2 * f);
  hi = b <= 0 ? 0 : (b + 2 * f - 1) / (2 * f);
}

__device__ __forceinline__ Placement Placement::load(const int* __restrict__ table, int i) { return load_placement(table, i); }

struct TileLists {
  int2 entry[WAVES][LIST_CAP];  // (row index, y0 | y1 << 8 | x0 << 16 | x1 << 24: hit rectangle in tile cells, exclusive ends)
  int count[WAVES];
};

__device__ __forceinline__ bool Placement::ok(const SourceDims& d) const { return placement_ok(*this, d.Hs, d.Ws); }

// the rows [begin, end) of the table that own at least one cell of the tile at (ty0, tx0); f = page pixels per cell.  Row:
// the table's row type (Placement, WarpRow, MultiRow) - load(table, i), ok(ctx) and the destination rectangle dy, dx, dh, dw
template <class Row, class Word, class Ctx>
__device__ __forceinline__ void find_tile_rows(const Word* __restrict__ table, int begin, int end, const Ctx& ctx, int f,
                                               int ty0, int tx0, TileLists& L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
  for (int base = begin + wave * 64; base < end; base += THREADS) {
    const int i = base + lane;
    bool hit = false;
    int packed = 0;
    if (i < end) {
      const Row p = Row::load(table, i);
      if (p.ok(ctx)) {
        int y0, y1, x0, x1;
        cell_range((int)p.dy, (int)p.dh, f, y0, y1);
        cell_range((int)p.dx, (int)p.dw, f, x0, x1);
        y0 = max(y0 - ty0, 0); y1 = min(y1 - ty0, TILE_H);
        x0 = max(x0 - tx0, 0); x1 = min(x1 - tx0, TILE_W);
        hit = y0 < y1 && x0 < x1;
        packed = y0 | (y1 << 8) | (x0 << 16) | (x1 << 24);
      }
    }
    const unsigned long long mask = __ballot(hit);
    if (hit) {
      const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (pos < LIST_CAP) L.entry[wave][pos] = make_int2(i, packed);
    }
    cnt += __popcll(mask);
  }
  if (lane == 0) L.count[wave] = min(cnt, LIST_CAP);
  __syncthreads();
}

__device__ __forceinline__ void find_tile_placements(const int* __restrict__ table, int n, int Hs, int Ws, int f, int ty0,
                                                     int tx0, TileLists& L) {
  find_tile_rows<Placement>(table, 0, n, SourceDims{Hs, Ws}, f, ty0, tx0, L);
}

// owner row of each of the thread's four cells (tile row r, tile columns c .. c + 3), -1 where there is none
__device__ __forceinline__ void resolve_owners(const TileLists& L, int r, int c, int owner[QUAD]) {
#pragma unroll
  for (int q = 0; q < QUAD; ++q) owner[q] = -1;
  for (int w = 0; w < WAVES; ++w) {
    const int cnt = L.count[w];
    for (int e = 0; e < cnt; ++e) {
      const int2 en = L.entry[w][e];
      const int y0 = en.y & 255, y1 = (en.y >> 8) & 255, x0 = (en.y >> 16) & 255, x1 = (en.y >> 24) & 255;
      if (r >= y0 && r < y1) {
#pragma unroll
        for (int q = 0; q < QUAD; ++q)
          if (c + q >= x0 && c + q < x1) owner[q] = en.x;
      }
    }
  }
}

// One axis of the rule for destination sample o of D from S source samples: taps j(k), weights w(k), k < n; their sum is den.
struct Axis {
  int n, j0, a, b, D, S, f;
  bool shrink;
  __device__ __forceinline__ void init(int o, int S_, int D_) {
    S = S_; D = D_;
    shrink = D < S;
    if (shrink) {
      a = o * S; b = a + S;
      j0 = a / D;
      n = (b - 1) / D - j0 + 1;
    } else {
      const int num = (2 * o + 1) * S - D;                      // >= -D: floor division by hand below zero
      j0 = num >= 0 ? num / (2 * D) : -1;
      f = num - j0 * 2 * D;
      n = f == 0 ? 1 : 2;
    }
  }
  __device__ __forceinline__ int den() const { return shrink ? S : 2 * D; }
  __device__ __forceinline__ int tap(int k) const { return shrink ? j0 + k : min(max(j0 + k, 0), S - 1); }
  __device__ __forceinline__ int weight(int k) const {
    if (shrink) {
      const int j = j0 + k;
      return min((j + 1) * D, b) - max(j * D, a);
    }
    return k == 0 ? 2 * D - f : f;
  }
};

// (num + den / 2) / den for num <= 255 * den, den < 2^29: a float estimate (within 1 of the quotient) and an exact fix-up
__device__ __forceinline__ unsigned round_div(unsigned long long num, unsigned den) {
  const unsigned long long t = num + (den >> 1);
  int q = (int)((float)t * (1.0f / (float)den));
  long long rem = (long long)t - (long long)q * den;
  if (rem < 0) { --q; rem += den; }
  if (rem < 0) { --q; rem += den; }
  if (rem >= (long long)den) { ++q; rem -= den; }
  if (rem >= (long long)den) ++q;
  return (unsigned)q;
}

__device__ __forceinline__ void resample_pixel(const unsigned char* __restrict__ src, int Ws, const Placement& p,
                                               const Axis& ay, int ox, unsigned out[3]) {
  Axis ax;
  ax.init(ox, p.sw, p.dw);
  unsigned long long acc0 = 0, acc1 = 0, acc2 = 0;
  for (int ky = 0; ky < ay.n; ++ky) {
    const unsigned char* row = src + ((long)(p.sy + ay.tap(ky)) * Ws + p.sx) * 3;
    unsigned in0 = 0, in1 = 0, in2 = 0;
    for (int kx = 0; kx < ax.n; ++kx) {
      const unsigned char* px = row + ax.tap(kx) * 3;
      const unsigned w = (unsigned)ax.weight(kx);
      in0 += w * px[0]; in1 += w * px[1]; in2 += w * px[2];
    }
    const unsigned long long wy = (unsigned long long)ay.weight(ky);
    acc0 += wy * in0; acc1 += wy * in1; acc2 += wy * in2;
  }
  const unsigned den = (unsigned)ay.den() * (unsigned)ax.den();
  out[0] = round_div(acc0, den); out[1] = round_div(acc1, den); out[2] = round_div(acc2, den);
}

// the thread's quad of page pixels: cells of them lie inside the page
__device__ __forceinline__ void store_pixels(unsigned char* __restrict__ out, const unsigned char bytes[QUAD * 3], int cells,
                                             int dword_stores) {
  if (dword_stores) {  // Wp % 4 == 0 and a 4-byte aligned page: the quad is whole and its 12 bytes are three aligned dwords
    unsigned* o = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int d = 0; d < 3; ++d)
      o[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | ((unsigned)bytes[4 * d + 3] << 24);
  } else {
    const int nb = cells * 3;
#pragma unroll
    for (int k = 0; k < QUAD * 3; ++k)
      if (k < nb) out[k] = bytes[k];
  }
}

__device__ __forceinline__ void store_labels(int* __restrict__ o, const int vals[QUAD], int cells, int vec_stores) {
  if (vec_stores) {
    *reinterpret_cast<int4*>(o) = make_int4(vals[0], vals[1], vals[2], vals[3]);
  } else {
#pragma unroll
    for (int q = 0; q < QUAD; ++q)
      if (q < cells) o[q] = vals[q];
  }
}

__global__ __launch_bounds__(THREADS) void resample_pack_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                                const int* __restrict__ table, int n,
                                                                unsigned char* __restrict__ page, int Hp, int Wp,
                                                                int dword_stores) {
  __shared__ TileLists L;
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  find_tile_placements(table, n, Hs, Ws, 1, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  const int y = ty0 + r, x = tx0 + c;
  if (y >= Hp || x >= Wp) return;
  int owner[QUAD];
  resolve_owners(L, r, c, owner);
  unsigned char bytes[QUAD * 3];
  int cur = -1;
  Placement p;
  Axis ay;
#pragma unroll
  for (int q = 0; q < QUAD; ++q) {
    unsigned v[3] = {0u, 0u, 0u};
    if (owner[q] >= 0 && x + q < Wp) {
      if (owner[q] != cur) {
        cur = owner[q];
        p = load_placement(table, cur);
        ay.init(y - p.dy, p.sh, p.dh);
      }
      resample_pixel(src, Ws, p, ay, x + q - p.dx, v);
    }
    bytes[q * 3] = (unsigned char)v[0]; bytes[q * 3 + 1] = (unsigned char)v[1]; bytes[q * 3 + 2] = (unsigned char)v[2];
  }
  store_pixels(page + ((long)y * Wp + x) * 3, bytes, min(QUAD, Wp - x), dword_stores);
}

// rough map coordinate under the centre of label cell c of a placement axis: packing.py's centre mapping
__device__ __forceinline__ int source_cell(int c, int f, int d0, int dlen, int s0, int slen, int valid, int full) {
  const long long t2 = 2LL * c * f + f - 2LL * d0;
  const long long num = (2LL * dlen * s0 + t2 * slen) * valid;
  const long long m = num / (2LL * dlen * full);
  return (int)(m < valid - 1 ? m : valid - 1);
}

__global__ __launch_bounds__(THREADS) void pack_labels_kernel(const int* __restrict__ labels, int Wl, int valid_h,
                                                              int valid_w, int Hs, int Ws, const int* __restrict__ table,
                                                              const int* __restrict__ region_ids, int n, int f,
                                                              int* __restrict__ out, int Hq, int Wq, int vec_stores) {
  __shared__ TileLists L;
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  find_tile_placements(table, n, Hs, Ws, f, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  const int y = ty0 + r, x = tx0 + c;
  if (y >= Hq || x >= Wq) return;
  int owner[QUAD];
  resolve_owners(L, r, c, owner);
  int vals[QUAD];
  int cur = -1, rid = 0, my = 0;
  Placement p;
#pragma unroll
  for (int q = 0; q < QUAD; ++q) {
    int v = 0;
    if (owner[q] >= 0 && x + q < Wq) {
      if (owner[q] != cur) {
        cur = owner[q];
        p = load_placement(table, cur);
        rid = region_ids[cur];
        my = source_cell(y, f, p.dy, p.dh, p.sy, p.sh, valid_h, Hs);
      }
      const int mx = source_cell(x + q, f, p.dx, p.dw, p.sx, p.sw, valid_w, Ws);
      const int other = labels[(long)my * Wl + mx];
      v = (other != 0 && other != rid) ? 0 : rid;
    }
    vals[q] = v;
  }
  store_labels(out + (long)y * Wq + x, vals, Wq - x, vec_stores);
}

// ---- several sources, several pages (infer_batch): one launch cuts the regions of many images into shared pages ---------
// A multi row is 12 int32 (src, page, sy, sx, sh, sw, dy, dx, dh, dw, local_id, global_id), 48 bytes; the rows are sorted by
// page and page_start (Q + 1) gives page q its slice.  The sources lie in ONE arena: a table of int64 rows per source gives
// its offset and sides, every address is arena + offset, and the offset is checked against the arena's size per row - a
// row whose source, page, sides, rectangles or table entry is out of range is absent, as a bad placement is.
struct MultiRow {
  int src, page, sy, sx, sh, sw, dy, dx, dh, dw, local_id, global_id;
  static __device__ __forceinline__ MultiRow load(const int* __restrict__ table, int i) {
    const int4* t = reinterpret_cast<const int4*>(table + (long)i * 12);
    const int4 a = t[0], b = t[1], c = t[2];
    return MultiRow{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
  }
  __device__ __forceinline__ Placement placement() const { return Placement{sy, sx, sh, sw, dy, dx, dh, dw}; }
  template <class Arena>
  __device__ __forceinline__ bool ok(const Arena& A) const {
    if (src < 0 || src >= A.S || page != A.q) return false;
    int Hs, Ws;
    return A.source_ok(src, Hs, Ws) && placement_ok(placement(), Hs, Ws);
  }
};

__device__ __forceinline__ bool side_ok(long long v) { return v >= 1 && v <= DIM_MAX; }

// image arena: bytes; a source row is (byte offset, Hs, Ws, 0) and the image takes 3*Hs*Ws bytes from its offset
struct ImageArena {
  const long long* __restrict__ sources;
  long long size;
  int S, q;
  static constexpr int WORDS = 4;
  __device__ __forceinline__ bool source_ok(int s, int& Hs, int& Ws) const {
    const long long* t = sources + (long)s * WORDS;
    const long long off = t[0], h = t[1], w = t[2];
    if (!side_ok(h) || !side_ok(w)) return false;
    Hs = (int)h; Ws = (int)w;
    return off >= 0 && off <= size && 3 * h * w <= size - off;
  }
};

// label arena: int32 words; a source row is (word offset, Hl, Wl, valid_h, valid_w, Hs, Ws, 0): the Hl x Wl map takes Hl*Wl
// words from its offset, valid_h x valid_w of it cover the Hs x Ws image the row's source rectangle refers to
struct LabelArena {
  const long long* __restrict__ sources;
  long long size;
  int S, q;
  static constexpr int WORDS = 8;
  __device__ __forceinline__ bool source_ok(int s, int& Hs, int& Ws) const {
    const long long* t = sources + (long)s * WORDS;
    const long long off = t[0], hl = t[1], wl = t[2], vh = t[3], vw = t[4], h = t[5], w = t[6];
    if (!side_ok(hl) || !side_ok(wl) || !side_ok(h) || !side_ok(w)) return false;
    Hs = (int)h; Ws = (int)w;
    return vh >= 1 && vh <= hl && vw >= 1 && vw <= wl && off >= 0 && off <= size && hl * wl <= size - off;
  }
};

// page q's slice of the rows, whatever page_start holds
__device__ __forceinline__ void page_slice(const int* __restrict__ page_start, int q, int n, int& lo, int& hi) {
  lo = min(max(page_start[q], 0), n);
  hi = min(max(page_start[q + 1], lo), n);
}

__global__ __launch_bounds__(THREADS) void resample_pack_multi_kernel(const unsigned char* __restrict__ arena,
                                                                      long long arena_bytes,
                                                                      const long long* __restrict__ sources, int S,
                                                                      const int* __restrict__ rows, int n,
                                                                      const int* __restrict__ page_start,
                                                                      unsigned char* __restrict__ pages, int Hp, int Wp,
                                                                      int dword_stores) {
  __shared__ TileLists L;
  const int q = blockIdx.z, ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  int lo, hi;
  page_slice(page_start, q, n, lo, hi);
  find_tile_rows<MultiRow>(rows, lo, hi, ImageArena{sources, arena_bytes, S, q}, 1, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  const int y = ty0 + r, x = tx0 + c;
  if (y >= Hp || x >= Wp) return;
  int owner[QUAD];
  resolve_owners(L, r, c, owner);
  unsigned char bytes[QUAD * 3];
  int cur = -1, Ws = 0;
  const unsigned char* src = arena;
  Placement p;
  Axis ay;
#pragma unroll
  for (int k = 0; k < QUAD; ++k) {
    unsigned v[3] = {0u, 0u, 0u};
    if (owner[k] >= 0 && x + k < Wp) {
      if (owner[k] != cur) {  // a row of the lists passed ok(): its source entry lies inside the arena
        cur = owner[k];
        const MultiRow m = MultiRow::load(rows, cur);
        const long long* t = sources + (long)m.src * ImageArena::WORDS;
        src = arena + t[0];
        Ws = (int)t[2];
        p = m.placement();
        ay.init(y - p.dy, p.sh, p.dh);
      }
      resample_pixel(src, Ws, p, ay, x + k - p.dx, v);
    }
    bytes[k * 3] = (unsigned char)v[0]; bytes[k * 3 + 1] = (unsigned char)v[1]; bytes[k * 3 + 2] = (unsigned char)v[2];
  }
  store_pixels(pages + (((long)q * Hp + y) * Wp + x) * 3, bytes, min(QUAD, Wp - x), dword_stores);
}

__global__ __launch_bounds__(THREADS) void pack_labels_multi_kernel(const int* __restrict__ arena, long long arena_words,
                                                                    const long long* __restrict__ sources, int S,
                                                                    const int* __restrict__ rows, int n,
                                                                    const int* __restrict__ page_start, int f,
                                                                    int* __restrict__ out, int Hq, int Wq, int vec_stores) {
  __shared__ TileLists L;
  const int q = blockIdx.z, ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  int lo, hi;
  page_slice(page_start, q, n, lo, hi);
  find_tile_rows<MultiRow>(rows, lo, hi, LabelArena{sources, arena_words, S, q}, f, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  const int y = ty0 + r, x = tx0 + c;
  if (y >= Hq || x >= Wq) return;
  int owner[QUAD];
  resolve_owners(L, r, c, owner);
  int vals[QUAD];
  int cur = -1, my = 0, Wl = 0, valid_w = 0, Ws = 0;
  const int* labels = arena;
  MultiRow m;
#pragma unroll
  for (int k = 0; k < QUAD; ++k) {
    int v = 0;
    if (owner[k] >= 0 && x + k < Wq) {
      if (owner[k] != cur) {
        cur = owner[k];
        m = MultiRow::load(rows, cur);
        const long long* t = sources + (long)m.src * LabelArena::WORDS;
        labels = arena + t[0];
        Wl = (int)t[2]; valid_w = (int)t[4]; Ws = (int)t[6];
        my = source_cell(y, f, m.dy, m.dh, m.sy, m.sh, (int)t[3], (int)t[5]);
      }
      const int mx = source_cell(x + k, f, m.dx, m.dw, m.sx, m.sw, valid_w, Ws);
      const int other = labels[(long)my * Wl + mx];
      v = (other != 0 && other != m.local_id) ? 0 : m.global_id;
    }
    vals[k] = v;
  }
  store_labels(out + ((long)q * Hq + y) * Wq + x, vals, Wq - x, vec_stores);
}

// ---- affine warps: a slanted region cut out along its own axis (inferencing/orient.py builds the rows) ----------------
// A warp row is 12 int64 (dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, 0): destination pixel (i, j) of the rectangle
// reads the source at Y = ay + i*myy + j*myx, X = ax + i*mxy + j*mxx in Q16, an integer coordinate being a pixel centre.
constexpr int WARP_WORDS = 12;
constexpr long long WARP_M_MAX = 1LL << 22, WARP_A_MAX = 1LL << 40;

struct WarpRow {
  long long dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n;
  static __device__ __forceinline__ WarpRow load(const long long* __restrict__ table, int i) {
    const long long* t = table + (long)i * WARP_WORDS;
    return WarpRow{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10]};
  }
  // as placement_ok: a row outside the bounds is absent.  Within them no intermediate leaves 64 bits (|Y| < 2^40 + 2^36)
  // and a tap outside the source reads 0, so no table content makes a kernel read outside the source.
  __device__ __forceinline__ bool ok(const SourceDims&) const {
    const auto m_ok = [](long long m) { return m >= -WARP_M_MAX && m <= WARP_M_MAX; };
    return dh >= 1 && dw >= 1 && dh <= SIDE_MAX && dw <= SIDE_MAX && dy >= 0 && dx >= 0 && dy <= DIM_MAX && dx <= DIM_MAX &&
           ay > -WARP_A_MAX && ay < WARP_A_MAX && ax > -WARP_A_MAX && ax < WARP_A_MAX && m_ok(myy) && m_ok(myx) &&
           m_ok(mxy) && m_ok(mxx) && log2n >= 0 && log2n <= 3;
  }
};

// two-tap bilinear in x on source row k (zero outside the source): sum over the taps of weight * pixel, below 2^24
__device__ __forceinline__ void warp_row_taps(const unsigned char* __restrict__ src, int Hs, int Ws, long long k,
                                              long long kx, unsigned fx, unsigned in[3]) {
  in[0] = in[1] = in[2] = 0u;
  if (k < 0 || k >= Hs) return;
  const unsigned char* row = src + (long)k * Ws * 3;
  if (kx >= 0 && kx < Ws) {
    const unsigned char* px = row + kx * 3;
    const unsigned w = 65536u - fx;
    in[0] += w * px[0]; in[1] += w * px[1]; in[2] += w * px[2];
  }
  if (fx != 0u && kx + 1 >= 0 && kx + 1 < Ws) {
    const unsigned char* px = row + (kx + 1) * 3;
    in[0] += fx * px[0]; in[1] += fx * px[1]; in[2] += fx * px[2];
  }
}

__device__ __forceinline__ void warp_pixel(const unsigned char* __restrict__ src, int Hs, int Ws, const WarpRow& p, int i,
                                           int j, unsigned out[3]) {
  const long long Y = p.ay + i * p.myy + j * p.myx, X = p.ax + i * p.mxy + j * p.mxx;
  const int ln = (int)p.log2n, n = 1 << ln;
  unsigned long long acc[3] = {0ull, 0ull, 0ull};
  for (int a = 0; a < n; ++a) {
    for (int b = 0; b < n; ++b) {
      const long long ka = 2 * a + 1 - n, kb = 2 * b + 1 - n;
      const long long Ys = Y + ((ka * p.myy + kb * p.myx) >> (1 + ln));  // arithmetic shifts: floors
      const long long Xs = X + ((ka * p.mxy + kb * p.mxx) >> (1 + ln));
      const long long ky = Ys >> 16, kx = Xs >> 16;
      const unsigned fy = (unsigned)(Ys & 65535), fx = (unsigned)(Xs & 65535);
      unsigned r0[3], r1[3] = {0u, 0u, 0u};
      warp_row_taps(src, Hs, Ws, ky, kx, fx, r0);
      if (fy != 0u) warp_row_taps(src, Hs, Ws, ky + 1, kx, fx, r1);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += (unsigned long long)(65536u - fy) * r0[c] + (unsigned long long)fy * r1[c];
    }
  }
  const int shift = 32 + 2 * ln;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (unsigned)((acc[c] + (1ull << (shift - 1))) >> shift);
}

// writes ONLY the pixels inside the destinations: the page keeps every other byte (resample_pack_kernel ran before)
__global__ __launch_bounds__(THREADS) void warp_pack_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                            const long long* __restrict__ table, int n,
                                                            unsigned char* __restrict__ page, int Hp, int Wp) {
  __shared__ TileLists L;
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  find_tile_rows<WarpRow>(table, 0, n, SourceDims{Hs, Ws}, 1, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  const int y = ty0 + r, x = tx0 + c;
  if (y >= Hp || x >= Wp) return;
  int owner[QUAD];
  resolve_owners(L, r, c, owner);
  int cur = -1;
  WarpRow p;
  for (int q = 0; q < QUAD; ++q) {
    if (owner[q] < 0 || x + q >= Wp) continue;
    if (owner[q] != cur) {
      cur = owner[q];
      p = WarpRow::load(table, cur);
    }
    unsigned v[3];
    warp_pixel(src, Hs, Ws, p, y - (int)p.dy, x + q - (int)p.dx, v);
    unsigned char* out = page + ((long)y * Wp + x + q) * 3;
    out[0] = (unsigned char)v[0]; out[1] = (unsigned char)v[1]; out[2] = (unsigned char)v[2];
  }
}

// rough map coordinate under source pixel P of an axis of S image pixels: the pixel's centre, as region_crops' inverse
__device__ __forceinline__ int map_cell(long long P, int S, int valid) {
  const long long m = ((2 * P + 1) * valid) / (2LL * S);
  return (int)(m < valid - 1 ? m : valid - 1);
}

// writes ONLY the cells whose centres lie inside the destinations (pack_labels_kernel ran before)
__global__ __launch_bounds__(THREADS) void warp_labels_kernel(const int* __restrict__ labels, int Wl, int valid_h, int valid_w,
                                                              int Hs, int Ws, const long long* __restrict__ table,
                                                              const int* __restrict__ region_ids, int n, int f,
                                                              int* __restrict__ out, int Hq, int Wq) {
  __shared__ TileLists L;
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  find_tile_rows<WarpRow>(table, 0, n, SourceDims{Hs, Ws}, f, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  const int y = ty0 + r, x = tx0 + c;
  if (y >= Hq || x >= Wq) return;
  int owner[QUAD];
  resolve_owners(L, r, c, owner);
  int cur = -1, rid = 0;
  WarpRow p;
  for (int q = 0; q < QUAD; ++q) {
    if (owner[q] < 0 || x + q >= Wq) continue;
    if (owner[q] != cur) {
      cur = owner[q];
      p = WarpRow::load(table, cur);
      rid = region_ids[cur];
    }
    const long long i2 = 2LL * y * f + f - 2 * p.dy - 1, j2 = 2LL * (x + q) * f + f - 2 * p.dx - 1;
    const long long Yp = (p.ay + ((i2 * p.myy + j2 * p.myx) >> 1) + 32768) >> 16;
    const long long Xp = (p.ax + ((i2 * p.mxy + j2 * p.mxx) >> 1) + 32768) >> 16;
    int v = 0;
    if (Yp >= 0 && Yp < Hs && Xp >= 0 && Xp < Ws) {
      const int other = labels[(long)map_cell(Yp, Hs, valid_h) * Wl + map_cell(Xp, Ws, valid_w)];
      v = (other != 0 && other != rid) ? 0 : rid;
    }
    out[(long)y * Wq + x + q] = v;
  }
}

}  // namespace

extern "C" int vkas_resample_pack_u8(const unsigned char* src, int Hs, int Ws, const int* placements, int n,
                                     unsigned char* page, int Hp, int Wp, void* stream) {
  VKAS_CHECK(src && page, "vkas_resample_pack_u8: null pointer");
  VKAS_CHECK(n >= 0 && (n == 0 || placements), "vkas_resample_pack_u8: bad table (n %d)", n);
  VKAS_CHECK(Hs >= 1 && Ws >= 1 && Hp >= 1 && Wp >= 1, "vkas_resample_pack_u8: bad dims");
  VKAS_CHECK(Hs <= DIM_MAX && Ws <= DIM_MAX && Hp <= DIM_MAX && Wp <= DIM_MAX,
             "vkas_resample_pack_u8: source and page sides must not exceed %d", DIM_MAX);
  VKAS_CHECK(vkas_aligned16(placements), "vkas_resample_pack_u8: the placement table must be 16-byte aligned");
  const int dword_stores = (Wp % 4 == 0) && ((((uintptr_t)page) & 3u) == 0);
  const dim3 grid((unsigned)vkas_cdiv(Wp, TILE_W), (unsigned)vkas_cdiv(Hp, TILE_H));
  resample_pack_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(src, Hs, Ws, placements, n, page, Hp, Wp, dword_stores);
  VKAS_LAUNCH_CHECK("resample_pack_u8");
  return VKAS_OK;
}

extern "C" int vkas_pack_region_labels(const int* labels, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws,
                                       const int* placements, const int* region_ids, int n, int fdf, int* out, int Hq,
                                       int Wq, void* stream) {
  VKAS_CHECK(labels && out, "vkas_pack_region_labels: null pointer");
  VKAS_CHECK(n >= 0 && (n == 0 || (placements && region_ids)), "vkas_pack_region_labels: bad table (n %d)", n);
  VKAS_CHECK(Hl >= 1 && Wl >= 1 && Hs >= 1 && Ws >= 1 && Hq >= 1 && Wq >= 1, "vkas_pack_region_labels: bad dims");
  VKAS_CHECK(valid_h >= 1 && valid_h <= Hl && valid_w >= 1 && valid_w <= Wl,
             "vkas_pack_region_labels: the valid part %d x %d does not fit the %d x %d label map", valid_h, valid_w, Hl, Wl);
  VKAS_CHECK(fdf >= 1 && fdf <= 64, "vkas_pack_region_labels: bad factor %d", fdf);
  VKAS_CHECK(Hl <= DIM_MAX && Wl <= DIM_MAX && Hs <= DIM_MAX && Ws <= DIM_MAX && (long)Hq * fdf <= DIM_MAX &&
                 (long)Wq * fdf <= DIM_MAX,
             "vkas_pack_region_labels: map, source and page sides must not exceed %d", DIM_MAX);
  VKAS_CHECK(vkas_aligned16(placements), "vkas_pack_region_labels: the placement table must be 16-byte aligned");
  const int vec_stores = (Wq % 4 == 0) && vkas_aligned16(out);
  const dim3 grid((unsigned)vkas_cdiv(Wq, TILE_W), (unsigned)vkas_cdiv(Hq, TILE_H));
  pack_labels_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(labels, Wl, valid_h, valid_w, Hs, Ws, placements,
                                                                region_ids, n, fdf, out, Hq, Wq, vec_stores);
  VKAS_LAUNCH_CHECK("pack_region_labels");
  return VKAS_OK;
}

extern "C" int vkas_resample_pack_u8_multi(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                           const int* rows, int n, const int* page_start, unsigned char* pages, int Q, int Hp,
                                           int Wp, void* stream) {
  VKAS_CHECK(arena && sources && page_start && pages, "vkas_resample_pack_u8_multi: null pointer");
  VKAS_CHECK(n >= 0 && (n == 0 || rows), "vkas_resample_pack_u8_multi: bad table (n %d)", n);
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "vkas_resample_pack_u8_multi: empty arena (%lld bytes, %d sources)", arena_bytes, S);
  VKAS_CHECK(Q >= 1 && Q <= 65535 && Hp >= 1 && Wp >= 1 && Hp <= DIM_MAX && Wp <= DIM_MAX,
             "vkas_resample_pack_u8_multi: %d pages of %d x %d: 1..65535 pages, sides 1..%d", Q, Hp, Wp, DIM_MAX);
  VKAS_CHECK(vkas_aligned16(rows), "vkas_resample_pack_u8_multi: the row table must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)page_start) & 3u) == 0,
             "vkas_resample_pack_u8_multi: the source table must be 8-byte aligned, page_start 4-byte aligned");
  // a page starts at a multiple of Hp*Wp*3 bytes: 4-byte aligned whenever Wp % 4 == 0 and the first one is
  const int dword_stores = (Wp % 4 == 0) && ((((uintptr_t)pages) & 3u) == 0);
  const dim3 grid((unsigned)vkas_cdiv(Wp, TILE_W), (unsigned)vkas_cdiv(Hp, TILE_H), (unsigned)Q);
  resample_pack_multi_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(arena, arena_bytes, sources, S, rows, n, page_start,
                                                                        pages, Hp, Wp, dword_stores);
  VKAS_LAUNCH_CHECK("resample_pack_u8_multi");
  return VKAS_OK;
}

extern "C" int vkas_pack_region_labels_multi(const int* label_arena, long long label_words, const long long* label_sources,
                                             int S, const int* rows, int n, const int* page_start, int fdf, int* out, int Q,
                                             int Hq, int Wq, void* stream) {
  VKAS_CHECK(label_arena && label_sources && page_start && out, "vkas_pack_region_labels_multi: null pointer");
  VKAS_CHECK(n >= 0 && (n == 0 || rows), "vkas_pack_region_labels_multi: bad table (n %d)", n);
  VKAS_CHECK(label_words >= 1 && S >= 1, "vkas_pack_region_labels_multi: empty arena (%lld words, %d sources)", label_words, S);
  VKAS_CHECK(fdf >= 1 && fdf <= 64, "vkas_pack_region_labels_multi: bad factor %d", fdf);
  VKAS_CHECK(Q >= 1 && Q <= 65535 && Hq >= 1 && Wq >= 1 && (long)Hq * fdf <= DIM_MAX && (long)Wq * fdf <= DIM_MAX,
             "vkas_pack_region_labels_multi: %d label pages of %d x %d at factor %d: 1..65535 pages, page sides up to %d", Q,
             Hq, Wq, fdf, DIM_MAX);
  VKAS_CHECK(vkas_aligned16(rows), "vkas_pack_region_labels_multi: the row table must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)label_sources) & 7u) == 0 && (((uintptr_t)page_start) & 3u) == 0 &&
                 (((uintptr_t)label_arena) & 3u) == 0,
             "vkas_pack_region_labels_multi: the source table must be 8-byte aligned, page_start and the arena 4-byte aligned");
  // a label page starts at a multiple of Hq*Wq words: 16-byte aligned whenever Wq % 4 == 0 and the first one is
  const int vec_stores = (Wq % 4 == 0) && vkas_aligned16(out);
  const dim3 grid((unsigned)vkas_cdiv(Wq, TILE_W), (unsigned)vkas_cdiv(Hq, TILE_H), (unsigned)Q);
  pack_labels_multi_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(label_arena, label_words, label_sources, S, rows, n,
                                                                      page_start, fdf, out, Hq, Wq, vec_stores);
  VKAS_LAUNCH_CHECK("pack_region_labels_multi");
  return VKAS_OK;
}

extern "C" int vkas_warp_pack_u8(const unsigned char* src, int Hs, int Ws, const long long* warps, int n, unsigned char* page,
                                 int Hp, int Wp, void* stream) {
  VKAS_CHECK(src && page, "vkas_warp_pack_u8: null pointer");
  VKAS_CHECK(n >= 0 && (n == 0 || warps), "vkas_warp_pack_u8: bad table (n %d)", n);
  VKAS_CHECK(Hs >= 1 && Ws >= 1 && Hp >= 1 && Wp >= 1, "vkas_warp_pack_u8: bad dims");
  VKAS_CHECK(Hs <= DIM_MAX && Ws <= DIM_MAX && Hp <= DIM_MAX && Wp <= DIM_MAX,
             "vkas_warp_pack_u8: source and page sides must not exceed %d", DIM_MAX);
  VKAS_CHECK((((uintptr_t)warps) & 7u) == 0, "vkas_warp_pack_u8: the warp table must be 8-byte aligned");
  if (n == 0) return VKAS_OK;  // nothing to write: the page stays as it is
  const dim3 grid((unsigned)vkas_cdiv(Wp, TILE_W), (unsigned)vkas_cdiv(Hp, TILE_H));
  warp_pack_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(src, Hs, Ws, warps, n, page, Hp, Wp);
  VKAS_LAUNCH_CHECK("warp_pack_u8");
  return VKAS_OK;
}

extern "C" int vkas_warp_region_labels(const int* labels, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws,
                                       const long long* warps, const int* region_ids, int n, int fdf, int* out, int Hq, int Wq,
                                       void* stream) {
  VKAS_CHECK(labels && out, "vkas_warp_region_labels: null pointer");
  VKAS_CHECK(n >= 0 && (n == 0 || (warps && region_ids)), "vkas_warp_region_labels: bad table (n %d)", n);
  VKAS_CHECK(Hl >= 1 && Wl >= 1 && Hs >= 1 && Ws >= 1 && Hq >= 1 && Wq >= 1, "vkas_warp_region_labels: bad dims");
  VKAS_CHECK(valid_h >= 1 && valid_h <= Hl && valid_w >= 1 && valid_w <= Wl,
             "vkas_warp_region_labels: the valid part %d x %d does not fit the %d x %d label map", valid_h, valid_w, Hl, Wl);
  VKAS_CHECK(fdf >= 1 && fdf <= 64, "vkas_warp_region_labels: bad factor %d", fdf);
  VKAS_CHECK(Hl <= DIM_MAX && Wl <= DIM_MAX && Hs <= DIM_MAX && Ws <= DIM_MAX && (long)Hq * fdf <= DIM_MAX &&
                 (long)Wq * fdf <= DIM_MAX,
             "vkas_warp_region_labels: map, source and page sides must not exceed %d", DIM_MAX);
  VKAS_CHECK((((uintptr_t)warps) & 7u) == 0, "vkas_warp_region_labels: the warp table must be 8-byte aligned");
  if (n == 0) return VKAS_OK;
  const dim3 grid((unsigned)vkas_cdiv(Wq, TILE_W), (unsigned)vkas_cdiv(Hq, TILE_H));
  warp_labels_kernel<<<grid, THREADS, 0, vkas_stream(stream)>>>(labels, Wl, valid_h, valid_w, Hs, Ws, warps, region_ids, n, fdf,
                                                                out, Hq, Wq);
  VKAS_LAUNCH_CHECK("warp_region_labels");
  return VKAS_OK;
}
