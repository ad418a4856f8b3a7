// Crop, rescale and pack the text regions into the pages of the precise pass (inferencing/adaptive_scaling.py:190-293 restated
// on pixels; the rule and the host oracles: inferencing/packing.py): a variable-ratio gather / resample of 3-byte pixels into
// the disjoint rectangles of packed pages, and the int32 region-label pages that go with them.
//
// Every kernel is driven from the output and begins with the one tile prologue: a workgroup owns a tile of TILE_H x TILE_W
// output cells (page pixels / label cells) and searches its table for the rows that reach into the tile - every wave takes
// 64 rows at a time, ballots the hits and appends (row index, hit rectangle clipped to the tile) to its own list in LDS; no
// atomics, and the order is irrelevant because destinations are disjoint, which also bounds a list by the tile's cell count
// - then every thread resolves the owner of its four adjacent cells from the lists (wave-uniform LDS reads).
//
// Two bodies produce the cells, each templated on the table's row type and on a source policy: pack_pixels, 12 bytes of page
// (three aligned dword stores when Wp % 4 == 0), and pack_labels, four labels (one 16-byte store when Wq % 4 == 0).  Both
// write every output byte exactly once - zero where no row reaches - so a call leaves nothing of the buffer's earlier
// contents.  The policy says whether a row is valid and what a row reads from: the kernel's one image / label map, or the
// row's entry in the source table of an arena (infer_batch).  The warp kernels (slanted regions) share the prologue and the
// one-source policies, keep their own cell arithmetic and write only inside their destinations.
//
// The source pixels are gathered directly (byte loads through the vector L1): see DESIGN.md for why source rows are not
// staged in LDS.  All arithmetic is integer: inner row sums in 32 bits, the outer sum in 64, one rounding division by the
// product of the axis denominators.
#include "vkas_common.h"
#include "warp_pixel.h"  // WarpRow, warp_pixel, SIDE_MAX, DIM_MAX, side_ok

namespace {

constexpr int TILE_H = 16, TILE_W = 64, QUAD = 4;           // cells per tile; cells per thread along x
constexpr int THREADS = TILE_H * TILE_W / QUAD;             // 256
constexpr int WAVES = THREADS / 64;
constexpr int LIST_CAP = TILE_H * TILE_W;                   // disjoint placements: at most one per cell of the tile

// ---- row types: load(table, i), the destination rectangle dy, dx, dh, dw in page pixels, and ok(what the check needs) -----
// The kernels trust the host's disjointness check, but never a row's bounds: a row that fails ok() is treated as absent, so
// no table content can make a kernel read outside its source (writes are bounded by the output tile in any case).

// 8 int32: the source rectangle of an Hs x Ws image and the destination rectangle
struct Placement {
  int sy, sx, sh, sw, dy, dx, dh, dw;
  static __device__ __forceinline__ Placement load(const int* __restrict__ table, int i) {
    const int4* t = reinterpret_cast<const int4*>(table + (long)i * 8);
    const int4 a = t[0], b = t[1];
    return Placement{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  }
  __device__ __forceinline__ bool ok(int Hs, int Ws) const {
    return sh >= 1 && sw >= 1 && dh >= 1 && dw >= 1 && sh <= SIDE_MAX && sw <= SIDE_MAX && dh <= SIDE_MAX && dw <= SIDE_MAX &&
           sy >= 0 && sx >= 0 && sy <= Hs - sh && sx <= Ws - sw && dy >= 0 && dx >= 0 && dy <= DIM_MAX && dx <= DIM_MAX;
  }
};

// 12 int32 (src, page, sy, sx, sh, sw, dy, dx, dh, dw, local_id, global_id), 48 bytes: a placement of source src of an arena
// on page `page`; the rows are sorted by page and page_start (Q + 1) gives page q its slice
struct MultiRow : Placement {
  int src, page, local_id, global_id;
  static __device__ __forceinline__ MultiRow load(const int* __restrict__ table, int i) {
    const int4* t = reinterpret_cast<const int4*>(table + (long)i * 12);
    const int4 a = t[0], b = t[1], c = t[2];
    return MultiRow{{a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y}, a.x, a.y, c.z, c.w};
  }
};

// ---- source policies: ok(row), and after select(row, its index) what that row reads from ----------------------------------

// the one image of the kernel's arguments
struct OneImage {
  const unsigned char* __restrict__ src;
  int Hs, Ws;
  __device__ __forceinline__ bool ok(const Placement& p) const { return p.ok(Hs, Ws); }
  __device__ __forceinline__ bool ok(const WarpRow& p) const { return p.ok(); }
  __device__ __forceinline__ void select(const Placement&, int) {}
};

// the one rough label map of the kernel's arguments, valid_h x valid_w of which cover the Hs x Ws image; ids: region_ids[row]
struct OneLabelMap {
  const int* __restrict__ labels;
  int Wl, valid_h, valid_w, Hs, Ws;
  const int* __restrict__ region_ids;
  int local_id = 0, global_id = 0;
  __device__ __forceinline__ bool ok(const Placement& p) const { return p.ok(Hs, Ws); }
  __device__ __forceinline__ bool ok(const WarpRow& p) const { return p.ok(); }
  template <class Row>
  __device__ __forceinline__ void select(const Row&, int i) { local_id = global_id = region_ids[i]; }
};

// The sources of a multi pack lie in ONE arena: a table of int64 rows per source gives its offset and sides, and every
// address is arena + offset.  select(row with src in [0, S)) says whether that entry lies inside the arena; a row is valid
// for the grid layer of page A.q when it does and the row's rectangles lie inside that source.
template <class Arena>
__device__ __forceinline__ bool arena_row_ok(Arena A, const MultiRow& r) {
  return r.src >= 0 && r.src < A.S && r.page == A.q && A.select(r, 0) && r.ok(A.Hs, A.Ws);
}

// image arena: bytes; a source row is (byte offset, Hs, Ws, 0) and the image takes 3*Hs*Ws bytes from its offset
struct ImageArena {
  const unsigned char* __restrict__ arena;
  long long size;
  const long long* __restrict__ sources;
  int S, q;
  const unsigned char* src = nullptr;  // of the selected row
  int Hs = 0, Ws = 0;
  __device__ __forceinline__ bool ok(const MultiRow& r) const { return arena_row_ok(*this, r); }
  __device__ __forceinline__ bool select(const MultiRow& r, int) {
    const long long* t = sources + (long)r.src * 4;
    const long long off = t[0], h = t[1], w = t[2];
    src = arena + off;
    Hs = (int)h; Ws = (int)w;
    return side_ok(h) && side_ok(w) && off >= 0 && off <= size && 3 * h * w <= size - off;
  }
};

// label arena: int32 words; a source row is (word offset, Hl, Wl, valid_h, valid_w, Hs, Ws, 0): the Hl x Wl map takes Hl*Wl
// words from its offset, valid_h x valid_w of it cover the Hs x Ws image the row's source rectangle refers to
struct LabelArena {
  const int* __restrict__ arena;
  long long size;
  const long long* __restrict__ sources;
  int S, q;
  const int* labels = nullptr;  // of the selected row
  int Wl = 0, valid_h = 0, valid_w = 0, Hs = 0, Ws = 0, local_id = 0, global_id = 0;
  __device__ __forceinline__ bool ok(const MultiRow& r) const { return arena_row_ok(*this, r); }
  __device__ __forceinline__ bool select(const MultiRow& r, int) {
    const long long* t = sources + (long)r.src * 8;
    const long long off = t[0], hl = t[1], wl = t[2], vh = t[3], vw = t[4], h = t[5], w = t[6];
    labels = arena + off;
    Wl = (int)wl; valid_h = (int)vh; valid_w = (int)vw; Hs = (int)h; Ws = (int)w;
    local_id = r.local_id; global_id = r.global_id;
    return side_ok(hl) && side_ok(wl) && side_ok(h) && side_ok(w) && vh >= 1 && vh <= hl && vw >= 1 && vw <= wl && off >= 0 &&
           off <= size && hl * wl <= size - off;
  }
};

// page q's slice of the rows, whatever page_start holds
__device__ __forceinline__ int2 page_slice(const int* __restrict__ page_start, int q, int n) {
  const int lo = min(max(page_start[q], 0), n);
  return make_int2(lo, min(max(page_start[q + 1], lo), n));
}

// ---- the tile prologue ------------------------------------------------------------------------------------------------------

// cells [lo, hi) of one axis whose centres c*f + f/2 lie in the page interval [d0, d0 + dlen); f == 1: the pixels themselves
__device__ __forceinline__ void cell_range(int d0, int dlen, int f, int& lo, int& hi) {
  const int a = 2 * d0 - f, b = 2 * (d0 + dlen) - f;
  lo = a <= 0 ? 0 : (a + 2 * f - 1) / (2 * f);
  hi = b <= 0 ? 0 : (b + 2 * f - 1) / (2 * f);
}

struct TileLists {
  int2 entry[WAVES][LIST_CAP];  // (row index, y0 | y1 << 8 | x0 << 16 | x1 << 24: hit rectangle in tile cells, exclusive ends)
  int count[WAVES];
};

// the rows [begin, end) of the table that own at least one cell of the tile at (ty0, tx0); f = page pixels per cell
template <class Row, class Word, class Source>
__device__ __forceinline__ void find_tile_rows(const Word* __restrict__ table, int begin, int end, const Source& S, int f,
                                               int ty0, int tx0, TileLists& L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
  for (int base = begin + wave * 64; base < end; base += THREADS) {
    const int i = base + lane;
    bool hit = false;
    int packed = 0;
    if (i < end) {
      const Row p = Row::load(table, i);
      if (S.ok(p)) {
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

// a thread's four cells (y, x .. x + 3) of the H x W output and their owner rows; outside: the quad begins off the output
// (owner is unset then, and the thread has passed the block's only barrier)
struct Tile {
  int y, x, owner[QUAD];
  bool outside;
};

template <class Row, class Word, class Source>
__device__ __forceinline__ Tile tile_prologue(const Word* __restrict__ table, int begin, int end, const Source& S, int f, int H,
                                              int W) {
  __shared__ TileLists L;
  const int ty0 = blockIdx.y * TILE_H, tx0 = blockIdx.x * TILE_W;
  find_tile_rows<Row>(table, begin, end, S, f, ty0, tx0, L);
  const int r = threadIdx.x / (TILE_W / QUAD), c = (threadIdx.x % (TILE_W / QUAD)) * QUAD;
  Tile t;
  t.y = ty0 + r; t.x = tx0 + c;
  t.outside = t.y >= H || t.x >= W;
  if (!t.outside) resolve_owners(L, r, c, t.owner);
  return t;
}

// ---- the pixel body ---------------------------------------------------------------------------------------------------------

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

// the Hp x Wp page at `page` from the rows [begin, end) of the table
template <class Row, class Source>
__device__ __forceinline__ void pack_pixels(Source S, const int* __restrict__ table, int begin, int end,
                                            unsigned char* __restrict__ page, int Hp, int Wp, int dword_stores) {
  const Tile t = tile_prologue<Row>(table, begin, end, S, 1, Hp, Wp);
  if (t.outside) return;
  unsigned char bytes[QUAD * 3];
  int cur = -1;
  Row p;
  Axis ay;
#pragma unroll
  for (int q = 0; q < QUAD; ++q) {
    unsigned v[3] = {0u, 0u, 0u};
    if (t.owner[q] >= 0 && t.x + q < Wp) {
      if (t.owner[q] != cur) {
        cur = t.owner[q];
        p = Row::load(table, cur);
        S.select(p, cur);
        ay.init(t.y - p.dy, p.sh, p.dh);
      }
      resample_pixel(S.src, S.Ws, p, ay, t.x + q - p.dx, v);
    }
    bytes[q * 3] = (unsigned char)v[0]; bytes[q * 3 + 1] = (unsigned char)v[1]; bytes[q * 3 + 2] = (unsigned char)v[2];
  }
  store_pixels(page + ((long)t.y * Wp + t.x) * 3, bytes, min(QUAD, Wp - t.x), dword_stores);
}

__global__ __launch_bounds__(THREADS) void resample_pack_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                                const int* __restrict__ table, int n,
                                                                unsigned char* __restrict__ page, int Hp, int Wp,
                                                                int dword_stores) {
  pack_pixels<Placement>(OneImage{src, Hs, Ws}, table, 0, n, page, Hp, Wp, dword_stores);
}

__global__ __launch_bounds__(THREADS) void resample_pack_multi_kernel(const unsigned char* __restrict__ arena,
                                                                      long long arena_bytes,
                                                                      const long long* __restrict__ sources, int S,
                                                                      const int* __restrict__ rows, int n,
                                                                      const int* __restrict__ page_start,
                                                                      unsigned char* __restrict__ pages, int Hp, int Wp,
                                                                      int dword_stores) {
  const int q = blockIdx.z;
  const int2 slice = page_slice(page_start, q, n);
  pack_pixels<MultiRow>(ImageArena{arena, arena_bytes, sources, S, q}, rows, slice.x, slice.y, pages + (long)q * Hp * Wp * 3,
                        Hp, Wp, dword_stores);
}

// ---- the label body ---------------------------------------------------------------------------------------------------------

// rough map coordinate under the centre of label cell c of a placement axis: packing.py's centre mapping
__device__ __forceinline__ int source_cell(int c, int f, int d0, int dlen, int s0, int slen, int valid, int full) {
  const long long t2 = 2LL * c * f + f - 2LL * d0;
  const long long num = (2LL * dlen * s0 + t2 * slen) * valid;
  const long long m = num / (2LL * dlen * full);
  return (int)(m < valid - 1 ? m : valid - 1);
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

// the Hq x Wq label page at `out`, f page pixels per cell, from the rows [begin, end) of the table
template <class Row, class Source>
__device__ __forceinline__ void pack_labels(Source S, const int* __restrict__ table, int begin, int end, int f,
                                            int* __restrict__ out, int Hq, int Wq, int vec_stores) {
  const Tile t = tile_prologue<Row>(table, begin, end, S, f, Hq, Wq);
  if (t.outside) return;
  int vals[QUAD];
  int cur = -1, my = 0;
  Row p;
#pragma unroll
  for (int q = 0; q < QUAD; ++q) {
    int v = 0;
    if (t.owner[q] >= 0 && t.x + q < Wq) {
      if (t.owner[q] != cur) {
        cur = t.owner[q];
        p = Row::load(table, cur);
        S.select(p, cur);
        my = source_cell(t.y, f, p.dy, p.dh, p.sy, p.sh, S.valid_h, S.Hs);
      }
      const int mx = source_cell(t.x + q, f, p.dx, p.dw, p.sx, p.sw, S.valid_w, S.Ws);
      const int other = S.labels[(long)my * S.Wl + mx];
      v = (other != 0 && other != S.local_id) ? 0 : S.global_id;
    }
    vals[q] = v;
  }
  store_labels(out + (long)t.y * Wq + t.x, vals, Wq - t.x, vec_stores);
}

__global__ __launch_bounds__(THREADS) void pack_labels_kernel(const int* __restrict__ labels, int Wl, int valid_h,
                                                              int valid_w, int Hs, int Ws, const int* __restrict__ table,
                                                              const int* __restrict__ region_ids, int n, int f,
                                                              int* __restrict__ out, int Hq, int Wq, int vec_stores) {
  pack_labels<Placement>(OneLabelMap{labels, Wl, valid_h, valid_w, Hs, Ws, region_ids}, table, 0, n, f, out, Hq, Wq,
                         vec_stores);
}

__global__ __launch_bounds__(THREADS) void pack_labels_multi_kernel(const int* __restrict__ arena, long long arena_words,
                                                                    const long long* __restrict__ sources, int S,
                                                                    const int* __restrict__ rows, int n,
                                                                    const int* __restrict__ page_start, int f,
                                                                    int* __restrict__ out, int Hq, int Wq, int vec_stores) {
  const int q = blockIdx.z;
  const int2 slice = page_slice(page_start, q, n);
  pack_labels<MultiRow>(LabelArena{arena, arena_words, sources, S, q}, rows, slice.x, slice.y, f,
                        out + (long)q * Hq * Wq, Hq, Wq, vec_stores);
}

// ---- the warp kernels: the prologue and the one-source policies, their own cell rules (the pixel: warp_pixel.h) -----------

// writes ONLY the pixels inside the destinations: the page keeps every other byte (resample_pack_kernel ran before)
__global__ __launch_bounds__(THREADS) void warp_pack_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                            const long long* __restrict__ table, int n,
                                                            unsigned char* __restrict__ page, int Hp, int Wp) {
  const OneImage S{src, Hs, Ws};
  const Tile t = tile_prologue<WarpRow>(table, 0, n, S, 1, Hp, Wp);
  if (t.outside) return;
  int cur = -1;
  WarpRow p;
  for (int q = 0; q < QUAD; ++q) {
    if (t.owner[q] < 0 || t.x + q >= Wp) continue;
    if (t.owner[q] != cur) {
      cur = t.owner[q];
      p = WarpRow::load(table, cur);
    }
    unsigned v[3];
    warp_pixel(S.src, S.Hs, S.Ws, p, t.y - (int)p.dy, t.x + q - (int)p.dx, v);
    unsigned char* out = page + ((long)t.y * Wp + t.x + q) * 3;
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
  OneLabelMap S{labels, Wl, valid_h, valid_w, Hs, Ws, region_ids};
  const Tile t = tile_prologue<WarpRow>(table, 0, n, S, f, Hq, Wq);
  if (t.outside) return;
  int cur = -1;
  WarpRow p;
  for (int q = 0; q < QUAD; ++q) {
    if (t.owner[q] < 0 || t.x + q >= Wq) continue;
    if (t.owner[q] != cur) {
      cur = t.owner[q];
      p = WarpRow::load(table, cur);
      S.select(p, cur);
    }
    const long long i2 = 2LL * t.y * f + f - 2 * p.dy - 1, j2 = 2LL * (t.x + q) * f + f - 2 * p.dx - 1;
    const long long Yp = (p.ay + ((i2 * p.myy + j2 * p.myx) >> 1) + 32768) >> 16;
    const long long Xp = (p.ax + ((i2 * p.mxy + j2 * p.mxx) >> 1) + 32768) >> 16;
    int v = 0;
    if (Yp >= 0 && Yp < S.Hs && Xp >= 0 && Xp < S.Ws) {
      const int other = S.labels[(long)map_cell(Yp, S.Hs, S.valid_h) * S.Wl + map_cell(Xp, S.Ws, S.valid_w)];
      v = (other != 0 && other != S.local_id) ? 0 : S.global_id;
    }
    out[(long)t.y * Wq + t.x + q] = v;
  }
}

// ---- the argument checks the entry points share; who: the entry point's name as its messages give it ---------------------

// a table of n rows (present: every pointer that n > 0 needs is there) whose row type needs the given alignment
int check_table(const char* who, int n, bool present, const void* table, const char* what, unsigned align) {
  VKAS_CHECK(n >= 0 && (n == 0 || present), "%s: bad table (n %d)", who, n);
  VKAS_CHECK((((uintptr_t)table) & (align - 1u)) == 0, "%s: the %s table must be %u-byte aligned", who, what, align);
  return VKAS_OK;
}

int check_image_dims(const char* who, int Hs, int Ws, int Hp, int Wp) {
  VKAS_CHECK(Hs >= 1 && Ws >= 1 && Hp >= 1 && Wp >= 1, "%s: bad dims", who);
  VKAS_CHECK(Hs <= DIM_MAX && Ws <= DIM_MAX && Hp <= DIM_MAX && Wp <= DIM_MAX, "%s: source and page sides must not exceed %d",
             who, DIM_MAX);
  return VKAS_OK;
}

// one Hl x Wl label map of an Hs x Ws image and an Hq x Wq label page at factor fdf
int check_label_geometry(const char* who, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws, int fdf, int Hq, int Wq) {
  VKAS_CHECK(Hl >= 1 && Wl >= 1 && Hs >= 1 && Ws >= 1 && Hq >= 1 && Wq >= 1, "%s: bad dims", who);
  VKAS_CHECK(valid_h >= 1 && valid_h <= Hl && valid_w >= 1 && valid_w <= Wl,
             "%s: the valid part %d x %d does not fit the %d x %d label map", who, valid_h, valid_w, Hl, Wl);
  VKAS_CHECK(fdf >= 1 && fdf <= 64, "%s: bad factor %d", who, fdf);
  VKAS_CHECK(Hl <= DIM_MAX && Wl <= DIM_MAX && Hs <= DIM_MAX && Ws <= DIM_MAX && (long)Hq * fdf <= DIM_MAX &&
                 (long)Wq * fdf <= DIM_MAX,
             "%s: map, source and page sides must not exceed %d", who, DIM_MAX);
  return VKAS_OK;
}

dim3 tile_grid(int H, int W, int Q = 1) {
  return dim3((unsigned)vkas_cdiv(W, TILE_W), (unsigned)vkas_cdiv(H, TILE_H), (unsigned)Q);
}

}  // namespace

extern "C" int vkas_resample_pack_u8(const unsigned char* src, int Hs, int Ws, const int* placements, int n,
                                     unsigned char* page, int Hp, int Wp, void* stream) {
  VKAS_CHECK(src && page, "%s: null pointer", __func__);
  if (int e = check_table(__func__, n, placements, placements, "placement", 16)) return e;
  if (int e = check_image_dims(__func__, Hs, Ws, Hp, Wp)) return e;
  const int dword_stores = (Wp % 4 == 0) && ((((uintptr_t)page) & 3u) == 0);
  resample_pack_kernel<<<tile_grid(Hp, Wp), THREADS, 0, vkas_stream(stream)>>>(src, Hs, Ws, placements, n, page, Hp, Wp,
                                                                               dword_stores);
  VKAS_LAUNCH_CHECK("resample_pack_u8");
  return VKAS_OK;
}

extern "C" int vkas_pack_region_labels(const int* labels, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws,
                                       const int* placements, const int* region_ids, int n, int fdf, int* out, int Hq,
                                       int Wq, void* stream) {
  VKAS_CHECK(labels && out, "%s: null pointer", __func__);
  if (int e = check_table(__func__, n, placements && region_ids, placements, "placement", 16)) return e;
  if (int e = check_label_geometry(__func__, Hl, Wl, valid_h, valid_w, Hs, Ws, fdf, Hq, Wq)) return e;
  const int vec_stores = (Wq % 4 == 0) && vkas_aligned16(out);
  pack_labels_kernel<<<tile_grid(Hq, Wq), THREADS, 0, vkas_stream(stream)>>>(labels, Wl, valid_h, valid_w, Hs, Ws, placements,
                                                                             region_ids, n, fdf, out, Hq, Wq, vec_stores);
  VKAS_LAUNCH_CHECK("pack_region_labels");
  return VKAS_OK;
}

extern "C" int vkas_resample_pack_u8_multi(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                           const int* rows, int n, const int* page_start, unsigned char* pages, int Q, int Hp,
                                           int Wp, void* stream) {
  VKAS_CHECK(arena && sources && page_start && pages, "%s: null pointer", __func__);
  if (int e = check_table(__func__, n, rows, rows, "row", 16)) return e;
  VKAS_CHECK(arena_bytes >= 1 && S >= 1, "%s: empty arena (%lld bytes, %d sources)", __func__, arena_bytes, S);
  VKAS_CHECK(Q >= 1 && Q <= 65535 && Hp >= 1 && Wp >= 1 && Hp <= DIM_MAX && Wp <= DIM_MAX,
             "%s: %d pages of %d x %d: 1..65535 pages, sides 1..%d", __func__, Q, Hp, Wp, DIM_MAX);
  VKAS_CHECK((((uintptr_t)sources) & 7u) == 0 && (((uintptr_t)page_start) & 3u) == 0,
             "%s: the source table must be 8-byte aligned, page_start 4-byte aligned", __func__);
  // a page starts at a multiple of Hp*Wp*3 bytes: 4-byte aligned whenever Wp % 4 == 0 and the first one is
  const int dword_stores = (Wp % 4 == 0) && ((((uintptr_t)pages) & 3u) == 0);
  resample_pack_multi_kernel<<<tile_grid(Hp, Wp, Q), THREADS, 0, vkas_stream(stream)>>>(
      arena, arena_bytes, sources, S, rows, n, page_start, pages, Hp, Wp, dword_stores);
  VKAS_LAUNCH_CHECK("resample_pack_u8_multi");
  return VKAS_OK;
}

extern "C" int vkas_pack_region_labels_multi(const int* label_arena, long long label_words, const long long* label_sources,
                                             int S, const int* rows, int n, const int* page_start, int fdf, int* out, int Q,
                                             int Hq, int Wq, void* stream) {
  VKAS_CHECK(label_arena && label_sources && page_start && out, "%s: null pointer", __func__);
  if (int e = check_table(__func__, n, rows, rows, "row", 16)) return e;
  VKAS_CHECK(label_words >= 1 && S >= 1, "%s: empty arena (%lld words, %d sources)", __func__, label_words, S);
  VKAS_CHECK(fdf >= 1 && fdf <= 64, "%s: bad factor %d", __func__, fdf);
  VKAS_CHECK(Q >= 1 && Q <= 65535 && Hq >= 1 && Wq >= 1 && (long)Hq * fdf <= DIM_MAX && (long)Wq * fdf <= DIM_MAX,
             "%s: %d label pages of %d x %d at factor %d: 1..65535 pages, page sides up to %d", __func__, Q, Hq, Wq, fdf,
             DIM_MAX);
  VKAS_CHECK((((uintptr_t)label_sources) & 7u) == 0 && (((uintptr_t)page_start) & 3u) == 0 &&
                 (((uintptr_t)label_arena) & 3u) == 0,
             "%s: the source table must be 8-byte aligned, page_start and the arena 4-byte aligned", __func__);
  // a label page starts at a multiple of Hq*Wq words: 16-byte aligned whenever Wq % 4 == 0 and the first one is
  const int vec_stores = (Wq % 4 == 0) && vkas_aligned16(out);
  pack_labels_multi_kernel<<<tile_grid(Hq, Wq, Q), THREADS, 0, vkas_stream(stream)>>>(
      label_arena, label_words, label_sources, S, rows, n, page_start, fdf, out, Hq, Wq, vec_stores);
  VKAS_LAUNCH_CHECK("pack_region_labels_multi");
  return VKAS_OK;
}

extern "C" int vkas_warp_pack_u8(const unsigned char* src, int Hs, int Ws, const long long* warps, int n, unsigned char* page,
                                 int Hp, int Wp, void* stream) {
  VKAS_CHECK(src && page, "%s: null pointer", __func__);
  if (int e = check_table(__func__, n, warps, warps, "warp", 8)) return e;
  if (int e = check_image_dims(__func__, Hs, Ws, Hp, Wp)) return e;
  if (n == 0) return VKAS_OK;  // nothing to write: the page stays as it is
  warp_pack_kernel<<<tile_grid(Hp, Wp), THREADS, 0, vkas_stream(stream)>>>(src, Hs, Ws, warps, n, page, Hp, Wp);
  VKAS_LAUNCH_CHECK("warp_pack_u8");
  return VKAS_OK;
}

extern "C" int vkas_warp_region_labels(const int* labels, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws,
                                       const long long* warps, const int* region_ids, int n, int fdf, int* out, int Hq, int Wq,
                                       void* stream) {
  VKAS_CHECK(labels && out, "%s: null pointer", __func__);
  if (int e = check_table(__func__, n, warps && region_ids, warps, "warp", 8)) return e;
  if (int e = check_label_geometry(__func__, Hl, Wl, valid_h, valid_w, Hs, Ws, fdf, Hq, Wq)) return e;
  if (n == 0) return VKAS_OK;
  warp_labels_kernel<<<tile_grid(Hq, Wq), THREADS, 0, vkas_stream(stream)>>>(labels, Wl, valid_h, valid_w, Hs, Ws, warps,
                                                                             region_ids, n, fdf, out, Hq, Wq);
  VKAS_LAUNCH_CHECK("warp_region_labels");
  return VKAS_OK;
}
