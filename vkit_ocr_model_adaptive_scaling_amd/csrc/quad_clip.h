// What the pair passes over match rows (quad_pairs.h) are made of: the tile constants, the staging of a tile's 128 rows into
// LDS and the convex clip.
//
// The clip is Sutherland-Hodgman in binary64, every operation rounded once (qm_* helpers under contract(off): see labels.hip
// for why __dmul_rn alone is not enough).  The two 8-vertex rings are indexed dynamically, so they live in per-thread LDS
// slots, [ring][vertex][coordinate][thread]: consecutive lanes hit consecutive 8-byte banks, and nothing goes to scratch.
#pragma once
#include "vkas_common.h"

#include <limits.h>

namespace {

constexpr int QM_TILE = 64;                // gts and preds per tile
constexpr int QM_THREADS = 128;            // pair pass
constexpr int QM_WAVES = QM_THREADS / 64;
constexpr int QM_LIST = QM_TILE * QM_TILE / QM_WAVES;  // list slots per wave
constexpr int QM_RING = 8;                 // vertices per ring
constexpr int QM_MAX = 8192;               // quads per image and side (the LDS state of the scan and matching passes)
constexpr int QM_BLOCK = 1024;             // scan and matching passes

#pragma clang fp contract(off)
__device__ __forceinline__ double qm_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double qm_add(double a, double b) { return a + b; }
__device__ __forceinline__ double qm_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double qm_div(double a, double b) { return a / b; }
#pragma clang fp contract(fast)

__device__ __forceinline__ int qm_clamp(int v, int hi) { return min(max(v, 0), hi); }
__device__ __forceinline__ bool qm_finite_bits(unsigned b) { return (b & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int qm_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

inline size_t qm_align(size_t v) { return (v + 255) & ~(size_t)255; }

// One half of the 128 rows of a tile (64 gts from g0, then 64 preds from p0) into s_rows[row * 4 + part]: half 0 = the
// corners (parts 0, 1), half 1 = the box (part 2) and area, valid, zero (part 3); two 16-byte loads per thread.  The row
// index is clamped to the table; a row beyond the count becomes a zero row (valid = 0) after the load.  fix(v, is_gt, at,
// part) may rewrite a loaded part before it is stored (the prob bits and care flags that ride in the zero word).
template <class Fix>
__device__ __forceinline__ void qm_stage_half(int4* s_rows, const int* __restrict__ gt_rows, const int* __restrict__ pred_rows,
                                              int b, int M, int N, int g0, int p0, int ng, int np, int half, int tid, Fix fix) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * QM_THREADS, row = i >> 1, part = 2 * half + (i & 1);
    int4 v;
    bool keep;
    int at;
    if (row < QM_TILE) {
      at = min(g0 + row, M - 1);
      v = reinterpret_cast<const int4*>(gt_rows)[((long)b * M + at) * 4 + part];
      keep = g0 + row < ng;
    } else {
      at = min(p0 + row - QM_TILE, N - 1);
      v = reinterpret_cast<const int4*>(pred_rows)[((long)b * N + at) * 4 + part];
      keep = p0 + row - QM_TILE < np;
    }
    fix(v, row < QM_TILE, at, part);
    s_rows[row * 4 + part] = keep ? v : make_int4(0, 0, 0, 0);
  }
}

// The rule's IoU of the LDS rows g and p (four int4 each), and through inter2_out the clamped twice-intersection it is made
// of (quad_inter2_host).  ring: this thread's slots, element (r, k, c) at ring[((r * QM_RING + k) * 2 + c) * QM_THREADS].
__device__ __forceinline__ double qm_inter2_iou(const int4* g, const int4* p, double* ring, double* inter2_out) {
#define QM_AT(r, k, c) ring[(((r) * QM_RING + (k)) * 2 + (c)) * QM_THREADS]
  const int4 g01 = g[0], g23 = g[1], gb = g[2], ga = g[3];
  const int4 p01 = p[0], p23 = p[1], pb = p[2], pa = p[3];
  const long oy = min(gb.x, pb.x), ox = min(gb.y, pb.y);
  const double gy[4] = {(double)(g01.x - oy), (double)(g01.z - oy), (double)(g23.x - oy), (double)(g23.z - oy)};
  const double gx[4] = {(double)(g01.y - ox), (double)(g01.w - ox), (double)(g23.y - ox), (double)(g23.w - ox)};
  QM_AT(0, 0, 0) = (double)(p01.x - oy);
  QM_AT(0, 0, 1) = (double)(p01.y - ox);
  QM_AT(0, 1, 0) = (double)(p01.z - oy);
  QM_AT(0, 1, 1) = (double)(p01.w - ox);
  QM_AT(0, 2, 0) = (double)(p23.x - oy);
  QM_AT(0, 2, 1) = (double)(p23.y - ox);
  QM_AT(0, 3, 0) = (double)(p23.z - oy);
  QM_AT(0, 3, 1) = (double)(p23.w - ox);
  int n = 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int src = e & 1, dst = src ^ 1;
    const double ay = gy[e], ax = gx[e];
    const double ey = qm_sub(gy[(e + 1) & 3], ay), ex = qm_sub(gx[(e + 1) & 3], ax);
    int m = 0;
    if (n > 0) {
      const double fy = QM_AT(src, 0, 0), fx = QM_AT(src, 0, 1);
      const double fd = qm_sub(qm_mul(ex, qm_sub(fy, ay)), qm_mul(ey, qm_sub(fx, ax)));
      double vy = fy, vx = fx, dv = fd;
      for (int k = 0; k < n; ++k) {
        double wy = fy, wx = fx, dw = fd;
        if (k + 1 < n) {
          wy = QM_AT(src, k + 1, 0);
          wx = QM_AT(src, k + 1, 1);
          dw = qm_sub(qm_mul(ex, qm_sub(wy, ay)), qm_mul(ey, qm_sub(wx, ax)));
        }
        if (dv >= 0.0 && m < QM_RING) {
          QM_AT(dst, m, 0) = vy;
          QM_AT(dst, m, 1) = vx;
          ++m;
        }
        if ((dv >= 0.0) != (dw >= 0.0) && m < QM_RING) {
          const double t = qm_div(dv, qm_sub(dv, dw));
          QM_AT(dst, m, 0) = qm_add(vy, qm_mul(t, qm_sub(wy, vy)));
          QM_AT(dst, m, 1) = qm_add(vx, qm_mul(t, qm_sub(wx, vx)));
          ++m;
        }
        vy = wy;
        vx = wx;
        dv = dw;
      }
    }
    n = m;
  }
  double acc = 0.0;  // four clips: the result is in ring 0
  if (n > 0) {
    const double fy = QM_AT(0, 0, 0), fx = QM_AT(0, 0, 1);
    double y0 = fy, x0 = fx;
    for (int k = 0; k < n; ++k) {
      double y1 = fy, x1 = fx;
      if (k + 1 < n) {
        y1 = QM_AT(0, k + 1, 0);
        x1 = QM_AT(0, k + 1, 1);
      }
      acc = qm_add(acc, qm_sub(qm_mul(x0, y1), qm_mul(x1, y0)));
      y0 = y1;
      x0 = x1;
    }
  }
#undef QM_AT
  const double ag = (double)(long)(((unsigned long long)(unsigned)ga.y << 32) | (unsigned)ga.x);
  const double ap = (double)(long)(((unsigned long long)(unsigned)pa.y << 32) | (unsigned)pa.x);
  const double hi = ap < ag ? ap : ag;
  double inter2 = acc;
  if (inter2 > hi) inter2 = hi;
  if (inter2 < 0.0) inter2 = 0.0;
  *inter2_out = inter2;
  const double den = qm_sub(qm_add(ag, ap), inter2);
  return den > 0.0 ? qm_div(inter2, den) : 0.0;
}

// the int64 twice-area of an LDS row's part 3
__device__ __forceinline__ long qm_area2(const int4 a) { return (long)(((unsigned long long)(unsigned)a.y << 32) | (unsigned)a.x); }

}  // namespace
