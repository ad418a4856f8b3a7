// The pooled branches of the pyramid-pooling block (upernext.py:48-84) as kernels of their own: for every scale s_k
//   cat[..., C + k Cb : C + (k+1) Cb] = bilinear(gelu(LN(pool_{s_k}(x) W_k^T + b_k)) -> H x W),   cat[..., :C] = x.
// The branches are arithmetically trivial (sum s^2 pooled pixels per image) and used to run as ~45 one-workgroup launches per
// pass; here they are three forward and four backward launches over ALL branches.
//
// Pooled rows are stored branch-major: branch k owns rows [B cell0_k, B cell0_{k+1}), row = B cell0_k + (b s^2 + bi s + bj),
// cell0_k = sum_{j<k} s_j^2, so the rows of one Linear / LayerNorm are contiguous.  col0_k = sum_{j<k} s_j numbers the bins
// along one axis over all branches (the separable halves of pooling and of the resize adjoint are indexed by it).
//
// Rounding points (16-bit storage type T, fp32 accumulation everywhere): the pooled map P, the Linear output Z and the
// LN + GELU output A are each rounded once to T, W_k is rounded to T on load from the fp32 parameter - exactly the values the
// unfused chain (vkas_adaptive_avgpool_fwd, the 1x1 GEMM on the packed weight image, vkas_layernorm_fwd, vkas_resize_fwd)
// works with, so the two differ by summation order only.  Backward rounds dZ to T (what the unfused LayerNorm backward hands
// to the GEMMs) and dx once; U^T dcat and dP stay in fp32.  Every sum has a fixed order and there are no atomics: two runs
// give the same bits.
#include "vkas_common.h"
#include "resize_index.h"

namespace {

constexpr int RG = 4;  // pooled rows per workgroup of the row kernels: one wave each for the LayerNorm statistics

struct PpmPlan {
  int nb, S, SS;  // branches, pooled cells per image (sum s^2), bins per axis over all branches (sum s)
  int s[VKAS_PPM_MAX_BRANCHES], cell0[VKAS_PPM_MAX_BRANCHES], col0[VKAS_PPM_MAX_BRANCHES];
  int grp0[VKAS_PPM_MAX_BRANCHES + 1];  // first row group (RG rows of ONE branch) of every branch
};
struct PpmParams {
  const float* w[VKAS_PPM_MAX_BRANCHES];
  const float* bias[VKAS_PPM_MAX_BRANCHES];
  const float* gamma[VKAS_PPM_MAX_BRANCHES];
  const float* beta[VKAS_PPM_MAX_BRANCHES];
};
struct PpmGrads {
  float* dst[4 * VKAS_PPM_MAX_BRANCHES];  // per branch: dW (Cb, C), db, dgamma, dbeta (Cb)
  int accumulate[4 * VKAS_PPM_MAX_BRANCHES];
};

// the value the packed 16-bit weight image holds for an fp32 parameter
template <typename T> __device__ __forceinline__ float round_t(float v) { return to_f32(from_f32<T>(v)); }

__device__ __forceinline__ int branch_of_col(const PpmPlan& p, int col) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < VKAS_PPM_MAX_BRANCHES; ++j) k += (j < p.nb && col >= p.col0[j]) ? 1 : 0;
  return k;
}
__device__ __forceinline__ int branch_of_group(const PpmPlan& p, int g) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < VKAS_PPM_MAX_BRANCHES; ++j) k += (j < p.nb && g >= p.grp0[j]) ? 1 : 0;
  return k;
}

// ---- forward 1: one pass over x ---------------------------------------------------------------------------------------------
// grid.x = B*H image rows, grid.y = chunks of 256 (item, 8-channel vector) pairs; items 0 .. W-1 copy pixel `item` of the row
// into cat[..., :C], items W .. W+SS-1 sum the row's pixels of one x bin (branch k, bin bj) into rowsum (B, H, SS, C) fp32.
// The bins of one scale may overlap and H, W < s is legal (a pixel then lies in several bins), hence bin-major sums; after the
// first touch the row comes from L1 / L2, so HBM sees x once.
template <typename T>
__global__ __launch_bounds__(256) void ppm_pool_fwd_kernel(const T* __restrict__ x, long ldx, T* __restrict__ cat, long ldcat,
                                                           float* __restrict__ rowsum, PpmPlan p, int H, int W, int C) {
  const int nvec = C >> 3;
  const int idx = blockIdx.y * 256 + threadIdx.x;
  const int item = idx / nvec;
  const int v = idx - item * nvec;
  if (item >= W + p.SS) return;
  const long prow = (long)blockIdx.x * W;  // first pixel of image row (b, y)
  const T* xr = x + prow * ldx + v * 8;
  if (item < W) {
    *reinterpret_cast<uint4*>(cat + (prow + item) * ldcat + v * 8) = *reinterpret_cast<const uint4*>(xr + (long)item * ldx);
    return;
  }
  const int col = item - W;
  const int k = branch_of_col(p, col);
  int x0, x1;
  pool_bin(col - p.col0[k], W, p.s[k], x0, x1);
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int xx = x0; xx < x1; xx += 4) {
    Raw8<T> raw[4];  // four requests in flight; a pixel beyond the bin re-reads the bin's last one and is not added
#pragma unroll
    for (int j = 0; j < 4; ++j) raw[j].load(xr + (long)(xx + j < x1 ? xx + j : x1 - 1) * ldx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t[8];
      raw[j].unpack(t);
      if (xx + j < x1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += t[i];
      }
    }
  }
  store8(rowsum + ((long)blockIdx.x * p.SS + col) * C + v * 8, acc);
}

// ---- forward 2: pooled rows -> Linear + bias -> LayerNorm -> GELU -----------------------------------------------------------
// One workgroup per group of RG rows of one branch (4 waves).  (a) the rows' y sums of rowsum, times 1 / bin pixels, rounded
// to T -> LDS (and `pooled` when kept); (b) Z = P W^T + b: a wave owns every 4th output column, its lanes split K and the
// partial sums meet in a wave reduction; (c) wave r normalises row r.  LDS: RG * (C + Cb) floats.
template <typename T>
__global__ __launch_bounds__(256) void ppm_rows_fwd_kernel(const float* __restrict__ rowsum, PpmParams prm, T* __restrict__ pooled,
                                                           T* __restrict__ lin, float* __restrict__ stats, T* __restrict__ act,
                                                           PpmPlan p, int B, int H, int W, int C, int Cb) {
  extern __shared__ float4 ppm_lds4[];
  float* Ps = reinterpret_cast<float*>(ppm_lds4);  // [RG][C]
  float* Zs = Ps + RG * C;                         // [RG][Cb]
  const int k = branch_of_group(p, blockIdx.x);
  const int s = p.s[k], ss = s * s;
  const int nk = B * ss;                              // rows of this branch
  const int q0 = ((int)blockIdx.x - p.grp0[k]) * RG;  // first of this group's rows inside the branch
  const long row0 = (long)B * p.cell0[k] + q0;
  const int nvec = C >> 3;
  for (int pair = threadIdx.x; pair < RG * nvec; pair += 256) {
    const int r = pair / nvec, v = pair - r * nvec;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q0 + r < nk) {
      const int q = q0 + r;
      const int b = q / ss, cell = q - b * ss;
      const int bi = cell / s, bj = cell - bi * s;
      int y0, y1, x0, x1;
      pool_bin(bi, H, s, y0, y1);
      pool_bin(bj, W, s, x0, x1);
      const float* src = rowsum + ((long)b * H * p.SS + p.col0[k] + bj) * C + v * 8;
      for (int yy = y0; yy < y1; yy += 8) {
        Raw8<float> raw[8];  // eight requests in flight: at s = 1 a row's sum is a chain of H / 8 round trips
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[j].load(src + (long)(yy + j < y1 ? yy + j : y1 - 1) * p.SS * C);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t[8];
          raw[j].unpack(t);
          if (yy + j < y1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += t[i];
          }
        }
      }
      const float inv = 1.f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] *= inv;
      if (pooled) store8(pooled + (row0 + r) * C + v * 8, acc);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) Ps[r * C + v * 8 + i] = round_t<T>(acc[i]);
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* wk = prm.w[k];
  const int nc4 = C >> 2;
  // four output columns n = n0 + 4 u per trip: their weight rows are requested together (one column per trip left the wave
  // waiting for a single L2 round trip per column); a column beyond Cb re-reads column n0 and is dropped
  for (int n0 = wave; n0 < Cb; n0 += 16) {
    float part[4][RG];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < RG; ++r) part[u][r] = 0.f;
    for (int c4 = lane; c4 < nc4; c4 += 64) {
      float4 wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        wv[u] = *reinterpret_cast<const float4*>(wk + (long)(n0 + 4 * u < Cb ? n0 + 4 * u : n0) * C + c4 * 4);
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const float4 pv = *reinterpret_cast<const float4*>(Ps + r * C + c4 * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          part[u][r] = fmaf(pv.x, round_t<T>(wv[u].x), part[u][r]);
          part[u][r] = fmaf(pv.y, round_t<T>(wv[u].y), part[u][r]);
          part[u][r] = fmaf(pv.z, round_t<T>(wv[u].z), part[u][r]);
          part[u][r] = fmaf(pv.w, round_t<T>(wv[u].w), part[u][r]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + 4 * u;
      if (n >= Cb) break;  // wave-uniform
      const float bn = prm.bias[k][n];
#pragma unroll
      for (int r = 0; r < RG; ++r) {
        const float z = wave_sum(part[u][r]) + bn;
        if (lane == 0) Zs[r * Cb + n] = round_t<T>(z);
      }
    }
  }
  __syncthreads();
  // wave `wave` owns row `wave`: statistics as layernorm_fwd_kernel forms them (mean, then centred squares)
  const int r = wave;
  if (q0 + r >= nk) return;  // whole waves leave; no barrier follows
  const long row = row0 + r;
  float sum = 0.f;
  for (int n = lane; n < Cb; n += 64) sum += Zs[r * Cb + n];
  const float mean = ln_mean(wave_sum(sum), Cb);
  float sq = 0.f;
  for (int n = lane; n < Cb; n += 64) {
    const float d = Zs[r * Cb + n] - mean;
    sq += d * d;
  }
  const float rstd = ln_rstd(wave_sum(sq), Cb);
  if (stats && lane == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
  for (int n = lane; n < Cb; n += 64) {
    const float z = Zs[r * Cb + n];
    if (lin) lin[row * Cb + n] = from_f32<T>(z);
    act[row * Cb + n] = from_f32<T>(gelu_t<T>(ln_affine(z, mean, rstd, prm.gamma[k][n], prm.beta[k][n])));
  }
}

// ---- forward 3: bilinear resize of every branch into its channel slice of cat -------------------------------------------------
// grid.x = B*H destination rows, grid.y = chunks of 256 (ox, branch, vector) triples - consecutive lanes walk the nb * Cb
// branch channels of one pixel.  Index function, weights and lerp of resize_fwd_kernel.
template <typename T>
__global__ __launch_bounds__(256) void ppm_resize_fwd_kernel(const T* __restrict__ act, T* __restrict__ cat, long ldcat,
                                                             PpmPlan p, int B, int H, int W, int C, int Cb) {
  const int nvb = Cb >> 3, per_px = p.nb * nvb;
  const int idx = blockIdx.y * 256 + threadIdx.x;
  const int ox = idx / per_px;
  if (ox >= W) return;
  const int cv = idx - ox * per_px;
  const int k = cv / nvb, v = cv - k * nvb;
  const int b = blockIdx.x / H, oy = blockIdx.x - b * H;
  const int s = p.s[k];
  const float sy = (float)s / (float)H, sx = (float)s / (float)W;
  int y0, y1, x0, x1;
  float wy, wx;
  bilinear_src(oy, sy, s, y0, y1, wy);
  bilinear_src(ox, sx, s, x0, x1, wx);
  const T* ab = act + ((long)B * p.cell0[k] + (long)b * s * s) * Cb + v * 8;
  float a[8], bq[8], c[8], d[8], o[8];
  load8(ab + (long)(y0 * s + x0) * Cb, a);
  load8(ab + (long)(y0 * s + x1) * Cb, bq);
  load8(ab + (long)(y1 * s + x0) * Cb, c);
  load8(ab + (long)(y1 * s + x1) * Cb, d);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = lerp2(lerp2(a[i], bq[i], wx), lerp2(c[i], d[i], wx), wy);
  store8(cat + ((long)blockIdx.x * W + ox) * ldcat + C + k * Cb + v * 8, o);
}

// ---- backward 1: x half of U^T on the branch slices of dcat, read in place --------------------------------------------------
// tx (B, H, SS, Cb) fp32: tx[b, oy, col0_k + ix] = sum_ox w_x(ox -> ix) dcat_k[b, oy, ox].  grid.x = B*H destination rows,
// grid.y = chunks of 256 (bin column, vector) pairs.  The y half is the prologue of the row kernel: the footprint of a large
// cell (all 32 x 32 pixels at s = 1) is thereby split over H workgroups and summed in ascending ox, then ascending oy.
template <typename T>
__global__ __launch_bounds__(256) void ppm_resize_bwd_x_kernel(const T* __restrict__ dcat, long lddcat, float* __restrict__ tx,
                                                               PpmPlan p, int W, int C, int Cb) {
  const int nvb = Cb >> 3;
  const int idx = blockIdx.y * 256 + threadIdx.x;
  const int col = idx / nvb;
  if (col >= p.SS) return;
  const int v = idx - col * nvb;
  const int k = branch_of_col(p, col);
  const int s = p.s[k], ix = col - p.col0[k];
  const float sx = (float)s / (float)W;
  int lo, hi;
  dst_range(ix, s, W, sx, 0, lo, hi);
  const T* src = dcat + (long)blockIdx.x * W * lddcat + C + k * Cb + v * 8;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int ox = lo; ox <= hi; ox += 4) {
    Raw8<T> raw[4];
    float w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int oc = ox + j <= hi ? ox + j : hi;
      raw[j].load(src + (long)oc * lddcat);
      w[j] = ox + j <= hi ? axis_weight(oc, sx, s, W, ix, 0) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t[8];
      raw[j].unpack(t);
      if (w[j] != 0.f) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(w[j], t[i], acc[i]);
      }
    }
  }
  store8(tx + ((long)blockIdx.x * p.SS + col) * Cb + v * 8, acc);
}

// ---- backward 2: y half of U^T, LN + GELU backward, dP = dZ W ---------------------------------------------------------------
// Row groups as in the forward.  Wave r: dA = sum_oy w_y tx, then layernorm_bwd_kernel's formulas on row r; dZ is rounded to T
// (global `dz` for the weight gradient, LDS for dP).  The group's sums of dA gelu' h | dA gelu' leave as one partial row
// (2 Cb floats) per group.  dP (rows, C) fp32 only when the input gradient is wanted.  LDS: 3 * RG * Cb floats.
template <typename T>
__global__ __launch_bounds__(256) void ppm_rows_bwd_kernel(const float* __restrict__ tx, PpmParams prm, const T* __restrict__ lin,
                                                           const float* __restrict__ stats, T* __restrict__ dz,
                                                           float* __restrict__ partial, float* __restrict__ dp, PpmPlan p, int B,
                                                           int H, int C, int Cb) {
  extern __shared__ float4 ppm_lds4[];
  float* dZs = reinterpret_cast<float*>(ppm_lds4);  // [RG][Cb]
  float* dGs = dZs + RG * Cb;                       // [RG][Cb]  dA gelu' h
  float* dBs = dGs + RG * Cb;                       // [RG][Cb]  dA gelu'
  const int k = branch_of_group(p, blockIdx.x);
  const int s = p.s[k], ss = s * s;
  const int nk = B * ss;
  const int q0 = ((int)blockIdx.x - p.grp0[k]) * RG;
  const long row0 = (long)B * p.cell0[k] + q0;
  const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* gm = prm.gamma[k];
  const float* bt = prm.beta[k];
  if (q0 + r < nk) {
    const int q = q0 + r;
    const long row = row0 + r;
    const int b = q / ss, cell = q - b * ss;
    const int iy = cell / s, ix = cell - iy * s;
    const float sy = (float)s / (float)H;
    int lo, hi;
    dst_range(iy, s, H, sy, 0, lo, hi);
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int n = lane; n < Cb; n += 64) {
      float da = 0.f;
      const float* src = tx + ((long)b * H * p.SS + p.col0[k] + ix) * Cb + n;
      for (int oy = lo; oy <= hi; oy += 4) {  // four requests in flight; zero weights are skipped as resize_bwd_kernel skips them
        float t[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int oc = oy + j <= hi ? oy + j : hi;
          t[j] = src[(long)oc * p.SS * Cb];
          w[j] = oy + j <= hi ? axis_weight(oc, sy, s, H, iy, 0) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) da = w[j] != 0.f ? fmaf(w[j], t[j], da) : da;
      }
      const float h = (to_f32(lin[row * Cb + n]) - mean) * rstd;
      const float gg = da * dgelu_t<T>(h * gm[n] + bt[n]);
      const float dxh = gg * gm[n];
      dGs[r * Cb + n] = gg * h;
      dBs[r * Cb + n] = gg;
      dZs[r * Cb + n] = dxh;  // rstd * (dxh - s1 - h s2) once the row sums are known
      s1 += dxh;
      s2 += dxh * h;
    }
    s1 = wave_sum(s1) / (float)Cb;
    s2 = wave_sum(s2) / (float)Cb;
    for (int n = lane; n < Cb; n += 64) {
      const float h = (to_f32(lin[row * Cb + n]) - mean) * rstd;
      const T o = from_f32<T>(rstd * (dZs[r * Cb + n] - s1 - h * s2));
      dz[row * Cb + n] = o;
      dZs[r * Cb + n] = to_f32(o);
    }
  } else {
    for (int n = lane; n < Cb; n += 64) {
      dGs[r * Cb + n] = 0.f;
      dBs[r * Cb + n] = 0.f;
      dZs[r * Cb + n] = 0.f;
    }
  }
  __syncthreads();
  float* prow = partial + (long)blockIdx.x * 2 * Cb;
  for (int n = threadIdx.x; n < Cb; n += 256) {
    float g = 0.f, bsum = 0.f;
#pragma unroll
    for (int rr = 0; rr < RG; ++rr) {
      g += dGs[rr * Cb + n];
      bsum += dBs[rr * Cb + n];
    }
    prow[n] = g;
    prow[Cb + n] = bsum;
  }
  if (!dp) return;
  const float* wk = prm.w[k];
  for (int c4 = threadIdx.x; c4 < (C >> 2); c4 += 256) {
    float acc[RG][4];
#pragma unroll
    for (int rr = 0; rr < RG; ++rr)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[rr][i] = 0.f;
#pragma unroll 8
    for (int n = 0; n < Cb; ++n) {  // Cb is a multiple of 8: eight weight rows requested per trip
      const float4 wv = *reinterpret_cast<const float4*>(wk + (long)n * C + c4 * 4);
      const float w[4] = {round_t<T>(wv.x), round_t<T>(wv.y), round_t<T>(wv.z), round_t<T>(wv.w)};
#pragma unroll
      for (int rr = 0; rr < RG; ++rr) {
        const float d = dZs[rr * Cb + n];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[rr][i] = fmaf(d, w[i], acc[rr][i]);
      }
    }
#pragma unroll
    for (int rr = 0; rr < RG; ++rr)
      if (q0 + rr < nk) store4(dp + (row0 + rr) * C + c4 * 4, acc[rr]);
  }
}

// ---- backward 3: dW_k = dZ_k^T P_k, db_k, and the final dgamma_k, dbeta_k ----------------------------------------------------
// One workgroup per (branch, 8 output channels n, 64 input channels c): 16 lanes x 4 channels, 16 row slices (rows r = slice,
// slice + 16, ...) whose 8 x 4 sums meet in LDS in slice order.  The c == 0 workgroups also sum dZ's columns (db) and the row
// groups' partial rows (dgamma, dbeta).  Every output has one writer: out = sum (+ out when it accumulates onto a gradient).
template <typename T>
__global__ __launch_bounds__(256) void ppm_param_grads_kernel(const T* __restrict__ dz, const T* __restrict__ pooled,
                                                              const float* __restrict__ partial, PpmGrads g, PpmPlan p, int B,
                                                              int C, int Cb) {
  __shared__ float red[16 * 16 * 32];
  const int ncc = (C + 63) >> 6, nnt = Cb >> 3;
  const int cchunk = blockIdx.x % ncc;
  const int nt = (blockIdx.x / ncc) % nnt;
  const int k = blockIdx.x / (ncc * nnt);
  const int nk = B * p.s[k] * p.s[k];
  const long row0 = (long)B * p.cell0[k];
  const int cl = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int c4 = cchunk * 16 + cl;
  const bool cok = c4 * 4 < C;
  float acc[8][4], accb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    accb[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
  }
#pragma unroll 4
  for (int r = slice; r < nk; r += 16) {
    float d[8], pv[4];
    load8(dz + (row0 + r) * Cb + nt * 8, d);
    load4(pooled + (row0 + r) * C + (cok ? c4 : 0) * 4, pv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      accb[j] += d[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = fmaf(d[j], pv[i], acc[j][i]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(slice * 16 + cl) * 32 + j * 4 + i] = acc[j][i];
  __syncthreads();
  float* dw = g.dst[4 * k];
  const int aw = g.accumulate[4 * k];
  for (int o = threadIdx.x; o < 16 * 32; o += 256) {
    const int ocl = o >> 5, e = o & 31;
    const int c = (cchunk * 16 + ocl) * 4 + (e & 3);
    if (c >= C) continue;
    float sum = 0.f;
    for (int sl = 0; sl < 16; ++sl) sum += red[(sl * 16 + ocl) * 32 + e];
    float* dst = dw + (long)(nt * 8 + (e >> 2)) * C + c;
    *dst = aw ? *dst + sum : sum;
  }
  if (cchunk != 0) return;  // uniform over the workgroup
  __syncthreads();
  if (cl == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[slice * 8 + j] = accb[j];
  }
  __syncthreads();
  // dgamma | dbeta: lane cl = (which, j) takes the partial rows grp0 + slice, + 16, ...; the 16 slice sums meet in slice order
  {
    const int which = cl >> 3, j = cl & 7;  // 0 dgamma, 1 dbeta
    float sum = 0.f;
    for (int grp = p.grp0[k] + slice; grp < p.grp0[k + 1]; grp += 16) sum += partial[(long)grp * 2 * Cb + which * Cb + nt * 8 + j];
    red[128 + slice * 16 + cl] = sum;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    float sum = 0.f;
    for (int sl = 0; sl < 16; ++sl) sum += red[sl * 8 + threadIdx.x];
    float* dst = g.dst[4 * k + 1] + nt * 8 + threadIdx.x;
    *dst = g.accumulate[4 * k + 1] ? *dst + sum : sum;
  } else if (threadIdx.x < 24) {
    const int o = threadIdx.x - 8, which = o >> 3, j = o & 7;
    float sum = 0.f;
    for (int sl = 0; sl < 16; ++sl) sum += red[128 + sl * 16 + o];
    float* dst = g.dst[4 * k + 2 + which] + nt * 8 + j;
    *dst = g.accumulate[4 * k + 2 + which] ? *dst + sum : sum;
  }
}

// ---- backward 4: dx = dcat[..., :C] + sum_k pool_k^T(dP_k), one rounding ----------------------------------------------------
// grid.x = B*H rows, grid.y = chunks of 256 (pixel, vector) pairs.  Every bin of every branch that holds the pixel adds
// dP / bin pixels (avgpool_bwd_kernel's enumeration), branches ascending.
template <typename T>
__global__ __launch_bounds__(256) void ppm_pool_bwd_kernel(const T* __restrict__ dcat, long lddcat, const float* __restrict__ dp,
                                                           T* __restrict__ dx, long lddx, PpmPlan p, int B, int H, int W, int C) {
  const int nvec = C >> 3;
  const int idx = blockIdx.y * 256 + threadIdx.x;
  const int xx = idx / nvec;
  if (xx >= W) return;
  const int v = idx - xx * nvec;
  const int b = blockIdx.x / H, yy = blockIdx.x - b * H;
  const long pix = (long)blockIdx.x * W + xx;
  float acc[8];
  load8(dcat + pix * lddcat + v * 8, acc);
  for (int k = 0; k < p.nb; ++k) {
    const int s = p.s[k];
    const float* dpk = dp + ((long)B * p.cell0[k] + (long)b * s * s) * C + v * 8;
    for (int bi = 0; bi < s; ++bi) {
      int y0, y1;
      pool_bin(bi, H, s, y0, y1);
      if (yy < y0 || yy >= y1) continue;
      for (int bj = 0; bj < s; ++bj) {
        int x0, x1;
        pool_bin(bj, W, s, x0, x1);
        if (xx < x0 || xx >= x1) continue;
        float t[8];
        load8(dpk + (long)(bi * s + bj) * C, t);
        const float inv = 1.f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(inv, t[i], acc[i]);
      }
    }
  }
  store8(dx + pix * lddx + v * 8, acc);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int ppm_plan(const char* who, int nb, const int* scales, int B, int H, int W, int C, int Cb, PpmPlan& p) {
  VKAS_CHECK(scales && nb >= 1 && nb <= VKAS_PPM_MAX_BRANCHES, "%s: 1 .. %d branches, got %d", who, VKAS_PPM_MAX_BRANCHES, nb);
  VKAS_CHECK(B >= 0 && H > 0 && W > 0, "%s: bad spatial dims", who);
  VKAS_CHECK(C > 0 && C % 8 == 0 && C <= VKAS_PPM_MAX_C && Cb > 0 && Cb % 8 == 0 && Cb <= VKAS_PPM_MAX_CB,
             "%s: C=%d (multiple of 8, at most %d), Cb=%d (multiple of 8, at most %d)", who, C, VKAS_PPM_MAX_C, Cb, VKAS_PPM_MAX_CB);
  p.nb = nb;
  p.S = p.SS = 0;
  p.grp0[0] = 0;
  for (int k = 0; k < VKAS_PPM_MAX_BRANCHES; ++k) {
    const int s = k < nb ? scales[k] : 1;
    VKAS_CHECK(s >= 1 && s <= VKAS_PPM_MAX_SCALE, "%s: scale %d outside 1 .. %d", who, s, VKAS_PPM_MAX_SCALE);
    p.s[k] = s;
    p.cell0[k] = p.S;
    p.col0[k] = p.SS;
    if (k < nb) {
      p.S += s * s;
      p.SS += s;
    }
    const long groups = k < nb ? vkas_cdiv((long)B * s * s, RG) : 0;
    VKAS_CHECK(p.grp0[k] + groups < (1L << 30), "%s: too many pooled rows", who);
    p.grp0[k + 1] = p.grp0[k] + (int)groups;
  }
  VKAS_CHECK(p.S <= VKAS_PPM_MAX_CELLS, "%s: %d pooled cells per image, at most %d", who, p.S, VKAS_PPM_MAX_CELLS);
  VKAS_CHECK((long)B * H < (1L << 31) && (long)B * p.S * (long)(C > Cb ? C : Cb) < (1L << 31), "%s: batch too large", who);
  return VKAS_OK;
}

int ppm_act(const char* who, const void* a, long lda, int width) {
  VKAS_CHECK(a && vkas_aligned16(a) && lda >= width && lda % 8 == 0, "%s: null / misaligned activation or bad pixel stride", who);
  return VKAS_OK;
}

int ppm_params(const char* who, const float* const* params, int nb, PpmParams& prm) {
  VKAS_CHECK(params, "%s: null parameter table", who);
  for (int k = 0; k < VKAS_PPM_MAX_BRANCHES; ++k) {
    const int j = k < nb ? k : 0;
    prm.w[k] = params[4 * j];
    prm.bias[k] = params[4 * j + 1];
    prm.gamma[k] = params[4 * j + 2];
    prm.beta[k] = params[4 * j + 3];
    VKAS_CHECK(prm.w[k] && prm.bias[k] && prm.gamma[k] && prm.beta[k] && vkas_aligned16(prm.w[k]), "%s: null / misaligned parameter", who);
  }
  return VKAS_OK;
}

inline unsigned chunks(long items) { return (unsigned)vkas_cdiv(items, 256); }

}  // namespace

#define PPM_DISPATCH16(dtype, NAME, ...)                                              \
  if ((dtype) == VKAS_BF16) {                                                         \
    using T = bf16_t;                                                                 \
    __VA_ARGS__                                                                       \
  } else if ((dtype) == VKAS_F16) {                                                   \
    using T = f16_t;                                                                  \
    __VA_ARGS__                                                                       \
  } else {                                                                            \
    vkas_set_error("%s: 16-bit storage only (dtype %d)", NAME, (int)(dtype));         \
    return VKAS_E_ARG;                                                                \
  }

extern "C" long vkas_ppm_row_groups(int B, int nb, const int* scales) {
  PpmPlan p;
  if (ppm_plan("vkas_ppm_row_groups", nb, scales, B, 1, 1, 8, 8, p)) return -1;
  return p.grp0[nb];
}

extern "C" int vkas_ppm_pool_fwd(const void* x, long ldx, void* cat, long ldcat, float* rowsum, int B, int H, int W, int C,
                                 int Cb, int nb, const int* scales, int dtype, void* stream) {
  const char* who = "vkas_ppm_pool_fwd";
  PpmPlan p;
  int rc = ppm_plan(who, nb, scales, B, H, W, C, Cb, p);
  if (rc) return rc;
  if ((rc = ppm_act(who, x, ldx, C)) || (rc = ppm_act(who, cat, ldcat, C + nb * Cb))) return rc;
  VKAS_CHECK(rowsum && vkas_aligned16(rowsum), "%s: null / misaligned workspace", who);
  if (B == 0) return VKAS_OK;
  const long items = (long)(W + p.SS) * (C / 8);
  VKAS_CHECK(vkas_cdiv(items, 256) <= 65535, "%s: row too wide", who);
  dim3 grid((unsigned)((long)B * H), chunks(items));
  PPM_DISPATCH16(dtype, who, {
    ppm_pool_fwd_kernel<T><<<grid, 256, 0, vkas_stream(stream)>>>((const T*)x, ldx, (T*)cat, ldcat, rowsum, p, H, W, C);
  })
  VKAS_LAUNCH_CHECK("ppm_pool_fwd");
  return VKAS_OK;
}

extern "C" int vkas_ppm_rows_fwd(const float* rowsum, const float* const* params, void* pooled, void* lin, float* stats,
                                 void* act, int B, int H, int W, int C, int Cb, int nb, const int* scales, int dtype,
                                 void* stream) {
  const char* who = "vkas_ppm_rows_fwd";
  PpmPlan p;
  PpmParams prm;
  int rc = ppm_plan(who, nb, scales, B, H, W, C, Cb, p);
  if (rc || (rc = ppm_params(who, params, nb, prm))) return rc;
  VKAS_CHECK(rowsum && act && vkas_aligned16(rowsum) && vkas_aligned16(act) && (!pooled || vkas_aligned16(pooled)),
             "%s: null / misaligned buffer", who);
  VKAS_CHECK((pooled != nullptr) == (lin != nullptr) && (lin != nullptr) == (stats != nullptr),
             "%s: pooled, lin and stats are kept together or not at all", who);
  if (B == 0) return VKAS_OK;
  const size_t lds = (size_t)RG * (C + Cb) * sizeof(float);
  PPM_DISPATCH16(dtype, who, {
    ppm_rows_fwd_kernel<T><<<(unsigned)p.grp0[nb], 256, lds, vkas_stream(stream)>>>(rowsum, prm, (T*)pooled, (T*)lin, stats, (T*)act,
                                                                                   p, B, H, W, C, Cb);
  })
  VKAS_LAUNCH_CHECK("ppm_rows_fwd");
  return VKAS_OK;
}

extern "C" int vkas_ppm_resize_fwd(const void* act, void* cat, long ldcat, int B, int H, int W, int C, int Cb, int nb,
                                   const int* scales, int dtype, void* stream) {
  const char* who = "vkas_ppm_resize_fwd";
  PpmPlan p;
  int rc = ppm_plan(who, nb, scales, B, H, W, C, Cb, p);
  if (rc || (rc = ppm_act(who, cat, ldcat, C + nb * Cb))) return rc;
  VKAS_CHECK(act && vkas_aligned16(act), "%s: null / misaligned buffer", who);
  if (B == 0) return VKAS_OK;
  const long items = (long)W * nb * (Cb / 8);
  VKAS_CHECK(vkas_cdiv(items, 256) <= 65535, "%s: row too wide", who);
  dim3 grid((unsigned)((long)B * H), chunks(items));
  PPM_DISPATCH16(dtype, who, {
    ppm_resize_fwd_kernel<T><<<grid, 256, 0, vkas_stream(stream)>>>((const T*)act, (T*)cat, ldcat, p, B, H, W, C, Cb);
  })
  VKAS_LAUNCH_CHECK("ppm_resize_fwd");
  return VKAS_OK;
}

extern "C" int vkas_ppm_resize_bwd_x(const void* dcat, long lddcat, float* tx, int B, int H, int W, int C, int Cb, int nb,
                                     const int* scales, int dtype, void* stream) {
  const char* who = "vkas_ppm_resize_bwd_x";
  PpmPlan p;
  int rc = ppm_plan(who, nb, scales, B, H, W, C, Cb, p);
  if (rc || (rc = ppm_act(who, dcat, lddcat, C + nb * Cb))) return rc;
  VKAS_CHECK(tx && vkas_aligned16(tx), "%s: null / misaligned workspace", who);
  if (B == 0) return VKAS_OK;
  dim3 grid((unsigned)((long)B * H), chunks((long)p.SS * (Cb / 8)));
  PPM_DISPATCH16(dtype, who, {
    ppm_resize_bwd_x_kernel<T><<<grid, 256, 0, vkas_stream(stream)>>>((const T*)dcat, lddcat, tx, p, W, C, Cb);
  })
  VKAS_LAUNCH_CHECK("ppm_resize_bwd_x");
  return VKAS_OK;
}

extern "C" int vkas_ppm_rows_bwd(const float* tx, const float* const* params, const void* lin, const float* stats, void* dz,
                                 float* partial, float* dp, int B, int H, int W, int C, int Cb, int nb, const int* scales,
                                 int dtype, void* stream) {
  const char* who = "vkas_ppm_rows_bwd";
  PpmPlan p;
  PpmParams prm;
  int rc = ppm_plan(who, nb, scales, B, H, W, C, Cb, p);
  if (rc || (rc = ppm_params(who, params, nb, prm))) return rc;
  VKAS_CHECK(tx && lin && stats && dz && partial && vkas_aligned16(dz) && (!dp || vkas_aligned16(dp)), "%s: null / misaligned buffer", who);
  if (B == 0) return VKAS_OK;
  const size_t lds = (size_t)3 * RG * Cb * sizeof(float);
  PPM_DISPATCH16(dtype, who, {
    ppm_rows_bwd_kernel<T><<<(unsigned)p.grp0[nb], 256, lds, vkas_stream(stream)>>>(tx, prm, (const T*)lin, stats, (T*)dz, partial, dp,
                                                                                   p, B, H, C, Cb);
  })
  VKAS_LAUNCH_CHECK("ppm_rows_bwd");
  return VKAS_OK;
}

extern "C" int vkas_ppm_param_grads(const void* dz, const void* pooled, const float* partial, float* const* grads,
                                    const int* accumulate, int B, int C, int Cb, int nb, const int* scales, int dtype,
                                    void* stream) {
  const char* who = "vkas_ppm_param_grads";
  PpmPlan p;
  int rc = ppm_plan(who, nb, scales, B, 1, 1, C, Cb, p);
  if (rc) return rc;
  VKAS_CHECK(dz && pooled && partial && grads && accumulate && vkas_aligned16(dz) && vkas_aligned16(pooled),
             "%s: null / misaligned buffer", who);
  PpmGrads g;
  for (int i = 0; i < 4 * VKAS_PPM_MAX_BRANCHES; ++i) {
    g.dst[i] = i < 4 * nb ? grads[i] : nullptr;
    g.accumulate[i] = i < 4 * nb ? accumulate[i] : 0;
    VKAS_CHECK(i >= 4 * nb || g.dst[i], "%s: null gradient destination", who);
  }
  // B == 0: the sums are empty and the kernel writes zeros (or leaves an accumulated gradient as it is)
  const long grid = (long)nb * (Cb / 8) * vkas_cdiv(C, 64);
  PPM_DISPATCH16(dtype, who, {
    ppm_param_grads_kernel<T><<<(unsigned)grid, 256, 0, vkas_stream(stream)>>>((const T*)dz, (const T*)pooled, partial, g, p, B, C, Cb);
  })
  VKAS_LAUNCH_CHECK("ppm_param_grads");
  return VKAS_OK;
}

extern "C" int vkas_ppm_pool_bwd(const void* dcat, long lddcat, const float* dp, void* dx, long lddx, int B, int H, int W,
                                 int C, int Cb, int nb, const int* scales, int dtype, void* stream) {
  const char* who = "vkas_ppm_pool_bwd";
  PpmPlan p;
  int rc = ppm_plan(who, nb, scales, B, H, W, C, Cb, p);
  if (rc || (rc = ppm_act(who, dcat, lddcat, C)) || (rc = ppm_act(who, dx, lddx, C))) return rc;
  VKAS_CHECK(dp && vkas_aligned16(dp), "%s: null / misaligned buffer", who);
  if (B == 0) return VKAS_OK;
  const long items = (long)W * (C / 8);
  VKAS_CHECK(vkas_cdiv(items, 256) <= 65535, "%s: row too wide", who);
  dim3 grid((unsigned)((long)B * H), chunks(items));
  PPM_DISPATCH16(dtype, who, {
    ppm_pool_bwd_kernel<T><<<grid, 256, 0, vkas_stream(stream)>>>((const T*)dcat, lddcat, dp, (T*)dx, lddx, p, B, H, W, C);
  })
  VKAS_LAUNCH_CHECK("ppm_pool_bwd");
  return VKAS_OK;
}
