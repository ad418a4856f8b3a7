// Fused head tail, backward side (the forward side lives in the NT GEMM epilogue, gemm_mfma.hip):
//   z (pre-LN conv output, kept by the forward) --LayerNorm--> u --GELU--> a --Linear(C -> oc <= 4)--> proj
// Given d(proj) this kernel recomputes u and a from z and the saved row statistics and produces dz together with the
// parameter gradients (gamma, beta, Wproj, bproj) in one pass over z: the (M, C) activation and its gradient never exist
// in HBM (model/upernext.py:215-223, model/fpn.py:165-183; backward of helper.py:96-101 + helper.py:18-22).
#include "vkas_common.h"

int vkas_colreduce_finalize(const float* partial, long P, int n, int ldp, float* out, int accumulate, hipStream_t st);

namespace {

// G = lanes per pixel row, one 8-channel vector each: 32 for heads up to 256 (padded) channels - ConvNeXt-T / S: 192-194 -,
// 64 up to 512 (Base: 256-258, Large: 384+)
constexpr int R = 2;    // rows in flight per lane group
#ifndef HT_R1
#define HT_R1 3
#endif

__global__ void pack_head_params_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                        const float* __restrict__ wproj, const float* __restrict__ bproj, int C, int oc,
                                        int pw, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * pw + 8) return;
  float v = 0.f;
  if (i < pw) v = i < C ? gamma[i] : 0.f;
  else if (i < 2 * pw) v = (i - pw) < C ? beta[i - pw] : 0.f;
  else if (i < 6 * pw) {
    const int q = (i - 2 * pw) / pw, c = (i - 2 * pw) - q * pw;
    v = (q < oc && c < C) ? wproj[(long)q * C + c] : 0.f;
  } else {
    const int q = i - 6 * pw;
    v = q < oc ? bproj[q] : 0.f;
  }
  out[i] = v;
}

// One launch handles ALL heads of a pass: lane group g (32 lanes) of a workgroup works on head g % NH of row g / NH, so a
// workgroup reads and writes whole rows of the shared (M, sum np) buffers (the per-head column slices are not
// 128-byte aligned; per-head launches left every row with partially written cache lines).
struct HeadBwdArgs {
  int n_heads, pw;
  int n0[4], np[4], c[4];
  const float* dproj[4];  // (M, 8) fp32 each
};

// OCM: upper bound of the heads' out_channels in this launch (1 for the rough pass: a quarter of the projection math and
// 48 fewer accumulator registers).  The z / statistics / d(proj) loads of the NEXT row pair are issued before the current
// pair is processed: with ~2 waves per SIMD the kernel was bound by the latency of one 16-byte load per lane per iteration.
template <typename T, int NH, int OCM, int G>
__global__ __launch_bounds__(256) void head_tail_bwd_kernel(const T* __restrict__ z, long ldz,
                                                            const float* __restrict__ params,
                                                            const float* __restrict__ stats, HeadBwdArgs a,
                                                            T* __restrict__ dz, long lddz, float* __restrict__ partial,
                                                            long M, long rows_per_block) {
  static_assert(NH == 1 || NH == 2 || NH == 4, "lane groups per row");
  // rows in flight per lane group: the 1-channel heads (the dense launches of a train step) leave the registers for four -
  // at two waves per SIMD the kernel is bound by the bytes it keeps in flight, not by its arithmetic alone
  constexpr int RR = OCM == 1 ? HT_R1 : R;
  constexpr int rpi = 256 / G / NH;  // rows per sub-iteration
  constexpr int VEC = 16 / sizeof(T);
  typedef uint4 raw_t;               // 16 bytes of z: 8 bf16 (one per lane and row) / first half of 8 fp32
  const int gl = threadIdx.x & (G - 1);
  const int grp = threadIdx.x / G;
  const int head = grp % NH, rl = grp / NH;
  const bool hok = head < a.n_heads;
  const int pw = a.pw, PS = 6 * pw + 8;
  const int C = hok ? a.c[head] : 1, np = hok ? a.np[head] : 0, n0 = hok ? a.n0[head] : 0;
  const float* hstats = stats + (long)head * M * 2;
  const int nvec = np >> 3;
  const long mbeg = (long)blockIdx.x * rows_per_block;
  const long mend = mbeg + rows_per_block < M ? mbeg + rows_per_block : M;
  const bool vok = hok && gl < nvec;
  // gamma | beta | Wproj[4] of every head live in LDS (each lane re-reads its 8-channel slice per row)
  // Each of a head's six vectors takes G * 8 floats, zero beyond pw: every lane of a group reads its 8-channel slice
  // UNCONDITIONALLY (lanes past the head's width get zeros).  Round 4: with these 16-byte LDS reads under a partial EXEC mask
  // (lanes >= np / 8 off) the last active 8-lane beat of the upper half-wave sporadically delivered stale registers when a
  // second process kept the CU's LDS busy (profiles/repro/repro_step_determinism5.py) - full-wave reads do not.
  constexpr int GW = G * 8;
  __shared__ __attribute__((aligned(16))) float sp[NH * 6 * GW];
  for (int i = threadIdx.x; i < NH * 6 * GW; i += 256) {
    const int h = i / (6 * GW), r = i - h * 6 * GW, k = r / GW, j = r - k * GW;
    sp[i] = (h < a.n_heads && j < pw) ? params[(long)h * PS + k * pw + j] : 0.f;
  }
  __syncthreads();
  const float* hp = sp + head * 6 * GW;
  // element pairs (round 4): packed fp32 arithmetic - v_pk_fma_f32 / v_pk_mul_f32 issue at the rate of their scalar forms, and
  // this kernel is bound by its vector instructions.  GELU' is the degree-9 polynomial of the MLP's GELU' epilogue (|error| <=
  // 1.8e-4) instead of Phi + u phi with a v_exp_f32 (quarter rate, and not packable).
  f32x2 dg[4], db[4], dwp[OCM][4];
  float dbp[OCM];
#pragma unroll
  for (int c = 0; c < 4; ++c) { dg[c] = f32x2{0.f, 0.f}; db[c] = f32x2{0.f, 0.f}; }
#pragma unroll
  for (int q = 0; q < OCM; ++q) {
    dbp[q] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) dwp[q][c] = f32x2{0.f, 0.f};
  }
  // channel validity of this lane's 8 channels as a mask of multiplicative 0/1 (pad channels carry gamma = beta = 0 and
  // Wproj = 0, so only the LayerNorm sums need it)
  float cm[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) cm[c] = (vok && gl * 8 + c < C) ? 1.f : 0.f;
  const float invC = 1.f / (float)C;

  // in-flight loads of one row pair
  Raw8<T> xr[RR];  // as loaded: converted when the pair is processed, not when it is requested
  float mean[RR], rstd[RR];
  float4 dp[RR];
  // every lane loads UNCONDITIONALLY from an address that is always valid (its row clamped into the block, a lane beyond the
  // head's width reads the head's first slice) and what it must not use is zeroed afterwards: no load under a partial EXEC mask
  const float* hdproj_c = a.dproj[hok ? head : 0];
  const float* hstats_c = hok ? hstats : stats;
  const T* zcol = z + n0 + (vok ? gl : 0) * 8;
  auto fetch = [&](long m0) {
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const long m = m0 + (long)r * rpi + rl;
      const long mc = m < mend ? m : mbeg;
      const float2 st2 = *reinterpret_cast<const float2*>(hstats_c + 2 * mc);
      mean[r] = st2.x;
      rstd[r] = st2.y;
      dp[r] = *reinterpret_cast<const float4*>(hdproj_c + mc * 8);
      xr[r].load(zcol + mc * ldz);
    }
  };
  fetch(mbeg);
  for (long m0 = mbeg; m0 < mend; m0 += (long)RR * rpi) {
    float x[RR][8], mu[RR], rs[RR];
    float4 d4v[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const bool ok = hok && m0 + (long)r * rpi + rl < mend;  // the masks of the unconditional loads, applied on use
      mu[r] = ok ? mean[r] : 0.f;
      rs[r] = ok ? rstd[r] : 0.f;
      d4v[r] = ok ? dp[r] : make_float4(0.f, 0.f, 0.f, 0.f);
      xr[r].keep_if(ok && vok);
      xr[r].unpack(x[r]);
    }
    if (m0 + (long)RR * rpi < mend) fetch(m0 + (long)RR * rpi);  // next pair: in flight behind this pair's arithmetic
    float gm[8], bt[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { gm[c] = 0.f; bt[c] = 0.f; }
    int lo = gl * 8;
    asm volatile("" : "+v"(lo));  // opaque per iteration: keeps the parameter loads in the loop (LICM would pin their VGPRs)
    load8(hp + lo, gm);
    load8(hp + GW + lo, bt);
    f32x2 g[RR][4], hh[RR][4];
    float s1[RR], s2[RR];
    f32x2 gm2[4], bt2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      gm2[c] = f32x2{gm[2 * c], gm[2 * c + 1]};
      bt2[c] = f32x2{bt[2 * c], bt[2 * c + 1]};
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const float d4[4] = {d4v[r].x, d4v[r].y, d4v[r].z, d4v[r].w};
      if (gl == 0) {
#pragma unroll
        for (int q = 0; q < OCM; ++q) dbp[q] += d4[q];
      }
      f32x2 act[4], gp[4], da[4];
      const f32x2 rs2 = pk_splat(rs[r]), nmr = pk_splat(-mu[r] * rs[r]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // (no validity masks in the sums: a pad channel has gamma = beta = Wproj = 0, so its d(act) and everything derived
        // from it is zero whatever h is; a row beyond the block has zero statistics and zero d(proj))
        const f32x2 h = pk_fma(f32x2{x[r][2 * c], x[r][2 * c + 1]}, rs2, nmr);
        const f32x2 u = pk_fma(h, gm2[c], bt2[c]);
        act[c] = gelu2_t<T>(u);
        gp[c] = dgelu2_t<T>(u);
        hh[r][c] = h;
        da[c] = f32x2{0.f, 0.f};
      }
#pragma unroll
      for (int q = 0; q < OCM; ++q) {
        float wp[8];
        load8(hp + (2 + q) * GW + lo, wp);
        const f32x2 dq = pk_splat(d4[q]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          da[c] = pk_fma(dq, f32x2{wp[2 * c], wp[2 * c + 1]}, da[c]);
          dwp[q][c] = pk_fma(dq, act[c], dwp[q][c]);
        }
      }
      f32x2 t1 = {0.f, 0.f}, t2 = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x2 gg = da[c] * gp[c];
        g[r][c] = gg;
        dg[c] = pk_fma(gg, hh[r][c], dg[c]);
        db[c] += gg;
        const f32x2 dxh = gg * gm2[c];
        t1 += dxh;
        t2 = pk_fma(dxh, hh[r][c], t2);
      }
      s1[r] = t1.x + t1.y;
      s2[r] = t2.x + t2.y;
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      s1[r] = group_sum<G>(s1[r]);
      s2[r] = group_sum<G>(s2[r]);
      s1[r] *= invC;
      s2[r] *= invC;
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      const long m = m0 + (long)r * rpi + rl;
      if (m >= mend || !vok) continue;
      float o[8];
      const f32x2 ns1 = pk_splat(-s1[r]), ns2 = pk_splat(-s2[r]), rs2 = pk_splat(rs[r]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x2 v = f32x2{cm[2 * c], cm[2 * c + 1]} * rs2 * pk_fma(hh[r][c], ns2, pk_fma(g[r][c], gm2[c], ns1));
        o[2 * c] = v.x;
        o[2 * c + 1] = v.y;
      }
      store8(dz + m * lddz + n0 + gl * 8, o);
    }
  }
  // reduce the per-thread column sums over the row lanes; partial row per head = dgamma | dbeta | dWp[4] | dbp[8]
  __shared__ float red[256 * 8];
  float* prow = partial + ((long)blockIdx.x * NH + head) * PS;
  auto reduce_store = [&](const float* vals, int dst_off) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c) red[threadIdx.x * 8 + c] = vals[c];
    __syncthreads();
    if (rl == 0 && gl * 8 < pw) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < rpi; ++r) s += red[(((r * NH + head) * G) + gl) * 8 + c];
        prow[dst_off + gl * 8 + c] = vok ? s : 0.f;
      }
    }
  };
  auto flat8 = [](const f32x2 (&v)[4], float (&f)[8]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) { f[2 * c] = v[c].x; f[2 * c + 1] = v[c].y; }
  };
  float f8[8];
  flat8(dg, f8);
  reduce_store(f8, 0);
  flat8(db, f8);
  reduce_store(f8, pw);
  const float zero8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < OCM) {
      flat8(dwp[q < OCM ? q : 0], f8);
      reduce_store(f8, (2 + q) * pw);
    } else {
      reduce_store(zero8, (2 + q) * pw);
    }
  }
  float b8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < OCM; ++q) b8[q] = dbp[q];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 8; ++c) red[threadIdx.x * 8 + c] = b8[c];
  __syncthreads();
  if (rl == 0 && gl < 8) {
    float s = 0.f;
    for (int r = 0; r < rpi; ++r) s += red[((r * NH + head) * G) * 8 + gl];  // gl == 0 lanes hold the row sums of d(proj)
    prow[6 * pw + gl] = s;
  }
}

// Forward side as a kernel of its own, for heads wider than the 224 columns the GEMM epilogue holds (ConvNeXt-Base / Large:
// 256-258 / 384+ channels): the convolution writes z = acc + bias through its plain epilogue and this pass turns z into the
// projected channels and the LayerNorm statistics - the (M, C) activation still never exists, z is read once.
struct HeadFwdArgs {
  int n_heads, pw;
  int n0[4], np[4], c[4];
};
template <typename T, int NH, int G>
__global__ __launch_bounds__(256) void head_tail_fwd_kernel(const T* __restrict__ z, long ldz, const float* __restrict__ params,
                                                            float* __restrict__ stats, float* __restrict__ proj,
                                                            HeadFwdArgs a, long M) {
  constexpr int rpi = 256 / G / NH;
  const int gl = threadIdx.x & (G - 1);
  const int grp = threadIdx.x / G;
  const int head = grp % NH, rl = grp / NH;
  const bool hok = head < a.n_heads;
  const int pw = a.pw, PS = 6 * pw + 8;
  const int C = hok ? a.c[head] : 1, np = hok ? a.np[head] : 0, n0 = hok ? a.n0[head] : 0;
  const bool vok = hok && gl < (np >> 3);
  __shared__ __attribute__((aligned(16))) float sp[NH * (6 * G * 8 + 8)];
  for (int i = threadIdx.x; i < NH * PS; i += 256) {
    const int h = i / PS;
    sp[i] = h < a.n_heads ? params[i] : 0.f;
  }
  __syncthreads();
  const float* hp = sp + head * PS;
  float gm[8], bt[8], wp[4][8], cm[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    gm[c] = bt[c] = 0.f;
    cm[c] = (vok && gl * 8 + c < C) ? 1.f : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) wp[q][c] = 0.f;
  }
  if (vok) {
    load8(hp + gl * 8, gm);
    load8(hp + pw + gl * 8, bt);
#pragma unroll
    for (int q = 0; q < 4; ++q) load8(hp + (2 + q) * pw + gl * 8, wp[q]);
  }
  const float invC = 1.f / (float)C;
  // four rows per trip: their 16-byte pieces are requested together as raw registers before the first one is converted (round 4;
  // one row per trip left every row's memory round trip exposed: 1.30 ms for 573 k pixels x 4 heads of config #5)
  constexpr int RU = 4;
  const long stride = (long)gridDim.x * rpi;
  for (long m0 = (long)blockIdx.x * rpi + rl; m0 < M; m0 += RU * stride) {
    Raw8<T> raw[RU];
    // unconditional loads from clamped addresses, as in the backward kernel above: a lane beyond the head's width reads the
    // head's first slice (its channel mask cm is zero), a row beyond M is never used
    const T* zcol = z + n0 + (vok ? gl : 0) * 8;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const long mu = m0 + u * stride;
      raw[u].load(zcol + (mu < M ? mu : M - 1) * ldz);
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
    const long m = m0 + u * stride;
    if (m >= M) break;
    float x[8];
    raw[u].unpack(x);
    // element pairs: packed fp32 arithmetic (v_pk_fma_f32 ...) - the kernel is bound by its vector instructions, not by HBM
    f32x2 xp[4], s2 = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      xp[c] = f32x2{x[2 * c], x[2 * c + 1]};
      s2 = pk_fma(xp[c], f32x2{cm[2 * c], cm[2 * c + 1]}, s2);
    }
    const float mean = group_sum<G>(s2.x + s2.y) * invC;
    f32x2 q2 = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      xp[c] = (xp[c] - pk_splat(mean)) * f32x2{cm[2 * c], cm[2 * c + 1]};
      q2 = pk_fma(xp[c], xp[c], q2);
    }
    const float rstd = rsqrtf(group_sum<G>(q2.x + q2.y) * invC + 1e-6f);
    f32x2 pr2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // pad channels: gamma = beta = 0 and the mask
      const f32x2 g2 = f32x2{gm[2 * c], gm[2 * c + 1]} * pk_splat(rstd);
      const f32x2 act = gelu2_t<T>(pk_fma(xp[c], g2, f32x2{bt[2 * c], bt[2 * c + 1]})) * f32x2{cm[2 * c], cm[2 * c + 1]};
#pragma unroll
      for (int q = 0; q < 4; ++q) pr2[q] = pk_fma(act, f32x2{wp[q][2 * c], wp[q][2 * c + 1]}, pr2[q]);
    }
    float pr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) pr[q] = group_sum<G>(pr2[q].x + pr2[q].y);
    if (gl == 0 && hok) {
      const float4 bp = *reinterpret_cast<const float4*>(hp + 6 * pw);
      float* po = proj + ((long)head * M + m) * 8;
      *reinterpret_cast<float4*>(po) = make_float4(pr[0] + bp.x, pr[1] + bp.y, pr[2] + bp.z, pr[3] + bp.w);
      *reinterpret_cast<float4*>(po + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (stats) {
        stats[((long)head * M + m) * 2] = mean;
        stats[((long)head * M + m) * 2 + 1] = rstd;
      }
    }
    }
  }
}

// Heads' forward at the neck's height: T (B, h, W2, 3 Nt) = the 1x3 row convolution of Ux x, column ky * Nt + n, holds per
// kernel row ky the convolution's sums BEFORE the y half of the x2 bilinear upsample.  This pass applies that half and the 3x3's
// sum over ky, z[r] = bias + sum_ky (Uy T_ky)[r + ky - 1] (a tap row outside [0, 2h) is the convolution's zero padding, not a
// clamped row), stores z as the fused epilogue does and runs the same tail on the unrounded sums (LayerNorm statistics from
// E[z^2] - mean^2, polynomial GELU, projection; pad columns are exact zeros).
// Eight lanes hold one (pixel, head): lane l owns the 8-channel vectors l, l + 8, l + 16, l + 24 of the head (every load or store
// of a group is one 128-byte run), a wave holds eight consecutive pixel columns of ONE head, so the vectors walked (nv) and the
// projection rows (oc) are wave-uniform, and a workgroup NH heads x 32 / NH columns.  The group streams down the source rows of
// a segment.  Source row j gives, per channel,
//             z[2j-2]  z[2j-1]  z[2j]  z[2j+1]  z[2j+2]  z[2j+3]
//   T0[j]        -        -      .25     .75      .75      .25
//   T1[j]        -       .25     .75     .75      .25       -
//   T2[j]       .25      .75     .75     .25       -        -
// (at the image's top and bottom the clamped blend has weight 1 and the tap row outside is dropped: workgroup-uniform weights).
// When row j arrives, z[2j-2] and z[2j-1] are completed and go through the tail together (the parameters are read from LDS once
// for both); then z[2j] and z[2j+1] start as fp32 partial sums from bias, the raw T0 / T1 of row j - 1 and row j.  Row j + 1 is
// requested before the tail.  Fixed order of every sum: bias, then the contributions in ascending source row and ky, each one
// fma (packed fp32); no atomics, two launches give the same bits.  A segment start costs one warm-up row (T0 / T1 of row i0 - 1).
struct HeadRowsArgs {
  int n_heads, pw;
  int n0[4], np[4], c[4], oc[4];
};
__device__ __forceinline__ int pick4(const int (&v)[4], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3])); }
template <typename T> __device__ __forceinline__ void unpack2(const Raw8<T>& r, f32x2 (&u)[4]) {
  float x[8];
  r.unpack(x);
#pragma unroll
  for (int c = 0; c < 4; ++c) u[c] = f32x2{x[2 * c], x[2 * c + 1]};
}

// NV: upper bound of the 8-channel vectors per lane (3: heads up to 192 padded columns, 4: up to 256)
template <typename T, int NH, int NV>
__global__ __launch_bounds__(256, 2) void head_rows_fwd_kernel(const T* __restrict__ Tt, const float* __restrict__ bias,
                                                               const float* __restrict__ params, T* __restrict__ z,
                                                               float* __restrict__ stats, float* __restrict__ proj,
                                                               HeadRowsArgs a, int h, int W2, int Nt, int seg, int nseg, long M) {
  constexpr int G = 8, GW = 256, HS = 7 * GW + 8;
  constexpr int CPB = 32 / NH;  // pixel columns per workgroup
  const int pw = a.pw, PS = 6 * pw + 8;
  // gamma | beta | Wproj[4] | conv bias of every head, each GW floats and zero beyond the head's width, then bproj
  __shared__ __attribute__((aligned(16))) float sp[NH * HS];
  for (int i = threadIdx.x; i < NH * HS; i += 256) {
    const int hh = i / HS, r = i - hh * HS;
    float v = 0.f;
    if (hh < a.n_heads) {
      if (r < 6 * GW) {
        const int k = r / GW, j = r - k * GW;
        if (j < pw) v = params[(long)hh * PS + k * pw + j];
      } else if (r < 7 * GW) {
        const int j = r - 6 * GW;
        if (j < pick4(a.np, hh)) v = bias[pick4(a.n0, hh) + j];
      } else {
        v = params[(long)hh * PS + 6 * pw + (r - 7 * GW)];
      }
    }
    sp[i] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, gl = lane & (G - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the heads rotate over a workgroup's waves from one workgroup to the next: a wave's cost follows its head's width and
  // projection rows, and wave k of every workgroup may land on the same SIMD
  const int head = (wave + (int)(blockIdx.x % NH)) % NH, cw = wave / NH;
  if (head >= a.n_heads) return;  // wave-uniform; no barrier follows
  const int cblocks = (W2 + CPB - 1) / CPB;
  long bx = blockIdx.x;
  const int cbk = (int)(bx % cblocks);
  bx /= cblocks;
  const int sgi = (int)(bx % nseg);
  const long b = bx / nseg;
  const int X0 = cbk * CPB + cw * 8;
  if (X0 >= W2) return;
  const int X = X0 + (lane >> 3);
  const bool xok = X < W2;
  const int C = pick4(a.c, head), np = pick4(a.np, head), n0 = pick4(a.n0, head), oc = pick4(a.oc, head);
  const int nvec = np >> 3, nv = (nvec + 7) >> 3;  // nv <= NV: the launcher's choice of NV
  const float* hp = sp + head * HS;
  const int i0 = sgi * seg, i1 = i0 + seg < h ? i0 + seg : h;
  const long ldT = 3L * Nt;
  // unconditional loads from clamped addresses (column clamped into the row, a vector beyond the head's width reads the head's
  // first one, a row beyond the image its last row); what must not be used is zeroed or skipped afterwards
  // Every address is a wave-uniform 64-bit base (image, row, ky, head) plus a 32-bit lane offset inside one row of T or z
  // (the launcher checks that a row fits): one offset register per vector instead of a pointer per load
  const long rowT = (long)W2 * ldT;
  const T* timg = Tt + (long)b * h * rowT + n0;
  bool ok[NV];
  unsigned offT[NV], offZ[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    ok[v] = gl + 8 * v < nvec;
    offT[v] = (unsigned)(xok ? X : W2 - 1) * (unsigned)ldT + (ok[v] ? (gl + 8 * v) * 8 : 0);
    offZ[v] = (unsigned)(xok ? X : 0) * (unsigned)Nt + (ok[v] ? (gl + 8 * v) * 8 : 0);
  }
  T* zimg = z ? z + (long)b * 2 * h * W2 * Nt + n0 : nullptr;
  const float fC = (float)C;
  const f32x2 q25 = pk_splat(0.25f), q75 = pk_splat(0.75f);
  f32x2 E[NV][4], O[NV][4];  // partial sums of the even and the odd output row in flight
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) E[v][c] = O[v][c] = pk_splat(0.f);
  Raw8<T> w0[NV][3], w1[NV][3];  // rows j and j + 1, alternating
  // T0 / T1 of row j - 1 wait in LDS, 16 bytes per lane, vector and ky, each lane reading what it wrote: beside the rows in
  // flight, the partial sums and the tail's temporaries they do not fit the 256 registers of two waves per SIMD at NV = 4
  typedef decltype(w0[0][0].a) raw_t;
  __shared__ __attribute__((aligned(16))) raw_t prev[2 * NV][256];
  auto fetch = [&](Raw8<T> (&r)[NV][3], int i, int nky) {
    const int ic = i < 0 ? 0 : (i > h - 1 ? h - 1 : i);
    const T* rp = timg + ic * rowT;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (v >= nv) break;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
        if (ky < nky) r[v][ky].load(rp + ky * Nt + offT[v]);
    }
  };
  auto keep = [&](Raw8<T> (&r)[NV][3]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (v >= nv) break;
      prev[2 * v][threadIdx.x] = r[v][0].a;
      prev[2 * v + 1][threadIdx.x] = r[v][1].a;
    }
  };
  // one source row: returns true after the segment's last output rows
  auto step = [&](Raw8<T> (&Cu)[NV][3], Raw8<T> (&Nx)[NV][3], int j) -> bool {
    const bool have = j < h;  // j == i1 == h: the rows in flight are complete as they stand
    if (j + 1 <= i1 && j + 1 < h) fetch(Nx, j + 1, 3);
    if (j > i0) {
      // output rows 2j - 2 (E) and 2j - 1 (O): last contributions, statistics, z
      T* zE = zimg + (long)(2 * j - 2) * W2 * Nt;
      T* zO = zE + (long)W2 * Nt;
      f32x2 sE = pk_splat(0.f), qE = sE, sO = sE, qO = sE;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (v >= nv) break;
        if (have) {
          f32x2 u1[4], u2[4];
          unpack2(Cu[v][1], u1);
          unpack2(Cu[v][2], u2);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            E[v][c] = pk_fma(u2[c], q25, E[v][c]);
            O[v][c] = pk_fma(u1[c], q25, O[v][c]);
            O[v][c] = pk_fma(u2[c], q75, O[v][c]);
          }
        }
        if (v == nv - 1) {  // the only vector step with lanes beyond the head's width
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            E[v][c] = ok[v] ? E[v][c] : pk_splat(0.f);
            O[v][c] = ok[v] ? O[v][c] : pk_splat(0.f);
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sE = sE + E[v][c];
          qE = pk_fma(E[v][c], E[v][c], qE);
          sO = sO + O[v][c];
          qO = pk_fma(O[v][c], O[v][c], qO);
        }
        if (zimg && xok && ok[v]) {
          float x[8];
#pragma unroll
          for (int c = 0; c < 4; ++c) { x[2 * c] = E[v][c].x; x[2 * c + 1] = E[v][c].y; }
          store8(zE + offZ[v], x);
#pragma unroll
          for (int c = 0; c < 4; ++c) { x[2 * c] = O[v][c].x; x[2 * c + 1] = O[v][c].y; }
          store8(zO + offZ[v], x);
        }
      }
      const float s_e = group_sum<G>(sE.x + sE.y), s_o = group_sum<G>(sO.x + sO.y);
      float q_e = group_sum<G>(qE.x + qE.y), q_o = group_sum<G>(qO.x + qO.y);
      const float meanE = s_e / fC, meanO = s_o / fC;
      q_e = fmaxf(q_e - s_e * meanE, 0.f);  // sum of squared deviations
      q_o = fmaxf(q_o - s_o * meanO, 0.f);
      const float rstdE = rsqrtf(q_e / fC + 1e-6f), rstdO = rsqrtf(q_o / fC + 1e-6f);
      const f32x2 muE = pk_splat(meanE), muO = pk_splat(meanO), rsE = pk_splat(rstdE), rsO = pk_splat(rstdO);
      f32x2 prE[4], prO[4];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) prE[qq] = prO[qq] = pk_splat(0.f);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (v >= nv) break;
        int lo = (gl + 8 * v) * 8;
        asm volatile("" : "+v"(lo));  // keeps the parameter reads in the loop
        // four channels at a time, fenced: gamma, beta, two activations per row and one weight quad are all that is live
        // beside the rows themselves (the whole vector at once does not fit the 256 registers at NV = 4)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          float gm[4], bt[4];
          load4(hp + lo + 4 * hf, gm);
          load4(hp + GW + lo + 4 * hf, bt);
          // the head's own projection rows (wave-uniform), requested before the activations so that their LDS latency passes
          // behind the GELU arithmetic
          float w[4][4];
#pragma unroll
          for (int qq = 0; qq < 4; ++qq)
            if (qq < oc) load4(hp + (2 + qq) * GW + lo + 4 * hf, w[qq]);
          f32x2 aE[2], aO[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) {  // pad and masked channels: z = gamma = beta = 0
            const f32x2 g2 = {gm[2 * c], gm[2 * c + 1]}, b2 = {bt[2 * c], bt[2 * c + 1]};
            aE[c] = gelu2_t<T>(pk_fma((E[v][2 * hf + c] - muE) * rsE, g2, b2));
            aO[c] = gelu2_t<T>(pk_fma((O[v][2 * hf + c] - muO) * rsO, g2, b2));
          }
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            if (qq >= oc) break;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const f32x2 wc = {w[qq][2 * c], w[qq][2 * c + 1]};
              prE[qq] = pk_fma(aE[c], wc, prE[qq]);
              prO[qq] = pk_fma(aO[c], wc, prO[qq]);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      float pe[4] = {0.f, 0.f, 0.f, 0.f}, po[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        if (qq >= oc) break;
        pe[qq] = group_sum<G>(prE[qq].x + prE[qq].y);
        po[qq] = group_sum<G>(prO[qq].x + prO[qq].y);
      }
      const float4 bp = *reinterpret_cast<const float4*>(hp + 7 * GW);  // zero beyond oc; read by the full wave
      if (gl == 0 && xok) {
        const long mE = ((long)b * 2 * h + 2 * j - 2) * W2 + X, mO = mE + W2;
        float* pE = proj + ((long)head * M + mE) * 8;
        float* pO = proj + ((long)head * M + mO) * 8;
        *reinterpret_cast<float4*>(pE) = make_float4(pe[0] + bp.x, pe[1] + bp.y, pe[2] + bp.z, pe[3] + bp.w);
        *reinterpret_cast<float4*>(pE + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(pO) = make_float4(po[0] + bp.x, po[1] + bp.y, po[2] + bp.z, po[3] + bp.w);
        *reinterpret_cast<float4*>(pO + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (stats) {
          *reinterpret_cast<float2*>(stats + ((long)head * M + mE) * 2) = make_float2(meanE, rstdE);
          *reinterpret_cast<float2*>(stats + ((long)head * M + mO) * 2) = make_float2(meanO, rstdO);
        }
      }
    }
    if (j >= i1) return true;
    // output rows 2j and 2j + 1 start: bias, row j - 1 (T0, T1), row j (T0, T1, T2); row j + 1 completes them
    const bool top = j == 0, bot = j + 1 >= h;  // workgroup-uniform
    const f32x2 wE0 = pk_splat(top ? 0.f : 0.25f), wE1 = pk_splat(top ? 1.f : 0.75f), wE2 = pk_splat(bot ? 1.f : 0.75f);
    const f32x2 wO0 = pk_splat(top ? 1.f : 0.75f), wO1 = pk_splat(bot ? 1.f : 0.75f), wO2 = pk_splat(bot ? 0.f : 0.25f);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (v >= nv) break;
      int lo = (gl + 8 * v) * 8;
      asm volatile("" : "+v"(lo));
      float bs[8];
      load8(hp + 6 * GW + lo, bs);
      f32x2 e[4], o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) e[c] = o[c] = f32x2{bs[2 * c], bs[2 * c + 1]};
      // one ky at a time, fenced: eight converted values are live at once.  The asm barrier stops the compiler from carrying
      // the fp32 form of T1 / T2, converted for the completion above, across the tail: twice the registers of the raw row
      if (!top) {
        Raw8<T> pr;
        f32x2 p[4];
        pr.a = prev[2 * v][threadIdx.x];
        unpack2(pr, p);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          e[c] = pk_fma(p[c], q75, e[c]);
          o[c] = pk_fma(p[c], q25, o[c]);
        }
        __builtin_amdgcn_sched_barrier(0);
        pr.a = prev[2 * v + 1][threadIdx.x];
        unpack2(pr, p);
#pragma unroll
        for (int c = 0; c < 4; ++c) e[c] = pk_fma(p[c], q25, e[c]);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("" : "+v"(Cu[v][1].a), "+v"(Cu[v][2].a));
      f32x2 u[4];
      unpack2(Cu[v][0], u);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        e[c] = pk_fma(u[c], wE0, e[c]);
        o[c] = pk_fma(u[c], wO0, o[c]);
      }
      __builtin_amdgcn_sched_barrier(0);
      unpack2(Cu[v][1], u);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        e[c] = pk_fma(u[c], wE1, e[c]);
        o[c] = pk_fma(u[c], wO1, o[c]);
      }
      __builtin_amdgcn_sched_barrier(0);
      unpack2(Cu[v][2], u);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        E[v][c] = pk_fma(u[c], wE2, e[c]);
        O[v][c] = pk_fma(u[c], wO2, o[c]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    keep(Cu);
    return false;
  };
  if (i0 > 0) {  // the warm-up row of a segment inside the image
    fetch(w1, i0 - 1, 2);
    keep(w1);
  }
  fetch(w0, i0, 3);
  // two register sets alternate: two source rows per trip keep every index a compile-time constant
  for (int j = i0;; j += 2) {
    if (step(w0, w1, j)) break;
    if (step(w1, w0, j + 1)) break;
  }
}

// Segment length of the row pass, by the criterion of cs_seg_rows (upconv_adj.hip): the fewest row steps per CU slot (a segment
// walks its rows and one warm-up row) among the lengths that fill the slots - two workgroups on each of the 256 CUs - four times
// over.  One workgroup per slot leaves every SIMD with the cost of its slowest wave until the launch ends: at B = 8, h = 256,
// W2 = 512 the precise set takes 2.80 ms in segments of 256 rows (one round), 2.64 at 128, 2.50 at 64, 2.46 at 32 and 2.50 at
// 16, the rough set 1.36 / 0.94 / 0.94 / 0.95 / 0.97 ms (profiles/head_rows_groups.log).
static inline int hr_seg_rows(long cols, int h) {
  const long slots = 4 * 2 * 256;
  long best = h, best_cost = -1;
  bool best_full = false;
  for (long seg = h; seg >= 1; --seg) {
    const long nseg = vkas_cdiv(h, seg);
    if (vkas_cdiv(h, nseg) != seg) continue;  // the same cut with a shorter last segment
    const long wgs = cols * nseg;
    const long cost = vkas_cdiv(wgs, slots) * (seg + 1);
    const bool full = wgs >= slots;
    if (best_cost < 0 || (full && !best_full) || (full == best_full && cost < best_cost)) {
      best = seg; best_cost = cost; best_full = full;
    }
  }
  return (int)best;
}

static inline int ht_lanes(int pw) { return pw <= 256 ? 32 : 64; }
static inline long ht_rows_per_block(long M, int G) {
  long r = vkas_cdiv(M > 0 ? M : 1, 1024);
  if (r < 32) r = 32;
  const long q = (long)(HT_R1 > R ? HT_R1 : R) * (256 / G);  // multiple of the rows per iteration for every NH and OCM
  return vkas_cdiv(r, q) * q;
}

}  // namespace

extern "C" int vkas_pack_head_params(const float* gamma, const float* beta, const float* wproj, const float* bproj, int C,
                                     int oc, int pw, float* out, void* stream) {
  VKAS_CHECK(gamma && beta && wproj && bproj && out, "vkas_pack_head_params: null pointer");
  VKAS_CHECK(C > 0 && oc >= 1 && oc <= 4 && pw % 8 == 0 && pw >= C && pw <= 512, "vkas_pack_head_params: bad C=%d oc=%d pw=%d", C,
             oc, pw);
  pack_head_params_kernel<<<(unsigned)vkas_cdiv(6 * pw + 8, 256), 256, 0, vkas_stream(stream)>>>(gamma, beta, wproj, bproj, C,
                                                                                                oc, pw, out);
  VKAS_LAUNCH_CHECK("pack_head_params");
  return VKAS_OK;
}

extern "C" size_t vkas_head_tail_bwd_ws_bytes(long M, int pw) {
  return (size_t)vkas_cdiv(M > 0 ? M : 1, ht_rows_per_block(M, ht_lanes(pw))) * 4 * (size_t)(6 * pw + 8) * sizeof(float);
}

extern "C" int vkas_head_tail_fwd(const void* z, long ldz, const vkas_head_desc* hd, long M, int dtype, void* stream) {
  VKAS_CHECK(z && hd && hd->params && hd->proj, "vkas_head_tail_fwd: null pointer");
  const int pw = hd->pw, nh = hd->n_heads;
  VKAS_CHECK(nh >= 1 && nh <= 4 && pw % 8 == 0 && pw >= 8 && pw <= 512, "vkas_head_tail_fwd: bad descriptor");
  HeadFwdArgs a;
  a.n_heads = nh;
  a.pw = pw;
  for (int h = 0; h < 4; ++h) {
    a.n0[h] = h < nh ? hd->n0[h] : 0;
    a.np[h] = h < nh ? hd->np[h] : 0;
    a.c[h] = h < nh ? hd->c[h] : 1;
    if (h < nh) {
      VKAS_CHECK(a.np[h] % 8 == 0 && a.np[h] > 0 && a.np[h] <= pw && a.c[h] > 0 && a.c[h] <= a.np[h] && a.n0[h] % 8 == 0 &&
                     a.n0[h] + a.np[h] <= ldz && hd->oc[h] >= 1 && hd->oc[h] <= 4,
                 "vkas_head_tail_fwd: bad head %d", h);
    }
  }
  VKAS_CHECK(ldz % 8 == 0 && vkas_aligned16(z) && vkas_aligned16(hd->params) && vkas_aligned16(hd->proj),
             "vkas_head_tail_fwd: bad strides/alignment");
  if (M <= 0) return VKAS_OK;
  hipStream_t st = vkas_stream(stream);
  const int GL = ht_lanes(pw);
  const int NH = nh == 1 ? 1 : (nh == 2 ? 2 : 4);
  const long rows_per_iter = 256 / GL / NH;
  long blocks = vkas_cdiv(M, rows_per_iter * 8);  // ~8 rows per lane group
  if (blocks > 4096) blocks = 4096;
#define VKAS_HF(NHV)                                                                                                          \
  do {                                                                                                                        \
    if (GL == 32)                                                                                                             \
      head_tail_fwd_kernel<T, NHV, 32><<<(unsigned)blocks, 256, 0, st>>>((const T*)z, ldz, hd->params, hd->stats, hd->proj, a, M); \
    else                                                                                                                      \
      head_tail_fwd_kernel<T, NHV, 64><<<(unsigned)blocks, 256, 0, st>>>((const T*)z, ldz, hd->params, hd->stats, hd->proj, a, M); \
  } while (0)
  VKAS_DISPATCH_DTYPE(dtype, "vkas_head_tail_fwd", {
    if (NH == 1) VKAS_HF(1);
    else if (NH == 2) VKAS_HF(2);
    else VKAS_HF(4);
  })
#undef VKAS_HF
  VKAS_LAUNCH_CHECK("head_tail_fwd");
  return VKAS_OK;
}

extern "C" int vkas_head_rows_fwd(const void* Tt, const float* bias, const vkas_head_desc* hd, void* z, int B, int h, int W2,
                                  int Nt, int seg_rows, int dtype, void* stream) {
  VKAS_CHECK(Tt && bias && hd && hd->params && hd->proj, "vkas_head_rows_fwd: null pointer");
  const int pw = hd->pw, nh = hd->n_heads;
  VKAS_CHECK(nh >= 1 && nh <= 4 && pw % 8 == 0 && pw >= 8 && pw <= 256, "vkas_head_rows_fwd: bad descriptor (pw <= 256)");
  VKAS_CHECK(B >= 0 && h > 0 && W2 > 0 && Nt > 0 && Nt % 8 == 0 && seg_rows >= 0, "vkas_head_rows_fwd: bad sizes");
  VKAS_CHECK(3L * Nt * W2 < (1L << 30), "vkas_head_rows_fwd: a row of T beyond 2^31 bytes (32-bit lane offsets)");
  VKAS_CHECK((hd->stats != nullptr) == (z != nullptr), "vkas_head_rows_fwd: z and the statistics are kept or dropped together");
  HeadRowsArgs a;
  a.n_heads = nh;
  a.pw = pw;
  int npm = 8;
  for (int k = 0; k < 4; ++k) {
    a.n0[k] = k < nh ? hd->n0[k] : 0;
    a.np[k] = k < nh ? hd->np[k] : 0;
    a.c[k] = k < nh ? hd->c[k] : 1;
    a.oc[k] = k < nh ? hd->oc[k] : 0;
    if (k < nh) {
      VKAS_CHECK(a.np[k] % 8 == 0 && a.np[k] > 0 && a.np[k] <= pw && a.c[k] > 0 && a.c[k] <= a.np[k] && a.n0[k] % 8 == 0 &&
                     a.n0[k] >= 0 && a.n0[k] + a.np[k] <= Nt && a.oc[k] >= 1 && a.oc[k] <= 4,
                 "vkas_head_rows_fwd: bad head %d", k);
      npm = a.np[k] > npm ? a.np[k] : npm;
    }
  }
  VKAS_CHECK(vkas_aligned16(Tt) && vkas_aligned16(bias) && vkas_aligned16(z) && vkas_aligned16(hd->params) && vkas_aligned16(hd->proj),
             "vkas_head_rows_fwd: misaligned pointer");
  if (B == 0) return VKAS_OK;
  const int NH = nh == 1 ? 1 : (nh == 2 ? 2 : 4);
  const int cpb = 32 / NH;
  const long cols = (long)B * vkas_cdiv(W2, cpb);
  const int seg = seg_rows > 0 ? (seg_rows < h ? seg_rows : h) : hr_seg_rows(cols, h);
  const int nseg = (int)vkas_cdiv(h, seg);
  const long blocks = cols * nseg;
  VKAS_CHECK(blocks < (1L << 31), "vkas_head_rows_fwd: too many workgroups");
  const long M = (long)B * 2 * h * W2;
  hipStream_t st = vkas_stream(stream);
#define VKAS_HR(NHV)                                                                                                          \
  do {                                                                                                                        \
    if (npm <= 192)                                                                                                           \
      head_rows_fwd_kernel<T, NHV, 3><<<(unsigned)blocks, 256, 0, st>>>((const T*)Tt, bias, hd->params, (T*)z, hd->stats,     \
                                                                        hd->proj, a, h, W2, Nt, seg, nseg, M);                \
    else                                                                                                                      \
      head_rows_fwd_kernel<T, NHV, 4><<<(unsigned)blocks, 256, 0, st>>>((const T*)Tt, bias, hd->params, (T*)z, hd->stats,     \
                                                                        hd->proj, a, h, W2, Nt, seg, nseg, M);                \
  } while (0)
  if (dtype == VKAS_BF16) {
    typedef bf16_t T;
    if (NH == 1) VKAS_HR(1); else if (NH == 2) VKAS_HR(2); else VKAS_HR(4);
  } else if (dtype == VKAS_F16) {
    typedef f16_t T;
    if (NH == 1) VKAS_HR(1); else if (NH == 2) VKAS_HR(2); else VKAS_HR(4);
  } else {
    VKAS_CHECK(false, "vkas_head_rows_fwd: 16-bit storage only");
  }
#undef VKAS_HR
  VKAS_LAUNCH_CHECK("head_rows_fwd");
  return VKAS_OK;
}

extern "C" int vkas_head_tail_bwd(const void* z, long ldz, const vkas_head_desc* hd, const float* const* dproj, void* dz,
                                  long lddz, float* dparams, float* ws, size_t ws_bytes, long M, int dtype, void* stream) {
  VKAS_CHECK(z && hd && dproj && dz && dparams && ws && hd->params && hd->stats, "vkas_head_tail_bwd: null pointer");
  const int pw = hd->pw, nh = hd->n_heads;
  VKAS_CHECK(nh >= 1 && nh <= 4 && pw % 8 == 0 && pw >= 8 && pw <= 512, "vkas_head_tail_bwd: bad descriptor");
  HeadBwdArgs a;
  a.n_heads = nh;
  a.pw = pw;
  for (int h = 0; h < 4; ++h) {
    a.n0[h] = h < nh ? hd->n0[h] : 0;
    a.np[h] = h < nh ? hd->np[h] : 0;
    a.c[h] = h < nh ? hd->c[h] : 1;
    a.dproj[h] = h < nh ? dproj[h] : nullptr;
    if (h < nh) {
      VKAS_CHECK(a.np[h] % 8 == 0 && a.np[h] > 0 && a.np[h] <= pw && a.c[h] > 0 && a.c[h] <= a.np[h] && a.n0[h] % 8 == 0 &&
                     a.n0[h] + a.np[h] <= ldz && a.n0[h] + a.np[h] <= lddz && a.dproj[h] && vkas_aligned16(a.dproj[h]),
                 "vkas_head_tail_bwd: bad head %d", h);
    }
  }
  VKAS_CHECK(ldz % 8 == 0 && lddz % 8 == 0 && vkas_aligned16(z) && vkas_aligned16(dz) && vkas_aligned16(hd->params),
             "vkas_head_tail_bwd: bad strides/alignment");
  VKAS_CHECK(ws_bytes >= vkas_head_tail_bwd_ws_bytes(M, pw), "vkas_head_tail_bwd: workspace too small");
  hipStream_t st = vkas_stream(stream);
  const int PS = 6 * pw + 8;
  if (M <= 0) {
    (void)hipMemsetAsync(dparams, 0, (size_t)nh * PS * sizeof(float), st);
    return VKAS_OK;
  }
  const int GL = ht_lanes(pw);
  const long rpb = ht_rows_per_block(M, GL);
  const long P = vkas_cdiv(M, rpb);
  const int NH = nh == 1 ? 1 : (nh == 2 ? 2 : 4);
  int ocm = 1;
  for (int h = 0; h < nh; ++h) ocm = hd->oc[h] > ocm ? hd->oc[h] : ocm;
  VKAS_CHECK(ocm <= 4, "vkas_head_tail_bwd: out_channels %d > 4", ocm);
#define VKAS_HT(NHV, OCV)                                                                                                      \
  do {                                                                                                                         \
    if (GL == 32)                                                                                                              \
      head_tail_bwd_kernel<T, NHV, OCV, 32><<<(unsigned)P, 256, 0, st>>>((const T*)z, ldz, hd->params, hd->stats, a, (T*)dz, lddz, ws, M, rpb); \
    else                                                                                                                       \
      head_tail_bwd_kernel<T, NHV, OCV, 64><<<(unsigned)P, 256, 0, st>>>((const T*)z, ldz, hd->params, hd->stats, a, (T*)dz, lddz, ws, M, rpb); \
  } while (0)
  VKAS_DISPATCH_DTYPE(dtype, "vkas_head_tail_bwd", {
    if (NH == 1) { if (ocm == 1) VKAS_HT(1, 1); else VKAS_HT(1, 4); }
    else if (NH == 2) { if (ocm == 1) VKAS_HT(2, 1); else VKAS_HT(2, 4); }
    else { if (ocm == 1) VKAS_HT(4, 1); else VKAS_HT(4, 4); }
  })
#undef VKAS_HT
  VKAS_LAUNCH_CHECK("head_tail_bwd");
  // partial rows are (block, lane-group head) pairs: NH * PS floats per block; heads beyond n_heads are zero
  return vkas_colreduce_finalize(ws, P, nh * PS, NH * PS, dparams, 0, st);
}
