// "nearest x f, then conv5x5 (pad 2)" without the upsample: the FPN heads' smoothing convolution at upsampling factors
// 3 and 4 (fpn.py:41-48,170-174).  Since pad 2 < f, every output phase (r, s) - the pixels (f i + r, f j + s) - is an
// exact small convolution over the low-resolution input with folded taps: 5x5 tap ky reads low-res row
// i + floor((r + ky - 2) / f), so phase r needs the rows lo(r) .. hi(r), lo = floor((r - 2) / f), hi = floor((r + 2) / f)
// (2 rows per phase at f = 4; 2, 3, 2 at f = 3), and its folded tap t is the sum of the 5x5 taps that land on row lo + t.
// Zero padding maps exactly: upsampled rows -2, -1 fall in low-res row -1, rows fH, fH + 1 in row H.
//
//  * upconv5_nt_kernel: D[m][n] = sum_k A(m,k) Bw[n][k] on the 16-bit matrix cores, 128 x 128 tiles of one phase per
//    workgroup (the phase is blockIdx.y), so the B operand of a workgroup is that phase's folded weight.  A(m, k) for
//    k = (group g, channel c) reads source pixel (a i + dy[g], a j + dx[g]); row m = (b, i, j) is written to output pixel
//    (o i + r, o j + s).  The forward is (a, o) = (1, f) with one group per folded tap; the input gradient is (a, o) =
//    (f, 1) with one group per (phase, tap) - dy read at the phase pixels times the transposed folded taps, summed in
//    registers over every phase (no atomics, deterministic).
//  * weight gradient: the phase sub-lattice of dy is gathered into a compact map (upconv5_gather_phase_kernel) that
//    the implicit-GEMM weight-gradient kernels reduce against the low-res input per phase (the folded dW'), then
//    upconv5_unfold_kernel sums the phases back onto the 5x5 taps.
#include "gemm_parts.h"

int vkas_gemm_tn_mfma_bf16(const void*, const vkas_conv_geom*, const void*, long, int, float*, float*, int, hipStream_t);
int vkas_gemm_tn_mfma_f16(const void*, const vkas_conv_geom*, const void*, long, int, float*, float*, int, hipStream_t);

namespace {

constexpr int UC_BK = 64;
constexpr int UC_MAXG = 64;  // groups of one launch: 16 phases x 4 taps (f = 4 input gradient)

// host + device: floor((r + k - 2) / f) for r + k - 2 >= -2 > -f
__host__ __device__ inline int uc_row(int r, int k, int f) { return (r + k - 2 + f) / f - 1; }
__host__ __device__ inline int uc_lo(int r, int f) { return uc_row(r, 0, f); }
__host__ __device__ inline int uc_ntaps(int r, int f) { return uc_row(r, 4, f) - uc_row(r, 0, f) + 1; }
inline int uc_gmax(int f) { return f == 3 ? 9 : 4; }  // folded taps of the widest phase

struct UcTaps {
  int G[16];       // groups of phase p (K = G[p] * Cg)
  int r[16], s[16];
  short dy[UC_MAXG], dx[UC_MAXG];  // group g of phase p is entry g0[p] + g
  int g0[16];
};

__device__ __forceinline__ int uc_swz(int row, int chunk) { return row * UC_BK + ((chunk ^ (row & 7)) << 3); }

template <typename T>
__device__ __forceinline__ f32x4 uc_mfma(const T& a, const T& b, f32x4 c);
template <>
__device__ __forceinline__ f32x4 uc_mfma<bf16x8>(const bf16x8& a, const bf16x8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 uc_mfma<f16x8>(const f16x8& a, const f16x8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 128 x 128 tile, 4 waves (2 x 2) of 64 x 64 = 4 x 4 MFMA tiles, BK = 64, operands staged global -> registers -> LDS
// (XOR-swizzled 16-byte chunks, double buffered, one barrier per K tile) as in gemm_nt_mfma_kernel.  The MFMA is issued
// with the operands swapped, so a lane holds 4 consecutive output columns of one row.
template <typename E, typename E8>
__global__ __launch_bounds__(256) void upconv5_nt_kernel(const E* __restrict__ src, int B, int HS, int WS, long lds_src,
                                                         int a, int Cg, int H, int W, const E* __restrict__ Bw,
                                                         long b_phase, long ldb, int Nout, const float* __restrict__ bias,
                                                         E* __restrict__ out, int HO, int WO, long ldo, int o, UcTaps tp) {
  constexpr int BM = 128, BN = 128, RSTEP = 32, ACH = BM / RSTEP, BCH = BN / RSTEP;
  __shared__ __attribute__((aligned(16))) E lds[2 * (BM + BN) * UC_BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int p = blockIdx.y;
  const int ntn = (Nout + BN - 1) / BN;
  const long m0 = (long)(blockIdx.x / ntn) * BM;
  const int n0 = (int)(blockIdx.x % ntn) * BN;
  const long M = (long)B * H * W;
  const int K = tp.G[p] * Cg;
  const E* Bp = Bw + (long)p * b_phase;
  const short* gdy = tp.dy + tp.g0[p];
  const short* gdx = tp.dx + tp.g0[p];

  const int cc = tid & 7, sr = tid >> 3;
  int a_b[ACH], a_i[ACH], a_j[ACH];
#pragma unroll
  for (int t = 0; t < ACH; ++t) {
    const long m = m0 + sr + RSTEP * t;
    const long mm = m < M ? m : 0;
    a_b[t] = m < M ? (int)(mm / ((long)H * W)) : -1;
    const int rem = (int)(mm - (long)(a_b[t] < 0 ? 0 : a_b[t]) * H * W);
    a_i[t] = rem / W;
    a_j[t] = rem - a_i[t] * W;
  }
  int kcur = cc * 8, grp = 0, c_in = kcur;
  while (c_in >= Cg) { c_in -= Cg; ++grp; }

  E8 ra[ACH], rb[BCH];
  auto load_tile = [&]() {
    const bool k_ok = kcur < K;
    const int ddy = k_ok ? gdy[grp] : 0, ddx = k_ok ? gdx[grp] : 0;
#pragma unroll
    for (int t = 0; t < ACH; ++t) {
      E8 v = {};
      const int sy = a * a_i[t] + ddy, sx = a * a_j[t] + ddx;
      if (k_ok && a_b[t] >= 0 && (unsigned)sy < (unsigned)HS && (unsigned)sx < (unsigned)WS)
        v = *reinterpret_cast<const E8*>(src + (((long)a_b[t] * HS + sy) * WS + sx) * lds_src + c_in);
      ra[t] = v;
    }
#pragma unroll
    for (int t = 0; t < BCH; ++t) {
      E8 v = {};
      const int n = n0 + sr + RSTEP * t;
      if (k_ok && n < Nout) v = *reinterpret_cast<const E8*>(Bp + (long)n * ldb + kcur);
      rb[t] = v;
    }
    kcur += UC_BK;
    c_in += UC_BK;
    while (c_in >= Cg) { c_in -= Cg; ++grp; }
  };
  auto store_tile = [&](int buf) {
    E* As = lds + buf * (BM + BN) * UC_BK;
    E* Bs = As + BM * UC_BK;
#pragma unroll
    for (int t = 0; t < ACH; ++t) *reinterpret_cast<E8*>(As + uc_swz(sr + RSTEP * t, cc)) = ra[t];
#pragma unroll
    for (int t = 0; t < BCH; ++t) *reinterpret_cast<E8*>(Bs + uc_swz(sr + RSTEP * t, cc)) = rb[t];
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (K + UC_BK - 1) / UC_BK;
  load_tile();
  store_tile(0);
  if (nk > 1) load_tile();
  __syncthreads();
  const int frow = lane & 15, fchunk = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const E* As = lds + buf * (BM + BN) * UC_BK;
    const E* Bs = As + BM * UC_BK;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      E8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const E8*>(As + uc_swz(wm * 64 + i * 16 + frow, s * 4 + fchunk));
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const E8*>(Bs + uc_swz(wn * 64 + j * 16 + frow, s * 4 + fchunk));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = uc_mfma<E8>(fb[j], fa[i], acc[i][j]);
      if (s == 0 && kt + 1 < nk) {
        store_tile(buf ^ 1);
        if (kt + 2 < nk) load_tile();
      }
    }
    __syncthreads();
  }

  // epilogue: row m -> output pixel (o i + r, o j + s); 4 consecutive columns per lane
  const int pr = tp.r[p], ps = tp.s[p];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long m = m0 + wm * 64 + i * 16 + frow;
    if (m >= M) continue;
    const int b = (int)(m / ((long)H * W));
    const int rem = (int)(m - (long)b * H * W);
    const int ii = rem / W, jj = rem - ii * W;
    E* orow = out + (((long)b * HO + o * ii + pr) * WO + o * jj + ps) * ldo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fchunk * 4;
      if (n >= Nout) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (bias) {
        const float4 bb = *reinterpret_cast<const float4*>(bias + n);
        v[0] += bb.x; v[1] += bb.y; v[2] += bb.z; v[3] += bb.w;
      }
      store4(orow + n, v);
    }
  }
}

// Folded weights from W (N, C, 5, 5) fp32, sums in fp32.  mode 0: Bf[p][n][(ty * Gs + tx) * Cp + c], row pitch Gmax * Cp
// (Np rows per phase); mode 1 (input gradient): Bt[c][g * Np + n] with g running over (phase, ty, tx) in phase order.
// Zero wherever n >= N or c >= C and behind a phase's own taps.
template <typename T>
__global__ void upconv5_fold_kernel(const float* __restrict__ w, T* __restrict__ out, int N, int C, int Np, int Cp, int f,
                                    int mode, long total, UcTaps tp) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int p, n, c, t;
  if (mode == 0) {
    const int gm = f == 3 ? 9 : 4;
    const long row = idx / ((long)gm * Cp);
    const int k = (int)(idx - row * gm * Cp);
    p = (int)(row / Np);
    n = (int)(row - (long)p * Np);
    t = k / Cp;
    c = k - t * Cp;
    if (t >= tp.G[p]) {
      out[idx] = (T)0.f;
      return;
    }
  } else {
    const long KT = total / Cp;
    c = (int)(idx / KT);
    const int k = (int)(idx - (long)c * KT);
    const int g = k / Np;
    n = k - g * Np;
    p = 0;
    while (p + 1 < f * f && tp.g0[p + 1] <= g) ++p;
    t = g - tp.g0[p];
  }
  float s = 0.f;
  if (n < N && c < C) {
    const int r = tp.r[p], q = tp.s[p];
    const int gs = uc_ntaps(q, f);
    const int ty = t / gs, tx = t - ty * gs;
    const float* wp = w + ((long)n * C + c) * 25;
    for (int ky = 0; ky < 5; ++ky) {
      if (uc_row(r, ky, f) - uc_lo(r, f) != ty) continue;
      for (int kx = 0; kx < 5; ++kx)
        if (uc_row(q, kx, f) - uc_lo(q, f) == tx) s += wp[ky * 5 + kx];
    }
  }
  out[idx] = (T)s;
}

// compact[b][y][x] = dy(b, f (y - ey) + r, f (x - ex) + s) on a (H + 1) x (W + 1) grid, zero outside the phase lattice
// (ey / ex = 1 where the phase's first folded tap reads offset 0: the weight-gradient GEMM then sees offsets -1 .. with
// pad 1 on both axes)
template <typename T>
__global__ void upconv5_gather_phase_kernel(const T* __restrict__ dy, long lddy, T* __restrict__ out, int B, int H, int W,
                                            int f, int r, int s, int ey, int ex, int Np) {
  const int nv = Np >> 3;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * (H + 1) * (W + 1) * nv;
  if (idx >= total) return;
  const int v = (int)(idx % nv);
  const long pix = idx / nv;
  const int x = (int)(pix % (W + 1));
  const long by = pix / (W + 1);
  const int y = (int)(by % (H + 1));
  const int b = (int)(by / (H + 1));
  const int i = y - ey, j = x - ex;
  Raw8<T> val;
  val.zero();
  if ((unsigned)i < (unsigned)H && (unsigned)j < (unsigned)W)
    val.load(dy + (((long)b * f * H + (long)f * i + r) * ((long)f * W) + (long)f * j + s) * lddy + v * 8);
  float t[8];
  val.unpack(t);
  store8(out + pix * Np + v * 8, t);
}

// dW[n][c][ky][kx] (+)= sum over phases of dW'[p][n][(tap(r, ky) * Gs + tap(s, kx)) * Cp + c]; phase p's (Np, G_p * Cp)
// block starts at p * Np * Gmax * Cp
__global__ void upconv5_unfold_kernel(const float* __restrict__ gwf, float* __restrict__ dw, int N, int C, int Np, int Cp,
                                      int f, int accumulate) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * C * 25) return;
  const int kk = (int)(idx % 25);
  const long nc = idx / 25;
  const int c = (int)(nc % C), n = (int)(nc / C);
  const int ky = kk / 5, kx = kk - ky * 5;
  const int gm = f == 3 ? 9 : 4;
  float s = 0.f;
  for (int r = 0; r < f; ++r)
    for (int q = 0; q < f; ++q) {
      const int ty = uc_row(r, ky, f) - uc_lo(r, f), tx = uc_row(q, kx, f) - uc_lo(q, f);
      const int p = r * f + q;
      const int gs = uc_ntaps(q, f), G = uc_ntaps(r, f) * gs;
      s += gwf[(long)p * Np * gm * Cp + ((long)n * G + ty * gs + tx) * Cp + c];
    }
  dw[idx] = accumulate ? dw[idx] + s : s;
}

// Groups in phase order, phase p = (r, s) = (p / f, p % f) owning entries g0[p] .. g0[p] + G[p] - 1, one per folded tap
// (ty, tx).  Forward (a = 1): low-res offsets (lo(r) + ty, lo(s) + tx).  Input gradient (a = f): dy offsets
// (r - f (lo(r) + ty), s - f (lo(s) + tx)) from (f i, f j); dgrad = true also makes it ONE launch phase holding every group.
UcTaps uc_taps(int f, bool dgrad) {
  UcTaps t = {};
  int g = 0;
  for (int r = 0; r < f; ++r)
    for (int q = 0; q < f; ++q) {
      const int p = r * f + q;
      const int gr = uc_ntaps(r, f), gs = uc_ntaps(q, f);
      t.G[p] = gr * gs;
      t.r[p] = r;
      t.s[p] = q;
      t.g0[p] = g;
      for (int ty = 0; ty < gr; ++ty)
        for (int tx = 0; tx < gs; ++tx, ++g) {
          const int oy = uc_lo(r, f) + ty, ox = uc_lo(q, f) + tx;
          t.dy[g] = (short)(dgrad ? r - f * oy : oy);
          t.dx[g] = (short)(dgrad ? q - f * ox : ox);
        }
    }
  if (dgrad) {
    t.G[0] = g;
    t.r[0] = t.s[0] = t.g0[0] = 0;
  }
  return t;
}

int uc_check(const char* who, const void* x, const vkas_conv_geom* g, int f, int Np, int dtype) {
  VKAS_CHECK(g && x, "%s: null input", who);
  VKAS_CHECK(f == 3 || f == 4, "%s: upsampling factor %d (3 or 4 only)", who, f);
  VKAS_CHECK(dtype == VKAS_BF16 || dtype == VKAS_F16, "%s: 16-bit storage only (dtype %d)", who, dtype);
  VKAS_CHECK(g->B > 0 && g->Hin > 0 && g->Win > 0 && g->Hout == f * g->Hin && g->Wout == f * g->Win,
             "%s: output %dx%d must be %d x the input %dx%d", who, g->Hout, g->Wout, f, g->Hin, g->Win);
  VKAS_CHECK(g->KH == 5 && g->KW == 5 && g->stride == 1 && g->pad == 2, "%s: a 5x5 / stride 1 / pad 2 geometry only", who);
  VKAS_CHECK(g->Cp > 0 && g->Cp % 8 == 0, "%s: Cp=%d must be a positive multiple of 8", who, g->Cp);
  VKAS_CHECK(g->ldx >= g->Cp && g->ldx % 8 == 0, "%s: ldx=%d must be >= Cp and a multiple of 8", who, g->ldx);
  VKAS_CHECK(Np > 0 && Np % 8 == 0, "%s: Np=%d must be a positive multiple of 8", who, Np);
  VKAS_CHECK(vkas_aligned16(x), "%s: x not 16-byte aligned", who);
  VKAS_CHECK((long)g->B * g->Hout * g->Wout < (1L << 31) && (long)g->B * g->Hin * g->Win * g->ldx < (1L << 40),
             "%s: tensor too large", who);
  return VKAS_OK;
}

template <typename E, typename E8>
void uc_launch_nt(const void* src, int B, int HS, int WS, long lds_src, int a, int Cg, int H, int W, const void* Bw,
                  long b_phase, long ldb, int Nout, const float* bias, void* out, int HO, int WO, long ldo, int o,
                  const UcTaps& tp, int phases, hipStream_t st) {
  const long M = (long)B * H * W;
  dim3 grid((unsigned)(vkas_cdiv(M, 128) * vkas_cdiv(Nout, 128)), (unsigned)phases);
  upconv5_nt_kernel<E, E8><<<grid, 256, 0, st>>>((const E*)src, B, HS, WS, lds_src, a, Cg, H, W, (const E*)Bw, b_phase, ldb,
                                                 Nout, bias, (E*)out, HO, WO, ldo, o, tp);
}

}  // namespace

extern "C" size_t vkas_upconv5_fold_elems(int Np, int Cp, int f, int transposed) {
  if ((f != 3 && f != 4) || Np <= 0 || Cp <= 0) return 0;
  return transposed ? (size_t)Cp * (f == 3 ? 49 : 64) * Np : (size_t)f * f * Np * uc_gmax(f) * Cp;
}

extern "C" int vkas_upconv5_fold(const float* w, void* out, int N, int C, int Np, int Cp, int f, int transposed, int dtype,
                                 void* stream) {
  VKAS_CHECK(w && out, "vkas_upconv5_fold: null pointer");
  VKAS_CHECK(f == 3 || f == 4, "vkas_upconv5_fold: upsampling factor %d (3 or 4 only)", f);
  VKAS_CHECK(N > 0 && C > 0 && Np % 8 == 0 && Cp % 8 == 0 && Np >= N && Cp >= C,
             "vkas_upconv5_fold: bad sizes N=%d C=%d Np=%d Cp=%d", N, C, Np, Cp);
  VKAS_CHECK(vkas_aligned16(out), "vkas_upconv5_fold: out not 16-byte aligned");
  const long total = (long)vkas_upconv5_fold_elems(Np, Cp, f, transposed);
  const UcTaps tf = uc_taps(f, false);  // per-phase tap counts and the first group of each phase
  const unsigned blocks = (unsigned)vkas_cdiv(total, 256);
  if (dtype == VKAS_BF16)
    upconv5_fold_kernel<bf16_t><<<blocks, 256, 0, vkas_stream(stream)>>>(w, (bf16_t*)out, N, C, Np, Cp, f, transposed, total, tf);
  else if (dtype == VKAS_F16)
    upconv5_fold_kernel<f16_t><<<blocks, 256, 0, vkas_stream(stream)>>>(w, (f16_t*)out, N, C, Np, Cp, f, transposed, total, tf);
  else
    VKAS_CHECK(false, "vkas_upconv5_fold: 16-bit storage only (dtype %d)", dtype);
  VKAS_LAUNCH_CHECK("upconv5_fold");
  return VKAS_OK;
}

extern "C" int vkas_upconv5_fwd(const void* x, const vkas_conv_geom* g, int f, const void* Bf, int Np, const float* bias,
                                void* out, long ldo, int dtype, void* stream) {
  int rc = uc_check("vkas_upconv5_fwd", x, g, f, Np, dtype);
  if (rc) return rc;
  VKAS_CHECK(Bf && vkas_aligned16(Bf), "vkas_upconv5_fwd: folded weights null/misaligned");
  VKAS_CHECK(out && vkas_aligned16(out) && ldo >= Np && ldo % 8 == 0, "vkas_upconv5_fwd: bad out (ldo=%ld)", ldo);
  VKAS_CHECK(!bias || vkas_aligned16(bias), "vkas_upconv5_fwd: bias must be 16-byte aligned");
  const UcTaps tp = uc_taps(f, false);
  const long kmax = (long)uc_gmax(f) * g->Cp;
  if (dtype == VKAS_BF16)
    uc_launch_nt<bf16_t, bf16x8>(x, g->B, g->Hin, g->Win, g->ldx, 1, g->Cp, g->Hin, g->Win, Bf, (long)Np * kmax, kmax, Np, bias,
                                 out, g->Hout, g->Wout, ldo, f, tp, f * f, vkas_stream(stream));
  else
    uc_launch_nt<f16_t, f16x8>(x, g->B, g->Hin, g->Win, g->ldx, 1, g->Cp, g->Hin, g->Win, Bf, (long)Np * kmax, kmax, Np, bias,
                               out, g->Hout, g->Wout, ldo, f, tp, f * f, vkas_stream(stream));
  VKAS_LAUNCH_CHECK("upconv5_fwd");
  return VKAS_OK;
}

extern "C" int vkas_upconv5_dgrad(const void* dy, long lddy, const vkas_conv_geom* g, int f, const void* Bt, int Np,
                                  void* dx, long lddx, int dtype, void* stream) {
  int rc = uc_check("vkas_upconv5_dgrad", dx, g, f, Np, dtype);
  if (rc) return rc;
  VKAS_CHECK(dy && vkas_aligned16(dy) && lddy >= Np && lddy % 8 == 0, "vkas_upconv5_dgrad: bad dy (lddy=%ld)", lddy);
  VKAS_CHECK(Bt && vkas_aligned16(Bt), "vkas_upconv5_dgrad: folded weights null/misaligned");
  VKAS_CHECK(lddx >= g->Cp && lddx % 8 == 0, "vkas_upconv5_dgrad: bad lddx=%ld", lddx);
  const UcTaps tp = uc_taps(f, true);
  const long K = (long)tp.G[0] * Np;
  if (dtype == VKAS_BF16)
    uc_launch_nt<bf16_t, bf16x8>(dy, g->B, g->Hout, g->Wout, lddy, f, Np, g->Hin, g->Win, Bt, 0, K, g->Cp, nullptr, dx, g->Hin,
                                 g->Win, lddx, 1, tp, 1, vkas_stream(stream));
  else
    uc_launch_nt<f16_t, f16x8>(dy, g->B, g->Hout, g->Wout, lddy, f, Np, g->Hin, g->Win, Bt, 0, K, g->Cp, nullptr, dx, g->Hin,
                               g->Win, lddx, 1, tp, 1, vkas_stream(stream));
  VKAS_LAUNCH_CHECK("upconv5_dgrad");
  return VKAS_OK;
}

extern "C" size_t vkas_upconv5_wgrad_ws_bytes(int B, int H, int W, int Np) {
  if (B <= 0 || H <= 0 || W <= 0 || Np <= 0) return 0;
  return (size_t)B * (H + 1) * (W + 1) * Np * 2;
}

extern "C" int vkas_upconv5_wgrad(const void* x, const vkas_conv_geom* g, int f, const void* dy, long lddy, int Np, void* ws,
                                  size_t ws_bytes, float* gwf, float* gb, int dtype, void* stream) {
  int rc = uc_check("vkas_upconv5_wgrad", x, g, f, Np, dtype);
  if (rc) return rc;
  VKAS_CHECK(dy && vkas_aligned16(dy) && lddy >= Np && lddy % 8 == 0, "vkas_upconv5_wgrad: bad dy (lddy=%ld)", lddy);
  VKAS_CHECK(gwf && (!gb || vkas_aligned16(gb)), "vkas_upconv5_wgrad: null gw / misaligned gb");
  VKAS_CHECK(ws && vkas_aligned16(ws) && ws_bytes >= vkas_upconv5_wgrad_ws_bytes(g->B, g->Hin, g->Win, Np),
             "vkas_upconv5_wgrad: workspace too small");
  const hipStream_t st = vkas_stream(stream);
  const int H = g->Hin, W = g->Win, gm = uc_gmax(f);
  const long total = (long)g->B * (H + 1) * (W + 1) * (Np / 8);
  for (int r = 0; r < f; ++r)
    for (int q = 0; q < f; ++q) {
      const int p = r * f + q;
      const int ey = uc_lo(r, f) == 0 ? 1 : 0, ex = uc_lo(q, f) == 0 ? 1 : 0;
      if (dtype == VKAS_BF16)
        upconv5_gather_phase_kernel<bf16_t><<<(unsigned)vkas_cdiv(total, 256), 256, 0, st>>>(
            (const bf16_t*)dy, lddy, (bf16_t*)ws, g->B, H, W, f, r, q, ey, ex, Np);
      else
        upconv5_gather_phase_kernel<f16_t><<<(unsigned)vkas_cdiv(total, 256), 256, 0, st>>>(
            (const f16_t*)dy, lddy, (f16_t*)ws, g->B, H, W, f, r, q, ey, ex, Np);
      VKAS_LAUNCH_CHECK("upconv5_gather_phase");
      // compact row y = i + ey reads low-res rows y - 1 + ty = i + lo(r) + ty
      vkas_conv_geom pg = {g->B, H, W, H + 1, W + 1, g->Cp, g->ldx, uc_ntaps(r, f), uc_ntaps(q, f), 1, 1};
      float* gw_p = gwf + (long)p * Np * gm * g->Cp;
      // phase p's (Np, G_p * Cp) weight gradient: its own block of Np * Gmax * Cp floats
      rc = dtype == VKAS_BF16 ? vkas_gemm_tn_mfma_bf16(x, &pg, ws, Np, Np, gw_p, gb, 0, st)
                              : vkas_gemm_tn_mfma_f16(x, &pg, ws, Np, Np, gw_p, gb, 0, st);
      if (rc) return rc;
    }
  return VKAS_OK;
}

extern "C" int vkas_upconv5_unfold_wgrad(const float* gwf, float* dw, int N, int C, int Np, int Cp, int f, int accumulate,
                                         void* stream) {
  VKAS_CHECK(gwf && dw, "vkas_upconv5_unfold_wgrad: null pointer");
  VKAS_CHECK(f == 3 || f == 4, "vkas_upconv5_unfold_wgrad: upsampling factor %d (3 or 4 only)", f);
  VKAS_CHECK(N > 0 && C > 0 && Np % 8 == 0 && Cp % 8 == 0 && Np >= N && Cp >= C,
             "vkas_upconv5_unfold_wgrad: bad sizes N=%d C=%d Np=%d Cp=%d", N, C, Np, Cp);
  upconv5_unfold_kernel<<<(unsigned)vkas_cdiv((long)N * C * 25, 256), 256, 0, vkas_stream(stream)>>>(gwf, dw, N, C, Np, Cp, f,
                                                                                                      accumulate);
  VKAS_LAUNCH_CHECK("upconv5_unfold");
  return VKAS_OK;
}
