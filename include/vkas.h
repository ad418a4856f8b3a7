/*
 * vkas.h — C ABI of libvkas.so: the MI355X (gfx950) kernels behind the adaptive-scaling
 * text-detection forward/backward path.
 *
 * The reference (vkit_open_model, pure PyTorch) has no FFI boundary of its own; its boundary for
 * this path is the nn.Module / loss-callable API.  Each entry point below replaces
 * the ATen op(s) that a reference call site dispatches to; the file:line given is that call site
 * (paths relative to /root/reference/vkit_open_model/).  The Python host layer
 * (vkit_ocr_model_adaptive_scaling_amd/) binds these through ctypes and mirrors the reference's
 * module API on top.  Nothing here depends on torch: plain pointers, sizes, a HIP stream.
 *
 * Conventions
 *  - every function returns 0 on success, a negative VKAS_E_* code otherwise (never aborts);
 *    vkas_last_error() returns a thread-local message for the last failure.
 *  - `dtype` selects the storage type of activations: VKAS_F32, VKAS_BF16 or VKAS_F16.  Accumulation is
 *    always fp32.  Parameters handed over in the reference's layout are always fp32.
 *  - activations are NHWC: element (b, y, x, c) of a tensor with pixel stride `ld` (elements) lives
 *    at base[((b*H + y)*W + x)*ld + c].  `ld >= C`, `ld % 8 == 0`, bases 16-byte aligned; a channel
 *    slice of a wider tensor is expressed by offsetting the base and keeping the wide `ld`
 *    (this is how torch.cat along C, upernext.py:82,197 / fpn.py:144, disappears).
 *  - logical channel counts are padded to a multiple of 8 (`Cp`); pad channels hold zeros.
 *  - all kernels are enqueued on `stream` (a hipStream_t passed as void*); no call synchronises,
 *    allocates or frees device memory.  Workspaces are caller-provided.
 */
#ifndef VKAS_H
#define VKAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VKAS_F32 0
#define VKAS_BF16 1
#define VKAS_F16 2 /* IEEE half storage, fp32 accumulate: BASELINE.json configs[4] (fp16 inference of the Base model) */

#define VKAS_OK 0
#define VKAS_E_ARG (-1)     /* bad shape / alignment / dtype */
#define VKAS_E_LAUNCH (-2)  /* hipGetLastError() != hipSuccess after a launch */

/* GEMM epilogues (vkas_conv_gemm_fwd) */
#define VKAS_EPI_NONE 0       /* out = acc + bias */
#define VKAS_EPI_GELU 1       /* out = acc + bias (pre-activation; NULL = not kept), out2 = gelu(out)  helper.py:100 */
#define VKAS_EPI_SCALE_RES 2  /* out2 = acc + bias; out = aux + rowscale[b]*colscale[n]*out2  convnext.py:56-58 */
#define VKAS_EPI_DGELU 3      /* out = (acc) * gelu'(aux)                                     backward of helper.py:100 */
#define VKAS_EPI_ADD 4        /* out = acc + bias + aux                                       gradient accumulation */
#define VKAS_EPI_PATCH 5      /* out scattered to non-overlapping kxk patches: dgrad of helper.py:43-58 */
#define VKAS_EPI_HEAD 6       /* fused head tail: out = z = acc + bias (pre-LN, kept for backward); per pixel
                               * LayerNorm -> GELU -> Linear(C -> 1..4) in the epilogue; the (M, C) activation never
                               * reaches HBM.  upernext.py:215-223 / fpn.py:165-183.  16-bit MFMA kernels only.  out = NULL
                               * together with head.stats = NULL: inference, z and the row statistics are not stored. */

const char* vkas_last_error(void);
int vkas_abi_version(void);

/* Geometry of a convolution seen as an implicit GEMM: M = B*Hout*Wout rows, K = KH*KW*Cp columns.
 * 1x1 / nn.Linear is KH=KW=1, stride 1, pad 0 (helper.py:18-22); 3x3 is pad 1 (helper.py:25-31);
 * the patchify convs are KH=KW=stride, pad 0 (helper.py:43-58). */
typedef struct vkas_conv_geom {
  int B, Hin, Win, Hout, Wout;
  int Cp;      /* input channels per tap, padded to a multiple of 8 */
  int ldx;     /* input pixel stride in elements */
  int KH, KW, stride, pad;
} vkas_conv_geom;

/* VKAS_EPI_HEAD: the N tiles of the launch are the heads (all reading the same input).  Head h owns output columns
 * [n0[h], n0[h] + np[h]) (np = rup8(c)), of which c are real; params + h*(6*pw+8) holds, as floats,
 * gamma[pw] | beta[pw] | Wproj[4][pw] | bproj[4] | pad[4] (zero padded; vkas_pack_head_params).
 * stats: (n_heads, M, 2) fp32 (mean, rstd); proj: (n_heads, M, 8) fp32, columns >= oc are zero. */
typedef struct vkas_head_desc {
  int n_heads, pw;
  int n0[4], np[4], c[4], oc[4];
  const float* params;
  float* stats;
  float* proj;
} vkas_head_desc;

typedef struct vkas_epilogue {
  int mode;               /* VKAS_EPI_* */
  const float* bias;      /* [Np] or NULL */
  void* out;  long ldo;   /* primary output, row stride (elements) */
  void* out2; long ldo2;  /* secondary output (GELU, SCALE_RES) or NULL */
  const void* aux; long ldaux; /* residual / saved pre-activation, same dtype as out */
  const float* colscale;  /* [Np]   SCALE_RES: block_scale */
  const float* rowscale;  /* [B] or NULL  SCALE_RES: stochastic-depth keep mask / keep prob */
  int rows_per_image;     /* Hout*Wout, to index rowscale */
  int patch;              /* PATCH: patch edge k; rows are the (B,Hs,Ws) grid, columns (ky,kx,c) */
  int patch_Hs, patch_Ws, patch_Cp;
  vkas_head_desc head;    /* HEAD */
} vkas_epilogue;

/* ---- parameter layout conversion (reference layouts -> kernel layouts and back) ------------------ */
/* w (N,C,KH,KW) fp32 [nn.Conv2d / nn.Linear weight] -> out (Np, KH, KW, Cp) in `dtype`, zero padded.
 * mode 0: forward operand.  mode 1: dgrad operand of a stride-1 conv: out (Cp_as_rows..) = W flipped and
 * in/out swapped: out[c][KH-1-ky][KW-1-kx][n] = w[n][c][ky][kx]  (rows = Cp(C), columns (ky,kx,Np)).
 * mode 2: dgrad operand of a patchify conv: out[(ky,kx,c)][n] = w[n][c][ky][kx] (rows KH*KW*Cp, cols Np). */
int vkas_pack_conv_weight(const float* w, void* out, int N, int C, int KH, int KW, int Np, int Cp, int mode,
                          int dtype, void* stream);
/* the same for one of several convolutions that share their input and are packed side by side (the heads of a pass,
 * adaptive_scaling.py:150-152,163-170): fills output channels [n_off, n_off + Np) of an operand with Nt output channels
 * in total; mode 0 (forward), 1 (dgrad) or 3: the rows image (KH, Nt, KW, Cp) - per kernel row ky a 1 x KW convolution whose
 * output channel ky * Nt + n is kernel row ky of output channel n (the operand of the heads' forward at the neck's height,
 * vkas_head_rows_fwd). */
int vkas_pack_conv_weight_slice(const float* w, void* out, int N, int C, int KH, int KW, int Np, int Cp, int mode,
                                int n_off, int Nt, int dtype, void* stream);
/* gw (Np, KH, KW, Cp) fp32 [wgrad output] -> grad (N,C,KH,KW) fp32, grad += (accumulate != 0) or = */
int vkas_unpack_conv_wgrad(const float* gw, float* grad, int N, int C, int KH, int KW, int Np, int Cp,
                           int accumulate, void* stream);
/* dst[k][0..n[k]) += src[k][0..n[k]) for count <= 16 fp32 vectors in one launch: the small per-parameter gradients of a
 * layer (bias, LayerNorm affine, block_scale; what autograd's AccumulateGrad does one launch per tensor) */
int vkas_accumulate_many(int count, const float* const* src, float* const* dst, const int* n, void* stream);
/* Up to 8 second-stage column sums in one launch: out[k][c] (+)= sum over the P[k] partial rows (row pitch ldp[k]) of column c <
   n[k].  vkas_layernorm_bwd / vkas_scale_res_bwd / vkas_dwconv7x7_wgrad called with NULL gradient outputs leave their
   per-workgroup partial rows in the workspace (vkas_*_parts() rows); the backward of a ConvNeXt layer (convnext.py:29-59) then
   sums all of them - straight into the parameters' gradient views - with this one launch.  Fixed order: deterministic. */
int vkas_finalize_many(int count, const float* const* partial, const long* P, const int* n, const int* ldp,
                       float* const* out, const int* accumulate, void* stream);
long vkas_layernorm_bwd_parts(long M, int Cp);
long vkas_scale_res_bwd_parts(long M, int Cp);
long vkas_dwconv7x7_wgrad_parts(int B, int H, int W, int Cp, int dtype);
/* v (n) fp32 -> out (np) fp32 zero padded (bias, LayerNorm affine, block_scale) */
int vkas_pad_vector(const float* v, float* out, int n, int np, void* stream);
/* depthwise weight (C,1,7,7) fp32 -> vkas_dw_weight_elems(Cp) fp32: (49, Cp) taps x channels followed by the same values
 * as (Cp/2, 7, 16) channel-pair kernel rows (scalar-load operand of the bf16 kernel); flip != 0 rotates the taps by 180
 * degrees (dgrad operand) */
size_t vkas_dw_weight_elems(int Cp);
int vkas_pack_dw_weight(const float* w, float* out, int C, int Cp, int flip, void* stream);
/* gw (49, Cp) fp32 -> grad (C,1,7,7) fp32 (+=) */
int vkas_unpack_dw_wgrad(const float* gw, float* grad, int C, int Cp, int accumulate, void* stream);
/* image (B,3,H,W) fp32 NCHW [dataset/adaptive_scaling.py:296] -> (B,H,W,8) `dtype`, channels 3..7 zero */
int vkas_image_nchw_to_nhwc8(const float* img, void* out, int B, int C, int H, int W, int dtype, void* stream);
/* small head outputs: (B,H,W,ld) `dtype` -> (B,C,H,W) fp32 and the reverse (gradient) direction */
int vkas_nhwc_to_nchw_f32(const void* x, long ld, float* out, int B, int H, int W, int C, int dtype, void* stream);
int vkas_nchw_f32_to_nhwc(const float* g, void* out, long ld, int B, int H, int W, int C, int Cp, int dtype, void* stream);

/* ---- implicit-GEMM convolution: helper.py:18-58 (conv1x1 / conv3x3 / pconv2x2 / pconv4x4) -------- */
/* D[m][n] = epilogue( sum_k A(m,k) * Bw[n][k] ), A gathered from x by `g`; Bw (Np, K) packed `dtype`. */
int vkas_conv_gemm_fwd(const void* x, const vkas_conv_geom* g, const void* Bw, int Np, const vkas_epilogue* epi,
                       int dtype, void* stream);
/* wgrad: gw[n][k] += sum_m dy[m][n] * A(m,k), gw (Np, K) fp32; optional fused bias gradient gb[n] += sum_m dy[m][n]
 * (gb (Np) fp32 or NULL).  gw and gb must be zero-filled by the caller: the kernel adds split-M partials with
 * fp32 atomics. */
int vkas_conv_gemm_wgrad(const void* x, const vkas_conv_geom* g, const void* dy, long lddy, int Np, float* gw,
                         float* gb, int dtype, void* stream);
/* the same without the split over M (no bias gradient): every gw tile is summed over all rows by one workgroup, in row
 * order, and added once to the zero-filled gw, so the fp32 result does not depend on the order workgroups run in.  For
 * the one use whose result is rounded into a 16-bit activation gradient afterwards (the input gradient of the heads the
 * loss reads at label points, loss_function/adaptive_scaling.py:235-262 -> upernext.py:215-223): there the last-bit
 * spread of atomically added partials flips 16-bit roundings from run to run and the backbone's backward amplifies it. */
int vkas_conv_gemm_wgrad_ordered(const void* x, const vkas_conv_geom* g, const void* dy, long lddy, int Np, float* gw,
                                 int dtype, void* stream);
/* the same with A(m,k) = gelu(x(m,k)): weight gradient of the second MLP Linear when the forward kept only the
 * pre-activation h (vkas_mlp_chain_fwd): backward of convnext.py:34-35 */
int vkas_conv_gemm_wgrad_gelu(const void* x, const vkas_conv_geom* g, const void* dy, long lddy, int Np, float* gw,
                              float* gb, int dtype, void* stream);

/* ---- nearest x f upsample followed by a 5x5 / pad 2 convolution, f in {3, 4} (FpnHead smoothing, fpn.py:41-48,170-174) -----
 * Never materialises the upsample: each output phase (r, s) = pixels (f i + r, f j + s) is a 2 x 2 (f = 4) or up to 3 x 3
 * (f = 3) convolution over the low-res input with folded taps (sums of the 5x5 taps).  16-bit storage only.
 * g: B, Hin, Win = the low-res input, Hout = f Hin, Wout = f Win, Cp, ldx, KH = KW = 5, stride 1, pad 2.
 * fold: w (N, C, 5, 5) fp32 -> `dtype` image of vkas_upconv5_fold_elems(Np, Cp, f, transposed) elements, sums in fp32.
 * transposed = 0: the forward operand, per phase (Np, Gmax * Cp) rows in the (tap, Cp) layout of the implicit GEMMs;
 * transposed = 1: the input-gradient operand (Cp, G * Np), one column block per (phase, tap). */
size_t vkas_upconv5_fold_elems(int Np, int Cp, int f, int transposed);
int vkas_upconv5_fold(const float* w, void* out, int N, int C, int Np, int Cp, int f, int transposed, int dtype, void* stream);
/* out (B, Hout, Wout, Np) pixel stride ldo = conv5x5(nearest_up(x)) + bias (Np fp32, or NULL) */
int vkas_upconv5_fwd(const void* x, const vkas_conv_geom* g, int f, const void* Bf, int Np, const float* bias, void* out,
                     long ldo, int dtype, void* stream);
/* dx (B, Hin, Win, Cp) pixel stride lddx = the input gradient for dy (B, Hout, Wout, Np) pixel stride lddy; every phase
 * is summed in registers (no atomics: deterministic) */
int vkas_upconv5_dgrad(const void* dy, long lddy, const vkas_conv_geom* g, int f, const void* Bt, int Np, void* dx, long lddx,
                       int dtype, void* stream);
/* per-phase folded weight gradient gwf (f*f blocks of Np * Gmax * Cp fp32, zero-filled by the caller) and the bias
 * gradient gb (Np fp32, zero-filled, or NULL); both are added with fp32 atomics.  ws: vkas_upconv5_wgrad_ws_bytes bytes
 * (the dy of one phase, compacted). */
size_t vkas_upconv5_wgrad_ws_bytes(int B, int H, int W, int Np);
int vkas_upconv5_wgrad(const void* x, const vkas_conv_geom* g, int f, const void* dy, long lddy, int Np, void* ws,
                       size_t ws_bytes, float* gwf, float* gb, int dtype, void* stream);
/* dw (N, C, 5, 5) fp32 (+)= the phases of gwf summed back onto the 5x5 taps */
int vkas_upconv5_unfold_wgrad(const float* gwf, float* dw, int N, int C, int Np, int Cp, int f, int accumulate, void* stream);

/* ---- fused ConvNeXt MLP (convnext.py:33-35,54-58), C % 8 == 0, C <= 512, 16-bit storage --------------------------------------
 * Linear(C,4C) -> GELU -> Linear(4C,C) -> layer scale -> stochastic depth -> residual as one kernel per direction; the
 * (M, 4C) activation is written once (h, for backward) and never read back between the two matrix products.
 * Weights are consumed as a packed, pre-swizzled LDS image: vkas_mlp_chain_image_elems(C) elements of `dtype`, built by
 * vkas_mlp_chain_pack from w1 (4C, C) / w2 (C, 4C) fp32 in the reference layout; mode 0 = forward image, 1 = backward
 * image (transposed roles; b1 may be NULL).  image_elems returns 0 when C is not covered. */
size_t vkas_mlp_chain_image_elems(int C);
int vkas_mlp_chain_pack(const float* w1, const float* w2, const float* b1, int C, int mode, void* img, int dtype,
                        void* stream);
/* h = yn W1^T + b1 (stored; b1 (4C) travels inside the forward image); z = gelu(h) W2^T + b2 (stored);
 * out = x + rowscale[m / rows_per_image] * colscale * z.  b2 (C), colscale (C) fp32; rowscale (images) fp32 or NULL.
 * h = z = NULL: inference (no-grad) call, nothing is stored for a backward pass. */
int vkas_mlp_chain_fwd(const void* yn, long ldyn, const void* img, const float* b2, const void* x, long ldx,
                       const float* colscale, const float* rowscale, int rows_per_image, void* h, long ldh, void* z,
                       long ldz, void* out, long ldo, long M, int C, int dtype, void* stream);
/* the same with the LayerNorm in front of the MLP (convnext.py:32, helper.py:96-101; eps 1e-6) applied to the rows on their
 * way into the first matrix product: y = the depthwise output (M, C), ln_gamma / ln_beta (C) fp32.  Training: the
 * normalised rows yn (operand of the W1 weight gradient) and stats (M, 2) fp32 = mean | rstd per row (what
 * vkas_layernorm_fwd writes, consumed by vkas_layernorm_bwd) are stored; inference: yn = stats = h = z = NULL and the
 * normalised rows never reach memory.  Replaces vkas_layernorm_fwd + vkas_mlp_chain_fwd of a ConvNeXt layer. */
int vkas_mlp_chain_ln_fwd(const void* y, long ldy, const float* ln_gamma, const float* ln_beta, void* yn, long ldyn,
                          float* stats, const void* img, const float* b2, const void* x, long ldx, const float* colscale,
                          const float* rowscale, int rows_per_image, void* h, long ldh, void* z, long ldz, void* out,
                          long ldo, long M, int C, int dtype, void* stream);
/* dh = (dz W2) * gelu'(h) (stored, operand of the W1 weight gradient); dyn = dh W1.  img_t = the mode-1 image. */
int vkas_mlp_chain_bwd(const void* dz, long lddz, const void* img_t, const void* h, long ldh, void* dh, long lddh,
                       void* dyn, long lddyn, long M, int C, int dtype, void* stream);
/* The three reporters below read the launch plan the 16-bit launchers execute (csrc/gemm_plan.h).
 * tile configuration a 16-bit call of these sizes runs.  fwd (wgrad == 0): 1 = 128x128 (4 waves), else the N extent 128 /
 * 192 / 224 of the 256-row 8-wave tile; wgrad: N extent 128 (4 waves), 192 / 224 (8 waves, 256 K columns) or 384 (8 waves,
 * 128 K columns); 0 when the plain fp32-FMA kernels are forced (VKAS_GEMM=simple). */
int vkas_conv_gemm_tile(int wgrad, long M, int Np, int K);
/* the kernel a 16-bit call with this geometry runs (wgrad: a plain vkas_conv_gemm_wgrad call).  0 = plain fp32-FMA kernels
 * forced.  fwd: 1 / 128 / 192 / 224 as above, 10 + depth = gemm_nt_ring_kernel<2 / 3 / 4>, 1000 + TN = the 3x3 row-slab kernel
 * conv3x3_slab_mfma_kernel<TN, .> (TN = 4, 6, 7); wgrad: 128 / 192 / 224 / 384, 2000 + TNn = conv3x3_wgrad_slab_kernel<TNn>
 * (6, 7, 8).  head_width > 0 for a fused-head launch (widest head). */
int vkas_conv_gemm_kernel_id(int wgrad, const vkas_conv_geom* g, int Np, long lddy, int head_width);
/* the A/B switches of the kernel choice, one per VKAS_* environment variable of INTEGRATION.md */
typedef struct vkas_gemm_switches {
  int nt_tile, tn_tile; /* VKAS_NT_TILE 1 / 128 / 192 / 224, VKAS_TN_TILE 128 / 192 / 224 / 384; any other value: unset */
  int nt_ring;          /* VKAS_NT_RING: < 0 unset, 2 / 3 / 4 the ring depth, any other value the register-staged kernel */
  int nt_noslab, nt_nobuf, tn_nobuf, tn_noslab, tn_no96; /* non-zero: set */
} vkas_gemm_switches;
/* the whole plan of a 16-bit call.  family: fwd 0 register-staged 128x128, 1 ring, 2 256-row tile, 3 row slab; wgrad 0
 * generic, 1 slab.  grid = tiles * splits; fwd: tiles = grid_m * grid_n and splits = 1 (a fused-head launch runs grid_m *
 * n_heads workgroups).  rows: rows per split (generic wgrad) or 64-row chunks per split (wgrad slab).  a_bytes / b_bytes:
 * the spans of x and of Bw (fwd) or dy (wgrad).  name: the kernel as a profiler prints it, template arguments shortened. */
typedef struct vkas_gemm_plan_info {
  int kernel_id, family, bn, ring, buf, head, pw, nobias, xg; /* kernel_id: vkas_conv_gemm_kernel_id; bn: N extent of the tile */
  long grid_m, grid_n, tiles, splits, rows, a_bytes, b_bytes;
  unsigned grid;
  char name[44];
} vkas_gemm_plan_info;
/* flags: 1 = vkas_conv_gemm_wgrad_gelu, 2 = vkas_conv_gemm_wgrad_ordered; has_gb: a bias gradient is asked for;
 * sw == NULL: the switches of this process's environment (and VKAS_GEMM=simple: kernel_id 0, name gemm_nt_simple /
 * gemm_tn_simple, nothing else filled). */
int vkas_conv_gemm_plan(int wgrad, const vkas_conv_geom* g, int Np, long lddy, int head_width, int flags, int has_gb,
                        const vkas_gemm_switches* sw, vkas_gemm_plan_info* out);
/* column sums: out[n] (+)= sum_m y[m][n]   (bias gradients) */
int vkas_colsum(const void* y, long ld, long M, int Np, float* out, int accumulate, float* ws, size_t ws_bytes,
                int dtype, void* stream);
size_t vkas_colsum_ws_bytes(long M, int Np);

/* ---- depthwise 7x7: helper.py:61-73 @ convnext.py:30 ------------------------------------------- */
/* y = dw7x7(x; w) + bias (+ addend).  w: the vkas_dw_weight_elems(Cp) floats written by vkas_pack_dw_weight. */
int vkas_dwconv7x7_fwd(const void* x, long ldx, const float* w, const float* bias, const void* addend, long ldadd,
                       void* y, long ldy, int B, int H, int W, int Cp, int dtype, void* stream);
/* gw (49, Cp) and gb (Cp) fp32, overwritten */
int vkas_dwconv7x7_wgrad(const void* x, long ldx, const void* dy, long lddy, float* gw, float* gb, float* ws,
                         size_t ws_bytes, int B, int H, int W, int Cp, int dtype, void* stream);
size_t vkas_dwconv7x7_wgrad_ws_bytes(int B, int H, int W, int Cp);

/* ---- LayerNorm over C (+ optional GELU): helper.py:96-101 --------------------------------------- */
/* y = act(LN(x) * gamma + beta); stats (M, 2) fp32 = (mean, rstd).  C = logical channels, pad channels -> 0.
 * gamma / beta: Cp floats, zero padded beyond C (vkas_pad_vector). */
int vkas_layernorm_fwd(const void* x, long ldx, const float* gamma, const float* beta, void* y, long ldy,
                       float* stats, long M, int C, int Cp, int act_gelu, int dtype, void* stream);
/* dx from dy; dgamma/dbeta (Cp) fp32 overwritten.  `x` is the forward input, `stats` from forward. */
int vkas_layernorm_bwd(const void* x, long ldx, const float* gamma, const float* beta, const float* stats,
                       const void* dy, long lddy, void* dx, long lddx, float* dgamma, float* dbeta, float* ws,
                       size_t ws_bytes, long M, int C, int Cp, int act_gelu, int dtype, void* stream);
size_t vkas_layernorm_bwd_ws_bytes(long M, int Cp);

/* ---- fused head tail (LayerNorm -> GELU -> Linear(C -> oc), oc <= 4): upernext.py:215-223, fpn.py:165-183 ------ */
/* gamma/beta (C), wproj (oc, C), bproj (oc) fp32 -> out[6*pw + 8] as laid out in vkas_head_desc */
int vkas_pack_head_params(const float* gamma, const float* beta, const float* wproj, const float* bproj, int C, int oc,
                          int pw, float* out, void* stream);
/* The same head tail as a pass of its own, for heads wider than the 224 columns the GEMM epilogue holds (ConvNeXt-Base /
 * Large: model/upernext.py:215-223 with 256-258 / 384+ channels; pw <= 512): z (M, ld ldz) = the convolution's output incl.
 * bias, written by a VKAS_EPI_NONE launch; hd->proj (n_heads, M, 8) and hd->stats (n_heads, M, 2; NULL = not kept) as
 * VKAS_EPI_HEAD writes them. */
int vkas_head_tail_fwd(const void* z, long ldz, const vkas_head_desc* hd, long M, int dtype, void* stream);
/* Forward of the x2 bilinear heads at the neck's height (upernext.py:237-244 followed by :215-223), z = b + conv3x3(U x) with
 * U = Uy (x) Ux: X1 = Ux x (vkas_resize2x_x_fwd); T (B, h, W2, 3 Nt) = the 1x3 row convolution of X1 with the mode-3 weight
 * image, column ky * Nt + n (vkas_conv_gemm_fwd with KH = 1, KW = 3, pad 1: the pad applies along x only, Hout = Hin; 16-bit
 * row-slab kernel, W2 % 256 == 0); this call forms z[r] = bias + sum_ky (Uy T_ky)[r + ky - 1] (tap rows outside [0, 2h) are the
 * convolution's zero padding) and runs the head tail on it.  z (B, 2h, W2, Nt) dense, or NULL together with hd->stats
 * (inference); hd->n0 count from column 0 of the Nt; hd->proj (n_heads, M, 8), hd->stats (n_heads, M, 2), M = B 2h W2, as
 * VKAS_EPI_HEAD writes them; pw <= 256.  seg_rows: source rows a workgroup walks down, 0 = the built-in rule; the results
 * do not depend on it.  Fixed summation order, no atomics: two launches give the same bits. */
int vkas_head_rows_fwd(const void* T, const float* bias, const vkas_head_desc* hd, void* z, int B, int h, int W2, int Nt,
                       int seg_rows, int dtype, void* stream);
/* backward of the fused tail for all heads of the launch at once: z / dz are the shared (M, sum np) buffers (strides ldz,
 * lddz), hd the descriptor used in the forward (params, stats; proj unused), dproj[h] the (M, 8) fp32 gradients of head
 * h's projection outputs -> dz and dparams[n_heads][6*pw + 8] (same layout as the packed parameters). */
int vkas_head_tail_bwd(const void* z, long ldz, const vkas_head_desc* hd, const float* const* dproj, void* dz, long lddz,
                       float* dparams, float* ws, size_t ws_bytes, long M, int dtype, void* stream);
size_t vkas_head_tail_bwd_ws_bytes(long M, int pw);

/* ---- block_scale / stochastic depth backward: convnext.py:56-58 ----------------------------------- */
/* dz = dout * rowscale[b] * colscale[c]; dscale[c] = sum_m dout*rowscale[b]*z; dbias2[c] = sum_m dz */
int vkas_scale_res_bwd(const void* dout, long lddo, const void* z, long ldz, const float* colscale,
                       const float* rowscale, int rows_per_image, void* dz, long lddz, float* dscale, float* dbias,
                       float* ws, size_t ws_bytes, long M, int Cp, int dtype, void* stream);
size_t vkas_scale_res_bwd_ws_bytes(long M, int Cp);

/* ---- resize: F.interpolate bilinear (upernext.py:79,178-195,237-244), nearest (fpn.py:125-142,197-204) */
/* mode 0 bilinear (align_corners=False), 1 nearest: src = min((int)floorf(dst * scale), in - 1) with scale = (float)in / out,
   product and quotient rounded to float32 as F.interpolate rounds them (not floor(dst * in / out) in integers: the two part
   where the exact quotient is an integer).  accumulate != 0: y += resize(x) (top-down add). */
int vkas_resize_fwd(const void* x, long ldx, void* y, long ldy, int B, int Hin, int Win, int Hout, int Wout,
                    int Cp, int mode, int accumulate, int dtype, void* stream);
/* y (B, H, 2 Win, Cp) = the x2 bilinear upsample of x (B, H, Win, Cp) along x only, with vkas_resize_fwd's arithmetic per
 * output (one rounded product, one fused multiply-add, one rounding to `dtype`); Win > 1 */
int vkas_resize2x_x_fwd(const void* x, long ldx, void* y, long ldy, int B, int H, int Win, int Cp, int dtype, void* stream);
/* dx (+)= resize^T(dy) */
int vkas_resize_bwd(const void* dy, long lddy, void* dx, long lddx, int B, int Hin, int Win, int Hout, int Wout,
                    int Cp, int mode, int accumulate, int dtype, void* stream);
/* the same with a workspace (fp32, vkas_resize_bwd_ws_bytes; 0 = none needed): large ratios - the necks' x4 / x8 resize to
   level-0 size, upernext.py:191-195 - then run as two separable gathers (along x into the workspace, then along y) */
size_t vkas_resize_bwd_ws_bytes(int B, int Hin, int Win, int Hout, int Wout, int Cp);
int vkas_resize_bwd_ws(const void* dy, long lddy, void* dx, long lddx, float* ws, size_t ws_bytes, int B, int Hin, int Win,
                       int Hout, int Wout, int Cp, int mode, int accumulate, int dtype, void* stream);

/* ---- head backward at the neck's resolution: z = conv3x3(U x), U = x2 bilinear (upernext.py:237-244) ---- */
/* dz (B, 2h, 2w, N) bf16 / fp16 with row stride lddz -> E (B, h, w, 9 N) dense, column k * N + n:
 * E_k[s, n] = sum_q U[q, s] * dz[q + (k - 1), n], k = (ky, kx) the tap of the dgrad convolution (the K order of the mode-1
 * weight image), zero where q + (k - 1) leaves the map.  Then dx = E . Bt^T and dW[n][c][8 - k] = sum_s E_k[s, n] x[s, c]. */
int vkas_upconv_adj(const void* dz, long lddz, void* E, int B, int h, int w, int N, int dtype, void* stream);
/* the same E (bit for bit), and out[n] (+)= the column sums of dz over all B * 2h * 2w rows - what vkas_colsum delivers - from
 * the values the kernel loads anyway.  N <= 2048; ws: vkas_upconv_adj_colsum_ws_bytes of per-workgroup partial rows; fixed
 * summation order.  A thread walks down the source rows of one segment of an image with the horizontal partial sums of its six
 * window rows in registers, so each dz row is loaded once per column instead of three times. */
size_t vkas_upconv_adj_colsum_ws_bytes(int B, int h, int w, int N);
int vkas_upconv_adj_colsum(const void* dz, long lddz, void* E, int B, int h, int w, int N, float* out, int accumulate, float* ws,
                           size_t ws_bytes, int dtype, void* stream);
/* the same with the segment length in source rows given: 0 = the rule of the plain entry, longer than the image = one segment.
 * The results do not depend on it (E bit for bit; the column sums up to the order of the fp32 additions). */
int vkas_upconv_adj_colsum_seg(const void* dz, long lddz, void* E, int B, int h, int w, int N, float* out, int accumulate,
                               float* ws, size_t ws_bytes, int dtype, void* stream, int seg_rows);
/* gE (9 N, Cp) fp32, row k * N + n [the weight-gradient GEMM of E against x] added onto the packed gradient of the forward
 * taps: gwp (N, 3, 3, Cp)[n][8 - k][c] += gE[k * N + n][c] */
int vkas_upconv_adj_unpack_wgrad(const float* gE, float* gwp, int N, int Cp, void* stream);

/* ---- nn.AdaptiveAvgPool2d(s): upernext.py:62 ------------------------------------------------------ */
int vkas_adaptive_avgpool_fwd(const void* x, long ldx, void* y, long ldy, int B, int H, int W, int s, int Cp,
                              int dtype, void* stream);
int vkas_adaptive_avgpool_bwd(const void* dy, long lddy, void* dx, long lddx, int B, int H, int W, int s, int Cp,
                              int accumulate, int dtype, void* stream);

/* ---- the pooled branches of the pyramid-pooling block as one set of kernels (csrc/ppm.hip): upernext.py:48-84 ----------
 * cat (B, H, W, >= C + nb Cb):  cat[..., :C] = x,  cat[..., C + k Cb : C + (k+1) Cb] = bilinear(gelu(LN(pool_{s_k}(x) W_k^T +
 * b_k)) -> H x W) for the nb scales s_k.  16-bit storage only (VKAS_BF16 / VKAS_F16), C and Cb multiples of 8, H and W
 * arbitrary (H < s included); limits below.  params: 4 nb device pointers, per branch W_k (Cb, C), b_k, gamma_k, beta_k (Cb),
 * all fp32 as the modules hold them (W_k is rounded to the storage type on load).  Pooled rows are branch-major: branch k owns
 * rows [B cell0_k, B cell0_{k+1}) of the (B S, .) buffers, cell0_k = sum_{j<k} s_j^2, S = cell0_nb; row = B cell0_k + b s_k^2 +
 * bi s_k + bj.  SS = sum s_k.  Three forward launches, four backward launches, no atomics, fixed summation order. */
#define VKAS_PPM_MAX_BRANCHES 4
#define VKAS_PPM_MAX_SCALE 16
#define VKAS_PPM_MAX_CELLS 256 /* S */
#define VKAS_PPM_MAX_C 2048
#define VKAS_PPM_MAX_CB 512
/* row groups of the two row kernels (4 rows of one branch each): the partial rows vkas_ppm_rows_bwd leaves; < 0: bad arguments */
long vkas_ppm_row_groups(int B, int nb, const int* scales);
/* forward 1: cat[..., :C] = x and rowsum (B, H, SS, C) fp32 = the sums of every image row over the x bins of every branch */
int vkas_ppm_pool_fwd(const void* x, long ldx, void* cat, long ldcat, float* rowsum, int B, int H, int W, int C, int Cb,
                      int nb, const int* scales, int dtype, void* stream);
/* forward 2: pooled P (B S, C), Linear output lin (B S, Cb), stats (B S, 2) fp32 [mean, rstd] - all three NULL when nothing is
 * kept for a backward - and act (B S, Cb) = gelu(LN(lin)); P, lin and act are each rounded once to `dtype` */
int vkas_ppm_rows_fwd(const float* rowsum, const float* const* params, void* pooled, void* lin, float* stats, void* act, int B,
                      int H, int W, int C, int Cb, int nb, const int* scales, int dtype, void* stream);
/* forward 3: every branch of act resized (vkas_resize_fwd's bilinear arithmetic) into its channel slice of cat */
int vkas_ppm_resize_fwd(const void* act, void* cat, long ldcat, int B, int H, int W, int C, int Cb, int nb, const int* scales,
                        int dtype, void* stream);
/* backward 1: tx (B, H, SS, Cb) fp32 = the x half of the resize adjoint of the branch slices of dcat (read in place, pixel
 * stride lddcat) */
int vkas_ppm_resize_bwd_x(const void* dcat, long lddcat, float* tx, int B, int H, int W, int C, int Cb, int nb,
                          const int* scales, int dtype, void* stream);
/* backward 2: the y half, LN + GELU backward -> dz (B S, Cb) in `dtype`, partial (vkas_ppm_row_groups, 2 Cb) fp32 rows of
 * dgamma | dbeta, and dp (B S, C) fp32 = dz W_k (NULL: no input gradient wanted) */
int vkas_ppm_rows_bwd(const float* tx, const float* const* params, const void* lin, const float* stats, void* dz,
                      float* partial, float* dp, int B, int H, int W, int C, int Cb, int nb, const int* scales, int dtype,
                      void* stream);
/* backward 3: grads[4 k + 0 .. 3] = dW_k (Cb, C), db_k, dgamma_k, dbeta_k (fp32, contiguous); accumulate[i] != 0: added onto
 * what grads[i] holds (a parameter's gradient view), else written */
int vkas_ppm_param_grads(const void* dz, const void* pooled, const float* partial, float* const* grads, const int* accumulate,
                         int B, int C, int Cb, int nb, const int* scales, int dtype, void* stream);
/* backward 4: dx = dcat[..., :C] + sum_k pool_k^T(dp_k), rounded once */
int vkas_ppm_pool_bwd(const void* dcat, long lddcat, const float* dp, void* dx, long lddx, int B, int H, int W, int C, int Cb,
                      int nb, const int* scales, int dtype, void* stream);

/* ---- elementwise ------------------------------------------------------------------------------------ */
/* y[m][0..Cp) = x[m][0..Cp) (+ y if accumulate): channel-slice copies for concat / its backward */
int vkas_copy_channels(const void* x, long ldx, void* y, long ldy, long M, int Cp, int accumulate, int dtype,
                       void* stream);
/* y[m][c_dst + c] = x[m][c_src + c] for c in [0, C), then zero_tail zero channels behind them; channel offsets are
   element-granular (no 8-channel alignment): torch.cat of parts whose widths are not multiples of 8 - e.g.
   FpnNeck(..., out_channels=400) -> 4 x 100 channels, fpn.py:75,144; upernext.py:82,144,197 - and its backward */
int vkas_copy_channel_range(const void* x, long ldx, int c_src, void* y, long ldy, int c_dst, long M, int C,
                            int zero_tail, int dtype, void* stream);
/* nn.Softplus() on fp32 maps: adaptive_scaling.py:101,140 */
int vkas_softplus_fwd(const float* x, float* y, long n, void* stream);
int vkas_softplus_bwd(const float* x, const float* dy, float* dx, long n, void* stream);

/* ---- dense losses: loss_function/adaptive_scaling.py -------------------------------------------------- */
typedef struct vkas_rough_loss_cfg {
  float focal_factor, dice_factor, l1_factor, score_min, height_min; /* :29-35 */
  float focal_alpha, focal_gamma;                                    /* focal_with_logits.py:21-23 */
  float out_scale;                                                   /* train.py:413 (1/2), x 1/world */
} vkas_rough_loss_cfg;
/* mask_feat/height_feat (B,1,H,W) fp32; gt_mask/gt_score (B,CH,CW) fp32; box = up,left of the crop.
 * sums: 8 doubles workspace kept for backward; loss: 1 float (already multiplied by out_scale). */
int vkas_rough_loss_fwd(const float* mask_feat, const float* height_feat, const float* gt_mask,
                        const float* gt_score, int B, int H, int W, int up, int left, int CH, int CW,
                        const vkas_rough_loss_cfg* cfg, double* sums, float* loss, void* stream);
int vkas_rough_loss_bwd(const float* mask_feat, const float* height_feat, const float* gt_mask,
                        const float* gt_score, int B, int H, int W, int up, int left, int CH, int CW,
                        const vkas_rough_loss_cfg* cfg, const double* sums, const float* dloss, float* d_mask_feat,
                        float* d_height_feat, void* stream);

typedef struct vkas_precise_loss_cfg {
  float pos_l2, neg_l2, offset_l1, reg_l1, angle_ce, dist_l1, loss_factor; /* :136-145 */
  float smooth_beta;                                                       /* 2.5, :159-165 */
  float out_scale;
} vkas_precise_loss_cfg;
/* margin[0] = min over the n label points of min(py, H-1-py, px, W-1-px): negative iff a point lies outside the (H, W) map.
 * The reference's advanced indexing (loss_function/adaptive_scaling.py:235-262) raises for such a point; the host reads this
 * value asynchronously instead of synchronising inside the step. */
int vkas_points_margin(const int64_t* py, const int64_t* px, long n, int H, int W, int64_t* margin, void* stream);
/* The three terms the reference's config can switch on (all off by default, :136-140):
 * mask_focal  sigmoid focal loss (mean over B*CH*CW) of the cropped mask logits against gt_mask, :272-277
 * prob_l1     smooth-L1 (beta prob_l1_beta) of sigmoid(prob) against gt_score, sum(e * gt_mask) / (sum(gt_mask) + 1e-6),
 *             :284-289
 * prob_wahr   weight-adaptive heatmap regression of sigmoid(prob) against gt_score (mean), :303-307 and
 *             weight_adaptive_heatmap_regression.py:20-32
 * A factor <= 0 switches its term off. */
typedef struct vkas_precise_loss_extra_cfg {
  float mask_focal, prob_l1, prob_wahr; /* char_mask_focal_factor, char_prob_l1_factor, char_prob_wahr_factor */
  float prob_l1_beta;                   /* 0.25, :156 (must be positive when prob_l1 > 0) */
  float wahr_gamma;                     /* 0.01, weight_adaptive_heatmap_regression.py:20 */
  float focal_alpha, focal_gamma;       /* 0.25, 2: focal_with_logits.py:21-23 (alpha < 0: no alpha weighting) */
} vkas_precise_loss_extra_cfg;
#define VKAS_PRECISE_LOSS_SUMS 16 /* doubles of the `sums` workspace, kept from forward for backward */
/* prob (B,1,H,W), offset (B,2,H,W), angle (B,4,H,W), dist (B,4,H,W) fp32 NCHW; py/px (B,P) int64;
 * gt_offsets (B,P,2), gt_angles (B,P,4), gt_dists (B,P,3) fp32.  ex is required.  mask_feat (B,1,H,W) fp32 mask logits,
 * read over the same crop as prob (may be NULL unless mask_focal > 0); sums of VKAS_PRECISE_LOSS_SUMS doubles;
 * d_mask_feat (B,1,H,W), written in full (zeros outside the crop and everywhere when mask_focal <= 0), may be NULL
 * unless mask_focal > 0.  Every output and the workspace are written by kernels alone, so both calls can be captured
 * into a graph. */
int vkas_precise_loss_fwd(const float* prob, const float* offset, const float* angle, const float* dist,
                          const float* gt_score, const float* gt_mask, const int64_t* py, const int64_t* px,
                          const float* gt_offsets, const float* gt_angles, const float* gt_dists, int B, int H,
                          int W, int up, int left, int CH, int CW, int P, const vkas_precise_loss_cfg* cfg,
                          const float* mask_feat, const vkas_precise_loss_extra_cfg* ex, double* sums, float* loss,
                          void* stream);
int vkas_precise_loss_bwd(const float* prob, const float* offset, const float* angle, const float* dist,
                          const float* gt_score, const float* gt_mask, const int64_t* py, const int64_t* px,
                          const float* gt_offsets, const float* gt_angles, const float* gt_dists, int B, int H,
                          int W, int up, int left, int CH, int CW, int P, const vkas_precise_loss_cfg* cfg,
                          const float* mask_feat, const vkas_precise_loss_extra_cfg* ex, const double* sums,
                          const float* dloss, float* d_prob, float* d_offset, float* d_angle, float* d_dist,
                          float* d_mask_feat, void* stream);

/* ---- primitive loss callables: loss_function/__init__.py:12-18 ------------------------------------------- */
#define VKAS_LOSS_FOCAL 0     /* focal_with_logits.py:18-47: p0 = alpha (< 0: no alpha weighting), p1 = gamma */
#define VKAS_LOSS_DICE 1      /* dice.py:17-35: pred are probabilities; 1 - 2 sum(pg) / (sum p + sum g + eps) */
#define VKAS_LOSS_L1 2        /* l1.py:19-47, smooth = False */
#define VKAS_LOSS_SMOOTH_L1 3 /* l1.py:19-47, smooth = True: p0 = smooth_beta */
#define VKAS_LOSS_L2 4        /* l2.py:18-34 */
#define VKAS_LOSS_WAHR 5      /* weight_adaptive_heatmap_regression.py:17-32: pred are probabilities, p0 = gamma,
                                 mean over n of (s(1-p) + (1-s)p)(p-g)^2 with s = g^gamma; takes no mask (must be NULL) */
/* pred, gt, mask (nullable): n fp32 elements each.  mask == NULL: mean over n; else sum(e * mask) / (sum(mask) + eps)
 * (dice: pred and gt are multiplied by the mask).  sums: 4 doubles kept for backward; loss: 1 float. */
int vkas_elementwise_loss_fwd(int kind, const float* pred, const float* gt, const float* mask, long n, float p0, float p1,
                              float eps, double* sums, float* loss, void* stream);
int vkas_elementwise_loss_bwd(int kind, const float* pred, const float* gt, const float* mask, long n, float p0, float p1,
                              float eps, const double* sums, const float* dloss, float* dpred, void* stream);
/* F.cross_entropy(logits (rows, classes), target), mean over rows: cross_entropy_with_logits.py:16-19.
 * hard = 0: target is (rows, classes) fp32 class probabilities; hard = 1: (rows,) int64 class indices in range. */
int vkas_cross_entropy_fwd(const float* logits, const void* target, int hard, long rows, int classes, double* sums,
                           float* loss, void* stream);
int vkas_cross_entropy_bwd(const float* logits, const void* target, int hard, long rows, int classes, const float* dloss,
                           float* dlogits, void* stream);

/* ---- label-point backward of the regression heads: loss_function/adaptive_scaling.py:167-179,235-262 -------------------- */
/* The precise loss reads the offset / angle / distance maps only at the (B,P) label points, so d(conv output) of those heads
 * has B*P non-zero rows.  These calls compact them (csrc/points.hip) for vkas_head_tail_bwd and the GEMMs.
 * prepare: py, px (B,P) int64 label points (clamped into the map like the loss does).  map (B*H*W int32 scratch) receives the
 * owner point of every pixel (0x7f7f7f7f = none); pix (Mp >= B*P int32) = pixel index of point i when it owns its pixel,
 * -1 - pixel for a duplicate of an earlier point, INT_MIN for the padding rows i >= B*P. */
int vkas_points_prepare(const long* py, const long* px, int B, int P, int H, int W, int* map, int* pix, long Mp, void* stream);
/* zs (Mp, Ns) = columns [c0, c0+Ns) of the z rows at the points; stats_s (n_heads, Mp, 2) / dproj_s (n_heads, Mp, 8) = the
 * LayerNorm statistics (n_heads, M, 2) and the heads' d(proj) rows (M, 8) there.  Duplicates and padding rows get zero
 * d(proj) (a pixel's gradient is taken once); padding rows are zero throughout.  16-bit activations. */
int vkas_points_gather_rows(const void* z, long ldz, int c0, int Ns, const float* stats, const float* const* dproj,
                            int n_heads, long M, const int* pix, long Mp, void* zs, float* stats_s, float* dproj_s,
                            int dtype, void* stream);
/* xs (Mp, 3, 3, Cp) = the zero-padded 3x3 neighbourhoods x[p + (ky-1, kx-1)] of the owner points (zeros elsewhere): the
 * activation operand of a 1x1 weight-gradient GEMM whose result has the 3x3 convolution's packed (N, ky, kx, Cp) layout. */
int vkas_points_gather_patches(const void* x, long ldx, int Cp, int B, int H, int W, const int* pix, long Mp, void* xs,
                               int dtype, void* stream);
/* the same patches of the x2 bilinear upsample of x (B, h, w, Cp) without materialising it: pix are pixels of the 2h x 2w map
 * (vkas_points_prepare with H = 2h, W = 2w); bit for bit what vkas_points_gather_patches reads from vkas_resize_fwd's output */
int vkas_points_gather_patches_up2(const void* x, long ldx, int Cp, int B, int h, int w, const int* pix, long Mp, void* xs,
                                   int dtype, void* stream);
/* D (Mp, 3, 3, Cp) fp32: D[i][ky][kx] is the input-gradient contribution of point i to pixel p_i + (ky-1, kx-1).  Adds them onto
 * dx (B,H,W,Cp; ld lddx): every touched pixel is summed in fp32 by one workgroup and written once.  Only the owners' rows of D
 * (pix[i] >= 0) are read: the rows of duplicates and of padding may hold anything. */
int vkas_points_scatter3x3(const float* D, const int* pix, const int* map, long Mp, int B, int H, int W, int Cp, void* dx,
                           long lddx, int dtype, void* stream);
/* The same contributions through U^T (U: x2 bilinear, align_corners=False, clamped) onto the gradient of the source map:
 * dx (B,h,w,Cp; ld lddx)[s] += sum U[q, s] * D[i][t] over the (point i, tap t) pairs that land on an upsampled pixel q reading
 * s.  pix / map are those of the upsampled (2h x 2w) map (vkas_points_prepare with H = 2h, W = 2w).  Every touched source pixel
 * is summed in fp32 in a fixed order by one workgroup and written once; no atomics. */
int vkas_points_scatter3x3_low(const float* D, const int* pix, const int* map, long Mp, int B, int h, int w, int Cp, void* dx,
                               long lddx, int dtype, void* stream);

/* (Mp, 8) fp32 rows <-> the (M, 8) projected-channel map of a head at the label points (opt-in label-point forward of
 * the regression heads, ops.HeadsAtPoints): scatter writes the owner rows (pix[i] >= 0) to their pixels (duplicates
 * and padding rows are skipped; dst is expected to be zero elsewhere); gather reads the owners' pixels and zero-fills the other rows. */
int vkas_points_scatter_vec8(const float* src, const int* pix, long Mp, float* dst, void* stream);
int vkas_points_gather_vec8(const float* src, const int* pix, long Mp, float* dst, void* stream);

/* ---- all packed operands of a step in one launch ------------------------------------------------------------------- */
/* One entry per packed image: kind 0 = vkas_pack_conv_weight(_slice) (mode, n_off, Nt, dtype as there; a plain weight has
 * n_off = 0, Nt = Np), kind 1 = vkas_pack_dw_weight (mode = flip; N, KH, KW, Np, n_off, Nt, dtype unused).  total =
 * elements of the image. */
typedef struct {
  const float* w;
  void* out;
  long total;
  int kind, N, C, KH, KW, Np, Cp, mode, n_off, Nt, dtype;
} vkas_pack_desc;
/* descs (count entries) and block_start (count + 1 ints: first workgroup of every entry - an entry takes
 * vkas_pack_many_blocks(&desc) workgroups -; block_start[count] = total_blocks) live in DEVICE memory and stay valid until the launch has run: the table of a model is
 * built once and re-used every step (the parameters and their images keep their addresses). */
int vkas_pack_many(const vkas_pack_desc* descs, const int* block_start, int count, int total_blocks, void* stream);
/* workgroups entry d takes: 32 x 64 tiles of the transposed image for kind 0 / mode 1 (dgrad layout), else 2048 elements each */
int vkas_pack_many_blocks(const vkas_pack_desc* d);

/* ---- inference post-processing on the device: inferencing/adaptive_scaling.py:129-188,318-396 ------------------------ */
/* mask_logit, height (B,1,H,W) fp32 -> out_mask (B,H,W) uint8 = sigmoid >= mask_thr, out_height (B,H,W) fp32 = height where
 * >= height_min else 0; both 0 on rows >= valid_h[b] / columns >= valid_w[b] (the divisible-by-32 padding, in feature
 * pixels; NULL = the whole map is valid). */
int vkas_rough_postprocess(const float* mask_logit, const float* height, int B, int H, int W, const int* valid_h,
                           const int* valid_w, float mask_thr, float height_min, unsigned char* out_mask,
                           float* out_height, void* stream);
/* prob_logit (B,1,H,W), offset (B,2,H,W), angle (B,4,H,W), dist (B,4,H,W) fp32 -> out_prob (B,H,W) = sigmoid (0 in the
 * padding), out_offset (B,H,W,2), out_angle (B,H,W,4) = softmax over the 4 logits, out_dist (B,H,W,4). */
int vkas_precise_postprocess(const float* prob_logit, const float* offset, const float* angle, const float* dist, int B,
                             int H, int W, const int* valid_h, const int* valid_w, float* out_prob, float* out_offset,
                             float* out_angle, float* out_dist, void* stream);
/* Character quadrilaterals from the precise maps (:399-465,481-491).  prob (B,H,W) as vkas_precise_postprocess writes it,
 * offset (B,H,W,2), angle (B,H,W,4) softmaxed, dist (B,H,W,4), all fp32.  A pixel is a peak when prob equals the max over the
 * size x size window [c - size/2, c + size - 1 - size/2] clamped to the map (scipy maximum_filter) and !(prob < thr).
 * Outputs, capacity B*H*W rows in np.nonzero (b, y, x) order: *count (int32), points (cap,3) int32 (b, y, x), probs (cap),
 * quads (cap,4,2) fp32 (y, x) corners up-left, up-right, down-right, down-left, at p = (y * scale_y, x * scale_x).
 * Capture-safe: no allocation, no synchronisation, no atomics (deterministic).  B*H*W < 2^31, size >= 1; workspace
 * 16-byte aligned, at least vkas_char_polygons_workspace_bytes (which returns -1 on bad arguments). */
long vkas_char_polygons_workspace_bytes(int B, int H, int W, int size);
int vkas_char_polygons(const float* prob, const float* offset, const float* angle, const float* dist, int B, int H, int W,
                       int size, float thr, float scale_y, float scale_x, void* workspace, size_t workspace_bytes,
                       int* count, int* points, float* probs, float* quads, void* stream);
/* Training label maps from character quadrilaterals (dataset/labels.py holds the rule - this project's own, restated on
 * pixels - and the host oracle char_label_maps_host).  rows (B,K,20) int32, one row per quad: 8 Q4 corners (y, x) of up-left,
 * up-right, down-right, down-left in map coordinates; the inclusive pixel box (y0, x0, y1, x1); fp32 bits of the centre (cy,
 * cx), of the inverse frame (m00, m01, m10, m11) and of the height; valid.  count (B) is clamped to [0, K] on the device.  A
 * cell (y, x) of the h x w map is inside a row iff the row is valid, the cell lies in the row's box and the four int64 edge
 * functions of the corners are >= 0 at (16y + 8, 16x + 8); its owner is the inside row with the smallest fp32 a = k * (s*s +
 * t*t), s = m00*dy + m01*dx, t = m10*dy + m11*dx, dy = (float(y) + 0.5f) - cy (every operation rounded, no fma), ties to the
 * lowest index.  Outputs, each (B,CH,CW) = the map cropped to rows [up, up+CH) and columns [left, left+CW), each may be NULL
 * (not all): owner int32 = index + 1 or 0; mask = owner != 0; height = the owner's; score = expf(-a) of the owner; 0 without
 * one.  One launch; no atomics, no allocation, no synchronisation; every output element is written exactly once: capture-safe
 * and bit-identical from run to run.  A row with valid == 0 is skipped and a row's box is intersected with the tile, whatever
 * it holds, so no table content makes the kernel touch memory outside its buffers.  B in 0..65535, K >= 0, B*h*w < 2^31, the
 * crop inside the map, k finite and positive; rows 16-byte aligned.  16-byte stores when CW % 4 == 0 and the outputs are
 * 16-byte aligned, scalar stores otherwise. */
int vkas_char_label_maps(const int* rows, const int* count, int B, int K, int h, int w, int up, int left, int CH, int CW,
                         float k, int* owner, float* mask, float* height, float* score, void* stream);
/* Matching predicted character quadrilaterals to annotated ones by IoU (inferencing/evaluation.py holds the rule - this
 * project's own - and the host oracles quad_iou_host / match_quads_host).  gt_rows (B,M,16) and pred_rows (B,N,16) int32, one
 * row per quad: 8 Q4 corners (y, x) of up-left, up-right, down-right, down-left; the inclusive Q4 box (y0, x0, y1, x1); twice
 * the area in Q4^2 as int64 (low word first); valid; zero.  gt_count, pred_count (B) are clamped to [0, M] / [0, N] on the
 * device.  A pair takes part iff both rows are valid and their boxes overlap (inclusive); its IoU is the Sutherland-Hodgman
 * clip of the pred against the gt's edges in binary64, every operation rounded once (no fma); pairs with iou >= iou_thr are
 * the candidates, matched one to one by the greedy rule (iou descending, gt ascending, pred ascending), computed as
 * mutual-best rounds.  Outputs: gt_match (B,M) int32 = the pred index or -1; pred_match (B,N) int32; gt_iou (B,M) binary64,
 * 0 where unmatched; stats (B,6) int64 = tp, n_gt, n_pred (valid rows within the count), pairs, candidates, status; rounds (B)
 * int32, may be NULL = the rounds that took an edge.  An image with more than max_pairs candidates keeps its true pairs and
 * candidates, and gets status = 1, every match -1, tp = 0 and rounds = 0: never a partial result.  Four launches on one
 * stream; integer atomics in LDS only, no allocation, no synchronisation, every output element and every workspace word that
 * is read is written by the call's own kernels: capture-safe and bit-identical from run to run.  Counts are clamped, ring
 * stores bounded by 8 vertices and candidate stores by max_pairs: no table content makes a kernel touch memory outside its
 * buffers.  B in 0..65535, M and N in 1..8192 (beyond: an error, not a clamp), max_pairs >= 0, B*max_pairs < 2^31, iou_thr in
 * (0, 1]; tables and workspace 16-byte aligned, workspace at least vkas_quad_match_workspace_bytes (which returns -1 on bad
 * arguments). */
long long vkas_quad_match_workspace_bytes(int B, int M, int N, int max_pairs);
int vkas_quad_match(const int* gt_rows, const int* gt_count, const int* pred_rows, const int* pred_count, int B, int M, int N,
                    double iou_thr, int max_pairs, void* workspace, size_t workspace_bytes, int* gt_match, int* pred_match,
                    double* gt_iou, long long* stats, int* rounds, void* stream);
/* Ranked matching of character quadrilaterals at T IoU thresholds with don't-care annotations, the device half of average
 * precision (inferencing/ranking.py holds the rule - this project's own - in its module docstring, and the host oracles
 * match_quads_ranked_host / match_quads_ranked_rounds_host).  gt_rows (B,M,16), pred_rows (B,N,16) match rows and counts as
 * for vkas_quad_match; gt_care (B,M) uint8, 0 = don't care, NULL = every annotation is a care one; probs (B,N) fp32;
 * iou_thrs = T binary64 values IN HOST MEMORY, strictly ascending in (0, 1], checked on the host; cover_thr in (0, 1].  A
 * pred takes part iff it lies within the count, its valid word is set and its prob is finite; a gt iff it lies within the
 * count and its valid word is set.  q outranks p iff probs[q] > probs[p], or they are equal and q < p (fp32 comparisons).
 * For a box-overlapping pair one clip of p against g (that of vkas_quad_match) gives inter2 and iou; p is covered iff
 * inter2 >= cover_thr * area2_p (one rounding, inclusive) for some don't-care g; the candidates at threshold t are the (care
 * gt, pred) pairs with iou >= iou_thrs[t].  Per threshold, independently, going down the ranks a pred takes the free
 * candidate with the highest iou (then the lowest gt): TP = 1 if it took one, else IGNORED = 3 if covered, else FP = 2;
 * ABSENT = 0 takes no part.  Computed as rounds: an undecided pred is decided unless a higher-ranked undecided pred shares a
 * free candidate with it; a round reads what the previous one left.  Outputs: pred_match (B,T,N) int32 gt index or -1;
 * pred_state (B,T,N) uint8; gt_match (B,T,M) int32; pred_iou (B,T,N) binary64, 0 unless TP; covered (B,N) uint8; stats
 * (B,T,8) int64 = tp, fp, ignored, n_gt (care gts), n_pred (preds taking part), pairs (care box pairs), candidates (at
 * iou_thrs[t]), status; dc_stats (B,3) int64 = n_dc, dc_pairs, n_covered; rounds (B,T) int32, may be NULL = the rounds that
 * decided a pred.  An image with more than max_pairs candidates at iou_thrs[0] keeps its true pairs and candidates (at every
 * threshold) and gets status = 1, every state 0, every match -1, tp = fp = ignored = 0 and rounds = 0: never a partial
 * result; covered and dc_stats are true all the same.  Four launches on one stream (the pair, scan and fill passes of
 * vkas_quad_match at iou_thrs[0], then B*T workgroups of rounds over the one candidate list); integer atomics in LDS only,
 * no allocation, no synchronisation, every output element and every workspace word that is read is written by the call's
 * own kernels: capture-safe and bit-identical from run to run; reads are bounded by the tables and stores by the buffers
 * whatever the tables hold.  B in 0..65535, M and N in 1..8192, T in 1..16, B*T <= 65535 (beyond: an error, not a clamp),
 * max_pairs >= 0, B*max_pairs < 2^31; tables and workspace 16-byte aligned, pred_iou, stats and dc_stats 8-byte aligned,
 * workspace at least vkas_quad_match_ranked_workspace_bytes (-1 on bad arguments). */
long long vkas_quad_match_ranked_workspace_bytes(int B, int M, int N, int T, int max_pairs);
int vkas_quad_match_ranked(const int* gt_rows, const int* gt_count, const unsigned char* gt_care, const int* pred_rows,
                           const int* pred_count, const float* probs, int B, int M, int N, const double* iou_thrs, int T,
                           double cover_thr, int max_pairs, void* workspace, size_t workspace_bytes, int* pred_match,
                           unsigned char* pred_state, int* gt_match, double* pred_iou, unsigned char* covered,
                           long long* stats, long long* dc_stats, int* rounds, void* stream);
/* inferencing.match_rows on the device: quads (B,K,4,2) binary64 (y, x) corners, valid (B,K) uint8 or NULL -> rows (B,K,16)
 * int32 as above.  Per quad: c16 = rint(c * 16) (half to even); the quad is valid iff its valid byte is non-zero, every
 * |c16| <= 2^19 (NaN and inf fail) and the four int64 cross products of successive edges are positive; twice the area is
 * the exact int64 shoelace sum; an invalid quad gets a zero row.  Equal to match_rows on every input.  One launch, no
 * atomics, every row written exactly once.  B, K >= 0, B*K < 2^27; quads 8-byte and rows 16-byte aligned. */
int vkas_quad_rows(const double* quads, const unsigned char* valid, int B, int K, int* rows, void* stream);
/* Greedy non-maximum suppression of character quadrilaterals by IoU (inferencing/nms.py holds the rule - this project's own
 * - and the host oracle nms_quads_host).  rows (B,K,16) int32 match rows, count (B) clamped to [0, K] on the device, probs
 * (B,K) fp32.  A row takes part iff it lies within the count, its valid word is set and its prob is finite; every other row
 * within the count passes through as kept.  j outranks i iff probs[j] > probs[i], or they are equal and j < i (fp32
 * comparisons).  j is a neighbour of i iff both take part, j outranks i, their boxes overlap (inclusive) and the IoU of
 * vkas_quad_match with i as the gt and j as the pred is >= iou_thr.  Going down the ranks a quad is kept iff none of its
 * neighbours was kept; computed as rounds (an undecided quad is suppressed once a neighbour is kept, kept once all are
 * suppressed; a round reads the states the previous round left).  Outputs: keep (B,K) uint8, 0 beyond the count;
 * suppressor (B,K) int32 = the highest-ranked kept neighbour of a suppressed quad, else -1; stats (B,6) int64 = kept (rows
 * with keep = 1), n (the clamped count), n_valid (rows that take part), pairs (box-overlapping pairs of them with j
 * outranking i), candidates (those at or above iou_thr), status; rounds (B) int32, may be NULL = the rounds that decided a
 * quad.  An image with more than max_pairs candidates keeps its true pairs and candidates and gets status = 1, keep = 1
 * within the count, every suppressor -1, kept = n and rounds = 0: never a partial result.  Four launches on one stream (the
 * pair, scan and fill passes of vkas_quad_match on one table, then the rounds); one integer atomic in LDS, no allocation,
 * no synchronisation, every output element and every workspace word that is read is written by the call's own kernels:
 * capture-safe and bit-identical from run to run.  Reads are bounded by K and stores by the buffers whatever the tables
 * hold.  B in 0..65535, K in 1..8192 (beyond: an error, not a clamp), max_pairs >= 0, B*max_pairs < 2^31, iou_thr in
 * (0, 1]; rows and workspace 16-byte aligned, workspace at least vkas_quad_nms_workspace_bytes (-1 on bad arguments). */
long long vkas_quad_nms_workspace_bytes(int B, int K, int max_pairs);
int vkas_quad_nms(const int* rows, const int* count, const float* probs, int B, int K, double iou_thr, int max_pairs,
                  void* workspace, size_t workspace_bytes, unsigned char* keep, int* suppressor, long long* stats, int* rounds,
                  void* stream);
/* Scoring detected text lines against annotated ones with one-to-one matches, splits and merges (inferencing/
 * line_evaluation.py holds the rule - this project's own - and the host oracles match_lines_host, the sequential form, and
 * match_lines_rounds_host).  Tables as for vkas_quad_match_ranked (no probs); tr_q8 and tp_q8 in 1..256 are the recall and
 * precision thresholds as rint(x * 256); cover_thr in (0, 1].  A row takes part iff it lies within the (clamped) count and
 * its valid word is set.  For a box-overlapping pair one clip of p against g (that of vkas_quad_match) gives inter2.  With a
 * don't-care g: p is IGNORED iff inter2 >= cover_thr * area2_p (one rounding, inclusive); don't-care gts and ignored preds
 * take no further part.  With a care g: I = int64(floor(min(inter2, 2^41))), A = min(max(area2, 0), 2^41) of either row;
 * rec_ok <=> 256 I >= tr_q8 A_g, prec_ok <=> 256 I >= tp_q8 A_p, all int64; the pair is a candidate iff I > 0 and one of the
 * two holds.  Phase A: (g, p) match one to one iff both tests hold and no other pair of g's row or p's column passes both.
 * Phase B, free care gts ascending: S_g = the free preds with prec_ok; g is SPLIT into them iff |S_g| >= 2 and
 * 256 sum I >= tr_q8 A_g.  Phase C, free preds ascending: M_p = the free care gts with rec_ok; they are MERGED into p iff
 * |M_p| >= 2 and 256 sum I >= tp_q8 A_p.  B and C are computed as rounds: every ready gt (pred) offers itself to its set, a
 * pred (gt) keeps the lowest offer, a ready gt (pred) takes its set iff it holds all of it; a round reads what the previous
 * one left.  Outputs: gt_kind (B,M) uint8 = 0 absent, 1 unmatched, 2 one-to-one, 3 split, 4 merged, 5 don't care; gt_group
 * (B,M) int32 = the pred for 2 and 4, g for 3, else -1; pred_kind (B,N) uint8 = 0 absent, 1 unmatched, 2 one-to-one, 3 split
 * part, 4 merge, 5 ignored; pred_group (B,N) int32 = the gt for 2 and 3, p for 4, else -1; stats (B,16) int64 = n_gt (care),
 * n_pred (taking part, not ignored), one_to_one, split_gt, split_pred, merged_gt, merge_pred, n_dc, n_ignored, pairs (box
 * pairs of rows taking part), candidates (among care gts and preds not ignored), status, rounds_split, rounds_merge, 0, 0;
 * rounds (B,2) int32, may be NULL = the two round counts again.  An image with more than max_pairs candidates keeps its
 * true counts and gets status = 1, no match of any kind and both round counts 0: never a partial result.  Four launches on
 * one stream (counting pass over 64 x 64 tiles, scan, filling pass, one workgroup per image for the phases); integer
 * atomics in LDS only, no allocation, no synchronisation, every output element and every workspace word that is read is
 * written by the call's own kernels: capture-safe and bit-identical from run to run; reads are bounded by the tables and
 * stores by the buffers whatever the tables hold.  B in 0..65535, M and N in 1..8192 (beyond: an error, not a clamp),
 * max_pairs >= 0, B*max_pairs < 2^31; tables and workspace 16-byte aligned, stats 8-byte aligned, workspace at least
 * vkas_line_match_workspace_bytes (-1 on bad arguments).  Argument errors return before any launch. */
long long vkas_line_match_workspace_bytes(int B, int M, int N, int max_pairs);
int vkas_line_match(const int* gt_rows, const int* gt_count, const unsigned char* gt_care, const int* pred_rows,
                    const int* pred_count, int B, int M, int N, int tr_q8, int tp_q8, double cover_thr, int max_pairs,
                    void* workspace, size_t workspace_bytes, unsigned char* gt_kind, int* gt_group, unsigned char* pred_kind,
                    int* pred_group, long long* stats, int* rounds, void* stream);
/* Scoring curved text lines as ribbons of quads (inferencing/ribbon_evaluation.py holds the rule - this project's own - and
 * the host oracles match_ribbons_host, the sequential form, and match_ribbons_rounds_host).  Per side a ribbon table
 * (B,K,16) int32 with counts as for vkas_line_match and a segment table (B,S,16) int32 of match rows.  A ribbon row: word 0 =
 * seg_start, an index into its image's segment table; word 1 = seg_count in 1..256; words 2..7 zero; 8..11 the union of the
 * segment boxes; 12..13 the sum of the segments' area2 as one int64; 14 valid; 15 zero.  For a pair of ribbons that both take
 * part and whose boxes overlap, I = min(sum over the segment pairs (i, j) whose boxes overlap and whose valid words are set
 * of int64(floor(min(inter2(gseg_i, pseg_j), 2^41))), 2^41), inter2 from the one clip of vkas_quad_match on the two segment
 * rows; the sum is over integers.  Everything else is vkas_line_match's with this I in place of floor(inter2): the coverage
 * test of a don't-care gt is (double)I >= cover_thr * area2_p, A_g and A_p are the clamped areas of the ribbon rows, and the
 * tests, the phases, the outputs, stats, rounds, capacity and status are those of vkas_line_match word for word.  A ribbon
 * row with seg_count outside 1..256, seg_start < 0 or seg_start + seg_count > S has no segments (every I with it is 0) and
 * still takes part as its valid word says; both are checked against S before any use as an index.  Segment boxes and areas
 * are believed as written.  Four launches on one stream (counting pass over 64 x 64 tiles of ribbons with one wave per listed
 * pair, its lanes striding over the segment pairs; scan; filling pass, which computes I again for the candidates only;
 * the phases); integer atomics in LDS only, no allocation, no synchronisation, every output element and every workspace
 * word that is read is written by the call's own kernels: capture-safe and bit-identical from run to run; reads are bounded
 * by the tables and stores by the buffers whatever the tables hold.  B in 0..65535, M and N in 1..8192, Sg and Sp in
 * 1..2^21 (beyond: an error, not a clamp), max_pairs >= 0, B*max_pairs < 2^31; all four tables and the workspace 16-byte
 * aligned, stats 8-byte aligned, workspace at least vkas_ribbon_match_workspace_bytes (-1 on bad arguments; the size is that
 * of vkas_line_match).  Argument errors return before any launch. */
long long vkas_ribbon_match_workspace_bytes(int B, int M, int N, int max_pairs);
int vkas_ribbon_match(const int* gt_rows, const int* gt_count, const unsigned char* gt_care, const int* gt_segs, int Sg,
                      const int* pred_rows, const int* pred_count, const int* pred_segs, int Sp, int B, int M, int N, int tr_q8,
                      int tp_q8, double cover_thr, int max_pairs, void* workspace, size_t workspace_bytes,
                      unsigned char* gt_kind, int* gt_group, unsigned char* pred_kind, int* pred_group, long long* stats,
                      int* rounds, void* stream);
/* Grouping character quadrilaterals into text lines (inferencing/lines.py holds the rule - this project's own, all integer -
 * and the host oracle quad_lines_host).  rows (B,K,16) int32 match rows, count (B) clamped to [0, K] on the device; gap_q4
 * and cross_q4 in 1..4096, ratio_q4 in 16..256 (Q4).  A row takes part iff it lies within the count and its valid word is
 * set.  Per quad, in int64: s = P0+P1+P2+P3, v = (P3+P2)-(P0+P1), u = (P1+P2)-(P0+P3), vv = v.v.  i and j are linked iff
 * both take part and, with d = s_j - s_i, for a in {i, j}: 8|d.v_a| <= cross_q4 vv_a and 8|d_y v_a,x - d_x v_a,y| <= gap_q4
 * vv_a; 256 vv_i <= ratio_q4^2 vv_j and the same swapped; v_i.v_j > 0.  A line is a connected component of the links; lines
 * are numbered from 0 by their smallest member.  Per line U = the sum of u over its members, (0, 16) if that is (0, 0);
 * the members are listed in ascending (s.U, index); a = P.U and b = P_y U_x - P_x U_y over all corners of all members give
 * the extent.  Outputs: line (B,K) int32 = the line number, -1 for a row that takes no part or lies beyond the count; order
 * (B,K) int32 = the member indices line after line in reading order, -1 beyond the n_part entries; table (B,K,8) int64 rows
 * start, size, U_y, U_x, a_min, a_max, b_min, b_max for lines 0..L-1 and zero rows after them (K rows is the exact worst
 * case: no overflow path); stats (B,4) int64 = n (the clamped count), n_part, links (pairs i < j), lines.  Eight launches
 * on one stream (init, the pair tiles with an atomicMin union-find on a global parent array, flatten, line numbers, sums,
 * starts, extents, ranks); integer atomics only (32-bit minima on the parents, 64-bit adds, minima and maxima on the
 * table), no floating point, no allocation, no synchronisation, every output element and every workspace word that is
 * read is written by the call's own kernels: capture-safe and bit-identical from run to run.  Reads are bounded by K and
 * stores by the buffers whatever the tables hold.  B in 0..65535, K in 1..8192 (beyond: an error, not a clamp); rows and
 * workspace 16-byte aligned, table and stats 8-byte aligned, workspace at least vkas_quad_lines_workspace_bytes (-1 on bad
 * arguments). */
long long vkas_quad_lines_workspace_bytes(int B, int K);
int vkas_quad_lines(const int* rows, const int* count, int B, int K, int gap_q4, int cross_q4, int ratio_q4, void* workspace,
                    size_t workspace_bytes, int* line, int* order, long long* table, long long* stats, void* stream);
/* Text regions of the rough maps (the step between the passes, :190-279, restated on pixels).  mask (B,H,W) uint8 and height
 * (B,H,W) fp32 as vkas_rough_postprocess writes them.  A region is an 8-connected component of mask != 0; the regions of each
 * image are numbered 1..N by their first pixel in row-major order.  Outputs: count (B) = the true N of each image; labels
 * (B,H,W) int32, 0 = background; and, with R = max_regions rows per image, row r-1 for region r <= R: boxes (B,R,4) =
 * (y0, x0, y1, x1) inclusive, areas (B,R), valid (B,R) = the region's pixels with height > 0, medians (B,R) = the fp32 median
 * of those heights (the middle element, (a + b) * 0.5f of the two middle ones, 0 without any) - np.median's bits.  Rows
 * beyond an image's count are zero.  An image with N > R regions keeps its true count and labels (values above R occur)
 * and fills R rows; nothing is written beyond them.  Capture-safe: no allocation, no synchronisation, every workspace word
 * and table row is (re)written by the call's own kernels; integer atomics only (deterministic).  B, H, W, max_regions >= 1,
 * B*H*W < 2^31; workspace 16-byte aligned, at least vkas_text_regions_workspace_bytes (which returns -1 on bad arguments). */
long long vkas_text_regions_workspace_bytes(int B, int H, int W, int max_regions);
int vkas_text_regions(const unsigned char* mask, const float* height, int B, int H, int W, int max_regions, void* workspace,
                      long long workspace_bytes, int* count, int* labels, int* boxes, int* areas, int* valid, float* medians,
                      void* stream);
/* Crop, rescale and pack text regions into the page of the precise pass (:190-293 restated on pixels; the resampling rule
 * in integers and the host oracles: inferencing/packing.py).  src (Hs,Ws,3) uint8; placements (n,8) int32 rows (sy, sx, sh,
 * sw, dy, dx, dh, dw): source rectangle [sy,sy+sh) x [sx,sx+sw) inside src -> destination rectangle [dy,dy+dh) x
 * [dx,dx+dw) inside page (Hp,Wp,3) uint8; sides 1..8192; destinations pairwise disjoint (the caller's check: the table
 * lives in device memory).  Per axis, S -> D samples: D < S area coverage, D >= S two-tap bilinear with half-pixel centres
 * and clamped taps; a channel = (sum wy*wx*p + den/2) / den, integers only.  EVERY page byte is written: resampled pixels
 * inside the placements, 0 elsewhere; n = 0 gives a zero page.  A row whose sides or source rectangle are out of range is
 * skipped, so no table content makes the kernel read outside src or write outside page.  One launch; capture-safe: no
 * allocation, no synchronisation, no atomics.  Hs, Ws, Hp, Wp in 1..32768; table 16-byte aligned. */
int vkas_resample_pack_u8(const unsigned char* src, int Hs, int Ws, const int* placements, int n, unsigned char* page,
                          int Hp, int Wp, void* stream);
/* The region-label page that goes with it: out (Hq,Wq) int32 at 1/fdf of the page.  A label pixel (v,u) whose centre
 * (v*fdf + fdf/2, u*fdf + fdf/2) lies in the destination of placement k gets region_ids[k] - unless the rough label map
 * (labels (Hl,Wl) int32, of which valid_h x valid_w cover the Hs x Ws image the sources refer to) holds the label of ANOTHER
 * region (neither 0 nor region_ids[k]) at the pixel's source position; then, and outside every placement, it gets 0.  Source
 * position: map row min(valid_h - 1, ((2*dh*sy + t*sh) * valid_h) / (2*dh*Hs)) with t = 2*v*fdf + fdf - 2*dy; columns
 * likewise.  Every out element is written; same contract as above otherwise; fdf in 1..64. */
int vkas_pack_region_labels(const int* labels, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws,
                            const int* placements, const int* region_ids, int n, int fdf, int* out, int Hq, int Wq,
                            void* stream);
/* The same step for a batch (infer_batch): several sources, several pages, one launch.  The sources lie in one byte arena;
 * sources (S,4) int64 rows (byte offset, Hs, Ws, 0): image s is (Hs,Ws,3) uint8 at arena + offset.  rows (n,12) int32 (src,
 * page, sy, sx, sh, sw, dy, dx, dh, dw, local_id, global_id), sorted by page; page_start (Q+1) int32: page q owns
 * rows[page_start[q] .. page_start[q+1]) (clamped to 0..n).  pages (Q,Hp,Wp,3) uint8; grid (ceil(Wp/64), ceil(Hp/16), Q).
 * The resampling rule is vkas_resample_pack_u8's; EVERY byte of every page is written, 0 where no row reaches.  A row is
 * skipped when src is outside 0..S-1, page != q, its sides or rectangles are out of range, or its source entry is (sides
 * outside 1..32768, offset < 0, offset + 3*Hs*Ws > arena_bytes): every address is arena + offset and is checked against
 * arena_bytes per row, so no table content makes the kernel touch memory outside its buffers.  Destinations are disjoint
 * per page (the caller's check).  One launch; capture-safe: no allocation, no synchronisation, no atomics.  Q in 1..65535,
 * Hp, Wp in 1..32768; rows 16-byte, sources 8-byte aligned. */
int vkas_resample_pack_u8_multi(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                                const int* rows, int n, const int* page_start, unsigned char* pages, int Q, int Hp, int Wp,
                                void* stream);
/* The label pages that go with them: out (Q,Hq,Wq) int32 at 1/fdf of the pages.  The rough label maps of the batch (local
 * ids 1..N_i per image) lie in one int32 arena; label_sources (S,8) int64 rows (word offset, Hl, Wl, valid_h, valid_w, Hs,
 * Ws, 0).  A label cell whose centre lies in a row's destination gets the row's global_id - unless the rough label under
 * it (the source position of vkas_pack_region_labels) is neither 0 nor the row's local_id; then, and outside every row, 0.
 * A row is skipped as above (entry: map and image sides outside 1..32768, valid part outside the map, offset < 0, offset +
 * Hl*Wl > label_words).  Every out element is written; same contract otherwise; fdf in 1..64. */
int vkas_pack_region_labels_multi(const int* label_arena, long long label_words, const long long* label_sources, int S,
                                  const int* rows, int n, const int* page_start, int fdf, int* out, int Q, int Hq, int Wq,
                                  void* stream);
/* Orientation of the text regions (inferencing/orient.py holds the rule and the host oracles).  labels (B,H,W) int32 as
 * vkas_text_regions writes them; R = max_regions rows per image, row r-1 for region r; label 0 and labels above R are
 * ignored.  moments (B,R,6) int64 = n, sum y, sum x, sum y^2, sum x^2, sum x*y over the region's pixels, exact (sides up to
 * 32768 and B*H*W < 2^31 keep every sum below 2^61); a region without pixels gets zeros.  Capture-safe: no allocation, no
 * synchronisation, every table row is (re)written by the call; 64-bit integer atomics only (deterministic).  B <= 65535. */
int vkas_region_moments(const int* labels, int B, int H, int W, int max_regions, long long* moments, void* stream);
/* dirs (B,R,2) int32 (c, s), |c|, |s| <= 2^14: extents (B,R,4) int32 = min u, max u, min v, max v over the region's pixels
 * with u = c*x + s*y, v = -s*x + c*y; a region without pixels keeps (INT_MAX, INT_MIN, INT_MAX, INT_MIN).  Same contract;
 * extents 16-byte aligned. */
int vkas_region_extents(const int* labels, int B, int H, int W, int max_regions, const int* dirs, int* extents,
                        void* stream);
/* Affine warps into the page.  warps (n,12) int64 rows (dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, 0): destination
 * pixel (i, j) of [dy,dy+dh) x [dx,dx+dw) reads src at Y = ay + i*myy + j*myx, X = ax + i*mxy + j*mxx in Q16 (an integer
 * coordinate is a pixel centre).  Bounds: sides 1..8192, |m| <= 2^22, |ay|, |ax| < 2^40, log2n in 0..3; a row outside them is
 * skipped.  With N = 2^log2n a pixel is the mean of N x N sub-samples at Y + ((2a+1-N)*myy + (2b+1-N)*myx) >> (1+log2n) (X
 * likewise; arithmetic shifts), each two-tap bilinear per axis (k = Y >> 16, f = Y & 65535, weights 65536 - f and f on k and
 * k+1; a tap outside src reads 0); a channel = (sum + den/2) >> (32 + 2*log2n).  Writes ONLY the pixels inside the
 * destinations (it runs after vkas_resample_pack_u8 on the same page); destinations are disjoint from each other and from
 * the placements (the caller's check).  One launch (none for n = 0); capture-safe; table 8-byte aligned. */
int vkas_warp_pack_u8(const unsigned char* src, int Hs, int Ws, const long long* warps, int n, unsigned char* page, int Hp,
                      int Wp, void* stream);
/* The label cells of the warps: a cell (v,u) whose centre lies in the destination of warp k (the test of
 * vkas_pack_region_labels) has i2 = 2*v*fdf + fdf - 2*dy - 1, j2 likewise, Y = ay + ((i2*myy + j2*myx) >> 1), source pixel
 * Yp = (Y + 32768) >> 16 (X likewise).  Outside the Hs x Ws source it gets 0; else region_ids[k] unless the rough map holds
 * another region's label at row min(valid_h - 1, ((2*Yp+1)*valid_h) / (2*Hs)), column likewise.  Writes ONLY those cells. */
int vkas_warp_region_labels(const int* labels, int Hl, int Wl, int valid_h, int valid_w, int Hs, int Ws,
                            const long long* warps, const int* region_ids, int n, int fdf, int* out, int Hq, int Wq,
                            void* stream);
/* Training crops from annotated pages (dataset/crops.py holds the rule and the host oracle crop_host).  The pages lie in one
 * byte arena with the (S,4) int64 source table of vkas_resample_pack_u8_multi.  rows (B,16) int64, one per output image:
 * source, ay, ax, myy, myx, mxy, mxx (Q16: the map of vkas_warp_pack_u8 for a destination at (0, 0) of H x W), log2n, the fp32
 * bits (low 32) of three gains, three biases and the noise amplitude, the 64-bit noise key.  out (B,3,H,W) fp32: the
 * geometric value v of a pixel and channel is that warp's uint8 (N x N bilinear sub-samples, a tap outside the page reading
 * 0, one rounding); then, every product and sum rounded once, t = gain_c*v; t += bias_c; t += amp*r; out = t > 0 ? min(t, 255)
 * : 0, with r = float(u >> 40) * 2^-23 - 1, u = mix((idx + 1) * 0x9E3779B97F4A7C15 + key), idx = (c*H + y)*W + x, mix the
 * splitmix64 finaliser.  An image whose row has a source outside 0..S-1, a source entry with a side outside 1..8192, offset < 0
 * or offset + 3*Hs*Ws > arena_bytes, |m| > 2^22 or |a| >= 2^40 is written as zeros; log2n is clamped to 0..3; taps are
 * bounded by the source's sides: no table content makes the kernel touch memory outside its buffers.  One launch (none for
 * B = 0), grid (ceil(W/64), ceil(H/16), B); every out element is written exactly once; capture-safe: no allocation, no
 * synchronisation, no atomics.  B in 0..65535, H, W in 1..8192; tables 8-byte aligned; 16-byte stores when W % 4 == 0 and
 * out is 16-byte aligned, plain stores otherwise. */
int vkas_crop_warp_f32(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                       const long long* rows, int B, float* out, int H, int W, void* stream);
/* The same crops, blurred between the geometric value and the jitter (dataset/blur.py holds the rule and the host oracle
 * crop_blur_host).  blur_rows (B,226) int32, one per output image: the radius R in 0..7, then a 15 x 15 weight table, row-major,
 * centred at (7,7); valid when every weight is in 0..65536, every weight outside the central (2R+1)^2 square is 0 and the sum
 * is 65536.  With v(i, j) the geometric value of vkas_crop_warp_f32 at crop cell (i, j) - the row's map continues outside the
 * H x W crop, zero outside the page - acc = sum over a, b in -R..R of w[7+a][7+b] * v(y+a, x+b) (below 2^24), and the steps of
 * vkas_crop_warp_f32 run on fp32(acc) * 2^-16 (exact) instead of v; R = 0 gives its output bit for bit.  An image whose crop row
 * cannot be trusted (as there) or whose blur row is invalid or has R > radius_max is written as zeros.  Two launches (none for
 * B = 0): the geometric values of the cells -radius_max .. H+radius_max-1 x -radius_max .. W+radius_max-1, each computed once,
 * as uint8 planes (B, 3, H + 2*radius_max, pitch), pitch = W + 2*radius_max rounded up to 16, in `work` (work_bytes at least
 * that size, else VKAS_E_ARG before any launch); then the weighted sums from 16 x 64 tiles staged through LDS.  Every out
 * element is written exactly once; capture-safe: no allocation, no synchronisation, no atomics; bit-identical from run to
 * run.  B in 0..65535, H, W in 1..8192, radius_max in 0..7; tables 8-byte aligned, blur_rows 4-byte, work 16-byte; the stores
 * of vkas_crop_warp_f32. */
int vkas_crop_warp_blur_f32(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                            const long long* rows, const int* blur_rows, int B, int radius_max, unsigned char* work,
                            long long work_bytes, float* out, int H, int W, void* stream);
/* Text lines cut into upright strips of one height h (inferencing/strips.py holds the rule from a quadrilateral to a row and
 * the host oracle quad_strips_host).  The images lie in one byte arena with the (S,4) int64 source table of
 * vkas_resample_pack_u8_multi.  The table `rows` holds 13*n + 1 int64 words: n strip rows of 12 words (src, offset, slot_w,
 * w, ay, ax, myy, myx, mxy, mxx, log2n, 0), then tile_start, n + 1 words: tile_start[0] = 0 and tile_start[r + 1] =
 * tile_start[r] + ceil(h/16) * ceil(slot_w[r]/64), the tiles of 16 x 64 pixels that the kernel gives row r (a workgroup finds
 * the row of its tile by binary search).  Strip row r owns the slot of h x slot_w x 3 bytes at out + offset: pixel (i, j)
 * with j < w is the pixel of vkas_warp_pack_u8 for the warp (0, 0, h, w, ay, ax, myy, myx, mxy, mxx, log2n) of image src
 * (N x N bilinear sub-samples, a tap outside the image reading 0, one rounding), the columns w..slot_w-1 are 0.  Every byte
 * of every slot is written, no other byte of out is touched; slots are pairwise disjoint (the caller's check).  The kernel
 * checks every row itself: a row whose slot is not defined inside out (slot_w outside 1..8192, offset < 0, offset +
 * 3*h*slot_w > out_bytes) is skipped; a row with src outside 0..S-1, a source entry with a side outside 1..32768, offset < 0
 * or offset + 3*Hs*Ws > arena_bytes, w outside 1..slot_w, |m| > 2^22, |a| >= 2^40 or log2n outside 0..3 gets a slot of zeros.
 * tile_start is not trusted either: its total is clamped to n * ceil(h/16) * 128, and a tile outside its row's own count is
 * dropped (a wrong tile_start leaves tiles unwritten, nothing else): no table content makes the kernel touch memory outside
 * its buffers.  One launch (none for n = 0) of min(n * ceil(h/16) * 128, 2048) workgroups that stride over the tiles;
 * capture-safe: no allocation, no synchronisation, no atomics; bit-identical from run to run.  h in 1..256, n >= 0,
 * out_bytes < 2^40, tables 8-byte aligned; three aligned dword stores per 4 pixels where the address is 4-byte aligned
 * (always when out, offset and slot_w are multiples of 4), byte stores otherwise. */
int vkas_quad_strips_u8(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                        const long long* rows, int n, int h, unsigned char* out, long long out_bytes, void* stream);
/* Curved text lines cut into strips along their spines (inferencing/spines.py holds the rule from a line's character quads
 * to its knots, the integer rule from knots to columns and the host oracle spine_strips_host).  Arena, source table, slots
 * and tiles are those of vkas_quad_strips_u8.  `table` holds 13*n + 1 + 6*knots_total int64 words: n spine rows of 12 words
 * (src, offset, slot_w, w, knot_start, knots, col_start, log2n, 0, 0, 0, 0), then tile_start (n + 1 words, as above), then
 * knots_total knot records of 6 words (q, cy, cx, vy, vx, 0: the strip column, the centre and the down vector in Q16, an
 * integer coordinate being a pixel centre).  Row r reads the knots knot_start .. knot_start + knots - 1 and owns the column
 * records col_start .. col_start + w - 1 of the workspace, 6 words each (ay, ax, myy, myx, mxy, mxx).
 * Column j: lo = 0, hi = knots; while hi - lo > 1: mid = (lo + hi) >> 1, lo = mid if q[mid] <= j else hi = mid.  It is valid
 * iff lo + 1 < knots, q[lo] <= j < q[lo+1], n = q[lo+1] - q[lo] <= 8192, both knots have |c| < 2^39 and |v| <= 2^30 and the
 * record is within |a| < 2^40, |m| <= 2^22.  With fdiv the floor division, rdiv(x, d) = fdiv(2x + d, 2d), a = 2*(j - q[lo]) +
 * 1: Cy = cy_lo + fdiv((cy_hi - cy_lo) * a, 2n) (Cx, Vy, Vx likewise), myy = rdiv(Vy, h), mxy = rdiv(Vx, h), ay = Cy -
 * fdiv((h - 1) * myy, 2) (ax likewise), myx = rdiv(cy_hi - cy_lo, n), mxx likewise.  An invalid column is six words of
 * INT64_MIN.  Pixel (i, j) with j < w is the pixel (i, 0) of vkas_warp_pack_u8 for the warp (0, 0, h, 1, ay, ax, myy, myx,
 * mxy, mxx, log2n) of image src, 0 in an invalid column; the columns w..slot_w-1 are 0.
 * vkas_spine_strips_workspace_bytes(columns) = 48 * columns (-1 for columns < 0): the caller's workspace holds the sum of
 * w records (at most out_bytes / (3*h) when the slots are disjoint).  vkas_spine_columns writes the column records alone
 * (columns_cap: the records there is room for); vkas_spine_strips_u8 runs that launch and the strips launch on one stream.
 * The kernels check every row themselves: a row whose slot is not defined inside out (as above) is skipped; a row that
 * fails any other check (those of vkas_quad_strips_u8 on src, the source entry, w and log2n; knot_start < 0, knots < 2,
 * knot_start + knots > knots_total; col_start < 0, col_start + w > the workspace's records) gets a slot of zeros and no
 * column records.  tile_start is not trusted either (as above), and a tile reads column records only where the columns
 * launch, which walks the same tiles by the same search, has written them - else it is dropped: no table content makes a
 * kernel touch memory outside its buffers.  Rows whose column ranges or slots overlap give an unspecified winner (the
 * caller's check).  Capture-safe: no allocation, no synchronisation, no atomics; bit-identical from run to run.  h in
 * 1..256, n >= 0, knots_total >= 0, out_bytes < 2^40, ws_bytes >= 48 * n (columns_cap >= n), pointers non-null, table,
 * source table and workspace 8-byte aligned: otherwise an error and no launch; no launch for n = 0. */
long long vkas_spine_strips_workspace_bytes(long long columns);
int vkas_spine_columns(const long long* table, int n, long long knots_total, int h, long long* columns,
                       long long columns_cap, void* stream);
int vkas_spine_strips_u8(const unsigned char* arena, long long arena_bytes, const long long* sources, int S,
                         const long long* table, int n, long long knots_total, int h, void* ws, long long ws_bytes,
                         unsigned char* out, long long out_bytes, void* stream);

/* ---- optimizer on the flat parameter / gradient buffers: train.py:468-478 ------------------------------ */
/* sumsq (1 double, zeroed by the call) = sum g^2 */
int vkas_l2norm_sq(const float* g, long n, double* sumsq, void* stream);
/* clip coefficient = min(1, max_norm / (sqrt(sumsq) + 1e-6)) [torch clip_grad_norm_]; AdamW (decoupled wd):
 * p -= lr*wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v/(1-b2^t)) + eps) */
int vkas_adamw_step(float* p, const float* g, float* m, float* v, long n, const double* sumsq, float max_norm,
                    float grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKAS_H */
