// Launch plans of the 16-bit implicit-GEMM kernels (gemm_mfma.hip): which kernel a call reaches, with which grid and split
// over M.  Pure host arithmetic on the geometry and the switches - no environment, no statics, no device state - so the
// launchers, the reporters of gemm_api.hip and tests/test_cpu_gemm_plan.py read one rule.
#pragma once
#include "../../include/vkas.h"

constexpr int VKAS_TN_ROWS = 64;  // reduction rows per iteration of the weight-gradient kernels

enum vkas_nt_family { VKAS_NT_REG128, VKAS_NT_RING, VKAS_NT_TILE256, VKAS_NT_SLAB };
enum vkas_tn_family { VKAS_TN_GENERIC, VKAS_TN_SLAB };

struct vkas_nt_plan {
  vkas_nt_family family;  // register-staged 128x128 | gemm_nt_ring_kernel | 256-row 8-wave tile | conv3x3_slab_mfma_kernel
  int bn;                 // N extent of the tile: 128 / 192 / 224
  int ring;               // ring depth 2 / 3 / 4 (VKAS_NT_RING), else 0
  int kh;                 // 1: the 1x3 row convolution (row slab only; any other family: no kernel), else 3
  bool buf, head;         // operands addressed with 32-bit buffer offsets; fused head epilogue
  long a_bytes, b_bytes;  // bytes spanned by x and Bw
  long grid_m, grid_n;    // the grid is grid_m x (a fused-head launch: the number of heads, else grid_n) workgroups
};

struct vkas_tn_plan {
  vkas_tn_family family;      // gemm_tn_mfma_kernel | conv3x3_wgrad_slab_kernel
  int tile;                   // N extent: 128 (4 waves), 192 / 224 / 384 (8 waves) generic; 96 / 112 / 128 slab
  bool buf, pw, nobias, xg;   // buffer loads; the pointwise and the no-bias-gradient instantiation; gelu(x) on load
  long splits, rows;          // splits over M; rows per split (generic) or 64-row chunks per split (slab)
  long tiles;                 // output tiles
  unsigned grid;              // tiles * splits
  long x_bytes, dy_bytes;     // bytes spanned by x and dy
};

// the switches this process's environment sets (read once)
const vkas_gemm_switches* vkas_gemm_env_switches();

// bytes spanned by a 16-bit (rows, width) operand of pixel stride ld (x may be a channel slice: the last pixel ends after
// width of its ld channels), and whether such a span can be addressed with 32-bit buffer offsets
inline long vkas_span_bytes(long rows, long ld, long width) { return ((rows - 1) * ld + width) * 2; }
inline bool vkas_fits_buffer(long bytes) { return bytes < 0xFFFFFFF0L; }

// what vkas_conv_gemm_tile reports: forward 1 = the 4-wave 128x128 tile, else the N extent of the 256-row tile; wgrad the N extent
int vkas_nt_tile_rule(long M, int Np, const vkas_gemm_switches& sw);
int vkas_tn_tile_rule(long M, int Np, int K, const vkas_gemm_switches& sw);

// head_width: 0, or the columns of the widest head of a fused-head launch
vkas_nt_plan vkas_plan_nt(const vkas_conv_geom& g, int Np, int head_width, const vkas_gemm_switches& sw);
// flags: 1 = gelu(x) on load (vkas_conv_gemm_wgrad_gelu), 2 = no split over M (vkas_conv_gemm_wgrad_ordered)
vkas_tn_plan vkas_plan_tn(const vkas_conv_geom& g, int Np, long lddy, int flags, bool has_gb, const vkas_gemm_switches& sw);

// the values of vkas_conv_gemm_kernel_id (include/vkas.h)
inline int vkas_nt_kernel_id(const vkas_nt_plan& p) {
  return p.family == VKAS_NT_SLAB ? (p.kh == 1 ? 1100 : 1000) + p.bn / 32 : (p.family == VKAS_NT_RING ? 10 + p.ring : (p.family == VKAS_NT_REG128 ? 1 : p.bn));
}
inline int vkas_tn_kernel_id(const vkas_tn_plan& p) { return p.family == VKAS_TN_SLAB ? 2000 + p.tile / 16 : p.tile; }
