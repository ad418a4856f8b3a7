// The kernel choice of the 16-bit implicit GEMMs as pure functions (gemm_plan.h).  Host code only.
#include "gemm_plan.h"

#include <stdlib.h>

#include <initializer_list>

static long cdiv(long a, long b) { return (a + b - 1) / b; }
static long padded(long n, long t) { return cdiv(n, t) * t; }

const vkas_gemm_switches* vkas_gemm_env_switches() {
  static const vkas_gemm_switches sw = [] {
    const auto num = [](const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; };
    const auto set = [](const char* name) { return (int)(getenv(name) != nullptr); };
    return vkas_gemm_switches{num("VKAS_NT_TILE", 0), num("VKAS_TN_TILE", 0), num("VKAS_NT_RING", -1), set("VKAS_NT_NOSLAB"),
                              set("VKAS_NT_NOBUF"),   set("VKAS_TN_NOBUF"),   set("VKAS_TN_NOSLAB"),   set("VKAS_TN_NO96")};
  }();
  return &sw;
}

static bool row_aligned_3x3(const vkas_conv_geom& g, int wmod) {
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && g.Hout == g.Hin && g.Wout == g.Win && g.Win % wmod == 0;
}

// 256-row tiles once there is enough work to fill the chip with them; N extent = the candidate with the least zero padding
// (ties -> wider tile, fewer re-reads of A)
int vkas_nt_tile_rule(long M, int Np, const vkas_gemm_switches& sw) {
  const int f = sw.nt_tile;
  if (f == 1 || f == 128 || f == 192 || f == 224) return f;
  if (M < 16384) return 1;
  int bn = 224;
  for (int c : {192, 128})
    if (padded(Np, c) < padded(Np, bn)) bn = c;
  return bn;
}

// 8-wave tiles when there is enough work and K is wide enough; N extent = least zero padding
int vkas_tn_tile_rule(long M, int Np, int K, const vkas_gemm_switches& sw) {
  const int f = sw.tn_tile;
  if (f == 128 || f == 192 || f == 224 || f == 384) return f;
  int bn = 128;
  if (M >= 16384 && K >= 192) {
    for (int c : {192, 224})
      if (padded(Np, c) <= padded(Np, bn)) bn = c;
    // 384 (N) x 128 (K) instead of 192 x 256 - the same 96 x 64 per wave - where the 256-wide K tiles would be padded and the
    // 128-wide ones are not (K = 384: the W1 weight gradient of a C = 384 ConvNeXt MLP ran a quarter of its products on zeros)
    if (bn == 192 && Np % 384 == 0 && padded(K, 128) < padded(K, 256)) bn = 384;
  }
  return bn;
}

vkas_nt_plan vkas_plan_nt(const vkas_conv_geom& g, int Np, int head_width, const vkas_gemm_switches& sw) {
  const long M = (long)g.B * g.Hout * g.Wout, K = (long)g.KH * g.KW * g.Cp;
  vkas_nt_plan p = {};
  p.head = head_width > 0;
  p.a_bytes = vkas_span_bytes((long)g.B * g.Hin * g.Win, g.ldx, g.Cp);
  p.b_bytes = (long)Np * K * 2;
  const bool fits = vkas_fits_buffer(p.a_bytes) && vkas_fits_buffer(p.b_bytes);
  p.kh = 3;
  if (g.KH == 1 && g.KW == 3) {
    // 1x3 along image rows (pad applies to x alone): conv1x3_slab_mfma_kernel, 256-row tiles whatever M is; the family says
    // whether the geometry is one the kernel takes
    p.kh = 1;
    // N extent: 224 or 192, whichever pads less; the 128-column tile only for launches it holds in one tile (it pads the
    // precise heads' N = 2 328 least, but ran them in 5.87 ms against 5.30 ms with 224 columns); VKAS_NT_TILE overrides
    const int f = sw.nt_tile;
    p.bn = f == 128 || f == 192 || f == 224 ? f : (Np <= 128 ? 128 : (padded(Np, 192) < padded(Np, 224) ? 192 : 224));
    p.grid_n = cdiv(Np, p.bn);
    p.grid_m = M / 256;
    const bool rows = g.stride == 1 && g.pad == 1 && g.Hout == g.Hin && g.Wout == g.Win && g.Win % 256 == 0;
    p.family = rows && fits && !p.head ? VKAS_NT_SLAB : VKAS_NT_TILE256;
    p.buf = true;
    return p;
  }
  // one 256-row tile per head: the narrowest N extent that holds the widest head
  const int choice = p.head ? (head_width <= 128 ? 128 : (head_width <= 192 ? 192 : 224)) : vkas_nt_tile_rule(M, Np, sw);
  p.bn = choice == 1 ? 128 : choice;
  p.grid_n = cdiv(Np, p.bn);
  if (choice != 1) {
    // 3x3 / stride 1 / pad 1 with rows of whole 256-pixel tiles, operands addressable with 32-bit buffer offsets: the row slab
    const bool slab = !sw.nt_noslab && row_aligned_3x3(g, 256) && fits;
    p.family = slab ? VKAS_NT_SLAB : VKAS_NT_TILE256;
    p.buf = slab || (!sw.nt_nobuf && fits);
    p.grid_m = slab ? M / 256 : cdiv(M, 256);
    return p;
  }
  // Ring depth of gemm_nt_ring_kernel (0 = the register-staged kernel; the ring addresses its operands with 32-bit buffer
  // offsets).  At most one round of workgroups (<= 256 tiles): four stages (128 KB of LDS, one workgroup per CU, three K tiles in
  // flight) - the launch lasts as long as one workgroup's K loop; more tiles: two stages, so that two workgroups share a CU and
  // one's prologue / epilogue sits behind the other's K loop (profiles/sweep_small.py: 4 stages 26.6 / 37.1 us against 31.7 /
  // 52.1 at M = 7 168, N = 512, K = 2 048 / M = 1 792, N = 1 024, K = 4 096; 2 stages 34.2 against 44.3 at M = 7 168,
  // N = 2 048, K = 512; the register-staged kernel: 42.2, 70.2 and 40.0).
  p.grid_m = cdiv(M, 128);
  if (fits) p.ring = sw.nt_ring < 0 ? (p.grid_m * p.grid_n <= 256 ? 4 : 2) : (sw.nt_ring >= 2 && sw.nt_ring <= 4 ? sw.nt_ring : 0);
  p.family = p.ring ? VKAS_NT_RING : VKAS_NT_REG128;
  p.buf = p.ring || (!sw.nt_nobuf && fits);
  return p;
}

vkas_tn_plan vkas_plan_tn(const vkas_conv_geom& g, int Np, long lddy, int flags, bool has_gb, const vkas_gemm_switches& sw) {
  const long M = (long)g.B * g.Hout * g.Wout;
  const int K = g.KH * g.KW * g.Cp;
  const bool one_split = (flags & 2) != 0;
  vkas_tn_plan p = {};
  p.xg = (flags & 1) != 0;
  p.x_bytes = vkas_span_bytes((long)g.B * g.Hin * g.Win, g.ldx, g.Cp);
  p.dy_bytes = vkas_span_bytes(M, lddy, Np);
  const bool fits = vkas_fits_buffer(p.x_bytes) && vkas_fits_buffer(p.dy_bytes);
  // conv3x3_wgrad_slab_kernel: rows of whole 64-pixel chunks, at least one full n tile and channel block, plain entry only
  if (!p.xg && !one_split && !sw.tn_noslab && row_aligned_3x3(g, 64) && M >= 65536 && Np >= 112 && g.Cp >= 128 && fits) {
    p.family = VKAS_TN_SLAB;
    p.buf = true;
    // the N extent that pads least; 96 only where it beats both wider ones (N = 192: no padding against 224 / 256 columns)
    p.tile = padded(Np, 112) < padded(Np, 128) ? 112 : 128;
    if (!sw.tn_no96 && padded(Np, 96) < padded(Np, 112) && padded(Np, 96) < padded(Np, 128)) p.tile = 96;
    p.tiles = cdiv(Np, p.tile) * 3 * cdiv(g.Cp, 128);
    const long chunks = M / VKAS_TN_ROWS;
    // Pixel splits: whole splits per XCD (multiple of 8).  The tiles of one split walk the same dy / x chunks at the same
    // time and share them through that XCD's L2 (every operand byte is used by 9 tiles): keeping a split's tiles
    // together matters more than filling the last round of workgroups (a round-balanced, XCD-straddling split count
    // measured 5% slower).  About 3 rounds of the 256 resident workgroups, at least 16 chunks per split.
    p.splits = padded(cdiv(3 * 256, p.tiles), 8);
    if (p.splits > chunks / 16) p.splits = chunks / 16 > 0 ? chunks / 16 : 1;
    p.rows = cdiv(chunks, p.splits);
    p.splits = cdiv(chunks, p.rows);
    p.grid = (unsigned)(p.tiles * p.splits);
    return p;
  }
  p.tile = vkas_tn_tile_rule(M, Np, K, sw);
  const bool waves8 = p.tile != 128;
  const int bkc = p.tile == 192 || p.tile == 224 ? 256 : 128;  // K columns of the tile
  p.tiles = cdiv(Np, p.tile) * cdiv(K, bkc);
  // Splits over M: pick the count that minimises a two-term cost model.
  //   main loop: rounds of resident workgroups (256 CUs x 1 block of 8 waves | 2 blocks of 4) x 64-row iterations of a
  //     split x time per iteration (measured: ~1.2 us for the 8-wave tiles, ~0.5 us for the 4-wave tile);
  //   reduction: every split adds a full copy of its tile with fp32 atomics, ~1.3 TB/s chip-wide (MI355X_MICROARCH.md).
  // On the stage-3/4 weight gradients (M = 16-64 K rows) the atomic tail was half the launch with the old "3 rounds"
  // rule.  Ties go to multiples of 8 (whole splits per XCD, see the kernel's work order).
  const long resident = 256L * (waves8 ? 1 : 2);
  const double t_iter = waves8 ? 1.2e-6 : 0.5e-6;
  const double tile_bytes = (double)p.tile * bkc * 4.0;
  // one_split: every output tile is reduced over all M rows by one workgroup, in row order, and added once to the zeroed
  // gw: the result does not depend on the order workgroups run in (vkas_conv_gemm_wgrad_ordered)
  const long max_splits = one_split ? 1 : cdiv(M, 4 * VKAS_TN_ROWS);
  p.splits = 1;
  double best_t = 1e30;
  for (long sp = 1; sp <= max_splits && sp * p.tiles <= 8 * resident; ++sp) {
    const long blocks = sp * p.tiles;
    const double t = (double)cdiv(blocks, resident) * (double)cdiv(cdiv(M, sp), VKAS_TN_ROWS) * t_iter +
                     (double)blocks * tile_bytes / 1.3e12;
    if (t < best_t * (sp % 8 == 0 ? 1.02 : 0.999)) {
      best_t = t;
      p.splits = sp;
    }
  }
  if (p.splits > 65535) p.splits = 65535;
  p.rows = padded(cdiv(M > 0 ? M : 1, p.splits), VKAS_TN_ROWS);
  p.splits = cdiv(M > 0 ? M : 1, p.rows);
  p.grid = (unsigned)(p.tiles * p.splits);
  const bool pointwise = g.KH == 1 && g.KW == 1 && g.stride == 1 && g.pad == 0 && g.Hin == g.Hout && g.Win == g.Wout;
  p.buf = !sw.tn_nobuf && fits;
  p.pw = p.buf && pointwise;
  p.nobias = p.pw && !has_gb && !p.xg && (p.tile == 192 || p.tile == 384);  // instantiated for the 96-column wave tile only
  return p;
}
