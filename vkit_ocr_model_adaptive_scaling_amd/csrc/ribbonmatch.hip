// Scoring curved text lines as ribbons of quads (inferencing/ribbon_evaluation.py holds the rule - this project's own - and
// the host oracles match_ribbons_host / match_ribbons_rounds_host).  A ribbon row (B, K, 16) int32 names a run of rows of
// its image's segment table (B, S, 16): word 0 = seg_start, word 1 = seg_count in 1..256, words 8..11 the union of the
// segment boxes, 12..13 the sum of their areas, 14 valid.  A segment row is a match row of quadmatch.hip.  Four launches on
// one stream, those of linematch.hip: the tile body of quad_pairs.h under RbRule - rb_pair_kernel<false>, lm_scan_kernel,
// rb_pair_kernel<true> - then lm_phase_kernel (line_phases.h: the scan and the phases read the count, valid, area and care
// words only, which a ribbon row holds where a match row does).
//
//   RbRule   LmRule with PAIR_LANES = 64: a listed pair of ribbons is the work of one wave.  Its lanes stride over the
//            seg_count_g * seg_count_p segment pairs, read the two segment boxes and valid words from global memory and, where both are valid and
//            the boxes overlap, clip the two segment rows with qm_inter2_iou as it is (ring slots per thread in LDS, row
//            pointers into the segment tables) and add floor(min(inter2, 2^41)) in int64.  The wave sum (shuffles; integer,
//            so order-free), clamped to 2^41, is I; as a double it is exact, and LmRule's pair test takes it in place of
//            inter2: its floor and clamp change nothing, and the coverage test of a don't-care gt sees float(I).
//
// seg_start and seg_count are checked against S before any use as an index: a ribbon row whose run is not inside its
// image's table, or whose count is outside 1..256, has no segments (I = 0) and still takes part as its valid word says.
// Segment reads are thereby bounded by the tables; everything else is bounded as in quad_pairs.h.  The fill pass computes
// I again for the candidates only, by the same code: the same bits.
#include "line_phases.h"

namespace {

constexpr int RB_SEG_MAX = 256;        // segments of a ribbon
constexpr int RB_TABLE_MAX = 1 << 21;  // rows of an image's segment table

struct RbRule : LmRule {
  static constexpr int PAIR_LANES = 64;  // a whole wave; 16 lanes a pair were measured too: 1.6x slower at 10 segments
  const int* gt_segs;    // (B, Sg, 16)
  const int* pred_segs;  // (B, Sp, 16)
  int Sg, Sp;
  // the run of a ribbon row in a table of S rows -> its count, 0 for a run the table does not hold
  __device__ __forceinline__ static int run(const int4& part0, int S, int& start) {
    const int s = part0.x, c = part0.y;
    const bool ok = c >= 1 && c <= RB_SEG_MAX && s >= 0 && s <= S - c;  // S >= 1 and c >= 1: no overflow
    start = ok ? s : 0;
    return ok ? c : 0;
  }
  __device__ __forceinline__ double group_inter2(const int4* g, const int4* p, int b, double* ring, int lane) const {
    int gs, ps;
    const int gc = run(g[0], Sg, gs), pc = run(p[0], Sp, ps);
    const int4* gseg = reinterpret_cast<const int4*>(gt_segs) + ((long)b * Sg + gs) * 4;
    const int4* pseg = reinterpret_cast<const int4*>(pred_segs) + ((long)b * Sp + ps) * 4;
    long sum = 0;
    for (int e = lane; e < gc * pc; e += PAIR_LANES) {  // <= 2^16 segment pairs
      const int i = e / pc, j = e - i * pc;     // i < gc, j < pc: inside the two runs
      const int4* gq = gseg + i * 4;
      const int4* pq = pseg + j * 4;
      const int4 gb = gq[2], pb = pq[2];
      if (!(gb.x <= pb.z && pb.x <= gb.z && gb.y <= pb.w && pb.y <= gb.w)) continue;
      if (gq[3].z == 0 || pq[3].z == 0) continue;
      double inter2;
      qm_inter2_iou(gq, pq, ring, &inter2);
      sum += (long)__builtin_floor(inter2 < (double)LM_AREA_MAX ? inter2 : (double)LM_AREA_MAX);  // <= 2^16 * 2^41 in all
    }
#pragma unroll
    for (int o = PAIR_LANES / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, PAIR_LANES);
    return (double)min(sum, LM_AREA_MAX);  // an integer <= 2^41: exact
  }
};

template <bool FILL>
__global__ __launch_bounds__(QM_THREADS) void rb_pair_kernel(const QpTables t, const RbRule r) {
  qp_tile<FILL>(t, r);
}

}  // namespace

extern "C" long long vkas_ribbon_match_workspace_bytes(int B, int M, int N, int max_pairs) {
  if (qp_check_dims("vkas_ribbon_match_workspace_bytes", B, M, N, max_pairs) != VKAS_OK) return -1;
  return (long long)lm_layout(B, M, N, max_pairs).bytes;
}

extern "C" int vkas_ribbon_match(const int* gt_rows, const int* gt_count, const unsigned char* gt_care, const int* gt_segs,
                                 int Sg, const int* pred_rows, const int* pred_count, const int* pred_segs, int Sp, int B,
                                 int M, int N, int tr_q8, int tp_q8, double cover_thr, int max_pairs, void* workspace,
                                 size_t workspace_bytes, unsigned char* gt_kind, int* gt_group, unsigned char* pred_kind,
                                 int* pred_group, long long* stats, int* rounds, void* stream) {
  const char* what = "vkas_ribbon_match";
  VKAS_CHECK(Sg >= 1 && Sg <= RB_TABLE_MAX && Sp >= 1 && Sp <= RB_TABLE_MAX, "%s: Sg=%d and Sp=%d must lie in 1..%d", what, Sg,
             Sp, RB_TABLE_MAX);
  const int rc = lm_check_args(what, gt_rows, gt_count, pred_rows, pred_count, B, M, N, tr_q8, tp_q8, cover_thr, max_pairs,
                               workspace, workspace_bytes, gt_kind, gt_group, pred_kind, pred_group, stats);
  if (rc != VKAS_OK || B == 0) return rc;
  VKAS_CHECK(gt_segs && pred_segs, "%s: null pointer", what);
  VKAS_CHECK(vkas_aligned16(gt_segs) && vkas_aligned16(pred_segs), "%s: the segment tables must be 16-byte aligned", what);
  const LmLayout l = lm_layout(B, M, N, max_pairs);
  const size_t lds = lm_lds_bytes(M, N);
  if (const int e = qp_allow_lds<lm_phase_kernel>(what, lds, lm_lds_bytes(QM_MAX, QM_MAX))) return e;
  const QpTables t = qp_tables(gt_rows, gt_count, pred_rows, pred_count, M, N, max_pairs, workspace, l);
  const RbRule r{{{}, gt_care, tr_q8, tp_q8, cover_thr, qp_at<unsigned long long>(workspace, l.cover), stats,
                  qp_at<unsigned long long>(workspace, l.cand)},
                 gt_segs, pred_segs, Sg, Sp};
  unsigned long long* ignored = qp_at<unsigned long long>(workspace, l.ignored);
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  rb_pair_kernel<false><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("ribbon_match pairs");
  lm_scan_kernel<<<B, QM_BLOCK, 0, s>>>(t, r, ignored);
  VKAS_LAUNCH_CHECK("ribbon_match scan");
  rb_pair_kernel<true><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("ribbon_match fill");
  lm_phase_kernel<<<B, QM_BLOCK, lds, s>>>(gt_rows, gt_count, gt_care, pred_rows, pred_count, M, N, l.Mp, l.NT, tr_q8, tp_q8,
                                           ignored, t.rowoff, r.cand, max_pairs, gt_kind, gt_group, pred_kind, pred_group,
                                           stats, rounds);
  VKAS_LAUNCH_CHECK("ribbon_match rounds");
  return VKAS_OK;
}
