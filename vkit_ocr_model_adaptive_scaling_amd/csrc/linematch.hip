// Scoring detected text lines against annotated ones with one-to-one matches, splits and merges (inferencing/
// line_evaluation.py holds the rule and the host oracles match_lines_host / match_lines_rounds_host; the rule is this
// project's own).  rows (B, K, 16) int32 are the match rows of quadmatch.hip.  Four launches on one stream: the three pair
// passes of quad_pairs.h under LmRule - lm_pair_kernel<false>, lm_scan_kernel, lm_pair_kernel<true> - then the phases
// (line_phases.h, shared with ribbonmatch.hip).
#include "line_phases.h"

extern "C" long long vkas_line_match_workspace_bytes(int B, int M, int N, int max_pairs) {
  if (qp_check_dims("vkas_line_match_workspace_bytes", B, M, N, max_pairs) != VKAS_OK) return -1;
  return (long long)lm_layout(B, M, N, max_pairs).bytes;
}

extern "C" int vkas_line_match(const int* gt_rows, const int* gt_count, const unsigned char* gt_care, const int* pred_rows,
                               const int* pred_count, int B, int M, int N, int tr_q8, int tp_q8, double cover_thr,
                               int max_pairs, void* workspace, size_t workspace_bytes, unsigned char* gt_kind, int* gt_group,
                               unsigned char* pred_kind, int* pred_group, long long* stats, int* rounds, void* stream) {
  const int rc = lm_check_args("vkas_line_match", gt_rows, gt_count, pred_rows, pred_count, B, M, N, tr_q8, tp_q8, cover_thr,
                               max_pairs, workspace, workspace_bytes, gt_kind, gt_group, pred_kind, pred_group, stats);
  if (rc != VKAS_OK || B == 0) return rc;
  const LmLayout l = lm_layout(B, M, N, max_pairs);
  // the phases keep 14 bytes per pred and 3 per gt in LDS
  const size_t lds = lm_lds_bytes(M, N);
  if (const int e = qp_allow_lds<lm_phase_kernel>("vkas_line_match", lds, lm_lds_bytes(QM_MAX, QM_MAX))) return e;
  const QpTables t = qp_tables(gt_rows, gt_count, pred_rows, pred_count, M, N, max_pairs, workspace, l);
  const LmRule r{{}, gt_care, tr_q8, tp_q8, cover_thr, qp_at<unsigned long long>(workspace, l.cover), stats,
                 qp_at<unsigned long long>(workspace, l.cand)};
  unsigned long long* ignored = qp_at<unsigned long long>(workspace, l.ignored);
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  lm_pair_kernel<false><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("line_match pairs");
  lm_scan_kernel<<<B, QM_BLOCK, 0, s>>>(t, r, ignored);
  VKAS_LAUNCH_CHECK("line_match scan");
  lm_pair_kernel<true><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("line_match fill");
  lm_phase_kernel<<<B, QM_BLOCK, lds, s>>>(gt_rows, gt_count, gt_care, pred_rows, pred_count, M, N, l.Mp, l.NT, tr_q8, tp_q8,
                                           ignored, t.rowoff, r.cand, max_pairs, gt_kind, gt_group, pred_kind, pred_group,
                                           stats, rounds);
  VKAS_LAUNCH_CHECK("line_match rounds");
  return VKAS_OK;
}
