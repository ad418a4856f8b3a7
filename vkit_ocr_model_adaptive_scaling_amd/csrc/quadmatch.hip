// Matching predicted character quadrilaterals to annotated ones by IoU (inferencing/evaluation.py holds the rule and the host
// oracles quad_iou_host / match_quads_host; the rule is this project's own).  rows (B, K, 16) int32: Q4 corners (8), the
// inclusive Q4 box (4), twice the area as int64 (2), valid, zero.  Four launches on one stream: the three pair passes of
// quad_pairs.h - qm_pair_kernel<false>, qm_scan_kernel, qm_pair_kernel<true> - under the rule of the op, then its rounds:
//
//   QmMatchRule  (vkas_quad_match)  a pair at or above iou_thr is a candidate; its slot holds the pred and the iou bits.
//                qm_match_kernel: one workgroup per image, mutual-best rounds on integer atomicMax / atomicMin in LDS.
//   QmSelfRule   (vkas_quad_nms; inferencing/nms.py holds the rule and the oracle nms_quads_host)  one table against itself:
//                the row that is judged in the gt's place, the row that may suppress it in the pred's.  A row takes part iff
//                it is valid and its prob is finite, and a pair only where the pred outranks the gt (the higher float32
//                prob, then the lower index): the diagonal and one of (i, j), (j, i) drop out before the clip.  The prob
//                bits travel in the row's zero word in LDS; a slot holds the pred alone.  qn_rounds_kernel: one workgroup
//                per image.
//   QrRule       (vkas_quad_match_ranked; inferencing/ranking.py holds the rule and the oracles)  T IoU thresholds with
//                don't-care annotations; the passes run at iou_thrs[0].  A pred takes part iff it is valid and its prob is
//                finite; the care flag rides in the gt row's zero word.  In the counting pass a pair with a don't-care gt is
//                clipped for the coverage test alone and sets the pred's bit of the tile's cover word instead of a candidate
//                bit, and a care pair is counted at every threshold it reaches; the fill never meets a don't-care gt, whose
//                words are zero.  qr_rounds_kernel: one workgroup per (image, threshold), all of them walking the one
//                candidate list.
//
// qm_rows_kernel (vkas_quad_rows) is inferencing.match_rows on the device.
#include "quad_pairs.h"

namespace {

constexpr int QM_STATS = 6;                // tp, n_gt, n_pred, pairs, candidates, status
constexpr int QR_STATS = 8;                // ranked: tp, fp, ignored, n_gt, n_pred, pairs, candidates, status
constexpr int QR_TMAX = 16;                // ranked: IoU thresholds per call
constexpr unsigned long long QM_TAKEN = ~0ull;

// What only the ranked matching passes to the shared passes and to its rounds.
struct QrArgs {
  const unsigned char* gt_care;  // (B, M), 0 = don't care; null = every gt is a care gt
  unsigned long long* cover;     // (B, MT * NT): per tile, bit j = pred j of the tile is covered by a don't-care gt of the tile
  int* tile_info;                // (B, MT * NT, 1 + T): the tile's don't-care pairs, its candidates at each threshold
  double cover_thr;
  int T;
  double thr[QR_TMAX];           // ascending; thr[0] is the threshold of the three passes
};

// ---- the rules (quad_pairs.h says what each member is for) ---------------------------------------------------------------

__device__ __forceinline__ unsigned long long qm_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
// a row that takes part in the self and the ranked matching: valid, and its prob finite
__device__ __forceinline__ bool qm_ranked_part(const int* rows, const float* probs, int K, int b, int i) {
  return qp_valid(rows, K, b, i) && qm_finite_bits(__float_as_uint(probs[(long)b * K + i]));
}

// stats (B, 6): words 1..5 are the scan's - n_gt, n_pred (the valid rows within the counts), pairs, candidates, status
struct QmMatchRule : QpRule {
  double thr;
  long long* stats;
  int* cand_pred;               // (B, max_pairs)
  unsigned long long* cand_iou; // (B, max_pairs)
  __device__ __forceinline__ long long status(int b) const { return stats[(long)b * QM_STATS + 5]; }
  template <bool FILL>
  __device__ __forceinline__ bool pair(Tile&, const int4&, const int4&, int, double iou, double, unsigned long long& val) const {
    val = qm_bits(iou);
    return iou >= thr;
  }
  __device__ __forceinline__ void store(long at, int pred, unsigned long long val) const {
    cand_pred[at] = pred;
    cand_iou[at] = val;
  }
  __device__ __forceinline__ bool gt_part(const QpTables& t, int b, int g) const { return qp_valid(t.gt_rows, t.M, b, g); }
  __device__ __forceinline__ bool pred_part(const QpTables& t, int b, int p) const { return qp_valid(t.pred_rows, t.N, b, p); }
};

// stats (B, 6): kept (written by the rounds), n = the clamped count, n_valid = the rows that take part, pairs, candidates,
// status.  M == N: one table, one count.
struct QmSelfRule : QpRule {
  double thr;
  long long* stats;
  const float* probs;  // (B, K)
  int* cand;           // (B, max_pairs)
  __device__ __forceinline__ void fix(int4& v, bool, int b, int M, int, int at, int part) const {
    if (part == 3) qp_fix_prob(v, probs, (long)b * M + at);
  }
  __device__ __forceinline__ bool admit(const int4& g3, const int4& p3, int g, int p) const {
    const float gprob = __int_as_float(g3.w), pprob = __int_as_float(p3.w);
    return pprob > gprob || (pprob == gprob && p < g);
  }
  __device__ __forceinline__ long long status(int b) const { return stats[(long)b * QM_STATS + 5]; }
  template <bool FILL>
  __device__ __forceinline__ bool pair(Tile&, const int4&, const int4&, int, double iou, double, unsigned long long&) const {
    return iou >= thr;
  }
  __device__ __forceinline__ void store(long at, int pred, unsigned long long) const { cand[at] = pred; }
  __device__ __forceinline__ bool gt_part(const QpTables&, int, int) const { return true; }
  __device__ __forceinline__ bool pred_part(const QpTables& t, int b, int p) const {
    return qm_ranked_part(t.pred_rows, probs, t.N, b, p);
  }
};

struct QrRule : QpRule {
  QrArgs x;
  const float* probs;  // (B, N)
  long long* stats;    // (B, T, 8)
  int* cand_pred;
  unsigned long long* cand_iou;
  struct Tile {
    unsigned long long cover;
    int dc;            // the tile's pairs with a don't-care gt
    int ct[QR_TMAX];   // its candidates at each threshold
  };
  __device__ __forceinline__ void begin(Tile& s, int tid) const {
    if (tid == 0) {
      s.cover = 0ull;
      s.dc = 0;
    }
    if (tid < QR_TMAX) s.ct[tid] = 0;
  }
  __device__ __forceinline__ void fix(int4& v, bool is_gt, int b, int M, int N, int at, int part) const {
    if (part != 3) return;
    if (is_gt) qp_fix_care(v, x.gt_care, (long)b * M + at);
    else qp_fix_prob(v, probs, (long)b * N + at);
  }
  __device__ __forceinline__ long long status(int b) const { return stats[(long)b * x.T * QR_STATS + 7]; }
  template <bool FILL>
  __device__ __forceinline__ bool pair(Tile& s, const int4& g3, const int4& p3, int pj, double iou, double inter2,
                                       unsigned long long& val) const {
    if (!FILL) {
      if (g3.w == 0) {  // a don't-care gt: the coverage test, never a candidate
        atomicAdd(&s.dc, 1);
        if (qp_covers(x.cover_thr, inter2, p3)) atomicOr(&s.cover, 1ull << pj);
        return false;
      }
      for (int t = 0; t < x.T; ++t)
        if (iou >= x.thr[t]) atomicAdd(&s.ct[t], 1);
    }
    val = qm_bits(iou);
    return iou >= x.thr[0];
  }
  __device__ __forceinline__ void store(long at, int pred, unsigned long long val) const {
    cand_pred[at] = pred;
    cand_iou[at] = val;
  }
  __device__ __forceinline__ int apart(const Tile& s) const { return s.dc; }  // pairs counts the care pairs alone
  __device__ __forceinline__ void tile_out(const Tile& s, long tile, int tid) const {
    if (tid == 0) {
      x.cover[tile] = s.cover;
      x.tile_info[tile * (1 + x.T)] = s.dc;
    }
    if (tid < x.T) x.tile_info[tile * (1 + x.T) + 1 + tid] = s.ct[tid];
  }
};

template <bool FILL, class Rule>
__global__ __launch_bounds__(QM_THREADS) void qm_pair_kernel(const QpTables t, const Rule r) {
  qp_tile<FILL>(t, r);
}

// the one-to-one and the self matching
template <class Rule>
__global__ __launch_bounds__(QM_BLOCK) void qm_scan_kernel(const QpTables t, const Rule r) {
  __shared__ int s_sum[3];  // n_gt, n_pred, pairs
  const int tid = threadIdx.x, b = blockIdx.x;
  const int ng = qm_clamp(t.gt_count[b], t.M), np = qm_clamp(t.pred_count[b], t.N);
  if (tid < 3) s_sum[tid] = 0;
  int sums[2] = {0, 0};
  for (int g = tid; g < ng; g += QM_BLOCK) sums[0] += r.gt_part(t, b, g);
  for (int p = tid; p < np; p += QM_BLOCK) sums[1] += r.pred_part(t, b, p);
  const int all = qp_scan(t, b, nullptr, sums, s_sum);
  if (tid == 0) {
    long long* st = r.stats + (long)b * QM_STATS;
    st[0] = 0;
    st[1] = s_sum[0];
    st[2] = s_sum[1];
    st[3] = s_sum[2];
    st[4] = all;
    st[5] = all > t.max_pairs ? 1 : 0;
  }
}

// The ranked matching: stats (B, T, 8) words 3..7 of every threshold = n_gt (care gts), n_pred, pairs (care), the candidates
// at that threshold, status; covered (B, N) = the OR of the tiles' cover words down the gt tiles; dc_stats (B, 3) = n_dc,
// dc_pairs, n_covered.  Words 0..2 are the rounds'.
__global__ __launch_bounds__(QM_BLOCK) void qm_scan_kernel(const QpTables t, const QrRule r, unsigned char* __restrict__ covered,
                                                            long long* __restrict__ dc_stats) {
  __shared__ int s_sum[3];              // n_gt, n_pred, pairs
  __shared__ int s_more[3 + QR_TMAX];   // n_dc, dc_pairs, n_covered, candidates at t
  __shared__ unsigned long long s_cov[QM_MAX / QM_TILE];
  const QrArgs& x = r.x;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x, M = t.M, N = t.N, tiles = t.MT * t.NT;
  const int ng = qm_clamp(t.gt_count[b], M), np = qm_clamp(t.pred_count[b], N);
  if (tid < 3) s_sum[tid] = 0;
  if (tid < 3 + QR_TMAX) s_more[tid] = 0;
  if (tid < t.NT) {  // NT <= QM_MAX / QM_TILE
    unsigned long long w = 0ull;
    for (int tm = 0; tm < t.MT; ++tm) w |= x.cover[((long)b * t.MT + tm) * t.NT + tid];
    s_cov[tid] = w;
  }
  __syncthreads();
  int sums[2] = {0, 0}, n_dc = 0, n_cov = 0;
  for (int g = tid; g < ng; g += QM_BLOCK) {
    const bool part = qp_valid(t.gt_rows, M, b, g), care = !x.gt_care || x.gt_care[(long)b * M + g] != 0;
    sums[0] += part && care;
    n_dc += part && !care;
  }
  for (int p = tid; p < np; p += QM_BLOCK) sums[1] += qm_ranked_part(t.pred_rows, r.probs, N, b, p);
  for (int p = tid; p < N; p += QM_BLOCK) {
    const int c = (int)((s_cov[p >> 6] >> (p & 63)) & 1ull);
    covered[(long)b * N + p] = (unsigned char)c;
    n_cov += c;
  }
  n_dc = qm_wave_sum_i(n_dc);
  n_cov = qm_wave_sum_i(n_cov);
  if (lane == 0) {
    atomicAdd(&s_more[0], n_dc);
    atomicAdd(&s_more[2], n_cov);
  }
  for (int k = 0; k < 1 + x.T; ++k) {  // the tiles' don't-care pairs (k = 0) and candidates at threshold k - 1
    int v = 0;
    for (int i = tid; i < tiles; i += QM_BLOCK) v += x.tile_info[((long)b * tiles + i) * (1 + x.T) + k];
    v = qm_wave_sum_i(v);
    if (lane == 0) atomicAdd(&s_more[k == 0 ? 1 : 2 + k], v);
  }
  const int all = qp_scan(t, b, nullptr, sums, s_sum);
  if (tid == 0)
    for (int k = 0; k < 3; ++k) dc_stats[(long)b * 3 + k] = s_more[k];
  if (tid < x.T) {
    long long* st = r.stats + ((long)b * x.T + tid) * QR_STATS;
    st[3] = s_sum[0];
    st[4] = s_sum[1];
    st[5] = s_sum[2];
    st[6] = s_more[3 + tid];
    st[7] = all > t.max_pairs ? 1 : 0;
  }
}

// Mutual-best rounds.  Thread t owns the gts t + 1024 k (k < 8: one taken bit each, in a register); per pred the LDS holds the
// best iou bits offered this round (QM_TAKEN once the pred is matched: no offer exceeds it, no offer equals it) and the lowest
// gt that offers them.  Integer max / min only: the result does not depend on arrival order.
__global__ __launch_bounds__(QM_BLOCK) void qm_match_kernel(const int* __restrict__ gt_count, const int* __restrict__ pred_count,
                                                             int M, int N, int Mp, const int* __restrict__ rowoff,
                                                             const int* __restrict__ cand_pred,
                                                             const unsigned long long* __restrict__ cand_iou, int max_pairs,
                                                             int* __restrict__ gt_match, int* __restrict__ pred_match,
                                                             double* __restrict__ gt_iou, long long* __restrict__ stats,
                                                             int* __restrict__ rounds) {
  extern __shared__ unsigned long long s_dyn[];
  __shared__ int s_any, s_tp;
  unsigned long long* best_iou = s_dyn;                  // N
  int* best_gt = reinterpret_cast<int*>(s_dyn + N);      // N
  const int t = threadIdx.x, b = blockIdx.x;
  static_assert(QM_MAX <= QM_BLOCK * 32, "one taken bit per owned gt");
  for (int g = t; g < M; g += QM_BLOCK) {
    gt_match[(long)b * M + g] = -1;
    gt_iou[(long)b * M + g] = 0.0;
  }
  for (int p = t; p < N; p += QM_BLOCK) {
    pred_match[(long)b * N + p] = -1;
    best_iou[p] = 0ull;
  }
  if (t == 0) s_tp = 0;
  int done = 0;
  if (stats[(long)b * QM_STATS + 5] == 0) {  // uniform over the workgroup; an overflowed image keeps every match at -1
    const int ng = qm_clamp(gt_count[b], M);
    const int* off = rowoff + (long)b * (Mp + 1);
    const int* cp = cand_pred + (long)b * max_pairs;
    const unsigned long long* cw = cand_iou + (long)b * max_pairs;
    unsigned taken = 0;
    const int cap = min(M, N) + 1;
    for (int round = 0; round < cap; ++round) {
      for (int p = t; p < N; p += QM_BLOCK) {
        if (best_iou[p] != QM_TAKEN) best_iou[p] = 0ull;
        best_gt[p] = INT_MAX;
      }
      if (t == 0) s_any = 0;
      __syncthreads();
      for (int g = t, k = 0; g < ng; g += QM_BLOCK, ++k) {  // every free gt offers its iou to its free candidates
        if ((taken >> k) & 1u) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        for (int i = lo; i < hi; ++i) {
          const int p = cp[i];
          if ((unsigned)p < (unsigned)N && best_iou[p] != QM_TAKEN) atomicMax(&best_iou[p], cw[i]);
        }
      }
      __syncthreads();
      for (int g = t, k = 0; g < ng; g += QM_BLOCK, ++k) {  // the gts that offered a pred's best: the lowest of them
        if ((taken >> k) & 1u) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        for (int i = lo; i < hi; ++i) {
          const int p = cp[i];
          if ((unsigned)p < (unsigned)N && best_iou[p] == cw[i]) atomicMin(&best_gt[p], g);
        }
      }
      __syncthreads();
      for (int g = t, k = 0; g < ng; g += QM_BLOCK, ++k) {  // a gt takes its own best if it is that pred's best
        if ((taken >> k) & 1u) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        unsigned long long bw = 0ull;
        int bp = -1;
        for (int i = lo; i < hi; ++i) {
          const int p = cp[i];
          if ((unsigned)p < (unsigned)N && best_iou[p] != QM_TAKEN && cw[i] > bw) {  // strictly: the lowest p of a tie
            bw = cw[i];
            bp = p;
          }
        }
        if (bp >= 0 && best_gt[bp] == g) {
          taken |= 1u << k;
          gt_match[(long)b * M + g] = bp;
          gt_iou[(long)b * M + g] = __longlong_as_double((long long)bw);
          pred_match[(long)b * N + bp] = g;
          best_gt[bp] = -1 - g;  // only this thread holds best_gt[bp] == g: marks the pred for the sweep below
          atomicAdd(&s_tp, 1);
          s_any = 1;
        }
      }
      __syncthreads();
      for (int p = t; p < N; p += QM_BLOCK)
        if (best_gt[p] < 0) best_iou[p] = QM_TAKEN;
      const int any = s_any;
      __syncthreads();
      if (!any) break;
      ++done;
    }
  }
  __syncthreads();
  if (t == 0) {
    stats[(long)b * QM_STATS + 0] = s_tp;
    if (rounds) rounds[b] = done;
  }
}

// ---- ranked matching (inferencing/ranking.py holds the rule and the host oracles) ------------------------------------

constexpr unsigned char QR_ABSENT = 0, QR_TP = 1, QR_FP = 2, QR_IGNORED = 3, QR_UNDECIDED = 4;  // the last never leaves
constexpr unsigned short QR_NONE = 0xffff;

__host__ __device__ constexpr size_t qr_lds_bytes(int M, int N) {
  return (size_t)N * (sizeof(unsigned long long) + sizeof(int) + 2) + (size_t)M * (sizeof(unsigned short) + 1);
}

// The rounds of the ranked matching, one workgroup per (image, threshold); every threshold walks the image's one CSR (gt
// major, preds ascending) and skips the candidates below its own threshold.  Thread t owns the gts and the preds
// t + 1024 k.  Per gt the LDS holds a free byte and `want`: while free, the top-ranked undecided pred among its candidates
// (its row is its owner's, so this is a plain loop and a plain store; the probs come from global memory, where the
// candidates come from as well), once taken, the pred that took it.  Per pred: the state, a blocked byte (some free
// candidate wants another pred; every writer stores 1), and the best free candidate as iou bits by atomicMax and the lowest
// gt that offers them by atomicMin, as in qm_match_kernel.  A round reads the states and free bytes the previous round
// left and changes them only in its last step, between barriers: what it decides, and the count of rounds, do not depend
// on the order in which threads run.  An undecided pred that is not blocked takes its best free candidate or none; two of
// them cannot want one gt, because that gt wants only one.  The top-ranked undecided pred is never blocked, so the loop
// ends within n rounds (the cap n + 1 bounds it whatever the tables hold).  The last sweep writes every output.
__global__ __launch_bounds__(QM_BLOCK) void qr_rounds_kernel(const int* __restrict__ gt_count, const int* __restrict__ pred_rows,
                                                              const int* __restrict__ pred_count,
                                                              const float* __restrict__ probs,
                                                              const unsigned char* __restrict__ covered, int M, int N, int Mp,
                                                              const QrArgs x, const int* __restrict__ rowoff,
                                                              const int* __restrict__ cand_pred,
                                                              const unsigned long long* __restrict__ cand_iou, int max_pairs,
                                                              int* __restrict__ pred_match,
                                                              unsigned char* __restrict__ pred_state,
                                                              int* __restrict__ gt_match, double* __restrict__ pred_iou,
                                                              long long* __restrict__ stats, int* __restrict__ rounds) {
  extern __shared__ unsigned long long s_dyn[];
  __shared__ int s_any, s_out[3];
  unsigned long long* best_iou = s_dyn;                              // N
  int* best_gt = reinterpret_cast<int*>(s_dyn + N);                  // N
  unsigned short* want = reinterpret_cast<unsigned short*>(best_gt + N);  // M
  unsigned char* state = reinterpret_cast<unsigned char*>(want + M);  // N
  unsigned char* blocked = state + N;                                // N
  unsigned char* free_gt = blocked + N;                              // M
  static_assert(QM_MAX < QR_NONE, "a pred index fits want");
  const int t = threadIdx.x;
  const long bt = blockIdx.x;
  const int b = (int)(bt / x.T), ti = (int)(bt % x.T);
  const double thr = x.thr[ti];
  const int ng = qm_clamp(gt_count[b], M), np = qm_clamp(pred_count[b], N);
  const bool over = stats[bt * QR_STATS + 7] != 0;  // uniform: an overflowed image gets every state 0 and every match -1
  const int* off = rowoff + (long)b * (Mp + 1);
  const int* cp = cand_pred + (long)b * max_pairs;
  const unsigned long long* cw = cand_iou + (long)b * max_pairs;
  const float* pr = probs + (long)b * N;
  for (int p = t; p < N; p += QM_BLOCK) {
    const bool part = !over && p < np && pred_rows[((long)b * N + p) * 16 + 14] != 0 && qm_finite_bits(__float_as_uint(pr[p]));
    state[p] = part ? QR_UNDECIDED : QR_ABSENT;
    blocked[p] = 0;
    best_iou[p] = 0ull;
    best_gt[p] = INT_MAX;
  }
  for (int g = t; g < M; g += QM_BLOCK) {
    free_gt[g] = 1;
    want[g] = QR_NONE;
  }
  if (t < 3) s_out[t] = 0;
  int done = 0;
  if (!over) {
    for (int round = 0; round < np + 1; ++round) {
      for (int p = t; p < N; p += QM_BLOCK) {  // the owner's own preds
        if (state[p] != QR_UNDECIDED) continue;
        blocked[p] = 0;
        best_iou[p] = 0ull;
        best_gt[p] = INT_MAX;
      }
      if (t == 0) s_any = 0;
      __syncthreads();
      for (int g = t; g < ng; g += QM_BLOCK) {  // what every free gt wants
        if (!free_gt[g]) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        int top = -1;
        float top_prob = 0.f;
        for (int i = lo; i < hi; ++i) {
          const int p = cp[i];
          if ((unsigned)p >= (unsigned)N || state[p] != QR_UNDECIDED || !(__longlong_as_double((long long)cw[i]) >= thr)) continue;
          const float pp = pr[p];
          if (top < 0 || pp > top_prob) {  // ascending p: among equal probs the first one stays
            top = p;
            top_prob = pp;
          }
        }
        want[g] = top < 0 ? QR_NONE : (unsigned short)top;
      }
      __syncthreads();
      for (int g = t; g < ng; g += QM_BLOCK) {  // blocked preds; every free gt offers its iou to its undecided candidates
        if (!free_gt[g]) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        const int w = want[g];
        for (int i = lo; i < hi; ++i) {
          const int p = cp[i];
          if ((unsigned)p >= (unsigned)N || state[p] != QR_UNDECIDED || !(__longlong_as_double((long long)cw[i]) >= thr)) continue;
          if (p != w) blocked[p] = 1;
          atomicMax(&best_iou[p], cw[i]);
        }
      }
      __syncthreads();
      for (int g = t; g < ng; g += QM_BLOCK) {  // the gts that offered a pred's best: the lowest of them
        if (!free_gt[g]) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        for (int i = lo; i < hi; ++i) {
          const int p = cp[i];
          if ((unsigned)p >= (unsigned)N || state[p] != QR_UNDECIDED || !(__longlong_as_double((long long)cw[i]) >= thr)) continue;
          if (best_iou[p] == cw[i]) atomicMin(&best_gt[p], g);
        }
      }
      __syncthreads();
      for (int p = t; p < N; p += QM_BLOCK) {  // the only step that changes a state or a free byte
        if (state[p] != QR_UNDECIDED || blocked[p]) continue;
        const int g = best_gt[p];
        if (g != INT_MAX) {  // g < ng: it came from the loop above
          state[p] = QR_TP;
          free_gt[g] = 0;
          want[g] = (unsigned short)p;
        } else {
          state[p] = covered[(long)b * N + p] ? QR_IGNORED : QR_FP;
        }
        s_any = 1;
      }
      __syncthreads();
      const int any = s_any;
      __syncthreads();
      if (!any) break;
      ++done;
    }
  }
  __syncthreads();
  int tp = 0, fp = 0, ig = 0;
  for (int p = t; p < N; p += QM_BLOCK) {
    unsigned char st = state[p];
    if (st == QR_UNDECIDED) st = QR_ABSENT;  // can be left only by tables that are not this call's own
    pred_state[bt * N + p] = st;
    pred_match[bt * N + p] = st == QR_TP ? best_gt[p] : -1;
    pred_iou[bt * N + p] = st == QR_TP ? __longlong_as_double((long long)best_iou[p]) : 0.0;
    tp += st == QR_TP;
    fp += st == QR_FP;
    ig += st == QR_IGNORED;
  }
  for (int g = t; g < M; g += QM_BLOCK) gt_match[bt * M + g] = free_gt[g] ? -1 : (int)want[g];
  tp = qm_wave_sum_i(tp);
  fp = qm_wave_sum_i(fp);
  ig = qm_wave_sum_i(ig);
  if ((t & 63) == 0) {
    atomicAdd(&s_out[0], tp);
    atomicAdd(&s_out[1], fp);
    atomicAdd(&s_out[2], ig);
  }
  __syncthreads();
  if (t < 3) stats[bt * QR_STATS + t] = s_out[t];
  if (t == 0 && rounds) rounds[bt] = done;
}

// ---- suppression (inferencing/nms.py holds the rule and the host oracle nms_quads_host) -----------------------------

constexpr unsigned char QN_UNDECIDED = 0, QN_KEPT = 1, QN_SUPPRESSED = 2, QN_APART = 3;  // APART: takes no part

// The rounds of the suppression, one workgroup per image.  The CSR row of quad i lists the quads that outrank it and overlap
// it at or above the threshold.  The state of every quad lives in LDS twice: a round reads the previous round's states
// and writes the next ones, so what a round decides - and with it the count of rounds - does not depend on the order in
// which threads run.  Thread t owns the quads t + 1024 k.  An undecided quad becomes suppressed once a neighbour is kept
// and kept once all its neighbours are suppressed; the top-ranked undecided quad can always be decided, so the loop ends
// within n rounds (the cap n + 1 bounds it whatever the tables hold).  The suppressor is read off the final states: the
// highest-ranked kept neighbour.  One integer LDS atomic (the kept count); plain stores otherwise.
__global__ __launch_bounds__(QM_BLOCK) void qn_rounds_kernel(const int* __restrict__ rows, const int* __restrict__ count,
                                                              const float* __restrict__ probs, int K, int Kp,
                                                              const int* __restrict__ rowoff,
                                                              const int* __restrict__ cand, int max_pairs,
                                                              unsigned char* __restrict__ keep, int* __restrict__ suppressor,
                                                              long long* __restrict__ stats, int* __restrict__ rounds) {
  __shared__ unsigned char s_state[2][QM_MAX];
  __shared__ int s_any, s_kept;
  const int t = threadIdx.x, b = blockIdx.x;
  const int n = qm_clamp(count[b], K);
  const int* off = rowoff + (long)b * (Kp + 1);
  const int* cp = cand + (long)b * max_pairs;
  const float* pr = probs + (long)b * K;
  if (t == 0) s_kept = 0;
  int done = 0;
  if (stats[(long)b * QM_STATS + 5] != 0) {  // uniform over the workgroup: over capacity, nothing is suppressed
    for (int i = t; i < K; i += QM_BLOCK) {
      keep[(long)b * K + i] = i < n ? 1 : 0;
      suppressor[(long)b * K + i] = -1;
    }
    __syncthreads();
    if (t == 0) {
      stats[(long)b * QM_STATS + 0] = n;
      if (rounds) rounds[b] = 0;
    }
    return;
  }
  for (int i = t; i < K; i += QM_BLOCK) {
    const bool part = i < n && rows[((long)b * K + i) * 16 + 14] != 0 && qm_finite_bits(__float_as_uint(pr[i]));
    s_state[0][i] = part ? QN_UNDECIDED : QN_APART;
  }
  int cur = 0;
  for (int round = 0; round < n + 1; ++round) {
    if (t == 0) s_any = 0;
    __syncthreads();
    const unsigned char* prev = s_state[cur];
    unsigned char* next = s_state[cur ^ 1];
    for (int i = t; i < K; i += QM_BLOCK) {
      unsigned char st = prev[i];
      if (st == QN_UNDECIDED) {
        const int lo = max(off[i], 0), hi = min(off[i + 1], max_pairs);
        bool any_kept = false, all_suppressed = true;
        for (int e = lo; e < hi; ++e) {
          const int j = cp[e];
          if ((unsigned)j >= (unsigned)K) continue;
          const unsigned char sj = prev[j];
          any_kept = any_kept || sj == QN_KEPT;
          all_suppressed = all_suppressed && sj == QN_SUPPRESSED;
        }
        if (any_kept) st = QN_SUPPRESSED;
        else if (all_suppressed) st = QN_KEPT;
        if (st != QN_UNDECIDED) s_any = 1;
      }
      next[i] = st;
    }
    __syncthreads();
    const int any = s_any;
    __syncthreads();
    if (!any) break;  // next equals prev
    cur ^= 1;
    ++done;
  }
  const unsigned char* fin = s_state[cur];
  int kept = 0;
  for (int i = t; i < K; i += QM_BLOCK) {
    const unsigned char st = fin[i];
    // an undecided quad can be left only by tables that are not this call's own: it is reported as kept
    const int k = i < n && st != QN_SUPPRESSED ? 1 : 0;
    int sup = -1;
    if (st == QN_SUPPRESSED) {
      const int lo = max(off[i], 0), hi = min(off[i + 1], max_pairs);
      float best = 0.f;
      for (int e = lo; e < hi; ++e) {  // ascending j: among equal probs the first one stays
        const int j = cp[e];
        if ((unsigned)j >= (unsigned)K || fin[j] != QN_KEPT) continue;
        const float pj = pr[j];
        if (sup < 0 || pj > best) {
          best = pj;
          sup = j;
        }
      }
    }
    keep[(long)b * K + i] = (unsigned char)k;
    suppressor[(long)b * K + i] = sup;
    kept += k;
  }
  kept = qm_wave_sum_i(kept);
  if ((t & 63) == 0) atomicAdd(&s_kept, kept);
  __syncthreads();
  if (t == 0) {
    stats[(long)b * QM_STATS + 0] = s_kept;
    if (rounds) rounds[b] = done;
  }
}

// inferencing.match_rows on the device: one thread per quad, four 16-byte stores.  Integer arithmetic is exact; the only
// rounding is rint (half to even) of the exact product c * 16.
__global__ __launch_bounds__(256) void qm_rows_kernel(const double* __restrict__ quads, const unsigned char* __restrict__ valid,
                                                       long total, int* __restrict__ rows) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  bool ok = valid ? valid[i] != 0 : true;
  double c16[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c16[k] = __builtin_rint(quads[i * 8 + k] * 16.0);
    ok = ok && __builtin_fabs(c16[k]) <= 524288.0;  // NaN and inf compare false
  }
  long cy[4], cx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cy[k] = ok ? (long)c16[2 * k] : 0;
    cx[k] = ok ? (long)c16[2 * k + 1] : 0;
  }
  long area2 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int k1 = (k + 1) & 3, k2 = (k + 2) & 3;
    const long ey = cy[k1] - cy[k], ex = cx[k1] - cx[k], ny = cy[k2] - cy[k1], nx = cx[k2] - cx[k1];
    ok = ok && ex * ny - ey * nx > 0;
    area2 += cx[k] * cy[k1] - cx[k1] * cy[k];
  }
  int4 r0 = make_int4(0, 0, 0, 0), r1 = r0, r2 = r0, r3 = r0;
  if (ok) {
    r0 = make_int4((int)cy[0], (int)cx[0], (int)cy[1], (int)cx[1]);
    r1 = make_int4((int)cy[2], (int)cx[2], (int)cy[3], (int)cx[3]);
    r2 = make_int4((int)min(min(cy[0], cy[1]), min(cy[2], cy[3])), (int)min(min(cx[0], cx[1]), min(cx[2], cx[3])),
                   (int)max(max(cy[0], cy[1]), max(cy[2], cy[3])), (int)max(max(cx[0], cx[1]), max(cx[2], cx[3])));
    r3 = make_int4((int)(unsigned)((unsigned long long)area2 & 0xffffffffull), (int)(unsigned)((unsigned long long)area2 >> 32),
                   1, 0);
  }
  int4* out = reinterpret_cast<int4*>(rows) + i * 4;
  out[0] = r0;
  out[1] = r1;
  out[2] = r2;
  out[3] = r3;
}


// workspace: QpLayout's, then cand_iou (B, max_pairs) u64 (not for the self matching) and cand_pred (B, max_pairs) int
struct QmLayout : QpLayout {
  size_t cand_iou, cand_pred;
};

QmLayout qm_layout(int B, int M, int N, int max_pairs, bool with_iou = true) {
  QmLayout l{qp_layout(B, M, N)};
  l.cand_iou = l.bytes;
  l.cand_pred = qm_align(l.cand_iou + (with_iou ? (size_t)B * max_pairs * sizeof(unsigned long long) : 0));
  l.bytes = qm_align(l.cand_pred + (size_t)B * max_pairs * sizeof(int));
  return l;
}

}  // namespace

extern "C" long long vkas_quad_match_workspace_bytes(int B, int M, int N, int max_pairs) {
  if (qp_check_dims("vkas_quad_match_workspace_bytes", B, M, N, max_pairs) != VKAS_OK) return -1;
  return (long long)qm_layout(B, M, N, max_pairs).bytes;
}

extern "C" int vkas_quad_match(const int* gt_rows, const int* gt_count, const int* pred_rows, const int* pred_count, int B,
                               int M, int N, double iou_thr, int max_pairs, void* workspace, size_t workspace_bytes,
                               int* gt_match, int* pred_match, double* gt_iou, long long* stats, int* rounds,
                               void* stream) {
  const int rc = qp_check_dims("vkas_quad_match", B, M, N, max_pairs);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(iou_thr > 0.0 && iou_thr <= 1.0, "vkas_quad_match: iou_thr = %g must lie in (0, 1]", iou_thr);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(gt_rows && gt_count && pred_rows && pred_count && workspace && gt_match && pred_match && gt_iou && stats,
             "vkas_quad_match: null pointer");
  VKAS_CHECK(vkas_aligned16(gt_rows) && vkas_aligned16(pred_rows) && vkas_aligned16(workspace),
             "vkas_quad_match: the row tables and the workspace must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)gt_iou) & 7u) == 0 && (((uintptr_t)stats) & 7u) == 0,
             "vkas_quad_match: gt_iou and stats must be 8-byte aligned");
  const QmLayout l = qm_layout(B, M, N, max_pairs);
  VKAS_CHECK(workspace_bytes >= l.bytes, "vkas_quad_match: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  // the matching pass keeps 12 bytes per pred in LDS
  constexpr size_t per_pred = sizeof(unsigned long long) + sizeof(int);
  const size_t lds = (size_t)N * per_pred;
  if (const int e = qp_allow_lds<qm_match_kernel>("vkas_quad_match", lds, QM_MAX * per_pred)) return e;
  const QpTables t = qp_tables(gt_rows, gt_count, pred_rows, pred_count, M, N, max_pairs, workspace, l);
  const QmMatchRule r{{}, iou_thr, stats, qp_at<int>(workspace, l.cand_pred), qp_at<unsigned long long>(workspace, l.cand_iou)};
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  qm_pair_kernel<false><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_match pairs");
  qm_scan_kernel<<<B, QM_BLOCK, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_match scan");
  qm_pair_kernel<true><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_match fill");
  qm_match_kernel<<<B, QM_BLOCK, lds, s>>>(gt_count, pred_count, M, N, l.Mp, t.rowoff, r.cand_pred, r.cand_iou, max_pairs,
                                           gt_match, pred_match, gt_iou, stats, rounds);
  VKAS_LAUNCH_CHECK("quad_match rounds");
  return VKAS_OK;
}

extern "C" int vkas_quad_rows(const double* quads, const unsigned char* valid, int B, int K, int* rows, void* stream) {
  VKAS_CHECK(B >= 0 && K >= 0 && (long)B * K < (1L << 27), "vkas_quad_rows: bad B=%d, K=%d (B*K below 2^27)", B, K);
  if ((long)B * K == 0) return VKAS_OK;
  VKAS_CHECK(quads && rows, "vkas_quad_rows: null pointer");
  VKAS_CHECK((((uintptr_t)quads) & 7u) == 0 && vkas_aligned16(rows),
             "vkas_quad_rows: quads must be 8-byte aligned and rows 16-byte aligned");
  const long total = (long)B * K;
  qm_rows_kernel<<<(unsigned)vkas_cdiv(total, 256), 256, 0, vkas_stream(stream)>>>(quads, valid, total, rows);
  VKAS_LAUNCH_CHECK("quad_rows");
  return VKAS_OK;
}

extern "C" long long vkas_quad_nms_workspace_bytes(int B, int K, int max_pairs) {
  if (qp_check_dims("vkas_quad_nms_workspace_bytes", B, K, K, max_pairs) != VKAS_OK) return -1;
  return (long long)qm_layout(B, K, K, max_pairs, false).bytes;
}

extern "C" int vkas_quad_nms(const int* rows, const int* count, const float* probs, int B, int K, double iou_thr,
                             int max_pairs, void* workspace, size_t workspace_bytes, unsigned char* keep, int* suppressor,
                             long long* stats, int* rounds, void* stream) {
  const int rc = qp_check_dims("vkas_quad_nms", B, K, K, max_pairs);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(iou_thr > 0.0 && iou_thr <= 1.0, "vkas_quad_nms: iou_thr = %g must lie in (0, 1]", iou_thr);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(rows && count && probs && workspace && keep && suppressor && stats, "vkas_quad_nms: null pointer");
  VKAS_CHECK(vkas_aligned16(rows) && vkas_aligned16(workspace),
             "vkas_quad_nms: the row table and the workspace must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)probs) & 3u) == 0 && (((uintptr_t)suppressor) & 3u) == 0 && (((uintptr_t)stats) & 7u) == 0,
             "vkas_quad_nms: probs and suppressor must be 4-byte aligned, stats 8-byte aligned");
  const QmLayout l = qm_layout(B, K, K, max_pairs, false);
  VKAS_CHECK(workspace_bytes >= l.bytes, "vkas_quad_nms: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  const QpTables t = qp_tables(rows, count, rows, count, K, K, max_pairs, workspace, l);
  const QmSelfRule r{{}, iou_thr, stats, probs, qp_at<int>(workspace, l.cand_pred)};
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  qm_pair_kernel<false><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_nms pairs");
  qm_scan_kernel<<<B, QM_BLOCK, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_nms scan");
  qm_pair_kernel<true><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_nms fill");
  qn_rounds_kernel<<<B, QM_BLOCK, 0, s>>>(rows, count, probs, K, l.Mp, t.rowoff, r.cand, max_pairs, keep, suppressor, stats,
                                          rounds);
  VKAS_LAUNCH_CHECK("quad_nms rounds");
  return VKAS_OK;
}

namespace {

// ---- ranked matching: the launcher ---------------------------------------------------------------------------------
// workspace: QmLayout's, then cover (B, MT * NT) u64 and tile_info (B, MT * NT, 1 + T) int
struct QrLayout : QmLayout {
  size_t cover, tile_info;
};

QrLayout qr_layout(int B, int M, int N, int T, int max_pairs) {
  QrLayout l{qm_layout(B, M, N, max_pairs)};
  l.cover = l.bytes;
  l.tile_info = qm_align(l.cover + l.tiles * sizeof(unsigned long long));
  l.bytes = qm_align(l.tile_info + l.tiles * (1 + (size_t)T) * sizeof(int));
  return l;
}

int qr_check_dims(const char* what, int B, int M, int N, int T, int max_pairs) {
  const int rc = qp_check_dims(what, B, M, N, max_pairs);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(T >= 1 && T <= QR_TMAX, "%s: T=%d thresholds must lie in 1..%d", what, T, QR_TMAX);
  VKAS_CHECK((long)B * T <= 65535, "%s: B*T = %ld above 65535", what, (long)B * T);
  return VKAS_OK;
}

}  // namespace

extern "C" long long vkas_quad_match_ranked_workspace_bytes(int B, int M, int N, int T, int max_pairs) {
  if (qr_check_dims("vkas_quad_match_ranked_workspace_bytes", B, M, N, T, max_pairs) != VKAS_OK) return -1;
  return (long long)qr_layout(B, M, N, T, max_pairs).bytes;
}

extern "C" int vkas_quad_match_ranked(const int* gt_rows, const int* gt_count, const unsigned char* gt_care,
                                      const int* pred_rows, const int* pred_count, const float* probs, int B, int M, int N,
                                      const double* iou_thrs, int T, double cover_thr, int max_pairs, void* workspace,
                                      size_t workspace_bytes, int* pred_match, unsigned char* pred_state, int* gt_match,
                                      double* pred_iou, unsigned char* covered, long long* stats, long long* dc_stats,
                                      int* rounds, void* stream) {
  const int rc = qr_check_dims("vkas_quad_match_ranked", B, M, N, T, max_pairs);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(iou_thrs, "vkas_quad_match_ranked: null iou_thrs");
  QrArgs x{};
  for (int t = 0; t < T; ++t) {  // on the host: iou_thrs is host memory
    const double v = iou_thrs[t];
    VKAS_CHECK(v > 0.0 && v <= 1.0, "vkas_quad_match_ranked: iou_thrs[%d] = %g must lie in (0, 1]", t, v);
    VKAS_CHECK(t == 0 || v > iou_thrs[t - 1], "vkas_quad_match_ranked: iou_thrs must ascend strictly, [%d] = %g after %g", t, v,
               iou_thrs[t - 1]);
    x.thr[t] = v;
  }
  VKAS_CHECK(cover_thr > 0.0 && cover_thr <= 1.0, "vkas_quad_match_ranked: cover_thr = %g must lie in (0, 1]", cover_thr);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(gt_rows && gt_count && pred_rows && pred_count && probs && workspace && pred_match && pred_state && gt_match &&
                 pred_iou && covered && stats && dc_stats,
             "vkas_quad_match_ranked: null pointer");
  VKAS_CHECK(vkas_aligned16(gt_rows) && vkas_aligned16(pred_rows) && vkas_aligned16(workspace),
             "vkas_quad_match_ranked: the row tables and the workspace must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)pred_iou) & 7u) == 0 && (((uintptr_t)stats) & 7u) == 0 && (((uintptr_t)dc_stats) & 7u) == 0 &&
                 (((uintptr_t)probs) & 3u) == 0,
             "vkas_quad_match_ranked: pred_iou, stats and dc_stats must be 8-byte aligned, probs 4-byte aligned");
  const QrLayout l = qr_layout(B, M, N, T, max_pairs);
  VKAS_CHECK(workspace_bytes >= l.bytes, "vkas_quad_match_ranked: workspace of %zu bytes, %zu needed", workspace_bytes,
             l.bytes);
  // the rounds keep 14 bytes per pred and 3 per gt in LDS
  const size_t lds = qr_lds_bytes(M, N);
  if (const int e = qp_allow_lds<qr_rounds_kernel>("vkas_quad_match_ranked", lds, qr_lds_bytes(QM_MAX, QM_MAX))) return e;
  x.gt_care = gt_care;
  x.cover = qp_at<unsigned long long>(workspace, l.cover);
  x.tile_info = qp_at<int>(workspace, l.tile_info);
  x.cover_thr = cover_thr;
  x.T = T;
  const QpTables t = qp_tables(gt_rows, gt_count, pred_rows, pred_count, M, N, max_pairs, workspace, l);
  const QrRule r{{}, x, probs, stats, qp_at<int>(workspace, l.cand_pred), qp_at<unsigned long long>(workspace, l.cand_iou)};
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  qm_pair_kernel<false><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_match_ranked pairs");
  qm_scan_kernel<<<B, QM_BLOCK, 0, s>>>(t, r, covered, dc_stats);
  VKAS_LAUNCH_CHECK("quad_match_ranked scan");
  qm_pair_kernel<true><<<grid, QM_THREADS, 0, s>>>(t, r);
  VKAS_LAUNCH_CHECK("quad_match_ranked fill");
  qr_rounds_kernel<<<(unsigned)(B * T), QM_BLOCK, lds, s>>>(gt_count, pred_rows, pred_count, probs, covered, M, N, l.Mp, x,
                                                            t.rowoff, r.cand_pred, r.cand_iou, max_pairs, pred_match,
                                                            pred_state, gt_match, pred_iou, stats, rounds);
  VKAS_LAUNCH_CHECK("quad_match_ranked rounds");
  return VKAS_OK;
}
