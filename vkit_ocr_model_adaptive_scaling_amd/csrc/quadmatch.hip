// Matching predicted character quadrilaterals to annotated ones by IoU (inferencing/evaluation.py holds the rule and the host
// oracles quad_iou_host / match_quads_host; the rule is this project's own).  rows (B, K, 16) int32: Q4 corners (8), the
// inclusive Q4 box (4), twice the area as int64 (2), valid, zero.  Four launches on one stream:
//
//   qm_pair_kernel<false>  a 128-thread workgroup owns a 64 gt x 64 pred tile of one image.  The boxes and valid words of its
//                          128 rows go to LDS; wave w box-tests gts [32w, 32w + 32) against pred = lane and appends the
//                          overlapping valid pairs to its LDS list at the ballot's prefix count (a list is bounded by the
//                          tile: no overflow path).  A tile without a pair - most tiles of a page - ends there.  Otherwise
//                          the corners follow and all threads take pairs from the two lists, so the clip is balanced
//                          whatever the tile holds.  A pair at or above iou_thr sets bit pj of the tile's 64-bit word of its
//                          gt (LDS atomic OR: integer, order-free).  Out: the tile's words and its pair count.
//   qm_scan_kernel         one workgroup per image: per gt the prefix of the words' popcounts over the pred tiles, then the
//                          exclusive scan over the gts = the CSR row offsets; n_gt, n_pred, pairs, candidates, status.
//   qm_pair_kernel<true>   the same tile body with the stored words in place of the box test: only candidates are clipped
//                          again (same code, same bits), each stored at  row offset + tile prefix + popcount of the lower
//                          bits: no slot atomics, pred ascending within a gt.  A tile whose words are all zero ends on
//                          them, and an image with status set is skipped.
//   qm_match_kernel        one workgroup per image, mutual-best rounds on integer atomicMax / atomicMin in LDS.
//
// The suppression of duplicate quads (vkas_quad_nms; inferencing/nms.py holds the rule and the oracle nms_quads_host) runs
// the same three passes on one table against itself - qm_pair_kernel<.., QM_SELF> and qm_scan_kernel<QM_SELF>: the row that is
// judged in the gt's place, the row that may suppress it in the pred's, pairs only where the pred outranks the gt - and
// then qn_rounds_kernel, one workgroup per image.  qm_rows_kernel (vkas_quad_rows) is inferencing.match_rows on the device.
//
// The ranked matching at T IoU thresholds with don't-care annotations (vkas_quad_match_ranked; inferencing/ranking.py holds
// the rule and the oracles) runs the three passes once more - qm_pair_kernel<.., QM_RANKED> and qm_scan_kernel<QM_RANKED>
// with thr = iou_thrs[0]: a pred without a finite prob loses its valid word as it is staged, the care flag rides in the
// gt row's zero word, a pair with a don't-care gt is clipped in the counting pass only and sets the pred's bit of the
// tile's cover word instead of a candidate bit, and the tile counts its candidates at every threshold - and then
// qr_rounds_kernel, one workgroup per (image, threshold), all of them walking the one candidate list.
//
// The clip is Sutherland-Hodgman in binary64, every operation rounded once (qm_* helpers under contract(off): see labels.hip
// for why __dmul_rn alone is not enough).  The two 8-vertex rings are indexed dynamically, so they live in per-thread LDS
// slots, [ring][vertex][coordinate][thread]: consecutive lanes hit consecutive 8-byte banks, and nothing goes to scratch.
// No float atomics, no allocation, no synchronisation: capture-safe and bit-identical from run to run.  Table reads are
// bounded by the tables' K rows (a row beyond the clamped count is dropped after its load), ring stores by RING_MAX, candidate stores by max_pairs, tile stores by the padded tile grid
// the workspace is sized for: no table content makes a kernel touch memory outside its buffers.
// The tile constants, the row staging and the clip live in quad_clip.h, which linematch.hip shares.
#include "quad_clip.h"

namespace {

constexpr int QM_STATS = 6;                // tp, n_gt, n_pred, pairs, candidates, status
constexpr int QR_STATS = 8;                // ranked: tp, fp, ignored, n_gt, n_pred, pairs, candidates, status
constexpr int QR_TMAX = 16;                // ranked: IoU thresholds per call
constexpr int QM_MATCH = 0, QM_SELF = 1, QM_RANKED = 2;  // what the three shared passes serve
constexpr unsigned long long QM_TAKEN = ~0ull;

__device__ __forceinline__ double qm_iou(const int4* g, const int4* p, double* ring) {
  double inter2;
  return qm_inter2_iou(g, p, ring, &inter2);
}

// What only the ranked matching passes to the shared passes and to its rounds.
struct QrArgs {
  const unsigned char* gt_care;  // (B, M), 0 = don't care; null = every gt is a care gt
  unsigned long long* cover;     // (B, MT * NT): per tile, bit j = pred j of the tile is covered by a don't-care gt of the tile
  int* tile_info;                // (B, MT * NT, 1 + T): the tile's don't-care pairs, its candidates at each threshold
  double cover_thr;
  int T;
  double thr[QR_TMAX];           // ascending; thr[0] is the threshold of the three passes
};

// workspace: words (B, NT, Mp) u64, cand_iou (B, max_pairs) u64, tpre (B, NT, Mp) int, rowoff (B, Mp + 1) int,
// tile_pairs (B, MT * NT) int, cand_pred (B, max_pairs) int
struct QmLayout {
  size_t words, cand_iou, tpre, rowoff, tile_pairs, cand_pred, bytes;
  int MT, NT, Mp;
};

// SELF: one table against itself for the suppression (gt = the row that is judged, pred = the row that may suppress it).  A
// row takes part iff it is valid and its prob is finite, and a pair only where the pred outranks the gt (the higher float32
// prob, then the lower index): the diagonal and one of (i, j), (j, i) drop out before the clip.  The prob bits travel in the
// row's zero word in LDS.
// RANKED: a pred takes part iff it is valid and its prob is finite; the zero word of a gt row carries its care flag.  In the
// counting pass a pair with a don't-care gt is clipped for the coverage test alone (inter2 >= cover_thr * area2_p, the
// product rounded once) and a care pair is counted at every threshold it reaches; the fill never meets a don't-care gt,
// whose words are zero.
template <bool FILL, int KIND>
__global__ __launch_bounds__(QM_THREADS) void qm_pair_kernel(const int* __restrict__ gt_rows, const int* __restrict__ gt_count,
                                                              const int* __restrict__ pred_rows,
                                                              const int* __restrict__ pred_count, int M, int N, int Mp,
                                                              int NT, double thr, unsigned long long* __restrict__ words,
                                                              int* __restrict__ tpre, int* __restrict__ tile_pairs,
                                                              const int* __restrict__ rowoff,
                                                              const long long* __restrict__ stats, int* __restrict__ cand_pred,
                                                              unsigned long long* __restrict__ cand_iou, int max_pairs,
                                                              const float* __restrict__ probs, const QrArgs x) {
  constexpr bool SELF = KIND == QM_SELF, RANKED = KIND == QM_RANKED;
  __shared__ int4 s_rows[2 * QM_TILE * 4];
  __shared__ unsigned long long s_word[QM_TILE];
  __shared__ unsigned short s_list[QM_WAVES * QM_LIST];
  __shared__ int s_cnt[QM_WAVES];
  __shared__ double s_ring[2 * QM_RING * 2 * QM_THREADS];
  __shared__ unsigned long long s_cover;  // RANKED counting pass only, as the next two
  __shared__ int s_dc[QM_WAVES];
  __shared__ int s_ct[QR_TMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tn = blockIdx.x, tm = blockIdx.y, b = blockIdx.z;
  const int g0 = tm * QM_TILE, p0 = tn * QM_TILE;
  const long word_at = ((long)b * NT + tn) * Mp + g0;
  // Most tiles of a page end early: the status, the counts, the words and (below) the rows are read at addresses that depend
  // on no other load, so such a workgroup lives one load's latency.  Every early return is taken by the whole workgroup.
  const long long status = FILL ? stats[RANKED ? (long)b * x.T * QR_STATS + 7 : (long)b * QM_STATS + 5] : 0;
  const int ng = qm_clamp(gt_count[b], M), np = qm_clamp(pred_count[b], N);
  if (FILL && status != 0) return;  // nothing of this image is stored
  unsigned long long word = 0ull;
  if (FILL && tid < QM_TILE) word = words[word_at + tid];
  // a part of the 128 rows of the tile: 0, 1 = the corners, 2 = the box, 3 = area and valid (qm_stage_half); what rides in
  // the zero word of part 3 is put there as the row is staged
  const auto fix = [&](int4& v, bool is_gt, int at, int part) {
    if (SELF && part == 3) {  // M == N: one table
      const unsigned pb = __float_as_uint(probs[(long)b * M + at]);
      v.z = (v.z != 0 && qm_finite_bits(pb)) ? 1 : 0;
      v.w = (int)pb;
    }
    if (RANKED && part == 3) {
      if (is_gt) {
        v.w = x.gt_care ? (x.gt_care[(long)b * M + at] != 0 ? 1 : 0) : 1;
      } else {
        const unsigned pb = __float_as_uint(probs[(long)b * N + at]);
        v.z = (v.z != 0 && qm_finite_bits(pb)) ? 1 : 0;
        v.w = (int)pb;
      }
    }
  };
  const auto stage = [&](int half) { qm_stage_half(s_rows, gt_rows, pred_rows, b, M, N, g0, p0, ng, np, half, tid, fix); };
  if (tid < QM_TILE) s_word[tid] = word;
  if (RANKED && !FILL) {
    if (tid == 0) s_cover = 0ull;
    if (tid < QR_TMAX) s_ct[tid] = 0;
  }
  if (FILL) {  // most tiles of a page hold no candidate: they end here, on 512 bytes
    __syncthreads();
    if (__ballot(s_word[lane] != 0ull) == 0ull) return;
  }
  stage(1);  // the box test needs boxes and valid only; a tile without a pair ends on them
  __syncthreads();

  const int4 pbox = s_rows[(QM_TILE + lane) * 4 + 2];
  const bool pvalid = s_rows[(QM_TILE + lane) * 4 + 3].z != 0;
  const float pprob = __int_as_float(s_rows[(QM_TILE + lane) * 4 + 3].w);  // SELF only
  int cnt = 0, dcnt = 0;
  for (int s = 0; s < QM_TILE / QM_WAVES; ++s) {
    const int gi = wave * (QM_TILE / QM_WAVES) + s;
    bool hit;
    if (FILL) {
      hit = (s_word[gi] >> lane) & 1ull;
    } else {
      const int4 gbox = s_rows[gi * 4 + 2];
      hit = pvalid && s_rows[gi * 4 + 3].z != 0 && gbox.x <= pbox.z && pbox.x <= gbox.z && gbox.y <= pbox.w &&
            pbox.y <= gbox.w;
      if (SELF) {
        const float gprob = __int_as_float(s_rows[gi * 4 + 3].w);
        hit = hit && (pprob > gprob || (pprob == gprob && p0 + lane < g0 + gi));
      }
    }
    const unsigned long long bits = __ballot(hit);
    if (hit) s_list[wave * QM_LIST + cnt + __popcll(bits & ((1ull << lane) - 1ull))] = (unsigned short)(gi * QM_TILE + lane);
    cnt += __popcll(bits);  // <= 32 * 64 = QM_LIST
    if (RANKED && !FILL && s_rows[gi * 4 + 3].w == 0) dcnt += __popcll(bits);  // gi is the wave's: uniform
  }
  if (lane == 0) s_cnt[wave] = cnt;
  if (RANKED && !FILL && lane == 0) s_dc[wave] = dcnt;
  __syncthreads();
  const int c0 = s_cnt[0], total = c0 + s_cnt[1];
  static_assert(QM_WAVES == 2, "the two lists are read as one");
  if (total == 0) {  // the whole workgroup
    if (!FILL) {
      if (tid < QM_TILE) words[word_at + tid] = 0ull;
      if (tid == 0) tile_pairs[((long)b * gridDim.y + tm) * NT + tn] = 0;
      if (RANKED) {
        const long tile = ((long)b * gridDim.y + tm) * NT + tn;
        if (tid == 0) x.cover[tile] = 0ull;
        if (tid < 1 + x.T) x.tile_info[tile * (1 + x.T) + tid] = 0;
      }
    }
    return;
  }
  stage(0);
  __syncthreads();
  for (int e = tid; e < total; e += QM_THREADS) {
    const int q = e < c0 ? s_list[e] : s_list[QM_LIST + e - c0];
    const int gi = q >> 6, pj = q & 63;
    double inter2;
    const double iou = qm_inter2_iou(s_rows + gi * 4, s_rows + (QM_TILE + pj) * 4, s_ring + tid, &inter2);
    if (RANKED && !FILL) {
      if (s_rows[gi * 4 + 3].w == 0) {  // a don't-care gt: the coverage test, never a candidate
        const int4 pa = s_rows[(QM_TILE + pj) * 4 + 3];
        const double ap = (double)(long)(((unsigned long long)(unsigned)pa.y << 32) | (unsigned)pa.x);
        if (inter2 >= qm_mul(x.cover_thr, ap)) atomicOr(&s_cover, 1ull << pj);
        continue;
      }
      for (int t = 0; t < x.T; ++t)
        if (iou >= x.thr[t]) atomicAdd(&s_ct[t], 1);
    }
    if (!(iou >= thr)) continue;
    if (FILL) {
      const int g = g0 + gi;
      const long slot = (long)rowoff[(long)b * (Mp + 1) + g] + tpre[word_at + gi] +
                        __popcll(s_word[gi] & ((1ull << pj) - 1ull));
      if (slot >= 0 && slot < max_pairs) {
        cand_pred[(long)b * max_pairs + slot] = p0 + pj;
        if (!SELF) cand_iou[(long)b * max_pairs + slot] = (unsigned long long)__double_as_longlong(iou);
      }
    } else {
      atomicOr(&s_word[gi], 1ull << pj);
    }
  }
  if (!FILL) {
    __syncthreads();
    if (tid < QM_TILE) words[word_at + tid] = s_word[tid];
    if (RANKED) {  // pairs counts the care pairs alone
      const long tile = ((long)b * gridDim.y + tm) * NT + tn;
      const int dc = s_dc[0] + s_dc[1];
      if (tid == 0) {
        tile_pairs[tile] = total - dc;
        x.cover[tile] = s_cover;
        x.tile_info[tile * (1 + x.T)] = dc;
      }
      if (tid < x.T) x.tile_info[tile * (1 + x.T) + 1 + tid] = s_ct[tid];
    } else if (tid == 0) {
      tile_pairs[((long)b * gridDim.y + tm) * NT + tn] = total;
    }
  }
}

// SELF (the suppression): stats = kept (written by the rounds), n = the clamped count, n_valid = the rows that take part.
// RANKED: stats (B, T, 8) words 3..7 of every threshold = n_gt (care gts), n_pred, pairs (care), the candidates at that
// threshold, status; covered (B, N) = the OR of the tiles' cover words down the gt tiles; dc_stats (B, 3) = n_dc, dc_pairs,
// n_covered.  Words 0..2 are the rounds'.
template <int KIND>
__global__ __launch_bounds__(QM_BLOCK) void qm_scan_kernel(const int* __restrict__ gt_rows, const int* __restrict__ gt_count,
                                                            const int* __restrict__ pred_rows,
                                                            const int* __restrict__ pred_count, int M, int N, int Mp, int NT,
                                                            int MT, const unsigned long long* __restrict__ words,
                                                            int* __restrict__ tpre, const int* __restrict__ tile_pairs,
                                                            int* __restrict__ rowoff, long long* __restrict__ stats,
                                                            int max_pairs, const float* __restrict__ probs, const QrArgs x,
                                                            unsigned char* __restrict__ covered,
                                                            long long* __restrict__ dc_stats) {
  constexpr bool SELF = KIND == QM_SELF, RANKED = KIND == QM_RANKED;
  __shared__ int s_cnt[QM_MAX];
  __shared__ int s_wave[QM_BLOCK / 64];
  __shared__ int s_sum[3];
  __shared__ int s_more[3 + QR_TMAX];                  // RANKED only, as the next: n_dc, dc_pairs, n_covered, candidates at t
  __shared__ unsigned long long s_cov[QM_MAX / QM_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const int ng = qm_clamp(gt_count[b], M), np = qm_clamp(pred_count[b], N);
  if (t < 3) s_sum[t] = 0;
  if (RANKED) {
    if (t < 3 + QR_TMAX) s_more[t] = 0;
    if (t < NT) {  // NT <= QM_MAX / QM_TILE
      unsigned long long w = 0ull;
      for (int tm = 0; tm < MT; ++tm) w |= x.cover[((long)b * MT + tm) * NT + t];
      s_cov[t] = w;
    }
    __syncthreads();
    int n_dc = 0, n_cov = 0;
    for (int g = t; g < ng; g += QM_BLOCK)
      n_dc += gt_rows[((long)b * M + g) * 16 + 14] != 0 && x.gt_care && x.gt_care[(long)b * M + g] == 0;
    for (int p = t; p < N; p += QM_BLOCK) {
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
      for (int i = t; i < MT * NT; i += QM_BLOCK) v += x.tile_info[((long)b * MT * NT + i) * (1 + x.T) + k];
      v = qm_wave_sum_i(v);
      if (lane == 0) atomicAdd(&s_more[k == 0 ? 1 : 2 + k], v);
    }
  }
  for (int g = t; g < Mp; g += QM_BLOCK) {  // Mp <= QM_MAX
    int run = 0;
#pragma unroll 8
    for (int tn = 0; tn < NT; ++tn) {
      const long at = ((long)b * NT + tn) * Mp + g;
      tpre[at] = run;
      run += __popcll(words[at]);
    }
    s_cnt[g] = run;
  }
  int n_gt = 0, n_pred = 0, pairs = 0;
  if (SELF) {
    n_gt = t == 0 ? ng : 0;
    for (int g = t; g < ng; g += QM_BLOCK)
      n_pred += gt_rows[((long)b * M + g) * 16 + 14] != 0 && qm_finite_bits(__float_as_uint(probs[(long)b * M + g]));
  } else if (RANKED) {
    for (int g = t; g < ng; g += QM_BLOCK)
      n_gt += gt_rows[((long)b * M + g) * 16 + 14] != 0 && (!x.gt_care || x.gt_care[(long)b * M + g] != 0);
    for (int p = t; p < np; p += QM_BLOCK)
      n_pred += pred_rows[((long)b * N + p) * 16 + 14] != 0 && qm_finite_bits(__float_as_uint(probs[(long)b * N + p]));
  } else {
    for (int g = t; g < ng; g += QM_BLOCK) n_gt += gt_rows[((long)b * M + g) * 16 + 14] != 0;
    for (int p = t; p < np; p += QM_BLOCK) n_pred += pred_rows[((long)b * N + p) * 16 + 14] != 0;
  }
  for (int i = t; i < MT * NT; i += QM_BLOCK) pairs += tile_pairs[(long)b * MT * NT + i];  // <= M * N <= 2^26
  __syncthreads();
  n_gt = qm_wave_sum_i(n_gt);
  n_pred = qm_wave_sum_i(n_pred);
  pairs = qm_wave_sum_i(pairs);
  if (lane == 0) {
    atomicAdd(&s_sum[0], n_gt);
    atomicAdd(&s_sum[1], n_pred);
    atomicAdd(&s_sum[2], pairs);
  }
  // exclusive scan of s_cnt: each thread owns a contiguous run of gts
  const int seg = (Mp + QM_BLOCK - 1) / QM_BLOCK;
  const int lo = min(Mp, t * seg), hi = min(Mp, lo + seg);
  int own = 0;
  for (int g = lo; g < hi; ++g) own += s_cnt[g];
  int v = own;
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int run = v - own, all = 0;
  for (int w = 0; w < QM_BLOCK / 64; ++w) {
    if (w < wave) run += s_wave[w];
    all += s_wave[w];
  }
  for (int g = lo; g < hi; ++g) {
    rowoff[(long)b * (Mp + 1) + g] = run;
    run += s_cnt[g];
  }
  if (RANKED) {
    if (t == 0) {
      rowoff[(long)b * (Mp + 1) + Mp] = all;
      for (int k = 0; k < 3; ++k) dc_stats[(long)b * 3 + k] = s_more[k];
    }
    if (t < x.T) {
      long long* st = stats + ((long)b * x.T + t) * QR_STATS;
      st[3] = s_sum[0];
      st[4] = s_sum[1];
      st[5] = s_sum[2];
      st[6] = s_more[3 + t];
      st[7] = all > max_pairs ? 1 : 0;
    }
    return;
  }
  if (t == 0) {
    rowoff[(long)b * (Mp + 1) + Mp] = all;
    long long* st = stats + (long)b * QM_STATS;
    st[0] = 0;
    st[1] = s_sum[0];
    st[2] = s_sum[1];
    st[3] = s_sum[2];
    st[4] = all;
    st[5] = all > max_pairs ? 1 : 0;
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


QmLayout qm_layout(int B, int M, int N, int max_pairs, bool with_iou = true) {
  QmLayout l;
  l.MT = (int)vkas_cdiv(M, QM_TILE);
  l.NT = (int)vkas_cdiv(N, QM_TILE);
  l.Mp = l.MT * QM_TILE;
  const size_t tiles = (size_t)B * l.NT * l.Mp;
  l.words = 0;
  l.cand_iou = qm_align(l.words + tiles * sizeof(unsigned long long));
  l.tpre = qm_align(l.cand_iou + (with_iou ? (size_t)B * max_pairs * sizeof(unsigned long long) : 0));
  l.rowoff = qm_align(l.tpre + tiles * sizeof(int));
  l.tile_pairs = qm_align(l.rowoff + (size_t)B * (l.Mp + 1) * sizeof(int));
  l.cand_pred = qm_align(l.tile_pairs + (size_t)B * l.MT * l.NT * sizeof(int));
  l.bytes = qm_align(l.cand_pred + (size_t)B * max_pairs * sizeof(int));
  return l;
}

int qm_check_dims(const char* what, int B, int M, int N, int max_pairs) {
  VKAS_CHECK(B >= 0 && B <= 65535, "%s: bad B=%d (0..65535)", what, B);
  VKAS_CHECK(M >= 1 && M <= QM_MAX && N >= 1 && N <= QM_MAX, "%s: M=%d and N=%d must lie in 1..%d", what, M, N, QM_MAX);
  VKAS_CHECK(max_pairs >= 0, "%s: max_pairs=%d must be >= 0", what, max_pairs);
  VKAS_CHECK((long)B * max_pairs < (1L << 31), "%s: B*max_pairs = %ld must stay below 2^31", what, (long)B * max_pairs);
  return VKAS_OK;
}

}  // namespace

extern "C" long long vkas_quad_match_workspace_bytes(int B, int M, int N, int max_pairs) {
  if (qm_check_dims("vkas_quad_match_workspace_bytes", B, M, N, max_pairs) != VKAS_OK) return -1;
  return (long long)qm_layout(B, M, N, max_pairs).bytes;
}

extern "C" int vkas_quad_match(const int* gt_rows, const int* gt_count, const int* pred_rows, const int* pred_count, int B,
                               int M, int N, double iou_thr, int max_pairs, void* workspace, size_t workspace_bytes,
                               int* gt_match, int* pred_match, double* gt_iou, long long* stats, int* rounds,
                               void* stream) {
  const int rc = qm_check_dims("vkas_quad_match", B, M, N, max_pairs);
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
  // the matching pass keeps 12 bytes per pred in LDS: above the default 64 KB the kernel is opted in, once
  const size_t lds = (size_t)N * (sizeof(unsigned long long) + sizeof(int));
  static size_t lds_allowed = 48 * 1024;
  if (lds > lds_allowed) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(qm_match_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)((size_t)QM_MAX * (sizeof(unsigned long long) + sizeof(int))));
    if (e != hipSuccess) {
      vkas_set_error("vkas_quad_match: %zu bytes of LDS for N = %d refused: %s", lds, N, hipGetErrorString(e));
      return VKAS_E_LAUNCH;
    }
    lds_allowed = (size_t)QM_MAX * (sizeof(unsigned long long) + sizeof(int));
  }
  char* ws = static_cast<char*>(workspace);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + l.words);
  unsigned long long* cand_iou = reinterpret_cast<unsigned long long*>(ws + l.cand_iou);
  int* tpre = reinterpret_cast<int*>(ws + l.tpre);
  int* rowoff = reinterpret_cast<int*>(ws + l.rowoff);
  int* tile_pairs = reinterpret_cast<int*>(ws + l.tile_pairs);
  int* cand_pred = reinterpret_cast<int*>(ws + l.cand_pred);
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  qm_pair_kernel<false, QM_MATCH><<<grid, QM_THREADS, 0, s>>>(gt_rows, gt_count, pred_rows, pred_count, M, N, l.Mp, l.NT,
                                                            iou_thr, words, tpre, tile_pairs, rowoff, stats, cand_pred,
                                                            cand_iou, max_pairs, nullptr, QrArgs{});
  VKAS_LAUNCH_CHECK("quad_match pairs");
  qm_scan_kernel<QM_MATCH><<<B, QM_BLOCK, 0, s>>>(gt_rows, gt_count, pred_rows, pred_count, M, N, l.Mp, l.NT, l.MT, words, tpre,
                                               tile_pairs, rowoff, stats, max_pairs, nullptr, QrArgs{}, nullptr, nullptr);
  VKAS_LAUNCH_CHECK("quad_match scan");
  qm_pair_kernel<true, QM_MATCH><<<grid, QM_THREADS, 0, s>>>(gt_rows, gt_count, pred_rows, pred_count, M, N, l.Mp, l.NT,
                                                           iou_thr, words, tpre, tile_pairs, rowoff, stats, cand_pred,
                                                           cand_iou, max_pairs, nullptr, QrArgs{});
  VKAS_LAUNCH_CHECK("quad_match fill");
  qm_match_kernel<<<B, QM_BLOCK, lds, s>>>(gt_count, pred_count, M, N, l.Mp, rowoff, cand_pred, cand_iou, max_pairs, gt_match,
                                           pred_match, gt_iou, stats, rounds);
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
  if (qm_check_dims("vkas_quad_nms_workspace_bytes", B, K, K, max_pairs) != VKAS_OK) return -1;
  return (long long)qm_layout(B, K, K, max_pairs, false).bytes;
}

extern "C" int vkas_quad_nms(const int* rows, const int* count, const float* probs, int B, int K, double iou_thr,
                             int max_pairs, void* workspace, size_t workspace_bytes, unsigned char* keep, int* suppressor,
                             long long* stats, int* rounds, void* stream) {
  const int rc = qm_check_dims("vkas_quad_nms", B, K, K, max_pairs);
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
  char* ws = static_cast<char*>(workspace);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + l.words);
  int* tpre = reinterpret_cast<int*>(ws + l.tpre);
  int* rowoff = reinterpret_cast<int*>(ws + l.rowoff);
  int* tile_pairs = reinterpret_cast<int*>(ws + l.tile_pairs);
  int* cand = reinterpret_cast<int*>(ws + l.cand_pred);
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  qm_pair_kernel<false, QM_SELF><<<grid, QM_THREADS, 0, s>>>(rows, count, rows, count, K, K, l.Mp, l.NT, iou_thr, words, tpre,
                                                           tile_pairs, rowoff, stats, cand, nullptr, max_pairs, probs, QrArgs{});
  VKAS_LAUNCH_CHECK("quad_nms pairs");
  qm_scan_kernel<QM_SELF><<<B, QM_BLOCK, 0, s>>>(rows, count, rows, count, K, K, l.Mp, l.NT, l.MT, words, tpre, tile_pairs,
                                              rowoff, stats, max_pairs, probs, QrArgs{}, nullptr, nullptr);
  VKAS_LAUNCH_CHECK("quad_nms scan");
  qm_pair_kernel<true, QM_SELF><<<grid, QM_THREADS, 0, s>>>(rows, count, rows, count, K, K, l.Mp, l.NT, iou_thr, words, tpre,
                                                          tile_pairs, rowoff, stats, cand, nullptr, max_pairs, probs, QrArgs{});
  VKAS_LAUNCH_CHECK("quad_nms fill");
  qn_rounds_kernel<<<B, QM_BLOCK, 0, s>>>(rows, count, probs, K, l.Mp, rowoff, cand, max_pairs, keep, suppressor, stats,
                                          rounds);
  VKAS_LAUNCH_CHECK("quad_nms rounds");
  return VKAS_OK;
}

namespace {

// ---- ranked matching: the launcher ---------------------------------------------------------------------------------
// workspace: QmLayout's, then cover (B, MT * NT) u64 and tile_info (B, MT * NT, 1 + T) int
struct QrLayout {
  QmLayout q;
  size_t cover, tile_info, bytes;
};

QrLayout qr_layout(int B, int M, int N, int T, int max_pairs) {
  QrLayout l;
  l.q = qm_layout(B, M, N, max_pairs);
  const size_t tiles = (size_t)B * l.q.MT * l.q.NT;
  l.cover = l.q.bytes;
  l.tile_info = qm_align(l.cover + tiles * sizeof(unsigned long long));
  l.bytes = qm_align(l.tile_info + tiles * (1 + (size_t)T) * sizeof(int));
  return l;
}

int qr_check_dims(const char* what, int B, int M, int N, int T, int max_pairs) {
  const int rc = qm_check_dims(what, B, M, N, max_pairs);
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
  // the rounds keep 14 bytes per pred and 3 per gt in LDS: above the default 64 KB the kernel is opted in, once
  const size_t lds = qr_lds_bytes(M, N);
  static size_t lds_allowed = 48 * 1024;
  if (lds > lds_allowed) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(qr_rounds_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)qr_lds_bytes(QM_MAX, QM_MAX));
    if (e != hipSuccess) {
      vkas_set_error("vkas_quad_match_ranked: %zu bytes of LDS for M = %d, N = %d refused: %s", lds, M, N,
                     hipGetErrorString(e));
      return VKAS_E_LAUNCH;
    }
    lds_allowed = qr_lds_bytes(QM_MAX, QM_MAX);
  }
  char* ws = static_cast<char*>(workspace);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + l.q.words);
  unsigned long long* cand_iou = reinterpret_cast<unsigned long long*>(ws + l.q.cand_iou);
  int* tpre = reinterpret_cast<int*>(ws + l.q.tpre);
  int* rowoff = reinterpret_cast<int*>(ws + l.q.rowoff);
  int* tile_pairs = reinterpret_cast<int*>(ws + l.q.tile_pairs);
  int* cand_pred = reinterpret_cast<int*>(ws + l.q.cand_pred);
  x.gt_care = gt_care;
  x.cover = reinterpret_cast<unsigned long long*>(ws + l.cover);
  x.tile_info = reinterpret_cast<int*>(ws + l.tile_info);
  x.cover_thr = cover_thr;
  x.T = T;
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.q.NT, (unsigned)l.q.MT, (unsigned)B);
  qm_pair_kernel<false, QM_RANKED><<<grid, QM_THREADS, 0, s>>>(gt_rows, gt_count, pred_rows, pred_count, M, N, l.q.Mp, l.q.NT,
                                                               x.thr[0], words, tpre, tile_pairs, rowoff, stats, cand_pred,
                                                               cand_iou, max_pairs, probs, x);
  VKAS_LAUNCH_CHECK("quad_match_ranked pairs");
  qm_scan_kernel<QM_RANKED><<<B, QM_BLOCK, 0, s>>>(gt_rows, gt_count, pred_rows, pred_count, M, N, l.q.Mp, l.q.NT, l.q.MT, words,
                                                   tpre, tile_pairs, rowoff, stats, max_pairs, probs, x, covered, dc_stats);
  VKAS_LAUNCH_CHECK("quad_match_ranked scan");
  qm_pair_kernel<true, QM_RANKED><<<grid, QM_THREADS, 0, s>>>(gt_rows, gt_count, pred_rows, pred_count, M, N, l.q.Mp, l.q.NT,
                                                              x.thr[0], words, tpre, tile_pairs, rowoff, stats, cand_pred,
                                                              cand_iou, max_pairs, probs, x);
  VKAS_LAUNCH_CHECK("quad_match_ranked fill");
  qr_rounds_kernel<<<(unsigned)(B * T), QM_BLOCK, lds, s>>>(gt_count, pred_rows, pred_count, probs, covered, M, N, l.q.Mp, x,
                                                            rowoff, cand_pred, cand_iou, max_pairs, pred_match, pred_state,
                                                            gt_match, pred_iou, stats, rounds);
  VKAS_LAUNCH_CHECK("quad_match_ranked rounds");
  return VKAS_OK;
}
