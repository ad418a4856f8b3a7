// Scoring detected text lines against annotated ones with one-to-one matches, splits and merges (inferencing/
// line_evaluation.py holds the rule and the host oracles match_lines_host / match_lines_rounds_host; the rule is this
// project's own).  rows (B, K, 16) int32 are the match rows of quadmatch.hip.  Four launches on one stream:
//
//   lm_pair_kernel<false>  the counting pass: a 128-thread workgroup owns a 64 gt x 64 pred tile of one image, box-tests it
//                          and clips the overlapping pairs exactly as qm_pair_kernel does (quad_clip.h: the same staging,
//                          the same clip).  A pair with a don't-care gt takes the coverage test of the ranked matching and
//                          sets the pred's bit of the tile's cover word; a care pair takes I = floor(min(inter2, 2^41)),
//                          the two integer tests rec_ok / prec_ok on the clamped areas, and sets bit pj of the gt's word
//                          when it is a candidate (LDS atomic OR: integer, order-free).
//   lm_scan_kernel         one workgroup per image: the cover words OR-ed down the gt tiles = the ignored preds (kept as
//                          B x NT words); every candidate word loses the ignored preds' bits and is written back; per gt the
//                          prefix of the popcounts over the pred tiles, then the exclusive scan over the gts = the CSR row
//                          offsets; n_gt, n_pred, n_dc, n_ignored, pairs, candidates, status.
//   lm_pair_kernel<true>   the filling pass: the same tile body with the stored words in place of the box test; a candidate
//                          is clipped again (same code, same bits) and stored as one 64-bit word  I << 15 | prec_ok << 14 |
//                          rec_ok << 13 | pred  at  row offset + tile prefix + popcount of the lower bits: no slot
//                          atomics, preds ascending within a gt.
//   lm_phase_kernel        one workgroup per image: phase A (row and column counts of Q, integer LDS atomics), the split
//                          rounds, the merge rounds, then one sweep that writes every output.
//
// Integer atomics only (add, min on 32 and 64-bit words in LDS): nothing depends on arrival order.  No allocation, no
// synchronisation: capture-safe and bit-identical from run to run.  Table reads are bounded by the tables' K rows, ring
// stores by the ring's 8 slots, candidate stores by max_pairs, tile stores by the padded tile grid the workspace is sized
// for, and a pred index read back from a candidate word is checked against N: no table content makes a kernel touch memory
// outside its buffers.  Every output word and every workspace word that is read is written earlier in the same call.
#include "quad_clip.h"

namespace {

constexpr int LM_STATS = 16;
constexpr long LM_AREA_MAX = 1L << 41;  // twice the area of a quad whose Q4 corners lie within +-2^19
constexpr unsigned char LM_ABSENT = 0, LM_FREE = 1, LM_ONE = 2, LM_SPLIT = 3, LM_MERGE = 4, LM_APART = 5;
constexpr unsigned short LM_NONE = 0xffff;
constexpr int LM_PRED_BITS = 13;  // a pred index below QM_MAX
static_assert(QM_MAX == 1 << LM_PRED_BITS, "the packing of a candidate word");

__host__ __device__ constexpr size_t lm_lds_bytes(int M, int N) {
  return (size_t)N * (sizeof(unsigned long long) + sizeof(int) + 2) + (size_t)M * (sizeof(unsigned short) + 1);
}

__device__ __forceinline__ long lm_area(long a) { return min(max(a, 0L), LM_AREA_MAX); }

// workspace: words (B, NT, Mp) u64, cand (B, max_pairs) u64, cover (B, MT * NT) u64, ignored (B, NT) u64,
// tpre (B, NT, Mp) int, rowoff (B, Mp + 1) int, tile_pairs (B, MT * NT) int
struct LmLayout {
  size_t words, cand, cover, ignored, tpre, rowoff, tile_pairs, bytes;
  int MT, NT, Mp;
};

template <bool FILL>
__global__ __launch_bounds__(QM_THREADS) void lm_pair_kernel(const int* __restrict__ gt_rows, const int* __restrict__ gt_count,
                                                              const unsigned char* __restrict__ gt_care,
                                                              const int* __restrict__ pred_rows,
                                                              const int* __restrict__ pred_count, int M, int N, int Mp,
                                                              int NT, int tr_q8, int tp_q8, double cover_thr,
                                                              unsigned long long* __restrict__ words,
                                                              unsigned long long* __restrict__ cover,
                                                              const int* __restrict__ tpre, int* __restrict__ tile_pairs,
                                                              const int* __restrict__ rowoff,
                                                              const long long* __restrict__ stats,
                                                              unsigned long long* __restrict__ cand, int max_pairs) {
  __shared__ int4 s_rows[2 * QM_TILE * 4];
  __shared__ unsigned long long s_word[QM_TILE];
  __shared__ unsigned short s_list[QM_WAVES * QM_LIST];
  __shared__ int s_cnt[QM_WAVES];
  __shared__ double s_ring[2 * QM_RING * 2 * QM_THREADS];
  __shared__ unsigned long long s_cover;  // the counting pass only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tn = blockIdx.x, tm = blockIdx.y, b = blockIdx.z;
  const int g0 = tm * QM_TILE, p0 = tn * QM_TILE;
  const long word_at = ((long)b * NT + tn) * Mp + g0;
  const long tile = ((long)b * gridDim.y + tm) * NT + tn;
  // every early return is taken by the whole workgroup
  const long long status = FILL ? stats[(long)b * LM_STATS + 11] : 0;
  const int ng = qm_clamp(gt_count[b], M), np = qm_clamp(pred_count[b], N);
  if (FILL && status != 0) return;  // nothing of this image is stored
  unsigned long long word = 0ull;
  if (FILL && tid < QM_TILE) word = words[word_at + tid];
  const auto fix = [&](int4& v, bool is_gt, int at, int part) {  // the care flag rides in the gt row's zero word
    if (part == 3 && is_gt) v.w = gt_care ? (gt_care[(long)b * M + at] != 0 ? 1 : 0) : 1;
  };
  const auto stage = [&](int half) { qm_stage_half(s_rows, gt_rows, pred_rows, b, M, N, g0, p0, ng, np, half, tid, fix); };
  if (tid < QM_TILE) s_word[tid] = word;
  if (!FILL && tid == 0) s_cover = 0ull;
  if (FILL) {  // most tiles of a page hold no candidate: they end here, on 512 bytes
    __syncthreads();
    if (__ballot(s_word[lane] != 0ull) == 0ull) return;
  }
  stage(1);  // the box test needs boxes and valid only; a tile without a pair ends on them
  __syncthreads();

  const int4 pbox = s_rows[(QM_TILE + lane) * 4 + 2];
  const bool pvalid = s_rows[(QM_TILE + lane) * 4 + 3].z != 0;
  int cnt = 0;
  for (int s = 0; s < QM_TILE / QM_WAVES; ++s) {
    const int gi = wave * (QM_TILE / QM_WAVES) + s;
    bool hit;
    if (FILL) {
      hit = (s_word[gi] >> lane) & 1ull;
    } else {
      const int4 gbox = s_rows[gi * 4 + 2];
      hit = pvalid && s_rows[gi * 4 + 3].z != 0 && gbox.x <= pbox.z && pbox.x <= gbox.z && gbox.y <= pbox.w &&
            pbox.y <= gbox.w;
    }
    const unsigned long long bits = __ballot(hit);
    if (hit) s_list[wave * QM_LIST + cnt + __popcll(bits & ((1ull << lane) - 1ull))] = (unsigned short)(gi * QM_TILE + lane);
    cnt += __popcll(bits);  // <= 32 * 64 = QM_LIST
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  const int c0 = s_cnt[0], total = c0 + s_cnt[1];
  static_assert(QM_WAVES == 2, "the two lists are read as one");
  if (total == 0) {  // the whole workgroup
    if (!FILL) {
      if (tid < QM_TILE) words[word_at + tid] = 0ull;
      if (tid == 0) {
        tile_pairs[tile] = 0;
        cover[tile] = 0ull;
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
    qm_inter2_iou(s_rows + gi * 4, s_rows + (QM_TILE + pj) * 4, s_ring + tid, &inter2);
    const int4 ga = s_rows[gi * 4 + 3], pa = s_rows[(QM_TILE + pj) * 4 + 3];
    if (ga.w == 0) {  // a don't-care gt: the coverage test, never a candidate (the fill never meets one: its words are zero)
      if (!FILL && inter2 >= qm_mul(cover_thr, (double)qm_area2(pa))) atomicOr(&s_cover, 1ull << pj);
      continue;
    }
    const long I = (long)__builtin_floor(inter2 < (double)LM_AREA_MAX ? inter2 : (double)LM_AREA_MAX);  // inter2 >= 0, never NaN
    const bool rec = 256L * I >= (long)tr_q8 * lm_area(qm_area2(ga));
    const bool prec = 256L * I >= (long)tp_q8 * lm_area(qm_area2(pa));
    if (!(I > 0 && (rec || prec))) continue;
    if (FILL) {
      const long slot = (long)rowoff[(long)b * (Mp + 1) + g0 + gi] + tpre[word_at + gi] +
                        __popcll(s_word[gi] & ((1ull << pj) - 1ull));
      if (slot >= 0 && slot < max_pairs)
        cand[(long)b * max_pairs + slot] = ((unsigned long long)I << (LM_PRED_BITS + 2)) |
                                           ((unsigned long long)prec << (LM_PRED_BITS + 1)) |
                                           ((unsigned long long)rec << LM_PRED_BITS) | (unsigned)(p0 + pj);
    } else {
      atomicOr(&s_word[gi], 1ull << pj);
    }
  }
  if (!FILL) {
    __syncthreads();
    if (tid < QM_TILE) words[word_at + tid] = s_word[tid];
    if (tid == 0) {
      tile_pairs[tile] = total;
      cover[tile] = s_cover;
    }
  }
}

// stats words 0, 1 and 7..11: n_gt (care gts), n_pred (preds taking part that are not ignored), n_dc, n_ignored, pairs,
// candidates, status.  The others are the phase kernel's.
__global__ __launch_bounds__(QM_BLOCK) void lm_scan_kernel(const int* __restrict__ gt_rows, const int* __restrict__ gt_count,
                                                            const unsigned char* __restrict__ gt_care,
                                                            const int* __restrict__ pred_rows,
                                                            const int* __restrict__ pred_count, int M, int N, int Mp, int NT,
                                                            int MT, unsigned long long* __restrict__ words,
                                                            const unsigned long long* __restrict__ cover,
                                                            unsigned long long* __restrict__ ignored, int* __restrict__ tpre,
                                                            const int* __restrict__ tile_pairs, int* __restrict__ rowoff,
                                                            long long* __restrict__ stats, int max_pairs) {
  __shared__ int s_cnt[QM_MAX];
  __shared__ int s_wave[QM_BLOCK / 64];
  __shared__ int s_sum[5];  // n_gt, n_dc, preds taking part, n_ignored, pairs
  __shared__ unsigned long long s_cov[QM_MAX / QM_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const int ng = qm_clamp(gt_count[b], M), np = qm_clamp(pred_count[b], N);
  if (t < 5) s_sum[t] = 0;
  int n_ign = 0;
  if (t < NT) {  // NT <= QM_MAX / QM_TILE <= QM_BLOCK
    unsigned long long w = 0ull;
    for (int tm = 0; tm < MT; ++tm) w |= cover[((long)b * MT + tm) * NT + t];
    s_cov[t] = w;
    ignored[(long)b * NT + t] = w;
    n_ign = __popcll(w);
  }
  __syncthreads();
  for (int g = t; g < Mp; g += QM_BLOCK) {  // Mp <= QM_MAX
    int run = 0;
#pragma unroll 8
    for (int tn = 0; tn < NT; ++tn) {
      const long at = ((long)b * NT + tn) * Mp + g;
      const unsigned long long w = words[at] & ~s_cov[tn];  // an ignored pred takes no further part
      words[at] = w;
      tpre[at] = run;
      run += __popcll(w);
    }
    s_cnt[g] = run;
  }
  int n_gt = 0, n_dc = 0, n_part = 0, pairs = 0;
  for (int g = t; g < ng; g += QM_BLOCK) {
    const bool part = gt_rows[((long)b * M + g) * 16 + 14] != 0, care = !gt_care || gt_care[(long)b * M + g] != 0;
    n_gt += part && care;
    n_dc += part && !care;
  }
  for (int p = t; p < np; p += QM_BLOCK) n_part += pred_rows[((long)b * N + p) * 16 + 14] != 0;
  for (int i = t; i < MT * NT; i += QM_BLOCK) pairs += tile_pairs[(long)b * MT * NT + i];  // <= M * N <= 2^26
  __syncthreads();
  n_gt = qm_wave_sum_i(n_gt);
  n_dc = qm_wave_sum_i(n_dc);
  n_part = qm_wave_sum_i(n_part);
  n_ign = qm_wave_sum_i(n_ign);
  pairs = qm_wave_sum_i(pairs);
  if (lane == 0) {
    atomicAdd(&s_sum[0], n_gt);
    atomicAdd(&s_sum[1], n_dc);
    atomicAdd(&s_sum[2], n_part);
    atomicAdd(&s_sum[3], n_ign);
    atomicAdd(&s_sum[4], pairs);
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
  if (t == 0) {
    rowoff[(long)b * (Mp + 1) + Mp] = all;
    long long* st = stats + (long)b * LM_STATS;
    st[0] = s_sum[0];
    st[1] = s_sum[2] - s_sum[3];
    st[7] = s_sum[1];
    st[8] = s_sum[3];
    st[9] = s_sum[4];
    st[10] = all;
    st[11] = all > max_pairs ? 1 : 0;
  }
}

// Phases A, B and C of one image.  Thread t owns the gts and the preds t + 1024 k.  LDS per pred: psum (the merge sum, a
// 64-bit integer), pint (phase A: the column count of Q; split rounds: the lowest gt that offers itself; merge rounds: the
// members of M_p that have not chosen p yet; once a pred is one-to-one or a split part: its gt, for good), pkind, pready;
// per gt: gkind and gbest (the pred of a one-to-one or merged gt; in a merge round the lowest ready pred among its own).  A
// step changes only what its own threads own, or adds / takes minima with integer atomics, and steps are separated by
// barriers: what a round decides, and the count of rounds, do not depend on the order in which threads run.  The lowest
// ready gt (pred) of a round always takes its set, and a set has at least two members, so the split rounds end within
// min(M, N / 2) and the merge rounds within min(N, M / 2); the loops are capped one above that.
__global__ __launch_bounds__(QM_BLOCK) void lm_phase_kernel(const int* __restrict__ gt_rows, const int* __restrict__ gt_count,
                                                             const unsigned char* __restrict__ gt_care,
                                                             const int* __restrict__ pred_rows,
                                                             const int* __restrict__ pred_count, int M, int N, int Mp, int NT,
                                                             int tr_q8, int tp_q8,
                                                             const unsigned long long* __restrict__ ignored,
                                                             const int* __restrict__ rowoff,
                                                             const unsigned long long* __restrict__ cand, int max_pairs,
                                                             unsigned char* __restrict__ gt_kind, int* __restrict__ gt_group,
                                                             unsigned char* __restrict__ pred_kind,
                                                             int* __restrict__ pred_group, long long* __restrict__ stats,
                                                             int* __restrict__ rounds) {
  extern __shared__ unsigned long long s_dyn[];
  __shared__ int s_any, s_out[5];
  unsigned long long* psum = s_dyn;                                          // N
  int* pint = reinterpret_cast<int*>(s_dyn + N);                             // N
  unsigned short* gbest = reinterpret_cast<unsigned short*>(pint + N);       // M
  unsigned char* pkind = reinterpret_cast<unsigned char*>(gbest + M);        // N
  unsigned char* pready = pkind + N;                                         // N
  unsigned char* gkind = pready + N;                                         // M
  const int t = threadIdx.x, b = blockIdx.x;
  const int ng = qm_clamp(gt_count[b], M), np = qm_clamp(pred_count[b], N);
  const bool over = stats[(long)b * LM_STATS + 11] != 0;  // uniform: an overflowed image gets no match
  const int* off = rowoff + (long)b * (Mp + 1);
  const unsigned long long* cw = cand + (long)b * max_pairs;
  constexpr unsigned long long PMASK = (1ull << LM_PRED_BITS) - 1ull, REC = 1ull << LM_PRED_BITS, PREC = REC << 1;
  for (int p = t; p < N; p += QM_BLOCK) {
    unsigned char k = LM_ABSENT;
    if (p < np && pred_rows[((long)b * N + p) * 16 + 14] != 0)
      k = ((ignored[(long)b * NT + (p >> 6)] >> (p & 63)) & 1ull) ? LM_APART : LM_FREE;
    pkind[p] = k;
    pint[p] = 0;
    psum[p] = 0ull;
    pready[p] = 0;
  }
  for (int g = t; g < M; g += QM_BLOCK) {
    unsigned char k = LM_ABSENT;
    if (g < ng && gt_rows[((long)b * M + g) * 16 + 14] != 0) k = (!gt_care || gt_care[(long)b * M + g] != 0) ? LM_FREE : LM_APART;
    gkind[g] = k;
    gbest[g] = LM_NONE;
  }
  if (t < 5) s_out[t] = 0;
  int done_split = 0, done_merge = 0;
  __syncthreads();
  if (!over) {
    // ---- phase A: the column counts of Q, then the pairs alone in their row and their column
    for (int g = t; g < ng; g += QM_BLOCK) {
      if (gkind[g] != LM_FREE) continue;
      const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
      for (int i = lo; i < hi; ++i) {
        const unsigned long long w = cw[i];
        const int p = (int)(w & PMASK);
        if ((w & REC) && (w & PREC) && p < N && pkind[p] == LM_FREE) atomicAdd(&pint[p], 1);
      }
    }
    __syncthreads();
    for (int g = t; g < ng; g += QM_BLOCK) {
      if (gkind[g] != LM_FREE) continue;
      const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
      int row = 0, only = -1;
      for (int i = lo; i < hi; ++i) {
        const unsigned long long w = cw[i];
        const int p = (int)(w & PMASK);
        // pkind is read for the Q entries of this row alone: a pred that another thread turns one-to-one in this step has
        // its one Q in that thread's row, so it is never read here
        if ((w & REC) && (w & PREC) && p < N && pkind[p] == LM_FREE) {
          ++row;
          only = p;
        }
      }
      if (row == 1 && pint[only] == 1) {  // only this thread's row holds a Q of that pred
        gkind[g] = LM_ONE;
        gbest[g] = (unsigned short)only;
        pkind[only] = LM_ONE;
        pint[only] = g;
      }
    }
    __syncthreads();
    // ---- phase B: the split rounds
    const int cap_split = min(M, N / 2) + 1;
    for (int round = 0; round < cap_split; ++round) {
      for (int p = t; p < N; p += QM_BLOCK)
        if (pkind[p] == LM_FREE) pint[p] = INT_MAX;
      if (t == 0) s_any = 0;
      __syncthreads();
      unsigned ready = 0;  // bit k: the owned gt t + 1024 k
      for (int g = t, k = 0; g < ng; g += QM_BLOCK, ++k) {
        if (gkind[g] != LM_FREE) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        long sum = 0;
        int cnt = 0;
        for (int i = lo; i < hi; ++i) {
          const unsigned long long w = cw[i];
          const int p = (int)(w & PMASK);
          if ((w & PREC) && p < N && pkind[p] == LM_FREE) {
            sum += (long)(w >> (LM_PRED_BITS + 2));
            ++cnt;
          }
        }
        const long ag = lm_area(((long)gt_rows[((long)b * M + g) * 16 + 13] << 32) | (unsigned)gt_rows[((long)b * M + g) * 16 + 12]);
        if (!(cnt >= 2 && 256L * sum >= (long)tr_q8 * ag)) continue;
        ready |= 1u << k;
        s_any = 1;
        for (int i = lo; i < hi; ++i) {
          const unsigned long long w = cw[i];
          const int p = (int)(w & PMASK);
          if ((w & PREC) && p < N && pkind[p] == LM_FREE) atomicMin(&pint[p], g);
        }
      }
      __syncthreads();
      const int any = s_any;
      if (!any) break;  // uniform
      ++done_split;
      for (int g = t, k = 0; g < ng; g += QM_BLOCK, ++k) {  // a ready gt takes its set iff it holds every pred of it
        if (!((ready >> k) & 1u)) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        bool all = true;
        for (int i = lo; i < hi; ++i) {
          const unsigned long long w = cw[i];
          const int p = (int)(w & PMASK);
          if ((w & PREC) && p < N && pkind[p] == LM_FREE) all = all && pint[p] == g;
        }
        if (all) gkind[g] = LM_SPLIT;
      }
      __syncthreads();
      for (int p = t; p < N; p += QM_BLOCK) {  // the preds of the gts that took their sets; pint keeps the gt
        if (pkind[p] != LM_FREE) continue;
        const int g = pint[p];
        if (g != INT_MAX && gkind[g] == LM_SPLIT) pkind[p] = LM_SPLIT;
      }
      __syncthreads();
    }
    // ---- phase C: the merge rounds
    const int cap_merge = min(N, M / 2) + 1;
    for (int round = 0; round < cap_merge; ++round) {
      for (int p = t; p < N; p += QM_BLOCK) {
        if (pkind[p] != LM_FREE) continue;
        pint[p] = 0;
        psum[p] = 0ull;
      }
      if (t == 0) s_any = 0;
      __syncthreads();
      for (int g = t; g < ng; g += QM_BLOCK) {  // every free gt adds itself to the sets of its free preds
        if (gkind[g] != LM_FREE) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        for (int i = lo; i < hi; ++i) {
          const unsigned long long w = cw[i];
          const int p = (int)(w & PMASK);
          if ((w & REC) && p < N && pkind[p] == LM_FREE) {
            atomicAdd(&psum[p], w >> (LM_PRED_BITS + 2));  // <= 8192 * 2^41
            atomicAdd(&pint[p], 1);
          }
        }
      }
      __syncthreads();
      for (int p = t; p < N; p += QM_BLOCK) {
        if (pkind[p] != LM_FREE) continue;
        const long ap = lm_area(((long)pred_rows[((long)b * N + p) * 16 + 13] << 32) | (unsigned)pred_rows[((long)b * N + p) * 16 + 12]);
        const bool r = pint[p] >= 2 && 256L * (long)psum[p] >= (long)tp_q8 * ap;
        pready[p] = r ? 1 : 0;
        if (r) s_any = 1;
      }
      __syncthreads();
      const int any = s_any;
      if (!any) break;  // uniform
      ++done_merge;
      for (int g = t; g < ng; g += QM_BLOCK) {  // a gt keeps the lowest ready pred that counts it
        if (gkind[g] != LM_FREE) continue;
        const int lo = max(off[g], 0), hi = min(off[g + 1], max_pairs);
        int m = -1;
        for (int i = lo; i < hi && m < 0; ++i) {  // preds ascend within a gt
          const unsigned long long w = cw[i];
          const int p = (int)(w & PMASK);
          if ((w & REC) && p < N && pkind[p] == LM_FREE && pready[p]) m = p;
        }
        gbest[g] = m < 0 ? LM_NONE : (unsigned short)m;
        if (m >= 0) atomicSub(&pint[m], 1);
      }
      __syncthreads();
      for (int g = t; g < ng; g += QM_BLOCK) {  // a ready pred that holds every gt of its set takes it
        if (gkind[g] != LM_FREE) continue;
        const int m = gbest[g];
        if (m != LM_NONE && pint[m] == 0) gkind[g] = LM_MERGE;
        else gbest[g] = LM_NONE;
      }
      __syncthreads();
      for (int p = t; p < N; p += QM_BLOCK)
        if (pkind[p] == LM_FREE && pready[p] && pint[p] == 0) pkind[p] = LM_MERGE;
      __syncthreads();
    }
  }
  __syncthreads();
  int c[5] = {0, 0, 0, 0, 0};  // one_to_one, split_gt, split_pred, merged_gt, merge_pred
  for (int g = t; g < M; g += QM_BLOCK) {
    const unsigned char k = gkind[g];
    gt_kind[(long)b * M + g] = k;
    gt_group[(long)b * M + g] = (k == LM_ONE || k == LM_MERGE) ? (int)gbest[g] : k == LM_SPLIT ? g : -1;
    c[0] += k == LM_ONE;
    c[1] += k == LM_SPLIT;
    c[3] += k == LM_MERGE;
  }
  for (int p = t; p < N; p += QM_BLOCK) {
    const unsigned char k = pkind[p];
    pred_kind[(long)b * N + p] = k;
    pred_group[(long)b * N + p] = (k == LM_ONE || k == LM_SPLIT) ? pint[p] : k == LM_MERGE ? p : -1;
    c[2] += k == LM_SPLIT;
    c[4] += k == LM_MERGE;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int v = qm_wave_sum_i(c[i]);
    if ((t & 63) == 0) atomicAdd(&s_out[i], v);
  }
  __syncthreads();
  long long* st = stats + (long)b * LM_STATS;
  if (t < 5) st[2 + t] = s_out[t];
  if (t == 5) st[12] = done_split;
  if (t == 6) st[13] = done_merge;
  if (t == 7) st[14] = 0;
  if (t == 8) st[15] = 0;
  if (t == 0 && rounds) {
    rounds[2 * b] = done_split;
    rounds[2 * b + 1] = done_merge;
  }
}

LmLayout lm_layout(int B, int M, int N, int max_pairs) {
  LmLayout l;
  l.MT = (int)vkas_cdiv(M, QM_TILE);
  l.NT = (int)vkas_cdiv(N, QM_TILE);
  l.Mp = l.MT * QM_TILE;
  const size_t tiles = (size_t)B * l.NT * l.Mp;
  l.words = 0;
  l.cand = qm_align(l.words + tiles * sizeof(unsigned long long));
  l.cover = qm_align(l.cand + (size_t)B * max_pairs * sizeof(unsigned long long));
  l.ignored = qm_align(l.cover + (size_t)B * l.MT * l.NT * sizeof(unsigned long long));
  l.tpre = qm_align(l.ignored + (size_t)B * l.NT * sizeof(unsigned long long));
  l.rowoff = qm_align(l.tpre + tiles * sizeof(int));
  l.tile_pairs = qm_align(l.rowoff + (size_t)B * (l.Mp + 1) * sizeof(int));
  l.bytes = qm_align(l.tile_pairs + (size_t)B * l.MT * l.NT * sizeof(int));
  return l;
}

int lm_check_dims(const char* what, int B, int M, int N, int max_pairs) {
  VKAS_CHECK(B >= 0 && B <= 65535, "%s: bad B=%d (0..65535)", what, B);
  VKAS_CHECK(M >= 1 && M <= QM_MAX && N >= 1 && N <= QM_MAX, "%s: M=%d and N=%d must lie in 1..%d", what, M, N, QM_MAX);
  VKAS_CHECK(max_pairs >= 0, "%s: max_pairs=%d must be >= 0", what, max_pairs);
  VKAS_CHECK((long)B * max_pairs < (1L << 31), "%s: B*max_pairs = %ld must stay below 2^31", what, (long)B * max_pairs);
  return VKAS_OK;
}

}  // namespace

extern "C" long long vkas_line_match_workspace_bytes(int B, int M, int N, int max_pairs) {
  if (lm_check_dims("vkas_line_match_workspace_bytes", B, M, N, max_pairs) != VKAS_OK) return -1;
  return (long long)lm_layout(B, M, N, max_pairs).bytes;
}

extern "C" int vkas_line_match(const int* gt_rows, const int* gt_count, const unsigned char* gt_care, const int* pred_rows,
                               const int* pred_count, int B, int M, int N, int tr_q8, int tp_q8, double cover_thr,
                               int max_pairs, void* workspace, size_t workspace_bytes, unsigned char* gt_kind, int* gt_group,
                               unsigned char* pred_kind, int* pred_group, long long* stats, int* rounds, void* stream) {
  const int rc = lm_check_dims("vkas_line_match", B, M, N, max_pairs);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(tr_q8 >= 1 && tr_q8 <= 256, "vkas_line_match: recall threshold tr_q8 = %d must lie in 1..256", tr_q8);
  VKAS_CHECK(tp_q8 >= 1 && tp_q8 <= 256, "vkas_line_match: precision threshold tp_q8 = %d must lie in 1..256", tp_q8);
  VKAS_CHECK(cover_thr > 0.0 && cover_thr <= 1.0, "vkas_line_match: cover_thr = %g must lie in (0, 1]", cover_thr);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(gt_rows && gt_count && pred_rows && pred_count && workspace && gt_kind && gt_group && pred_kind && pred_group &&
                 stats,
             "vkas_line_match: null pointer");
  VKAS_CHECK(vkas_aligned16(gt_rows) && vkas_aligned16(pred_rows) && vkas_aligned16(workspace),
             "vkas_line_match: the row tables and the workspace must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)stats) & 7u) == 0 && (((uintptr_t)gt_group) & 3u) == 0 && (((uintptr_t)pred_group) & 3u) == 0,
             "vkas_line_match: stats must be 8-byte aligned, gt_group and pred_group 4-byte aligned");
  const LmLayout l = lm_layout(B, M, N, max_pairs);
  VKAS_CHECK(workspace_bytes >= l.bytes, "vkas_line_match: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  // the phases keep 14 bytes per pred and 3 per gt in LDS: above the default 64 KB the kernel is opted in, once
  const size_t lds = lm_lds_bytes(M, N);
  static size_t lds_allowed = 48 * 1024;
  if (lds > lds_allowed) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lm_phase_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lm_lds_bytes(QM_MAX, QM_MAX));
    if (e != hipSuccess) {
      vkas_set_error("vkas_line_match: %zu bytes of LDS for M = %d, N = %d refused: %s", lds, M, N, hipGetErrorString(e));
      return VKAS_E_LAUNCH;
    }
    lds_allowed = lm_lds_bytes(QM_MAX, QM_MAX);
  }
  char* ws = static_cast<char*>(workspace);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + l.words);
  unsigned long long* cand = reinterpret_cast<unsigned long long*>(ws + l.cand);
  unsigned long long* cover = reinterpret_cast<unsigned long long*>(ws + l.cover);
  unsigned long long* ignored = reinterpret_cast<unsigned long long*>(ws + l.ignored);
  int* tpre = reinterpret_cast<int*>(ws + l.tpre);
  int* rowoff = reinterpret_cast<int*>(ws + l.rowoff);
  int* tile_pairs = reinterpret_cast<int*>(ws + l.tile_pairs);
  hipStream_t s = vkas_stream(stream);
  const dim3 grid((unsigned)l.NT, (unsigned)l.MT, (unsigned)B);
  lm_pair_kernel<false><<<grid, QM_THREADS, 0, s>>>(gt_rows, gt_count, gt_care, pred_rows, pred_count, M, N, l.Mp, l.NT, tr_q8,
                                                    tp_q8, cover_thr, words, cover, tpre, tile_pairs, rowoff, stats, cand,
                                                    max_pairs);
  VKAS_LAUNCH_CHECK("line_match pairs");
  lm_scan_kernel<<<B, QM_BLOCK, 0, s>>>(gt_rows, gt_count, gt_care, pred_rows, pred_count, M, N, l.Mp, l.NT, l.MT, words, cover,
                                        ignored, tpre, tile_pairs, rowoff, stats, max_pairs);
  VKAS_LAUNCH_CHECK("line_match scan");
  lm_pair_kernel<true><<<grid, QM_THREADS, 0, s>>>(gt_rows, gt_count, gt_care, pred_rows, pred_count, M, N, l.Mp, l.NT, tr_q8,
                                                   tp_q8, cover_thr, words, cover, tpre, tile_pairs, rowoff, stats, cand,
                                                   max_pairs);
  VKAS_LAUNCH_CHECK("line_match fill");
  lm_phase_kernel<<<B, QM_BLOCK, lds, s>>>(gt_rows, gt_count, gt_care, pred_rows, pred_count, M, N, l.Mp, l.NT, tr_q8, tp_q8,
                                           ignored, rowoff, cand, max_pairs, gt_kind, gt_group, pred_kind, pred_group, stats,
                                           rounds);
  VKAS_LAUNCH_CHECK("line_match rounds");
  return VKAS_OK;
}
