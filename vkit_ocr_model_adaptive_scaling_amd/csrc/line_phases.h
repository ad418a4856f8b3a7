// What the two text-line scores are made of (linematch.hip: lines as quads; ribbonmatch.hip: lines as ribbons of quads):
// the pair rule, the scan, the phases, the workspace layout and the argument check.  rows (B, K, 16) int32 are match rows,
// or ribbon rows, which hold the count, valid, area and care words where a match row does - the scan and the phases read
// no other word of a row.
//
//   LmRule           a pair with a don't-care gt takes the coverage test of the ranked matching and sets the pred's bit of the
//                    tile's cover word; a care pair takes I = floor(min(inter2, 2^41)) and the two integer tests rec_ok /
//                    prec_ok on the clamped areas, and is a candidate when I > 0 and one of them holds.  Its slot holds one
//                    64-bit word  I << 15 | prec_ok << 14 | rec_ok << 13 | pred.
//   lm_scan_kernel   the cover words OR-ed down the gt tiles = the ignored preds (kept as B x NT words), which are the scan's
//                    mask: every candidate word loses their bits; n_gt, n_pred, n_dc, n_ignored, pairs, candidates, status.
//   lm_phase_kernel  one workgroup per image: phase A (row and column counts of Q, integer LDS atomics), the split rounds,
//                    the merge rounds, then one sweep that writes every output.
//
// Integer atomics only (add, min on 32 and 64-bit words in LDS): nothing depends on arrival order.  A pred index read back
// from a candidate word is checked against N.  Every output word and every workspace word that is read is written earlier
// in the same call.
#pragma once
#include "quad_pairs.h"

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

struct LmRule : QpRule {
  const unsigned char* gt_care;  // (B, M), 0 = don't care; null = every gt is a care gt
  int tr_q8, tp_q8;
  double cover_thr;
  unsigned long long* cover;     // (B, MT * NT): per tile, bit j = pred j of the tile is covered by a don't-care gt of the tile
  long long* stats;              // (B, 16)
  unsigned long long* cand;      // (B, max_pairs)
  struct Tile {
    unsigned long long cover;
  };
  __device__ __forceinline__ void begin(Tile& s, int tid) const {
    if (tid == 0) s.cover = 0ull;
  }
  __device__ __forceinline__ void fix(int4& v, bool is_gt, int b, int M, int, int at, int part) const {
    if (part == 3 && is_gt) qp_fix_care(v, gt_care, (long)b * M + at);  // the care flag rides in the gt row's zero word
  }
  __device__ __forceinline__ long long status(int b) const { return stats[(long)b * LM_STATS + 11]; }
  template <bool FILL>
  __device__ __forceinline__ bool pair(Tile& s, const int4& g3, const int4& p3, int pj, double, double inter2,
                                       unsigned long long& val) const {
    if (g3.w == 0) {  // a don't-care gt: the coverage test, never a candidate (the fill never meets one: its words are zero)
      if (!FILL && qp_covers(cover_thr, inter2, p3)) atomicOr(&s.cover, 1ull << pj);
      return false;
    }
    const long I = (long)__builtin_floor(inter2 < (double)LM_AREA_MAX ? inter2 : (double)LM_AREA_MAX);  // inter2 >= 0, never NaN
    const bool rec = 256L * I >= (long)tr_q8 * lm_area(qm_area2(g3));
    const bool prec = 256L * I >= (long)tp_q8 * lm_area(qm_area2(p3));
    val = ((unsigned long long)I << (LM_PRED_BITS + 2)) | ((unsigned long long)prec << (LM_PRED_BITS + 1)) |
          ((unsigned long long)rec << LM_PRED_BITS);
    return I > 0 && (rec || prec);
  }
  __device__ __forceinline__ void store(long at, int pred, unsigned long long val) const { cand[at] = val | (unsigned)pred; }
  __device__ __forceinline__ void tile_out(const Tile& s, long tile, int tid) const {
    if (tid == 0) cover[tile] = s.cover;
  }
};

template <bool FILL>
__global__ __launch_bounds__(QM_THREADS) void lm_pair_kernel(const QpTables t, const LmRule r) {
  qp_tile<FILL>(t, r);
}

// stats words 0, 1 and 7..11: n_gt (care gts), n_pred (preds taking part that are not ignored), n_dc, n_ignored, pairs,
// candidates, status.  The others are the phase kernel's.
__global__ __launch_bounds__(QM_BLOCK) void lm_scan_kernel(const QpTables t, const LmRule r,
                                                            unsigned long long* __restrict__ ignored) {
  __shared__ int s_sum[5];  // n_gt, n_dc, preds taking part, n_ignored, pairs
  __shared__ unsigned long long s_cov[QM_MAX / QM_TILE];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int ng = qm_clamp(t.gt_count[b], t.M), np = qm_clamp(t.pred_count[b], t.N);
  if (tid < 5) s_sum[tid] = 0;
  int sums[4] = {0, 0, 0, 0};
  if (tid < t.NT) {  // NT <= QM_MAX / QM_TILE <= QM_BLOCK
    unsigned long long w = 0ull;
    for (int tm = 0; tm < t.MT; ++tm) w |= r.cover[((long)b * t.MT + tm) * t.NT + tid];
    s_cov[tid] = w;
    ignored[(long)b * t.NT + tid] = w;
    sums[3] = __popcll(w);
  }
  __syncthreads();
  for (int g = tid; g < ng; g += QM_BLOCK) {
    const bool part = qp_valid(t.gt_rows, t.M, b, g), care = !r.gt_care || r.gt_care[(long)b * t.M + g] != 0;
    sums[0] += part && care;
    sums[1] += part && !care;
  }
  for (int p = tid; p < np; p += QM_BLOCK) sums[2] += qp_valid(t.pred_rows, t.N, b, p);
  const int all = qp_scan(t, b, s_cov, sums, s_sum);  // an ignored pred takes no further part
  if (tid == 0) {
    long long* st = r.stats + (long)b * LM_STATS;
    st[0] = s_sum[0];
    st[1] = s_sum[2] - s_sum[3];
    st[7] = s_sum[1];
    st[8] = s_sum[3];
    st[9] = s_sum[4];
    st[10] = all;
    st[11] = all > t.max_pairs ? 1 : 0;
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

// workspace: QpLayout's, then cand (B, max_pairs) u64, cover (B, MT * NT) u64, ignored (B, NT) u64
struct LmLayout : QpLayout {
  size_t cand, cover, ignored;
};

LmLayout lm_layout(int B, int M, int N, int max_pairs) {
  LmLayout l{qp_layout(B, M, N)};
  l.cand = l.bytes;
  l.cover = qm_align(l.cand + (size_t)B * max_pairs * sizeof(unsigned long long));
  l.ignored = qm_align(l.cover + l.tiles * sizeof(unsigned long long));
  l.bytes = qm_align(l.ignored + (size_t)B * l.NT * sizeof(unsigned long long));
  return l;
}

// What the two entries hold their arguments to before any launch: the dimensions, the three thresholds, the pointers and
// their alignment, the workspace.  `what` names the entry in the error.
int lm_check_args(const char* what, const int* gt_rows, const int* gt_count, const int* pred_rows, const int* pred_count, int B,
                  int M, int N, int tr_q8, int tp_q8, double cover_thr, int max_pairs, const void* workspace,
                  size_t workspace_bytes, const unsigned char* gt_kind, const int* gt_group, const unsigned char* pred_kind,
                  const int* pred_group, const long long* stats) {
  const int rc = qp_check_dims(what, B, M, N, max_pairs);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(tr_q8 >= 1 && tr_q8 <= 256, "%s: recall threshold tr_q8 = %d must lie in 1..256", what, tr_q8);
  VKAS_CHECK(tp_q8 >= 1 && tp_q8 <= 256, "%s: precision threshold tp_q8 = %d must lie in 1..256", what, tp_q8);
  VKAS_CHECK(cover_thr > 0.0 && cover_thr <= 1.0, "%s: cover_thr = %g must lie in (0, 1]", what, cover_thr);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(gt_rows && gt_count && pred_rows && pred_count && workspace && gt_kind && gt_group && pred_kind && pred_group &&
                 stats,
             "%s: null pointer", what);
  VKAS_CHECK(vkas_aligned16(gt_rows) && vkas_aligned16(pred_rows) && vkas_aligned16(workspace),
             "%s: the row tables and the workspace must be 16-byte aligned", what);
  VKAS_CHECK((((uintptr_t)stats) & 7u) == 0 && (((uintptr_t)gt_group) & 3u) == 0 && (((uintptr_t)pred_group) & 3u) == 0,
             "%s: stats must be 8-byte aligned, gt_group and pred_group 4-byte aligned", what);
  const size_t need = lm_layout(B, M, N, max_pairs).bytes;
  VKAS_CHECK(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  return VKAS_OK;
}

}  // namespace
