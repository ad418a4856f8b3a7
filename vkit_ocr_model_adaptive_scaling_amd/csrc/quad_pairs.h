// The three passes over pairs of match rows that every pair-based op runs before its own rounds kernel (quadmatch.hip: the
// one-to-one, the self and the ranked matching of character quads; linematch.hip: the text-line score; ribbonmatch.hip:
// the same score with every line a ribbon of quads), stated once:
//
//   count  qp_tile<false>  a 128-thread workgroup owns a 64 gt x 64 pred tile of one image.  The boxes and valid words of its
//                          128 rows go to LDS; wave w box-tests gts [32w, 32w + 32) against pred = lane and appends the
//                          overlapping valid pairs the rule admits to its LDS list at the ballot's prefix count (a list is
//                          bounded by the tile, QM_LIST: no overflow path).  A tile without a pair - most tiles of a page -
//                          ends there.  Otherwise the corners follow and all threads take pairs from the two lists, so the
//                          clip is balanced whatever the tile holds.  A pair the rule calls a candidate sets bit pj of the
//                          tile's 64-bit word of its gt (LDS atomic OR: integer, order-free).  Out: the tile's words, its
//                          pair count and what the rule keeps per tile.
//   scan   qp_scan         one workgroup per image: per gt the prefix of the words' popcounts over the pred tiles, then the
//                          exclusive scan over the gts = the CSR row offsets; the caller's own sums ride on its barriers.
//   fill   qp_tile<true>   the same tile body with the stored words in place of the box test: only candidates are clipped
//                          again (same code, same bits), each stored at  row offset + tile prefix + popcount of the lower
//                          bits: no slot atomics, preds ascending within a gt.  A tile whose words are all zero ends on
//                          them, and an image with status set is skipped.
//
// A Rule is a struct of __device__ __forceinline__ members, passed to the kernel by value and resolved at compile time; it
// derives from QpRule, which holds the members most rules leave alone:
//
//   Tile                          what the counting pass keeps per tile in LDS beside the words (none: an empty struct)
//   begin(s, tid)                 clears it
//   fix(v, is_gt, b, M, N, at, part)   rewrites a row's part as it is staged (qm_stage_half)
//   admit(g3, p3, g, p)           the test before the clip, on part 3 of both rows and their indices
//   status(b)                     the image's status word, as the scan left it
//   pair<FILL>(s, g3, p3, pj, iou, inter2, val)   what a clipped pair means: true = a candidate, val = what its slot holds
//                                 beside the pred; side effects go to s (counting pass only)
//   PAIR_LANES, group_inter2(g, p, b, ring, lane)   1: a listed pair is one thread's work and its quantity the clip of the
//                                 two rows (qm_inter2_iou).  L = 2..64, a power of two: a listed pair is the work of L
//                                 neighbouring lanes of one wave, the rule computes the quantity itself from the two
//                                 LDS rows (all L lanes call with lane = 0..L-1 and all get the same value; iou is 0),
//                                 and lane 0 of the group alone goes on to pair() and the store
//   store(at, pred, val)          fills slot `at` (image and slot in one index)
//   apart(s)                      the tile's pairs that its pair count leaves out
//   tile_out(s, tile, tid)        the rule's outputs per tile; an empty tile takes the same path with s as begin left it
//
// Table reads are bounded by the tables' K rows (a row beyond the clamped count is dropped after its load), ring stores by
// QM_RING, candidate stores by max_pairs, tile stores by the padded tile grid the workspace is sized for: no table content
// makes a pass touch memory outside its buffers.  No float atomics, no allocation, no synchronisation: capture-safe and
// bit-identical from run to run.  The host half - the dimension check, the layout of the four common workspace arrays and
// the LDS opt-in of a rounds kernel - is at the end.
#pragma once
#include "quad_clip.h"

namespace {

// the tables of a call and the workspace arrays the three passes share
struct QpTables {
  const int* gt_rows;
  const int* gt_count;
  const int* pred_rows;
  const int* pred_count;
  int M, N, Mp, MT, NT, max_pairs;
  unsigned long long* words;  // (B, NT, Mp)
  int* tpre;                  // (B, NT, Mp)
  int* tile_pairs;            // (B, MT * NT)
  int* rowoff;                // (B, Mp + 1)
};

struct QpRule {
  static constexpr int PAIR_LANES = 1;
  struct Tile {};
  template <class S> __device__ __forceinline__ void begin(S&, int) const {}
  __device__ __forceinline__ void fix(int4&, bool, int, int, int, int, int) const {}
  __device__ __forceinline__ bool admit(const int4&, const int4&, int, int) const { return true; }
  template <class S> __device__ __forceinline__ int apart(const S&) const { return 0; }
  template <class S> __device__ __forceinline__ void tile_out(const S&, long, int) const {}
};

// what rides in the zero word of part 3: a pred's (or self row's) prob bits, the row losing its valid word unless the prob
// is finite; a gt's care flag (no table = every gt is a care gt)
__device__ __forceinline__ void qp_fix_prob(int4& v, const float* probs, long at) {
  const unsigned pb = __float_as_uint(probs[at]);
  v.z = (v.z != 0 && qm_finite_bits(pb)) ? 1 : 0;
  v.w = (int)pb;
}
__device__ __forceinline__ void qp_fix_care(int4& v, const unsigned char* gt_care, long at) {
  v.w = gt_care ? (gt_care[at] != 0 ? 1 : 0) : 1;
}
// the valid word of row i of image b in a (B, K, 16) table
__device__ __forceinline__ bool qp_valid(const int* rows, int K, int b, int i) { return rows[((long)b * K + i) * 16 + 14] != 0; }
// the coverage test of a don't-care gt: inter2 >= cover_thr * area2_p, the product rounded once
__device__ __forceinline__ bool qp_covers(double cover_thr, double inter2, const int4& p3) {
  return inter2 >= qm_mul(cover_thr, (double)qm_area2(p3));
}

template <bool FILL, class Rule>
__device__ __forceinline__ void qp_tile(const QpTables& t, const Rule& r) {
  __shared__ int4 s_rows[2 * QM_TILE * 4];
  __shared__ unsigned long long s_word[QM_TILE];
  __shared__ unsigned short s_list[QM_WAVES * QM_LIST];
  __shared__ int s_cnt[QM_WAVES];
  __shared__ double s_ring[2 * QM_RING * 2 * QM_THREADS];
  __shared__ typename Rule::Tile s_rule;  // the counting pass only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tn = blockIdx.x, tm = blockIdx.y, b = blockIdx.z;
  const int g0 = tm * QM_TILE, p0 = tn * QM_TILE;
  const long word_at = ((long)b * t.NT + tn) * t.Mp + g0;
  const long tile = ((long)b * gridDim.y + tm) * t.NT + tn;
  // Most tiles of a page end early: the status, the counts, the words and (below) the rows are read at addresses that depend
  // on no other load, so such a workgroup lives one load's latency.  Every early return is taken by the whole workgroup.
  const long long status = FILL ? r.status(b) : 0;
  const int ng = qm_clamp(t.gt_count[b], t.M), np = qm_clamp(t.pred_count[b], t.N);
  if (FILL && status != 0) return;  // nothing of this image is stored
  unsigned long long word = 0ull;
  if (FILL && tid < QM_TILE) word = t.words[word_at + tid];
  // a part of the 128 rows of the tile: 0, 1 = the corners, 2 = the box, 3 = area and valid (qm_stage_half)
  const auto fix = [&](int4& v, bool is_gt, int at, int part) { r.fix(v, is_gt, b, t.M, t.N, at, part); };
  const auto stage = [&](int half) {
    qm_stage_half(s_rows, t.gt_rows, t.pred_rows, b, t.M, t.N, g0, p0, ng, np, half, tid, fix);
  };
  if (tid < QM_TILE) s_word[tid] = word;
  if (!FILL) r.begin(s_rule, tid);
  if (FILL) {  // most tiles of a page hold no candidate: they end here, on 512 bytes
    __syncthreads();
    if (__ballot(s_word[lane] != 0ull) == 0ull) return;
  }
  stage(1);  // the box test needs boxes and valid only; a tile without a pair ends on them
  __syncthreads();

  const int4 pbox = s_rows[(QM_TILE + lane) * 4 + 2], p3 = s_rows[(QM_TILE + lane) * 4 + 3];
  int cnt = 0;
  for (int s = 0; s < QM_TILE / QM_WAVES; ++s) {
    const int gi = wave * (QM_TILE / QM_WAVES) + s;
    bool hit;
    if (FILL) {
      hit = (s_word[gi] >> lane) & 1ull;
    } else {
      const int4 gbox = s_rows[gi * 4 + 2], g3 = s_rows[gi * 4 + 3];
      hit = p3.z != 0 && g3.z != 0 && gbox.x <= pbox.z && pbox.x <= gbox.z && gbox.y <= pbox.w && pbox.y <= gbox.w &&
            r.admit(g3, p3, g0 + gi, p0 + lane);
    }
    const unsigned long long bits = __ballot(hit);
    if (hit) s_list[wave * QM_LIST + cnt + __popcll(bits & ((1ull << lane) - 1ull))] = (unsigned short)(gi * QM_TILE + lane);
    cnt += __popcll(bits);  // <= 32 * 64 = QM_LIST
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  const int c0 = s_cnt[0], total = c0 + s_cnt[1];
  static_assert(QM_WAVES == 2, "the two lists are read as one");
  const auto tile_out = [&]() {  // the counting pass: the words, the pair count, the rule's own
    if (tid < QM_TILE) t.words[word_at + tid] = s_word[tid];
    if (tid == 0) t.tile_pairs[tile] = total - r.apart(s_rule);
    r.tile_out(s_rule, tile, tid);
  };
  if (total == 0) {  // the whole workgroup; s_word and s_rule are as they were cleared, two barriers ago
    if (!FILL) tile_out();
    return;
  }
  stage(0);
  __syncthreads();
  const auto settle = [&](int gi, int pj, double iou, double inter2) {  // what the rule makes of a clipped pair
    unsigned long long val = 0ull;
    if (!r.template pair<FILL>(s_rule, s_rows[gi * 4 + 3], s_rows[(QM_TILE + pj) * 4 + 3], pj, iou, inter2, val)) return;
    if (FILL) {
      const long slot = (long)t.rowoff[(long)b * (t.Mp + 1) + g0 + gi] + t.tpre[word_at + gi] +
                        __popcll(s_word[gi] & ((1ull << pj) - 1ull));
      if (slot >= 0 && slot < t.max_pairs) r.store((long)b * t.max_pairs + slot, p0 + pj, val);
    } else {
      atomicOr(&s_word[gi], 1ull << pj);
    }
  };
  constexpr int PL = Rule::PAIR_LANES;
  static_assert(PL >= 1 && PL <= 64 && (PL & (PL - 1)) == 0, "a group of lanes lies inside one wave");
  for (int e = tid / PL; e < total; e += QM_THREADS / PL) {
    const int q = e < c0 ? s_list[e] : s_list[QM_LIST + e - c0];
    const int gi = q >> 6, pj = q & 63;
    if constexpr (PL > 1) {  // e is uniform over the group: all its lanes are in the call, one settles
      const double inter2 = r.group_inter2(s_rows + gi * 4, s_rows + (QM_TILE + pj) * 4, b, s_ring + tid, tid % PL);
      if (tid % PL == 0) settle(gi, pj, 0.0, inter2);
    } else {
      double inter2;
      const double iou = qm_inter2_iou(s_rows + gi * 4, s_rows + (QM_TILE + pj) * 4, s_ring + tid, &inter2);
      settle(gi, pj, iou, inter2);
    }
  }
  if (!FILL) {
    __syncthreads();
    tile_out();
  }
}

// The scan of one image by its one workgroup of QM_BLOCK threads: tpre, rowoff (Mp + 1 words), and the return value = the
// image's candidates.  mask, if given, holds one word per pred tile in LDS, written before a barrier: its preds lose their
// bits, and the masked words are written back.  sums are this thread's K counts for the caller: they are added up into
// s_sum[0..K), and the image's pairs into s_sum[K]; s_sum is zeroed by the caller before the call (no barrier needed) and
// is complete on return.  Two barriers, reached by every thread.
template <int K>
__device__ __forceinline__ int qp_scan(const QpTables& t, int b, const unsigned long long* mask, const int (&sums)[K], int* s_sum) {
  __shared__ int s_cnt[QM_MAX];
  __shared__ int s_wave[QM_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int g = tid; g < t.Mp; g += QM_BLOCK) {  // Mp <= QM_MAX
    int run = 0;
#pragma unroll 8
    for (int tn = 0; tn < t.NT; ++tn) {
      const long at = ((long)b * t.NT + tn) * t.Mp + g;
      unsigned long long w = t.words[at];
      if (mask) {
        w &= ~mask[tn];
        t.words[at] = w;
      }
      t.tpre[at] = run;
      run += __popcll(w);
    }
    s_cnt[g] = run;
  }
  int pairs = 0;
  for (int i = tid; i < t.MT * t.NT; i += QM_BLOCK) pairs += t.tile_pairs[(long)b * t.MT * t.NT + i];  // <= M * N <= 2^26
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int v = qm_wave_sum_i(sums[k]);
    if (lane == 0) atomicAdd(&s_sum[k], v);
  }
  pairs = qm_wave_sum_i(pairs);
  if (lane == 0) atomicAdd(&s_sum[K], pairs);
  // exclusive scan of s_cnt: each thread owns a contiguous run of gts
  const int seg = (t.Mp + QM_BLOCK - 1) / QM_BLOCK;
  const int lo = min(t.Mp, tid * seg), hi = min(t.Mp, lo + seg);
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
    t.rowoff[(long)b * (t.Mp + 1) + g] = run;
    run += s_cnt[g];
  }
  if (tid == 0) t.rowoff[(long)b * (t.Mp + 1) + t.Mp] = all;
  return all;
}

// ---- host ------------------------------------------------------------------------------------------------------------

int qp_check_dims(const char* what, int B, int M, int N, int max_pairs) {
  VKAS_CHECK(B >= 0 && B <= 65535, "%s: bad B=%d (0..65535)", what, B);
  VKAS_CHECK(M >= 1 && M <= QM_MAX && N >= 1 && N <= QM_MAX, "%s: M=%d and N=%d must lie in 1..%d", what, M, N, QM_MAX);
  VKAS_CHECK(max_pairs >= 0, "%s: max_pairs=%d must be >= 0", what, max_pairs);
  VKAS_CHECK((long)B * max_pairs < (1L << 31), "%s: B*max_pairs = %ld must stay below 2^31", what, (long)B * max_pairs);
  return VKAS_OK;
}

// workspace: words (B, NT, Mp) u64, tpre (B, NT, Mp) int, rowoff (B, Mp + 1) int, tile_pairs (B, MT * NT) int; a caller's own
// arrays follow from `bytes` on, each qm_align-ed
struct QpLayout {
  size_t words, tpre, rowoff, tile_pairs, bytes;
  int MT, NT, Mp;
  size_t tiles;  // B * MT * NT
};

QpLayout qp_layout(int B, int M, int N) {
  QpLayout l;
  l.MT = (int)vkas_cdiv(M, QM_TILE);
  l.NT = (int)vkas_cdiv(N, QM_TILE);
  l.Mp = l.MT * QM_TILE;
  l.tiles = (size_t)B * l.MT * l.NT;
  const size_t words = (size_t)B * l.NT * l.Mp;
  l.words = 0;
  l.tpre = qm_align(l.words + words * sizeof(unsigned long long));
  l.rowoff = qm_align(l.tpre + words * sizeof(int));
  l.tile_pairs = qm_align(l.rowoff + (size_t)B * (l.Mp + 1) * sizeof(int));
  l.bytes = qm_align(l.tile_pairs + l.tiles * sizeof(int));
  return l;
}

template <class T>
T* qp_at(void* workspace, size_t offset) {
  return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset);
}

QpTables qp_tables(const int* gt_rows, const int* gt_count, const int* pred_rows, const int* pred_count, int M, int N,
                   int max_pairs, void* ws, const QpLayout& l) {
  return QpTables{gt_rows, gt_count, pred_rows, pred_count, M, N, l.Mp, l.MT, l.NT, max_pairs,
                  qp_at<unsigned long long>(ws, l.words), qp_at<int>(ws, l.tpre), qp_at<int>(ws, l.tile_pairs),
                  qp_at<int>(ws, l.rowoff)};
}

// A rounds kernel that keeps its per-image state in `need` bytes of dynamic LDS: above the default 48 KB the kernel is opted
// in to `most` (its need at QM_MAX), once per kernel.
template <auto Kernel>
int qp_allow_lds(const char* what, size_t need, size_t most) {
  static size_t allowed = 48 * 1024;
  if (need <= allowed) return VKAS_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)most);
  if (e != hipSuccess) {
    vkas_set_error("%s: %zu bytes of LDS refused: %s", what, need, hipGetErrorString(e));
    return VKAS_E_LAUNCH;
  }
  allowed = most;
  return VKAS_OK;
}

}  // namespace
