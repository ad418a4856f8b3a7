// Grouping character quadrilaterals into text lines (inferencing/lines.py holds the rule - this project's own, all integer -
// and the host oracle quad_lines_host).  rows (B, K, 16) int32 match rows as in quadmatch.hip; per quad, in int64,
// s = P0+P1+P2+P3, v = (P3+P2)-(P0+P1), u = (P1+P2)-(P0+P3), vv = v.v.  Eight launches on one stream:
//
//   ql_init_kernel     parent[i] = i for a row that takes part (within the count, valid word set), -1 otherwise; line and
//                      order to -1; table rows to (0, 0, 0, 0, max, min, max, min); stats to (n, 0, 0, 0)
//   ql_link_kernel     a 256-thread workgroup owns a 64 x 64 tile of (i, j) pairs of one image, upper-triangle tiles only.
//                      The frames of its 128 rows go to LDS; wave w tests i in [16w, 16w + 16) against j = lane, i < j.  A
//                      linked pair is united on the global parent array (the atomicMin union of regions.hip: the larger
//                      root under the smaller, a lost race continues with the displaced parent; finds halve their path
//                      by atomicMin as they go) and counted by ballot; one 64-bit atomicAdd per wave with links.
//   ql_flatten_kernel  root[i] = the root of i = its line's smallest member (reads only)
//   ql_number_kernel   one workgroup per image: thread t owns a run of consecutive quads, counts its roots, the workgroup
//                      scans the counts, and line[i] = the roots in front of root[i] (numbers held in LDS); n_part, lines
//   ql_sum_kernel      per member: size += 1 and U += u on the line's table row (64-bit integer atomicAdd; a wave whose lanes
//                      all belong to one line adds once)
//   ql_start_kernel    one workgroup per image: start = exclusive scan of the sizes; U = (0, 0) becomes (0, 16); rows from
//                      L on are zeroed
//   ql_extent_kernel   per member: key = s.U to the workspace; a = P.U and b = P_y U_x - P_x U_y of its four corners into the
//                      row's a_min, a_max, b_min, b_max (64-bit integer atomicMin / atomicMax, once per uniform wave)
//   ql_rank_kernel     a workgroup owns 64 members i (lane) and walks all n rows j in LDS chunks, a quarter per wave: the
//                      position of i is the number of members of its line with a smaller (key, index);
//                      order[start + position] = i.  No atomics.
//
// Every loop is bounded by the data: a parent is never larger than its child and links only ever lower a parent, so a find
// from a ends within a steps and a union retries only after some parent went down.  No workgroup waits on another;
// ordering comes from the kernel boundaries alone.  Integer arithmetic only (the atomics are integer adds, minima and maxima:
// order-free), no allocation, no synchronisation: capture-safe and bit-identical from run to run.  Row reads are bounded
// by K, and every store index is an in-range quad index, a line number below the number of roots or start + position
// below n_part: no table content makes a kernel touch memory outside its buffers.
#include "vkas_common.h"

#include <limits.h>

namespace {

constexpr int QL_TILE = 64;      // quads per tile side
constexpr int QL_THREADS = 256;  // pair, rank and per-quad passes
constexpr int QL_MAX = 8192;     // quads per image (the LDS state of the numbering pass)
constexpr int QL_BLOCK = 1024;   // per-image passes
constexpr int QL_PER = QL_MAX / QL_BLOCK;
constexpr int QL_TABLE = 8;      // start, size, U_y, U_x, a_min, a_max, b_min, b_max
constexpr int QL_STATS = 4;      // n, n_part, links, lines
constexpr int QL_CHUNK = 1024;   // rows per LDS chunk of the rank pass

typedef unsigned long long u64;

__device__ __forceinline__ int ql_clamp(int v, int hi) { return min(max(v, 0), hi); }
__device__ __forceinline__ long ql_abs(long v) { return v < 0 ? -v : v; }

struct QlFrame {
  long sy, sx, vy, vx, uy, ux, vv;
};

// the corners of a row as two int4 -> its frame
__device__ __forceinline__ QlFrame ql_frame(const int4 a, const int4 c) {
  const long p0y = a.x, p0x = a.y, p1y = a.z, p1x = a.w, p2y = c.x, p2x = c.y, p3y = c.z, p3x = c.w;
  QlFrame f;
  f.sy = p0y + p1y + p2y + p3y;
  f.sx = p0x + p1x + p2x + p3x;
  f.vy = (p3y + p2y) - (p0y + p1y);
  f.vx = (p3x + p2x) - (p0x + p1x);
  f.uy = (p1y + p2y) - (p0y + p3y);
  f.ux = (p1x + p2x) - (p0x + p3x);
  f.vv = f.vy * f.vy + f.vx * f.vx;
  return f;
}

__device__ __forceinline__ bool ql_linked(long siy, long six, long viy, long vix, long vvi, long sjy, long sjx, long vjy,
                                          long vjx, long vvj, long gap, long cross, long ratio2) {
  const long dy = sjy - siy, dx = sjx - six;
  if (8 * ql_abs(dy * vix - dx * viy) > gap * vvi || 8 * ql_abs(dy * vjx - dx * vjy) > gap * vvj) return false;
  if (8 * ql_abs(dy * viy + dx * vix) > cross * vvi || 8 * ql_abs(dy * vjy + dx * vjx) > cross * vvj) return false;
  if (256 * vvi > ratio2 * vvj || 256 * vvj > ratio2 * vvi) return false;
  return viy * vjy + vix * vjx > 0;
}

// ---- union-find on the global parent array: a parent is never larger than its child, a root is its own parent ----------
__device__ __forceinline__ int ql_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int ql_find(int* parent, int a) {
  int p = ql_load(parent + a);
  while (p != a) {  // p < a: ends within a steps
    const int g = ql_load(parent + p);
    if (g != p) atomicMin(parent + a, g);  // halving: g is an ancestor of a below p
    a = p;
    p = g;
  }
  return a;
}

__device__ __forceinline__ void ql_union(int* parent, int a, int b) {
  for (;;) {
    a = ql_find(parent, a);
    b = ql_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);  // a was a root when read: hang it under the smaller root b
    if (old == a) return;
    a = old;  // somebody linked a first: a now hangs under min(old, b), and old and b still have to be joined
  }
}

__device__ __forceinline__ void ql_add64(long* p, long v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

__device__ __forceinline__ long ql_shfl_xor(long v, int o) {
  const int lo = __shfl_xor((int)(unsigned)((u64)v & 0xffffffffull), o, 64);
  const int hi = __shfl_xor((int)(unsigned)((u64)v >> 32), o, 64);
  return (long)(((u64)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ long ql_wave_sum(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += ql_shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long ql_wave_min(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, ql_shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ long ql_wave_max(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, ql_shfl_xor(v, o));
  return v;
}

// every lane of the wave is active and holds the same non-negative label
__device__ __forceinline__ bool ql_wave_uniform(int label) {
  const int first = __builtin_amdgcn_readfirstlane(label);
  return first >= 0 && __ballot(label == first) == ~0ull;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(QL_THREADS) void ql_init_kernel(const int* __restrict__ rows, const int* __restrict__ count, int K,
                                                              int* __restrict__ parent, int* __restrict__ line,
                                                              int* __restrict__ order, long* __restrict__ table,
                                                              long* __restrict__ stats) {
  const int i = blockIdx.x * QL_THREADS + threadIdx.x, b = blockIdx.y;
  const int n = ql_clamp(count[b], K);
  if (i == 0) {
    long* st = stats + (long)b * QL_STATS;
    st[0] = n;
    st[1] = 0;
    st[2] = 0;
    st[3] = 0;
  }
  if (i >= K) return;
  const long g = (long)b * K + i;
  parent[g] = (i < n && rows[g * 16 + 14] != 0) ? i : -1;
  line[g] = -1;
  order[g] = -1;
  long* row = table + g * QL_TABLE;
  row[0] = 0;
  row[1] = 0;
  row[2] = 0;
  row[3] = 0;
  row[4] = LONG_MAX;
  row[5] = LONG_MIN;
  row[6] = LONG_MAX;
  row[7] = LONG_MIN;
}

__global__ __launch_bounds__(QL_THREADS) void ql_link_kernel(const int* __restrict__ rows, const int* __restrict__ count, int K,
                                                              int NT, long gap, long cross, long ratio2, int* parent,
                                                              long* stats) {
  __shared__ long s_sy[2 * QL_TILE], s_sx[2 * QL_TILE], s_vy[2 * QL_TILE], s_vx[2 * QL_TILE], s_vv[2 * QL_TILE];
  __shared__ int s_part[2 * QL_TILE];
  const int t = threadIdx.x, b = blockIdx.y;
  const int n = ql_clamp(count[b], K);
  int ti = 0, rem = blockIdx.x;  // the tile's place in the upper triangle, row after row
  while (rem >= NT - ti) {
    rem -= NT - ti;
    ++ti;
  }
  const int tj = ti + rem;
  if (tj * QL_TILE >= n) return;  // uniform over the workgroup; ti <= tj
  if (t < 2 * QL_TILE) {
    const int q = (t < QL_TILE ? ti * QL_TILE : tj * QL_TILE - QL_TILE) + t;
    bool part = false;
    QlFrame f = {0, 0, 0, 0, 0, 0, 0};
    if (q < n) {
      const int4* r = reinterpret_cast<const int4*>(rows) + ((long)b * K + q) * 4;
      part = r[3].z != 0;
      f = ql_frame(r[0], r[1]);
    }
    s_sy[t] = f.sy;
    s_sx[t] = f.sx;
    s_vy[t] = f.vy;
    s_vx[t] = f.vx;
    s_vv[t] = f.vv;
    s_part[t] = part ? 1 : 0;
  }
  __syncthreads();
  const int lane = t & 63, wave = t >> 6;
  const int gj = tj * QL_TILE + lane;
  const long sjy = s_sy[QL_TILE + lane], sjx = s_sx[QL_TILE + lane], vjy = s_vy[QL_TILE + lane], vjx = s_vx[QL_TILE + lane];
  const long vvj = s_vv[QL_TILE + lane];
  const bool pj = s_part[QL_TILE + lane] != 0;
  int* par = parent + (long)b * K;
  int links = 0;
  for (int k = 0; k < QL_TILE / 4; ++k) {
    const int il = wave * (QL_TILE / 4) + k, gi = ti * QL_TILE + il;
    const bool link = pj && s_part[il] != 0 && gi < gj &&
                      ql_linked(s_sy[il], s_sx[il], s_vy[il], s_vx[il], s_vv[il], sjy, sjx, vjy, vjx, vvj, gap, cross, ratio2);
    links += __popcll(__ballot(link));
    if (link) ql_union(par, gi, gj);
  }
  if (lane == 0 && links > 0) ql_add64(stats + (long)b * QL_STATS + 2, links);
}

__global__ __launch_bounds__(QL_THREADS) void ql_flatten_kernel(const int* __restrict__ parent, int K, int* __restrict__ root) {
  const int i = blockIdx.x * QL_THREADS + threadIdx.x, b = blockIdx.y;
  if (i >= K) return;
  const int* par = parent + (long)b * K;
  int a = i, p = par[i];
  if (p >= 0) {
    while (p != a) {  // p < a
      a = p;
      p = par[a];
    }
  }
  root[(long)b * K + i] = p;  // -1 for a row that takes no part
}

// thread t owns the quads [t * per, (t + 1) * per): consecutive threads own ascending runs, so the scan over the threads
// numbers the roots in ascending order of their index
__global__ __launch_bounds__(QL_BLOCK) void ql_number_kernel(const int* __restrict__ root, int K, int* __restrict__ line,
                                                              long* __restrict__ stats) {
  __shared__ int s_num[QL_MAX];
  __shared__ int s_wave[QL_BLOCK / 64], s_wpart[QL_BLOCK / 64];
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
  const int per = (K + QL_BLOCK - 1) / QL_BLOCK;
  const int lo = min(t * per, K), hi = min(lo + per, K);
  const int* rt = root + (long)b * K;
  int roots = 0, part = 0;
  for (int i = lo; i < hi; ++i) {
    const int r = rt[i];
    roots += r == i ? 1 : 0;
    part += r >= 0 ? 1 : 0;
  }
  int incl = roots;  // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  int psum = part;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) psum += __shfl_xor(psum, o, 64);
  if (lane == 63) s_wave[wave] = incl;
  if (lane == 0) s_wpart[wave] = psum;
  __syncthreads();
  int before = 0, total = 0, n_part = 0;
  for (int w = 0; w < QL_BLOCK / 64; ++w) {
    before += w < wave ? s_wave[w] : 0;
    total += s_wave[w];
    n_part += s_wpart[w];
  }
  int num = before + incl - roots;
  for (int i = lo; i < hi; ++i)
    if (rt[i] == i) s_num[i] = num++;
  __syncthreads();
  for (int i = lo; i < hi; ++i) {
    const int r = rt[i];
    line[(long)b * K + i] = (r >= 0 && r < K) ? s_num[r] : -1;
  }
  if (t == 0) {
    stats[(long)b * QL_STATS + 1] = n_part;
    stats[(long)b * QL_STATS + 3] = total;
  }
}

__global__ __launch_bounds__(QL_THREADS) void ql_sum_kernel(const int* __restrict__ rows, const int* __restrict__ line, int K,
                                                             long* table) {
  const int i = blockIdx.x * QL_THREADS + threadIdx.x, b = blockIdx.y;
  const long g = (long)b * K + i;
  const int l = i < K ? line[g] : -1;
  long uy = 0, ux = 0;
  if (l >= 0) {
    const int4* r = reinterpret_cast<const int4*>(rows) + g * 4;
    const QlFrame f = ql_frame(r[0], r[1]);
    uy = f.uy;
    ux = f.ux;
  }
  if (ql_wave_uniform(l)) {  // one line's members side by side: one add for the wave
    uy = ql_wave_sum(uy);
    ux = ql_wave_sum(ux);
    if ((threadIdx.x & 63) == 0) {
      long* row = table + ((long)b * K + l) * QL_TABLE;
      ql_add64(row + 1, 64);
      ql_add64(row + 2, uy);
      ql_add64(row + 3, ux);
    }
  } else if (l >= 0) {
    long* row = table + ((long)b * K + l) * QL_TABLE;
    ql_add64(row + 1, 1);
    ql_add64(row + 2, uy);
    ql_add64(row + 3, ux);
  }
}

__global__ __launch_bounds__(QL_BLOCK) void ql_start_kernel(int K, long* __restrict__ table, const long* __restrict__ stats) {
  __shared__ int s_wave[QL_BLOCK / 64];
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
  const int L = ql_clamp((int)stats[(long)b * QL_STATS + 3], K);
  const int per = (K + QL_BLOCK - 1) / QL_BLOCK;
  const int lo = min(t * per, K), hi = min(lo + per, K);
  long* tab = table + (long)b * K * QL_TABLE;
  int sizes[QL_PER];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < QL_PER; ++k) {
    const int l = lo + k;
    sizes[k] = (l < hi && l < L) ? (int)tab[(long)l * QL_TABLE + 1] : 0;
    mine += sizes[k];
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int start = incl - mine;
  for (int w = 0; w < wave; ++w) start += s_wave[w];
#pragma unroll
  for (int k = 0; k < QL_PER; ++k) {
    const int l = lo + k;
    if (l >= hi) continue;
    long* row = tab + (long)l * QL_TABLE;
    if (l < L) {
      row[0] = start;
      start += sizes[k];
      if (row[2] == 0 && row[3] == 0) row[3] = 16;
    } else {
#pragma unroll
      for (int w = 0; w < QL_TABLE; ++w) row[w] = 0;
    }
  }
}

__global__ __launch_bounds__(QL_THREADS) void ql_extent_kernel(const int* __restrict__ rows, const int* __restrict__ line,
                                                                int K, long* table, long* __restrict__ key) {
  const int i = blockIdx.x * QL_THREADS + threadIdx.x, b = blockIdx.y;
  const long g = (long)b * K + i;
  const int l = i < K ? line[g] : -1;
  long a0 = LONG_MAX, a1 = LONG_MIN, b0 = LONG_MAX, b1 = LONG_MIN;
  long* row = table + ((long)b * K + max(l, 0)) * QL_TABLE;
  if (l >= 0) {
    const long Uy = row[2], Ux = row[3];
    const int4* r = reinterpret_cast<const int4*>(rows) + g * 4;
    const int4 c01 = r[0], c23 = r[1];
    const QlFrame f = ql_frame(c01, c23);
    key[g] = f.sy * Uy + f.sx * Ux;
    const long py[4] = {c01.x, c01.z, c23.x, c23.z}, px[4] = {c01.y, c01.w, c23.y, c23.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long a = py[k] * Uy + px[k] * Ux, bb = py[k] * Ux - px[k] * Uy;
      a0 = min(a0, a);
      a1 = max(a1, a);
      b0 = min(b0, bb);
      b1 = max(b1, bb);
    }
  }
  const bool uniform = ql_wave_uniform(l);
  if (uniform) {
    a0 = ql_wave_min(a0);
    a1 = ql_wave_max(a1);
    b0 = ql_wave_min(b0);
    b1 = ql_wave_max(b1);
  }
  if (l >= 0 && (!uniform || (threadIdx.x & 63) == 0)) {
    atomicMin(reinterpret_cast<long long*>(row + 4), (long long)a0);
    atomicMax(reinterpret_cast<long long*>(row + 5), (long long)a1);
    atomicMin(reinterpret_cast<long long*>(row + 6), (long long)b0);
    atomicMax(reinterpret_cast<long long*>(row + 7), (long long)b1);
  }
}

__global__ __launch_bounds__(QL_THREADS) void ql_rank_kernel(const int* __restrict__ count, const int* __restrict__ line,
                                                              const long* __restrict__ key, const long* __restrict__ table,
                                                              int K, int* __restrict__ order) {
  __shared__ long s_key[QL_CHUNK];
  __shared__ int s_line[QL_CHUNK];
  __shared__ int s_pos[QL_THREADS];
  const int t = threadIdx.x, b = blockIdx.y, lane = t & 63, wave = t >> 6;
  const int n = ql_clamp(count[b], K);
  if (blockIdx.x * QL_TILE >= n) return;  // uniform over the workgroup
  const int i = blockIdx.x * QL_TILE + lane;
  const int* ln = line + (long)b * K;
  const long* ky = key + (long)b * K;
  const int li = i < n ? ln[i] : -1;
  const long ki = li >= 0 ? ky[i] : 0;
  int pos = 0;
  for (int c0 = 0; c0 < n; c0 += QL_CHUNK) {
    __syncthreads();
    for (int k = t; k < QL_CHUNK; k += QL_THREADS) {
      const int j = c0 + k;
      const int lj = j < n ? ln[j] : -1;
      s_line[k] = lj;
      s_key[k] = lj >= 0 ? ky[j] : 0;  // a key is written for members only
    }
    __syncthreads();
    const int q0 = wave * (QL_CHUNK / 4);
    const int q1 = min(q0 + QL_CHUNK / 4, n - c0);  // uniform over the wave
    for (int k = q0; k < q1; ++k) {
      const long kj = s_key[k];
      const int j = c0 + k;
      pos += (s_line[k] == li && (kj < ki || (kj == ki && j < i))) ? 1 : 0;
    }
  }
  s_pos[t] = pos;
  __syncthreads();
  if (wave == 0 && li >= 0) {
    const int at = s_pos[lane] + s_pos[64 + lane] + s_pos[128 + lane] + s_pos[192 + lane];
    const long start = table[((long)b * K + li) * QL_TABLE];
    const long slot = start + at;
    if (slot >= 0 && slot < K) order[(long)b * K + slot] = i;
  }
}

size_t ql_align(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: key (B, K) int64, parent (B, K) int32, root (B, K) int32
struct QlLayout {
  size_t key, parent, root, bytes;
};

QlLayout ql_layout(int B, int K) {
  QlLayout l;
  const size_t quads = (size_t)B * K;
  l.key = 0;
  l.parent = ql_align(l.key + quads * sizeof(long));
  l.root = ql_align(l.parent + quads * sizeof(int));
  l.bytes = ql_align(l.root + quads * sizeof(int));
  return l;
}

int ql_check_dims(const char* what, int B, int K) {
  VKAS_CHECK(B >= 0 && B <= 65535, "%s: bad B=%d (0..65535)", what, B);
  VKAS_CHECK(K >= 1 && K <= QL_MAX, "%s: K=%d must lie in 1..%d", what, K, QL_MAX);
  return VKAS_OK;
}

}  // namespace

extern "C" long long vkas_quad_lines_workspace_bytes(int B, int K) {
  if (ql_check_dims("vkas_quad_lines_workspace_bytes", B, K) != VKAS_OK) return -1;
  return (long long)ql_layout(B, K).bytes;
}

extern "C" int vkas_quad_lines(const int* rows, const int* count, int B, int K, int gap_q4, int cross_q4, int ratio_q4,
                               void* workspace, size_t workspace_bytes, int* line, int* order, long long* table,
                               long long* stats, void* stream) {
  const int rc = ql_check_dims("vkas_quad_lines", B, K);
  if (rc != VKAS_OK) return rc;
  VKAS_CHECK(gap_q4 >= 1 && gap_q4 <= 4096, "vkas_quad_lines: gap_q4 = %d must lie in 1..4096", gap_q4);
  VKAS_CHECK(cross_q4 >= 1 && cross_q4 <= 4096, "vkas_quad_lines: cross_q4 = %d must lie in 1..4096", cross_q4);
  VKAS_CHECK(ratio_q4 >= 16 && ratio_q4 <= 256, "vkas_quad_lines: ratio_q4 = %d must lie in 16..256", ratio_q4);
  if (B == 0) return VKAS_OK;
  VKAS_CHECK(rows && count && workspace && line && order && table && stats, "vkas_quad_lines: null pointer");
  VKAS_CHECK(vkas_aligned16(rows) && vkas_aligned16(workspace),
             "vkas_quad_lines: the row table and the workspace must be 16-byte aligned");
  VKAS_CHECK((((uintptr_t)line) & 3u) == 0 && (((uintptr_t)order) & 3u) == 0 && (((uintptr_t)count) & 3u) == 0 &&
                 (((uintptr_t)table) & 7u) == 0 && (((uintptr_t)stats) & 7u) == 0,
             "vkas_quad_lines: count, line and order must be 4-byte aligned, table and stats 8-byte aligned");
  const QlLayout l = ql_layout(B, K);
  VKAS_CHECK(workspace_bytes >= l.bytes, "vkas_quad_lines: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
  char* ws = static_cast<char*>(workspace);
  long* key = reinterpret_cast<long*>(ws + l.key);
  int* parent = reinterpret_cast<int*>(ws + l.parent);
  int* root = reinterpret_cast<int*>(ws + l.root);
  long* tab = reinterpret_cast<long*>(table);
  long* st = reinterpret_cast<long*>(stats);
  hipStream_t s = vkas_stream(stream);
  const int NT = (int)vkas_cdiv(K, QL_TILE);
  const dim3 per_quad((unsigned)vkas_cdiv(K, QL_THREADS), (unsigned)B);
  ql_init_kernel<<<per_quad, QL_THREADS, 0, s>>>(rows, count, K, parent, line, order, tab, st);
  VKAS_LAUNCH_CHECK("quad_lines init");
  ql_link_kernel<<<dim3((unsigned)(NT * (NT + 1) / 2), (unsigned)B), QL_THREADS, 0, s>>>(
      rows, count, K, NT, (long)gap_q4, (long)cross_q4, (long)ratio_q4 * ratio_q4, parent, st);
  VKAS_LAUNCH_CHECK("quad_lines links");
  ql_flatten_kernel<<<per_quad, QL_THREADS, 0, s>>>(parent, K, root);
  VKAS_LAUNCH_CHECK("quad_lines flatten");
  ql_number_kernel<<<B, QL_BLOCK, 0, s>>>(root, K, line, st);
  VKAS_LAUNCH_CHECK("quad_lines numbers");
  ql_sum_kernel<<<per_quad, QL_THREADS, 0, s>>>(rows, line, K, tab);
  VKAS_LAUNCH_CHECK("quad_lines sums");
  ql_start_kernel<<<B, QL_BLOCK, 0, s>>>(K, tab, st);
  VKAS_LAUNCH_CHECK("quad_lines starts");
  ql_extent_kernel<<<per_quad, QL_THREADS, 0, s>>>(rows, line, K, tab, key);
  VKAS_LAUNCH_CHECK("quad_lines extents");
  ql_rank_kernel<<<dim3((unsigned)NT, (unsigned)B), QL_THREADS, 0, s>>>(count, line, key, tab, K, order);
  VKAS_LAUNCH_CHECK("quad_lines ranks");
  return VKAS_OK;
}
