// Brute-force descriptor matching on the int8 matrix cores.
//
// For every query row the two smallest (d2, train index) pairs over the
// unmasked train rows, d2 = sum_k (Q[q][k] - T[t][k])^2 over 128 bytes, in
// lexicographic order.  Integer arithmetic only: the result is exact and does
// not depend on the grid or on the train split.
//
// k_match_prep: x' = x - 128 as int8 (byte ^ 0x80) of every row into a packed
//   copy padded with zero rows to whole tiles, masked rows zeroed too -- train
//   rows as t', query rows as -q' - 1 (~q', still int8), so that the matrix
//   cores return -q'.t' - sum t' and the key below is one shift-add; and per
//   row |q'|^2 (queries: -1 = masked) or, for train rows, the key base
//   ((|t'|^2 + 2 sum t') << 8) + (row & 255) (INT32_MAX = masked or padding).
//   The main loop then loads 16 bytes per lane with no bound or mask test.
// k_match: d2 = |q'|^2 + |t'|^2 - 2 q'.t' with the dot products on
//   v_mfma_i32_32x32x32_i8, train rows as the A operand (accumulator register
//   index), queries as B (accumulator column = lane & 31).  Both fragments are
//   loaded by one rule -- k-step s of lane (r, h) is bytes [32 s + 16 h, + 16)
//   of row r -- so the instruction's own k-order cancels in the dot product.
//   A wave keeps kMatchNQ query fragments (128 queries) in registers and
//   reuses each train fragment for all of them.  Per element one signed key
//   base + (acc << 9) = (|t'|^2 - 2 dot) << 8 | row-in-chunk (the query norm is
//   the same for the whole lane, so it is added at the fold) and second = min(second,
//   max(best, key)), best = min(best, key); every 256-row chunk folds the two
//   keys into the lane's running (d2, index) pairs.  The two lane halves that
//   share a column merge through one xor-32 shuffle at the end.
// k_match_merge: lexicographic min over the train splits' partial records.
// k_match_flag / k_match_emit: the selection (ratio, mutual check) as a flag
//   array, its exclusive scan and an ordered emission -- no sort, no atomics.
#include "sift_kernels.h"

#include <climits>

#pragma clang fp contract(off)

namespace sift {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kNone = INT_MAX;

// Running top-2 of one query in (d2, index) order; a missing entry is (kNone, -1).
struct Top2 {
  int d1, i1, d2, i2;
};

__device__ __forceinline__ bool lex_less(int da, int ia, int db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ void top2_insert(Top2& t, int d, int i) {
  if (i < 0) return;
  if (t.i1 < 0 || lex_less(d, i, t.d1, t.i1)) {
    t.d2 = t.d1;
    t.i2 = t.i1;
    t.d1 = d;
    t.i1 = i;
  } else if (t.i2 < 0 || lex_less(d, i, t.d2, t.i2)) {
    t.d2 = d;
    t.i2 = i;
  }
}

// One thread per 16 bytes, eight per row; rows [0, n_pad).
__global__ void __launch_bounds__(256) k_match_prep(const uint4* __restrict__ src, const unsigned char* __restrict__ mask,
                                                    int n, long long n_pad, int train, uint4* __restrict__ dst,
                                                    int* __restrict__ norm) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long row = t >> 3;
  if (row >= n_pad) return;  // n_pad rows are a whole number of waves' worth (multiple of 32 rows)
  const int seg = (int)(t & 7);
  const bool live = row < n && (!mask || mask[row] != 0);
  uint4 v = make_uint4(0, 0, 0, 0);
  if (live) v = src[row * 8 + seg];
  v.x ^= 0x80808080u;
  v.y ^= 0x80808080u;
  v.z ^= 0x80808080u;
  v.w ^= 0x80808080u;
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  int s = 0, s1 = 0;  // sum of squares, sum
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int x = (int)(signed char)(w[j] >> (8 * b));
      s += x * x;
      s1 += x;
    }
#pragma unroll
  for (int m = 1; m < 8; m <<= 1) {
    s += __shfl_xor(s, m);
    s1 += __shfl_xor(s1, m);
  }
  if (!train) v = make_uint4(~v.x, ~v.y, ~v.z, ~v.w);  // queries as -q' - 1
  dst[row * 8 + seg] = live ? v : make_uint4(0, 0, 0, 0);
  if (seg == 0)
    norm[row] = !live ? (train ? kNone : -1) : (train ? (s + 2 * s1) * 256 + (int)(row & (kMatchChunk - 1)) : s);
}

// grid (query blocks, train splits); wave w of block bx owns queries bx kMatchQB + 128 w ..
__global__ void __launch_bounds__(64 * kMatchWaves)
    k_match(const v4i* __restrict__ qs, const int* __restrict__ qn, const v4i* __restrict__ ts,
            const int* __restrict__ kb, int n_query, int n_chunks, int chunks_per_split, Match* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, h = lane >> 5;
  const long long q0 = (long long)blockIdx.x * kMatchQB + wave * (32 * kMatchNQ);
  if (q0 >= n_query) return;  // no barrier below: a wave without queries leaves

  v4i b[kMatchNQ][4];
  int nq[kMatchNQ];
  Top2 g[kMatchNQ];
#pragma unroll
  for (int f = 0; f < kMatchNQ; ++f) {
    const long long q = q0 + 32 * f + col;  // < padded query rows
    const v4i* p = qs + q * 8 + h;
#pragma unroll
    for (int s = 0; s < 4; ++s) b[f][s] = p[2 * s];
    nq[f] = qn[q];
    g[f] = Top2{kNone, -1, kNone, -1};
  }

  const int c0 = blockIdx.y * chunks_per_split;
  const int c1 = min(n_chunks, c0 + chunks_per_split);
  for (int c = c0; c < c1; ++c) {
    int k1[kMatchNQ], k2[kMatchNQ];
#pragma unroll
    for (int f = 0; f < kMatchNQ; ++f) k1[f] = k2[f] = kNone;
#pragma unroll 2
    for (int t = 0; t < kMatchChunk / 32; ++t) {
      const long long base = (long long)c * kMatchChunk + 32 * t;  // < padded train rows
      const v4i* pa = ts + (base + col) * 8 + h;
      v4i a[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = pa[2 * s];
      // accumulator register r holds train row base + (r & 3) + 8 (r >> 2) + 4 h
      v4i kv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) kv[j] = *reinterpret_cast<const v4i*>(kb + base + 8 * j + 4 * h);
#pragma unroll
      for (int f = 0; f < kMatchNQ; ++f) {
        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b[f][s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // acc = -dot - sum t', |acc| <= 2^21, and the base's low byte is the row: no carry into it, no overflow
          const int key = kv[r >> 2][r & 3] + acc[r] * 512;
          k2[f] = min(k2[f], max(k1[f], key));
          k1[f] = min(k1[f], key);
        }
      }
    }
#pragma unroll
    for (int f = 0; f < kMatchNQ; ++f) {
      // a masked or padding row has a zero fragment and base kNone: its key is kNone itself
      if (k1[f] != kNone) top2_insert(g[f], (k1[f] >> 8) + nq[f], c * kMatchChunk + (k1[f] & (kMatchChunk - 1)));
      if (k2[f] != kNone) top2_insert(g[f], (k2[f] >> 8) + nq[f], c * kMatchChunk + (k2[f] & (kMatchChunk - 1)));
    }
  }

#pragma unroll
  for (int f = 0; f < kMatchNQ; ++f) {
    const int od1 = __shfl_xor(g[f].d1, 32), oi1 = __shfl_xor(g[f].i1, 32);
    const int od2 = __shfl_xor(g[f].d2, 32), oi2 = __shfl_xor(g[f].i2, 32);
    top2_insert(g[f], od1, oi1);
    top2_insert(g[f], od2, oi2);
    const long long q = q0 + 32 * f + col;
    if (h == 0 && q < n_query) {
      Match m{g[f].i1, g[f].i2, g[f].d1, g[f].d2};
      if (nq[f] < 0) m = Match{-1, -1, kNone, kNone};
      part[(long long)blockIdx.y * n_query + q] = m;
    }
  }
}

// out[q] = the two smallest of the splits' records of q (splits == 0: none).
__global__ void __launch_bounds__(256) k_match_merge(const Match* __restrict__ part, int splits, int n_query,
                                                     Match* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // the grid may pass 2^31 threads
  if (q >= n_query) return;
  Top2 t{kNone, -1, kNone, -1};
  for (int s = 0; s < splits; ++s) {
    const Match m = part[(long long)s * n_query + q];
    top2_insert(t, m.d2_best, m.best);
    top2_insert(t, m.d2_second, m.second);
  }
  out[q] = Match{t.i1, t.i2, t.d1, t.d2};
}

__global__ void __launch_bounds__(256) k_match_flag(const Match* __restrict__ fwd, int n_query,
                                                    const Match* __restrict__ rev, int n_train, double r2,
                                                    unsigned* __restrict__ flag) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // the grid may pass 2^31 threads
  if (q > n_query) return;
  unsigned ok = 0;
  if (q < n_query) {  // flag[n_query] = 0: the scan's output there is the pair count
    const Match m = fwd[q];
    ok = m.best >= 0;
    if (ok && r2 > 0.0 && m.second >= 0) ok = (double)m.d2_best < r2 * (double)m.d2_second;
    if (ok && rev) ok = m.best < n_train && rev[m.best].best == q;  // rev holds n_train records
  }
  flag[q] = ok;
}

__global__ void __launch_bounds__(256) k_match_emit(const Match* __restrict__ fwd, const unsigned* __restrict__ flag,
                                                    const unsigned* __restrict__ off, int n_query, unsigned cap,
                                                    MatchPair* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // the grid may pass 2^31 threads
  if (q >= n_query || !flag[q]) return;
  const unsigned at = off[q];
  if (at >= cap) return;
  const Match m = fwd[q];
  out[at] = MatchPair{(int)q, m.best, m.d2_best, m.d2_second};
}

}  // namespace

hipError_t launch_match_prep(const unsigned char* src, const unsigned char* mask, int n, long long n_pad, int train,
                             unsigned char* dst, int* norm, hipStream_t st) {
  if (n_pad <= 0) return hipSuccess;
  const long long threads = n_pad * 8;
  hipLaunchKernelGGL(k_match_prep, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(src), mask, n, n_pad, train, reinterpret_cast<uint4*>(dst), norm);
  return hipGetLastError();
}

hipError_t launch_match(const unsigned char* qs, const int* qn, int n_query, const unsigned char* ts, const int* kb,
                        int n_train, Match* part, hipStream_t st) {
  if (n_query <= 0 || n_train <= 0) return hipSuccess;
  const MatchSplit s = match_split(n_query, n_train);
  hipLaunchKernelGGL(k_match, dim3(s.query_blocks, s.splits), dim3(64 * kMatchWaves), 0, st,
                     reinterpret_cast<const v4i*>(qs), qn, reinterpret_cast<const v4i*>(ts), kb, n_query, s.chunks,
                     s.chunks_per_split, part);
  return hipGetLastError();
}

hipError_t launch_match_merge(const Match* part, int splits, int n_query, Match* out, hipStream_t st) {
  if (n_query <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_match_merge, dim3(n_query / 256 + 1), dim3(256), 0, st, part, splits, n_query, out);
  return hipGetLastError();
}

hipError_t launch_match_flag(const Match* fwd, int n_query, const Match* rev, int n_train, double r2, unsigned* flag,
                             hipStream_t st) {
  hipLaunchKernelGGL(k_match_flag, dim3(n_query / 256 + 1), dim3(256), 0, st, fwd, n_query, rev, n_train, r2, flag);
  return hipGetLastError();
}

hipError_t launch_match_emit(const Match* fwd, const unsigned* flag, const unsigned* off, int n_query, unsigned cap,
                             MatchPair* out, hipStream_t st) {
  if (n_query <= 0 || cap == 0) return hipSuccess;
  hipLaunchKernelGGL(k_match_emit, dim3(n_query / 256 + 1), dim3(256), 0, st, fwd, flag, off, n_query, cap, out);
  return hipGetLastError();
}

}  // namespace sift
