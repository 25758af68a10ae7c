// Guided descriptor matching on gfx950: the two nearest train rows among those within a radius of H x.
// The definition is in include/sift_hip.h (sift_match_guided); DESIGN.md section 18 has the proof that the grid
// below never hides a candidate.  The records are a lexicographic minimum of integer keys over a set that the
// definition fixes, so neither the grid, the order inside a cell nor the launch shape can change them.
//
// k_guided_gather  (features form) the position of every record: abs_x, abs_y of the keypoint its orientation names.
// k_guided_cells   one thread per train row: its cell, or -1 for a masked row or a NaN coordinate, and one integer
//                  add to the cell's count.  hipcub's exclusive scan of the counts follows (sift_api_guided.hip).
// k_guided_fill    eight lanes per train row file it in cell order: a slot of its cell's range, taken by counting the
//                  cell's count back down (an atomic cursor), then the position, the index, the squared norm and the
//                  128 bytes go to that slot.  Which slot of the range a row gets depends on arrival; the match
//                  takes a minimum of (d2, index) keys over the range, which no order inside it can change.
// k_guided_match   one wave per query row (one-wave blocks striding over the rows).  The projection, the cell
//                  range and the 128 query bytes are wave-uniform.  The cells of one grid row are one contiguous run
//                  of the filed arrays: 64 lanes test 64 positions, the survivors' slots are queued in LDS behind the
//                  ballot's prefix, and whenever 64 are queued each lane takes one: eight 16-byte loads, 32
//                  v_dot4_u32_u8, d2 = |q|^2 + |t|^2 - 2 q.t, and the key (d2 << 32) | index into the lane's top-2.
//                  The position test precedes every descriptor load.  One wave reduction per query; the three info
//                  sums stay in wave-uniform registers until the wave's last row, then three integer adds.
//
// Every atomic is an integer add: no result depends on arrival order.
#include "sift_kernels.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace sift {

namespace {

constexpr int kGuidedThreads = 256;
constexpr unsigned long long kNoKey = ~0ull;

// The budget's clamped rule (sift_budget.hip, cell_axis): the test comes before the cast.
__device__ __forceinline__ int guided_axis(double a, int cell_px, int nc) {
  const double t = a / (double)cell_px;
  return t >= 0.0 ? (t < (double)nc ? (int)__builtin_floor(t) : nc - 1) : 0;
}

__global__ void __launch_bounds__(kGuidedThreads) k_guided_gather(const Orientation* __restrict__ ori, int n,
                                                                  const Keypoint* __restrict__ kp, int n_kp,
                                                                  double2* __restrict__ xy) {
  const long long i = (long long)blockIdx.x * kGuidedThreads + threadIdx.x;
  if (i >= n) return;
  const double nan = __builtin_nan("");
  double2 p = make_double2(nan, nan);
  const int k = ori[i].keypoint;
  if (k >= 0 && k < n_kp) p = make_double2(kp[k].abs_x, kp[k].abs_y);
  xy[i] = p;
}

__global__ void __launch_bounds__(kGuidedThreads) k_guided_cells(const double2* __restrict__ xy,
                                                                 const unsigned char* __restrict__ mask, int n,
                                                                 GuidedGrid g, int* __restrict__ cell,
                                                                 unsigned* __restrict__ count) {
  const long long i = (long long)blockIdx.x * kGuidedThreads + threadIdx.x;
  if (i >= n) return;
  const double2 p = xy[i];
  int c = -1;
  if ((!mask || mask[i]) && p.x == p.x && p.y == p.y)
    c = guided_axis(p.y, g.cell_px, g.ncy) * g.ncx + guided_axis(p.x, g.cell_px, g.ncx);
  cell[i] = c;
  if (c >= 0) atomicAdd(&count[c], 1u);
}

// Lanes 8 j .. 8 j + 7 of a wave file train row (wave's first row) + j; lane 8 j takes the slot.
__global__ void __launch_bounds__(kGuidedThreads) k_guided_fill(const unsigned char* __restrict__ rows,
                                                                const double2* __restrict__ xy,
                                                                const int* __restrict__ cell, int n,
                                                                const unsigned* __restrict__ off,
                                                                unsigned* __restrict__ count, GuidedFiled F) {
  const long long t = (long long)blockIdx.x * kGuidedThreads + threadIdx.x;
  const long long i = t >> 3;
  const int part = (int)(t & 7), lane = threadIdx.x & 63;
  const int c = i < n ? cell[i] : -1;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (c >= 0) v = *reinterpret_cast<const uint4*>(rows + (size_t)i * kDescBytes + part * 16);
  unsigned norm = __builtin_amdgcn_udot4(v.x, v.x, 0u, false);
  norm = __builtin_amdgcn_udot4(v.y, v.y, norm, false);
  norm = __builtin_amdgcn_udot4(v.z, v.z, norm, false);
  norm = __builtin_amdgcn_udot4(v.w, v.w, norm, false);
  norm += __shfl_xor(norm, 1, 64);
  norm += __shfl_xor(norm, 2, 64);
  norm += __shfl_xor(norm, 4, 64);
  unsigned slot = 0;
  if (c >= 0 && part == 0) slot = off[c] + atomicSub(&count[c], 1u) - 1u;  // count[c] >= 1 here: this row was counted
  slot = __shfl(slot, lane & ~7, 64);
  if (c < 0) return;
  *reinterpret_cast<uint4*>(F.rows + (size_t)slot * kDescBytes + part * 16) = v;
  if (part == 0) {
    F.xy[slot] = xy[i];
    F.tag[slot] = make_int2((int)i, (int)norm);
  }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)k, d, 64), hi = __shfl_xor((unsigned)(k >> 32), d, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    k = o < k ? o : k;
  }
  return k;
}

__device__ __forceinline__ void top2_insert(unsigned long long key, unsigned long long& k1, unsigned long long& k2) {
  const unsigned long long lo = key < k1 ? key : k1, hi = key < k1 ? k1 : key;
  k1 = lo;
  k2 = hi < k2 ? hi : k2;
}

// The lane's candidate (filed slot `slot`, or none when slot < 0) against the wave-uniform query row.
__device__ __forceinline__ void guided_score(int slot, const uint4 (&q)[8], unsigned qn, const GuidedFiled& F,
                                             unsigned long long& k1, unsigned long long& k2) {
  if (slot < 0) return;
  const uint4* row = reinterpret_cast<const uint4*>(F.rows + (size_t)slot * kDescBytes);
  const int2 tag = F.tag[slot];
  unsigned dot = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint4 v = row[j];
    dot = __builtin_amdgcn_udot4(q[j].x, v.x, dot, false);
    dot = __builtin_amdgcn_udot4(q[j].y, v.y, dot, false);
    dot = __builtin_amdgcn_udot4(q[j].z, v.z, dot, false);
    dot = __builtin_amdgcn_udot4(q[j].w, v.w, dot, false);
  }
  const unsigned d2 = qn + (unsigned)tag.y - 2u * dot;  // each term is at most 128 * 255^2
  top2_insert(((unsigned long long)d2 << 32) | (unsigned)tag.x, k1, k2);
}

// One wave per block: __syncthreads() orders the wave's LDS queue and costs no barrier wait.
__global__ void __launch_bounds__(64) k_guided_match(GuidedMatch M) {
  __shared__ int s_queue[128];
  const int lane = threadIdx.x;
  unsigned long long n_proj = 0, n_vis = 0, n_cand = 0;  // wave-uniform
  for (long long qi = blockIdx.x; qi < M.n_query; qi += gridDim.x) {
    unsigned long long k1 = kNoKey, k2 = kNoKey;
    const double2 p = M.qxy[qi];
    const double u = (M.h[0] * p.x + M.h[1] * p.y) + M.h[2];
    const double v = (M.h[3] * p.x + M.h[4] * p.y) + M.h[5];
    const double w = (M.h[6] * p.x + M.h[7] * p.y) + M.h[8];
    const double rinv = 1.0 / w;
    const double px = u * rinv, py = v * rinv;
    const bool projected = (!M.qmask || M.qmask[qi]) && w > 0.0 && px - px == 0.0 && py - py == 0.0;
    if (projected) {
      ++n_proj;
      const uint4* qrow = reinterpret_cast<const uint4*>(M.query + (size_t)qi * kDescBytes);
      uint4 q[8];
      unsigned qn = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q[j] = qrow[j];
        qn = __builtin_amdgcn_udot4(q[j].x, q[j].x, qn, false);
        qn = __builtin_amdgcn_udot4(q[j].y, q[j].y, qn, false);
        qn = __builtin_amdgcn_udot4(q[j].z, q[j].z, qn, false);
        qn = __builtin_amdgcn_udot4(q[j].w, q[j].w, qn, false);
      }
      const GuidedGrid g = M.grid;
      const int x0 = max(guided_axis(px - M.radius, g.cell_px, g.ncx) - 1, 0);
      const int x1 = min(guided_axis(px + M.radius, g.cell_px, g.ncx) + 1, g.ncx - 1);
      const int y0 = max(guided_axis(py - M.radius, g.cell_px, g.ncy) - 1, 0);
      const int y1 = min(guided_axis(py + M.radius, g.cell_px, g.ncy) + 1, g.ncy - 1);
      int queued = 0;  // wave-uniform, below 64 between rounds
      for (int iy = y0; iy <= y1; ++iy) {
        const size_t c0 = (size_t)iy * g.ncx;
        const unsigned s = __builtin_amdgcn_readfirstlane(M.off[c0 + x0]);
        const unsigned e = __builtin_amdgcn_readfirstlane(M.off[c0 + x1 + 1]);  // off has cells + 1 entries
        n_vis += e - s;
        for (unsigned base = s; base < e; base += 64) {
          const unsigned i = base + lane;
          bool pass = false;
          if (i < e) {
            const double2 t = M.filed.xy[i];
            const double dx = t.x - px, dy = t.y - py;
            pass = (dx * dx + dy * dy) <= M.r2;
          }
          const unsigned long long hit = __ballot(pass);
          if (hit == 0) continue;
          if (pass) s_queue[queued + __popcll(hit & ((1ull << lane) - 1ull))] = (int)i;
          const int got = __popcll(hit);
          n_cand += got;
          queued += got;
          if (queued >= 64) {
            __syncthreads();
            const int mine = s_queue[lane];
            const int tail = lane < queued - 64 ? s_queue[64 + lane] : 0;
            __syncthreads();
            if (lane < queued - 64) s_queue[lane] = tail;
            queued -= 64;
            guided_score(mine, q, qn, M.filed, k1, k2);
          }
        }
      }
      if (queued > 0) {
        __syncthreads();
        const int mine = lane < queued ? s_queue[lane] : -1;
        __syncthreads();  // the next row's queue writes come after this read
        guided_score(mine, q, qn, M.filed, k1, k2);
      }
    }
    // keys are distinct (distinct train indices), so exactly one lane holds the best
    const unsigned long long best = wave_min_u64(k1);
    const unsigned long long second = wave_min_u64(k1 == best ? k2 : k1);
    if (lane == 0) {
      Match m;
      m.best = best == kNoKey ? -1 : (int)(unsigned)best;
      m.d2_best = best == kNoKey ? INT32_MAX : (int)(best >> 32);
      m.second = second == kNoKey ? -1 : (int)(unsigned)second;
      m.d2_second = second == kNoKey ? INT32_MAX : (int)(second >> 32);
      M.out[qi] = m;
    }
  }
  if (lane == 0 && M.info) {
    if (n_proj) atomicAdd(&M.info[0], n_proj);
    if (n_vis) atomicAdd(&M.info[1], n_vis);
    if (n_cand) atomicAdd(&M.info[2], n_cand);
  }
}

inline unsigned guided_blocks(long long items) { return (unsigned)((items + kGuidedThreads - 1) / kGuidedThreads); }

}  // namespace

GuidedGrid guided_grid(int width, int height, double radius) {
  const long long W = width, H = height, big = std::max(W, H);
  const double cr = std::ceil(radius);  // radius is finite and > 0
  long long lo = cr < (double)big ? std::max(1LL, (long long)cr) : big;
  auto cells = [&](long long c) { return ((W + c - 1) / c) * ((H + c - 1) / c); };
  long long hi = big;  // one cell
  while (lo < hi) {    // the cell count does not grow with c
    const long long mid = lo + (hi - lo) / 2;
    if (cells(mid) <= kGuidedMaxCells)
      hi = mid;
    else
      lo = mid + 1;
  }
  return GuidedGrid{(int)lo, (int)((W + lo - 1) / lo), (int)((H + lo - 1) / lo)};
}

hipError_t launch_guided_gather(const Orientation* ori, int n, const Keypoint* kp, int n_kp, double2* xy,
                                hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_guided_gather, dim3(guided_blocks(n)), dim3(kGuidedThreads), 0, st, ori, n, kp, n_kp, xy);
  return hipGetLastError();
}

hipError_t launch_guided_cells(const double2* xy, const unsigned char* mask, int n, const GuidedGrid& g, int* cell,
                               unsigned* count, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_guided_cells, dim3(guided_blocks(n)), dim3(kGuidedThreads), 0, st, xy, mask, n, g, cell, count);
  return hipGetLastError();
}

hipError_t launch_guided_fill(const unsigned char* rows, const double2* xy, const int* cell, int n, const unsigned* off,
                              unsigned* count, const GuidedFiled& F, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_guided_fill, dim3(guided_blocks(8LL * n)), dim3(kGuidedThreads), 0, st, rows, xy, cell, n, off,
                     count, F);
  return hipGetLastError();
}

hipError_t launch_guided_match(const GuidedMatch& M, hipStream_t st) {
  if (M.n_query <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<long long>(M.n_query, kGuidedMatchBlocks);
  hipLaunchKernelGGL(k_guided_match, dim3(blocks), dim3(64), 0, st, M);
  return hipGetLastError();
}

}  // namespace sift
