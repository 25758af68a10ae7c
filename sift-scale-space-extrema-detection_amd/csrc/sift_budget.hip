// Keypoint budget on gfx950: the N strongest keypoints, overall or per grid cell, chosen without a sort.
// The definition is in include/sift_hip.h (sift_budget); everything below decides on integers.
//
// "Record i precedes j" is a total order: the 64-bit strength key descending, then the index ascending.  Both go
// into one composite of 8 + nb bytes, most significant first: the key's eight bytes, then the low nb bytes of
// n - 1 - i (nb = the bytes n - 1 needs, so an earlier record has the larger tail).  Composites are distinct, so
// "fewer than q records of my cell precede me" is "my composite is at least the q-th largest of my cell": a
// most-significant-digit radix SELECT per cell, one byte per pass, and no tie is left for a scan to break.
//
// k_budget_keys   key and cell of every record.
// k_budget_hist   pass p: every active record whose composite still agrees with its cell's threshold prefix adds 1
//                 to bin (cell, byte p).  Few cells: the bins live in LDS and a block adds one value per non-empty
//                 bin (a single cell would otherwise put all n adds on 256 addresses).  Many cells: global adds.
// k_budget_walk   pass p, one wave per cell: walks the 256 bins from the top, fixes byte p of the threshold, takes
//                 the records strictly above it off the cell's remaining quota, and zeroes the bins for pass p + 1.
//                 Pass 0 also clamps the quota to the cell's population; a quota of 0 closes the cell.
// k_budget_flag   flag[i] = active and composite >= the cell's threshold; flag[n] = 0 for the scan that follows.
// k_budget_emit   the ascending index list from the flags' exclusive scan, and the gathered records when asked.
//
// Every atomic is an integer add, so neither arrival order nor the grid changes a result.
#include "sift_kernels.h"

namespace sift {

namespace {

constexpr unsigned long long kAbsMask = 0x7FFFFFFFFFFFFFFFull;
constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;

// Threads past n idle: the grid is whole tiles of kBudgetTile records, thread t of a block takes records t, t + 256, ...
__device__ __forceinline__ long long tile_base() { return (long long)blockIdx.x * kBudgetTile + threadIdx.x; }

// Column (or row) of a coordinate: the test comes before the cast; a NaN or a negative coordinate goes to 0.
__device__ __forceinline__ int cell_axis(double a, int cell_px, int nc) {
  const double t = a / (double)cell_px;
  return t >= 0.0 ? (t < (double)nc ? (int)__builtin_floor(t) : nc - 1) : 0;
}

__global__ void __launch_bounds__(kBudgetThreads) k_budget_keys(const Keypoint* __restrict__ kp, int n, int cell_px,
                                                                int ncx, int ncy,
                                                                unsigned long long* __restrict__ key,
                                                                unsigned* __restrict__ cell) {
  const long long b = tile_base();
#pragma unroll
  for (int r = 0; r < kBudgetPerThread; ++r) {
    const long long i = b + r * kBudgetThreads;
    if (i >= n) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(kp[i].interp_value) & kAbsMask;
    key[i] = bits > kInfBits ? 0ull : bits;  // a NaN is as weak as a zero
    if (cell_px > 0)
      cell[i] = (unsigned)(cell_axis(kp[i].abs_y, cell_px, ncy) * ncx + cell_axis(kp[i].abs_x, cell_px, ncx));
  }
}

// Byte p of record i's composite, and whether the bytes before it equal those of the threshold (tk, tl).
__device__ __forceinline__ bool budget_digit(unsigned long long k, unsigned tail, unsigned long long tk, unsigned tl,
                                             int p, int nb, unsigned& digit) {
  if (p < 8) {
    const int sh = 8 * (7 - p);
    digit = (unsigned)(k >> sh) & 255u;
    return p == 0 || (k >> (sh + 8)) == (tk >> (sh + 8));
  }
  const int sh = 8 * (nb - 1 - (p - 8));  // 0 <= sh <= 24
  digit = (tail >> sh) & 255u;
  return k == tk && (p == 8 || (tail >> (sh + 8)) == (tl >> (sh + 8)));  // p > 8: sh + 8 <= 24
}

struct BudgetPass {
  const unsigned long long* key;
  const unsigned* cell;     // nullptr: one cell
  const unsigned* active;   // nullptr: every record takes part
  int n, p, nb;
  const unsigned long long* tkey;  // per cell: the threshold so far
  const unsigned* ttail;
  const unsigned* rem;      // per cell: quota left (0: the cell is closed)
  unsigned* hist;           // [cells][256]
};

template <bool kLds>
__global__ void __launch_bounds__(kBudgetThreads) k_budget_hist(BudgetPass B, int cells) {
  extern __shared__ unsigned s_hist[];  // kLds: cells * 256 bins
  if (kLds) {
    for (int j = threadIdx.x; j < cells * 256; j += kBudgetThreads) s_hist[j] = 0;
    __syncthreads();
  }
  const long long b = tile_base();
#pragma unroll
  for (int r = 0; r < kBudgetPerThread; ++r) {
    const long long i = b + r * kBudgetThreads;
    if (i >= B.n) break;
    if (B.active && !B.active[i]) continue;
    const unsigned c = B.cell ? B.cell[i] : 0u;
    if (c >= (unsigned)cells || (B.p > 0 && B.rem[c] == 0)) continue;
    unsigned digit;
    if (!budget_digit(B.key[i], (unsigned)(B.n - 1 - i), B.tkey[c], B.ttail[c], B.p, B.nb, digit)) continue;
    if (kLds)
      atomicAdd(&s_hist[c * 256 + digit], 1u);
    else
      atomicAdd(&B.hist[(size_t)c * 256 + digit], 1u);
  }
  if (kLds) {
    __syncthreads();
    for (int j = threadIdx.x; j < cells * 256; j += kBudgetThreads)
      if (const unsigned v = s_hist[j]) atomicAdd(&B.hist[j], v);
  }
}

// One wave per cell; lane l holds bins 4 l .. 4 l + 3, so lane 63 holds the top ones.
__global__ void __launch_bounds__(64) k_budget_walk(unsigned* __restrict__ hist, int cells, int p, int nb, unsigned quota,
                                                    unsigned long long* __restrict__ tkey, unsigned* __restrict__ ttail,
                                                    unsigned* __restrict__ rem) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (c >= cells) return;
  uint4* bins = reinterpret_cast<uint4*>(hist + (size_t)c * 256) + lane;
  const uint4 h = *bins;
  *bins = make_uint4(0u, 0u, 0u, 0u);
  const unsigned own = h.x + h.y + h.z + h.w;
  unsigned incl = own;  // own + every higher lane
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned v = __shfl_down(incl, d, 64);
    if (lane + d < 64) incl += v;
  }
  unsigned need;
  if (p == 0) {
    const unsigned total = __shfl(incl, 0, 64);
    need = quota < total ? quota : total;
    if (lane == 0 && need == 0) {  // a closed cell: no key reaches this threshold
      tkey[c] = ~0ull;
      ttail[c] = ~0u;
      rem[c] = 0;
    }
  } else {
    need = rem[c];
  }
  if (need == 0) return;
  const unsigned above = incl - own;  // records in the bins of the higher lanes
  if (!(above < need && need <= incl)) return;  // exactly one lane holds the need-th record from the top
  const unsigned v[4] = {h.x, h.y, h.z, h.w};
  unsigned acc = above;
  int j = 3;
  while (j > 0 && acc + v[j] < need) acc += v[j--];
  const unsigned digit = (unsigned)(4 * lane + j);
  if (p < 8)
    tkey[c] = (p == 0 ? 0ull : tkey[c]) | ((unsigned long long)digit << (8 * (7 - p)));
  else
    ttail[c] = (p == 8 ? 0u : ttail[c]) | (digit << (8 * (nb - 1 - (p - 8))));
  rem[c] = need - acc;
}

__global__ void __launch_bounds__(kBudgetThreads) k_budget_flag(const unsigned long long* __restrict__ key,
                                                                const unsigned* __restrict__ cell,
                                                                const unsigned* __restrict__ active, int n, int cells,
                                                                const unsigned long long* __restrict__ tkey,
                                                                const unsigned* __restrict__ ttail,
                                                                unsigned* __restrict__ flag) {
  const long long b = tile_base();
#pragma unroll
  for (int r = 0; r < kBudgetPerThread; ++r) {
    const long long i = b + r * kBudgetThreads;
    if (i > n) return;
    unsigned ok = 0;
    if (i < n && (!active || active[i])) {  // flag[n] = 0: the scan's output there is the kept count
      const unsigned c = cell ? cell[i] : 0u;
      if (c < (unsigned)cells) {
        const unsigned long long k = key[i], tk = tkey[c];
        ok = k > tk || (k == tk && (unsigned)(n - 1 - i) >= ttail[c]);
      }
    }
    flag[i] = ok;
  }
}

// flag[n] = 0 behind flags that another kernel left (no budget step ran: every record is kept).
__global__ void __launch_bounds__(kBudgetThreads) k_budget_fill(unsigned* __restrict__ flag, int n) {
  const long long b = tile_base();
#pragma unroll
  for (int r = 0; r < kBudgetPerThread; ++r) {
    const long long i = b + r * kBudgetThreads;
    if (i > n) return;
    flag[i] = i < n;
  }
}

__global__ void __launch_bounds__(kBudgetThreads) k_budget_emit(const unsigned* __restrict__ flag,
                                                                const unsigned* __restrict__ off, int n, unsigned cap,
                                                                int32_t* __restrict__ index,
                                                                const Keypoint* __restrict__ kp,
                                                                Keypoint* __restrict__ kp_out) {
  const long long b = tile_base();
#pragma unroll
  for (int r = 0; r < kBudgetPerThread; ++r) {
    const long long i = b + r * kBudgetThreads;
    if (i >= n) return;
    if (!flag[i]) continue;
    const unsigned at = off[i];
    if (at >= cap) continue;
    if (index) index[at] = (int32_t)i;
    if (kp_out) kp_out[at] = kp[i];
  }
}

inline unsigned budget_tiles(long long items) { return (unsigned)((items + kBudgetTile - 1) / kBudgetTile); }

}  // namespace

int budget_tail_bytes(int n) {
  int nb = 1;
  for (unsigned v = n > 0 ? (unsigned)(n - 1) : 0u; v >>= 8;) ++nb;
  return nb;
}

hipError_t launch_budget_keys(const Keypoint* kp, int n, int cell_px, int ncx, int ncy, unsigned long long* key,
                              unsigned* cell, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_budget_keys, dim3(budget_tiles(n)), dim3(kBudgetThreads), 0, st, kp, n, cell_px, ncx, ncy, key,
                     cell);
  return hipGetLastError();
}

hipError_t launch_budget_select(const unsigned long long* key, const unsigned* cell, const unsigned* active, int n,
                                int cells, unsigned quota, unsigned long long* tkey, unsigned* ttail, unsigned* rem,
                                unsigned* hist, unsigned* flag, hipStream_t st) {
  if (n <= 0 || cells <= 0) return hipSuccess;
  const int nb = budget_tail_bytes(n);
  BudgetPass B{key, cell, active, n, 0, nb, tkey, ttail, rem, hist};
  const bool lds = cells <= kBudgetLdsCells;
  for (int p = 0; p < 8 + nb; ++p) {
    B.p = p;
    if (lds)
      hipLaunchKernelGGL(k_budget_hist<true>, dim3(budget_tiles(n)), dim3(kBudgetThreads),
                         (size_t)cells * 256 * sizeof(unsigned), st, B, cells);
    else
      hipLaunchKernelGGL(k_budget_hist<false>, dim3(budget_tiles(n)), dim3(kBudgetThreads), 0, st, B, cells);
    hipLaunchKernelGGL(k_budget_walk, dim3(cells), dim3(64), 0, st, hist, cells, p, nb, quota, tkey, ttail, rem);
  }
  hipLaunchKernelGGL(k_budget_flag, dim3(budget_tiles((long long)n + 1)), dim3(kBudgetThreads), 0, st, key, cell,
                     active, n, cells, tkey, ttail, flag);
  return hipGetLastError();
}

hipError_t launch_budget_fill(unsigned* flag, int n, hipStream_t st) {
  hipLaunchKernelGGL(k_budget_fill, dim3(budget_tiles((long long)n + 1)), dim3(kBudgetThreads), 0, st, flag, n);
  return hipGetLastError();
}

hipError_t launch_budget_emit(const unsigned* flag, const unsigned* off, int n, unsigned cap, int32_t* index,
                              const Keypoint* kp, Keypoint* kp_out, hipStream_t st) {
  if (n <= 0 || cap == 0 || (!index && !kp_out)) return hipSuccess;
  hipLaunchKernelGGL(k_budget_emit, dim3(budget_tiles(n)), dim3(kBudgetThreads), 0, st, flag, off, n, cap, index, kp,
                     kp_out);
  return hipGetLastError();
}

}  // namespace sift
