// RANSAC homography verification of match pairs (the
// definition is stated in include/sift_hip.h and restated in numpy in
// tests/ransac_ref.py).
//
// Everything is fp64 `+ - * /` and comparisons with contraction off, and every
// sum over pairs is an integer: the result is exact with respect to the
// definition and does not depend on the grid.
//
// k_pair_points: (abs_x, abs_y) of the two keypoints behind each match pair.
// k_homography_hypotheses: one thread per hypothesis: four distinct indices from
//   the counter-based splitmix64 mixer, the 8 x 9 system, Gaussian elimination
//   with partial pivoting.  The matrix sits in LDS, entry e of lane l at
//   a[e][l]: the pivot row is a runtime index, which in registers would mean
//   scratch; here it is an LDS address, and lanes never share an entry.
// k_homography_score (the hot path): a lane keeps kScoreR pairs in registers
//   for the whole kernel and walks a tile of hypotheses whose coefficients are
//   wave-uniform loads; per hypothesis the wave's count is the popcount of its
//   ballots, the block's waves meet in LDS once after the tile, and one integer
//   atomicAdd per block and hypothesis lands in counts.  Lanes past the last
//   pair hold NaN pairs, which are never inliers: no bound test in the loop.
// k_homography_best: invalid hypotheses get count -1; one block takes the
//   arg-max of (count, -k) and writes the model record.
// k_inlier_flag / k_inlier_emit: the best model's inliers as a flag array, its
//   exclusive scan and an ordered emission -- no sort.
#include "sift_kernels.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace sift {

namespace {

constexpr int kHypLanes = 64;  // hypotheses (threads) per block of k_homography_hypotheses

__device__ __forceinline__ unsigned long long splitmix64_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) k_pair_points(const MatchPair* __restrict__ pairs, int n,
                                                     const Orientation* __restrict__ q_ori, int nq_ori,
                                                     const Keypoint* __restrict__ q_kp, int nq_kp,
                                                     const Orientation* __restrict__ t_ori, int nt_ori,
                                                     const Keypoint* __restrict__ t_kp, int nt_kp,
                                                     PointPair* __restrict__ points) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // the grid may pass 2^31 threads
  if (i >= n) return;
  const double nan = __builtin_nan("");
  PointPair out{nan, nan, nan, nan};
  const MatchPair m = pairs[i];
  if (m.query >= 0 && m.query < nq_ori && m.train >= 0 && m.train < nt_ori) {
    const int kq = q_ori[m.query].keypoint, kt = t_ori[m.train].keypoint;
    if (kq >= 0 && kq < nq_kp && kt >= 0 && kt < nt_kp)
      out = PointPair{q_kp[kq].abs_x, q_kp[kq].abs_y, t_kp[kt].abs_x, t_kp[kt].abs_y};
  }
  points[i] = out;
}

__global__ void __launch_bounds__(kHypLanes) k_homography_hypotheses(const PointPair* __restrict__ points, int n, int K,
                                                                     unsigned long long seed, double* __restrict__ H,
                                                                     int* __restrict__ valid) {
  __shared__ double a[72][kHypLanes];
  const int lane = threadIdx.x;
  const int k = blockIdx.x * kHypLanes + lane;
  if (k >= K) return;  // no barrier below: lanes never share an entry
#define A_(r, c) a[(r) * 9 + (c)][lane]

  // four distinct indices in draw order; srt holds the earlier ones ascending
  unsigned srt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned long long z =
        splitmix64_mix(seed + (4ull * (unsigned long long)k + (unsigned long long)(i + 1)) * 0x9E3779B97F4A7C15ull);
    unsigned r = (unsigned)(((z >> 32) * (unsigned long long)(n - i)) >> 32);  // < n - i
#pragma unroll
    for (int j = 0; j < i; ++j)
      if (r >= srt[j]) ++r;  // < n after at most i steps
    const PointPair p = points[r];
    A_(2 * i, 0) = p.qx, A_(2 * i, 1) = p.qy, A_(2 * i, 2) = 1.0;
    A_(2 * i, 3) = 0.0, A_(2 * i, 4) = 0.0, A_(2 * i, 5) = 0.0;
    A_(2 * i, 6) = -p.tx * p.qx, A_(2 * i, 7) = -p.tx * p.qy, A_(2 * i, 8) = p.tx;
    A_(2 * i + 1, 0) = 0.0, A_(2 * i + 1, 1) = 0.0, A_(2 * i + 1, 2) = 0.0;
    A_(2 * i + 1, 3) = p.qx, A_(2 * i + 1, 4) = p.qy, A_(2 * i + 1, 5) = 1.0;
    A_(2 * i + 1, 6) = -p.ty * p.qx, A_(2 * i + 1, 7) = -p.ty * p.qy, A_(2 * i + 1, 8) = p.ty;
    unsigned v = r;
#pragma unroll
    for (int j = 0; j < i; ++j) {
      const unsigned lo = min(srt[j], v);
      v = max(srt[j], v);
      srt[j] = lo;
    }
    srt[i] = v;
  }

#undef A_
  double h[8];
  const bool ok = homography_solve<kHypLanes>(&a[0][lane], h);
#pragma unroll
  for (int j = 0; j < 8; ++j) H[(size_t)k * 9 + j] = ok ? h[j] : 0.0;
  H[(size_t)k * 9 + 8] = ok ? 1.0 : 0.0;
  valid[k] = ok;
}

// grid (pair blocks, hypothesis tiles)
__global__ void __launch_bounds__(64 * kScoreWaves)
    k_homography_score(const PointPair* __restrict__ points, int n, const double* __restrict__ H, int K, double t2,
                       int* __restrict__ counts) {
  __shared__ int s_cnt[kScoreWaves][kScoreTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double x[kScoreR], y[kScoreR], X[kScoreR], Y[kScoreR];
#pragma unroll
  for (int r = 0; r < kScoreR; ++r) {
    const long long i = (long long)blockIdx.x * kScorePairs + r * (64 * kScoreWaves) + threadIdx.x;
    x[r] = y[r] = X[r] = Y[r] = __builtin_nan("");
    if (i < n) {
      const PointPair p = points[i];
      x[r] = p.qx, y[r] = p.qy, X[r] = p.tx, Y[r] = p.ty;
    }
  }
  const int k0 = blockIdx.y * kScoreTile;
  const int kn = min(kScoreTile, K - k0);
  for (int kk = 0; kk < kn; ++kk) {
    const double* h = H + (size_t)(k0 + kk) * 9;  // wave-uniform
    const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7], h8 = h[8];
    int c = 0;
#pragma unroll
    for (int r = 0; r < kScoreR; ++r)
      c += __popcll(__ballot(homography_inlier(h0, h1, h2, h3, h4, h5, h6, h7, h8, x[r], y[r], X[r], Y[r], t2)));
    if (lane == 0) s_cnt[wave][kk] = c;
  }
  __syncthreads();
  if ((int)threadIdx.x < kn) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kScoreWaves; ++w) s += s_cnt[w][threadIdx.x];
    if (s) atomicAdd(&counts[k0 + threadIdx.x], s);
  }
}

__global__ void __launch_bounds__(1024) k_homography_best(const double* __restrict__ H, const int* __restrict__ valid,
                                                          int* __restrict__ counts, int K,
                                                          Homography* __restrict__ model) {
  __shared__ long long s_key[1024];
  // (count, -k) as one signed key: count >= -1 and k < 65536
  long long key = LLONG_MIN;
  for (int k = threadIdx.x; k < K; k += 1024) {
    const int c = valid[k] ? counts[k] : -1;
    counts[k] = c;
    key = max(key, (long long)c * kMaxHypotheses + (kMaxHypotheses - 1 - k));
  }
  s_key[threadIdx.x] = key;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_key[threadIdx.x] = max(s_key[threadIdx.x], s_key[threadIdx.x + s]);
    __syncthreads();
  }
  key = s_key[0];
  const bool any = key >= 0;  // an invalid hypothesis' key is negative; so is that of K == 0
  const int k = any ? kMaxHypotheses - 1 - (int)(key % kMaxHypotheses) : -1;
  if (threadIdx.x < 9) model->h[threadIdx.x] = any ? H[(size_t)k * 9 + threadIdx.x] : 0.0;
  if (threadIdx.x == 0) {
    model->hypothesis = k;
    model->inliers = any ? (int)(key / kMaxHypotheses) : 0;
  }
}

__global__ void __launch_bounds__(256) k_inlier_flag(const PointPair* __restrict__ points, int n,
                                                     const Homography* __restrict__ model, double t2,
                                                     unsigned* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // the grid may pass 2^31 threads
  if (i > n) return;
  unsigned ok = 0;
  if (i < n && model->hypothesis >= 0) {  // flag[n] = 0: the scan's output there is the inlier count
    const double* h = model->h;
    const PointPair p = points[i];
    ok = homography_inlier(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], p.qx, p.qy, p.tx, p.ty, t2);
  }
  flag[i] = ok;
}

__global__ void __launch_bounds__(256) k_inlier_emit(const unsigned* __restrict__ flag, const unsigned* __restrict__ off,
                                                     int n, unsigned cap, int32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // the grid may pass 2^31 threads
  if (i >= n || !flag[i]) return;
  const unsigned at = off[i];
  if (at >= cap) return;
  out[at] = (int32_t)i;
}

}  // namespace

hipError_t launch_pair_points(const MatchPair* pairs, int n, const Orientation* q_ori, int nq_ori, const Keypoint* q_kp,
                              int nq_kp, const Orientation* t_ori, int nt_ori, const Keypoint* t_kp, int nt_kp,
                              PointPair* points, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pair_points, dim3(n / 256 + 1), dim3(256), 0, st, pairs, n, q_ori, nq_ori, q_kp, nq_kp,
                     t_ori, nt_ori, t_kp, nt_kp, points);
  return hipGetLastError();
}

hipError_t launch_homography_hypotheses(const PointPair* points, int n, int K, unsigned long long seed, double* H,
                                        int* valid, hipStream_t st) {
  if (K <= 0 || n < 4) return hipSuccess;
  hipLaunchKernelGGL(k_homography_hypotheses, dim3((K + kHypLanes - 1) / kHypLanes), dim3(kHypLanes), 0, st, points, n,
                     K, seed, H, valid);
  return hipGetLastError();
}

hipError_t launch_homography_score(const PointPair* points, int n, const double* H, int K, double t2, int* counts,
                                   hipStream_t st) {
  if (K <= 0 || n <= 0) return hipSuccess;
  const unsigned bx = (unsigned)(((long long)n + kScorePairs - 1) / kScorePairs);  // < 2^21
  hipLaunchKernelGGL(k_homography_score, dim3(bx, (K + kScoreTile - 1) / kScoreTile), dim3(64 * kScoreWaves), 0, st,
                     points, n, H, K, t2, counts);
  return hipGetLastError();
}

hipError_t launch_homography_best(const double* H, const int* valid, int* counts, int K, Homography* model,
                                  hipStream_t st) {
  hipLaunchKernelGGL(k_homography_best, dim3(1), dim3(1024), 0, st, H, valid, counts, K, model);
  return hipGetLastError();
}

hipError_t launch_inlier_flag(const PointPair* points, int n, const Homography* model, double t2, unsigned* flag,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_inlier_flag, dim3(n / 256 + 1), dim3(256), 0, st, points, n, model, t2, flag);
  return hipGetLastError();
}

hipError_t launch_inlier_emit(const unsigned* flag, const unsigned* off, int n, unsigned cap, int32_t* out,
                              hipStream_t st) {
  if (n <= 0 || cap == 0) return hipSuccess;
  hipLaunchKernelGGL(k_inlier_emit, dim3(n / 256 + 1), dim3(256), 0, st, flag, off, n, cap, out);
  return hipGetLastError();
}

}  // namespace sift
