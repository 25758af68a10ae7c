// Least-squares homography fit of a list of pairs: the refit of the RANSAC
// inliers (the definition is stated in include/sift_hip.h and
// restated in numpy in tests/refit_ref.py).
//
// The fit is the one stage whose result is a floating-point sum over a
// data-dependent list, so the order of every addition is part of the
// definition: a fixed tree over the list order, leaves of 64 terms summed by
// halving, the chunk sums reduced by the same rule.  The tree depends on the
// list's length alone -- not on the grid, the block size or an atomic's arrival
// order -- and there is no floating-point atomic anywhere.  Everything is fp64
// `+ - * /`, comparisons and negation with contraction off.
//
// k_fit_box: the bounding boxes of the listed query and train points.  Min and
//   max are exact and order-free; the doubles travel as order-preserving
//   integer keys through integer atomicMin (the maxima as complemented keys), so
//   one memset of 0xFF initialises all of them; a block reduces in registers
//   and LDS first and issues eight atomics.  A list entry outside [0, n) is
//   not read: it clears the ok word, which makes the fit invalid.
// k_fit_sums (the hot path): a wave owns whole chunks of 64 list entries.  A
//   lane gathers its pair through the list, normalises it, forms its 44 terms
//   t = a_j a_k + b_j b_k (both products rounded, then added; the structural
//   zeros are multiplied like every other entry, so -0 and NaN come out as the
//   definition has them), and the wave reduces each with the butterfly
//   p[i] += p[i ^ s], s = 32 .. 1, through lane swaps and DPP moves (no LDS):
//   lane 0's pairing is the halving tree's, and since fp addition commutes every
//   lane holds the same bits.  Lanes past the list's end hold +0.0.  Lane 0
//   writes the chunk's 44 sums.
// k_fit_level: the same butterfly over 64 consecutive chunk sums.
// k_fit_solve: one wave.  It reduces the last level (at most 64 partials), then
//   lane 0 fills the symmetric 8 x 9 system in LDS, solves it with
//   homography_solve -- the routine k_homography_hypotheses calls -- and
//   denormalises.  It writes the FitRecord.
#include "sift_kernels.h"

#pragma clang fp contract(off)

namespace sift {

namespace {

constexpr int kFitWaves = 4;          // waves per block of k_fit_sums / k_fit_level
constexpr int kFitBoxBlocks = 256;    // grid caps: the kernels stride over the list
constexpr int kFitSumBlocks = 2048;
constexpr unsigned long long kSignBit = 1ull << 63;

// v < w  <=>  order_key(v) < order_key(w) for doubles that are not NaN (-0 < +0).
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u & kSignBit) ? ~u : (u | kSignBit);
}
// The double behind a key; the untouched 0xFF.. of a minimum and the complement
// of that of a maximum both give a NaN.
__device__ __forceinline__ double key_value(unsigned long long k) {
  return __longlong_as_double((long long)((k & kSignBit) ? (k ^ kSignBit) : ~k));
}

struct FitBox {
  double cx, cy, dq, cX, cY, dt;
};

// Centre and half of the longer side of one image side's box; a zero bound is +0.
__device__ __forceinline__ void box_side(const unsigned long long* keys, int c, double& mx, double& my, double& d) {
  const double lx = key_value(keys[c]) + 0.0, hx = key_value(~keys[4 + c]) + 0.0;
  const double ly = key_value(keys[c + 1]) + 0.0, hy = key_value(~keys[5 + c]) + 0.0;
  mx = (lx + hx) * 0.5;
  my = (ly + hy) * 0.5;
  const double w = hx - lx, h = hy - ly;
  d = (h > w ? h : w) * 0.5;
}

__device__ __forceinline__ FitBox fit_box(const unsigned long long* keys) {
  FitBox B;
  box_side(keys, 0, B.cx, B.cy, B.dq);
  box_side(keys, 2, B.cX, B.cY, B.dt);
  return B;
}

// p[i] + p[i ^ s] in every lane i, without LDS: the step-s partner of the
// halving tree (p[i] + p[i + s], i < s) is lane i ^ s, and since every earlier
// step left its result in both partners, the values have period 2 s across the
// wave when step s begins.  s = 32 and 16 use gfx950's lane swaps: with both
// operands the same register, v_permlane32_swap leaves the low half of the wave
// in both halves of one result and the high half in both halves of the other
// (v_permlane16_swap: the even rows of 16, the odd rows).  s = 8 and 4 are DPP
// row rotations by s within a row of 16 -- either direction reaches a lane that
// holds the partner's value, the period being 2 s -- and s = 2 and 1 are DPP
// quad permutations.  fp addition commutes, so both partners get the same bits.
template <int kCtrl>
__device__ __forceinline__ double dpp_move(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, kCtrl, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), kCtrl, 0xF, 0xF, true);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ double tree_step32(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)u, (unsigned)u, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
  return __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0])) +
         __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
}

__device__ __forceinline__ double tree_step16(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
  return __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0])) +
         __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
}

// The halving tree of 64 values, one per lane, for each of the 44 quantities; every lane ends with the sum.
__device__ __forceinline__ void wave_tree(double (&t)[kFitSums]) {
#pragma unroll
  for (int q = 0; q < kFitSums; ++q) {
    double v = tree_step16(tree_step32(t[q]));
    v = v + dpp_move<0x128>(v);  // row_ror:8
    v = v + dpp_move<0x124>(v);  // row_ror:4
    v = v + dpp_move<0x4E>(v);   // quad_perm:[2,3,0,1]
    v = v + dpp_move<0xB1>(v);   // quad_perm:[1,0,3,2]
    t[q] = v;
  }
}

__global__ void __launch_bounds__(256) k_fit_box(const PointPair* __restrict__ points, int n,
                                                 const int32_t* __restrict__ index, int m,
                                                 unsigned long long* __restrict__ keys) {
  unsigned long long k[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) k[c] = ~0ull;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
    const int at = index ? index[i] : (int)i;
    if (at < 0 || at >= n) {  // never read through it
      bad = true;
      continue;
    }
    const PointPair p = points[at];
    const double v[4] = {p.qx, p.qy, p.tx, p.ty};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (v[c] == v[c]) {  // a NaN has no place in the order
        const unsigned long long key = order_key(v[c]);
        k[c] = min(k[c], key);
        k[4 + c] = min(k[4 + c], ~key);
      }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) k[c] = min(k[c], (unsigned long long)__shfl_xor(k[c], s));
  }
  // the block's waves meet in LDS: eight atomics per block, all blocks on the same eight words
  __shared__ unsigned long long s_key[4][8];
  const int bad_block = __syncthreads_or(bad);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) s_key[threadIdx.x >> 6][c] = k[c];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int c = threadIdx.x;
    const unsigned long long v = min(min(s_key[0][c], s_key[1][c]), min(s_key[2][c], s_key[3][c]));
    if (v != ~0ull) atomicMin(&keys[c], v);
  }
  if (threadIdx.x == 8 && bad_block) atomicMin(&keys[8], 0ull);
}

__global__ void __launch_bounds__(64 * kFitWaves)
    k_fit_sums(const PointPair* __restrict__ points, int n, const int32_t* __restrict__ index, int m,
               const unsigned long long* __restrict__ keys, double* __restrict__ parts, long long chunks) {
  const int lane = threadIdx.x & 63;
  const FitBox B = fit_box(keys);
  for (long long c = (long long)blockIdx.x * kFitWaves + (threadIdx.x >> 6); c < chunks;
       c += (long long)gridDim.x * kFitWaves) {
    const long long i = c * kFitChunk + lane;
    double t[kFitSums];
#pragma unroll
    for (int q = 0; q < kFitSums; ++q) t[q] = 0.0;
    int at = -1;
    if (i < m) at = index ? index[i] : (int)i;
    if (at >= 0 && at < n) {
      const PointPair p = points[at];
      const double x = (p.qx - B.cx) / B.dq, y = (p.qy - B.cy) / B.dq;
      const double X = (p.tx - B.cX) / B.dt, Y = (p.ty - B.cY) / B.dt;
      const double a[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(X * x), -(X * y), X};
      const double b[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(Y * x), -(Y * y), Y};
      int q = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int k = j; k < 9; ++k, ++q) t[q] = a[j] * a[k] + b[j] * b[k];
      }
    }
    wave_tree(t);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kFitSums; ++q) parts[c * kFitSums + q] = t[q];
    }
  }
}

__global__ void __launch_bounds__(64 * kFitWaves)
    k_fit_level(const double* __restrict__ in, long long count, double* __restrict__ out, long long chunks) {
  const int lane = threadIdx.x & 63;
  for (long long c = (long long)blockIdx.x * kFitWaves + (threadIdx.x >> 6); c < chunks;
       c += (long long)gridDim.x * kFitWaves) {
    const long long i = c * kFitChunk + lane;
    double t[kFitSums];
#pragma unroll
    for (int q = 0; q < kFitSums; ++q) t[q] = i < count ? in[i * kFitSums + q] : 0.0;
    wave_tree(t);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kFitSums; ++q) out[c * kFitSums + q] = t[q];
    }
  }
}

// count partials, 1 <= count <= 64
__global__ void __launch_bounds__(64) k_fit_solve(const double* __restrict__ parts, int count,
                                                  const unsigned long long* __restrict__ keys,
                                                  FitRecord* __restrict__ rec) {
  __shared__ double a[72];
  const int lane = threadIdx.x;
  double t[kFitSums];
#pragma unroll
  for (int q = 0; q < kFitSums; ++q) t[q] = lane < count ? parts[(size_t)lane * kFitSums + q] : 0.0;
  if (count > 1) wave_tree(t);  // one value left is the sum: nothing is added to it
  if (lane != 0) return;        // no barrier below: lane 0 alone touches the LDS
  {
    int q = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int k = j; k < 9; ++k, ++q) {
        rec->sums[q] = t[q];
        a[j * 9 + k] = t[q];
        if (k < 8) a[k * 9 + j] = t[q];
      }
    }
  }
  const FitBox B = fit_box(keys);
  const double inf = __builtin_huge_val();
  bool ok = keys[8] != 0ull && B.dq > 0.0 && B.dt > 0.0 && B.dq < inf && B.dt < inf;
  double hn[8];
  ok &= homography_solve<1>(a, hn);
  const double Hn[3][3] = {{hn[0], hn[1], hn[2]}, {hn[3], hn[4], hn[5]}, {hn[6], hn[7], 1.0}};
  double G[3][3], F[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[r][0] = Hn[r][0] / B.dq;
    G[r][1] = Hn[r][1] / B.dq;
    G[r][2] = Hn[r][2] - (Hn[r][0] * B.cx + Hn[r][1] * B.cy) / B.dq;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[0][c] = B.dt * G[0][c] + B.cX * G[2][c];
    F[1][c] = B.dt * G[1][c] + B.cY * G[2][c];
    F[2][c] = G[2][c];
  }
  const double d = F[2][2];
  ok &= d != 0.0 && __builtin_fabs(d) < inf;
  double h[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    h[e] = F[e / 3][e % 3] / d;
    ok &= __builtin_fabs(h[e]) < inf;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) rec->model.h[e] = ok ? h[e] : 0.0;
  rec->model.hypothesis = ok ? 0 : -1;
  rec->model.inliers = 0;
  rec->box[0] = B.cx, rec->box[1] = B.cy, rec->box[2] = B.dq;
  rec->box[3] = B.cX, rec->box[4] = B.cY, rec->box[5] = B.dt;
}

}  // namespace

hipError_t launch_homography_fit(const PointPair* points, int n, const int32_t* index, int m, unsigned long long* keys,
                                 double* parts_a, double* parts_b, FitRecord* rec, hipStream_t st) {
  if (hipError_t e = hipMemsetAsync(keys, 0xFF, kFitKeys * sizeof(unsigned long long), st)) return e;
  const unsigned bb = (unsigned)std::min<long long>(((long long)m + 255) / 256, kFitBoxBlocks);
  hipLaunchKernelGGL(k_fit_box, dim3(bb), dim3(256), 0, st, points, n, index, m, keys);
  long long count = fit_chunks(m);
  auto blocks = [](long long chunks) {
    return dim3((unsigned)std::min<long long>((chunks + kFitWaves - 1) / kFitWaves, kFitSumBlocks));
  };
  hipLaunchKernelGGL(k_fit_sums, blocks(count), dim3(64 * kFitWaves), 0, st, points, n, index, m, keys, parts_a, count);
  double *in = parts_a, *out = parts_b;
  while (count > kFitChunk) {
    const long long next = fit_chunks(count);
    hipLaunchKernelGGL(k_fit_level, blocks(next), dim3(64 * kFitWaves), 0, st, in, count, out, next);
    std::swap(in, out);
    count = next;
  }
  hipLaunchKernelGGL(k_fit_solve, dim3(1), dim3(64), 0, st, in, (int)count, keys, rec);
  return hipGetLastError();
}

}  // namespace sift
