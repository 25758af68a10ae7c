// Homography warp of a gray (fp32) or RGBA (4 x uint8) image (gfx950); the definition is in include/sift_hip.h
// ("Homography warp").  Everything is fp64 with contraction off and no library function but floor.
//
// One lane per destination pixel of a 64 x 16 tile: a block is 64 x 4 lanes and walks the tile's rows in four
// steps, so a wave stores 64 consecutive pixels of one destination row (256 B gray or RGBA, 64 B of mask).  The
// matrix, the dimensions and the strides are kernel arguments (SGPRs).  The neighbours are direct global loads: for
// the near-identity maps registration produces, a wave's four loads cover two source rows of ~65 consecutive pixels,
// and an RGBA neighbour is one 32-bit load.  The validity test comes before every cast to an integer and every
// load; an invalid lane loads nothing.  At most kWarpMaxBlocks blocks stride over the tiles; valid pixels are counted
// with ballots into one word per block, which k_warp_count (one block) sums: integers, no atomics.
#include <type_traits>

#include "sift_kernels.h"

#pragma clang fp contract(off)

namespace sift {

namespace {

constexpr int kWarpTW = 64;                      // tile width = lanes of a wave
constexpr int kWarpWaves = 4;                    // rows of one step = waves of a block
constexpr int kWarpSteps = 4;                    // steps of a block
constexpr int kWarpTH = kWarpWaves * kWarpSteps;  // tile height

struct WarpMap {
  double m[9];
};

// Source position of destination pixel (X, Y); true iff it is valid.
__device__ __forceinline__ bool warp_source(const WarpMap& M, int X, int Y, int sw, int sh, double& sx, double& sy) {
  const double x = (double)X, y = (double)Y;
  const double u = (M.m[0] * x + M.m[1] * y) + M.m[2];
  const double v = (M.m[3] * x + M.m[4] * y) + M.m[5];
  const double w = (M.m[6] * x + M.m[7] * y) + M.m[8];
  const double r = 1.0 / w;
  sx = u * r;
  sy = v * r;
  return w > 0.0 && sx >= 0.0 && sy >= 0.0 && sx <= (double)(sw - 1) && sy <= (double)(sh - 1);
}

// One axis of the bilinear form for a valid position s in [0, n-1]: i0 = min(floor(s), max(n-2, 0)),
// i1 = min(i0+1, n-1), f = s - i0, g = 1 - f.
__device__ __forceinline__ void warp_axis(double s, int n, int& i0, int& i1, double& f, double& g) {
  const double lim = (double)(n >= 2 ? n - 2 : 0);
  double b = floor(s);
  if (b > lim) b = lim;
  i0 = (int)b;
  i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
  f = s - b;
  g = 1.0 - f;
}

struct WarpWeights {
  double fx, gx, fy, gy;
};

// Every product rounded, then added.
__device__ __forceinline__ double warp_lerp2(double p00, double p01, double p10, double p11, const WarpWeights& k) {
  const double top = p00 * k.gx + p01 * k.fx;
  const double bot = p10 * k.gx + p11 * k.fx;
  return top * k.gy + bot * k.fy;
}

__device__ __forceinline__ float warp_pixel(float a, float b, float c, float d, const WarpWeights& k) {
  return (float)warp_lerp2((double)a, (double)b, (double)c, (double)d, k);  // rounded once
}

// The four channels of an RGBA word, each floor(val + 0.5); val lies in [0, 255], so nothing clamps.
__device__ __forceinline__ unsigned warp_pixel(unsigned a, unsigned b, unsigned c, unsigned d, const WarpWeights& k) {
  unsigned out = 0;
#pragma unroll
  for (int sh = 0; sh < 32; sh += 8) {
    const double val = warp_lerp2((double)((a >> sh) & 0xffu), (double)((b >> sh) & 0xffu),
                                  (double)((c >> sh) & 0xffu), (double)((d >> sh) & 0xffu), k);
    out |= (unsigned)floor(val + 0.5) << sh;
  }
  return out;
}

// The tiles blockIdx.x, blockIdx.x + gridDim.x, ... < tiles.  T = float (gray) or unsigned (RGBA, one word per pixel);
// strides in elements of T.  partial[blockIdx.x] receives the block's valid pixels (nullptr: not counted).
template <bool kBilinear, class T>
__device__ __forceinline__ void warp_tiles(const T* __restrict__ src, int sw, int sh, size_t sstride, const WarpMap& M,
                                           T fill, T* __restrict__ dst, int dw, int dh, size_t dstride,
                                           unsigned char* __restrict__ mask, unsigned* __restrict__ partial,
                                           unsigned tiles_x, unsigned tiles) {
  static_assert(std::is_same<T, float>::value || std::is_same<T, unsigned>::value, "gray or RGBA");
  __shared__ unsigned s_cnt[kWarpWaves];
  unsigned wave_valid = 0;  // wave-uniform
  for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
    const unsigned ty = t / tiles_x, tx = t - ty * tiles_x;
    const unsigned Xu = tx * kWarpTW + threadIdx.x;  // < 2^31 + 64
    const int X = (int)Xu;                           // used where Xu < dw
#pragma unroll
    for (int step = 0; step < kWarpSteps; ++step) {
      const unsigned Yu = ty * kWarpTH + step * kWarpWaves + threadIdx.y;  // < 2^31 + 16
      const bool inside = Xu < (unsigned)dw && Yu < (unsigned)dh;
      const int Y = (int)Yu;
      double sx = 0.0, sy = 0.0;
      const bool valid = inside && warp_source(M, X, Y, sw, sh, sx, sy);
      wave_valid += (unsigned)__popcll(__ballot(valid));
      T out = fill;
      if (valid) {
        if (!kBilinear) {
          const int xn = (int)floor(sx + 0.5), yn = (int)floor(sy + 0.5);
          out = src[(size_t)yn * sstride + xn];
        } else {
          int x0, x1, y0, y1;
          WarpWeights k;
          warp_axis(sx, sw, x0, x1, k.fx, k.gx);
          warp_axis(sy, sh, y0, y1, k.fy, k.gy);
          const T* r0 = src + (size_t)y0 * sstride;
          const T* r1 = src + (size_t)y1 * sstride;
          out = warp_pixel(r0[x0], r0[x1], r1[x0], r1[x1], k);
        }
      }
      if (inside) {
        dst[(size_t)Y * dstride + X] = out;
        if (mask) mask[(size_t)Y * dw + X] = valid ? 1 : 0;
      }
    }
  }
  if (partial) {  // uniform over the grid
    if (threadIdx.x == 0) s_cnt[threadIdx.y] = wave_valid;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
      unsigned n = 0;
      for (int w = 0; w < kWarpWaves; ++w) n += s_cnt[w];
      partial[blockIdx.x] = n;
    }
  }
}

// *count = the sum of partial[0 .. n), n <= kWarpMaxBlocks: one block.
__global__ void __launch_bounds__(256) k_warp_count(const unsigned* __restrict__ partial, int n,
                                                    unsigned* __restrict__ count) {
  __shared__ unsigned s_sum[4];
  unsigned v = 0;
  for (int i = threadIdx.x; i < n; i += 256) v += partial[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *count = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

template <bool kBilinear>
__global__ void __launch_bounds__(kWarpTW* kWarpWaves)
    k_warp_gray(const float* __restrict__ src, int sw, int sh, size_t sstride, WarpMap M, float fill,
                float* __restrict__ dst, int dw, int dh, size_t dstride, unsigned char* __restrict__ mask,
                unsigned* __restrict__ partial, unsigned tiles_x, unsigned tiles) {
  warp_tiles<kBilinear, float>(src, sw, sh, sstride, M, fill, dst, dw, dh, dstride, mask, partial, tiles_x, tiles);
}

template <bool kBilinear>
__global__ void __launch_bounds__(kWarpTW* kWarpWaves)
    k_warp_rgba(const unsigned* __restrict__ src, int sw, int sh, size_t sstride, WarpMap M, unsigned fill,
                unsigned* __restrict__ dst, int dw, int dh, size_t dstride, unsigned char* __restrict__ mask,
                unsigned* __restrict__ partial, unsigned tiles_x, unsigned tiles) {
  warp_tiles<kBilinear, unsigned>(src, sw, sh, sstride, M, fill, dst, dw, dh, dstride, mask, partial, tiles_x, tiles);
}

struct WarpGrid {
  unsigned tiles_x, tiles;
};
inline WarpGrid warp_grid(int dw, int dh) {
  const unsigned tx = ((unsigned)dw + kWarpTW - 1) / kWarpTW, ty = ((unsigned)dh + kWarpTH - 1) / kWarpTH;
  return {tx, tx * ty};  // dw * dh < 2^31, so tx * ty < 2^31 / 64 + tx + ty < 2^31
}

WarpMap warp_map(const double* m) {
  WarpMap M;
  for (int i = 0; i < 9; ++i) M.m[i] = m[i];
  return M;
}

// partial: kWarpMaxBlocks words, read when count is not nullptr.
template <class T, class KB, class KN>
hipError_t launch_warp(KB bilinear_kernel, KN nearest_kernel, const T* src, int sw, int sh, size_t sstride,
                       const double* m, bool bilinear, T fill, T* dst, int dw, int dh, size_t dstride,
                       unsigned char* mask, unsigned* partial, unsigned* count, hipStream_t st) {
  const WarpGrid g = warp_grid(dw, dh);
  const unsigned blocks = std::min(g.tiles, (unsigned)kWarpMaxBlocks);
  const dim3 block(kWarpTW, kWarpWaves);
  unsigned* part = count ? partial : nullptr;
  if (bilinear)
    hipLaunchKernelGGL(bilinear_kernel, dim3(blocks), block, 0, st, src, sw, sh, sstride, warp_map(m), fill, dst, dw,
                       dh, dstride, mask, part, g.tiles_x, g.tiles);
  else
    hipLaunchKernelGGL(nearest_kernel, dim3(blocks), block, 0, st, src, sw, sh, sstride, warp_map(m), fill, dst, dw,
                       dh, dstride, mask, part, g.tiles_x, g.tiles);
  if (count) hipLaunchKernelGGL(k_warp_count, dim3(1), dim3(256), 0, st, (const unsigned*)part, (int)blocks, count);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_warp_gray(const float* src, int sw, int sh, size_t sstride_px, const double* m, bool bilinear,
                            float fill, float* dst, int dw, int dh, size_t dstride_px, unsigned char* mask,
                            unsigned* partial, unsigned* count, hipStream_t st) {
  return launch_warp(k_warp_gray<true>, k_warp_gray<false>, src, sw, sh, sstride_px, m, bilinear, fill, dst, dw, dh,
                     dstride_px, mask, partial, count, st);
}

hipError_t launch_warp_rgba(const unsigned* src, int sw, int sh, size_t sstride_px, const double* m, bool bilinear,
                            unsigned fill, unsigned* dst, int dw, int dh, size_t dstride_px, unsigned char* mask,
                            unsigned* partial, unsigned* count, hipStream_t st) {
  return launch_warp(k_warp_rgba<true>, k_warp_rgba<false>, src, sw, sh, sstride_px, m, bilinear, fill, dst, dw, dh,
                     dstride_px, mask, partial, count, st);
}

}  // namespace sift
