// The k_gauss_dog instantiations on a base plane (octaves >= 1, octave 0 materialised); the split vertical pass.
#include "sift_gauss_tile.h"

namespace sift {

// Split vertical pass (large radii, kGaussSplitTiles).  A 64-column tile
// recomputes the vertical sums of its 2r halo columns: (64 + 2r) / 64 of the
// vertical work (2.5x at r = 47, 6.9x at r = 188), serialised in the tile's
// waves.  k_gauss_vert computes every (scale, row, column) sum once, one lane
// per column and eight rows per wave, into fp64 scratch planes, with
// vert_glob_gen's exact chunking (rows yb + jb + k, zero-padded taps in
// increasing order from 0.0): every value is bit-identical to the tile
// kernel's own.  The tile kernel then copies its strip (vert_copy).
__global__ __launch_bounds__(256) void k_gauss_vert(const Pyramid P, int o, const double* __restrict__ base,
                                                    double* __restrict__ vout, long long bstride,
                                                    long long vstride) {
  const Octave& oc = P.oct[o];
  // z = image * NS + (NS - 1 - scale): largest radius (longest chains) first,
  // blocks are dispatched in z order
  const int im = (int)blockIdx.z / P.NS;
  const int s = P.NS - 1 - ((int)blockIdx.z - im * P.NS);
  base += im * bstride;
  vout += im * vstride;
  const int r = oc.rad[s], h = oc.h, w = oc.w;
  const cdouble* wp = (const cdouble*)(P.wts + oc.wofs[s]);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = blockIdx.x * kGX + lane;
  const int y0 = blockIdx.y * kVertRows + kVertNO * wv;
  if (y0 >= h) return;  // wave-uniform
  const __amdgpu_buffer_rsrc_t rs = urs(const_cast<double*>(base), h * w * 8);
  const int xoff = min(x, w - 1) * 8;
  const int NJ = 2 * r + kVertNO, yb = y0 - r;
  double acc[kVertNO];
#pragma unroll
  for (int t = 0; t < kVertNO; ++t) acc[t] = 0.0;
  auto chunk = [&](int jb, auto C, auto first) {
    using CC = decltype(C);
    double v[8];
#pragma unroll
    for (int k = 0; k < CC::kRows; ++k)
      v[k] = load_f64(rs, xoff, __builtin_amdgcn_readfirstlane(clampi(yb + jb + k, 0, h - 1) * w * 8));
    const cdouble* wq = wp + jb;
    CC::template run<decltype(first)::value>([&](int k, int t) { acc[t] = fma((double)wq[k - t], v[k], acc[t]); });
    pin(acc);
  };
  // 16 rows per wave: the window's 2r + 16 rows serve 16 outputs (2r + 8
  // for 8 before: 12.75 -> 6.9 loads per output at r = 47), the same fma
  // chain per output (taps in increasing order from 0.0).
  vchunk16_dispatch<true>(2 * r, [&](auto C, auto f) { chunk(0, C, f); });
  for (int jb = 8; jb < NJ; jb += 8)
    vchunk16_dispatch<false>(2 * r - jb, [&](auto C, auto f) { chunk(jb, C, f); });
  if (x < w) {
    double* dst = vout + (long long)s * h * w + (long long)y0 * w + x;
#pragma unroll
    for (int t = 0; t < kVertNO; ++t)
      if (y0 + t < h) dst[(long long)t * w] = acc[t];
  }
}

GaussKernelFn gauss_tile1_kernel(int k) {
  return k == kKTiles ? k_gauss_dog<false, 0, kUR1, false> : k_gauss_dog<false, 0, SIFT_VS_RMAX, false, true>;
}

}  // namespace sift
