// Orientation assignment and 128-byte descriptors of the refined keypoints
// (gfx950): Rey-Otero & Delbracio, "Anatomy of the SIFT Method", algorithms 11
// and 12, on the context's device-resident fp32 Gaussian planes.  All
// arithmetic is fp64 in octave-local pixel units, with contraction off so the
// expressions round as written; tests/feature_ref.py states the definition.
//
// k_orient: one wave (one 64-thread block) per keypoint.  Pixel i of the box
//   (row-major) belongs to lane i mod 64; a lane adds its pixels, in
//   increasing i, into its own 36-bin histogram in LDS ([bin][lane], rows
//   padded to 65 doubles), so no two lanes ever add to one word: no atomics.
//   Bin b is then the sum of its 64 lane partials in lane order 0..63, taken
//   by lane b.  The order of every addition is a function of the keypoint
//   alone.  Six circular smoothing passes and the peak test run on lanes
//   0..35; the peaks go out as a 36-bit mask and up to 18 angles per keypoint
//   (slot = rank of the bin among the peaks).
// k_orient_emit: after the exclusive scan of the peak counts, one thread per
//   keypoint writes its records at its offset, ascending bin: ordered and
//   sort-free, like the candidate emission.
// k_describe: one wave per record, a gather by cell.  Lanes 4c .. 4c+3 own
//   cell c = 4 i + j (i from yh, j from xh) and keep its eight orientation
//   bins in registers.  The cell's support, |xh - cx_j| < 3 and |yh - cy_i| <
//   3, is a rotated square; the lanes walk its pixel bounding box (cut to the
//   descriptor box) row-major, lane q taking the pixels p = q mod 4, adding in
//   increasing p.  The cell's bins are (f0 + f1) + (f2 + f3) over its lanes
//   (two xor-shuffles); the norms add a cell's eight squares in bin order and
//   then the sixteen cells through the xor-4/8/16/32 butterfly.  No LDS, no
//   atomics, and again an order fixed by the record alone.
#include "sift_kernels.h"

#pragma clang fp contract(off)

namespace sift {

namespace {

constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 6.283185307179586;
constexpr int kHistStride = 65;  // doubles per LDS histogram row: lane b's walk over row b hits every bank

// floor(t + 0.5) of the definition, as a double (NaN stays NaN).
__device__ __forceinline__ double rnd(double t) { return floor(t + 0.5); }

// Central differences of the fp32 plane at (u, v), 1 <= u <= w-2, 1 <= v <= h-2.
__device__ __forceinline__ void gradient(const float* __restrict__ pl, int w, int u, int v, double& gx, double& gy) {
  const float* c = pl + (long long)v * w + u;
  gx = ((double)c[1] - (double)c[-1]) / 2.0;
  gy = ((double)c[w] - (double)c[-w]) / 2.0;
}

// The octave-local frame of keypoint k (the whole wave holds the same k; its
// octave and scale are made wave-uniform so they index the kernel arguments
// with scalar loads): false when it has no plane.
__device__ __forceinline__ bool local_frame(const Pyramid& P, Keypoint& k, int planes_first, double& x, double& y,
                                            double& sg) {
  const int o = k.octave = __builtin_amdgcn_readfirstlane(k.octave);
  const int s = k.scale_level = __builtin_amdgcn_readfirstlane(k.scale_level);
  if (o < planes_first || o >= P.O || s < 0 || s >= P.NS) return false;
  const double delta = ldexp(1.0, o - 1);  // background.js:611
  x = k.abs_x / delta;
  y = k.abs_y / delta;
  sg = k.abs_sigma / delta;
  return sg > 0.0;
}

// The box rnd(x -+ r) x rnd(y -+ r) if it lies within [1, w-2] x [1, h-2]
// (the comparisons run in fp64, so a NaN or an overflowing bound rejects).
__device__ __forceinline__ bool inner_box(double x, double y, double r, int w, int h, int& u0, int& u1, int& v0,
                                          int& v1) {
  const double a0 = rnd(x - r), a1 = rnd(x + r), b0 = rnd(y - r), b1 = rnd(y + r);
  if (!(a0 >= 1.0 && b0 >= 1.0 && a1 <= (double)(w - 2) && b1 <= (double)(h - 2) && a0 <= a1 && b0 <= b1))
    return false;
  u0 = (int)a0;
  u1 = (int)a1;
  v0 = (int)b0;
  v1 = (int)b1;
  return true;
}

__global__ void __launch_bounds__(64) k_orient(const Pyramid P, const float* __restrict__ gauss, int planes_first,
                                               const Keypoint* __restrict__ kp, int n,
                                               unsigned* __restrict__ count, unsigned long long* __restrict__ mask,
                                               double* __restrict__ theta) {
  __shared__ double hist[kOriBins * kHistStride];
  __shared__ double hs[2][kOriBins];
  const int i = blockIdx.x;  // < n
  const int lane = threadIdx.x;
  if (i == 0 && lane == 0) count[n] = 0;  // the scan's last input: its output there is the record count
  Keypoint k = kp[i];
  double x = 0, y = 0, sg = 0;
  int u0 = 0, u1 = 0, v0 = 0, v1 = 0;
  bool ok = local_frame(P, k, planes_first, x, y, sg);
  int w = 0;
  const float* pl = nullptr;
  if (ok) {
    const Octave& oc = P.oct[k.octave];
    w = oc.w;
    pl = gauss + oc.gauss_off + (long long)k.scale_level * oc.h * oc.w;
    ok = inner_box(x, y, 3.0 * kOriLambda * sg, oc.w, oc.h, u0, u1, v0, v1);
  }
  if (!ok) {  // uniform over the block
    if (lane == 0) {
      count[i] = 0;
      mask[i] = 0;
    }
    return;
  }
  for (int b = 0; b < kOriBins; ++b) hist[b * kHistStride + lane] = 0.0;
  const int bw = u1 - u0 + 1, npx = bw * (v1 - v0 + 1);
  const double den = 2.0 * ((kOriLambda * sg) * (kOriLambda * sg));
  for (int p = lane; p < npx; p += 64) {
    const int v = v0 + p / bw, u = u0 + p % bw;
    double gx, gy;
    gradient(pl, w, u, v, gx, gy);
    const double dx = (double)u - x, dy = (double)v - y;
    const double c = exp(-(dx * dx + dy * dy) / den) * sqrt(gx * gx + gy * gy);
    int bin;
    if (fabs(gx) == fabs(gy) && gx != 0.0) {  // t is exactly 4.5, 13.5, 22.5 or 31.5
      bin = gy > 0.0 ? (gx > 0.0 ? 5 : 14) : (gx < 0.0 ? 23 : 32);
    } else {
      double a = atan2(gy, gx);
      if (a < 0.0) a += kTwoPi;
      bin = (int)((unsigned)(int)rnd(36.0 * a / kTwoPi) % (unsigned)kOriBins);  // t in [0, 36]; 36 -> 0
    }
    hist[bin * kHistStride + lane] += c;
  }
  __syncthreads();
  if (lane < kOriBins) {
    double t = 0.0;
    for (int l = 0; l < 64; ++l) t += hist[lane * kHistStride + l];
    hs[0][lane] = t;
  }
  __syncthreads();
  const int km = lane == 0 ? kOriBins - 1 : lane - 1, kn = lane == kOriBins - 1 ? 0 : lane + 1;
  for (int it = 0; it < kOriSmooth; ++it) {
    if (lane < kOriBins) hs[(it + 1) & 1][lane] = (hs[it & 1][km] + hs[it & 1][lane] + hs[it & 1][kn]) / 3.0;
    __syncthreads();
  }
  const double* h = hs[kOriSmooth & 1];
  bool peak = false;
  double hm = 0, h0 = 0, hp = 0;
  if (lane < kOriBins) {
    double mx = h[0];
    for (int b = 1; b < kOriBins; ++b) mx = fmax(mx, h[b]);
    hm = h[km];
    h0 = h[lane];
    hp = h[kn];
    peak = h0 > hm && h0 > hp && h0 >= kOriPeakRatio * mx;
  }
  const unsigned long long m = __ballot(peak);
  if (peak) {
    double th = kTwoPi * (double)lane / 36.0 + (kPi / 36.0) * (hm - hp) / (hm - 2.0 * h0 + hp);
    if (th < 0.0) th += kTwoPi;
    if (th >= kTwoPi) th -= kTwoPi;
    theta[(long long)i * kOriMaxPeaks + __popcll(m & ((1ull << lane) - 1))] = th;
  }
  if (lane == 0) {
    count[i] = (unsigned)__popcll(m);
    mask[i] = m;
  }
}

__global__ void __launch_bounds__(256) k_orient_emit(const unsigned* __restrict__ off,
                                                     const unsigned long long* __restrict__ mask,
                                                     const double* __restrict__ theta, int n, unsigned cap,
                                                     Orientation* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long m = mask[i];
  unsigned at = off[i];
  for (int j = 0; m; ++j, ++at, m &= m - 1) {
    if (at >= cap) return;
    Orientation r;
    r.keypoint = i;
    r.bin = __ffsll((long long)m) - 1;
    r.theta = theta[(long long)i * kOriMaxPeaks + j];
    out[at] = r;
  }
}

__global__ void __launch_bounds__(256) k_describe(const Pyramid P, const float* __restrict__ gauss, int planes_first,
                                                  const Keypoint* __restrict__ kp,
                                                  const Orientation* __restrict__ ori, int n,
                                                  unsigned char* __restrict__ desc,
                                                  unsigned char* __restrict__ described,
                                                  unsigned* __restrict__ n_described) {
  const int rec = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // one wave per record
  if (rec >= n) return;
  const int lane = threadIdx.x & 63;
  const int cell = lane >> 2, q = lane & 3;
  const Orientation r = ori[rec];
  Keypoint k = kp[r.keypoint];
  unsigned long long* out = reinterpret_cast<unsigned long long*>(desc + (long long)rec * kDescBytes);
  double x = 0, y = 0, sg = 0;
  int U0 = 0, U1 = 0, V0 = 0, V1 = 0;
  bool ok = local_frame(P, k, planes_first, x, y, sg);
  int w = 0;
  const float* pl = nullptr;
  if (ok) {
    const Octave& oc = P.oct[k.octave];
    w = oc.w;
    pl = gauss + oc.gauss_off + (long long)k.scale_level * oc.h * oc.w;
    ok = inner_box(x, y, sqrt(2.0) * kDescLambda * sg * 5.0 / 4.0, oc.w, oc.h, U0, U1, V0, V1);
  }
  if (!ok) {  // uniform over the wave
    if (q == 0) out[cell] = 0ull;
    if (lane == 0) described[rec] = 0;
    return;
  }
  const double ct = cos(r.theta), st = sin(r.theta);
  const double cx = ((double)(cell & 3) - 1.5) * 3.0, cy = ((double)(cell >> 2) - 1.5) * 3.0;
  // Pixel bounding box of the cell's support (a square of half-side 3 sg
  // about the rotated cell centre), one pixel wider each way than its real
  // bounds need; the weights below decide every pixel.
  const double px = x + sg * (cx * ct - cy * st), py = y + sg * (cx * st + cy * ct);
  const double e = 3.0 * sg * (fabs(ct) + fabs(st)) + 1.0;
  const int u0 = max(U0, (int)fmax(floor(px - e), (double)U0)), u1 = min(U1, (int)fmin(ceil(px + e), (double)U1));
  const int v0 = max(V0, (int)fmax(floor(py - e), (double)V0)), v1 = min(V1, (int)fmin(ceil(py + e), (double)V1));
  const int bw = u1 - u0 + 1, npx = (bw > 0 && v1 >= v0) ? bw * (v1 - v0 + 1) : 0;
  // Per pixel the definition divides by sg, 3, 2 (lambda sg)^2 and, per bin,
  // 2 pi / 8; fp64 division is the dearest instruction here, so the loop
  // multiplies by the reciprocals and measures the orientation distance in
  // bins (t = a 8 / 2 pi, one division): the same function, rounded
  // differently in the last bits.
  const double inv_sg = 1.0 / sg, third = 1.0 / 3.0;
  const double neg_inv_den = -1.0 / (2.0 * ((kDescLambda * sg) * (kDescLambda * sg)));
  double f[kDescOri];
#pragma unroll
  for (int b = 0; b < kDescOri; ++b) f[b] = 0.0;
  for (int p = q; p < npx; p += 4) {
    const int v = v0 + p / bw, u = u0 + p % bw;
    const double dx = (double)u - x, dy = (double)v - y;
    const double xh = (dx * ct + dy * st) * inv_sg, yh = (-dx * st + dy * ct) * inv_sg;
    if (!(fmax(fabs(xh), fabs(yh)) < 7.5)) continue;
    const double wx = 1.0 - fabs(xh - cx) * third, wy = 1.0 - fabs(yh - cy) * third;
    if (!(wx > 0.0 && wy > 0.0)) continue;
    double gx, gy;
    gradient(pl, w, u, v, gx, gy);
    const double c = exp((dx * dx + dy * dy) * neg_inv_den) * sqrt(gx * gx + gy * gy);
    double a = atan2(gy, gx) - r.theta;  // in (-3 pi, pi]
    if (a < 0.0) a += kTwoPi;
    if (a < 0.0) a += kTwoPi;
    // wk = 1 - d_k is positive for the bin at or below t and the one above
    // it (circularly) only: d = t - floor(t) and floor(t) + 1 - t, both exact.
    const double t = a * 8.0 / kTwoPi, wc = wy * wx * c, tf = floor(t);
    const int b0 = (int)tf & 7, b1 = (b0 + 1) & 7;
    const double w0 = wc * (1.0 - (t - tf)), w1 = wc * (1.0 - ((tf + 1.0) - t));
#pragma unroll
    for (int b = 0; b < kDescOri; ++b) f[b] += b == b0 ? w0 : (b == b1 ? w1 : 0.0);
  }
  double ss = 0.0;
#pragma unroll
  for (int b = 0; b < kDescOri; ++b) {
    f[b] += __shfl_xor(f[b], 1);
    f[b] += __shfl_xor(f[b], 2);
    ss += f[b] * f[b];
  }
#pragma unroll
  for (int sh = 4; sh < 64; sh <<= 1) ss += __shfl_xor(ss, sh);
  const double nrm = sqrt(ss);
  unsigned long long bytes = 0ull;
  if (nrm > 0.0) {
    const double cap = kDescCap * nrm;
    double s2 = 0.0;
#pragma unroll
    for (int b = 0; b < kDescOri; ++b) {
      f[b] = fmin(f[b], cap);
      s2 += f[b] * f[b];
    }
#pragma unroll
    for (int sh = 4; sh < 64; sh <<= 1) s2 += __shfl_xor(s2, sh);
    const double n2 = sqrt(s2);
#pragma unroll
    for (int b = 0; b < kDescOri; ++b)
      bytes |= (unsigned long long)fmin(floor(512.0 * f[b] / n2), 255.0) << (8 * b);
  }
  if (q == 0) out[cell] = bytes;
  if (lane == 0) {
    described[rec] = 1;
    atomicAdd(n_described, 1u);  // an integer count: the order of the adds does not show
  }
}

}  // namespace

hipError_t launch_orient(const Pyramid& P, const float* gauss, int planes_first, const Keypoint* kp, int n,
                         unsigned* count, unsigned long long* mask, double* theta, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_orient, dim3(n), dim3(64), 0, st, P, gauss, planes_first, kp, n, count, mask, theta);
  return hipGetLastError();
}

hipError_t launch_orient_emit(const unsigned* off, const unsigned long long* mask, const double* theta, int n,
                              unsigned cap, Orientation* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_orient_emit, dim3((n + 255) / 256), dim3(256), 0, st, off, mask, theta, n, cap, out);
  return hipGetLastError();
}

hipError_t launch_describe(const Pyramid& P, const float* gauss, int planes_first, const Keypoint* kp,
                           const Orientation* ori, int n, unsigned char* desc, unsigned char* described,
                           unsigned* n_described, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_describe, dim3((n + 3) / 4), dim3(256), 0, st, P, gauss, planes_first, kp, ori, n, desc,
                     described, n_described);
  return hipGetLastError();
}

}  // namespace sift
