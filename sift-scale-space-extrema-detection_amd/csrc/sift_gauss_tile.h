// Gaussian scale space + Difference-of-Gaussians for one octave (gfx950).
//
// Replaces background.js:71-237 (computeGaussianScaleSpace, whose hot loop is
// SIFT_blurMatrix2DChunk, sift.js:72-149) and background.js:258-354
// (computeDifferenceOfGaussians / SIFT_subtractMatrix2DChunk, sift.js:154-188).
//
// The reference convolves every scale of an octave with a full 2D kernel of
// the SAME octave base (the blur is not incremental, background.js:173-177).
// The 2D kernel is exactly separable (w(i) w(j), sift.js:22-67).  One block
// owns a 64x32 output tile; each of its 4 waves owns 8 rows of it and walks
// all scales of the octave on its own (no block barrier after the staging):
//
//   vertical pass   base -> fp64 LDS strip rows 8 wv .. 8 wv + 7, columns
//                   x0 - r .. x0 + 63 + r: lanes are columns with an 8-row
//                   register window (every base value loaded once per
//                   window); the 2r halo columns are packed into one pass of
//                   (column, row-slice) lanes;
//   horizontal pass strip -> 4 adjacent columns x 2 rows per lane, the row
//                   window read with 16-byte LDS loads;
//   epilogue        L_s and DoG L_{s-1} - L_s (formed in fp64, rounded once)
//                   as 16-byte buffer stores; for s == S the fp64 seed of the
//                   next octave (background.js:114-118).
//
// A wave touches only its own strip rows, so the only ordering it needs is
// its own (wave_lds_fence).  Radii 0..RMAX run fully unrolled code
// specialised on the radius (every tap an SGPR operand of v_fma_f64, every
// load an immediate-offset LDS read or a buffer load with the row in an
// SGPR); larger radii run 8-wide chunks over zero-padded taps (fma(0, v, acc)
// == acc, so the results are identical).
//
// Octave 0's base is the 2x nearest-neighbour upsample of the input
// (background.js:84): B[y][x] = I[clamp(y>>1)][clamp(x>>1)], never
// materialised.  The block stages its input region (fp64) in LDS; the
// vertical pass runs on input columns only (the vertical sums depend on x
// only through x>>1) and the horizontal pass reads the half-resolution strip
// through the same index map -- the same operations on the same values as a
// full-resolution pass, half the loads.
//
// Every output pixel runs the same fma chain (taps in increasing order,
// vertical then horizontal, starting from 0.0) on its clamped neighbourhood:
// the result is translation invariant like the reference's 2D sum, and
// sift_exact.h reproduces any single pixel bit for bit.
//
// Roofline: octave 0 is HBM-bound on the plane stores (per octave pixel
// 4(S+3) + 4(S+2) bytes written against 1 byte of input read); the small
// octaves, whose radii double per octave, are bound by fp64 FMA issue.
// (Instantiated in sift_gauss_tile0.hip and sift_gauss_tile1.hip.)
#pragma once
#include "sift_gauss_dev.h"
#include "sift_xmask.h"

namespace sift {

constexpr int kPFV = 12;            // rows in flight, vertical pass from global memory
constexpr int kPFL = 4;              // rows in flight, vertical pass from LDS
constexpr int kPFH = 3;              // 16-byte reads in flight, horizontal pass

struct GTile {
  int h, w, x0, y0;
  int bx;              // tile column
  int lane, wv;        // wv wave-uniform (SGPR)
  int cg, rs;          // horizontal mapping (64-column tiles)
  int sw;              // strip stride
  int hrm;             // octave 0: ceil(RM / 2) of the staged region
  const double* S0;    // octave 0: staged input region [..][kBW0]
  __amdgpu_buffer_rsrc_t rsrc;  // o >= 1 (or materialised octave 0): fp64 base plane h x w
};

// ---------------------------------------------------------------------------
// Vertical window: acc[t] = sum_k w_k row_{t+k} (t < NO, k <= 2R) over the
// rows ld() returns in order, kPFV loads in flight.
// ---------------------------------------------------------------------------
template <int R, int NO, class Ld>
__device__ __forceinline__ void vwin(const cdouble* wp, Ld&& ld, double (&acc)[NO]) {
  constexpr int NJ = 2 * R + NO;
  constexpr int PF = NJ < kPFV ? NJ : kPFV;
  double v[NJ];
#pragma unroll
  for (int t = 0; t < NO; ++t) acc[t] = 0.0;
#pragma unroll
  for (int j = 0; j < PF; ++j) v[j] = ld();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j + PF < NJ) v[j + PF] = ld();
#pragma unroll
    for (int t = 0; t < NO; ++t) {
      const int k = j - t;
      if (k >= 0 && k <= 2 * R) acc[t] = fma((double)wp[k], v[j], acc[t]);
    }
    pin(acc);  // program order: loads and fma chains stay in their iteration
  }
}

// ---------------------------------------------------------------------------
// Vertical pass, base plane in global memory (L1/L2), this wave's rows:
// V[8 wv + t][c] = sum_k w_k B[y0 + 8 wv + t - R + k][x0 - R + c],
// c in [0, 64 + 2R).  Pass A: columns 0..63, one lane each, 8 rows.  Pass B:
// the 2R halo columns, lane -> (column 64 + l % 2R, row slice l / 2R of RB
// rows), so few lanes idle.
// ---------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void vert_glob(const GTile& T, const cdouble* wp, double* V) {
  const int yb = __builtin_amdgcn_readfirstlane(T.y0 + 8 * T.wv - R);
  const int w8 = T.w * 8;
  double* Vw = V + 8 * T.wv * T.sw;
  {
    const int xoff = clampi(T.x0 - R + T.lane, 0, T.w - 1) * 8;
    // Row offsets from a loop-carried SGPR counter (opaque to the compiler,
    // so it cannot precompute one SGPR per row of the window).
    int yy = yb;
    auto ld = [&]() -> double {
      const double v = load_f64(T.rsrc, xoff, clampi(yy, 0, T.h - 1) * w8);
      asm volatile("" : "+s"(yy));
      yy += 1;
      return v;
    };
    double acc[8];
    vwin<R, 8>(wp, ld, acc);
#pragma unroll
    for (int t = 0; t < 8; ++t) Vw[t * T.sw + T.lane] = acc[t];
  }
  if constexpr (R > 0) {
    constexpr int NB = 2 * R;
    static_assert(NB <= 64, "halo columns fit one packed pass");
    constexpr int G = 64 / NB;              // row slices side by side
    constexpr int RB = (8 + G - 1) / G;     // rows per slice
    constexpr int NSL = (8 + RB - 1) / RB;  // slices in use
    const int col = T.lane % NB, sl = T.lane / NB;
    if (sl < NSL) {
      const int lr = sl * RB;
      const int xoff = clampi(T.x0 - R + kGX + col, 0, T.w - 1) * 8;
      double acc[RB];
      if (yb >= 0 && yb + NSL * RB - 1 + 2 * R <= T.h - 1) {  // interior: no row clamping
        const int vo = xoff + lr * w8;
        int yy = yb;
        auto ld = [&]() -> double {
          const double v = load_f64(T.rsrc, vo, yy * w8);
          asm volatile("" : "+s"(yy));
          yy += 1;
          return v;
        };
        vwin<R, RB>(wp, ld, acc);
      } else {
        int yy = yb + lr;
        auto ld = [&]() -> double {
          const double v = load_f64(T.rsrc, xoff + clampi(yy, 0, T.h - 1) * w8, 0);
          yy += 1;
          return v;
        };
        vwin<R, RB>(wp, ld, acc);
      }
#pragma unroll
      for (int t = 0; t < RB; ++t)
        if (lr + t < 8) Vw[(lr + t) * T.sw + kGX + col] = acc[t];
    }
  }
}

// The same vertical pass with two adjacent strip columns per lane and one
// 16-byte load per row: the (64 + 2R) columns in ONE packed pass (no separate
// halo pass) and half the load instructions of vert_glob -- the octave-1
// launch is bound by its vertical loads' address processing (TA busy 0.84).
// Column clamping: the pair (x, x+1) is read at xa = clamp(x, 0, w - 2); at
// the left edge both columns are B[0] (the pair's first), at the right edge
// both are B[w-1] (its second).  Same fma chain per column, bit-identical.
template <int R>
__device__ __forceinline__ void vert_glob2(const GTile& T, const cdouble* wp, double* V) {
  constexpr int NC = kGX + 2 * R;  // even
  constexpr int NPAIR = NC / 2;
  static_assert(NPAIR <= 64, "one lane per column pair");
  constexpr int NJ = 2 * R + 8;
  constexpr int PF = NJ < SIFT_V2PF ? NJ : SIFT_V2PF;  // 16-byte rows in flight
  const int p = T.lane;
  if (p >= NPAIR) return;
  const int yb = __builtin_amdgcn_readfirstlane(T.y0 + 8 * T.wv - R);
  const int w8 = T.w * 8;
  const int x = T.x0 - R + 2 * p;
  const int xoff = clampi(x, 0, T.w - 2) * 8;
  double a0[8], a1[8];
  double2 v[NJ];
  auto run = [&](auto ld) {
#pragma unroll
    for (int t = 0; t < 8; ++t) a0[t] = a1[t] = 0.0;
#pragma unroll
    for (int j = 0; j < PF; ++j) v[j] = ld();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j + PF < NJ) v[j + PF] = ld();
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int k = j - t;
        if (k >= 0 && k <= 2 * R) {
          a0[t] = fma((double)wp[k], v[j].x, a0[t]);
          a1[t] = fma((double)wp[k], v[j].y, a1[t]);
        }
      }
      pin(a0);
      pin(a1);
    }
  };
  int yy = yb;
  auto raw = [&]() -> double2 {
    const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(T.rsrc, xoff, clampi(yy, 0, T.h - 1) * w8, 0);
    asm volatile("" : "+s"(yy));
    yy += 1;
    return __builtin_bit_cast(double2, q);
  };
  // Tiles whose strip columns x0 - R .. x0 + 63 + R all lie inside the
  // plane (wave-uniform) need no edge selects (4 VALU per 16-byte row).
  if (T.x0 - R >= 0 && T.x0 + kGX + R <= T.w) {
    run(raw);
  } else {
    const bool lo_edge = x < 0, hi_edge = x >= T.w - 1;
    run([&]() -> double2 {
      const double2 d = raw();
      return make_double2(hi_edge ? d.y : d.x, lo_edge ? d.x : d.y);
    });
  }
  double* Vw = V + 8 * T.wv * T.sw + 2 * p;
#pragma unroll
  for (int t = 0; t < 8; ++t) *reinterpret_cast<double2*>(Vw + t * T.sw) = make_double2(a0[t], a1[t]);
}

// vert_glob_gen with two columns per lane and 16-byte loads (radii up to 32:
// the 64 + 2r columns in one packed pass); the same 8-row chunks over
// zero-padded taps, so the same fma chains as vert_glob_gen.
__device__ __forceinline__ void vert_glob_gen2(const GTile& T, int r, const cdouble* wp, double* V) {
  const int NC = kGX + 2 * r, NJ = 2 * r + 8;
  const int p = T.lane;
  if (p >= NC / 2) return;
  const int yb = T.y0 + 8 * T.wv - r;
  const int x = T.x0 - r + 2 * p;
  const int xoff = clampi(x, 0, T.w - 2) * 8;
  const bool lo_edge = x < 0, hi_edge = x >= T.w - 1;
  // Tiles whose strip columns all lie inside the plane (wave-uniform) skip
  // the edge selects (4 VALU per 16-byte row), as in vert_glob2.
  const bool interior = T.x0 - r >= 0 && T.x0 + kGX + r <= T.w;
  double a0[8], a1[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) a0[t] = a1[t] = 0.0;
  auto sweep = [&](auto edge) {
    auto chunk = [&](int jb, auto C, auto first) {
      using CC = decltype(C);
      double2 v[8];
#pragma unroll
      for (int k = 0; k < CC::kRows; ++k) {
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(
            T.rsrc, xoff, __builtin_amdgcn_readfirstlane(clampi(yb + jb + k, 0, T.h - 1) * T.w * 8), 0);
        const double2 d = __builtin_bit_cast(double2, q);
        if constexpr (decltype(edge)::value) v[k] = make_double2(hi_edge ? d.y : d.x, lo_edge ? d.x : d.y);
        else v[k] = d;
      }
      const cdouble* w = wp + jb;
      CC::template run<decltype(first)::value>([&](int k, int t) {
        a0[t] = fma((double)w[k - t], v[k].x, a0[t]);
        a1[t] = fma((double)w[k - t], v[k].y, a1[t]);
      });
      pin(a0);
      pin(a1);
    };
    vchunk_dispatch<true>(2 * r, [&](auto C, auto f) { chunk(0, C, f); });
    for (int jb = 8; jb < NJ; jb += 8)
      vchunk_dispatch<false>(2 * r - jb, [&](auto C, auto f) { chunk(jb, C, f); });
  };
  if (interior) sweep(std::false_type{});
  else sweep(std::true_type{});
  double* Vw = V + 8 * T.wv * T.sw + 2 * p;
#pragma unroll
  for (int t = 0; t < 8; ++t) *reinterpret_cast<double2*>(Vw + t * T.sw) = make_double2(a0[t], a1[t]);
}

__device__ __forceinline__ void vert_glob_gen(const GTile& T, int r, const cdouble* wp, double* V) {
  const int NC = kGX + 2 * r, NJ = 2 * r + 8;
  const int yb = T.y0 + 8 * T.wv - r;
  for (int cb = 0; cb < NC; cb += 64) {
    const int c = cb + T.lane;
    const int xoff = clampi(T.x0 - r + min(c, NC - 1), 0, T.w - 1) * 8;
    double acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.0;
    for (int jb = 0; jb < NJ; jb += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v[k] = load_f64(T.rsrc, xoff, __builtin_amdgcn_readfirstlane(clampi(yb + jb + k, 0, T.h - 1) * T.w * 8));
#pragma unroll
      for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = fma((double)wp[jb + k - t], v[k], acc[t]);  // zero-padded taps
      pin(acc);
    }
    if (c < NC) {
      double* dst = V + 8 * T.wv * T.sw + c;
#pragma unroll
      for (int t = 0; t < 8; ++t) dst[t * T.sw] = acc[t];
    }
  }
}

// The wave's 8 strip rows, columns x0 - r .. x0 + 63 + r (clamped), from the
// split pass's plane of this scale; rows past the plane (outputs dropped)
// read its last row.
__device__ __forceinline__ void vert_copy(const GTile& T, int r, const double* __restrict__ src, double* V) {
  const int NC = kGX + 2 * r;
  double* Vw = V + 8 * T.wv * T.sw;
  const int yr = T.y0 + 8 * T.wv;
  for (int cb = 0; cb < NC; cb += 64) {
    const int c = cb + T.lane;
    const int xo = clampi(T.x0 - r + min(c, NC - 1), 0, T.w - 1);
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = src[(long long)min(yr + t, T.h - 1) * T.w + xo];
    if (c < NC)
#pragma unroll
      for (int t = 0; t < 8; ++t) Vw[t * T.sw + c] = v[t];
  }
}

// ---------------------------------------------------------------------------
// Vertical pass, octave 0, staged input region: input column kb + c (kb =
// x0/2 - ceil(r/2)), output rows e + t (e = y0 + 8 wv, even).  Tap k of
// output row e + t reads input row e/2 + floor((t + k - r)/2), i.e. window
// row m = floor((t + k - r)/2) + ceil(r/2).
// ---------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void vert_o0(const GTile& T, const cdouble* wp, double* V) {
  constexpr int HR = cl2(R);
  constexpr int NC = fl2(kGX - 1 + R) + HR + 1;
  constexpr int M = fl2(7 + R) + HR + 1;
  static_assert(NC <= 64, "one lane per input column");
  const int c = T.lane;
  if (c < NC) {
    const double* sp = T.S0 + (4 * T.wv + T.hrm - HR) * kBW0 + (c + T.hrm - HR);
    double acc[8], v[M];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.0;
#pragma unroll
    for (int m = 0; m < kPFL && m < M; ++m) v[m] = sp[m * kBW0];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (m + kPFL < M) v[m + kPFL] = sp[(m + kPFL) * kBW0];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const int k = 2 * (m - HR) + R - t + d;
          if (k >= 0 && k <= 2 * R) acc[t] = fma((double)wp[k], v[m], acc[t]);
        }
      }
      pin(acc);
    }
    double* dst = V + 8 * T.wv * T.sw + c;
#pragma unroll
    for (int t = 0; t < 8; ++t) dst[t * T.sw] = acc[t];
  }
}

// ---------------------------------------------------------------------------
// Horizontal pass: lane -> columns 4 cg .. 4 cg + 3, rows 8 wv + rs + 4 i.
// o >= 1: out[q] = sum_k w_k V[row][4 cg + q + k].
// ---------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void horz_full(const GTile& T, const cdouble* wp, const double* V,
                                          double (&out)[kNR][4]) {
  // Both rows of the lane in one loop: 8 independent fma chains per wave
  // (4 leave the fp64 pipeline latency exposed).
  constexpr int NP = R + 2;  // double2 pairs per row
  const double* rp[kNR];
  double2 u[kNR][NP];
#pragma unroll
  for (int i = 0; i < kNR; ++i) {
    rp[i] = V + (8 * T.wv + T.rs + kRS * i) * T.sw + 4 * T.cg;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[i][q] = 0.0;
  }
#pragma unroll
  for (int n2 = 0; n2 < kPFH && n2 < NP; ++n2)
#pragma unroll
    for (int i = 0; i < kNR; ++i) u[i][n2] = *reinterpret_cast<const double2*>(rp[i] + 2 * n2);
#pragma unroll
  for (int n2 = 0; n2 < NP; ++n2) {
    if (n2 + kPFH < NP)
#pragma unroll
      for (int i = 0; i < kNR; ++i) u[i][n2 + kPFH] = *reinterpret_cast<const double2*>(rp[i] + 2 * (n2 + kPFH));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int n = 2 * n2 + e;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = n - q;
        if (k >= 0 && k <= 2 * R)
#pragma unroll
          for (int i = 0; i < kNR; ++i) out[i][q] = fma((double)wp[k], e ? u[i][n2].y : u[i][n2].x, out[i][q]);
      }
    }
#pragma unroll
    for (int i = 0; i < kNR; ++i) pin(out[i]);
  }
}

__device__ __forceinline__ void horz_full_gen(const GTile& T, int r, const cdouble* wp, const double* V,
                                              double (&out)[kNR][4]) {
  const int NV = 2 * r + 4;
  const double* rp[kNR];
#pragma unroll
  for (int i = 0; i < kNR; ++i) {
    rp[i] = V + (8 * T.wv + T.rs + kRS * i) * T.sw + 4 * T.cg;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[i][q] = 0.0;
  }
  for (int nb = 0; nb < NV; nb += 8) {
    double u[kNR][8];
#pragma unroll
    for (int i = 0; i < kNR; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double2 p = *reinterpret_cast<const double2*>(rp[i] + nb + 2 * e);
        u[i][2 * e] = p.x;
        u[i][2 * e + 1] = p.y;
      }
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < kNR; ++i) out[i][q] = fma((double)wp[nb + e - q], u[i][e], out[i][q]);  // zero-padded taps
#pragma unroll
    for (int i = 0; i < kNR; ++i) pin(out[i]);
  }
}

// Octave 0: strip column n <-> input column x0/2 - ceil(r/2) + n; tap k of
// output column x0 + 4 cg + q reads strip column 2 cg + floor((q + k - r)/2) + ceil(r/2).
template <int R>
__device__ __forceinline__ void horz_o0(const GTile& T, const cdouble* wp, const double* V,
                                        double (&out)[kNR][4]) {
  constexpr int HR = cl2(R);
  constexpr int NP = (fl2(R + 3) + HR + 2) / 2;  // double2 pairs per row
  const double* rp[kNR];
  double2 u[kNR][NP];
#pragma unroll
  for (int i = 0; i < kNR; ++i) {
    rp[i] = V + (8 * T.wv + T.rs + kRS * i) * T.sw + 2 * T.cg;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[i][q] = 0.0;
  }
#pragma unroll
  for (int n2 = 0; n2 < kPFH && n2 < NP; ++n2)
#pragma unroll
    for (int i = 0; i < kNR; ++i) u[i][n2] = *reinterpret_cast<const double2*>(rp[i] + 2 * n2);
#pragma unroll
  for (int n2 = 0; n2 < NP; ++n2) {
    if (n2 + kPFH < NP)
#pragma unroll
      for (int i = 0; i < kNR; ++i) u[i][n2 + kPFH] = *reinterpret_cast<const double2*>(rp[i] + 2 * (n2 + kPFH));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int n = 2 * n2 + e;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const int k = 2 * (n - HR) + R - q + d;
          if (k >= 0 && k <= 2 * R)
#pragma unroll
            for (int i = 0; i < kNR; ++i) out[i][q] = fma((double)wp[k], e ? u[i][n2].y : u[i][n2].x, out[i][q]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kNR; ++i) pin(out[i]);
  }
}

// The pass of one scale by its radius r; radii 0..RMAX have unrolled code
// (octave 0: all of its radii).  Every pass finds its radius by binary search
// (rdispatch) but octave 0's horizontal pass, which keeps the compare chain:
// binary in both takes octave 0 from 92 to 105 VGPRs, 5 -> 4 waves per SIMD
// (0.364 -> 0.383 ms; bounded to 96 it spills: 0.370 ms;
// profiles/r6g_radius_dispatch_ab.txt).
template <bool OCT0, int RMAX>
__device__ __forceinline__ void vert_any(const GTile& T, int r, const cdouble* wp, double* V) {
  if constexpr (OCT0) {
    rdispatch<0, RMAX>(r, [&](auto R) { vert_o0<decltype(R)::value>(T, wp, V); });
  } else if (r <= RMAX) {
    if (T.w >= 2) rdispatch<0, RMAX>(r, [&](auto R) { vert_glob2<decltype(R)::value>(T, wp, V); });
    else rdispatch<0, RMAX>(r, [&](auto R) { vert_glob<decltype(R)::value>(T, wp, V); });
  } else if (T.w >= 2 && r <= 32) {
    vert_glob_gen2(T, r, wp, V);
  } else {
    vert_glob_gen(T, r, wp, V);
  }
}

template <int... Rs>
__device__ __forceinline__ void horz_o0_chain(std::integer_sequence<int, Rs...>, const GTile& T, int r,
                                              const cdouble* wp, const double* V, double (&out)[kNR][4]) {
  bool done = false;
  ((!done && r == Rs ? (horz_o0<Rs>(T, wp, V, out), done = true) : false), ...);
}
template <bool OCT0, int RMAX>
__device__ __forceinline__ void horz_any(const GTile& T, int r, const cdouble* wp, const double* V,
                                         double (&out)[kNR][4]) {
  if constexpr (OCT0) horz_o0_chain(std::make_integer_sequence<int, RMAX + 1>{}, T, r, wp, V, out);
  else if (r <= RMAX) rdispatch<0, RMAX>(r, [&](auto R) { horz_full<decltype(R)::value>(T, wp, V, out); });
  else horz_full_gen(T, r, wp, V, out);
}

// ---------------------------------------------------------------------------
// Extrema decisions fused into the pass (XF).  Tiles overlap: a block
// computes 64 x 32 pixels at a stride of kFX x kFY, stores the kFX x kFY it
// owns (the last tile of a row / column all of its in-plane pixels) and
// decides the kFX x kFY pixels one column and one row in from its origin,
// whose 26 neighbours all lie in its tile (translation invariance makes the
// overlapping pixels bit-identical to their owners').  Each scale's DoG tile
// goes to an LDS ring of 3 fp32 planes; once DoG t+1 is there, every wave
// decides scale t for its own rows with the scan's logic (x_row_decide:
// fp32 comparisons, ties and threshold-adjacent values to the exact pass).
// Replaces the scan of this octave: its DoG planes are not read back.
// ---------------------------------------------------------------------------
// Scale t (DoG t-1, t, t+1 in ring slots (t-1)%3, t%3, (t+1)%3) for the
// wave's rows 8 wv .. 8 wv + 7; one lane per tile column.
__device__ __forceinline__ void fused_decide(const Pyramid& P, const GaussLaunch& L, const GTile& T,
                                             const float* ring, int t, unsigned& low) {
  const Octave& oc = P.oct[L.o];
  const int l = T.lane;
  const float* q0 = ring + ((t - 1) % 3) * kRingPlane + l;
  const float* q1 = ring + (t % 3) * kRingPlane + l;
  const float* q2 = ring + ((t + 1) % 3) * kRingPlane + l;
  const int x = T.x0 + l;
  const unsigned long long colmask = __ballot(l >= 1 && l <= kFX && x >= 1 && x <= T.w - 2);
  const unsigned key0 = oc.key_off + (unsigned)(t - 1) * (unsigned)T.h * (unsigned)T.w + (unsigned)x;
  const int r0 = 8 * T.wv;
  XWin<3> Wn;
  auto load = [&](float (&dst)[3], int j) {  // tile row r0 - 1 + j (clamped: only undecided rows read past)
    const int r = clampi(r0 - 1 + j, 0, kGY - 1) * kGX;
    dst[0] = q0[r];
    dst[1] = q1[r];
    dst[2] = q2[r];
  };
  {
    float a[3], b[3];
    load(a, 0);
    load(b, 1);
    x_derive<3, 0>(Wn, a);
    x_derive<3, 1>(Wn, b);
  }
  auto centre = [&](auto A_, auto B_, auto C_, int j) {
    constexpr int A = decltype(A_)::value, B = decltype(B_)::value, C = decltype(C_)::value;
    const int c = r0 + j - 1;  // tile row of the centre
    const int y = T.y0 + c;
    if (c < 1 || c > kFY || y < 1 || y > T.h - 2) return;  // wave-uniform
    const float vx0 = max3f(Wn.hx[A][0], Wn.hx[B][0], Wn.hx[C][0]), vn0 = min3f(Wn.hn[A][0], Wn.hn[B][0], Wn.hn[C][0]);
    const float vx2 = max3f(Wn.hx[A][2], Wn.hx[B][2], Wn.hx[C][2]), vn2 = min3f(Wn.hn[A][2], Wn.hn[B][2], Wn.hn[C][2]);
    const float v = Wn.cv[B][1];
    const float nmax = max3f(vx0, vx2, max3f(Wn.hx[A][1], Wn.hx[C][1], Wn.ex[B][1]));
    const float nmin = min3f(vn0, vn2, min3f(Wn.hn[A][1], Wn.hn[C][1], Wn.en[B][1]));
    unsigned long long ambmask;  // (the fused path lists ambiguous keys itself)
    unsigned long long lowmask;  // the low-contrast list is not fused (build_common)
    const unsigned long long bit =
        x_row_decide(v, nmax, nmin, colmask, L.X.c_lo, L.X.c_hi, false, key0 + (unsigned)y * (unsigned)T.w,
                     &L.X.counters[kCntAmb], L.X.amb_keys, L.X.amb_cap, low, lowmask, ambmask);
    const unsigned long long word = bit >> 1;  // lanes 1..kFX -> bits 0..kFX-1
    if (l == 0) {
      const long long row = (long long)(t - 1) * T.h + y;
      L.X.bitmap[row * L.X.nw + T.bx] = word;
      if (word) atomicAdd(&L.X.rowcount[row], (unsigned)__popcll(word));
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  // rows j = 2..9 are derived into slot j % 3, centre row j - 1 uses slots (j-2, j-1, j) % 3
  {
    float a[3];
    load(a, 2); x_derive<3, 2>(Wn, a); centre(I0{}, I1{}, I2{}, 1);
    load(a, 3); x_derive<3, 0>(Wn, a); centre(I1{}, I2{}, I0{}, 2);
    load(a, 4); x_derive<3, 1>(Wn, a); centre(I2{}, I0{}, I1{}, 3);
    load(a, 5); x_derive<3, 2>(Wn, a); centre(I0{}, I1{}, I2{}, 4);
    load(a, 6); x_derive<3, 0>(Wn, a); centre(I1{}, I2{}, I0{}, 5);
    load(a, 7); x_derive<3, 1>(Wn, a); centre(I2{}, I0{}, I1{}, 6);
    load(a, 8); x_derive<3, 2>(Wn, a); centre(I0{}, I1{}, I2{}, 7);
    load(a, 9); x_derive<3, 0>(Wn, a); centre(I1{}, I2{}, I0{}, 8);
  }
}

// SWC > 0: compile-time strip stride (immediate LDS offsets); 0: L.sw.
// RMAX: radii with unrolled code.  XF: extrema decisions fused (above).
// VS: the split-pass instance (octaves with a k_gauss_vert launch): its strips
// come from the split pass's vertical sums only, so the vertical radius
// variants are not compiled into it (round 6: the shared instance spilled
// 126 SGPRs into VGPR lanes, readlane / writelane in every scale).
template <bool OCT0, int SWC, int RMAX, bool XF, bool VS = false>
__global__ __launch_bounds__(256, OCT0 ? SIFT_W0 : SIFT_MINW1) void k_gauss_dog(const Pyramid P, const GaussLaunch L) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Octave& oc = P.oct[L.o];
  // 1D grid: block -> (scale group, tile).  Blocks are dispatched round-robin
  // over the 8 XCDs; with xcd_band, XCD k runs the k-th contiguous range of
  // tiles (a band of tile rows), so the base rows its vertical passes re-read
  // stay in its own L2.  Groups of one tile are adjacent (same base region).
  // Batch (L.nimg images of one geometry): blocks of image im follow those
  // of image im - 1; its planes, base and seeds are im * (stride) further.
  int lb = blockIdx.x;
  const int bpi = L.gx * L.gy * L.G;  // blocks per image
  if (L.xcd_band) {
    const int nb = bpi * L.nimg, q = nb >> 3, rm = nb & 7, xc = lb & 7;
    lb = xc * q + min(xc, rm) + (lb >> 3);
  }
  const int im = lb / bpi;
  lb -= im * bpi;
  float* const L_gauss = L.gauss ? L.gauss + im * L.gauss_bs : nullptr;
  float* const L_dog = L.dog + im * L.dog_bs;
  double* const L_next_seed = L.next_seed ? L.next_seed + im * L.seed_bs : nullptr;
  const double* const L_base = L.base ? L.base + im * L.base_bs : nullptr;
  double* const L_l64 = L.l64 ? L.l64 + im * L.l64_bs : nullptr;
  const double* const L_vsplit = L.vsplit ? L.vsplit + im * L.vsplit_bs : nullptr;
  const float* const img_b = OCT0 ? P.img + im * P.img_bstride : nullptr;
  const int bz = lb % L.G, bt = lb / L.G;
  const int bx = bt % L.gx, by = bt / L.gx;
  GTile T;
  T.bx = bx;
  T.h = oc.h;
  T.w = oc.w;
  T.x0 = bx * (XF ? kFX : kGX);
  T.y0 = by * (XF ? kFY : kGY);
  T.lane = threadIdx.x & 63;
  T.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T.cg = T.lane & (kCG - 1);
  T.rs = T.lane / kCG;
  T.sw = SWC > 0 ? SWC : L.sw;
  T.hrm = cl2(oc.rmax);
  if (!OCT0)
    T.rsrc = urs(const_cast<double*>(L_base), T.h * T.w * 8);
  // One strip: every wave writes (vertical pass) and reads (horizontal pass)
  // only its own 8 strip rows.
  const int nstrip = kGY * T.sw;
  T.S0 = smem + nstrip;
  double* V = smem;
  // fused extrema: fp32 DoG ring after the strip and the staged region
  float* ring = nullptr;
  if constexpr (XF)
    ring = reinterpret_cast<float*>(smem + nstrip + (OCT0 ? (fl2(kGY - 1 + oc.rmax) + T.hrm + 1) * kBW0 : 0));
  unsigned xlow = 0;

  // The generic horizontal path reads (with zero taps) past the columns a
  // scale writes: those must be finite.
  if (L.zero)
    for (int i = threadIdx.x; i < nstrip; i += 256) smem[i] = 0.0;
  if (OCT0) {
    // Stage input rows y0/2 - hrm .. and columns x0/2 - hrm .. as fp64,
    // clamped (replicate edges): the region every scale's windows read.
    const int q0 = T.y0 / 2 - T.hrm, k0 = T.x0 / 2 - T.hrm;
    const int nr = fl2(kGY - 1 + oc.rmax) + T.hrm + 1;
    const int nc = fl2(kGX - 1 + oc.rmax) + T.hrm + 1;
    double* S0 = smem + nstrip;
    const int kk = clampi(k0 + T.lane, 0, P.W - 1);
    for (int rr = T.wv; rr < nr; rr += 4) {
      const float* src = img_b + (long long)clampi(q0 + rr, 0, P.H - 1) * P.img_stride;
      if (T.lane < nc) S0[rr * kBW0 + T.lane] = (double)src[kk];
    }
  }
  const long long plane = (long long)T.h * T.w;
  // Pixels this block stores: all of its tile, or with fused extrema the
  // kFX x kFY it owns (the last tile of a row / column: all it computes).
  bool own[kNR];
  // Per-lane byte offsets of its output items in a plane (past the plane or
  // not owned: the store is dropped).
  int voff[kNR];
#pragma unroll
  for (int i = 0; i < kNR; ++i) {
    const int r = 8 * T.wv + T.rs + kRS * i;
    const int y = T.y0 + r;
    const int x = T.x0 + 4 * T.cg;
    const bool own_c = !XF || 4 * T.cg < kFX || bx == L.gx - 1;
    own[i] = y < T.h && T.w - x > 0 && own_c && (!XF || r < kFY || by == L.gy - 1);
    voff[i] = own[i] ? (y * T.w + x) * 4 : 0x7ffffff0;
  }

  // Scale group of this block (small octaves split their scales over
  // blockIdx.z for parallelism; a group recomputes the scale before it as
  // the DoG's L_{s-1}, without storing it).
  const int s_begin = L.gb[bz], s_end = L.gb[bz + 1];
  const int s_first = max(0, s_begin - 1);
  __syncthreads();  // staged region / zeroed strip visible to every wave

  double lprev[kNR][4];
  for (int s = s_first; s < s_end; ++s) {
    const cdouble* wp = (const cdouble*)(P.wts + oc.wofs[s]);
    // Per-lane indices made opaque each scale: otherwise the compiler hoists
    // every radius variant's address arithmetic out of the scale loop and
    // keeps it all live (dozens of VGPRs, half the occupancy).
    GTile Ts = T;
    asm volatile("" : "+v"(Ts.lane), "+v"(Ts.cg), "+v"(Ts.rs));
    double out[kNR][4];
    if constexpr (VS) {
      vert_copy(Ts, oc.rad[s], L_vsplit + (long long)s * plane, V);
    } else if constexpr (!OCT0) {
      if (L_vsplit) vert_copy(Ts, oc.rad[s], L_vsplit + (long long)s * plane, V);
      else vert_any<OCT0, RMAX>(Ts, oc.rad[s], wp, V);
    } else {
      vert_any<OCT0, RMAX>(Ts, oc.rad[s], wp, V);
    }
    wave_lds_fence();  // this wave's strip rows written -> read by its other lanes
    horz_any<OCT0, RMAX>(Ts, oc.rad[s], wp, V, out);
    wave_lds_fence();  // strip rows read before the next scale overwrites them

    double d[kNR][4];
#pragma unroll
    for (int i = 0; i < kNR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) d[i][q] = lprev[i][q] - out[i][q];
    if (s >= s_begin) {
      if (L.vec) {
        const unsigned pb = (unsigned)plane * 4u;
        if (L_gauss) {
          const __amdgpu_buffer_rsrc_t rg = urs(L_gauss + s * plane, pb);
#pragma unroll
          for (int i = 0; i < kNR; ++i) bstore4(rg, voff[i], out[i]);
        }
        if (s > 0) {
          const __amdgpu_buffer_rsrc_t rd = urs(L_dog + (s - 1) * plane, pb);
#pragma unroll
          for (int i = 0; i < kNR; ++i) bstore4(rd, voff[i], d[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < kNR; ++i) {
          const int y = T.y0 + 8 * T.wv + T.rs + kRS * i;
          const int x = T.x0 + 4 * T.cg, nvalid = T.w - x;
          if (own[i]) {
            const long long pp = (long long)y * T.w + x;
            if (L_gauss) store4(L_gauss + s * plane + pp, out[i], nvalid);
            if (s > 0) store4(L_dog + (s - 1) * plane + pp, d[i], nvalid);
          }
        }
      }
    }
    if constexpr (XF) {
      // DoG s-1 into ring slot (s-1) % 3, then decide scale s-2 once DoG
      // s-3, s-2, s-1 are all there (scales 1..S; s runs to S+2).
      if (s >= 1) {
        if (s >= 4) lds_barrier();  // the decision of scale s-3 has read slot (s-1) % 3
#pragma unroll
        for (int i = 0; i < kNR; ++i) {
          const float4 f = make_float4((float)d[i][0], (float)d[i][1], (float)d[i][2], (float)d[i][3]);
          *reinterpret_cast<float4*>(ring + ((s - 1) % 3) * kRingPlane + (8 * T.wv + T.rs + kRS * i) * kGX +
                                     4 * T.cg) = f;
        }
        if (s >= 3) {
          lds_barrier();  // every wave's rows of DoG s-1 are in the ring
          fused_decide(P, L, Ts, ring, s - 2, xlow);
        }
      }
    }
    if (L_l64 && s >= s_begin) {  // fp64 plane for the exact passes
      double* lp = L_l64 + s * plane;
#pragma unroll
      for (int i = 0; i < kNR; ++i) {
        const int y = T.y0 + 8 * T.wv + T.rs + kRS * i;
        const int x = T.x0 + 4 * T.cg, nvalid = T.w - x;
        if (own[i]) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < nvalid) lp[(long long)y * T.w + x + q] = out[i][q];
        }
      }
    }
    if (s == P.S && L_next_seed && s >= s_begin) {
#pragma unroll
      for (int i = 0; i < kNR; ++i) {
        const int y = T.y0 + 8 * T.wv + T.rs + kRS * i;
        const int x = T.x0 + 4 * T.cg, nvalid = T.w - x;
        if (own[i] && !(y & 1)) {
          double* sd = L_next_seed + (long long)(y >> 1) * L.next_w + (x >> 1);
          sd[0] = out[i][0];
          if (nvalid > 2) sd[1] = out[i][2];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kNR; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) lprev[i][q] = out[i][q];
  }
  if constexpr (XF) {
    if (T.lane == 0 && xlow) atomicAdd(&L.X.counters[kCntLow], xlow);
  }
}

}  // namespace sift
