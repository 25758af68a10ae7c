// Register-window tiles for octaves >= 1 (k_gauss_rw).  k_gauss_dog re-reads
// its fp64 base window from L1/L2 once per SCALE (S+3 times) and every wave
// re-reads the 2r rows it shares with the waves above and below: at 4K the
// active blocks of an XCD need ~4 MiB of base lines, its L2 holds 40-60 % of
// those re-reads and the rest stream from the Infinity Cache at ~7 TB/s,
// which bounds the vertical pass (the same loop from an L2-resident plane or
// from LDS issues fp64 fmas 3-4x faster: profiles/r4_fma_probe.txt).  Here
// every lane of a 256-lane block owns ONE strip column and keeps that
// column's window of 8 + 2 RW base rows in registers for ALL scales of the
// octave (RW >= the octave's largest radius): each base value is loaded once
// per block, and the vertical pass of every scale is register fmas only,
//   V[t][c] = sum_k w_k win_c[t + k + RW - r],  t < 8,
// taps in increasing order from 0.0 (k_gauss_dog's chain).  Strip column c
// <-> image column x0 - RW + c, so the 256 columns hold the vertical sums of
// an output tile of TW = 224 (RW <= 16) or 192 (RW <= 24) columns and its
// halo for every radius <= RW: no separate halo pass.  The strip (8 rows,
// double-buffered in LDS) is shared by the block's 4 waves: one barrier per
// scale.  Horizontal pass: items of 8 columns x 1 row (8 fma chains per
// lane); the items of a ds_read_b128 lane group are 4 column groups x 4 rows
// (strip stride 2 mod 4 doubles: conflict-free).  Same fma chain per output
// as k_gauss_dog: bit-identical planes.
#include "sift_gauss_dev.h"

namespace sift {

// Vertical pass of one strip column: acc[t] = sum_k w_k win[t + k + RW - R].
// Tap loads: the tap pointer is made opaque every 8 taps, so the compiler
// loads each group of taps where it is used instead of keeping 2r + 1 taps
// in SGPRs.
template <int R, int RW>
__device__ __forceinline__ void rw_vert(const double (&win)[RwGeom<RW>::NW], const cdouble* wp, double (&acc)[8]) {
  constexpr int D = RW - R;
  const cdouble* wq = wp;
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = 0.0;
#pragma unroll
  for (int k = 0; k <= 2 * R; ++k) {
    if (SIFT_RWTAPS > 0 && k % (SIFT_RWTAPS > 0 ? SIFT_RWTAPS : 1) == 0) asm volatile("" : "+s"(wq));
    const double wk = wq[k];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = fma(wk, win[t + k + D], acc[t]);
  }
}

// Horizontal pass of one item (4 columns x rows A, B): out[i][q] = sum_k w_k
// V[row_i][b + q + k], b = 4 cg + RW - R (strip column of the first tap of
// output column x0 + 4 cg); 16-byte reads from the even column at or before b.
template <int R, int RW>
__device__ __forceinline__ void rw_horz(const double* ra, const double* rb, const cdouble* wp, double (&out)[2][4]) {
  constexpr int D = (RW - R) & 1;           // b odd: element n is pair (n + 1) / 2, half (n + 1) & 1
  constexpr int NE = 4 + 2 * R;             // elements n = 0 .. 3 + 2R
  constexpr int NP = (NE - 1 + D) / 2 + 1;  // pairs per row
  constexpr int PF = NP < SIFT_RWPF ? NP : SIFT_RWPF;
  const double* pa = ra + ((RW - R) - D);   // even column
  const double* pb = rb + ((RW - R) - D);
  double2 u[2][NP];
  const cdouble* wq = wp;
#pragma unroll
  for (int q = 0; q < 4; ++q) out[0][q] = out[1][q] = 0.0;
  // An odd-D item does not use its first pair's .x: that value is marked used
  // (empty asm), so every read stays one aligned ds_read_b128 (the compiler
  // would otherwise drop it and re-pair the reads as 8-byte-aligned
  // ds_read2_b64s, which conflict).
  auto rd = [](const double* q) { return *reinterpret_cast<const double2*>(q); };
#pragma unroll
  for (int n2 = 0; n2 < PF; ++n2) {
    u[0][n2] = rd(pa + 2 * n2);
    u[1][n2] = rd(pb + 2 * n2);
  }
  if constexpr (D) asm volatile("" ::"v"(u[0][0].x), "v"(u[1][0].x));
#pragma unroll
  for (int n2 = 0; n2 < NP; ++n2) {
    if (n2 + PF < NP) {
      u[0][n2 + PF] = rd(pa + 2 * (n2 + PF));
      u[1][n2 + PF] = rd(pb + 2 * (n2 + PF));
    }
    if (SIFT_RWTAPS > 0 && n2 % (SIFT_RWTAPS > 0 ? SIFT_RWTAPS / 2 : 1) == 0) asm volatile("" : "+s"(wq));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int n = 2 * n2 + e - D;  // element index
      if (n < 0 || n >= NE) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = n - q;
        if (k >= 0 && k <= 2 * R) {
          const double wk = wq[k];
          out[0][q] = fma(wk, e ? u[0][n2].y : u[0][n2].x, out[0][q]);
          out[1][q] = fma(wk, e ? u[1][n2].y : u[1][n2].x, out[1][q]);
        }
      }
    }
    pin(out[0]);
    pin(out[1]);
  }
}

template <int RW, int... Rs>
__device__ __forceinline__ void rw_vert_any_(std::integer_sequence<int, Rs...>, int r,
                                            const double (&win)[RwGeom<RW>::NW], const cdouble* wp,
                                            double (&acc)[8]) {
  rdispatch<0, sizeof...(Rs) - 1>(r, [&](auto R) { rw_vert<decltype(R)::value, RW>(win, wp, acc); });
}
template <int RW, int... Rs>
__device__ __forceinline__ void rw_horz_any_(std::integer_sequence<int, Rs...>, int r, const double* ra,
                                            const double* rb, const cdouble* wp, double (&out)[2][4]) {
  rdispatch<0, sizeof...(Rs) - 1>(r, [&](auto R) { rw_horz<decltype(R)::value, RW>(ra, rb, wp, out); });
}
// Streamed vertical pass of one strip column (k_gauss_rw<RW, true>): the
// scale's own window rows y0 - r .. y0 + 7 + r loaded per scale from the base
// plane (L2-resident for the mid-radius octaves: XCD-banded tiles), in
// vert_glob_gen's 8-row chunks over zero-padded taps -- the same fma chain per
// output as the register window, bit for bit.
__device__ __forceinline__ void rw_vert_stream(__amdgpu_buffer_rsrc_t rs, int xoff, int y0, int h, int w, int r,
                                               const cdouble* wp, double (&acc)[8]) {
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = 0.0;
  const int yb = y0 - r, NJ = 2 * r + 8;
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
  vchunk_dispatch<true>(2 * r, [&](auto C, auto f) { chunk(0, C, f); });
  for (int jb = 8; jb < NJ; jb += 8) vchunk_dispatch<false>(2 * r - jb, [&](auto C, auto f) { chunk(jb, C, f); });
}

template <int RW, bool STREAM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SIFT_RW_WPE))) void k_gauss_rw(const Pyramid P, const GaussLaunch L) {
  using G = RwGeom<RW>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Octave& oc = P.oct[L.o];
  // 1D grid: block -> (scale group, tile) as in k_gauss_dog (XCD bands, batches image-major).
  int lb = blockIdx.x;
  const int bpi = L.gx * L.gy * L.G;
  if (L.xcd_band) {
    const int nb = bpi * L.nimg, q = nb >> 3, rm = nb & 7, xc = lb & 7;
    lb = xc * q + min(xc, rm) + (lb >> 3);
  }
  const int im = lb / bpi;
  lb -= im * bpi;
  float* const L_gauss = L.gauss ? L.gauss + im * L.gauss_bs : nullptr;
  float* const L_dog = L.dog + im * L.dog_bs;
  double* const L_next_seed = L.next_seed ? L.next_seed + im * L.seed_bs : nullptr;
  const double* const L_base = L.base + im * L.base_bs;
  const int bz = lb % L.G, bt = lb / L.G;
  const int bx = bt % L.gx, by = bt / L.gx;
  const int h = oc.h, w = oc.w;
  const int x0 = bx * G::TW, y0 = by * kRwRows;
  const int c = threadIdx.x;  // strip column
  // The lane's base window: rows y0 - RW .. y0 + 7 + RW of image column x0 - RW + c (clamped).
  const __amdgpu_buffer_rsrc_t brs =
      urs(const_cast<double*>(L_base), h * w * 8);
  const int bxoff = clampi(x0 - RW + c, 0, w - 1) * 8;
  double win[STREAM ? 1 : G::NW];
  if constexpr (!STREAM) {
#pragma unroll
    for (int j = 0; j < G::NW; ++j)
      win[j] = load_f64(brs, bxoff, __builtin_amdgcn_readfirstlane(clampi(y0 - RW + j, 0, h - 1) * w * 8));
  }
  // Horizontal items of 4 columns x 2 rows: ds_read_b128 lane group gid =
  // 4 wv + g (b128_group) at position j: column group cg = 8 (gid >> 1) +
  // (j & 7), rows a = gid & 1 or 2 + (gid & 1) and a + 4, the half-groups in
  // opposite order (j < 8: a = gid & 1 first; j >= 8: a + 4 first), so every
  // read instruction covers two rows 6 or 2 apart (odd quad offsets through
  // rw_row: conflict-free) and every store instruction 128 contiguous bytes
  // of a row per half-group.
  int hcg, hr0, hr1;
  {
    int g, j;
    b128_group(c & 63, g, j);
    const int gid = 4 * (c >> 6) + g;
    hcg = 8 * (gid >> 1) + (j & 7);
    hr0 = j < 8 ? (gid & 1) : 6 + (gid & 1);
    hr1 = j < 8 ? 4 + (gid & 1) : 2 + (gid & 1);
  }
  const bool hact = hcg < G::NCG;  // lanes with an item
  const long long plane = (long long)h * w;
  const int s_begin = L.gb[bz], s_end = L.gb[bz + 1];
  const int s_first = max(0, s_begin - 1);
  double lprev[2][4];
  for (int s = s_first; s < s_end; ++s) {
    const cdouble* wp = (const cdouble*)(P.wts + oc.wofs[s]);
    const int r = oc.rad[s];
    double* Vs = smem + (s & 1) * kRwStrip;
    {
      double acc[8];
      if constexpr (STREAM) {
        int xo = bxoff;
        asm volatile("" : "+v"(xo));  // per-scale opaque: no hoisted per-radius addresses
        rw_vert_stream(brs, xo, y0, h, w, r, wp, acc);
      } else {
        rw_vert_any_<RW>(std::make_integer_sequence<int, RW + 1>{}, r, win, wp, acc);
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) Vs[rw_row(t) + c] = acc[t];
    }
    // Strip s complete; every wave is past its horizontal pass of scale s - 1
    // (the other buffer), so the next scale may overwrite that one.
    lds_barrier();
    if (hact) {
      int hc = hcg, h0 = hr0, h1 = hr1;
      asm volatile("" : "+v"(hc), "+v"(h0), "+v"(h1));  // per-scale opaque: no hoisted per-radius addresses
      double o[2][4];
      rw_horz_any_<RW>(std::make_integer_sequence<int, RW + 1>{}, r, Vs + rw_row(h0) + 4 * hc,
                       Vs + rw_row(h1) + 4 * hc, wp, o);
      const int x = x0 + 4 * hc, nvalid = w - x;
      const unsigned pb = (unsigned)plane * 4u;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int y = y0 + (i ? h1 : h0);
        const bool own = y < h && nvalid > 0;
        double d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = lprev[i][q] - o[i][q];
        if (s >= s_begin) {
          if (L.vec) {
            const int voff = own ? (y * w + x) * 4 : 0x7ffffff0;  // dropped past the plane
            if (L_gauss)
              bstore4(urs(L_gauss + s * plane, pb), voff, o[i]);
            if (s > 0)
              bstore4(urs(L_dog + (s - 1) * plane, pb), voff, d);
          } else if (own) {
            const long long pp = (long long)y * w + x;
            if (L_gauss) store4(L_gauss + s * plane + pp, o[i], nvalid);
            if (s > 0) store4(L_dog + (s - 1) * plane + pp, d, nvalid);
          }
        }
        if (s == P.S && L_next_seed && s >= s_begin && own && !(y & 1)) {
          double* sd = L_next_seed + (long long)(y >> 1) * L.next_w + (x >> 1);
          sd[0] = o[i][0];
          if (nvalid > 2) sd[1] = o[i][2];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) lprev[i][q] = o[i][q];
      }
    }
  }
}

GaussKernelFn gauss_rw_kernel(int k) {  // kKWindow12 .. kKStreamed24
  static const GaussKernelFn f[] = {k_gauss_rw<12>,       k_gauss_rw<16>,       k_gauss_rw<24>,
                                    k_gauss_rw<12, true>, k_gauss_rw<16, true>, k_gauss_rw<24, true>};
  return f[k - kKWindow12];
}

}  // namespace sift
