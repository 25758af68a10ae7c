// Internal header of the Gaussian + DoG pass; only the sift_gauss_*.hip
// translation units include it (the public launch interface of the stage is
// in sift_kernels.h).  Layout of the stage:
//
//   sift_gauss_dev.h     this file: the compile-time knobs, the tile and strip
//                        geometry (host and device), the device helpers that
//                        both kernel families use, and the declarations by
//                        which the launcher reaches each family's kernels
//   sift_gauss_tile.h    the 64-column tile kernel k_gauss_dog and its passes
//                        (templates); the algorithm is described there
//   sift_gauss_tile0.hip its four staged octave-0 instantiations
//   sift_gauss_tile1.hip its two instantiations for octaves >= 1, and the
//                        split vertical pass k_gauss_vert (two units: all six
//                        in one took longer to compile than any other file)
//   sift_gauss_rw.hip    the register-window and streamed kernels: k_gauss_rw
//                        (six instantiations)
//   sift_gauss_plan.hip  the host side: gauss_plan, launch_gauss_dog and the
//                        small kernels with their launchers; no heavy
//                        instantiation, so a change of the plan compiles fast
#pragma once
#include <utility>

#include "sift_common.h"
#include "sift_kernels.h"

// Compile-time knobs of the stage.  The defaults are the measured winners;
// tools/build_variant.sh overrides one with EXTRA=-D... for an A/B build.
#ifndef SIFT_UR1
#define SIFT_UR1 12  // radii with unrolled code in octaves >= 1 (SGPR budget; 24: 0.093 -> 0.124 ms, r5d_unrolled_octave2_ab)
#endif
#ifndef SIFT_VS_RMAX
#define SIFT_VS_RMAX 12  // ... in the horizontal pass of the split-pass instance
#endif
#ifndef SIFT_STORE_AUX
#define SIFT_STORE_AUX 18  // cache-policy bits of the plane stores (gfx950: 1 sc0, 2 nt, 16 sc1; r2g_store_policy_ab)
#endif
#ifndef SIFT_W0
#define SIFT_W0 1  // octave-0 k_gauss_dog: minimum blocks (= waves) per SIMD the register allocation must allow
#endif
#ifndef SIFT_MINW1
#define SIFT_MINW1 1  // ... k_gauss_dog of octaves >= 1
#endif
#ifndef SIFT_V2PF
#define SIFT_V2PF 4  // 16-byte rows in flight in vert_glob2 (4 and 6 measured equal; 4: 108 VGPRs)
#endif
#ifndef SIFT_RWPF
#define SIFT_RWPF 3  // k_gauss_rw: 16-byte strip reads in flight per row, horizontal pass
#endif
#ifndef SIFT_RWTAPS
#define SIFT_RWTAPS 8  // ... taps per reload of the tap pointer (0: never: the compiler keeps them in SGPRs; 0 / 16 no gain)
#endif
#ifndef SIFT_RW_WPE
#define SIFT_RW_WPE 1  // ... minimum waves per SIMD the register allocation must allow (r5f_octave1_knobs_ab)
#endif
#ifndef SIFT_RWS_DEFAULT
#define SIFT_RWS_DEFAULT 1  // streamed k_gauss_rw for radii 13..24 (gauss_plan; profiles/r5k_streamed_rw_ab.txt)
#endif
#ifndef SIFT_SEED_BATCH
#define SIFT_SEED_BATCH 8  // k_seed_*: loads in flight; 16 measured the same (r5aq: 34.7 vs 35.2 us at 8K octave 3)
#endif

namespace sift {

// Geometry of the 64-column tiles (k_gauss_dog, k_gauss_vert).
constexpr int kGX = 64;              // tile columns
constexpr int kGY = 32;              // tile rows: 4 waves x 8
constexpr int kUR = 16;              // radii with unrolled code (octave 0)
constexpr int kUR1 = SIFT_UR1;       // ... octaves >= 1 (SGPR budget: taps are SGPR operands)
constexpr int kCG = kGX / 4;         // column groups of 4 outputs (16)
constexpr int kRS = 64 / kCG;        // row sub-groups per wave (4)
constexpr int kNR = 8 / kRS;         // rows per lane in the horizontal pass (2)
constexpr int kBW0 = kGX / 2 + kUR + 4;  // staged octave-0 region width (input columns)
constexpr int kSW0 = 2 * (kCG - 1) + 8 + 6;    // octave-0 strip stride for rmax <= 8
constexpr int kSW1 = 2 * (kCG - 1) + kUR + 6;  // ... rmax <= kUR
static_assert(kGY == kFY + 2 && kGX >= kFX + 2, "a fused tile decides the pixels one in from its 64 x 32 origin");
constexpr int kRingPlane = kGY * kGX;  // fused extrema: floats per plane of the DoG ring
constexpr int kVertNO = 16;          // k_gauss_vert: rows per wave
constexpr int kVertRows = 4 * kVertNO;  // ... per block
__host__ __device__ constexpr int fl2(int a) { return a >> 1; }   // floor(a / 2)
__host__ __device__ constexpr int cl2(int a) { return (a + 1) >> 1; }  // ceil(a / 2), a >= 0

// Geometry of the register-window tiles (k_gauss_rw): 256 strip columns hold
// an output tile of TW columns and its halo for every radius <= RW.
template <int RW>
struct RwGeom {
  static constexpr int NW = 8 + 2 * RW;              // window rows per lane
  static constexpr int TW = RW <= 16 ? 224 : 192;  // output columns per tile
  static constexpr int NCG = TW / 4;                  // column groups of 4
  static_assert(2 * RW <= 256 - TW, "halo fits the strip");
};
constexpr int kRwRows = 8;    // output rows per tile
constexpr int kRwSW = 264;    // strip row stride (doubles), 0 mod 8
constexpr int kRwStrip = kRwRows * kRwSW + 8;  // doubles per strip buffer
// Strip row t starts at rw_row(t): rows 4..7 one 16-byte quad further, so a
// ds_read_b128 lane group reading 8 column groups of rows t and t + 4 hits
// 16 distinct bank quads.
__host__ __device__ constexpr int rw_row(int t) { return t * kRwSW + 2 * (t >> 2); }

// Every instantiation the library launches, named once; the k_gauss_dog ones
// first: they may need > 64 KiB of LDS.  Each unit hands out its own.
enum GaussKernel {
  kKStaged8, kKStaged16, kKStaged8Fused, kKStaged16Fused, kKTiles, kKSplitTiles, kKNumDog,
  kKWindow12 = kKNumDog, kKWindow16, kKWindow24, kKStreamed12, kKStreamed16, kKStreamed24
};
using GaussKernelFn = void (*)(const Pyramid, const GaussLaunch);
GaussKernelFn gauss_tile0_kernel(int k);  // kKStaged8 .. kKStaged16Fused (sift_gauss_tile0.hip)
GaussKernelFn gauss_tile1_kernel(int k);  // kKTiles, kKSplitTiles (sift_gauss_tile1.hip)
GaussKernelFn gauss_rw_kernel(int k);     // kKWindow12 .. kKStreamed24 (sift_gauss_rw.hip)
__global__ void k_gauss_vert(const Pyramid P, int o, const double* __restrict__ base, double* __restrict__ vout,
                             long long bstride, long long vstride);  // sift_gauss_tile1.hip

// Device helpers of both kernel families.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ds_read_b128 serves a wave in four 16-lane groups, {0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same +32; lane -> (group, position in group).
__device__ __forceinline__ void b128_group(int lane, int& g, int& j) {
  const int l = lane & 31;
  int ga, ja;
  if (l < 4) ga = 0, ja = l;
  else if (l < 12) ga = 1, ja = l - 4;
  else if (l < 16) ga = 0, ja = l - 8;
  else if (l < 20) ga = 1, ja = l - 8;
  else if (l < 28) ga = 0, ja = l - 12;
  else ga = 1, ja = l - 16;
  g = 2 * (lane >> 5) + ga;
  j = ja;
}

// Register pinning: an empty asm that reads and writes the accumulators and
// clobbers memory.  The compiler keeps the source order of the fma chains
// and cannot hoist later loads above it, so the register window stays the
// size written (the scheduling-barrier builtin does not stop the selection
// DAG from delaying whole fma chains and keeping every loaded value alive).
template <int N>
__device__ __forceinline__ void pin(double (&a)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(a[i])::"memory");
}

// LDS hand-off between the lanes of ONE wave: the wave's LDS operations
// execute in order, so waiting for its own outstanding ones (and keeping the
// compiler from moving LDS accesses across) is all the ordering needed.
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Block barrier that orders LDS only: __syncthreads() is a release/acquire
// fence at workgroup scope and would also wait for every outstanding plane
// store of the wave (they are fire-and-forget otherwise).
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Buffer descriptor of a wave-uniform pointer, the pointer's halves taken
// through readfirstlane: a per-scale plane offset the compiler computed in
// VGPRs (s * plane as a 64-bit VALU product) otherwise makes the descriptor
// divergent and every store through it a waterfall loop (4 readfirstlanes,
// compares and an exec loop per store instruction; r6 ISA of k_gauss_rw).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t urs(const void* p, unsigned bytes) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  void* q = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

__device__ __forceinline__ double load_f64(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0));
}

// Generic radii: rows in chunks of 8 (chunk base jb), output t of the
// wave's 8 rows takes tap jb + k - t of chunk row k.  Taps outside [0, 2r]
// are zero and fma(0, v, acc) == acc, so the chunks skip them: the first
// chunk (jb = 0) has no taps for k < t, a tail chunk none for k - t > M =
// 2r - jb (and loads no row k > M + 7, past the window).  The same fma
// chains as the zero-padded form, term for term.
// With NO outputs per lane (k_gauss_vert: 16 rows per wave, half the window
// rows loaded per output): rows k <= M + NO - 1, the same skips.
template <int M, int NO = 8>
struct VChunk {
  static constexpr int kRows = M + NO < 8 ? M + NO : 8;  // rows k <= M + NO - 1
  template <bool FIRST, class Fma>
  __device__ __forceinline__ static void run(Fma&& f) {
#pragma unroll
    for (int k = 0; k < kRows; ++k)
#pragma unroll
      for (int t = 0; t < NO; ++t)
        if (!(FIRST && k < t) && k - t <= M) f(k, t);
  }
};
// m = 2r - jb (even): one body per tail (no zero taps at all: a chunk of 16
// outputs would spend most of a tail's 128 pairs on them).
template <bool FIRST, class Body>
__device__ __forceinline__ void vchunk16_dispatch(int m, Body&& body) {
  using F = std::integral_constant<bool, FIRST>;
  using N = std::integral_constant<bool, false>;
  if (FIRST) {
    if (m >= 7) body(VChunk<7, 16>{}, F{});
    else body(VChunk<7, 16>{}, N{});  // 2r < 7: zero-padded taps on both sides
    return;
  }
  switch (m >= 7 ? 7 : m) {
    case 7: body(VChunk<7, 16>{}, N{}); break;
    case 6: body(VChunk<6, 16>{}, N{}); break;
    case 4: body(VChunk<4, 16>{}, N{}); break;
    case 2: body(VChunk<2, 16>{}, N{}); break;
    case 0: body(VChunk<0, 16>{}, N{}); break;
    case -2: body(VChunk<-2, 16>{}, N{}); break;
    case -4: body(VChunk<-4, 16>{}, N{}); break;
    case -6: body(VChunk<-6, 16>{}, N{}); break;
    case -8: body(VChunk<-8, 16>{}, N{}); break;
    case -10: body(VChunk<-10, 16>{}, N{}); break;
    case -12: body(VChunk<-12, 16>{}, N{}); break;
    default: body(VChunk<-14, 16>{}, N{}); break;
  }
}

// m = 2r - jb (even).  Full chunks, and tail chunks with m >= 0, run all 64
// (k, t) pairs (a tail's few taps past 2r are zero padding); the first chunk
// skips its k < t triangle, the last chunks with m < 0 their rows past the
// window -- five bodies, so the register allocation of the kernel is not
// driven by a variant per radius.
template <bool FIRST, class Body>
__device__ __forceinline__ void vchunk_dispatch(int m, Body&& body) {
  using F = std::integral_constant<bool, FIRST>;
  using N = std::integral_constant<bool, false>;
  if (FIRST) {
    if (m >= 7) body(VChunk<7>{}, F{});
    else body(VChunk<7>{}, N{});  // 2r < 7: zero-padded taps on both sides
  } else if (m >= 0) {
    body(VChunk<7>{}, N{});
  } else if (m == -2) {
    body(VChunk<-2>{}, N{});
  } else if (m == -4) {
    body(VChunk<-4>{}, N{});
  } else {
    body(VChunk<-6>{}, N{});
  }
}

// Radius dispatch (uniform branch): a binary search over the unrolled radii
// LO..HI, log2 compares and branches instead of a compare chain of up to HI
// (every scale of every block dispatches twice).  Measured against the chain
// (profiles/r6g_radius_dispatch_ab.txt): 4K octave 1 0.162 -> 0.149 ms, octave
// 2 0.095 -> 0.089 ms, octave 3 -2 us.  (Octave 0's horz_any keeps a chain.)
template <int LO, int HI, class F>
__device__ __forceinline__ void rdispatch(int r, F&& f) {
  if constexpr (LO == HI) {
    f(std::integral_constant<int, LO>{});
  } else {
    constexpr int MID = (LO + HI) / 2;
    if (r <= MID) rdispatch<LO, MID>(r, f);
    else rdispatch<MID + 1, HI>(r, f);
  }
}

__device__ __forceinline__ void store4(float* p, const double (&v)[4], int nvalid) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q < nvalid) p[q] = (float)v[q];
}

// 16-byte buffer store; lanes whose offset is past the plane are dropped by
// the descriptor's range check.
__device__ __forceinline__ void bstore4(__amdgpu_buffer_rsrc_t rs, int voff, const double (&v)[4]) {
  const float4 f = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f), rs, voff, 0, SIFT_STORE_AUX);
}

}  // namespace sift
