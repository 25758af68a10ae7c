// Host side of the Gaussian + DoG pass: the launch plan of an octave, its
// launch, and the small kernels around the pass with their launchers.  Of the
// tile and window kernels it needs only the geometry (sift_gauss_dev.h).
#include <algorithm>
#include <vector>

#include "../../include/sift_hip.h"
#include "sift_gauss_dev.h"

namespace sift {

// sift_gauss_plan_info (include/sift_hip.h) reports these enumerators by value.
static_assert(SIFT_GAUSS_K_STAGED8 == kKStaged8 && SIFT_GAUSS_K_STAGED16 == kKStaged16 &&
                  SIFT_GAUSS_K_STAGED8_FUSED == kKStaged8Fused && SIFT_GAUSS_K_STAGED16_FUSED == kKStaged16Fused &&
                  SIFT_GAUSS_K_TILES == kKTiles && SIFT_GAUSS_K_SPLIT_TILES == kKSplitTiles &&
                  SIFT_GAUSS_K_WINDOW12 == kKWindow12 && SIFT_GAUSS_K_WINDOW16 == kKWindow16 &&
                  SIFT_GAUSS_K_WINDOW24 == kKWindow24 && SIFT_GAUSS_K_STREAMED12 == kKStreamed12 &&
                  SIFT_GAUSS_K_STREAMED16 == kKStreamed16 && SIFT_GAUSS_K_STREAMED24 == kKStreamed24,
              "public kernel enumerators");
static_assert(SIFT_GAUSS_PATH_STAGED0 == kGaussStaged0 && SIFT_GAUSS_PATH_BASE0 == kGaussBase0 &&
                  SIFT_GAUSS_PATH_TILES == kGaussTiles && SIFT_GAUSS_PATH_SPLIT_TILES == kGaussSplitTiles &&
                  SIFT_GAUSS_PATH_WINDOW == kGaussWindow && SIFT_GAUSS_PATH_STREAMED == kGaussStreamed &&
                  SIFT_GAUSS_MAX_GROUPS == kMaxScales,
              "public path enumerators");

// Materialised octave-0 base (fp64), for octave-0 radii beyond kUR.
__global__ __launch_bounds__(256) void k_upsample_base(const Pyramid P, double* __restrict__ b) {
  const int h = P.oct[0].h, w = P.oct[0].w;
  const long long n = (long long)h * w;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    b[i] = (double)P.img[(long long)min(y >> 1, P.H - 1) * P.img_stride + min(x >> 1, P.W - 1)];
  }
}

// DoG from a caller-supplied fp32 Gaussian pyramid (foreign scale space):
// D[t] = L[t] - L[t+1] in fp64 (exact for fp32 operands), rounded once.
__global__ __launch_bounds__(256) void k_dog_from_gauss(const float* __restrict__ g,
                                                        float* __restrict__ d, long long plane,
                                                        int nd) {
  const long long n = plane * nd;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    d[i] = (float)((double)g[i] - (double)g[i + plane]);
  }
}

// Cost of one scale of a tile, in units of one fp64 tap per output of both
// passes; the constant covers the strip round trip and the plane stores.
static int scale_cost(const Octave& oc, int s) { return 2 * oc.rad[s] + 1 + 8; }

// Split the NS scales of octave o into G contiguous groups (blockIdx.z) so
// that the most expensive group -- which also recomputes the scale before it
// as the DoG's L[s-1] -- is as cheap as possible (radii grow with s, so equal
// scale counts would leave the last group with most of the work).  Returns
// the max group cost; gb[0..G] are the group boundaries.
static int split_scales(const Pyramid& P, int o, int G, int* gb) {
  const Octave& oc = P.oct[o];
  const int NS = P.NS;
  // best[g][e]: min over splits of scales [0, e) into g groups of the max group cost
  int best[kMaxScales + 1][kMaxScales + 1], cut[kMaxScales + 1][kMaxScales + 1];
  auto cost = [&](int b, int e) {
    int c = 0;
    for (int s = std::max(0, b - 1); s < e; ++s) c += scale_cost(oc, s);
    return c;
  };
  for (int e = 0; e <= NS; ++e) best[1][e] = cost(0, e), cut[1][e] = 0;
  for (int g = 2; g <= G; ++g)
    for (int e = g; e <= NS; ++e) {
      best[g][e] = 1 << 30;
      for (int b = g - 1; b < e; ++b) {
        const int c = std::max(best[g - 1][b], cost(b, e));
        if (c < best[g][e]) best[g][e] = c, cut[g][e] = b;
      }
    }
  gb[G] = NS;
  for (int g = G, e = NS; g >= 1; --g) {
    gb[g - 1] = g > 1 ? cut[g][e] : 0;
    e = gb[g - 1];
  }
  return best[G][NS];
}

// The launch plan of one octave (GaussPlan, sift_kernels.h): which kernel
// runs it and with what geometry, decided here and nowhere else.
static GaussKernelFn gauss_kernel(int k) {
  return k < kKTiles ? gauss_tile0_kernel(k) : k < kKNumDog ? gauss_tile1_kernel(k) : gauss_rw_kernel(k);
}

// "a,b,..." from the environment of an experiments build (empty in the shipping library).
static std::vector<int> exp_list(const char* name) {
  std::vector<int> v;
#ifdef SIFT_EXPERIMENTS
  if (const char* e = std::getenv(name))
    for (const char* p = e; *p;) {
      v.push_back(std::atoi(p));
      while (*p && *p != ',') ++p;
      if (*p) ++p;
    }
#else
  (void)name;
#endif
  return v;
}

GaussPlan gauss_plan(const Pyramid& P, int o) {
  static const int rw_on = exp_knob("SIFT_RW", 1);
  static const int rws_on = exp_knob("SIFT_RWS", SIFT_RWS_DEFAULT);
  static const int rw_r = std::min(exp_knob("SIFT_RW_R", 12), 24);
  static const int rw_minb = exp_knob("SIFT_RW_MINB", 600);
  static const int l64_r = exp_knob("SIFT_L64_R", 90);
  static const int vsplit_r = exp_knob("SIFT_VSPLIT_R", 40);
  static const int xband = exp_knob("SIFT_XCD_BAND", -1);
  static const int xband0 = exp_knob("SIFT_XCD_BAND0", 0);
  static const std::vector<int> groups = exp_list("SIFT_GAUSS_GROUPS");  // "g1,g2,...": tile octaves 1, 2, ...
  static const std::vector<int> bpc = exp_list("SIFT_GAUSS_BPC");        // "b1,b2,...": octaves 1, 2, ...
  const Octave& oc = P.oct[o];
  const int R = oc.rmax;
  GaussPlan G{};
  // Octaves o >= 1 whose largest radius reaches SIFT_L64_R (default 90; 0 =
  // never) also store their fp64 Gaussian planes: the exact passes read them
  // instead of recomputing 3x3x3 patches with 189- and 377-tap chains (8K O=6
  // S=5: octaves 4 and 5; at 4K octave 3, radius 47, it measured slower: 0.71 -> 0.74 ms pass).
  G.keep_l64 = o >= 1 && l64_r > 0 && R >= l64_r;
  // Octaves >= 1 through k_gauss_rw (planes of at least 2 columns, no fp64
  // planes).  Radii up to SIFT_RW_R keep the register window of 8 + 2 RW rows
  // per lane (default 12: octave 1 at 4K and 1080p, 0.172 -> 0.158 ms at 4K;
  // RW 24 for octave 2 measured slower, 0.097 -> 0.100 ms:
  // profiles/r4r_register_window_ab.txt).  Radii above it up to 24 stream
  // the window per scale (rw_vert_stream, profiles/r5k_streamed_rw_ab.txt):
  // 192-column tiles in a 256-column strip instead of 64-column tiles with
  // (64 + 2r) / 64 of the vertical work.  SIFT_RWS bit 0: radii above
  // SIFT_RW_R; bit 1: the register-window octaves streamed too.  Radii above
  // 24 never run k_gauss_rw.
  const bool rw_ok = o >= 1 && oc.w >= 2 && !G.keep_l64;
  const bool streamed = rw_ok && R <= 24 && (rws_on & (R > rw_r ? 1 : 2)) != 0;
  const bool window = rw_ok && rw_on && R <= rw_r;
  if (o == 0) {
    // Radii above the unrolled range run on a materialised fp64 upsample of
    // the input (4 H W doubles) instead of the staged input region.
    G.path = R <= kUR ? kGaussStaged0 : kGaussBase0;
  } else if (streamed || window) {
    G.path = streamed ? kGaussStreamed : kGaussWindow;
  } else {
    // Largest radius from SIFT_VSPLIT_R (default 40; 0 = never): the split
    // vertical pass (k_gauss_vert) before the tile kernel.
    G.path = vsplit_r > 0 && R >= vsplit_r ? kGaussSplitTiles : kGaussTiles;
  }
  G.vsplit = G.path == kGaussSplitTiles;
  if (G.path == kGaussWindow || G.path == kGaussStreamed) {
    // (the streamed kernels use the tile geometry of their RW, as the window ones)
    G.rw = R <= 12 ? 12 : R <= 16 ? 16 : 24;
    G.tile_w = G.rw <= 16 ? RwGeom<16>::TW : RwGeom<24>::TW;
    G.tile_rows = kRwRows;
    G.sw = kRwSW;
    G.lds = sizeof(double) * 2 * kRwStrip;
    G.kernel = (streamed ? kKStreamed12 : kKWindow12) + (G.rw == 12 ? 0 : G.rw == 16 ? 1 : 2);
  } else {
    const bool staged = G.path == kGaussStaged0;
    G.tile_w = kGX;
    G.tile_rows = kGY;
    // Strip row stride (doubles).  Octaves >= 1: covers the widest read of
    // the horizontal pass (generic path: 4 (kCG - 1) + round_up(2r + 4, 8)),
    // and is 2 mod 4 so that the two rows a ds_read_b128 phase reads fall in
    // disjoint bank halves.
    if (staged) {
      G.sw = R <= 8 ? kSW0 : kSW1;
    } else {
      G.sw = R <= kUR1 ? kGX + 2 * R + 4 : kGX + 2 * R + 12;
      if (G.sw % 4 == 0) G.sw += 2;
    }
    G.lds = sizeof(double) * kGY * G.sw +
            (staged ? sizeof(double) * (size_t)(fl2(kGY - 1 + R) + cl2(R) + 1) * kBW0 : 0);  // + the staged region
    G.zero = R > (staged ? kUR : kUR1);  // generic-radius path present
    G.kernel = staged ? (R <= 8 ? kKStaged8 : kKStaged16) : G.vsplit ? kKSplitTiles : kKTiles;
    // Fused extrema decisions: the staged octave 0 (one scale group), a plane
    // of at least 3 x 3, the fp32 DoG ring after the strip and the region.
    G.lds_fused = G.lds + sizeof(float) * 3 * kRingPlane;
    G.can_fuse = staged && oc.h >= 3 && oc.w >= 3 && P.S >= 1 && G.lds_fused <= kGaussMaxLds;
  }
  G.gx = (oc.w + G.tile_w - 1) / G.tile_w;
  G.gy = (oc.h + G.tile_rows - 1) / G.tile_rows;
  // Scale groups: small octaves split their scales so that enough blocks fill
  // the 256 CUs; every group recomputes the scale before it.  Octave 0 never
  // splits (it is HBM-write bound).
  const long long tiles = (long long)G.gx * G.gy;
  G.G = 1;
  if (G.rw) {
    while (G.G < P.NS && tiles * G.G < rw_minb) ++G.G;  // fewer than SIFT_RW_MINB tiles x groups
  } else if (o >= 1 && o - 1 < (int)groups.size() && groups[o - 1] > 0) {
    G.G = std::min(groups[o - 1], P.NS);
  } else if (o >= 1) {
    // Measured (4K, O=4, S=5; tools/experiments/gpu_groups.sh): every split adds the
    // recomputed scale to the total work, so an octave splits only until it
    // has ~1.5 blocks per CU -- 60x68 tiles: 1 group; 30x34: 1 (G=2: 116 us,
    // G=4: 126-140 us, G=1: 103 us); 15x17: 2 (70.8 us; G=1 94 us, G=4 85 us).
    // (Split-pass octaves measured the same: 2048 instead of 400 blocks made
    // 4K octave 3 0.054 -> 0.073 ms.)
    while (G.G < P.NS && tiles * G.G < 400) ++G.G;
  }
  split_scales(P, o, G.G, G.gb);
  // XCD-banded tile order for octaves >= 1 (SIFT_XCD_BAND: bit o-1 of the
  // value; default all).  Measured (4K, O=4, S=5): isolated pass 0.748 ->
  // 0.730 ms, pipelined bench +0.5-1 % (tools/gpu_envab.sh).
  G.xcd_band = o >= 1 ? (xband >> (o - 1)) & 1 : xband0;
  // Blocks per CU of the octave-o >= 1 launches: the vertical passes re-read
  // the base window of every active block once per scale, and the active
  // blocks of an XCD share its 4 MiB L2.  SIFT_GAUSS_BPC caps the blocks per
  // CU by padding the dynamic LDS (experiments; 0 = no cap).
  if (o >= 1 && o - 1 < (int)bpc.size() && bpc[o - 1] > 0)
    G.lds = std::max(G.lds, kGaussMaxLds / bpc[o - 1] - 1024);
  static const char* const names[] = {
      "k_gauss_dog<octave0>", "k_gauss_dog<octave0>", kGaussFusedName, kGaussFusedName, "k_gauss_dog<64>",
      "k_gauss_vert + k_gauss_dog<64>", "k_gauss_rw<12>", "k_gauss_rw<16>", "k_gauss_rw<24>",
      "k_gauss_rw<12,true>", "k_gauss_rw<16,true>", "k_gauss_rw<24,true>"};
  G.kname = G.path == kGaussBase0 ? "k_upsample_base + k_gauss_dog<octave0,fp64 base>" : names[G.kernel];
  return G;
}

// The base of octave o+1 alone (sift_detect_from_seed_range_device: an
// octave below the scanned one only feeds its successor).  background.js:
// 114-118 samples L_o[S] at even rows and columns, so only those values are
// evaluated, with the tile kernels' fma chains (vertical then horizontal,
// taps in increasing order, from 0.0; the oracle's CONV_SEPARABLE_FMA_VH):
// k_seed_vert forms the vertical sums of the even rows (every column),
// k_seed_horz the horizontal sums at the even columns.  3/8 of one scale's
// work instead of all S+3 scales with their planes.
constexpr int kSeedBatch = SIFT_SEED_BATCH;

__global__ __launch_bounds__(256) void k_seed_vert(const Pyramid P, int o, const double* __restrict__ base,
                                                   double* __restrict__ vrow) {
  const Octave& oc = P.oct[o];
  const int x = blockIdx.x * 256 + threadIdx.x, yp = blockIdx.y;
  if (x >= oc.w) return;
  const int r = oc.rad[P.S], h = oc.h;
  const double* __restrict__ wt = P.wts + oc.wofs[P.S];
  const double* __restrict__ col = base + x;
  const long long w = oc.w;
  // kSeedBatch loads in flight ahead of their fma steps (the chain's order is
  // kept): 95 taps at r = 47 are 6 dependent load rounds instead of 95
  double acc = 0.0;
  int j = 0;
  for (; j + kSeedBatch <= 2 * r + 1; j += kSeedBatch) {
    double v[kSeedBatch];
#pragma unroll
    for (int k = 0; k < kSeedBatch; ++k) v[k] = col[clampi(2 * yp + j + k - r, 0, h - 1) * w];
#pragma unroll
    for (int k = 0; k < kSeedBatch; ++k) acc = __builtin_fma(wt[j + k], v[k], acc);
  }
  for (; j <= 2 * r; ++j) acc = __builtin_fma(wt[j], col[clampi(2 * yp + j - r, 0, h - 1) * w], acc);
  vrow[(long long)yp * w + x] = acc;
}

__global__ __launch_bounds__(256) void k_seed_horz(const Pyramid P, int o, const double* __restrict__ vrow,
                                                   double* __restrict__ next) {
  const Octave& oc = P.oct[o];
  const int nw = P.oct[o + 1].w;
  const int xp = blockIdx.x * 256 + threadIdx.x, yp = blockIdx.y;
  if (xp >= nw) return;
  const int r = oc.rad[P.S], w = oc.w;
  const double* __restrict__ wt = P.wts + oc.wofs[P.S];
  const double* __restrict__ row = vrow + (long long)yp * w;
  double acc = 0.0;
  int i = 0;
  for (; i + kSeedBatch <= 2 * r + 1; i += kSeedBatch) {
    double v[kSeedBatch];
#pragma unroll
    for (int k = 0; k < kSeedBatch; ++k) v[k] = row[clampi(2 * xp + i + k - r, 0, w - 1)];
#pragma unroll
    for (int k = 0; k < kSeedBatch; ++k) acc = __builtin_fma(wt[i + k], v[k], acc);
  }
  for (; i <= 2 * r; ++i) acc = __builtin_fma(wt[i], row[clampi(2 * xp + i - r, 0, w - 1)], acc);
  next[(long long)yp * nw + xp] = acc;
}

size_t seed_only_scratch(const Pyramid& P, int o) {
  return (size_t)P.oct[o + 1].h * P.oct[o].w;
}

hipError_t launch_seed_only(const Pyramid& P, int o, const double* base, double* vrow, double* next,
                            hipStream_t st) {
  if (o < 0 || o + 1 >= P.O || !base || !vrow || !next) return hipErrorInvalidValue;
  const Octave& oc = P.oct[o];
  const Octave& on = P.oct[o + 1];
  if (2 * (on.h - 1) > oc.h - 1 || 2 * (on.w - 1) > oc.w - 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_seed_vert, dim3((oc.w + 255) / 256, on.h), dim3(256), 0, st, P, o, base, vrow);
  hipLaunchKernelGGL(k_seed_horz, dim3((on.w + 255) / 256, on.h), dim3(256), 0, st, P, o, vrow, next);
  return hipGetLastError();
}

hipError_t launch_upsample_base(const Pyramid& P, double* base0, hipStream_t st) {
  const long long n = (long long)P.oct[0].h * P.oct[0].w;
  const int blocks = (int)std::min<long long>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(k_upsample_base, dim3(blocks), dim3(256), 0, st, P, base0);
  return hipGetLastError();
}

// Fills the launch fields of L from the plan and launches; decides nothing.
hipError_t launch_gauss_dog(const Pyramid& P, const GaussPlan& G, GaussLaunch L, hipStream_t st, GaussLaunched* rec) {
  const Octave& oc = P.oct[L.o];
  if (L.nimg < 1) L.nimg = 1;
  if (L.fuse && (!G.can_fuse || L.nimg > 1)) return hipErrorInvalidValue;  // batches: no fused decisions
  if (G.path != kGaussStaged0 && !L.base) return hipErrorInvalidValue;
  if (G.vsplit != (L.vsplit != nullptr)) return hipErrorInvalidValue;
  L.gx = L.fuse ? fused_words_per_row(oc.w) : G.gx;
  L.gy = L.fuse ? (oc.h - 2 + kFY - 1) / kFY : G.gy;
  if (L.fuse && L.gx != L.X.nw) return hipErrorInvalidValue;
  L.G = G.G;
  std::copy(G.gb, G.gb + G.G + 1, L.gb);
  L.xcd_band = G.xcd_band;
  L.sw = G.sw;
  L.zero = G.zero;
  const bool a16 = !((reinterpret_cast<uintptr_t>(L.dog)) & 15) &&
                   (!L.gauss || !((reinterpret_cast<uintptr_t>(L.gauss)) & 15)) &&
                   (L.nimg <= 1 || ((L.dog_bs & 3) == 0 && (!L.gauss || (L.gauss_bs & 3) == 0)));  // every image's planes
  L.vec = (a16 && (oc.w & 3) == 0 && 4.0 * oc.h * oc.w < 2147483648.0) ? 1 : 0;
  static bool attr_set = false;
  if (!attr_set) {  // allow > 64 KiB of dynamic LDS (gfx950 has 160 KiB per CU)
    for (int k = 0; k < kKNumDog; ++k)
      (void)hipFuncSetAttribute((const void*)gauss_kernel(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kGaussMaxLds);
    attr_set = true;
  }
  if (G.vsplit)
    hipLaunchKernelGGL(k_gauss_vert, dim3((oc.w + kGX - 1) / kGX, (oc.h + kVertRows - 1) / kVertRows, P.NS * L.nimg),
                       dim3(256), 0, st, P, L.o, L.base, L.vsplit, L.base_bs, L.vsplit_bs);
  const int k = L.fuse ? G.kernel + (kKStaged8Fused - kKStaged8) : G.kernel;
  hipLaunchKernelGGL(gauss_kernel(k), dim3(L.gx * L.gy * L.G * L.nimg), dim3(256), L.fuse ? G.lds_fused : G.lds, st, P,
                     L);
  if (rec) *rec = GaussLaunched{true, k, L.fuse, L.gx, L.gy, L.G, L.vec};
  return hipGetLastError();
}

hipError_t launch_dog_from_gauss(const float* g, float* d, long long plane, int nd,
                                 hipStream_t st) {
  long long n = plane * nd;
  int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_dog_from_gauss, dim3(blocks), dim3(256), 0, st, g, d, plane, nd);
  return hipGetLastError();
}

}  // namespace sift
