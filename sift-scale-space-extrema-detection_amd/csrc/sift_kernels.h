// Launch interfaces of the gfx950 SIFT kernels (internal to libsift_hip.so).
#pragma once
#include <algorithm>

#include "sift_common.h"

namespace sift {

// Device twin of sift_keypoint (include/sift_hip.h), same 48-byte layout.
struct Keypoint {
  int32_t octave, scale_level, local_x, local_y;
  double abs_x, abs_y, abs_sigma, interp_value;
};

#ifndef SIFT_FX
#define SIFT_FX 60
#endif
constexpr int kFX = SIFT_FX; // fused extrema: tile stride in x (64 computed columns, 60 owned, 60 decided)
constexpr int kFY = 30;      // ... in y (32 computed rows, 30 owned, 30 decided)

// Extrema decisions fused into the Gaussian+DoG pass of one octave (see
// k_gauss_dog): bitmap words of kFX columns, word bx of a row = tile column
// bx, bit b <-> x = kFX bx + 1 + b.
struct FusedExtrema {
  unsigned long long* bitmap;  // (scale 1, row 0, word 0) of the octave: [S][h][nw]
  unsigned* rowcount;          // (scale 1, row 0) of the octave: [S][h]
  int nw;                      // words per row (= tile columns of the launch)
  unsigned* amb_keys;          // keys needing an exact fp64 decision
  unsigned* counters;          // kCntAmb, kCntLow (below)
  unsigned amb_cap;
  float c_lo, c_hi;            // fp32 contrast thresholds (see ExtremaLaunch)
};

struct GaussLaunch {
  int o;
  int fuse;           // 1: extrema decisions of this octave in the same pass (X fields)
  FusedExtrema X;
  float* gauss;       // plane (o, 0) of the Gaussian pyramid, nullptr = do not store
  float* dog;         // plane (o, 0) of the DoG pyramid
  double* next_seed;  // base of octave o+1 (nullptr for the last octave)
  int next_w;
  const double* base; // fp64 octave base h x w (o >= 1: the seed; o == 0: only when materialised)
  double* l64;        // plane (o, 0) of the kept fp64 Gaussian planes, nullptr = not kept
  double* vsplit;     // split pass (GaussPlan.vsplit): fp64 scratch of NS vertical-sum planes h x w, filled by a
                      // separate launch; the tile kernel copies its strip from it (nullptr = one pass)
  // filled by launch_gauss_dog from the GaussPlan
  int sw;             // strip row stride (doubles)
  int vec;            // float4 plane stores are aligned
  int zero;           // strips need zeroing (generic-radius path present)
  int gb[kMaxScales + 1];  // scale groups: group g computes scales gb[g] .. gb[g+1]-1
  int gx, gy, G;      // tiles per row, tile rows, scale groups (1D grid of gx gy G blocks)
  int xcd_band;       // 1: block -> tile so that each XCD runs a contiguous band of tile rows
  // batch: nimg images in one launch (blocks image-major); image im's
  // pointers are the fields above + im * these element strides
  int nimg;
  long long gauss_bs, dog_bs, seed_bs, base_bs, l64_bs, vsplit_bs;
};

constexpr int kXW = 62;      // output columns per extrema wave (lanes 1..62; lanes 0, 63 are halo)
#ifndef SIFT_XROWS
#define SIFT_XROWS 30
#endif
constexpr int kXRows = SIFT_XROWS;  // centre rows per extrema wave (multiple of 3)
#ifndef SIFT_XMAXGROUP
#define SIFT_XMAXGROUP 5
#endif
constexpr int kXMaxGroup = SIFT_XMAXGROUP;// scales per extrema wave (S > 5 splits the scales into groups)

// Geometry of the candidate bitmap and its row counts, built once per extrema
// stage and carried by value in every launch struct that addresses them.
// Octave o holds [S][h] rows of nw[o] words: rows row_off[o] .., words
// word_off[o] ..; bit b of word xw of a row <-> column xw ww[o] + woff[o] + b.
// Octaves decided by the scan have kXW-column words from column 0, octaves
// decided in the Gaussian pass (FusedExtrema) kFX-column words from column 1.
// A batch (P.nimg images) repeats the rows and words image-major.
struct BitmapGeom {
  int n_oct;
  int row_off[kMaxOctaves + 1];     // first row of each octave; [n_oct] = rows per image
  long long word_off[kMaxOctaves];  // first bitmap word of each octave
  int nw[kMaxOctaves];              // words per row
  int ww[kMaxOctaves];              // columns per word
  int woff[kMaxOctaves];            // column of bit 0 of word 0
  long long words_per_img;
  int rows_per_img;
};

// One launch scans every octave: unit u (one wave) = (octave, strip of kXRows
// rows, 62-column word, scale group).
struct ExtremaLaunch {
  int u_begin, u_end;            // units of this launch (a range of octaves)
  int exact_planes;              // DoG planes are the data itself (caller-supplied): no fp32 ties
  int ng;                        // scale groups per (strip, word)
  int xcd_band;                  // 1: block -> units so that each XCD scans a contiguous range of units
  float c_lo, c_hi;              // |v| < c_lo: certainly low contrast; |v| >= c_hi: certainly not
  int unit_off[kMaxOctaves + 1]; // first unit of each octave
  BitmapGeom G;                  // of bitmap, rowcount, lowbitmap, lowrowcount, ambbitmap
  unsigned long long* bitmap;
  unsigned* rowcount;
  unsigned* amb_keys;            // keys needing an exact fp64 decision (unordered)
  unsigned* counters;            // kCntAmb, kCntLow, kCntDrop (below)
  unsigned amb_cap;
  unsigned long long* lowbitmap; // certain low-contrast extrema, same layout as bitmap (nullptr = not listed)
  unsigned* lowrowcount;
  // Ambiguous words (ambbitmap != nullptr): instead of one key per ambiguous
  // pixel, the scan writes the word's ambiguous bits to ambbitmap (same
  // layout as bitmap) and lists the word's index (into bitmap) in amb_keys
  // (counters[kAmbWords] of them); k_exact_words re-decides a whole word.
  unsigned long long* ambbitmap;
};
constexpr int kAmbWords = 8;     // counters slot: listed ambiguous words
// The other slots of the device counters (sift_ctx::counters), written by the
// extrema and refinement kernels and read back by the host.
enum {
  kCntAmb = 0,       // ambiguous keys
  kCntLow = 1,       // low-contrast extrema
  kCntDrop = 2,      // slots dropped by the exact pass
  kCntUnc = 3,       // uncertain refinements
  kCntSing = 4,      // singular Hessians
  kCntLowLate = 6,   // late (exact-pass) low-contrast entries
  kCntLowSure = 7,   // ordered (certain) low-contrast entries
  kCntN = 12,        // candidate slots
  kCntKp = 13,       // keypoints
  kCntDbg = 16,      // debug block, kCntDbgWords slots: [kCntDbg + b] refinements uncertain for reason b
  kCntDbgIter = 22,  // ... [kCntDbgIter + min(it, 4)] by iteration count
  kCntDbgPrec = 27,  // ... uncertain for output precision
  kCntDbgWords = 16,
  kBlk = 64          // from here: the kept keypoints per (octave, scale) block (kBlkWords slots, below)
};

// One launch over every octave: global row g (one wave each) = G.row_off[o] +
// (s-1) h_o + y.
struct EmitLaunch {
  BitmapGeom G;
  int o_first;                   // first octave with decisions (earlier octaves' rows hold none: no waves)
  const unsigned long long* bitmap;
  const unsigned* rowcount;      // [all rows]
  const unsigned* rowoff;        // exclusive scan of rowcount
  unsigned* keys;                // ordered candidate keys
  double* value;
  unsigned* keep;                // nullptr: not written
  unsigned cap;                  // slots in keys/value/keep (overflow is detected by the host)
  int deferred;                  // 1: value = NaN ("the fp32 plane value"): the refinement reads it from the
                                 // DoG plane (the centre of the 3x3x3 neighbourhood it gathers anyway),
                                 // launch_fill_values before the list is copied out; no plane gather here
  unsigned* n_out;               // != nullptr: *n_out = rowoff[n_index] (the list's length), by thread 0
  long long n_index;
};

// Fills the deferred (NaN) candidate values of slots [0, *n) from the DoG planes.
hipError_t launch_fill_values(const Pyramid& P, const unsigned* keys, double* value, const unsigned* n, int cap,
                              hipStream_t st);

struct ExactLaunch {
  const unsigned* amb_keys;      // counters[kCntAmb] of them (at most amb_cap stored)
  unsigned amb_cap;
  const unsigned* keys;          // ordered candidates
  const unsigned* n;             // device: number of candidates
  unsigned cap;
  unsigned* keep;
  double* value;
  unsigned* counters;            // kCntLowLate: late low-contrast extrema (ambiguous ones decided low)
  unsigned* late_keys;           // their keys / exact values (nullptr = not listed), amb_cap slots
  double* late_vals;
  // A key's list position is its row's offset plus the candidate bits before
  // it in the row's bitmap words (bitmap == nullptr: binary search over keys).
  const unsigned long long* bitmap;
  const unsigned* rowoff;
  BitmapGeom G;
  const unsigned long long* ambbitmap;  // ambiguous words (k_exact_words; nullptr: amb_keys are pixel keys)
  int amb_lds_stride;            // k_exact_words: doubles per vertical-sum row (64 + 2 rmax)
  int amb_patch_stride;          // ... doubles per wave of the per-pixel patch scratch
};

struct RefineLaunch {
  const unsigned* cand_key;
  const double* cand_val;
  const unsigned* keep;  // nullptr = every entry is a candidate
  const unsigned* n;     // device: number of entries (<= cap)
  int cap;
  int exact_planes;
  double min_blur, min_interpixel_distance;
  int* status;        // per candidate kRef*
  Keypoint* kp;       // per candidate (valid where status == kRefKeep)
  unsigned* uncertain;// indices for the exact pass
  unsigned* counters; // [3] n uncertain, [4] n singular
  const unsigned* perm; // processing order: thread t refines slot perm[t] (nullptr = slot t)
  int wide_exact;       // k_refine_exact: 256 threads per patch (latency) instead of one wave (throughput)
};

// Processing order of the fast refinement (band_order): the slots of the
// extrema stage are ordered (octave, scale, row, column); the refinement
// takes them as (octave, band of kBandRows rows, scale, row, column) so the
// candidates whose 3x3x3 patches share DoG lines of adjacent scales run
// together (one XCD's L2) instead of a whole plane apart.
#ifndef SIFT_BAND_ROWS
#define SIFT_BAND_ROWS 16
#endif
constexpr int kBandRows = SIFT_BAND_ROWS;
struct BandOrder {
  BitmapGeom G;                   // rows of rowoff: global row (o, s = 1, y = 0) = G.row_off[o]
  int S, n_items;
  int item_off[kMaxOctaves + 1];  // first item of each octave: items (band, scale) of octave o
  const unsigned* rowoff;         // exclusive scan of the extrema stage's row counts
  unsigned* count;                // per item: slots in it
  unsigned* first;                // per item: its first slot
  const unsigned* start;          // per item: exclusive scan of count (first position in the new order)
  unsigned* perm;                 // out: position -> slot
  int cap;                        // (a batch: items are image-major, item_off per image)
};
hipError_t launch_band_items(const Pyramid& P, const BandOrder& B, hipStream_t st);
hipError_t launch_band_fill(const Pyramid& P, const BandOrder& B, hipStream_t st);

// Everything that is decided about octave o's Gaussian+DoG pass, built once
// per geometry by gauss_plan (the context holds one per octave) and read by
// the launcher and by the stages that size buffers for it.
enum GaussPath {
  kGaussStaged0,     // octave 0 from the staged input region (k_gauss_dog<octave0>; strip stride kSW0 / kSW1)
  kGaussBase0,       // octave 0 on a materialised fp64 upsample (launch_upsample_base first), 64-column tiles
  kGaussTiles,       // 64-column tiles (k_gauss_dog<64>)
  kGaussSplitTiles,  // split vertical pass (k_gauss_vert) + 64-column tiles
  kGaussWindow,      // register-window tiles (k_gauss_rw<RW>)
  kGaussStreamed,    // ... with the window streamed per scale (k_gauss_rw<RW,true>)
};
constexpr size_t kGaussMaxLds = 160 * 1024;  // LDS of one gfx950 CU: a plan with more cannot launch
constexpr const char* kGaussFusedName = "k_gauss_dog<octave0,fused extrema>";
struct GaussPlan {
  GaussPath path;
  int kernel;              // the instantiation (GaussKernel, sift_gauss_dev.h)
  const char* kname;       // its launches, e.g. "k_gauss_rw<12>" or "k_gauss_vert + k_gauss_dog<64>" (static string;
                           // sift_last_pass_kernels); a fused launch is kGaussFusedName
  int rw;                  // k_gauss_rw: window radius RW (12, 16, 24); 0 otherwise
  int tile_w, tile_rows;   // output columns x rows per block
  int gx, gy;              // tiles per row, tile rows (unfused)
  int sw;                  // strip row stride (doubles)
  size_t lds, lds_fused;   // dynamic LDS bytes of the launch, unfused / fused
  int zero;                // strips need zeroing (generic-radius path present)
  bool keep_l64;           // the octave stores its fp64 Gaussian planes too (GaussLaunch.l64): the exact passes
                           // then read the patch values instead of recomputing them
  bool vsplit;             // needs the split pass's scratch (GaussLaunch.vsplit: NS x h x w doubles)
  bool can_fuse;           // may run with its extrema decisions fused (GaussLaunch.fuse)
  int xcd_band;            // GaussLaunch.xcd_band
  int G;                   // scale groups; group g computes scales gb[g] .. gb[g+1]-1
  int gb[kMaxScales + 1];
};
GaussPlan gauss_plan(const Pyramid& P, int o);
// What launch_gauss_dog launched for an octave (sift_last_gauss_plan): the instantiation, fused variants included, and
// the launch fields it filled.
struct GaussLaunched {
  bool valid;
  int kernel, fuse, gx, gy, G, vec;
};
hipError_t launch_gauss_dog(const Pyramid& P, const GaussPlan& G, GaussLaunch L, hipStream_t st,
                            GaussLaunched* rec = nullptr);
hipError_t launch_upsample_base(const Pyramid& P, double* base0, hipStream_t st);
// The base of octave o+1 from octave o's base alone (no planes): L_o[S] at
// even rows / columns; vrow: seed_only_scratch(P, o) doubles.
size_t seed_only_scratch(const Pyramid& P, int o);
hipError_t launch_seed_only(const Pyramid& P, int o, const double* base, double* vrow, double* next, hipStream_t st);
// Tile columns of a fused launch over a w-column octave (= bitmap words per row).
inline int fused_words_per_row(int w) { return w > 2 ? (w - 2 + kFX - 1) / kFX : 1; }
hipError_t launch_dog_from_gauss(const float* g, float* d, long long plane, int nd, hipStream_t st);

// Fills the unit table of L and launches the scan; returns the launch error.
// The octaves [o_begin, o_end) of L.G must have the scan's word geometry
// (extrema_words_per_row words of kXW columns), else hipErrorInvalidValue.
hipError_t launch_extrema(const Pyramid& P, ExtremaLaunch& L, hipStream_t st, int o_begin, int o_end);
inline int extrema_words_per_row(int w) { return (w + kXW - 1) / kXW; }
hipError_t launch_emit(const Pyramid& P, const EmitLaunch& E, hipStream_t st);
// Zeroes up to three word ranges in one launch (the extrema stage's counters
// and row counts: one kernel instead of hipMemsetAsync's body + tail fills each).
hipError_t launch_zero_words(unsigned* a, long long na, unsigned* b, long long nb, unsigned* c, long long nc,
                             hipStream_t st);
// One wave per ambiguous candidate: fp64 pointwise recompute of the 3x3x3 DoG patch.
// Persistent grid over the device-side count of ambiguous keys (no host sync).
hipError_t launch_exact_extrema(const Pyramid& P, const ExactLaunch& X, hipStream_t st);
// One wave per listed ambiguous word (ExtremaLaunch.ambbitmap mode).
hipError_t launch_exact_words(const Pyramid& P, ExactLaunch X, hipStream_t st);

hipError_t launch_refine_fast(const Pyramid& P, const RefineLaunch& R, hipStream_t st);
hipError_t launch_refine_exact(const Pyramid& P, const RefineLaunch& R, hipStream_t st);

// Order-preserving compaction helpers.
// Entries i >= *n (device count) of the cap-sized arrays are inactive.
// launch_keep_compact: keep[i] = status[i] is a kept keypoint whose candidate
// row (whole-image octave rows, P.row0 applied) lies in the input rows
// [own_lo, own_hi) (own_lo < 0: every row; own_hi < 0: no upper bound).  blk
// (kBlkWords, zeroed by the caller) receives the first slot of every (octave,
// scale) block of the candidate list at blk[kBlkStart + b], b = o * S + s - 1
// (candidates are in key order, so a block is a slot range), or sets
// blk[kBlkUnsorted] when the list is not in key order.
constexpr int kBlkN = 1024;  // blk[b]: kept keypoints of block b = (image, octave, scale) (launch_count_keypoints)
static_assert(kBlkN >= kMaxOctaves * kMaxScales, "one image's blocks");
constexpr int kBlkStart = kBlkN;                  // blk[kBlkStart + b], b <= O*S: first slot of block b
constexpr int kBlkUnsorted = kBlkStart + kBlkN + 1;
constexpr int kBlkWords = kBlkUnsorted + 1;
constexpr int kCntAll = kBlk + kBlkWords;  // all counter slots: per-block counts, block starts, order flag
hipError_t launch_scatter_keys(const unsigned* keep, const unsigned* pos, const unsigned* key, const unsigned* n,
                               int cap, unsigned* out, hipStream_t st);
// The keep flags, their exclusive scan into pos and the kept keypoints'
// copies into out, with the work bounded by *n instead of cap: keep and pos
// are written for the slots of the tiles up to slot min(*n, cap) (what
// launch_count_keypoints and launch_scatter_keys read); tile holds
// keep_tiles(cap) words of scratch.
constexpr int kKeepTile = 512;  // two slots per thread: 4K (714 K candidates) 1400 tiles
inline size_t keep_tiles(int cap) { return cap > 0 ? (size_t)(cap + kKeepTile - 1) / kKeepTile : 0; }
hipError_t launch_keep_compact(const Pyramid& P, const int* status, const unsigned* key, unsigned* keep,
                               unsigned* pos, unsigned* tile, const unsigned* n, int cap, int own_lo, int own_hi,
                               unsigned* blk, const Keypoint* kp, Keypoint* out, hipStream_t st);
// out = pos[n-1] + keep[n-1] (0 if n == 0): the number of keypoints; blk[b] =
// kept keypoints of block b, from the block starts and the exclusive scan pos
// (a histogram over the slots when the list was not in key order).
hipError_t launch_count_keypoints(const Pyramid& P, const unsigned* pos, const unsigned* keep, const unsigned* key,
                                  const unsigned* n, int cap, unsigned* out, unsigned* blk, hipStream_t st);

size_t exact_lds_bytes(const Pyramid& P);

// Block-major merge (sift_merge_keypoint_blocks_device) as copies of the
// nseg contiguous (part, block) runs: seg[3 i] = {source byte offset,
// destination byte offset, bytes}, cstart[i] = first 16-KiB chunk of run i,
// n_chunks = cstart[nseg] (device tables).
constexpr long long kMergeChunk = 16384;
hipError_t launch_merge_blocks(const Keypoint* in, const long long* seg, const long long* cstart, int nseg,
                               long long n_chunks, Keypoint* out, hipStream_t st);

// Keypoint records -> field arrays (4 int32 + 4 doubles per keypoint, sift_copy_keypoints_soa's layout).
hipError_t launch_kp_soa(const Keypoint* kp, int n, int32_t* ints, double* reals, hipStream_t st);

// keys -> 4 int32 per keypoint: octave, scale, whole-image octave row (row0 applied), x.
hipError_t launch_decode_origins(const Pyramid& P, const unsigned* keys, int n, int32_t* out, hipStream_t st);

// Orientation assignment and descriptors (sift_feature.hip).  The constants
// are the SIFT_ORI_* / SIFT_DESC_* of include/sift_hip.h
// (sift_api_feature.hip asserts the match).
constexpr int kOriBins = 36, kOriSmooth = 6, kOriMaxPeaks = 18;
constexpr double kOriLambda = 1.5, kOriPeakRatio = 0.8;
constexpr int kDescOri = 8, kDescBytes = 128;
constexpr double kDescLambda = 6.0, kDescCap = 0.2;
// Device twin of sift_orientation, same 16-byte layout.
struct Orientation {
  int32_t keypoint, bin;
  double theta;
};
// One wave per keypoint i < n of planes gauss (the pyramid's fp32 Gaussian
// planes): count[i] = its peaks (count[n] = 0), mask[i] = their bins, theta[18
// i + j] = the angle of its j-th peak in bin order.
hipError_t launch_orient(const Pyramid& P, const float* gauss, int planes_first, const Keypoint* kp, int n,
                         unsigned* count, unsigned long long* mask, double* theta, hipStream_t st);
// off = the exclusive scan of count: keypoint i's records at out[off[i] ..], ascending bin (cap slots).
hipError_t launch_orient_emit(const unsigned* off, const unsigned long long* mask, const double* theta, int n,
                              unsigned cap, Orientation* out, hipStream_t st);
// One wave per record: desc[128 r ..], described[r]; *n_described (zeroed by the caller) counts the described.
hipError_t launch_describe(const Pyramid& P, const float* gauss, int planes_first, const Keypoint* kp,
                           const Orientation* ori, int n, unsigned char* desc, unsigned char* described,
                           unsigned* n_described, hipStream_t st);

// Descriptor matching (sift_match.hip).  Device twins of sift_match and of the
// selected pair record (include/sift_hip.h), same 16-byte layouts.
struct Match {
  int32_t best, second, d2_best, d2_second;
};
struct MatchPair {
  int32_t query, train, d2, d2_second;
};
constexpr int kMatchNQ = 4;                          // query fragments of 32 a wave keeps in registers
constexpr int kMatchWaves = 4;                       // waves per block
constexpr int kMatchQB = 32 * kMatchNQ * kMatchWaves;  // queries per block
constexpr int kMatchChunk = 256;                     // train rows per key fold: the key's low byte is the row
constexpr int kMatchBlocks = 1024;                   // blocks worth launching: four per CU
// The train split, a function of the two counts alone: as many splits of whole
// chunks as bring the grid to kMatchBlocks blocks, when the queries alone do not.
struct MatchSplit {
  int query_blocks, chunks, chunks_per_split, splits;
};
inline MatchSplit match_split(int n_query, int n_train) {
  MatchSplit s{};
  s.query_blocks = (int)(((long long)n_query + kMatchQB - 1) / kMatchQB);
  s.chunks = (int)(((long long)n_train + kMatchChunk - 1) / kMatchChunk);
  if (s.query_blocks < 1 || s.chunks < 1) return s;
  const int want = std::min(s.chunks, (kMatchBlocks + s.query_blocks - 1) / s.query_blocks);
  s.chunks_per_split = (s.chunks + want - 1) / want;
  s.splits = (s.chunks + s.chunks_per_split - 1) / s.chunks_per_split;
  return s;
}
inline long long match_query_rows(int n) { return ((long long)n + kMatchQB - 1) / kMatchQB * kMatchQB; }
inline long long match_train_rows(int n) { return ((long long)n + kMatchChunk - 1) / kMatchChunk * kMatchChunk; }
// dst = the n_pad-row packed copy of src's n rows of 128 bytes, each byte ^
// 0x80, masked (mask[r] == 0; mask may be nullptr) and padding rows zero;
// norm[r] = the shifted row's squared norm, -1 for those rows (train == 0), or
// its key base (norm << 8) | (r & 255), INT32_MAX for those rows (train != 0).
hipError_t launch_match_prep(const unsigned char* src, const unsigned char* mask, int n, long long n_pad, int train,
                             unsigned char* dst, int* norm, hipStream_t st);
// part[s n_query + q] = the top-2 of query q over the train rows of split s
// (match_split(n_query, n_train).splits of them); qs / ts, qn / kb from launch_match_prep.
hipError_t launch_match(const unsigned char* qs, const int* qn, int n_query, const unsigned char* ts, const int* kb,
                        int n_train, Match* part, hipStream_t st);
// out[q] = the top-2 over the splits' records; splits == 0 writes missing neighbours.
hipError_t launch_match_merge(const Match* part, int splits, int n_query, Match* out, hipStream_t st);
// flag[q] = fwd[q] is accepted (q < n_query), flag[n_query] = 0; r2 = ratio^2 or <= 0; rev may be nullptr.
hipError_t launch_match_flag(const Match* fwd, int n_query, const Match* rev, int n_train, double r2, unsigned* flag,
                             hipStream_t st);
// off = the exclusive scan of flag: the accepted pairs in ascending query index (cap slots).
hipError_t launch_match_emit(const Match* fwd, const unsigned* flag, const unsigned* off, int n_query, unsigned cap,
                             MatchPair* out, hipStream_t st);

// RANSAC homography verification of match pairs (sift_verify.hip).  Device
// twins of sift_point_pair and sift_homography (include/sift_hip.h), same layouts.
struct PointPair {
  double qx, qy, tx, ty;
};
struct Homography {
  double h[9];
  int32_t hypothesis, inliers;
};
constexpr int kMaxHypotheses = 65536;
constexpr int kScoreR = 4;                            // pairs a lane keeps in registers
constexpr int kScoreWaves = 4;                        // waves per block
constexpr int kScorePairs = 64 * kScoreWaves * kScoreR;  // pairs per block
constexpr int kScoreTile = 64;                        // hypotheses a block walks
// The inlier rule of include/sift_hip.h, the one statement of it: the score
// kernel, the flag kernel and nothing else decide with it.  (x, y) -> (X, Y)
// under row-major h; no division; a NaN anywhere compares false.
__host__ __device__ inline bool homography_inlier(double h0, double h1, double h2, double h3, double h4, double h5,
                                                  double h6, double h7, double h8, double x, double y, double X,
                                                  double Y, double t2) {
#pragma clang fp contract(off)
  const double u = (h0 * x + h1 * y) + h2;
  const double v = (h3 * x + h4 * y) + h5;
  const double w = (h6 * x + h7 * y) + h8;
  const double du = u - X * w, dv = v - Y * w;
  const bool front = w > 0.0, near = (du * du + dv * dv) < t2 * (w * w);
  return front & near;  // both evaluated: no branch around the second in the score loop
}
// Step 3 of the RANSAC definition, the one statement of it: the hypothesis
// kernel and the refit's solve kernel call it.  Entry (r, c) of the 8 x 9
// system [A | b] is a[(r * 9 + c) * kStride] (LDS: the pivot row is a runtime
// index, which in registers would mean scratch); h receives the eight
// unknowns.  False for a zero or non-finite pivot or a non-finite h; the
// elimination is carried to the end either way.
template <int kStride>
__device__ __forceinline__ bool homography_solve(double* a, double (&h)[8]) {
#pragma clang fp contract(off)
#define A_(r, c) a[((r) * 9 + (c)) * kStride]
  bool ok = true;
  for (int c = 0; c < 8; ++c) {
    int p = c;
    double best = __builtin_fabs(A_(c, c));
    for (int r = c + 1; r < 8; ++r) {
      const double m = __builtin_fabs(A_(r, c));
      if (m > best) best = m, p = r;
    }
    if (!(best > 0.0 && best < __builtin_huge_val())) ok = false;  // zero, infinite or NaN
    for (int j = c; j < 9; ++j) {                                   // p == c swaps a row with itself
      const double t = A_(p, j);
      A_(p, j) = A_(c, j);
      A_(c, j) = t;
    }
    const double piv = A_(c, c);
    for (int r = c + 1; r < 8; ++r) {
      const double f = A_(r, c) / piv;
      for (int j = c + 1; j < 9; ++j) A_(r, j) = A_(r, j) - f * A_(c, j);
    }
  }
#pragma unroll
  for (int c = 7; c >= 0; --c) {
    double t = A_(c, 8);
#pragma unroll
    for (int j = c + 1; j < 8; ++j) t = t - A_(c, j) * h[j];
    h[c] = t / A_(c, c);
    if (!(__builtin_fabs(h[c]) < __builtin_huge_val())) ok = false;
  }
#undef A_
  return ok;
}
// points[i] = (abs_x, abs_y) of the query and of the train keypoint behind pair
// i's orientation records; four NaNs when an index is outside its list.
hipError_t launch_pair_points(const MatchPair* pairs, int n, const Orientation* q_ori, int nq_ori, const Keypoint* q_kp,
                              int nq_kp, const Orientation* t_ori, int nt_ori, const Keypoint* t_kp, int nt_kp,
                              PointPair* points, hipStream_t st);
// H[9 k ..], valid[k] of hypothesis k < K for this seed over n >= 4 pairs.
hipError_t launch_homography_hypotheses(const PointPair* points, int n, int K, unsigned long long seed, double* H,
                                        int* valid, hipStream_t st);
// counts[k] += the inliers of H[9 k ..] among the n pairs (counts zeroed by the caller).
hipError_t launch_homography_score(const PointPair* points, int n, const double* H, int K, double t2, int* counts,
                                   hipStream_t st);
// counts[k] = -1 where !valid[k]; *model = the arg-max of (count, -k), or (-1, 0, zeros).
hipError_t launch_homography_best(const double* H, const int* valid, int* counts, int K, Homography* model,
                                  hipStream_t st);
// flag[i] = pair i is an inlier of *model (i < n), flag[n] = 0.
hipError_t launch_inlier_flag(const PointPair* points, int n, const Homography* model, double t2, unsigned* flag,
                              hipStream_t st);
// off = the exclusive scan of flag: the inlier indices in ascending order (cap slots).
hipError_t launch_inlier_emit(const unsigned* flag, const unsigned* off, int n, unsigned cap, int32_t* out,
                              hipStream_t st);

// Least-squares homography fit of a list of pairs (sift_refit.hip; the
// definition is in include/sift_hip.h).
constexpr int kFitSums = 44;    // the upper triangle of the 8 x 8 normal matrix with column 8, row-major
constexpr int kFitChunk = 64;   // terms per leaf of the summation tree: one wave
constexpr int kFitKeys = 9;     // box bounds as ordered integer keys (k_fit_box), and the list's ok word
constexpr int kMaxRefitRounds = 16;
// What one fit leaves on the device: the model first (hypothesis 0 for a valid
// fit, -1 with nine zeros for an invalid one, so that k_inlier_flag of an
// invalid fit flags nothing), then cx, cy, dq, cX, cY, dt and the 44 sums.
struct FitRecord {
  Homography model;
  double box[6];
  double sums[kFitSums];
};
// Chunk sums the first level of the tree writes for a list of m entries.
inline long long fit_chunks(long long m) { return (m + kFitChunk - 1) / kFitChunk; }
// One fit of index[0 .. m) (nullptr: 0 .. m-1, m == n) over n pairs, m >= 4:
// box, sums, the tree's levels and the solve, all enqueued on st.  keys:
// kFitKeys words; parts_a / parts_b: fit_chunks(m) * 44 and
// fit_chunks(fit_chunks(m)) * 44 doubles.
hipError_t launch_homography_fit(const PointPair* points, int n, const int32_t* index, int m, unsigned long long* keys,
                                 double* parts_a, double* parts_b, FitRecord* rec, hipStream_t st);

// Keypoint budget (sift_budget.hip; the definition is in include/sift_hip.h).
constexpr int kBudgetThreads = 256;
constexpr int kBudgetPerThread = 8;                                // records of one thread
constexpr int kBudgetTile = kBudgetThreads * kBudgetPerThread;     // records of one block
constexpr int kBudgetLdsCells = 16;                                // up to here a block keeps the bins in LDS (16 KiB)
constexpr int kBudgetMaxCells = 16384;
// Bytes of the composite behind the key: those of n - 1 (at least one); a selection runs 8 + this many passes.
int budget_tail_bytes(int n);
// key[i], and with cell_px > 0 cell[i], of the n records.
hipError_t launch_budget_keys(const Keypoint* kp, int n, int cell_px, int ncx, int ncy, unsigned long long* key,
                              unsigned* cell, hipStream_t st);
// flag[i] = record i is active (active == nullptr: all are) and fewer than quota active records of its cell (cell ==
// nullptr: one cell) precede it; flag[n] = 0.  tkey, ttail, rem: one word per cell; hist: cells * 256 zeroed words,
// left zeroed.
hipError_t launch_budget_select(const unsigned long long* key, const unsigned* cell, const unsigned* active, int n,
                                int cells, unsigned quota, unsigned long long* tkey, unsigned* ttail, unsigned* rem,
                                unsigned* hist, unsigned* flag, hipStream_t st);
// flag[i] = 1 for i < n, flag[n] = 0: a budget without a limit.
hipError_t launch_budget_fill(unsigned* flag, int n, hipStream_t st);
// off = the exclusive scan of flag: index[off[i]] = i and kp_out[off[i]] = kp[i] for the flagged records (cap slots;
// either output may be nullptr).
hipError_t launch_budget_emit(const unsigned* flag, const unsigned* off, int n, unsigned cap, int32_t* index,
                              const Keypoint* kp, Keypoint* kp_out, hipStream_t st);

// Guided descriptor matching (sift_guided.hip; the definition is in include/sift_hip.h).
constexpr int kGuidedMaxCells = 1 << 20;
constexpr int kGuidedMatchBlocks = 8192;  // one-wave blocks of one match launch: 32 waves on each of 256 CUs
struct GuidedGrid {
  int cell_px, ncx, ncy;
};
// The grid of the definition for a train size and a radius (both validated).
GuidedGrid guided_grid(int width, int height, double radius);
// The train rows in cell order: slot j holds a row's position, (index, squared norm) and 128 bytes.
struct GuidedFiled {
  double2* xy;
  int2* tag;
  unsigned char* rows;
};
struct GuidedMatch {
  const unsigned char* query;   // n_query x 128, 16-byte aligned
  const unsigned char* qmask;   // or nullptr
  const double2* qxy;
  int n_query;
  double h[9], radius, r2;
  GuidedGrid grid;
  const unsigned* off;          // cells + 1: the exclusive scan of the cell counts
  GuidedFiled filed;
  Match* out;
  unsigned long long* info;     // projected rows, visited rows, candidates: added to (zeroed by the caller)
};
// xy[r] = (abs_x, abs_y) of the keypoint record r names; NaNs when the index is outside the list.
hipError_t launch_guided_gather(const Orientation* ori, int n, const Keypoint* kp, int n_kp, double2* xy,
                                hipStream_t st);
// cell[i] of the n train rows (-1: masked or a NaN coordinate); count[c] += 1 (cells + 1 zeroed words).
hipError_t launch_guided_cells(const double2* xy, const unsigned char* mask, int n, const GuidedGrid& g, int* cell,
                               unsigned* count, hipStream_t st);
// Files the rows with cell[i] >= 0: off = the exclusive scan of count, which is counted back down to zero.
hipError_t launch_guided_fill(const unsigned char* rows, const double2* xy, const int* cell, int n, const unsigned* off,
                              unsigned* count, const GuidedFiled& F, hipStream_t st);
hipError_t launch_guided_match(const GuidedMatch& M, hipStream_t st);

// Image products either side of the path (sift_image.hip).
// gray/alpha rows are dense (w floats); alpha may be nullptr.
hipError_t launch_rgba_to_gray(const unsigned char* rgba, size_t stride_bytes, int w, int h, float* gray,
                               float* alpha, hipStream_t st);
// float2 partials needed by the sampled mode for an n-pixel plane.
int plane_image_parts(long long n);
hipError_t launch_plane_image(const float* plane, long long n, int mode, double coefficient, float2* parts,
                              unsigned* out, hipStream_t st);

// Homography warp (sift_warp.hip; the definition is in include/sift_hip.h).  m: nine host doubles, destination
// pixel -> source position; strides in pixels (an RGBA pixel is one word); mask (dense, dw * dh bytes) and count
// (one word, set to the valid pixels) may be nullptr; partial: kWarpMaxBlocks words of scratch, used when count is
// given.  0 < dw * dh < 2^31.
constexpr int kWarpMaxBlocks = 4096;  // blocks of one warp launch: two rounds of 8 blocks on each of 256 CUs
hipError_t launch_warp_gray(const float* src, int sw, int sh, size_t sstride_px, const double* m, bool bilinear,
                            float fill, float* dst, int dw, int dh, size_t dstride_px, unsigned char* mask,
                            unsigned* partial, unsigned* count, hipStream_t st);
hipError_t launch_warp_rgba(const unsigned* src, int sw, int sh, size_t sstride_px, const double* m, bool bilinear,
                            unsigned fill, unsigned* dst, int dw, int dh, size_t dstride_px, unsigned char* mask,
                            unsigned* partial, unsigned* count, hipStream_t st);

}  // namespace sift
