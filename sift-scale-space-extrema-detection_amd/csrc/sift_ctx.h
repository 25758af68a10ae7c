// The context behind the C ABI, its state grouped by stage, and what its host files share: sift_api.hip (lifetime,
// shared helpers), sift_api_pyramid / _extrema / _detect / _shard / _image.hip (detection) and sift_api_feature /
// _match / _verify / _refit / _warp / _budget / _guided.hip (later stages).  No kernel file includes this.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sift_hip.h"
#include "sift_kernels.h"

struct sift_ctx;
namespace sift {

// Grow-only buffer, freed with its owner: device memory (DBuf), or pinned host
// memory (HBuf: staging of host images and keypoint records, count read-backs).
template <bool kDevice>
struct Buf {
  void* p = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  hipError_t ensure(size_t need) {
    if (need <= bytes) return hipSuccess;
    release();
    size_t want = need + need / 4 + 256;
    hipError_t e = kDevice ? hipMalloc(&p, want) : hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) bytes = want;
    return e;
  }
  void release() {
    if (p) (void)(kDevice ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};
using DBuf = Buf<true>;
using HBuf = Buf<false>;

// Events created on first use (or all at once: sift_ctx_create), destroyed with their owner.
template <int N, unsigned kFlags = hipEventDefault>
struct EventSet {
  hipEvent_t e[N]{};
  EventSet() = default;
  EventSet(const EventSet&) = delete;
  EventSet& operator=(const EventSet&) = delete;
  ~EventSet() {
    for (auto x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipError_t ensure() {
    for (auto& x : e)
      if (hipError_t r = x ? hipSuccess : hipEventCreateWithFlags(&x, kFlags)) return r;
    return hipSuccess;
  }
  hipEvent_t operator[](int i) const { return e[i]; }
};

enum DogSource { kNone = 0, kNative = 1, kForeign = 2 };

// Orientation and descriptor stages (sift_api_feature.hip) over the refinement's list (sift_ctx::kp).
struct FeatState {
  bool have_ori = false, have_desc = false;    // ori / desc hold the records of that list
  size_t n_ori = 0, n_desc_ok = 0;             // records, described records
  DBuf ori_count, ori_off, ori_mask, ori_theta;  // per keypoint: peaks, their exclusive scan, bins, angles
  DBuf ori, desc, desc_ok, desc_n;             // records, 128 bytes each, described flags, described count
  EventSet<4> ev;                               // around the orientation stage [0, 1] and the descriptor stage [2, 3]
  double orient_ms = 0, describe_ms = 0;
};

// Descriptor matching (sift_api_match.hip).
struct MatchState {
  DBuf qs, ts, qn, kb;                         // shifted, padded query / train rows; query norms, train key bases
  DBuf part, out;                              // per-split partial records; the last match's records
  DBuf in_q, in_t, in_qm, in_tm;               // host-form inputs (sift_match)
  DBuf fwd, rev, flag, off, pairs;             // selection: host-form inputs, flags, their scan, host-form pairs
  size_t n = 0; bool have = false;             // records in out
  EventSet<4> ev;                               // around the match [0, 1] and the selection [2, 3]
  double match_ms = 0, select_ms = 0;
};

// Homography verification (sift_api_verify.hip).
struct VerifyState {
  DBuf H, valid, cnt, model;                   // the last RANSAC's hypotheses, valid flags, counts; its model record
  DBuf flag, off;                              // inlier flags of the best model, their scan
  DBuf in_pts, in_H, in_cnt, pairs;            // host-form inputs and counts (sift_homography_score, sift_verify_features)
  DBuf pts, inl;                               // gathered points (sift_verify_features); host-form inlier list
  size_t n_hyp = 0; bool have = false;         // hypotheses in H / cnt
  EventSet<6> ev;                               // around the hypotheses [0, 1], the scoring [2, 3], the selection [4, 5]
  double hyp_ms = 0, score_ms = 0, select_ms = 0;
};

// Least-squares fit and refit of the inliers (sift_api_refit.hip).
struct RefitState {
  DBuf keys, parts_a, parts_b, rec;            // one fit: box keys, the tree's levels (ping-pong), its FitRecord
  DBuf start, flag, off;                       // the rounds: the start's model record, inlier flags, their scan
  DBuf list[2];                                // ... the accepted inlier list (cur) and the round's candidate
  DBuf in_pts, in_idx;                         // host-form inputs (sift_homography_fit, sift_homography_refit)
  int cur = 0; size_t n_list = 0;              // the last refit's list: list[cur][0 .. n_list)
  bool have_fit = false;                       // rec holds a fit (box and sums included)
  EventSet<3> ev;                              // a round: before the fit [0], after it [1], after the rescoring [2]
  double fit_ms = 0, rescore_ms = 0;
};

// Homography warp (sift_api_warp.hip).
struct WarpState {
  DBuf src, dst, mask;                         // host-form staging: the source, the destination, the mask (all dense)
  DBuf count;                                  // the last counted warp: its valid pixels, then one word per block
  EventSet<2> ev;                              // around the kernels
  double warp_ms = 0;
};

// Keypoint budget (sift_api_budget.hip).
struct BudgetState {
  DBuf key, cell;                              // per record: strength key, grid cell
  DBuf tkey, ttail, rem, hist;                 // per cell: threshold key and tail, quota left; 256 bins
  DBuf surv, flag, off;                        // per record: step 1's survivors, the kept flags, their scan
  DBuf in_kp, idx;                             // host-form input records and index list (sift_keypoint_select)
  DBuf kp2;                                    // sift_limit_keypoints gathers into it, then swaps it with sift_ctx::kp
  DBuf sel; size_t n_sel = 0;                  // the indices the last sift_limit_keypoints kept,
  bool have_sel = false;                       // ... while its list is the context's list
  EventSet<2> ev;                              // around one selection
  double select_ms = 0;
};

// Guided descriptor matching (sift_api_guided.hip); the host and features forms leave their records in MatchState::out.
struct GuidedState {
  DBuf cell, count, off;                       // per train row: its cell; per cell (+ 1): rows, their exclusive scan
  DBuf fxy, ftag, frows;                       // the train rows filed in cell order (GuidedFiled)
  DBuf info;                                   // three 64-bit sums of the last match
  DBuf in_q, in_t, in_qm, in_tm, in_qxy, in_txy;  // host-form inputs; the features form gathers into in_qxy / in_txy
  HBuf hinfo;                                  // pinned read-back of info
  sift_guided_info last{};                     // of the last guided match,
  bool have = false;                           // ... when there was one
  EventSet<3> ev;                              // before the filing [0], between it and the match [1], after it [2]
  double grid_ms = 0, match_ms = 0;
};

// Taps of the deepest schedule built so far (setup_geometry): per-(octave, scale) sigma, the padded tap vector, its
// length after each octave, and every scale's radius and tap offset.  Sigma does not depend on the octave count, so a
// schedule whose sigmas are a prefix of these reuses a prefix of the taps, not ~3 K exp() per call (8K O6 S5: ~35 us).
struct TapCache {
  int NS = 0;
  std::vector<double> sigma, w;
  std::vector<size_t> oct_end;
  std::vector<int> rad, wofs;
};

// The Gaussian + DoG pyramid (sift_api_pyramid.hip).
struct PyrState {
  std::vector<int> dims;                       // 2*O
  std::vector<double> blur, sigma;             // O*NS
  GaussPlan gplan[kMaxOctaves]{};              // of P's octaves (setup_geometry)
  GaussLaunched glaunch[kMaxOctaves]{};        // what the last build launched for each (sift_last_gauss_plan)
  int dog_source = kNone;                      // who supplied the DoG planes
  bool have_gauss = false;                     // the Gaussian planes are materialised
  int o_first = 0;                             // first octave of the pyramid in use (sift_detect_from_seed: > 0)
  int scan_first = 0;                          // first octave the extrema stage scans (>= o_first; ..._from_seed_range)
  int planes_first = 0;                        // first octave with Gaussian / DoG planes (below: its successor's base)
  DBuf img, seeds, gauss, dog, wts;            // image, octave bases, planes, taps
  DBuf base0;                                  // materialised octave-0 base (large radii only)
  DBuf l64;                                    // fp64 Gaussian planes of the large-radius octaves
  DBuf vsplit;                                 // vertical-sum scratch of the split-pass octaves (one at a time)
  long long vsplit_pi = 0;                     // ... doubles per image of a batch
  DBuf seedv;                                  // vertical sums of the seed-only octaves (launch_seed_only)
  std::vector<double> wts_host;                // taps last uploaded to wts
  TapCache taps;
  HBuf himg;                                   // pinned staging of host images
  EventSet<1, hipEventDisableTiming> ev_himg;  // the DMA out of himg is done (himg may be refilled)
  EventSet<kMaxOctaves> ev_go;                 // after octave o's Gaussian+DoG launch (per-octave timings)
  std::vector<double> oct_ms;                  // per-octave Gaussian+DoG launch time of the last build
  std::vector<std::string> pass_kn;            // per-octave pass kernels of the last build (sift_last_pass_kernels)
};

// The extrema stage (sift_api_extrema.hip) and its candidate slots.
struct ExtState {
  unsigned cand_cap = 0, amb_cap = 0, low_cap = 0;  // slots of the candidate arrays, ambiguous keys, low-contrast list
  int slot_cap = 0;                            // slots the refinement runs over
  DBuf bitmap, rowcount, rowoff, amb_keys;     // extrema scan
  DBuf ambbitmap;                              // ambiguous words (k_exact_words)
  DBuf cand_key, cand_val, cand_keep;          // ordered candidates
  DBuf lowbitmap, lowrowcount, lowrowoff;      // low-contrast list (SIFT_F_LOW_CONTRAST_LIST)
  DBuf low_key, low_val, late_key, late_val;
  ExtremaLaunch xl{};                          // launch state between prepare / scan / finish; xl.G is the bitmap
                                               // geometry of this stage, which every later launch copies
  int nf = 0;                                  // leading octaves whose decisions run fused into the Gaussian pass
  bool prepared = false;                       // extrema_prepare already ran for this detection (fused octaves)
  bool words = false;                          // this stage lists ambiguous words, not keys
  bool want_low = false, have_low = false;     // this stage lists the low-contrast extrema; the last one did
  bool has_keep = false;                       // slots carry keep flags
  bool slots_rows = false;                     // slots are this stage's emission (row offsets in rowoff): band order
  bool counters_zeroed = false;                // extrema_prepare zeroed the refinement counters too
  bool pending = false;                        // launched, counts not yet read back
  bool have_cand = false;                      // the counts below are those of this pyramid's candidates
  size_t n_cand = 0, n_low = 0, n_exact = 0;
  size_t n_slots = 0;                          // candidate slots (n_cand + entries dropped by the exact pass)
  size_t n_low_sure = 0, n_low_late = 0;       // ordered (certain) and exact-pass (late) low-contrast entries
};

// Refinement and keypoint compaction (sift_api_detect.hip); the list itself is sift_ctx::kp.
struct RefState {
  DBuf status, kp_tmp, uncertain;              // per slot: outcome, record, the uncertain slots
  DBuf keep, pos, keep_tile;                   // compaction: flags, their scan, per-tile counts (launch_keep_compact)
  DBuf band_cnt, band_first, band_start, perm;  // band order
  DBuf kp_soa;                                 // keypoint field arrays for a DMA into registered host arrays
  HBuf hkp;                                    // pinned staging of keypoint records
  size_t n_sing = 0;                           // singular Hessians of the last refinement
  std::vector<long long> blk_counts;           // its kept keypoints per (octave, scale)
  EventSet<1, hipEventDisableTiming> ev_heavy;  // after a detection's last bandwidth-heavy kernel (sift_order_after)
};

// Row bands and tail pieces of a sharded image (sift_api_shard.hip).
struct ShardState {
  int own_lo = -1, own_hi = -1;                // sift_set_owned_rows
  int row0 = 0;                                // sift_set_row_origin: input row of the image's first row
  DBuf xseed; bool has_xseed = false;          // SIFT_F_EXPORT_NEXT_SEED: the base of octave O,
  int xseed_h = 0, xseed_w = 0;                // ... its rows and columns
  DBuf kp_key; bool has_origins = false;       // SIFT_F_KEYPOINT_ORIGINS: the candidate key of every keypoint
  DBuf merge_tab;                              // sift_merge_keypoint_blocks_device tables
};

// Image products either side of the path (sift_api_image.hip): uploaded RGBA, its alpha plane, a display image and
// the min / max partials behind it.
struct ImgState { DBuf rgba, alpha, display, mm_parts; };

// Slots of sift_ctx::ev, recorded on the context stream by one detection: before the image (or seed) upload; after
// it = before the Gaussian+DoG pass; after the pass (all octaves); around the extrema stage; around the refinement
// (kEvRefEnd: its counts are in h_counters); after the first octave's Gaussian+DoG launch.
enum CtxEvent { kEvUpload, kEvPass, kEvPassEnd, kEvExt, kEvExtEnd, kEvRef, kEvRefEnd, kEvOct0, kEvN };

// Pinned read-backs of the later stages (sift_ctx::hscratch): one of each serves them all, as every user synchronises.
struct StageScratch {
  Homography model;  // the RANSAC's; a fit's
  unsigned word;     // a count
};

// What one Gaussian+DoG build is given (build_common); a caller sets what it means.
struct BuildRequest {
  const float *img_host = nullptr, *img_dev = nullptr;    // the image, in host or in device memory (o_first == 0)
  int W = 0, H = 0;
  size_t stride = 0;                                      // pixels per image row
  const sift_params* p = nullptr;
  const double* sig = nullptr;                            // offset sigmas instead of the schedule's
  int o_first = 0;                                        // > 0: no image; octaves o_first .. O-1 from the fp64 base
  const double *seed_host = nullptr, *seed_dev = nullptr;  // ... of octave o_first, in host or in device memory
  bool fuse_extrema = false;  // a detection: octave 0's extrema decisions may run inside its pass
  int nimg = 1;               // > 1: a batch of images of one geometry, one launch per stage,
  size_t img_bstride = 0;     // ... image b at img + b * img_bstride
  int seed_only_below = 0;    // octaves below it only feed their successor's base (no planes)
};
inline BuildRequest image_request(const float* img_host, const float* img_dev, int W, int H, size_t stride,
                                  const sift_params* p) {
  return BuildRequest{img_host, img_dev, W, H, stride, p};
}
constexpr int kRetry = 1;  // internal return code: a capacity overflowed, grow and run again

// sift_api.hip, where each is described: what every stage shares.
hipError_t exclusive_sum(sift_ctx* ctx, unsigned* in, unsigned* out, int n);
hipError_t d2h_staged(sift_ctx* ctx, void* dst, const void* src, size_t bytes);
hipError_t h2d_rows_staged(void* dev, void* stage, const void* src, size_t spitch, size_t width, size_t rows, int nt,
                           hipStream_t st);
int h2d_buffer(sift_ctx* ctx, DBuf& b, const void* src, size_t bytes);
double event_ms(hipEvent_t a, hipEvent_t b);
void take_event_ms(double* ms, hipEvent_t a, hipEvent_t b);
bool count_ok(size_t n);
int ordered_total(sift_ctx* ctx, unsigned* counts, unsigned* offsets, int n, unsigned* total);
enum StageNeed { kNeedKp = 1, kNeedOri = 2, kNeedDesc = 3 };
bool stage_has(const sift_ctx* c, StageNeed need);
bool host_registered(const void* p, size_t bytes);  // [p, p + bytes) is page-locked (sift_host_register)
int host_threads();                                  // threads of the library's own host copies
int check_params(const sift_params* p);              // SIFT_OK, or why the parameters cannot be used
// sift_api_pyramid.hip
int build_common(sift_ctx* ctx, const BuildRequest& q);  // queues the upload and the Gaussian+DoG pass
long long total_plane_px(const sift_ctx* ctx);           // pixels of one plane of every octave
void read_gauss_times(sift_ctx* ctx);                    // the last build's pass timings (its events have completed)
int host_image_exit(sift_ctx* ctx, int rc);              // rc, after waiting for the image upload when rc is an error
int find_plane(sift_ctx* ctx, int kind, int o, int s, size_t cap_px, const char* too_small, const float** src,
               size_t* plane_px);  // device plane (kind, o, s) for a destination of cap_px pixels
// sift_api_extrema.hip
int extrema_prepare(sift_ctx* ctx, hipStream_t st, int nf);  // capacities, buffers, counter resets of one stage
int launch_extrema_stage(sift_ctx* ctx);                     // the whole stage, queued; the counts stay on the device
int settle_extrema(sift_ctx* ctx);                           // reads them from h_counters; kRetry after growing
// sift_api_detect.hip
void read_stage_times(sift_ctx* ctx, bool extrema, bool refine);  // waits for kEvRefEnd, then those stages' timings

// f(i0, i1) over a split of [0, n) into up to `nt` ranges, one per thread
// (the caller's included).
template <class F>
void par_for(size_t n, int nt, F f) {
  std::vector<std::thread> th;
  const size_t per = nt > 1 ? (n + nt - 1) / nt : n;
  for (int t = 1; t < nt; ++t) {
    const size_t i0 = std::min(n, t * per), i1 = std::min(n, (t + 1) * per);
    if (i0 < i1) th.emplace_back(f, i0, i1);
  }
  f((size_t)0, std::min(n, per));
  for (auto& x : th) x.join();
}

}  // namespace sift

struct sift_ctx {
  using DBuf = sift::DBuf;
  using HBuf = sift::HBuf;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;          // false: the stream of another context (sift_ctx_create_shared)
  std::string err;
  sift_params p{};
  sift::Pyramid P{};
  bool detect_pending = false;     // sift_detect_device_async enqueued, sift_detect_wait not yet called
  bool begin_pending = false;      // sift_detect_begin_async enqueued, sift_detect_end_async not yet called
  bool detect_host_img = false;    // that detection uploaded a host image (its h2d_ms is measured)
  sift::PyrState pyr;
  sift::ExtState ext;
  sift::RefState ref;
  sift::ShardState shard;
  sift::ImgState img;
  DBuf kp;                         // the refinement's keypoint list (or sift_set_keypoints')
  size_t n_kp = 0;
  bool have_kp = false;            // a refinement has settled on this pyramid: kp / n_kp are its list
  sift::FeatState feat;
  sift::MatchState match;
  sift::VerifyState verify;
  sift::RefitState refit;
  sift::WarpState warp;
  sift::BudgetState budget;
  sift::GuidedState guided;
  HBuf hscratch;                  // pinned: one sift::StageScratch (sift_ctx_create)
  DBuf counters, temp;             // kCntAll counter slots (sift_kernels.h); scan scratch
  HBuf h_counters;                 // pinned mirror of counters
  HBuf hpl;                        // pinned staging of plane reads: two halves, double-buffered
  sift::EventSet<2, hipEventDisableTiming> ev_pl;
  sift::EventSet<sift::kEvN> ev;   // sift::CtxEvent
  sift_timings tm{};

  // The buffers and the event sets free themselves; the caller has made `device` current and the stream is idle.
  ~sift_ctx() {
    if (stream && own_stream) (void)hipStreamDestroy(stream);
  }
};

#define HIPCHK(call)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
      return SIFT_E_HIP;                                                                    \
    }                                                                                       \
  } while (0)

inline int set_err(sift_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// Drops the results that a new refinement invalidates, and with `candidates` those a new pyramid does.
inline void drop_results(sift_ctx* ctx, bool candidates) {
  if (candidates) ctx->ext.have_cand = false;
  ctx->have_kp = ctx->feat.have_ori = ctx->feat.have_desc = ctx->budget.have_sel = false;
}

