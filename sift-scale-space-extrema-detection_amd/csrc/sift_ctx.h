// The context behind the C ABI and what its host files share (sift_api.hip,
// sift_api_feature / _match / _verify / _refit.hip).  No kernel file includes this.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
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

// Pinned read-backs of those stages (sift_ctx::hscratch): one of each serves them all, since every user synchronises.
struct StageScratch {
  Homography model;  // the RANSAC's; a fit's
  unsigned word;     // a count
};

// Defined in sift_api.hip, where each is described.
hipError_t exclusive_sum(sift_ctx* ctx, unsigned* in, unsigned* out, int n);
hipError_t d2h_staged(sift_ctx* ctx, void* dst, const void* src, size_t bytes);
int h2d_buffer(sift_ctx* ctx, DBuf& b, const void* src, size_t bytes);
double event_ms(hipEvent_t a, hipEvent_t b);
bool count_ok(size_t n);
int ordered_total(sift_ctx* ctx, unsigned* counts, unsigned* offsets, int n, unsigned* total);
enum StageNeed { kNeedKp = 1, kNeedOri = 2, kNeedDesc = 3 };
bool stage_has(const sift_ctx* c, StageNeed need);

}  // namespace sift

struct sift_ctx {
  using DBuf = sift::DBuf;
  using HBuf = sift::HBuf;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;          // false: the stream of another context (sift_ctx_create_shared)
  std::string err;
  sift_params p{};
  int W = 0, H = 0;
  std::vector<int> dims;           // 2*O
  std::vector<double> blur, sigma; // O*NS
  sift::Pyramid P{};
  sift::GaussPlan gplan[sift::kMaxOctaves]{};  // of P's octaves (setup_geometry)
  int dog_source = sift::kNone;
  bool have_gauss = false;
  bool have_cand = false;
  size_t n_cand = 0, n_low = 0, n_kp = 0, n_sing = 0, n_exact = 0;
  size_t n_slots = 0;       // candidate slots (n_cand + entries dropped by the exact pass)
  bool want_low = false;    // this extrema stage lists the low-contrast extrema
  bool have_low = false;    // the last extrema stage did (sift_copy_low_contrast)
  unsigned low_cap = 0;     // slots of the ordered low-contrast list
  size_t n_low_sure = 0, n_low_late = 0;  // ordered (certain) and exact-pass (late) low-contrast entries
  unsigned cand_cap = 0;    // capacity of the candidate slot arrays (extrema path)
  unsigned amb_cap = 0;     // capacity of the ambiguous-key list
  int slot_cap = 0;         // slots the refinement runs over
  bool ext_pending = false; // extrema launched, counts not yet read back
  bool has_keep = false;    // slots carry keep flags
  bool slots_rows = false;  // slots are the extrema stage's emission (row offsets in rowoff): band order applies
  bool counters_zeroed = false;  // extrema_prepare zeroed the refinement counters too
  bool detect_pending = false;   // sift_detect_device_async enqueued, sift_detect_wait not yet called
  bool begin_pending = false;    // sift_detect_begin_async enqueued, sift_detect_end_async not yet called
  bool detect_host_img = false;
  sift::ExtremaLaunch xl{}; // extrema launch state between prepare / scan / finish; xl.G is the bitmap
                            // geometry of this extrema stage (bitmap_geometry), which every later launch copies
  int o_first = 0;          // first octave of the pyramid in use (sift_detect_from_seed: > 0)
  int scan_first = 0;       // first octave the extrema stage scans (>= o_first; sift_detect_from_seed_range)
  int planes_first = 0;     // first octave with Gaussian / DoG planes (below: only its successor's base)
  int row0 = 0;             // sift_set_row_origin: input row of the image's first row
  int xseed_h = 0, xseed_w = 0;  // SIFT_F_EXPORT_NEXT_SEED: the base of octave O
  bool has_xseed = false;
  bool has_origins = false; // kp_key holds the candidate key of every keypoint
  int x_nf = 0;             // leading octaves whose extrema decisions run fused into the Gaussian pass
  bool x_prepared = false;  // extrema_prepare already ran for this detection (fused octaves)
  // device memory
  DBuf img, seeds, gauss, dog, wts;
  DBuf base0;                                  // materialised octave-0 base (large radii only)
  DBuf l64;                                    // fp64 Gaussian planes of the large-radius octaves
  DBuf vsplit;                                 // vertical-sum scratch of the split-pass octaves (one at a time)
  DBuf seedv;                                  // vertical sums of the seed-only octaves (launch_seed_only)
  long long vsplit_pi = 0;                     // ... doubles per image of a batch
  std::vector<double> wts_host;                // taps last uploaded to wts
  // Taps of the deepest schedule built so far (setup_geometry): per-(octave,
  // scale) sigma, the padded tap vector, its length after each octave, and
  // every scale's radius and tap offset.  Sigma does not depend on the octave
  // count, so a schedule whose sigmas are a prefix of these reuses a prefix
  // of the taps instead of ~3 K exp() per call (8K O6 S5: ~35 us).
  struct TapCache {
    int NS = 0;
    std::vector<double> sigma, w;
    std::vector<size_t> oct_end;
    std::vector<int> rad, wofs;
  } taps;
  DBuf bitmap, rowcount, rowoff, amb_keys;     // extrema scan
  DBuf ambbitmap;                              // ambiguous words (k_exact_words)
  bool x_words = false;                        // this extrema stage lists ambiguous words, not keys
  DBuf cand_key, cand_val, cand_keep;          // ordered candidates
  DBuf lowbitmap, lowrowcount, lowrowoff;      // low-contrast list (SIFT_F_LOW_CONTRAST_LIST)
  DBuf low_key, low_val, late_key, late_val;
  DBuf keep, pos;                              // keypoint compaction
  DBuf keep_tile;                              // ... its per-tile counts (launch_keep_compact)
  DBuf band_cnt, band_first, band_start, perm;  // refinement band order
  DBuf status, kp_tmp, kp, uncertain;          // refinement
  DBuf kp_soa;                                 // keypoint field arrays for a DMA into registered host arrays
  DBuf xseed, kp_key;                          // next-octave base, keypoint origins
  DBuf merge_tab;                              // sift_merge_keypoint_blocks_device tables
  bool have_kp = false;                        // a refinement has settled on this pyramid: kp / n_kp are its list
  sift::FeatState feat;
  sift::MatchState match;
  sift::VerifyState verify;
  sift::RefitState refit;
  HBuf hscratch;                               // pinned: one sift::StageScratch (sift_ctx_create)
  DBuf counters, temp;
  DBuf rgba, alpha, display, mm_parts;         // image products (sift_image.hip)
  unsigned* h_counters = nullptr;              // pinned mirror of counters (+ per-block keypoint counts at kBlk)
  int own_lo = -1, own_hi = -1;                // sift_set_owned_rows
  std::vector<long long> blk_counts;           // kept keypoints per (octave, scale) of the last refinement
  HBuf himg, hkp;                  // pinned staging: host images in, keypoint records out
  hipEvent_t ev_himg = nullptr;    // the DMA out of himg is done (himg may be refilled)
  HBuf hpl;                        // pinned staging of plane reads: two halves, double-buffered
  sift::EventSet<2, hipEventDisableTiming> ev_pl;
  sift::EventSet<8> ev;
  hipEvent_t ev_heavy = nullptr;  // after the last bandwidth-heavy kernel of a detection (sift_order_after)
  sift::EventSet<sift::kMaxOctaves> ev_go;  // after octave o's Gaussian+DoG launch (per-octave timings)
  sift_timings tm{};
  std::vector<double> oct_ms;      // per-octave Gaussian+DoG launch time of the last build
  std::vector<std::string> pass_kn; // per-octave pass kernels of the last build (sift_last_pass_kernels)

  // The buffers and the event sets free themselves; the caller has made `device` current and the stream is idle.
  ~sift_ctx() {
    if (ev_heavy) (void)hipEventDestroy(ev_heavy);
    if (ev_himg) (void)hipEventDestroy(ev_himg);
    if (h_counters) (void)hipHostFree(h_counters);
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
