// C ABI of the RANSAC homography verification of match pairs (kernels: sift_verify.hip).
#include "sift_ctx.h"

using namespace sift;

static_assert(sizeof(sift_point_pair) == 32 && sizeof(PointPair) == 32 && sizeof(sift_homography) == 80 &&
                  sizeof(Homography) == 80 && SIFT_RANSAC_MAX_HYPOTHESES == kMaxHypotheses,
              "verification records and limits of include/sift_hip.h");

static int verify_check(sift_ctx* ctx, const void* points, size_t n, size_t K, double thresh) {
  if (!count_ok(n)) return set_err(ctx, SIFT_E_ARG, "too many pairs");
  if (K > (size_t)kMaxHypotheses) return set_err(ctx, SIFT_E_ARG, "more than SIFT_RANSAC_MAX_HYPOTHESES hypotheses");
  if (!(std::isfinite(thresh) && thresh > 0.0)) return set_err(ctx, SIFT_E_ARG, "thresh must be finite and > 0");
  if (n && !points) return set_err(ctx, SIFT_E_ARG, "null pairs");
  return SIFT_OK;
}

// counts[k] of validated device arrays (K > 0), between the scoring's two events; not waited for.
static int score_enqueue(sift_ctx* ctx, const PointPair* pts, int n, const double* H, int K, double t2, int* counts) {
  HIPCHK(hipEventRecord(ctx->verify.ev[2], ctx->stream));
  HIPCHK(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int), ctx->stream));
  HIPCHK(launch_homography_score(pts, n, H, K, t2, counts, ctx->stream));
  HIPCHK(hipEventRecord(ctx->verify.ev[3], ctx->stream));
  return SIFT_OK;
}

static int score_run(sift_ctx* ctx, const PointPair* pts, size_t n, const double* H, size_t K, double thresh,
                     int* counts) {
  VerifyState& V = ctx->verify;
  HIPCHK(V.ev.ensure());
  V.score_ms = 0;
  if (!K) return SIFT_OK;
  if (int rc = score_enqueue(ctx, pts, (int)n, H, (int)K, thresh * thresh, counts)) return rc;
  HIPCHK(hipEventSynchronize(V.ev[3]));
  V.score_ms = event_ms(V.ev[2], V.ev[3]);
  return SIFT_OK;
}

// RANSAC over validated device points: the model and the count always, the
// list into d_inliers when it is given and cap holds it.
static int ransac_run(sift_ctx* ctx, const PointPair* pts, size_t n, size_t K, uint64_t seed, double thresh,
                      sift_homography* model, int32_t* d_inliers, size_t cap, size_t* n_inliers) {
  VerifyState& V = ctx->verify;
  HIPCHK(V.ev.ensure());
  V.hyp_ms = V.score_ms = V.select_ms = 0;
  V.n_hyp = 0;
  V.have = n < 4 || K == 0;  // no hypothesis is formed: the last RANSAC is an empty one
  if (V.have) {
    std::memset(model, 0, sizeof *model);
    model->hypothesis = -1;
    if (n_inliers) *n_inliers = 0;
    return SIFT_OK;
  }
  const int ni = (int)n, Ki = (int)K;
  const double t2 = thresh * thresh;
  HIPCHK(V.H.ensure(K * 9 * sizeof(double)));
  HIPCHK(V.valid.ensure(K * sizeof(int)));
  HIPCHK(V.cnt.ensure(K * sizeof(int)));
  HIPCHK(V.model.ensure(sizeof(Homography)));
  HIPCHK(V.flag.ensure((n + 1) * sizeof(unsigned)));
  HIPCHK(V.off.ensure((n + 1) * sizeof(unsigned)));
  Homography* h_model = &static_cast<StageScratch*>(ctx->hscratch.p)->model;
  HIPCHK(hipEventRecord(V.ev[0], ctx->stream));
  HIPCHK(launch_homography_hypotheses(pts, ni, Ki, seed, V.H.as<double>(), V.valid.as<int>(), ctx->stream));
  HIPCHK(hipEventRecord(V.ev[1], ctx->stream));
  if (int rc = score_enqueue(ctx, pts, ni, V.H.as<double>(), Ki, t2, V.cnt.as<int>())) return rc;
  HIPCHK(hipEventRecord(V.ev[4], ctx->stream));
  HIPCHK(launch_homography_best(V.H.as<double>(), V.valid.as<int>(), V.cnt.as<int>(), Ki, V.model.as<Homography>(),
                                ctx->stream));
  HIPCHK(launch_inlier_flag(pts, ni, V.model.as<Homography>(), t2, V.flag.as<unsigned>(), ctx->stream));
  // the model record rides on the synchronisation of the count
  HIPCHK(hipMemcpyAsync(h_model, V.model.p, sizeof(Homography), hipMemcpyDeviceToHost, ctx->stream));
  unsigned total = 0;
  if (int rc = ordered_total(ctx, V.flag.as<unsigned>(), V.off.as<unsigned>(), ni, &total)) return rc;
  std::memcpy(model, h_model, sizeof *model);
  if (n_inliers) *n_inliers = total;
  const bool fits = cap >= total;
  if (d_inliers && fits)
    HIPCHK(launch_inlier_emit(V.flag.as<unsigned>(), V.off.as<unsigned>(), ni, total, d_inliers, ctx->stream));
  HIPCHK(hipEventRecord(V.ev[5], ctx->stream));
  HIPCHK(hipEventSynchronize(V.ev[5]));
  V.hyp_ms = event_ms(V.ev[0], V.ev[1]);
  V.score_ms = event_ms(V.ev[2], V.ev[3]);
  V.select_ms = event_ms(V.ev[4], V.ev[5]);
  V.n_hyp = K;
  V.have = true;
  if (d_inliers && !fits) return set_err(ctx, SIFT_E_CAPACITY, "inlier buffer too small");
  return SIFT_OK;
}

// ransac_run with the list through ctx->verify.inl into host memory.
static int ransac_to_host(sift_ctx* ctx, const PointPair* pts, size_t n, size_t K, uint64_t seed, double thresh,
                          sift_homography* model, int32_t* inliers, size_t cap, size_t* n_inliers) {
  VerifyState& V = ctx->verify;
  if (inliers) HIPCHK(V.inl.ensure(std::max<size_t>(n, 1) * sizeof(int32_t)));
  size_t total = 0;
  if (!n_inliers) n_inliers = &total;
  if (int rc = ransac_run(ctx, pts, n, K, seed, thresh, model, inliers ? V.inl.as<int32_t>() : nullptr, cap, n_inliers))
    return rc;
  if (inliers && *n_inliers) HIPCHK(d2h_staged(ctx, inliers, V.inl.p, *n_inliers * sizeof(int32_t)));
  return SIFT_OK;
}

// Both sides have the orientation records the pairs index, on one device.
static int pair_points_check(sift_ctx* ctx, sift_ctx* train_ctx) {
  if (!stage_has(ctx, kNeedOri) || !stage_has(train_ctx, kNeedOri))
    return set_err(ctx, SIFT_E_STATE, "no orientations: run sift_orient on both contexts first");
  if (ctx->device != train_ctx->device) return set_err(ctx, SIFT_E_ARG, "contexts on different devices");
  return SIFT_OK;
}

static int pair_points_enqueue(sift_ctx* ctx, sift_ctx* train_ctx, const MatchPair* d_pairs, size_t n,
                               PointPair* d_points) {
  const FeatState &Q = ctx->feat, &T = train_ctx->feat;
  HIPCHK(launch_pair_points(d_pairs, (int)n, Q.ori.as<Orientation>(), (int)Q.n_ori, ctx->kp.as<Keypoint>(),
                            (int)ctx->n_kp, T.ori.as<Orientation>(), (int)T.n_ori, train_ctx->kp.as<Keypoint>(),
                            (int)train_ctx->n_kp, d_points, ctx->stream));
  return SIFT_OK;
}

int sift_homography_score_device(sift_ctx* ctx, const sift_point_pair* d_points, size_t n, const double* d_H, size_t K,
                                 double thresh, int32_t* d_counts) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = verify_check(ctx, d_points, n, K, thresh)) return rc;
  if (K && (!d_H || !d_counts)) return set_err(ctx, SIFT_E_ARG, "null matrices or counts");
  HIPCHK(hipSetDevice(ctx->device));
  return score_run(ctx, reinterpret_cast<const PointPair*>(d_points), n, d_H, K, thresh, d_counts);
}

int sift_homography_score(sift_ctx* ctx, const sift_point_pair* points, size_t n, const double* H, size_t K,
                          double thresh, int32_t* counts) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = verify_check(ctx, points, n, K, thresh)) return rc;
  if (K && (!H || !counts)) return set_err(ctx, SIFT_E_ARG, "null matrices or counts");
  HIPCHK(hipSetDevice(ctx->device));
  if (!K) return score_run(ctx, nullptr, n, nullptr, 0, thresh, nullptr);
  VerifyState& V = ctx->verify;
  if (int rc = h2d_buffer(ctx, V.in_pts, points, n * sizeof(PointPair))) return rc;
  if (int rc = h2d_buffer(ctx, V.in_H, H, K * 9 * sizeof(double))) return rc;
  HIPCHK(V.in_cnt.ensure(K * sizeof(int)));
  if (int rc = score_run(ctx, V.in_pts.as<PointPair>(), n, V.in_H.as<double>(), K, thresh, V.in_cnt.as<int>()))
    return rc;
  HIPCHK(d2h_staged(ctx, counts, V.in_cnt.p, K * sizeof(int)));
  return SIFT_OK;
}

int sift_homography_ransac_device(sift_ctx* ctx, const sift_point_pair* d_points, size_t n, size_t K, uint64_t seed,
                                  double thresh, sift_homography* model, int32_t* d_inliers, size_t cap,
                                  size_t* n_inliers) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = verify_check(ctx, d_points, n, K, thresh)) return rc;
  if (!model) return set_err(ctx, SIFT_E_ARG, "null model");
  HIPCHK(hipSetDevice(ctx->device));
  return ransac_run(ctx, reinterpret_cast<const PointPair*>(d_points), n, K, seed, thresh, model, d_inliers, cap,
                    n_inliers);
}

int sift_homography_ransac(sift_ctx* ctx, const sift_point_pair* points, size_t n, size_t K, uint64_t seed,
                           double thresh, sift_homography* model, int32_t* inliers, size_t cap, size_t* n_inliers) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = verify_check(ctx, points, n, K, thresh)) return rc;
  if (!model) return set_err(ctx, SIFT_E_ARG, "null model");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = h2d_buffer(ctx, ctx->verify.in_pts, points, n * sizeof(PointPair))) return rc;
  return ransac_to_host(ctx, ctx->verify.in_pts.as<PointPair>(), n, K, seed, thresh, model, inliers, cap, n_inliers);
}

int sift_copy_homography_hypotheses(sift_ctx* ctx, double* H, int32_t* counts, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (!ctx->verify.have) return set_err(ctx, SIFT_E_STATE, "no RANSAC: run sift_homography_ransac first");
  const size_t K = ctx->verify.n_hyp;
  if (n_out) *n_out = K;
  if ((!H && !counts) || !K) return SIFT_OK;
  if (cap < K) return set_err(ctx, SIFT_E_CAPACITY, "hypothesis buffer too small");
  HIPCHK(hipSetDevice(ctx->device));
  if (H) HIPCHK(d2h_staged(ctx, H, ctx->verify.H.p, K * 9 * sizeof(double)));
  if (counts) HIPCHK(d2h_staged(ctx, counts, ctx->verify.cnt.p, K * sizeof(int)));
  return SIFT_OK;
}

int sift_pair_points_device(sift_ctx* ctx, sift_ctx* train_ctx, const sift_match_pair* d_pairs, size_t n,
                            sift_point_pair* d_points) {
  if (!ctx || !train_ctx) return SIFT_E_ARG;
  if (!count_ok(n)) return set_err(ctx, SIFT_E_ARG, "too many pairs");
  if (n && (!d_pairs || !d_points)) return set_err(ctx, SIFT_E_ARG, "null pairs or points");
  if (int rc = pair_points_check(ctx, train_ctx)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = pair_points_enqueue(ctx, train_ctx, reinterpret_cast<const MatchPair*>(d_pairs), n,
                                   reinterpret_cast<PointPair*>(d_points)))
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_verify_features(sift_ctx* ctx, sift_ctx* train_ctx, const sift_match_pair* pairs, size_t n, size_t K,
                         uint64_t seed, double thresh, sift_homography* model, int32_t* inliers, size_t cap,
                         size_t* n_inliers) {
  if (!ctx || !train_ctx) return SIFT_E_ARG;
  if (int rc = verify_check(ctx, pairs, n, K, thresh)) return rc;
  if (!model) return set_err(ctx, SIFT_E_ARG, "null model");
  if (int rc = pair_points_check(ctx, train_ctx)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  VerifyState& V = ctx->verify;
  if (int rc = h2d_buffer(ctx, V.pairs, pairs, n * sizeof(MatchPair))) return rc;
  HIPCHK(V.pts.ensure(std::max<size_t>(n, 1) * sizeof(PointPair)));
  if (int rc = pair_points_enqueue(ctx, train_ctx, V.pairs.as<MatchPair>(), n, V.pts.as<PointPair>())) return rc;
  return ransac_to_host(ctx, V.pts.as<PointPair>(), n, K, seed, thresh, model, inliers, cap, n_inliers);
}

int sift_last_verify_timings(sift_ctx* ctx, double* hypotheses_ms, double* score_ms, double* select_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (hypotheses_ms) *hypotheses_ms = ctx->verify.hyp_ms;
  if (score_ms) *score_ms = ctx->verify.score_ms;
  if (select_ms) *select_ms = ctx->verify.select_ms;
  return SIFT_OK;
}
