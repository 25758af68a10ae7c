// C ABI of the least-squares homography fit and the refit of the RANSAC inliers (kernels: sift_refit.hip).
#include "sift_ctx.h"

using namespace sift;

static_assert(SIFT_REFIT_MAX_ROUNDS == kMaxRefitRounds && offsetof(FitRecord, model) == 0 &&
                  offsetof(FitRecord, sums) == offsetof(FitRecord, box) + 6 * sizeof(double),
              "refit limits of include/sift_hip.h; the model leads a FitRecord, the sums follow the box");

static int refit_check(sift_ctx* ctx, const void* points, size_t n, double thresh, int max_rounds) {
  if (!count_ok(n)) return set_err(ctx, SIFT_E_ARG, "too many pairs");
  if (max_rounds < 0 || max_rounds > kMaxRefitRounds)
    return set_err(ctx, SIFT_E_ARG, "max_rounds outside [0, SIFT_REFIT_MAX_ROUNDS]");
  if (!(std::isfinite(thresh) && thresh > 0.0)) return set_err(ctx, SIFT_E_ARG, "thresh must be finite and > 0");
  if (n && !points) return set_err(ctx, SIFT_E_ARG, "null pairs");
  return SIFT_OK;
}

// One fit of d_index[0 .. m) (nullptr: 0 .. m-1) over validated device points, m >= 4, into ctx->refit.rec; not
// waited for.
static int fit_enqueue(sift_ctx* ctx, const PointPair* pts, int n, const int32_t* d_index, int m) {
  RefitState& R = ctx->refit;
  const size_t c1 = (size_t)fit_chunks(m), c2 = (size_t)fit_chunks((long long)c1);
  HIPCHK(R.keys.ensure(kFitKeys * sizeof(unsigned long long)));
  HIPCHK(R.parts_a.ensure(c1 * kFitSums * sizeof(double)));
  HIPCHK(R.parts_b.ensure(c2 * kFitSums * sizeof(double)));
  HIPCHK(R.rec.ensure(sizeof(FitRecord)));
  HIPCHK(launch_homography_fit(pts, n, d_index, m, R.keys.as<unsigned long long>(), R.parts_a.as<double>(),
                               R.parts_b.as<double>(), R.rec.as<FitRecord>(), ctx->stream));
  R.have_fit = true;
  return SIFT_OK;
}

// The fit entry points behind their checks: h and *valid in host memory.
static int fit_run(sift_ctx* ctx, const PointPair* pts, size_t n, const int32_t* d_index, size_t m, double* h,
                   int* valid) {
  std::memset(h, 0, 9 * sizeof(double));
  if (valid) *valid = 0;
  if (m < 4) {  // no box, no sums
    ctx->refit.have_fit = false;
    return SIFT_OK;
  }
  if (int rc = fit_enqueue(ctx, pts, (int)n, d_index, (int)m)) return rc;
  Homography* h_model = &static_cast<StageScratch*>(ctx->hscratch.p)->model;
  HIPCHK(hipMemcpyAsync(h_model, ctx->refit.rec.p, sizeof(Homography), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::memcpy(h, h_model->h, 9 * sizeof(double));
  if (valid) *valid = h_model->hypothesis >= 0;
  return SIFT_OK;
}

// The rounds over validated device points.  *refined, *rounds and *n_inliers are set; the list is
// ctx->refit.list[cur][0 .. n_list) on return, and the stream is idle.
static int refit_run(sift_ctx* ctx, const PointPair* pts, size_t n, const sift_homography* start, double thresh,
                     int max_rounds, sift_homography* refined, int32_t* rounds, size_t* n_inliers) {
  RefitState& R = ctx->refit;
  HIPCHK(R.ev.ensure());
  R.fit_ms = R.rescore_ms = 0;
  R.cur = 0;
  R.n_list = 0;
  sift_homography best = *start;  // refined may be start
  unsigned count = 0;
  int accepted = 0;
  if (n) {
    const int ni = (int)n;
    const double t2 = thresh * thresh;
    HIPCHK(R.start.ensure(sizeof(Homography)));
    HIPCHK(R.rec.ensure(sizeof(FitRecord)));
    HIPCHK(R.flag.ensure((n + 1) * sizeof(unsigned)));
    HIPCHK(R.off.ensure((n + 1) * sizeof(unsigned)));
    for (DBuf& l : R.list) HIPCHK(l.ensure(n * sizeof(int32_t)));
    unsigned *flag = R.flag.as<unsigned>(), *off = R.off.as<unsigned>();
    Homography* h_model = &static_cast<StageScratch*>(ctx->hscratch.p)->model;
    // I0: the start's inliers (its h[8] as given; hypothesis 0 lets the flag kernel read it)
    std::memcpy(h_model->h, start->h, sizeof h_model->h);
    h_model->hypothesis = 0;
    h_model->inliers = 0;
    HIPCHK(hipMemcpyAsync(R.start.p, h_model, sizeof(Homography), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_inlier_flag(pts, ni, R.start.as<Homography>(), t2, flag, ctx->stream));
    if (int rc = ordered_total(ctx, flag, off, ni, &count)) return rc;
    HIPCHK(launch_inlier_emit(flag, off, ni, count, R.list[0].as<int32_t>(), ctx->stream));
    for (int r = 1; r <= max_rounds && count >= 4; ++r) {
      HIPCHK(hipEventRecord(R.ev[0], ctx->stream));
      if (int rc = fit_enqueue(ctx, pts, ni, R.list[R.cur].as<int32_t>(), (int)count)) return rc;
      HIPCHK(hipEventRecord(R.ev[1], ctx->stream));
      const Homography* d_model = &R.rec.as<FitRecord>()->model;
      HIPCHK(launch_inlier_flag(pts, ni, d_model, t2, flag, ctx->stream));  // an invalid fit flags nothing
      // the model record rides on the synchronisation of the count
      HIPCHK(hipMemcpyAsync(h_model, d_model, sizeof(Homography), hipMemcpyDeviceToHost, ctx->stream));
      unsigned total = 0;
      if (int rc = ordered_total(ctx, flag, off, ni, &total)) return rc;
      const bool accept = h_model->hypothesis >= 0 && total >= count;  // integers alone decide
      if (accept) HIPCHK(launch_inlier_emit(flag, off, ni, total, R.list[R.cur ^ 1].as<int32_t>(), ctx->stream));
      HIPCHK(hipEventRecord(R.ev[2], ctx->stream));
      HIPCHK(hipEventSynchronize(R.ev[2]));
      R.fit_ms += event_ms(R.ev[0], R.ev[1]);
      R.rescore_ms += event_ms(R.ev[1], R.ev[2]);
      if (!accept) break;
      const bool settled = total == count;
      std::memcpy(best.h, h_model->h, sizeof best.h);
      R.cur ^= 1;
      count = total;
      accepted = r;
      if (settled) break;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  best.inliers = (int32_t)count;
  R.n_list = count;
  *refined = best;
  if (rounds) *rounds = accepted;
  if (n_inliers) *n_inliers = count;
  return SIFT_OK;
}

// The last refit's list into caller memory (device or host) when cap holds it.
static int refit_list_out(sift_ctx* ctx, int32_t* dst, size_t cap, bool to_host) {
  const RefitState& R = ctx->refit;
  if (!dst) return SIFT_OK;
  if (cap < R.n_list) return set_err(ctx, SIFT_E_CAPACITY, "inlier buffer too small");
  if (!R.n_list) return SIFT_OK;
  const size_t bytes = R.n_list * sizeof(int32_t);
  if (to_host) {
    HIPCHK(d2h_staged(ctx, dst, R.list[R.cur].p, bytes));
  } else {
    HIPCHK(hipMemcpyAsync(dst, R.list[R.cur].p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return SIFT_OK;
}

int sift_homography_fit_device(sift_ctx* ctx, const sift_point_pair* d_points, size_t n, const int32_t* d_index,
                               size_t m, double* h, int* valid) {
  if (!ctx) return SIFT_E_ARG;
  if (!d_index) m = n;
  if (!count_ok(n) || !count_ok(m)) return set_err(ctx, SIFT_E_ARG, "too many pairs or list entries");
  if ((n && !d_points) || !h) return set_err(ctx, SIFT_E_ARG, "null pairs or matrix");
  HIPCHK(hipSetDevice(ctx->device));
  return fit_run(ctx, reinterpret_cast<const PointPair*>(d_points), n, d_index, m, h, valid);
}

int sift_homography_fit(sift_ctx* ctx, const sift_point_pair* points, size_t n, const int32_t* index, size_t m,
                        double* h, int* valid) {
  if (!ctx) return SIFT_E_ARG;
  if (!index) m = n;
  if (!count_ok(n) || !count_ok(m)) return set_err(ctx, SIFT_E_ARG, "too many pairs or list entries");
  if ((n && !points) || !h) return set_err(ctx, SIFT_E_ARG, "null pairs or matrix");
  if (index)
    for (size_t i = 0; i < m; ++i)
      if (index[i] < 0 || (size_t)index[i] >= n) return set_err(ctx, SIFT_E_ARG, "list entry outside the pairs");
  HIPCHK(hipSetDevice(ctx->device));
  RefitState& R = ctx->refit;
  if (int rc = h2d_buffer(ctx, R.in_pts, points, n * sizeof(PointPair))) return rc;
  if (int rc = h2d_buffer(ctx, R.in_idx, index, m * sizeof(int32_t))) return rc;
  return fit_run(ctx, R.in_pts.as<PointPair>(), n, index ? R.in_idx.as<int32_t>() : nullptr, m, h, valid);
}

int sift_copy_homography_fit_sums(sift_ctx* ctx, double* box, double* sums) {
  if (!ctx) return SIFT_E_ARG;
  if (!ctx->refit.have_fit) return set_err(ctx, SIFT_E_STATE, "no fit: run sift_homography_fit first");
  if (!box && !sums) return SIFT_OK;
  HIPCHK(hipSetDevice(ctx->device));
  double both[6 + kFitSums];
  HIPCHK(d2h_staged(ctx, both, ctx->refit.rec.as<FitRecord>()->box, sizeof both));
  if (box) std::memcpy(box, both, 6 * sizeof(double));
  if (sums) std::memcpy(sums, both + 6, kFitSums * sizeof(double));
  return SIFT_OK;
}

int sift_homography_refit_device(sift_ctx* ctx, const sift_point_pair* d_points, size_t n, const sift_homography* start,
                                 double thresh, int max_rounds, sift_homography* refined, int32_t* rounds,
                                 int32_t* d_inliers, size_t cap, size_t* n_inliers) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = refit_check(ctx, d_points, n, thresh, max_rounds)) return rc;
  if (!start || !refined) return set_err(ctx, SIFT_E_ARG, "null model");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = refit_run(ctx, reinterpret_cast<const PointPair*>(d_points), n, start, thresh, max_rounds, refined,
                         rounds, n_inliers))
    return rc;
  return refit_list_out(ctx, d_inliers, cap, false);
}

int sift_homography_refit(sift_ctx* ctx, const sift_point_pair* points, size_t n, const sift_homography* start,
                          double thresh, int max_rounds, sift_homography* refined, int32_t* rounds, int32_t* inliers,
                          size_t cap, size_t* n_inliers) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = refit_check(ctx, points, n, thresh, max_rounds)) return rc;
  if (!start || !refined) return set_err(ctx, SIFT_E_ARG, "null model");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = h2d_buffer(ctx, ctx->refit.in_pts, points, n * sizeof(PointPair))) return rc;
  if (int rc = refit_run(ctx, ctx->refit.in_pts.as<PointPair>(), n, start, thresh, max_rounds, refined, rounds,
                         n_inliers))
    return rc;
  return refit_list_out(ctx, inliers, cap, true);
}

int sift_verify_features_refit(sift_ctx* ctx, sift_ctx* train_ctx, const sift_match_pair* pairs, size_t n, size_t K,
                               uint64_t seed, double thresh, int max_rounds, sift_homography* model, int32_t* rounds,
                               int32_t* inliers, size_t cap, size_t* n_inliers) {
  if (!ctx || !train_ctx) return SIFT_E_ARG;
  if (int rc = refit_check(ctx, pairs, n, thresh, max_rounds)) return rc;
  if (!model) return set_err(ctx, SIFT_E_ARG, "null model");
  sift_homography first;  // the RANSAC model; its list is not needed: the refit forms its own
  if (int rc = sift_verify_features(ctx, train_ctx, pairs, n, K, seed, thresh, &first, nullptr, 0, nullptr)) return rc;
  // the points sift_verify_features gathered are still on the device
  if (int rc = refit_run(ctx, ctx->verify.pts.as<PointPair>(), n, &first, thresh, max_rounds, model, rounds, n_inliers))
    return rc;
  return refit_list_out(ctx, inliers, cap, true);
}

int sift_last_refit_timings(sift_ctx* ctx, double* fit_ms, double* rescore_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (fit_ms) *fit_ms = ctx->refit.fit_ms;
  if (rescore_ms) *rescore_ms = ctx->refit.rescore_ms;
  return SIFT_OK;
}
