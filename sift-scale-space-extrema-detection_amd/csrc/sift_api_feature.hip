// C ABI of the orientation and descriptor stages (kernels: sift_feature.hip) and of their keypoint / orientation seams.
#include "sift_ctx.h"

using namespace sift;

static_assert(sizeof(sift_orientation) == 16 && sizeof(Orientation) == 16, "16-byte orientation records");
static_assert(kOriBins == SIFT_ORI_BINS && kOriSmooth == SIFT_ORI_SMOOTH && kOriMaxPeaks == SIFT_ORI_MAX_PEAKS &&
                  kOriLambda == SIFT_ORI_LAMBDA && kOriPeakRatio == SIFT_ORI_PEAK_RATIO,
              "orientation constants of include/sift_hip.h");
static_assert(kDescOri == SIFT_DESC_ORI && kDescBytes == SIFT_DESC_BYTES && kDescLambda == SIFT_DESC_LAMBDA &&
                  kDescCap == SIFT_DESC_CAP && SIFT_DESC_CELLS * SIFT_DESC_CELLS * SIFT_DESC_ORI == SIFT_DESC_BYTES,
              "descriptor constants of include/sift_hip.h");

// What the two stages need of the pyramid, whoever supplies the keypoints (sift_set_keypoints needs no more): one
// whole image whose octaves all have Gaussian planes.
static int check_feature_planes(sift_ctx* ctx) {
  if (ctx->detect_pending || ctx->begin_pending || ctx->pyr.dog_source == kNone)
    return set_err(ctx, SIFT_E_STATE, "no pyramid: build or load one first");
  if (ctx->P.nimg > 1) return set_err(ctx, SIFT_E_UNSUPPORTED, "orientations / descriptors of a batch");
  if (ctx->shard.row0 != 0 || ctx->shard.own_lo >= 0)
    return set_err(ctx, SIFT_E_UNSUPPORTED, "orientations / descriptors with a row origin or owned rows");
  if (ctx->pyr.planes_first > ctx->pyr.o_first)
    return set_err(ctx, SIFT_E_UNSUPPORTED, "orientations / descriptors of a seed-range detection");
  if (!ctx->pyr.have_gauss) return set_err(ctx, SIFT_E_STATE, "Gaussian planes not materialised");
  return SIFT_OK;
}

// ... and of the context: a settled refinement (or sift_set_keypoints) on that pyramid.
static int check_features(sift_ctx* ctx) {
  if (!stage_has(ctx, kNeedKp)) return set_err(ctx, SIFT_E_STATE, "no refinement: run sift_refine or a detection first");
  if (int rc = check_feature_planes(ctx)) return rc;
  HIPCHK(ctx->feat.ev.ensure());
  return SIFT_OK;
}

int sift_orient(sift_ctx* ctx, sift_orientation* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = check_features(ctx)) return rc;
  FeatState& F = ctx->feat;
  if (!F.have_ori) {
    const int n = (int)ctx->n_kp;
    F.have_desc = false;
    F.n_ori = 0;
    F.orient_ms = 0;
    if (n > 0) {
      HIPCHK(F.ori_count.ensure((size_t)(n + 1) * sizeof(unsigned)));
      HIPCHK(F.ori_off.ensure((size_t)(n + 1) * sizeof(unsigned)));
      HIPCHK(F.ori_mask.ensure((size_t)n * sizeof(unsigned long long)));
      HIPCHK(F.ori_theta.ensure((size_t)n * kOriMaxPeaks * sizeof(double)));
      HIPCHK(hipEventRecord(F.ev[0], ctx->stream));
      HIPCHK(launch_orient(ctx->P, ctx->pyr.gauss.as<float>(), ctx->pyr.planes_first, ctx->kp.as<Keypoint>(), n,
                           F.ori_count.as<unsigned>(), F.ori_mask.as<unsigned long long>(), F.ori_theta.as<double>(),
                           ctx->stream));
      unsigned total = 0;  // the record count sizes the record buffer
      if (int rc = ordered_total(ctx, F.ori_count.as<unsigned>(), F.ori_off.as<unsigned>(), n, &total)) return rc;
      HIPCHK(F.ori.ensure((size_t)std::max(total, 1u) * sizeof(Orientation)));
      HIPCHK(launch_orient_emit(F.ori_off.as<unsigned>(), F.ori_mask.as<unsigned long long>(),
                                F.ori_theta.as<double>(), n, total, F.ori.as<Orientation>(), ctx->stream));
      HIPCHK(hipEventRecord(F.ev[1], ctx->stream));
      HIPCHK(hipEventSynchronize(F.ev[1]));
      F.orient_ms = event_ms(F.ev[0], F.ev[1]);
      F.n_ori = total;
    }
    F.have_ori = true;
  }
  if (n_out) *n_out = F.n_ori;
  if (!out) return SIFT_OK;
  if (cap < F.n_ori) return set_err(ctx, SIFT_E_CAPACITY, "orientation buffer too small");
  if (F.n_ori) {
    HIPCHK(hipMemcpyAsync(out, F.ori.p, F.n_ori * sizeof(sift_orientation), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return SIFT_OK;
}

int sift_describe(sift_ctx* ctx, uint8_t* desc, uint8_t* described, size_t cap, size_t* n_out, size_t* n_described) {
  if (!ctx) return SIFT_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = check_features(ctx)) return rc;
  FeatState& F = ctx->feat;
  if (!F.have_ori) return set_err(ctx, SIFT_E_STATE, "no orientations: run sift_orient first");
  const size_t n = F.n_ori;
  if (!F.have_desc) {
    F.n_desc_ok = 0;
    F.describe_ms = 0;
    if (n > 0) {
      HIPCHK(F.desc.ensure(n * kDescBytes));
      HIPCHK(F.desc_ok.ensure(n));
      HIPCHK(F.desc_n.ensure(sizeof(unsigned)));
      HIPCHK(hipEventRecord(F.ev[2], ctx->stream));
      HIPCHK(hipMemsetAsync(F.desc_n.p, 0, sizeof(unsigned), ctx->stream));
      HIPCHK(launch_describe(ctx->P, ctx->pyr.gauss.as<float>(), ctx->pyr.planes_first, ctx->kp.as<Keypoint>(),
                             F.ori.as<Orientation>(), (int)n, F.desc.as<unsigned char>(),
                             F.desc_ok.as<unsigned char>(), F.desc_n.as<unsigned>(), ctx->stream));
      HIPCHK(hipEventRecord(F.ev[3], ctx->stream));
      unsigned ok = 0;
      if (int rc = ordered_total(ctx, nullptr, F.desc_n.as<unsigned>(), 0, &ok)) return rc;
      F.describe_ms = event_ms(F.ev[2], F.ev[3]);
      F.n_desc_ok = ok;
    }
    F.have_desc = true;
  }
  if (n_out) *n_out = n;
  if (n_described) *n_described = F.n_desc_ok;
  if (!desc) return described ? set_err(ctx, SIFT_E_ARG, "described without desc") : SIFT_OK;
  if (cap < n) return set_err(ctx, SIFT_E_CAPACITY, "descriptor buffer too small");
  if (n) {
    HIPCHK(d2h_staged(ctx, desc, F.desc.p, n * kDescBytes));
    if (described) HIPCHK(d2h_staged(ctx, described, F.desc_ok.p, n));
  }
  return SIFT_OK;
}

int sift_device_features(sift_ctx* ctx, const sift_orientation** d_ori, const uint8_t** d_desc,
                         const uint8_t** d_described, size_t* n) {
  if (!ctx || !n) return SIFT_E_ARG;
  if (!stage_has(ctx, kNeedDesc))
    return set_err(ctx, SIFT_E_STATE, "no features: run sift_orient and sift_describe first");
  if (d_ori) *d_ori = ctx->feat.ori.as<const sift_orientation>();
  if (d_desc) *d_desc = ctx->feat.desc.as<const uint8_t>();
  if (d_described) *d_described = ctx->feat.desc_ok.as<const uint8_t>();
  *n = ctx->feat.n_ori;
  return SIFT_OK;
}

int sift_last_feature_timings(sift_ctx* ctx, double* orient_ms, double* describe_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (orient_ms) *orient_ms = ctx->feat.orient_ms;
  if (describe_ms) *describe_ms = ctx->feat.describe_ms;
  return SIFT_OK;
}

int sift_set_keypoints(sift_ctx* ctx, const sift_keypoint* kp, size_t n) {
  if (!ctx || (!kp && n)) return SIFT_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = check_feature_planes(ctx)) return rc;
  if (!count_ok(n)) return set_err(ctx, SIFT_E_ARG, "too many keypoints");  // the scan runs over n + 1
  const Pyramid& P = ctx->P;
  for (size_t i = 0; i < n; ++i) {
    if (kp[i].octave < ctx->pyr.planes_first || kp[i].octave >= P.O)
      return set_err(ctx, SIFT_E_ARG, "keypoint octave out of range");
    if (kp[i].scale_level < 0 || kp[i].scale_level >= P.NS)
      return set_err(ctx, SIFT_E_ARG, "keypoint scale_level out of range");
  }
  HIPCHK(ctx->kp.ensure(std::max<size_t>(n, 1) * sizeof(Keypoint)));
  if (int rc = h2d_buffer(ctx, ctx->kp, kp, n * sizeof(sift_keypoint))) return rc;
  if (n) HIPCHK(hipStreamSynchronize(ctx->stream));
  FeatState& F = ctx->feat;
  ctx->n_kp = n;
  ctx->have_kp = true;
  F.have_ori = F.have_desc = false;
  F.n_ori = F.n_desc_ok = 0;
  // nothing of the refinement this list replaces is served afterwards
  ctx->ref.n_sing = 0;
  ctx->shard.has_origins = false;
  ctx->budget.have_sel = false;
  ctx->ref.blk_counts.clear();
  ctx->tm.refine_ms = 0;
  F.orient_ms = F.describe_ms = 0;
  return SIFT_OK;
}

int sift_set_orientations(sift_ctx* ctx, const sift_orientation* rec, size_t n) {
  if (!ctx || (!rec && n)) return SIFT_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = check_features(ctx)) return rc;
  if (n > (size_t)0x7fffffff) return set_err(ctx, SIFT_E_ARG, "too many orientation records");
  for (size_t i = 0; i < n; ++i) {
    if (rec[i].keypoint < 0 || (size_t)rec[i].keypoint >= ctx->n_kp)
      return set_err(ctx, SIFT_E_ARG, "orientation record of no keypoint");
    if (rec[i].bin < 0 || rec[i].bin >= kOriBins) return set_err(ctx, SIFT_E_ARG, "orientation bin out of range");
    if (!(rec[i].theta >= 0.0 && rec[i].theta < 2.0 * M_PI))  // a NaN fails both
      return set_err(ctx, SIFT_E_ARG, "theta outside [0, 2 pi)");
  }
  FeatState& F = ctx->feat;
  HIPCHK(F.ori.ensure(std::max<size_t>(n, 1) * sizeof(Orientation)));
  if (int rc = h2d_buffer(ctx, F.ori, rec, n * sizeof(sift_orientation))) return rc;
  if (n) HIPCHK(hipStreamSynchronize(ctx->stream));
  F.n_ori = n;
  F.have_ori = true;
  F.have_desc = false;
  F.n_desc_ok = 0;
  F.orient_ms = F.describe_ms = 0;
  return SIFT_OK;
}
