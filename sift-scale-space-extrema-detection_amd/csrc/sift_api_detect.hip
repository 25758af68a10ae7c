// C ABI of the refinement, the keypoint copies and the sift_detect* family: one whole detection (Gaussian+DoG,
// extrema, refinement) queued without a host round trip and settled by one synchronisation.  Kernels: sift_refine.hip.
#include <cstdio>

#include "sift_ctx.h"

using namespace sift;

// Refinement over ctx->ext.slot_cap slots, counters[kCntN] of them live, without
// a host round trip; refine_settle's one synchronisation reads every count
// back and returns kRetry when the extrema stage it follows overflowed.
static int refine_enqueue(sift_ctx* ctx) {
  Pyramid& P = ctx->P;
  ExtState& E = ctx->ext;
  RefState& F = ctx->ref;
  const int cap = E.slot_cap;
  unsigned* cnt = ctx->counters.as<unsigned>();
  HIPCHK(hipEventRecord(ctx->ev[kEvRef], ctx->stream));
  HIPCHK(F.status.ensure((size_t)std::max(cap, 1) * sizeof(int)));
  HIPCHK(F.kp_tmp.ensure((size_t)std::max(cap, 1) * sizeof(Keypoint)));
  HIPCHK(ctx->kp.ensure((size_t)std::max(cap, 1) * sizeof(Keypoint)));
  HIPCHK(F.uncertain.ensure((size_t)std::max(cap, 1) * sizeof(unsigned)));
  HIPCHK(F.keep.ensure((size_t)std::max(cap, 1) * sizeof(unsigned)));
  HIPCHK(F.pos.ensure((size_t)std::max(cap, 1) * sizeof(unsigned)));
  if (!E.counters_zeroed) {  // refinement without a fresh extrema stage (caller candidates / re-run)
    HIPCHK(hipMemsetAsync(cnt + kCntUnc, 0, 2 * sizeof(unsigned), ctx->stream));
    HIPCHK(hipMemsetAsync(cnt + kCntKp, 0, sizeof(unsigned), ctx->stream));
    HIPCHK(hipMemsetAsync(cnt + kCntDbg, 0, kCntDbgWords * sizeof(unsigned), ctx->stream));
    HIPCHK(hipMemsetAsync(cnt + kBlk, 0, (kCntAll - kBlk) * sizeof(unsigned), ctx->stream));
  }
  E.counters_zeroed = false;
  ctx->n_kp = 0;
  F.n_sing = 0;
  drop_results(ctx, false);
  if (cap > 0) {
    RefineLaunch R{};
    R.cand_key = E.cand_key.as<unsigned>();
    R.cand_val = E.cand_val.as<double>();
    R.keep = E.has_keep ? E.cand_keep.as<unsigned>() : nullptr;
    R.n = cnt + kCntN;
    R.cap = cap;
    R.exact_planes = ctx->pyr.dog_source == kForeign;
    R.min_blur = ctx->p.min_blur;
    R.min_interpixel_distance = ctx->p.min_interpixel_distance;
    R.status = F.status.as<int>();
    R.kp = F.kp_tmp.as<Keypoint>();
    R.uncertain = F.uncertain.as<unsigned>();
    R.counters = cnt;
    R.perm = nullptr;
    static const int band_order = exp_knob("SIFT_BAND_ORDER", 1);
    if (band_order && E.slots_rows) {
      BandOrder B{};
      B.G = E.xl.G;
      B.S = P.S;
      int items = 0;
      for (int o = 0; o < P.O; ++o) {
        B.item_off[o] = items;
        items += P.S * ((P.oct[o].h + kBandRows - 1) / kBandRows);
      }
      B.item_off[P.O] = items;
      items *= std::max(1, P.nimg);  // image-major
      B.n_items = items;
      HIPCHK(F.band_cnt.ensure((size_t)items * sizeof(unsigned)));
      HIPCHK(F.band_first.ensure((size_t)items * sizeof(unsigned)));
      HIPCHK(F.band_start.ensure((size_t)items * sizeof(unsigned)));
      HIPCHK(F.perm.ensure((size_t)cap * sizeof(unsigned)));
      B.rowoff = E.rowoff.as<unsigned>();
      B.count = F.band_cnt.as<unsigned>();
      B.first = F.band_first.as<unsigned>();
      B.start = F.band_start.as<unsigned>();
      B.perm = F.perm.as<unsigned>();
      B.cap = cap;
      HIPCHK(launch_band_items(P, B, ctx->stream));
      HIPCHK(exclusive_sum(ctx, B.count, F.band_start.as<unsigned>(), items));
      HIPCHK(launch_band_fill(P, B, ctx->stream));
      R.perm = B.perm;
    }
    HIPCHK(launch_refine_fast(P, R, ctx->stream));
    HIPCHK(hipEventRecord(F.ev_heavy[0], ctx->stream));  // the rest is latency-bound tail work
    // Uncertain decisions exist only with fp32-rounded native planes.
    R.wide_exact = ctx->pyr.o_first > 0;  // a tail piece (sift_detect_from_seed*): latency over throughput
    if (ctx->pyr.dog_source == kNative) HIPCHK(launch_refine_exact(P, R, ctx->stream));
    HIPCHK(F.keep_tile.ensure(keep_tiles(cap) * sizeof(unsigned)));
    HIPCHK(launch_keep_compact(P, R.status, R.cand_key, F.keep.as<unsigned>(), F.pos.as<unsigned>(),
                               F.keep_tile.as<unsigned>(), R.n, cap, ctx->shard.own_lo, ctx->shard.own_hi,
                               cnt + kBlk, R.kp, ctx->kp.as<Keypoint>(), ctx->stream));
    HIPCHK(launch_count_keypoints(P, F.pos.as<unsigned>(), F.keep.as<unsigned>(), R.cand_key, R.n, cap,
                                  cnt + kCntKp, cnt + kBlk, ctx->stream));
    if (ctx->p.flags & SIFT_F_KEYPOINT_ORIGINS) {
      HIPCHK(ctx->shard.kp_key.ensure((size_t)cap * sizeof(unsigned)));
      HIPCHK(launch_scatter_keys(F.keep.as<unsigned>(), F.pos.as<unsigned>(), R.cand_key, R.n, cap,
                                 ctx->shard.kp_key.as<unsigned>(), ctx->stream));
    }
  }
  ctx->shard.has_origins = (ctx->p.flags & SIFT_F_KEYPOINT_ORIGINS) != 0;
  // the counts and the kept keypoints per block (the block starts stay on the device)
  const int nblk = std::max(1, P.nimg) * P.O * P.S;
  HIPCHK(hipMemcpyAsync(ctx->h_counters.p, cnt, (kBlk + nblk) * sizeof(unsigned), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[kEvRefEnd], ctx->stream));
  return SIFT_OK;
}

// Waits for the refinement enqueued by refine_enqueue and reads its counts
// (and the extrema counts when those are still pending).
static int refine_settle(sift_ctx* ctx) {
  const int cap = ctx->ext.slot_cap;
  HIPCHK(hipEventSynchronize(ctx->ev[kEvRefEnd]));
  if (ctx->ext.pending) {
    const int rc = settle_extrema(ctx);
    if (rc) return rc;
  }
  const unsigned* h = ctx->h_counters.as<unsigned>();
  if (h[kCntUnc] > (unsigned)cap) return set_err(ctx, SIFT_E_STATE, "uncertain list overflow");
  if (h[kCntUnc] && ctx->pyr.dog_source != kNative)
    return set_err(ctx, SIFT_E_STATE, "uncertain refinement without a native pyramid");
  ctx->ext.n_exact += h[kCntUnc];
  ctx->n_kp = cap > 0 ? h[kCntKp] : 0;
  ctx->ref.n_sing = h[kCntSing];
  drop_results(ctx, false);
  ctx->have_kp = true;
  std::vector<long long>& blk = ctx->ref.blk_counts;
  blk.assign((size_t)std::max(1, ctx->P.nimg) * ctx->P.O * ctx->P.S, 0);
  if (cap > 0)
    for (size_t b = 0; b < blk.size(); ++b) blk[b] = h[kBlk + b];
  if (exp_knob("SIFT_DEBUG_REFINE", 0)) {
    const unsigned *why = h + kCntDbg, *it = h + kCntDbgIter;
    std::fprintf(stderr,
                 "refine uncertain %u: det %u alpha %u omega %u edge_dt %u edge_int %u round %u | iter %u %u %u %u %u"
                 " | output precision %u\n",
                 h[kCntUnc], why[0], why[1], why[2], why[3], why[4], why[5], it[0], it[1], it[2], it[3], it[4],
                 h[kCntDbgPrec]);
  }
  return SIFT_OK;
}

static int run_refine(sift_ctx* ctx) {
  const int rc = refine_enqueue(ctx);
  return rc ? rc : refine_settle(ctx);
}

void sift::read_stage_times(sift_ctx* ctx, bool extrema, bool refine) {
  (void)hipEventSynchronize(ctx->ev[kEvRefEnd]);
  if (extrema) take_event_ms(&ctx->tm.extrema_ms, ctx->ev[kEvExt], ctx->ev[kEvExtEnd]);
  if (refine) take_event_ms(&ctx->tm.refine_ms, ctx->ev[kEvRef], ctx->ev[kEvRefEnd]);
}

// The settled keypoints into out; SIFT_E_SINGULAR, after a good copy, when the refinement met a singular Hessian.
static int return_keypoints(sift_ctx* ctx, sift_keypoint* out, size_t cap, size_t* n_out) {
  const int rc = sift_copy_keypoints(ctx, out, cap, n_out);
  if (rc || !ctx->ref.n_sing) return rc;
  return set_err(ctx, SIFT_E_SINGULAR, "singular Hessian (the reference throws a TypeError here)");
}

// One whole detection is enqueued without waiting, in two phases: the Gaussian+DoG pass, then extrema + refinement
// (the caller may order the second phase after other contexts' work in between); detect_finish completes it.
static int detect_begin(sift_ctx* ctx, BuildRequest q) {
  if (!ctx) return SIFT_E_ARG;
  q.fuse_extrema = q.nimg == 1;
  int rc = build_common(ctx, q);
  if (rc) return rc;
  ctx->begin_pending = true;
  ctx->detect_host_img = q.img_host != nullptr;
  return SIFT_OK;
}

// The second phase on the pyramid just queued.
static int detect_launch(sift_ctx* ctx) {
  int rc = launch_extrema_stage(ctx);
  if (rc) return rc;
  rc = refine_enqueue(ctx);
  if (rc) return rc;
  ctx->detect_pending = true;
  return SIFT_OK;
}

static int detect_end(sift_ctx* ctx) {
  if (!ctx->begin_pending) return set_err(ctx, SIFT_E_STATE, "no detection begun (sift_detect_begin_async)");
  ctx->begin_pending = false;
  return detect_launch(ctx);
}

static int detect_enqueue(sift_ctx* ctx, const BuildRequest& q) {
  const int rc = detect_begin(ctx, q);
  return rc ? rc : detect_end(ctx);
}

// One host synchronisation per image; a capacity overflow (first images)
// grows the buffers and reruns extrema + refinement.
static int detect_finish(sift_ctx* ctx, sift_keypoint* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (!ctx->detect_pending) return set_err(ctx, SIFT_E_STATE, "no detection in flight");
  ctx->detect_pending = false;
  int rc = refine_settle(ctx);
  while (rc == kRetry) {
    rc = launch_extrema_stage(ctx);
    if (rc) return rc;
    rc = run_refine(ctx);
  }
  if (rc) return rc;
  (void)hipEventSynchronize(ctx->ev[kEvRefEnd]);
  if (ctx->detect_host_img) take_event_ms(&ctx->tm.h2d_ms, ctx->ev[kEvUpload], ctx->ev[kEvPass]);
  else ctx->tm.h2d_ms = 0;
  read_gauss_times(ctx);
  read_stage_times(ctx, true, true);
  return return_keypoints(ctx, out, cap, n_out);
}

static int detect_common(sift_ctx* ctx, const BuildRequest& q, sift_keypoint* out, size_t cap, size_t* n_out) {
  const int rc = detect_enqueue(ctx, q);
  return rc ? rc : detect_finish(ctx, out, cap, n_out);
}

// An asynchronous entry point starts only on a context with no detection in flight.
static int check_idle(sift_ctx* ctx) {
  if (ctx->detect_pending || ctx->begin_pending)
    return set_err(ctx, SIFT_E_STATE, "a detection is already in flight on this context");
  return SIFT_OK;
}

static int check_batch(sift_ctx* ctx, int n_images, size_t image_stride_px, int height, size_t stride_px) {
  if (n_images < 1 || (n_images > 1 && image_stride_px < (size_t)height * stride_px))
    return set_err(ctx, SIFT_E_ARG, "n_images < 1 or overlapping images");
  return SIFT_OK;
}

// Makes q, one image's request, that of n_images images image_stride_px apart; checks it and the context.
static int batch_request(sift_ctx* ctx, BuildRequest* q, int n_images, size_t image_stride_px) {
  if (!ctx) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (int rc = check_batch(ctx, n_images, image_stride_px, q->H, q->stride)) return rc;
  q->nimg = n_images, q->img_bstride = image_stride_px;
  return check_idle(ctx);
}

static int detect_from_seed(sift_ctx* ctx, int o_first, const double* seed_host, const double* seed_dev, int W,
                            int H, const sift_params* p, sift_keypoint* out, size_t cap, size_t* n_out,
                            int scan_first = 0) {
  if (!ctx || !p) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  // (weaker than check_idle: a detection begun with sift_detect_begin_async stays begun)
  if (ctx->detect_pending) return set_err(ctx, SIFT_E_STATE, "a detection is in flight on this context");
  if (o_first < 1) return set_err(ctx, SIFT_E_ARG, "octave_first must be >= 1");
  if (scan_first && (scan_first < o_first || scan_first >= p->num_octaves))
    return set_err(ctx, SIFT_E_ARG, "octave_scan_first outside [octave_first, num_octaves)");
  BuildRequest q;
  q.W = W, q.H = H, q.p = p;
  q.o_first = o_first, q.seed_host = seed_host, q.seed_dev = seed_dev;
  q.seed_only_below = scan_first;
  int rc = build_common(ctx, q);
  if (rc) return rc;
  if (scan_first) ctx->pyr.scan_first = scan_first;
  rc = detect_launch(ctx);
  if (rc) return rc;
  ctx->detect_host_img = false;
  return detect_finish(ctx, out, cap, n_out);
}

int sift_refine_params(sift_ctx* ctx, double min_blur_level, double min_interpixel_distance) {
  if (!ctx) return SIFT_E_ARG;
  if (!(min_blur_level > 0) || !(min_interpixel_distance > 0)) return set_err(ctx, SIFT_E_ARG, "bad refine scalars");
  ctx->p.min_blur = min_blur_level;
  ctx->p.min_interpixel_distance = min_interpixel_distance;
  return SIFT_OK;
}

int sift_copy_keypoints(sift_ctx* ctx, sift_keypoint* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (n_out) *n_out = ctx->n_kp;
  if (!out) return SIFT_OK;
  if (cap < ctx->n_kp) return set_err(ctx, SIFT_E_CAPACITY, "keypoint buffer too small");
  if (ctx->n_kp) {
    HIPCHK(hipMemcpyAsync(out, ctx->kp.p, ctx->n_kp * sizeof(sift_keypoint), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return SIFT_OK;
}

// The records as two field arrays (one DMA into the context's pinned staging,
// one pass over it on the host threads).
int sift_copy_keypoints_soa(sift_ctx* ctx, int32_t* ints, double* reals, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (n_out) *n_out = ctx->n_kp;
  if (!ints || !reals) return ints || reals ? SIFT_E_ARG : SIFT_OK;
  if (cap < ctx->n_kp) return set_err(ctx, SIFT_E_CAPACITY, "keypoint buffer too small");
  const size_t n = ctx->n_kp;
  if (!n) return SIFT_OK;
  HIPCHK(hipSetDevice(ctx->device));
  // Page-locked destinations (sift_host_register; the N-API result pool's
  // recycled buffers): split on the device, one DMA into each array.
  if (host_registered(ints, n * 4 * sizeof(int32_t)) && host_registered(reals, n * 4 * sizeof(double))) {
    HIPCHK(ctx->ref.kp_soa.ensure(n * sizeof(sift_keypoint)));
    int32_t* di = ctx->ref.kp_soa.as<int32_t>();
    double* dr = reinterpret_cast<double*>(di + 4 * n);  // 16 n bytes in: 16-byte aligned
    HIPCHK(launch_kp_soa(ctx->kp.as<Keypoint>(), (int)n, di, dr, ctx->stream));
    HIPCHK(hipMemcpyAsync(ints, di, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(reals, dr, n * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SIFT_OK;
  }
  HIPCHK(ctx->ref.hkp.ensure(n * sizeof(sift_keypoint)));
  HIPCHK(hipMemcpyAsync(ctx->ref.hkp.p, ctx->kp.p, n * sizeof(sift_keypoint), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const sift_keypoint* k = (const sift_keypoint*)ctx->ref.hkp.p;
  par_for(n, n >= 65536 ? host_threads() : 1, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      ints[4 * i] = k[i].octave;
      ints[4 * i + 1] = k[i].scale_level;
      ints[4 * i + 2] = k[i].local_x;
      ints[4 * i + 3] = k[i].local_y;
      reals[4 * i] = k[i].abs_sigma;
      reals[4 * i + 1] = k[i].abs_x;
      reals[4 * i + 2] = k[i].abs_y;
      reals[4 * i + 3] = k[i].interp_value;
    }
  });
  return SIFT_OK;
}

int sift_copy_keypoints_device(sift_ctx* ctx, void* d_dst, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (n_out) *n_out = ctx->n_kp;
  if (!d_dst) return SIFT_OK;
  if (cap < ctx->n_kp) return set_err(ctx, SIFT_E_CAPACITY, "keypoint buffer too small");
  if (ctx->n_kp) {
    HIPCHK(hipSetDevice(ctx->device));
    // The keypoints are final (the detection was waited for): copy off the
    // context stream, so a detection queued behind them is not waited for.
    HIPCHK(hipMemcpy(d_dst, ctx->kp.p, ctx->n_kp * sizeof(sift_keypoint), hipMemcpyDeviceToDevice));
  }
  return SIFT_OK;
}

int sift_device_keypoints(sift_ctx* ctx, const sift_keypoint** d_kp, size_t* n) {
  if (!ctx || !d_kp || !n) return SIFT_E_ARG;
  *d_kp = ctx->kp.as<const sift_keypoint>();
  *n = ctx->n_kp;
  return SIFT_OK;
}

int sift_refine(sift_ctx* ctx, sift_keypoint* out, size_t cap, size_t* n_out, size_t* n_singular) {
  if (!ctx) return SIFT_E_ARG;
  if (!ctx->ext.have_cand) return set_err(ctx, SIFT_E_STATE, "no candidates: run sift_find_extrema first");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = run_refine(ctx);
  if (rc) return rc == kRetry ? set_err(ctx, SIFT_E_STATE, "candidate capacity overflow") : rc;
  read_stage_times(ctx, false, true);
  if (n_singular) *n_singular = ctx->ref.n_sing;
  return return_keypoints(ctx, out, cap, n_out);
}

int sift_detect_device_async(sift_ctx* ctx, const float* d_img, int width, int height, size_t stride_px,
                             const sift_params* p) {
  if (!ctx) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (int rc = check_idle(ctx)) return rc;
  return detect_enqueue(ctx, image_request(nullptr, d_img, width, height, stride_px, p));
}

int sift_detect_batch_device_async(sift_ctx* ctx, const float* d_imgs, int n_images, size_t image_stride_px,
                                   int width, int height, size_t stride_px, const sift_params* p) {
  BuildRequest q = image_request(nullptr, d_imgs, width, height, stride_px, p);
  const int rc = batch_request(ctx, &q, n_images, image_stride_px);
  return rc ? rc : detect_enqueue(ctx, q);
}

int sift_detect_batch(sift_ctx* ctx, const float* imgs, int n_images, size_t image_stride_px, int width, int height,
                      size_t stride_px, const sift_params* p, sift_keypoint* out, size_t cap, size_t* n_out) {
  BuildRequest q = image_request(imgs, nullptr, width, height, stride_px, p);
  if (int rc = batch_request(ctx, &q, n_images, image_stride_px)) return rc;
  return host_image_exit(ctx, detect_common(ctx, q, out, cap, n_out));
}

int sift_detect_batch_device(sift_ctx* ctx, const float* d_imgs, int n_images, size_t image_stride_px, int width,
                             int height, size_t stride_px, const sift_params* p, sift_keypoint* out, size_t cap,
                             size_t* n_out) {
  const int rc = sift_detect_batch_device_async(ctx, d_imgs, n_images, image_stride_px, width, height, stride_px, p);
  return rc ? rc : detect_finish(ctx, out, cap, n_out);
}

int sift_detect_begin_async(sift_ctx* ctx, const float* d_img, int width, int height, size_t stride_px,
                            const sift_params* p) {
  if (!ctx) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (int rc = check_idle(ctx)) return rc;
  return detect_begin(ctx, image_request(nullptr, d_img, width, height, stride_px, p));
}

int sift_detect_end_async(sift_ctx* ctx) {
  if (!ctx) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  return detect_end(ctx);
}

int sift_detect_wait(sift_ctx* ctx, sift_keypoint* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  return detect_finish(ctx, out, cap, n_out);
}

int sift_detect(sift_ctx* ctx, const float* img, int width, int height, size_t stride_px, const sift_params* p,
                sift_keypoint* out, size_t cap, size_t* n_out) {
  if (ctx) (void)hipSetDevice(ctx->device);
  return host_image_exit(
      ctx, detect_common(ctx, image_request(img, nullptr, width, height, stride_px, p), out, cap, n_out));
}

int sift_detect_device(sift_ctx* ctx, const float* d_img, int width, int height, size_t stride_px,
                       const sift_params* p, sift_keypoint* out, size_t cap, size_t* n_out) {
  if (ctx) (void)hipSetDevice(ctx->device);
  return detect_common(ctx, image_request(nullptr, d_img, width, height, stride_px, p), out, cap, n_out);
}

int sift_detect_from_seed(sift_ctx* ctx, int octave_first, const double* seed, int width, int height,
                          const sift_params* p, sift_keypoint* out, size_t cap, size_t* n_out) {
  return detect_from_seed(ctx, octave_first, seed, nullptr, width, height, p, out, cap, n_out);
}

int sift_detect_from_seed_device(sift_ctx* ctx, int octave_first, const double* d_seed, int width, int height,
                                 const sift_params* p, sift_keypoint* out, size_t cap, size_t* n_out) {
  return detect_from_seed(ctx, octave_first, nullptr, d_seed, width, height, p, out, cap, n_out);
}

int sift_detect_from_seed_range_device(sift_ctx* ctx, int octave_first, int octave_scan_first, const double* d_seed,
                                       int width, int height, const sift_params* p, sift_keypoint* out, size_t cap,
                                       size_t* n_out) {
  return detect_from_seed(ctx, octave_first, nullptr, d_seed, width, height, p, out, cap, n_out,
                          std::max(octave_scan_first, octave_first));
}

int sift_order_after(sift_ctx* ctx, const sift_ctx* prev, int after) {
  if (!ctx || !prev) return SIFT_E_ARG;
  if (after < SIFT_AFTER_OCTAVE0 || after > SIFT_AFTER_REFINEMENT) return SIFT_E_ARG;
  if (ctx == prev || ctx->stream == prev->stream) return SIFT_OK;  // already ordered
  HIPCHK(hipSetDevice(ctx->device));
  // after the fast refinement the rest is the latency-bound tail
  const hipEvent_t e = after == SIFT_AFTER_OCTAVE0    ? prev->ev[kEvOct0]
                       : after == SIFT_AFTER_GAUSSIAN ? prev->ev[kEvPassEnd]
                                                      : prev->ref.ev_heavy[0];
  HIPCHK(hipStreamWaitEvent(ctx->stream, e, 0));
  return SIFT_OK;
}
