// C ABI of the Gaussian + DoG pyramid: geometry, schedule and taps, the build (build_common, which every detection
// starts with), plane read-back and caller-supplied planes.  Kernels: sift_gauss_*.hip.
#include "sift_ctx.h"

using namespace sift;

static double js_round(double x) {
  double f = std::floor(x);
  return (x - f >= 0.5) ? f + 1.0 : f;
}

// Geometry, schedule and weights (host), background.js:71-177 + sift.js:31-67.
static int setup_geometry(sift_ctx* ctx, int W, int H, const sift_params* p, const double* sig_in,
                          bool need_weights) {
  int rc = check_params(p);
  if (rc) return set_err(ctx, rc, "invalid or unsupported parameters");
  if (W < 1 || H < 1) return set_err(ctx, SIFT_E_ARG, "empty image");
  const int O = p->num_octaves, S = p->scales_per_octave, NS = S + 3, ND = S + 2;
  PyrState& Y = ctx->pyr;
  ctx->p = *p;
  Y.scan_first = Y.planes_first = 0;
  Y.dims.assign(2 * O, 0);
  sift_octave_dims(W, H, O, Y.dims.data());
  Y.blur.assign(O * NS, 0.0);
  Y.sigma.assign(O * NS, 0.0);
  sift_schedule(p, Y.blur.data(), Y.sigma.data());
  if (sig_in) std::copy(sig_in, sig_in + O * NS, Y.sigma.begin());
  Pyramid& P = ctx->P;
  std::memset(&P, 0, sizeof(P));
  P.O = O; P.S = S; P.NS = NS; P.ND = ND;
  P.W = W; P.H = H;
  const double thr = ((std::pow(2.0, 1.0 / S) - 1) / (std::pow(2.0, 1.0 / 3) - 1)) * 0.015;
  P.thr = thr;             // background.js:572
  P.row0 = ctx->shard.row0;
  P.pix_thr = thr * 0.8;   // sift.js:285-294
  std::vector<double> w;
  long long goff = 0, doff = 0, soff = 0;
  unsigned long long koff = 0;
  TapCache& tc = Y.taps;
  const bool taps_hit = need_weights && tc.NS == NS && tc.sigma.size() >= (size_t)O * NS &&
                        std::equal(Y.sigma.begin(), Y.sigma.end(), tc.sigma.begin());
  if (taps_hit) w.assign(tc.w.begin(), tc.w.begin() + (std::ptrdiff_t)tc.oct_end[O - 1]);
  std::vector<size_t> oct_end;
  for (int o = 0; o < O; ++o) {
    Octave& oc = P.oct[o];
    oc.h = Y.dims[2 * o];
    oc.w = Y.dims[2 * o + 1];
    const long long plane = (long long)oc.h * oc.w;
    oc.gauss_off = goff;
    oc.dog_off = doff;
    oc.seed_off = o > 0 ? soff : 0;
    if (o > 0) soff += plane;
    if (koff > 0xffffffffull) return set_err(ctx, SIFT_E_UNSUPPORTED, "image too large for 32-bit keys");
    oc.key_off = (unsigned)koff;
    koff += (unsigned long long)S * plane;
    goff += NS * plane;
    doff += ND * plane;
    oc.rmax = 0;
    oc.l64_off = -1;
    if (taps_hit) {
      for (int s = 0; s < NS; ++s) {
        oc.rad[s] = tc.rad[o * NS + s];
        oc.wofs[s] = tc.wofs[o * NS + s];
        oc.rmax = std::max(oc.rmax, oc.rad[s]);
      }
      continue;
    }
    for (int s = 0; s < NS; ++s) {
      const double sg = Y.sigma[o * NS + s];
      int r = 0;
      for (int z = 0; z < kWPad; ++z) w.push_back(0.0);
      oc.wofs[s] = (int)w.size();
      if (o > 0 && s == 0) {
        w.push_back(1.0);  // the un-blurred seed: exact copy
      } else {
        // sift.js:38-44: r = Math.round(3 sigma); the 2D kernel
        // exp(((i^2+j^2)/s^2)*-0.5)/(2 pi s^2) / sum factors as w(i) w(j)
        // with w(i) = exp((i^2/s^2)*-0.5) / sum_i exp(...).
        r = (int)js_round(3.0 * sg);
        std::vector<double> g(2 * r + 1);
        double sum = 0.0;
        for (int i = 0; i <= 2 * r; ++i) {
          const double a = i - r;
          g[i] = std::exp(((a * a) / (sg * sg)) * -0.5);
          sum += g[i];
        }
        for (int i = 0; i <= 2 * r; ++i) w.push_back(g[i] / sum);
      }
      for (int z = 0; z < kWPad; ++z) w.push_back(0.0);
      oc.rad[s] = r;
      oc.rmax = std::max(oc.rmax, r);
    }
    oct_end.push_back(w.size());
  }
  if (koff > 0xffffffffull) return set_err(ctx, SIFT_E_UNSUPPORTED, "image too large for 32-bit keys");
  if (need_weights && !taps_hit && (tc.NS != NS || O * NS >= (int)tc.sigma.size())) {
    // a miss at this depth or deeper replaces the cache; a shallower miss
    // (another schedule) leaves a deeper one in place
    tc.NS = NS;
    tc.sigma = Y.sigma;
    tc.w = w;
    tc.oct_end = oct_end;
    tc.rad.assign((size_t)O * NS, 0);
    tc.wofs.assign((size_t)O * NS, 0);
    for (int o = 0; o < O; ++o)
      for (int s = 0; s < NS; ++s) {
        tc.rad[o * NS + s] = P.oct[o].rad[s];
        tc.wofs[o * NS + s] = P.oct[o].wofs[s];
      }
  }
  P.nimg = 1;  // one image (build_common sets a batch)
  P.kpi = (unsigned)koff;
  // Every octave's Gaussian launch; its strip (32 rows x (76 + 2R) fp64) must fit the LDS.
  for (int o = 0; o < O; ++o) {
    Y.gplan[o] = gauss_plan(P, o);
    if (Y.gplan[o].lds > kGaussMaxLds)
      return set_err(ctx, SIFT_E_UNSUPPORTED, "blur radius too large for one LDS strip");
  }
  if (need_weights) {
    // Upload only when the taps changed (the same schedule image after image).
    // The taps are laid out octave after octave, so a schedule with fewer
    // octaves is a prefix of a deeper one: a context that alternates row bands
    // (octaves 0..K) and tail pieces (octaves 0..t) keeps the deepest taps
    // and uploads (a blocking copy) only when a deeper schedule arrives.
    const bool prefix = w.size() <= Y.wts_host.size() && std::equal(w.begin(), w.end(), Y.wts_host.begin());
    if (!prefix || !Y.wts.p) {
      if (Y.wts.ensure(w.size() * sizeof(double)) != hipSuccess)
        return set_err(ctx, SIFT_E_HIP, "hipMalloc weights");
      if (hipMemcpy(Y.wts.p, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return set_err(ctx, SIFT_E_HIP, "upload weights");
      Y.wts_host = w;
    }
    P.wts = Y.wts.as<double>();
  }
  return SIFT_OK;
}

long long sift::total_plane_px(const sift_ctx* ctx) {
  long long t = 0;
  for (int o = 0; o < ctx->P.O; ++o) t += (long long)ctx->P.oct[o].h * ctx->P.oct[o].w;
  return t;
}

// Fused extrema decisions (k_gauss_dog, XF): SIFT_F_FUSED_EXTREMA, or
// SIFT_FUSE=1 for every detection (experiments).
static bool fuse_enabled(const sift_params* p) {
  static const bool env = exp_knob("SIFT_FUSE", 0) != 0;
  return env || (p->flags & SIFT_F_FUSED_EXTREMA);
}

// The build a BuildRequest describes (sift_ctx.h), queued on the context stream.  With fused decisions the extrema
// stage then scans octaves >= 1 only; a batch keeps planes and seeds image-major.
int sift::build_common(sift_ctx* ctx, const BuildRequest& q) {
  if (!ctx) return SIFT_E_ARG;
  const int W = q.W, H = q.H, o_first = q.o_first, nimg = q.nimg;
  const sift_params* const p = q.p;
  if (o_first == 0 && !q.img_host && !q.img_dev) return set_err(ctx, SIFT_E_ARG, "null image");
  if (o_first > 0 && !q.seed_host && !q.seed_dev) return set_err(ctx, SIFT_E_ARG, "null seed");
  if (o_first == 0 && q.stride < (size_t)W) return set_err(ctx, SIFT_E_ARG, "stride < width");
  HIPCHK(hipSetDevice(ctx->device));
  // (the launch records go with the plans that setup_geometry replaces)
  std::fill(ctx->pyr.glaunch, ctx->pyr.glaunch + kMaxOctaves, GaussLaunched{});
  int rc = setup_geometry(ctx, W, H, p, q.sig, true);
  if (rc) return rc;
  Pyramid& P = ctx->P;
  PyrState& Y = ctx->pyr;
  ShardState& Sh = ctx->shard;
  const GaussPlan* const plan = Y.gplan;
  const bool needs_base0 = plan[0].path == kGaussBase0;
  if (o_first < 0 || o_first >= P.O) return set_err(ctx, SIFT_E_ARG, "octave_first out of range");
  Y.o_first = Y.scan_first = o_first;
  // Octaves [o_first, so_end) only feed their successor's base (a range
  // detection scans from so_end): launch_seed_only, no planes.
  const int so_end = std::min(std::max(o_first, q.seed_only_below), P.O - 1);
  if (so_end > o_first && (nimg > 1 || q.fuse_extrema))
    return set_err(ctx, SIFT_E_UNSUPPORTED, "seed-only octaves: single image, no fused decisions");
  Y.planes_first = so_end;
  Sh.has_xseed = false;
  const long long tot = total_plane_px(ctx);
  const bool keep_gauss = !(p->flags & SIFT_F_SKIP_GAUSS_PLANES);
  if (nimg > 1) {
    if (o_first != 0 || (!q.img_host && !q.img_dev) || q.fuse_extrema || needs_base0 || Sh.row0 != 0 ||
        Sh.own_lo >= 0 ||
        (p->flags & (SIFT_F_EXPORT_NEXT_SEED | SIFT_F_LOW_CONTRAST_LIST | SIFT_F_FUSED_EXTREMA |
                     SIFT_F_KEYPOINT_ORIGINS)))  // origins carry no image index
      return set_err(ctx, SIFT_E_UNSUPPORTED, "batch: whole device images, plain detection only");
    if ((unsigned long long)P.kpi * (unsigned long long)nimg > 0xffffffffull ||
        (long long)nimg * P.O * P.S > kBlkN)
      return set_err(ctx, SIFT_E_UNSUPPORTED, "batch too large for 32-bit keys / block counts");
  }
  const long long seeds_pi = std::max<long long>(1, tot - (long long)P.oct[0].h * P.oct[0].w);
  P.nimg = nimg;
  P.img_bstride = nimg > 1 ? (long long)q.img_bstride : 0;
  P.seed_bstride = seeds_pi;
  P.dog_bstride = tot * P.ND;
  HIPCHK(Y.dog.ensure((size_t)tot * P.ND * nimg * sizeof(float)));
  if (keep_gauss) HIPCHK(Y.gauss.ensure((size_t)tot * P.NS * nimg * sizeof(float)));
  HIPCHK(Y.seeds.ensure((size_t)seeds_pi * nimg * sizeof(double)));
  HIPCHK(hipEventRecord(ctx->ev[kEvUpload], ctx->stream));
  if (o_first > 0) {
    const Octave& of = P.oct[o_first];
    HIPCHK(hipMemcpyAsync(Y.seeds.as<double>() + of.seed_off, q.seed_host ? (const void*)q.seed_host : q.seed_dev,
                          (size_t)of.h * of.w * sizeof(double),
                          q.seed_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    P.img = nullptr;
    P.img_stride = 0;
  } else if (q.img_host) {  // (a batch: image b from img_host + b * img_bstride, dense on the device)
    // Through the context's pinned staging, pipelined (h2d_rows_staged): the
    // rows are copied on several host threads (the runtime's pageable path
    // stages them on one thread).  The staging is refilled only after the
    // previous DMA out of it has completed.
    const size_t img_bytes = (size_t)W * H * nimg * sizeof(float);
    HIPCHK(Y.img.ensure(img_bytes));
    const bool dense = q.stride == (size_t)W && (nimg == 1 || q.img_bstride == (size_t)W * H);
    if (dense && host_registered(q.img_host, img_bytes)) {
      // page-locked caller memory (sift_host_register): one DMA straight from
      // it -- every host-image entry point synchronises before it returns
      HIPCHK(hipMemcpyAsync(Y.img.p, q.img_host, img_bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
      if (!Y.ev_himg[0]) HIPCHK(Y.ev_himg.ensure());
      else HIPCHK(hipEventSynchronize(Y.ev_himg[0]));
      HIPCHK(Y.himg.ensure(img_bytes));
      for (int b = 0; b < nimg; ++b)
        HIPCHK(h2d_rows_staged(Y.img.as<float>() + (size_t)b * W * H, (float*)Y.himg.p + (size_t)b * W * H,
                               q.img_host + (size_t)b * q.img_bstride, q.stride * sizeof(float), W * sizeof(float), H,
                               host_threads(), ctx->stream));
      HIPCHK(hipEventRecord(Y.ev_himg[0], ctx->stream));
    }
    P.img = Y.img.as<float>();
    P.img_stride = W;
    P.img_bstride = nimg > 1 ? (long long)W * H : 0;
  } else {
    P.img = q.img_dev;
    P.img_stride = (int)q.stride;
  }
  P.seeds = Y.seeds.as<double>();
  P.dog = Y.dog.as<float>();
  {  // large-radius octaves keep their fp64 Gaussian planes (the exact passes read them)
    long long l64 = 0;
    for (int o = so_end; o < P.O; ++o)
      if (plan[o].keep_l64) {
        P.oct[o].l64_off = l64;
        l64 += (long long)P.NS * P.oct[o].h * P.oct[o].w;
      }
    if (l64) HIPCHK(Y.l64.ensure((size_t)l64 * nimg * sizeof(double)));
    P.l64 = l64 ? Y.l64.as<double>() : nullptr;
    P.l64_bstride = l64;
    size_t vs = 0;  // the split-pass octaves run in turn on this stream: one scratch (per image)
    for (int o = so_end; o < P.O; ++o)
      if (plan[o].vsplit) vs = std::max(vs, (size_t)P.NS * P.oct[o].h * P.oct[o].w);
    size_t sv = 0;
    for (int o = o_first; o < so_end; ++o) sv = std::max(sv, seed_only_scratch(P, o));
    if (sv) HIPCHK(Y.seedv.ensure(sv * sizeof(double)));
    if (vs) HIPCHK(Y.vsplit.ensure(vs * nimg * sizeof(double)));
    Y.vsplit_pi = (long long)vs;
    // after the pass the scratch holds the last split octave's sums (octaves run in order)
    P.vsum_oct = -1;
    for (int o = so_end; o < P.O; ++o)
      if (plan[o].vsplit) P.vsum_oct = o;
    static const int vsum_exact = exp_knob("SIFT_VSUM_EXACT", 1);  // 0: the exact passes recompute (A/B)
    if (!vsum_exact) P.vsum_oct = -1;
    P.vsum = P.vsum_oct >= 0 ? Y.vsplit.as<double>() : nullptr;
    P.vsum_bstride = Y.vsplit_pi;
  }
  HIPCHK(hipEventRecord(ctx->ev[kEvPass], ctx->stream));
  const double* base0 = nullptr;
  if (o_first == 0 && needs_base0) {
    HIPCHK(Y.base0.ensure((size_t)P.oct[0].h * P.oct[0].w * sizeof(double)));
    HIPCHK(launch_upsample_base(P, Y.base0.as<double>(), ctx->stream));
    base0 = Y.base0.as<double>();
  }
  ctx->ext.prepared = false;
  const int nf = (q.fuse_extrema && o_first == 0 && fuse_enabled(p) && plan[0].can_fuse &&
                  !(p->flags & SIFT_F_LOW_CONTRAST_LIST)) ? 1 : 0;
  if (nf) {  // bitmap geometry, counter resets: before the fused launch writes them
    Y.dog_source = kNative;
    rc = extrema_prepare(ctx, ctx->stream, nf);
    if (rc) return rc;
    ctx->ext.prepared = true;
  }
  const bool xseed = (p->flags & SIFT_F_EXPORT_NEXT_SEED) != 0;
  if (xseed) {
    Sh.xseed_h = (P.oct[P.O - 1].h + 1) / 2;  // background.js:118
    Sh.xseed_w = (P.oct[P.O - 1].w + 1) / 2;
    HIPCHK(Sh.xseed.ensure((size_t)Sh.xseed_h * Sh.xseed_w * sizeof(double)));
  }
  Y.pass_kn.assign(P.O, std::string());
  for (int o = o_first; o < P.O; ++o) {
    const Octave& oc = P.oct[o];
    if (o < so_end) {
      Y.pass_kn[o] = "k_seed_vert + k_seed_horz (next base only)";
      HIPCHK(launch_seed_only(P, o, Y.seeds.as<double>() + oc.seed_off, Y.seedv.as<double>(),
                              Y.seeds.as<double>() + P.oct[o + 1].seed_off, ctx->stream));
      if (o == o_first) HIPCHK(hipEventRecord(ctx->ev[kEvOct0], ctx->stream));
      HIPCHK(hipEventRecord(Y.ev_go[o], ctx->stream));
      continue;
    }
    GaussLaunch L{};
    L.o = o;
    L.base = o == 0 ? base0 : Y.seeds.as<double>() + oc.seed_off;
    L.gauss = keep_gauss ? Y.gauss.as<float>() + oc.gauss_off : nullptr;
    L.dog = Y.dog.as<float>() + oc.dog_off;
    L.next_seed = (o + 1 < P.O) ? Y.seeds.as<double>() + P.oct[o + 1].seed_off
                                : (xseed ? Sh.xseed.as<double>() : nullptr);
    L.next_w = (o + 1 < P.O) ? P.oct[o + 1].w : (xseed ? Sh.xseed_w : 0);
    if (o < nf) {
      const ExtremaLaunch& XL = ctx->ext.xl;
      L.fuse = 1;
      L.X.bitmap = XL.bitmap + XL.G.word_off[o];
      L.X.rowcount = XL.rowcount + XL.G.row_off[o];
      L.X.nw = XL.G.nw[o];
      L.X.amb_keys = XL.amb_keys;
      L.X.counters = XL.counters;
      L.X.amb_cap = XL.amb_cap;
      L.X.c_lo = XL.c_lo;
      L.X.c_hi = XL.c_hi;
    }
    L.l64 = P.oct[o].l64_off >= 0 ? Y.l64.as<double>() + P.oct[o].l64_off : nullptr;
    L.vsplit = plan[o].vsplit ? Y.vsplit.as<double>() : nullptr;
    L.nimg = nimg;
    L.gauss_bs = tot * P.NS;
    L.dog_bs = tot * P.ND;
    L.seed_bs = seeds_pi;
    L.base_bs = o == 0 ? 0 : seeds_pi;
    L.l64_bs = P.l64_bstride;
    L.vsplit_bs = Y.vsplit_pi;
    HIPCHK(launch_gauss_dog(P, plan[o], L, ctx->stream, &Y.glaunch[o]));
    Y.pass_kn[o] = L.fuse ? kGaussFusedName : plan[o].kname;
    if (o == o_first) HIPCHK(hipEventRecord(ctx->ev[kEvOct0], ctx->stream));
    HIPCHK(hipEventRecord(Y.ev_go[o], ctx->stream));
  }
  HIPCHK(hipEventRecord(ctx->ev[kEvPassEnd], ctx->stream));
  Y.dog_source = kNative;
  Y.have_gauss = keep_gauss;
  drop_results(ctx, true);
  Sh.has_xseed = xseed;
  return SIFT_OK;
}

// Gaussian+DoG timings of the last build (its events must have completed):
// the whole pass, octave 0's launch and every octave's launch.
void sift::read_gauss_times(sift_ctx* ctx) {
  PyrState& Y = ctx->pyr;
  take_event_ms(&ctx->tm.gauss_dog_ms, ctx->ev[kEvPass], ctx->ev[kEvPassEnd]);
  take_event_ms(&ctx->tm.gauss_oct0_ms, ctx->ev[kEvPass], ctx->ev[kEvOct0]);
  Y.oct_ms.assign(ctx->P.O, 0.0);
  hipEvent_t prev = ctx->ev[kEvPass];
  for (int o = Y.o_first; o < ctx->P.O; ++o) {
    take_event_ms(&Y.oct_ms[o], prev, Y.ev_go[o]);
    prev = Y.ev_go[o];
  }
}

// A page-locked caller image is uploaded by one DMA straight from the
// caller's memory (build_common), which every host-image entry point waits
// for before it returns -- on its error exits too, so the caller
// may free or overwrite the image as soon as the call returns.
int sift::host_image_exit(sift_ctx* ctx, int rc) {
  if (rc != SIFT_OK && ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// Device plane (kind, o, s) of the pyramid and its pixel count, for a
// destination of cap_px pixels (too_small: the message when it is not enough).
int sift::find_plane(sift_ctx* ctx, int kind, int o, int s, size_t cap_px, const char* too_small, const float** src,
                     size_t* plane_px) {
  const Pyramid& P = ctx->P;
  if (o < 0 || o >= P.O) return set_err(ctx, SIFT_E_ARG, "octave out of range");
  if (o < ctx->pyr.planes_first) return set_err(ctx, SIFT_E_STATE, "octave not built (sift_detect_from_seed[_range])");
  const Octave& oc = P.oct[o];
  const size_t plane = (size_t)oc.h * oc.w;
  if (cap_px < plane) return set_err(ctx, SIFT_E_CAPACITY, too_small);
  if (kind == SIFT_PLANE_GAUSS) {
    if (!ctx->pyr.have_gauss) return set_err(ctx, SIFT_E_STATE, "Gaussian planes not materialised");
    if (s < 0 || s >= P.NS) return set_err(ctx, SIFT_E_ARG, "scale out of range");
    *src = ctx->pyr.gauss.as<float>() + oc.gauss_off + (size_t)s * plane;
  } else if (kind == SIFT_PLANE_DOG) {
    if (s < 0 || s >= P.ND) return set_err(ctx, SIFT_E_ARG, "scale out of range");
    *src = ctx->pyr.dog.as<float>() + oc.dog_off + (size_t)s * plane;
  } else {
    return set_err(ctx, SIFT_E_ARG, "bad plane kind");
  }
  *plane_px = plane;
  return SIFT_OK;
}

// The context after caller-supplied planes were queued for upload (sift_load_*).
static int finish_load(sift_ctx* ctx, bool have_gauss) {
  PyrState& Y = ctx->pyr;
  ctx->P.dog = Y.dog.as<float>();
  ctx->P.img = nullptr;
  ctx->P.seeds = nullptr;
  Y.dog_source = kForeign;
  Y.o_first = Y.scan_first = Y.planes_first = 0;
  Y.have_gauss = have_gauss;
  drop_results(ctx, true);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

// The pyramid of one image, waited for.
static int build_scale_space(sift_ctx* ctx, BuildRequest q, const double* sig) {
  q.sig = sig;
  int rc = build_common(ctx, q);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->tm.h2d_ms = q.img_host ? event_ms(ctx->ev[kEvUpload], ctx->ev[kEvPass]) : 0;
  read_gauss_times(ctx);
  return SIFT_OK;
}

int sift_build_scale_space(sift_ctx* ctx, const float* img, int width, int height, size_t stride_px,
                           const sift_params* p, const double* sig) {
  return host_image_exit(ctx, build_scale_space(ctx, image_request(img, nullptr, width, height, stride_px, p), sig));
}

int sift_build_scale_space_device(sift_ctx* ctx, const float* d_img, int width, int height,
                                  size_t stride_px, const sift_params* p, const double* sig) {
  return build_scale_space(ctx, image_request(nullptr, d_img, width, height, stride_px, p), sig);
}

int sift_get_dims(sift_ctx* ctx, int o, int* rows, int* cols) {
  if (!ctx || !rows || !cols) return SIFT_E_ARG;
  if (ctx->pyr.dog_source == kNone) return set_err(ctx, SIFT_E_STATE, "no pyramid");
  if (o < 0 || o >= ctx->P.O) return set_err(ctx, SIFT_E_ARG, "octave out of range");
  *rows = ctx->P.oct[o].h;
  *cols = ctx->P.oct[o].w;
  return SIFT_OK;
}

int sift_last_gauss_plan(sift_ctx* ctx, int o, sift_gauss_plan_info* out) {
  if (!ctx || !out) return SIFT_E_ARG;
  const PyrState& Y = ctx->pyr;
  if (Y.dog_source != kNative) return set_err(ctx, SIFT_E_STATE, "no pyramid built here");
  if (o < 0 || o >= ctx->P.O) return set_err(ctx, SIFT_E_ARG, "octave out of range");
  const GaussPlan& G = Y.gplan[o];
  const GaussLaunched& L = Y.glaunch[o];
  if (!L.valid) return set_err(ctx, SIFT_E_STATE, "octave not built (sift_detect_from_seed[_range])");
  std::memset(out, 0, sizeof(*out));
  out->kernel = L.kernel;
  out->path = G.path;
  out->rw = G.rw;
  out->tile_w = G.tile_w;
  out->tile_rows = G.tile_rows;
  out->gx = L.gx;
  out->gy = L.gy;
  out->G = L.G;
  std::copy(G.gb, G.gb + L.G + 1, out->gb);
  out->sw = G.sw;
  out->zero = G.zero;
  out->keep_l64 = G.keep_l64;
  out->vsplit = G.vsplit;
  out->xcd_band = G.xcd_band;
  out->vec = L.vec;
  out->fused = L.fuse;
  return SIFT_OK;
}

int sift_get_blur_level(sift_ctx* ctx, int kind, int o, int s, double* blur) {
  if (!ctx || !blur) return SIFT_E_ARG;
  if (ctx->pyr.dog_source == kNone) return set_err(ctx, SIFT_E_STATE, "no pyramid");
  const int lim = kind == SIFT_PLANE_GAUSS ? ctx->P.NS : ctx->P.ND;
  if (o < 0 || o >= ctx->P.O || s < 0 || s >= lim) return set_err(ctx, SIFT_E_ARG, "index out of range");
  // DoG[s] carries L[s-1+1-1] = L[s].blurLevel (background.js:326-329).
  *blur = ctx->pyr.blur[o * ctx->P.NS + s];
  return SIFT_OK;
}

int sift_get_plane(sift_ctx* ctx, int kind, int o, int s, float* dst, size_t cap_px) {
  if (!ctx || !dst) return SIFT_E_ARG;
  if (ctx->pyr.dog_source == kNone) return set_err(ctx, SIFT_E_STATE, "no pyramid");
  const float* src = nullptr;
  size_t plane = 0;
  const int rc = find_plane(ctx, kind, o, s, cap_px, "destination too small", &src, &plane);
  if (rc) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(d2h_staged(ctx, dst, src, plane * sizeof(float)));
  return SIFT_OK;
}

int sift_load_dog(sift_ctx* ctx, const float* planes, int width, int height, const sift_params* p) {
  if (!ctx || !planes) return SIFT_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  int rc = setup_geometry(ctx, width, height, p, nullptr, false);
  if (rc) return rc;
  const long long tot = total_plane_px(ctx);
  HIPCHK(ctx->pyr.dog.ensure((size_t)tot * ctx->P.ND * sizeof(float)));
  HIPCHK(hipMemcpyAsync(ctx->pyr.dog.p, planes, (size_t)tot * ctx->P.ND * sizeof(float),
                        hipMemcpyHostToDevice, ctx->stream));
  return finish_load(ctx, false);
}

int sift_load_scale_space(sift_ctx* ctx, const float* planes, int width, int height,
                          const sift_params* p) {
  if (!ctx || !planes) return SIFT_E_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  int rc = setup_geometry(ctx, width, height, p, nullptr, false);
  if (rc) return rc;
  const Pyramid& P = ctx->P;
  PyrState& Y = ctx->pyr;
  const long long tot = total_plane_px(ctx);
  HIPCHK(Y.gauss.ensure((size_t)tot * P.NS * sizeof(float)));
  HIPCHK(Y.dog.ensure((size_t)tot * P.ND * sizeof(float)));
  HIPCHK(hipMemcpyAsync(Y.gauss.p, planes, (size_t)tot * P.NS * sizeof(float),
                        hipMemcpyHostToDevice, ctx->stream));
  for (int o = 0; o < P.O; ++o) {
    const Octave& oc = P.oct[o];
    HIPCHK(launch_dog_from_gauss(Y.gauss.as<float>() + oc.gauss_off, Y.dog.as<float>() + oc.dog_off,
                                 (long long)oc.h * oc.w, P.ND, ctx->stream));
  }
  return finish_load(ctx, true);
}
