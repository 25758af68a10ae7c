// C ABI of guided descriptor matching: nearest neighbours within a radius of H x (kernels: sift_guided.hip).
#include "sift_ctx.h"

using namespace sift;

static_assert(sizeof(sift_point) == 16 && sizeof(double2) == 16, "16-byte positions");
static_assert(sizeof(sift_guided_info) == 40, "40-byte info");
static_assert(kGuidedMaxCells == SIFT_GUIDED_MAX_CELLS, "guided constants of include/sift_hip.h");

namespace {

struct GuidedRows {
  const uint8_t* rows;
  const uint8_t* mask;
  const double2* xy;
  size_t n;
};

// The limits of include/sift_hip.h, those of the model and the train size first; nothing has been written when
// either fails.
int guided_model_check(sift_ctx* ctx, int width, int height, const double* h, double radius) {
  if (!h) return set_err(ctx, SIFT_E_ARG, "null homography");
  if (!(std::isfinite(radius) && radius > 0.0)) return set_err(ctx, SIFT_E_ARG, "radius must be finite and > 0");
  if (width <= 0 || height <= 0) return set_err(ctx, SIFT_E_ARG, "the train size must be positive");
  return SIFT_OK;
}

int guided_check(sift_ctx* ctx, const GuidedRows& q, const GuidedRows& t, int width, int height, const double* h,
                 double radius, const void* out) {
  if (!count_ok(q.n) || !count_ok(t.n)) return set_err(ctx, SIFT_E_ARG, "too many descriptors");
  if ((q.n && (!q.rows || !q.xy || !out)) || (t.n && (!t.rows || !t.xy)))
    return set_err(ctx, SIFT_E_ARG, "null descriptor, position or result pointer");
  return guided_model_check(ctx, width, height, h, radius);
}

// The guided match of validated device arrays into d_out (q.n records), timed and complete on return, with its info.
// Nothing between the stages is read back: no launch's size depends on device data.
int guided_run(sift_ctx* ctx, const GuidedRows& q, const GuidedRows& t, int width, int height, const double* h,
               double radius, Match* d_out) {
  GuidedState& G = ctx->guided;
  G.have = false;
  G.grid_ms = G.match_ms = 0;
  HIPCHK(G.ev.ensure());
  HIPCHK(G.hinfo.ensure(3 * sizeof(unsigned long long)));
  const GuidedGrid grid = guided_grid(width, height, radius);
  const size_t cells = (size_t)grid.ncx * grid.ncy;
  const int nq = (int)q.n, nt = (int)t.n;
  const size_t nt1 = std::max<size_t>(t.n, 1);
  HIPCHK(G.count.ensure((cells + 1) * sizeof(unsigned)));
  HIPCHK(G.off.ensure((cells + 1) * sizeof(unsigned)));
  HIPCHK(G.cell.ensure(nt1 * sizeof(int)));
  HIPCHK(G.fxy.ensure(nt1 * sizeof(double2)));
  HIPCHK(G.ftag.ensure(nt1 * sizeof(int2)));
  HIPCHK(G.frows.ensure(nt1 * kDescBytes));
  HIPCHK(G.info.ensure(3 * sizeof(unsigned long long)));
  const GuidedFiled filed{G.fxy.as<double2>(), G.ftag.as<int2>(), G.frows.as<unsigned char>()};
  unsigned long long* hinfo = G.hinfo.as<unsigned long long>();

  HIPCHK(hipEventRecord(G.ev[0], ctx->stream));
  HIPCHK(hipMemsetAsync(G.count.p, 0, (cells + 1) * sizeof(unsigned), ctx->stream));
  HIPCHK(hipMemsetAsync(G.info.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
  HIPCHK(launch_guided_cells(t.xy, t.mask, nt, grid, G.cell.as<int>(), G.count.as<unsigned>(), ctx->stream));
  HIPCHK(exclusive_sum(ctx, G.count.as<unsigned>(), G.off.as<unsigned>(), (int)(cells + 1)));
  HIPCHK(launch_guided_fill(t.rows, t.xy, G.cell.as<int>(), nt, G.off.as<unsigned>(), G.count.as<unsigned>(), filed,
                            ctx->stream));
  HIPCHK(hipEventRecord(G.ev[1], ctx->stream));
  GuidedMatch M{};
  M.query = q.rows;
  M.qmask = q.mask;
  M.qxy = q.xy;
  M.n_query = nq;
  std::memcpy(M.h, h, sizeof M.h);
  M.radius = radius;
  M.r2 = radius * radius;
  M.grid = grid;
  M.off = G.off.as<unsigned>();
  M.filed = filed;
  M.out = d_out;
  M.info = G.info.as<unsigned long long>();
  HIPCHK(launch_guided_match(M, ctx->stream));
  HIPCHK(hipEventRecord(G.ev[2], ctx->stream));
  HIPCHK(hipMemcpyAsync(hinfo, G.info.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  G.grid_ms = event_ms(G.ev[0], G.ev[1]);
  G.match_ms = event_ms(G.ev[1], G.ev[2]);
  G.last = sift_guided_info{grid.cell_px, grid.ncx, grid.ncy, 0, (int64_t)hinfo[0], (int64_t)hinfo[1],
                            (int64_t)hinfo[2]};
  G.have = true;
  return SIFT_OK;
}

// guided_run into ctx->match.out, which becomes the context's last match.
int guided_keep(sift_ctx* ctx, const GuidedRows& q, const GuidedRows& t, int width, int height, const double* h,
                double radius) {
  MatchState& M = ctx->match;
  HIPCHK(M.out.ensure(std::max<size_t>(q.n, 1) * sizeof(Match)));
  M.have = false;
  if (int rc = guided_run(ctx, q, t, width, height, h, radius, M.out.as<Match>())) return rc;
  M.n = q.n;
  M.have = true;
  return SIFT_OK;
}

}  // namespace

int sift_match_guided_device(sift_ctx* ctx, const uint8_t* d_query, const uint8_t* d_query_mask,
                             const sift_point* d_query_xy, size_t n_query, const uint8_t* d_train,
                             const uint8_t* d_train_mask, const sift_point* d_train_xy, size_t n_train, int train_width,
                             int train_height, const double h[9], double radius, struct sift_match* d_out) {
  if (!ctx) return SIFT_E_ARG;
  const GuidedRows q{d_query, d_query_mask, reinterpret_cast<const double2*>(d_query_xy), n_query};
  const GuidedRows t{d_train, d_train_mask, reinterpret_cast<const double2*>(d_train_xy), n_train};
  if (int rc = guided_check(ctx, q, t, train_width, train_height, h, radius, d_out)) return rc;
  if (((n_query ? (uintptr_t)d_query : 0) | (n_train ? (uintptr_t)d_train : 0)) & 15)
    return set_err(ctx, SIFT_E_ARG, "descriptors not 16-byte aligned");
  HIPCHK(hipSetDevice(ctx->device));
  return guided_run(ctx, q, t, train_width, train_height, h, radius, reinterpret_cast<Match*>(d_out));
}

int sift_match_guided(sift_ctx* ctx, const uint8_t* query, const uint8_t* query_mask, const sift_point* query_xy,
                      size_t n_query, const uint8_t* train, const uint8_t* train_mask, const sift_point* train_xy,
                      size_t n_train, int train_width, int train_height, const double h[9], double radius,
                      struct sift_match* out) {
  if (!ctx) return SIFT_E_ARG;
  {
    const GuidedRows q{query, query_mask, reinterpret_cast<const double2*>(query_xy), n_query};
    const GuidedRows t{train, train_mask, reinterpret_cast<const double2*>(train_xy), n_train};
    if (int rc = guided_check(ctx, q, t, train_width, train_height, h, radius, out)) return rc;
  }
  HIPCHK(hipSetDevice(ctx->device));
  GuidedState& G = ctx->guided;
  if (int rc = h2d_buffer(ctx, G.in_q, query, n_query * kDescBytes)) return rc;
  if (int rc = h2d_buffer(ctx, G.in_qm, n_query ? query_mask : nullptr, n_query)) return rc;
  if (int rc = h2d_buffer(ctx, G.in_qxy, query_xy, n_query * sizeof(double2))) return rc;
  if (int rc = h2d_buffer(ctx, G.in_t, train, n_train * kDescBytes)) return rc;
  if (int rc = h2d_buffer(ctx, G.in_tm, n_train ? train_mask : nullptr, n_train)) return rc;
  if (int rc = h2d_buffer(ctx, G.in_txy, train_xy, n_train * sizeof(double2))) return rc;
  const GuidedRows q{G.in_q.as<uint8_t>(), n_query && query_mask ? G.in_qm.as<uint8_t>() : nullptr,
                     G.in_qxy.as<double2>(), n_query};
  const GuidedRows t{G.in_t.as<uint8_t>(), n_train && train_mask ? G.in_tm.as<uint8_t>() : nullptr,
                     G.in_txy.as<double2>(), n_train};
  if (int rc = guided_keep(ctx, q, t, train_width, train_height, h, radius)) return rc;
  if (n_query) HIPCHK(d2h_staged(ctx, out, ctx->match.out.p, n_query * sizeof(Match)));
  return SIFT_OK;
}

int sift_match_features_guided(sift_ctx* ctx, sift_ctx* train_ctx, const double h[9], double radius,
                               struct sift_match* out, size_t cap, size_t* n_out) {
  if (!ctx || !train_ctx) return SIFT_E_ARG;
  if (!stage_has(ctx, kNeedDesc) || !stage_has(train_ctx, kNeedDesc))
    return set_err(ctx, SIFT_E_STATE, "no descriptors: run sift_orient and sift_describe on both contexts first");
  if (ctx->device != train_ctx->device) return set_err(ctx, SIFT_E_ARG, "contexts on different devices");
  const FeatState &Q = ctx->feat, &T = train_ctx->feat;
  const size_t nq = Q.n_ori, nt = T.n_ori;  // both below 2^31 - 1 (sift_orient's scan, sift_set_orientations)
  if (!count_ok(nq) || !count_ok(nt)) return set_err(ctx, SIFT_E_ARG, "too many descriptors");
  if (int rc = guided_model_check(ctx, train_ctx->P.W, train_ctx->P.H, h, radius)) return rc;
  GuidedState& G = ctx->guided;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(G.in_qxy.ensure(std::max<size_t>(nq, 1) * sizeof(double2)));
  HIPCHK(G.in_txy.ensure(std::max<size_t>(nt, 1) * sizeof(double2)));
  const GuidedRows q{Q.desc.as<uint8_t>(), Q.desc_ok.as<uint8_t>(), G.in_qxy.as<double2>(), nq};
  const GuidedRows t{T.desc.as<uint8_t>(), T.desc_ok.as<uint8_t>(), G.in_txy.as<double2>(), nt};
  HIPCHK(launch_guided_gather(Q.ori.as<Orientation>(), (int)nq, ctx->kp.as<Keypoint>(), (int)ctx->n_kp,
                              G.in_qxy.as<double2>(), ctx->stream));
  HIPCHK(launch_guided_gather(T.ori.as<Orientation>(), (int)nt, train_ctx->kp.as<Keypoint>(), (int)train_ctx->n_kp,
                              G.in_txy.as<double2>(), ctx->stream));
  if (int rc = guided_keep(ctx, q, t, train_ctx->P.W, train_ctx->P.H, h, radius)) return rc;
  if (n_out) *n_out = nq;
  if (!out) return SIFT_OK;
  if (cap < nq) return set_err(ctx, SIFT_E_CAPACITY, "match buffer too small");
  if (nq) HIPCHK(d2h_staged(ctx, out, ctx->match.out.p, nq * sizeof(Match)));
  return SIFT_OK;
}

int sift_last_guided_info(sift_ctx* ctx, sift_guided_info* out) {
  if (!ctx || !out) return SIFT_E_ARG;
  if (!ctx->guided.have) return set_err(ctx, SIFT_E_STATE, "no guided match: run sift_match_guided first");
  *out = ctx->guided.last;
  return SIFT_OK;
}

int sift_last_guided_timings(sift_ctx* ctx, double* grid_ms, double* match_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (grid_ms) *grid_ms = ctx->guided.grid_ms;
  if (match_ms) *match_ms = ctx->guided.match_ms;
  return SIFT_OK;
}
