// C ABI of descriptor matching and of the selection of match pairs (kernels: sift_match.hip).
#include "sift_ctx.h"

using namespace sift;

static_assert(sizeof(struct sift_match) == 16 && sizeof(Match) == 16 && sizeof(sift_match_pair) == 16 &&
                  sizeof(MatchPair) == 16,
              "16-byte match records");
static_assert(SIFT_MATCH_NONE_D2 == INT32_MAX && kDescBytes == SIFT_DESC_BYTES, "match constants of include/sift_hip.h");

// The match of validated device arrays into d_out (n_query records), timed and complete on return.
static int match_run(sift_ctx* ctx, const uint8_t* d_q, const uint8_t* d_qm, int nq, const uint8_t* d_t,
                     const uint8_t* d_tm, int nt, Match* d_out) {
  MatchState& M = ctx->match;
  HIPCHK(M.ev.ensure());
  M.match_ms = 0;
  if (nq == 0) return SIFT_OK;
  const MatchSplit sp = match_split(nq, nt);
  Match* part = d_out;
  if (nt > 0) {
    const size_t qrows = (size_t)match_query_rows(nq), trows = (size_t)match_train_rows(nt);
    HIPCHK(M.qs.ensure(qrows * kDescBytes));
    HIPCHK(M.qn.ensure(qrows * sizeof(int)));
    HIPCHK(M.ts.ensure(trows * kDescBytes));
    HIPCHK(M.kb.ensure(trows * sizeof(int)));
    if (sp.splits > 1) {
      HIPCHK(M.part.ensure((size_t)sp.splits * nq * sizeof(Match)));
      part = M.part.as<Match>();
    }
    HIPCHK(hipEventRecord(M.ev[0], ctx->stream));
    HIPCHK(launch_match_prep(d_q, d_qm, nq, (long long)qrows, 0, M.qs.as<unsigned char>(), M.qn.as<int>(),
                             ctx->stream));
    HIPCHK(launch_match_prep(d_t, d_tm, nt, (long long)trows, 1, M.ts.as<unsigned char>(), M.kb.as<int>(),
                             ctx->stream));
    HIPCHK(launch_match(M.qs.as<unsigned char>(), M.qn.as<int>(), nq, M.ts.as<unsigned char>(), M.kb.as<int>(), nt,
                        part, ctx->stream));
    if (sp.splits > 1) HIPCHK(launch_match_merge(part, sp.splits, nq, d_out, ctx->stream));
  } else {
    HIPCHK(hipEventRecord(M.ev[0], ctx->stream));
    HIPCHK(launch_match_merge(nullptr, 0, nq, d_out, ctx->stream));  // no train rows: every neighbour missing
  }
  HIPCHK(hipEventRecord(M.ev[1], ctx->stream));
  HIPCHK(hipEventSynchronize(M.ev[1]));
  M.match_ms = event_ms(M.ev[0], M.ev[1]);
  return SIFT_OK;
}

// match_run into ctx->match.out, which becomes the context's last match.
static int match_keep(sift_ctx* ctx, const uint8_t* d_q, const uint8_t* d_qm, size_t nq, const uint8_t* d_t,
                      const uint8_t* d_tm, size_t nt) {
  MatchState& M = ctx->match;
  HIPCHK(M.out.ensure(std::max<size_t>(nq, 1) * sizeof(Match)));
  M.have = false;
  if (int rc = match_run(ctx, d_q, d_qm, (int)nq, d_t, d_tm, (int)nt, M.out.as<Match>())) return rc;
  M.n = nq;
  M.have = true;
  return SIFT_OK;
}

static int select_check(sift_ctx* ctx, const void* fwd, size_t n_query, size_t n_train, double ratio) {
  if (!count_ok(n_query) || !count_ok(n_train)) return set_err(ctx, SIFT_E_ARG, "too many records");
  if (n_query && !fwd) return set_err(ctx, SIFT_E_ARG, "null match records");
  if (!(ratio <= 0.0) && !(std::isfinite(ratio) && ratio < 1.0))  // a NaN fails both
    return set_err(ctx, SIFT_E_ARG, "ratio must be below 1, or <= 0 for no ratio test");
  return SIFT_OK;
}

// The selection over validated device records, timed: the pair count always,
// the ordered pairs into d_pairs when it is given and cap holds them.
static int select_run(sift_ctx* ctx, const Match* fwd, size_t n_query, const Match* rev, size_t n_train, double ratio,
                      MatchPair* d_pairs, size_t cap, size_t* n_out) {
  MatchState& M = ctx->match;
  M.select_ms = 0;
  if (n_out) *n_out = 0;
  if (!n_query) return SIFT_OK;
  const int nq = (int)n_query;
  HIPCHK(M.ev.ensure());
  HIPCHK(M.flag.ensure((size_t)(nq + 1) * sizeof(unsigned)));
  HIPCHK(M.off.ensure((size_t)(nq + 1) * sizeof(unsigned)));
  HIPCHK(hipEventRecord(M.ev[2], ctx->stream));
  HIPCHK(launch_match_flag(fwd, nq, rev, (int)n_train, ratio > 0.0 ? ratio * ratio : 0.0, M.flag.as<unsigned>(),
                           ctx->stream));
  unsigned total = 0;
  if (int rc = ordered_total(ctx, M.flag.as<unsigned>(), M.off.as<unsigned>(), nq, &total)) return rc;
  if (n_out) *n_out = total;
  const bool fits = cap >= total;
  if (d_pairs && fits)
    HIPCHK(launch_match_emit(fwd, M.flag.as<unsigned>(), M.off.as<unsigned>(), nq, total, d_pairs, ctx->stream));
  HIPCHK(hipEventRecord(M.ev[3], ctx->stream));
  HIPCHK(hipEventSynchronize(M.ev[3]));
  M.select_ms = event_ms(M.ev[2], M.ev[3]);
  if (d_pairs && !fits) return set_err(ctx, SIFT_E_CAPACITY, "pair buffer too small");
  return SIFT_OK;
}

int sift_match_device(sift_ctx* ctx, const uint8_t* d_query, const uint8_t* d_query_mask, size_t n_query,
                      const uint8_t* d_train, const uint8_t* d_train_mask, size_t n_train, struct sift_match* d_out) {
  if (!ctx) return SIFT_E_ARG;
  if (!count_ok(n_query) || !count_ok(n_train)) return set_err(ctx, SIFT_E_ARG, "too many descriptors");
  if ((n_query && (!d_query || !d_out)) || (n_train && !d_train))
    return set_err(ctx, SIFT_E_ARG, "null descriptor or result pointer");
  if (((uintptr_t)d_query | (uintptr_t)d_train) & 15) return set_err(ctx, SIFT_E_ARG, "descriptors not 16-byte aligned");
  HIPCHK(hipSetDevice(ctx->device));
  return match_run(ctx, d_query, d_query_mask, (int)n_query, d_train, d_train_mask, (int)n_train,
                   reinterpret_cast<Match*>(d_out));
}

int sift_match(sift_ctx* ctx, const uint8_t* query, const uint8_t* query_mask, size_t n_query, const uint8_t* train,
               const uint8_t* train_mask, size_t n_train, struct sift_match* out) {
  if (!ctx) return SIFT_E_ARG;
  if (!count_ok(n_query) || !count_ok(n_train)) return set_err(ctx, SIFT_E_ARG, "too many descriptors");
  if ((n_query && (!query || !out)) || (n_train && !train))
    return set_err(ctx, SIFT_E_ARG, "null descriptor or result pointer");
  HIPCHK(hipSetDevice(ctx->device));
  MatchState& M = ctx->match;
  if (n_query == 0) return match_keep(ctx, nullptr, nullptr, 0, nullptr, nullptr, 0);  // the last match has no records
  if (int rc = h2d_buffer(ctx, M.in_q, query, n_query * kDescBytes)) return rc;
  if (int rc = h2d_buffer(ctx, M.in_qm, query_mask, n_query)) return rc;
  if (int rc = h2d_buffer(ctx, M.in_t, train, n_train * kDescBytes)) return rc;
  if (int rc = h2d_buffer(ctx, M.in_tm, n_train ? train_mask : nullptr, n_train)) return rc;
  if (int rc = match_keep(ctx, M.in_q.as<uint8_t>(), query_mask ? M.in_qm.as<uint8_t>() : nullptr, n_query,
                          M.in_t.as<uint8_t>(), n_train && train_mask ? M.in_tm.as<uint8_t>() : nullptr, n_train))
    return rc;
  HIPCHK(d2h_staged(ctx, out, M.out.p, n_query * sizeof(Match)));
  return SIFT_OK;
}

int sift_match_features(sift_ctx* ctx, sift_ctx* train_ctx, struct sift_match* out, size_t cap, size_t* n_out) {
  if (!ctx || !train_ctx) return SIFT_E_ARG;
  if (!stage_has(ctx, kNeedDesc) || !stage_has(train_ctx, kNeedDesc))
    return set_err(ctx, SIFT_E_STATE, "no descriptors: run sift_orient and sift_describe on both contexts first");
  if (ctx->device != train_ctx->device) return set_err(ctx, SIFT_E_ARG, "contexts on different devices");
  HIPCHK(hipSetDevice(ctx->device));
  const FeatState &Q = ctx->feat, &T = train_ctx->feat;
  const size_t nq = Q.n_ori, nt = T.n_ori;  // both below 2^31 - 1 (sift_orient's scan, sift_set_orientations)
  if (!count_ok(nq) || !count_ok(nt)) return set_err(ctx, SIFT_E_ARG, "too many descriptors");
  if (int rc = match_keep(ctx, Q.desc.as<uint8_t>(), Q.desc_ok.as<uint8_t>(), nq, T.desc.as<uint8_t>(),
                          T.desc_ok.as<uint8_t>(), nt))
    return rc;
  if (n_out) *n_out = nq;
  if (!out) return SIFT_OK;
  if (cap < nq) return set_err(ctx, SIFT_E_CAPACITY, "match buffer too small");
  if (nq) HIPCHK(d2h_staged(ctx, out, ctx->match.out.p, nq * sizeof(Match)));
  return SIFT_OK;
}

int sift_device_matches(sift_ctx* ctx, const struct sift_match** d_match, size_t* n) {
  if (!ctx || !d_match || !n) return SIFT_E_ARG;
  if (!ctx->match.have) return set_err(ctx, SIFT_E_STATE, "no match: run sift_match or sift_match_features first");
  *d_match = ctx->match.out.as<const struct sift_match>();
  *n = ctx->match.n;
  return SIFT_OK;
}

int sift_match_select(sift_ctx* ctx, const struct sift_match* d_fwd, size_t n_query, const struct sift_match* d_rev,
                      size_t n_train, double ratio, sift_match_pair* d_pairs, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = select_check(ctx, d_fwd, n_query, n_train, ratio)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  return select_run(ctx, reinterpret_cast<const Match*>(d_fwd), n_query, reinterpret_cast<const Match*>(d_rev), n_train,
                    ratio, reinterpret_cast<MatchPair*>(d_pairs), cap, n_out);
}

// select_run over uploaded records, with the pairs through ctx->match.pairs into host memory.
int sift_match_select_host(sift_ctx* ctx, const struct sift_match* fwd, size_t n_query, const struct sift_match* rev,
                           size_t n_train, double ratio, sift_match_pair* pairs, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (int rc = select_check(ctx, fwd, n_query, n_train, ratio)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  MatchState& M = ctx->match;
  if (n_query) {
    if (int rc = h2d_buffer(ctx, M.fwd, fwd, n_query * sizeof(Match))) return rc;
    if (int rc = h2d_buffer(ctx, M.rev, rev, n_train * sizeof(Match))) return rc;
    if (pairs) HIPCHK(M.pairs.ensure(std::max<size_t>(std::min(cap, n_query), 1) * sizeof(MatchPair)));
  }
  size_t total = 0;
  if (!n_out) n_out = &total;
  if (int rc = select_run(ctx, M.fwd.as<Match>(), n_query, rev && n_train ? M.rev.as<Match>() : nullptr, n_train, ratio,
                          pairs ? M.pairs.as<MatchPair>() : nullptr, cap, n_out))
    return rc;
  if (pairs && *n_out) HIPCHK(d2h_staged(ctx, pairs, M.pairs.p, *n_out * sizeof(MatchPair)));
  return SIFT_OK;
}

int sift_last_match_timings(sift_ctx* ctx, double* match_ms, double* select_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (match_ms) *match_ms = ctx->match.match_ms;
  if (select_ms) *select_ms = ctx->match.select_ms;
  return SIFT_OK;
}
