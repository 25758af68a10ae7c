// C ABI of the extrema stage: scan -> ordered emission (row counts' scan, no sort) -> exact tie resolution.
// Leaves ctx->ext.cand_key / cand_val / n_cand.  Kernels: sift_extrema.hip.
#include "sift_ctx.h"

using namespace sift;

// Nearest fp32 at or below (dir < 0) / at or above (dir > 0) a double.
static float round_toward(double v, int dir) {
  float f = (float)v;
  if (dir < 0 && (double)f > v) f = std::nextafter(f, -INFINITY);
  if (dir > 0 && (double)f < v) f = std::nextafter(f, INFINITY);
  return f;
}

// The extrema stage, launched without waiting, in three parts:
//   extrema_prepare  capacities, buffers, counter resets (on stream st);
//   launch_extrema   bitmap scan of octaves [o0, O) (k_extrema);
//   extrema_finish   row-count scan, ordered emission into cand_cap slots,
//                    exact tie resolution (context stream).
// Counts stay on the device.
// Row / word geometry of the candidate bitmap: octaves < nf are decided in
// the Gaussian pass (kFX-column words, bit 0 = column 1), the rest by the
// scan (kXW-column words, bit 0 = column 0).
static BitmapGeom bitmap_geometry(const Pyramid& P, int nf) {
  BitmapGeom G{};
  G.n_oct = P.O;
  long long words = 0, rows = 0;
  for (int o = 0; o < P.O; ++o) {
    const bool f = o < nf;
    G.nw[o] = f ? fused_words_per_row(P.oct[o].w) : extrema_words_per_row(P.oct[o].w);
    G.ww[o] = f ? kFX : kXW;
    G.woff[o] = f ? 1 : 0;
    G.word_off[o] = words;
    G.row_off[o] = (int)rows;
    words += (long long)P.S * P.oct[o].h * G.nw[o];
    rows += (long long)P.S * P.oct[o].h;
  }
  G.row_off[P.O] = (int)rows;
  G.words_per_img = words;
  G.rows_per_img = (int)rows;
  return G;
}

// Rows of the bitmap over all images of the batch (image-major).
static long long bitmap_rows(const sift_ctx* ctx) {
  return (long long)ctx->ext.xl.G.rows_per_img * std::max(1, ctx->P.nimg);
}

int sift::extrema_prepare(sift_ctx* ctx, hipStream_t st, int nf) {
  Pyramid& P = ctx->P;
  ExtState& E = ctx->ext;
  const bool exact_planes = ctx->pyr.dog_source == kForeign;
  unsigned* cnt = ctx->counters.as<unsigned>();
  E.nf = nf;
  ExtremaLaunch& L = E.xl;
  L = ExtremaLaunch{};
  L.G = bitmap_geometry(P, nf);
  // A batch (P.nimg images) repeats the per-image words and rows image-major.
  const int ni = std::max(1, P.nimg);
  const long long words = L.G.words_per_img * ni, rows = bitmap_rows(ctx);
  {  // capacities: an estimate for this geometry, grown on overflow (settle_extrema)
    const long long est = std::min<long long>(
        std::max<long long>((long long)P.S * total_plane_px(ctx) * ni / 192, 65536), 0x7fffffffLL);
    E.cand_cap = std::max(E.cand_cap, (unsigned)est);
    E.amb_cap = std::max(E.amb_cap, 4096 + (unsigned)est / 16);
  }
  HIPCHK(E.bitmap.ensure((size_t)words * sizeof(unsigned long long)));
  HIPCHK(E.rowcount.ensure((size_t)(rows + 1) * sizeof(unsigned)));
  HIPCHK(E.rowoff.ensure((size_t)(rows + 1) * sizeof(unsigned)));
  HIPCHK(E.amb_keys.ensure((size_t)E.amb_cap * sizeof(unsigned)));
  HIPCHK(E.cand_key.ensure((size_t)E.cand_cap * sizeof(unsigned)));
  HIPCHK(E.cand_val.ensure((size_t)E.cand_cap * sizeof(double)));
  HIPCHK(E.cand_keep.ensure((size_t)E.cand_cap * sizeof(unsigned)));
  E.want_low = (ctx->p.flags & SIFT_F_LOW_CONTRAST_LIST) != 0;
  E.have_low = false;
  if (E.want_low) {
    E.low_cap = std::max(E.low_cap, std::max(65536u, E.cand_cap / 4));
    HIPCHK(E.lowbitmap.ensure((size_t)words * sizeof(unsigned long long)));
    HIPCHK(E.lowrowcount.ensure((size_t)(rows + 1) * sizeof(unsigned)));
    HIPCHK(E.lowrowoff.ensure((size_t)(rows + 1) * sizeof(unsigned)));
    HIPCHK(E.low_key.ensure((size_t)E.low_cap * sizeof(unsigned)));
    HIPCHK(E.low_val.ensure((size_t)E.low_cap * sizeof(double)));
    HIPCHK(E.late_key.ensure((size_t)E.amb_cap * sizeof(unsigned)));
    HIPCHK(E.late_val.ensure((size_t)E.amb_cap * sizeof(double)));
  }
  // fp32 contrast thresholds: rounding is monotone, so |v32| < c_lo proves
  // |v64| < pix_thr and |v32| >= c_hi proves |v64| >= pix_thr.
  const float t_dn = round_toward(P.pix_thr, -1), t_up = round_toward(P.pix_thr, +1);
  // extrema and refinement counters and the refinement's per-block counts: one fill
  // (+ the row counts, and the low-contrast row counts when listed): one launch
  HIPCHK(launch_zero_words(cnt, kCntAll, E.rowcount.as<unsigned>(), rows + 1,
                           E.want_low ? E.lowrowcount.as<unsigned>() : nullptr, rows + 1, st));
  E.counters_zeroed = true;
  L.exact_planes = exact_planes;
  L.c_lo = exact_planes ? t_up : t_dn;
  L.c_hi = exact_planes ? t_up : std::nextafter(t_up, INFINITY);
  L.bitmap = E.bitmap.as<unsigned long long>();
  L.rowcount = E.rowcount.as<unsigned>();
  L.amb_keys = E.amb_keys.as<unsigned>();
  L.counters = cnt;
  L.amb_cap = E.amb_cap;
  // Ambiguous pixels are re-decided a word (62 pixels) at a time
  // (k_exact_words; SIFT_XWORDS=0: one wave per pixel key, experiments) --
  // not with fused octave-0 decisions, which list keys.
  static const int xwords = exp_knob("SIFT_XWORDS", 1);
  E.words = xwords && nf == 0 && !exact_planes;
  if (E.words) {
    HIPCHK(E.ambbitmap.ensure((size_t)words * sizeof(unsigned long long)));
    L.ambbitmap = E.ambbitmap.as<unsigned long long>();
  }
  L.lowbitmap = E.want_low ? E.lowbitmap.as<unsigned long long>() : nullptr;
  L.lowrowcount = E.want_low ? E.lowrowcount.as<unsigned>() : nullptr;
  return SIFT_OK;
}

// One ordered list from a bitmap of this extrema stage's geometry: the row
// counts' exclusive scan into rowoff, then k_emit expands the rows' words in
// order into keys / value / keep (cap slots); *n_out = the list's length,
// written by k_emit (no 4-byte copy launch).
static int emit_list(sift_ctx* ctx, const unsigned long long* bitmap, unsigned* rowcount, unsigned* rowoff,
                     unsigned* keys, double* value, unsigned* keep, unsigned cap, unsigned* n_out, bool deferred) {
  const Pyramid& P = ctx->P;
  const long long rows = bitmap_rows(ctx);
  HIPCHK(exclusive_sum(ctx, rowcount, rowoff, (int)(rows + 1)));
  EmitLaunch E{};
  E.G = ctx->ext.xl.G;
  // rows of earlier octaves hold no decisions
  E.o_first = std::min(std::max(ctx->pyr.o_first, ctx->pyr.scan_first), P.O - 1);
  E.bitmap = bitmap;
  E.rowcount = rowcount;
  E.rowoff = rowoff;
  E.keys = keys;
  E.value = value;
  E.keep = keep;
  E.cap = cap;
  E.deferred = deferred;
  E.n_out = n_out;
  E.n_index = rows;
  HIPCHK(launch_emit(P, E, ctx->stream));
  return SIFT_OK;
}

static int extrema_finish(sift_ctx* ctx) {
  Pyramid& P = ctx->P;
  ExtState& E = ctx->ext;
  unsigned* cnt = ctx->counters.as<unsigned>();
  // Deferred values (SIFT_DEFER_VALUES=0: gathered here, experiments): the
  // refinement reads each candidate's plane value from the DoG plane, with
  // the 3x3x3 neighbourhood it gathers there anyway.
  static const int defer = exp_knob("SIFT_DEFER_VALUES", 1);
  int rc = emit_list(ctx, E.bitmap.as<unsigned long long>(), E.rowcount.as<unsigned>(), E.rowoff.as<unsigned>(),
                     E.cand_key.as<unsigned>(), E.cand_val.as<double>(), E.cand_keep.as<unsigned>(), E.cand_cap,
                     cnt + kCntN, defer != 0);
  if (rc) return rc;
  if (E.want_low) {  // the certain low-contrast extrema, in order (same scan + emission as the candidates)
    rc = emit_list(ctx, E.lowbitmap.as<unsigned long long>(), E.lowrowcount.as<unsigned>(),
                   E.lowrowoff.as<unsigned>(), E.low_key.as<unsigned>(), E.low_val.as<double>(), nullptr, E.low_cap,
                   cnt + kCntLowSure, false);
    if (rc) return rc;
  }
  ExactLaunch X{};
  X.late_keys = E.want_low ? E.late_key.as<unsigned>() : nullptr;
  X.late_vals = E.want_low ? E.late_val.as<double>() : nullptr;
  X.amb_keys = E.amb_keys.as<unsigned>();
  X.amb_cap = E.amb_cap;
  X.keys = E.cand_key.as<unsigned>();
  X.n = cnt + kCntN;
  X.cap = E.cand_cap;
  X.keep = E.cand_keep.as<unsigned>();
  X.value = E.cand_val.as<double>();
  X.counters = cnt;
  X.G = E.xl.G;
  // List positions from the emission geometry (SIFT_XPOS=0: a binary search
  // over the keys, experiments; the word pass always takes the geometry).
  static const int xpos = exp_knob("SIFT_XPOS", 1);
  if (xpos || E.words) {
    X.bitmap = E.bitmap.as<unsigned long long>();
    X.rowoff = E.rowoff.as<unsigned>();
  }
  if (E.words) {
    X.ambbitmap = E.ambbitmap.as<unsigned long long>();
    HIPCHK(launch_exact_words(P, X, ctx->stream));
  } else {
    HIPCHK(launch_exact_extrema(P, X, ctx->stream));
  }
  HIPCHK(hipEventRecord(ctx->ev[kEvExtEnd], ctx->stream));
  E.slot_cap = (int)E.cand_cap;
  E.has_keep = true;
  E.slots_rows = true;
  E.pending = true;
  return SIFT_OK;
}

// The whole extrema stage on the context stream.
int sift::launch_extrema_stage(sift_ctx* ctx) {
  HIPCHK(hipEventRecord(ctx->ev[kEvExt], ctx->stream));
  int o0 = std::max(ctx->pyr.o_first, ctx->pyr.scan_first);
  if (ctx->ext.prepared) {  // octaves < nf were decided in the Gaussian pass
    ctx->ext.prepared = false;
    o0 = std::max(o0, ctx->ext.nf);
  } else {
    const int rc = extrema_prepare(ctx, ctx->stream, 0);
    if (rc) return rc;
  }
  HIPCHK(launch_extrema(ctx->P, ctx->ext.xl, ctx->stream, o0, ctx->P.O));
  return extrema_finish(ctx);
}

// Reads the extrema counts (ctx->h_counters must hold the device counters):
// kRetry after growing the capacities when one overflowed.
int sift::settle_extrema(sift_ctx* ctx) {
  const unsigned* h = ctx->h_counters.as<unsigned>();
  ExtState& E = ctx->ext;
  E.pending = false;
  const unsigned n = h[kCntN], n_amb = h[kCntAmb];
  const unsigned n_ls = E.want_low ? h[kCntLowSure] : 0u;
  if (n > E.cand_cap || n_amb > E.amb_cap || n_ls > E.low_cap || h[kAmbWords] > E.amb_cap) {
    if (n > E.cand_cap) E.cand_cap = n + n / 4 + 1024;
    if (n_amb > E.amb_cap) E.amb_cap = n_amb + n_amb / 4 + 1024;
    if (n_ls > E.low_cap) E.low_cap = n_ls + n_ls / 4 + 1024;
    return kRetry;
  }
  E.have_low = E.want_low;
  E.n_low_sure = n_ls;
  E.n_low_late = E.want_low ? h[kCntLowLate] : 0u;
  E.n_exact = n_amb;
  E.n_low = h[kCntLow];
  E.n_slots = n;
  E.n_cand = n - h[kCntDrop];
  E.have_cand = true;
  return SIFT_OK;
}

static int run_extrema(sift_ctx* ctx) {
  for (;;) {
    int rc = launch_extrema_stage(ctx);
    if (rc) return rc;
    // the extrema and refinement counts: every slot below the debug block
    HIPCHK(hipMemcpyAsync(ctx->h_counters.p, ctx->counters.p, kCntDbg * sizeof(unsigned), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    rc = settle_extrema(ctx);
    if (rc != kRetry) return rc;
  }
}

int sift_copy_candidates(sift_ctx* ctx, sift_extremum* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  ExtState& E = ctx->ext;
  if (ctx->P.nimg > 1) return set_err(ctx, SIFT_E_UNSUPPORTED, "a batch detection returns keypoints only");
  if (!E.have_cand) return set_err(ctx, SIFT_E_STATE, "no candidates");
  if (n_out) *n_out = E.n_cand;
  if (!out) return SIFT_OK;
  if (cap < E.n_cand) return set_err(ctx, SIFT_E_CAPACITY, "candidate buffer too small");
  const size_t n = E.n_slots;
  std::vector<unsigned> keys(n), keep(n, 1u);
  std::vector<double> vals(n);
  if (n) {
    HIPCHK(hipSetDevice(ctx->device));
    if (E.slots_rows)  // deferred candidate values (EmitLaunch.deferred) from the DoG planes
      HIPCHK(launch_fill_values(ctx->P, E.cand_key.as<unsigned>(), E.cand_val.as<double>(),
                                ctx->counters.as<unsigned>() + kCntN, (int)n, ctx->stream));
    HIPCHK(hipMemcpyAsync(keys.data(), E.cand_key.p, n * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(vals.data(), E.cand_val.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (E.has_keep)
      HIPCHK(hipMemcpyAsync(keep.data(), E.cand_keep.p, n * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  const Pyramid& P = ctx->P;
  size_t j = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    int b;
    decode_key(P, keys[i], b, out[j].octave, out[j].scale, out[j].y, out[j].x);
    out[j].value = vals[i];
    ++j;
  }
  if (n_out) *n_out = j;
  return SIFT_OK;
}

int sift_copy_low_contrast(sift_ctx* ctx, sift_extremum* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  ExtState& E = ctx->ext;
  if (!E.have_low) return set_err(ctx, SIFT_E_STATE, "no low-contrast list (SIFT_F_LOW_CONTRAST_LIST)");
  const size_t ns = E.n_low_sure, nl = E.n_low_late, n = ns + nl;
  if (n_out) *n_out = n;
  if (!out) return SIFT_OK;
  if (cap < n) return set_err(ctx, SIFT_E_CAPACITY, "low-contrast buffer too small");
  std::vector<unsigned> k(n);
  std::vector<double> v(n);
  if (n) {
    HIPCHK(hipSetDevice(ctx->device));
    if (ns) {
      HIPCHK(hipMemcpyAsync(k.data(), E.low_key.p, ns * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(v.data(), E.low_val.p, ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (nl) {
      HIPCHK(hipMemcpyAsync(k.data() + ns, E.late_key.p, nl * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(v.data() + ns, E.late_val.p, nl * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  // The late entries (exact-pass decisions, unordered) merge into the ordered list by key.
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; ++i) idx[i] = i;
  std::sort(idx.begin() + ns, idx.end(), [&](size_t a, size_t b) { return k[a] < k[b]; });
  std::inplace_merge(idx.begin(), idx.begin() + ns, idx.end(), [&](size_t a, size_t b) { return k[a] < k[b]; });
  const Pyramid& P = ctx->P;
  for (size_t j = 0; j < n; ++j) {
    int b;
    decode_key(P, k[idx[j]], b, out[j].octave, out[j].scale, out[j].y, out[j].x);
    out[j].value = v[idx[j]];
  }
  return SIFT_OK;
}

int sift_find_extrema(sift_ctx* ctx, sift_extremum* out, size_t cap, size_t* n_out, size_t* n_low) {
  if (!ctx) return SIFT_E_ARG;
  if (ctx->pyr.dog_source == kNone) return set_err(ctx, SIFT_E_STATE, "no DoG pyramid: build or load one first");
  HIPCHK(hipSetDevice(ctx->device));
  int rc = run_extrema(ctx);
  if (rc) return rc;
  HIPCHK(hipEventRecord(ctx->ev[kEvRefEnd], ctx->stream));
  read_stage_times(ctx, true, false);
  if (n_low) *n_low = ctx->ext.n_low;
  return sift_copy_candidates(ctx, out, cap, n_out);
}

int sift_set_candidates(sift_ctx* ctx, const sift_extremum* cand, size_t n) {
  if (!ctx || (!cand && n)) return SIFT_E_ARG;
  if (ctx->pyr.dog_source == kNone) return set_err(ctx, SIFT_E_STATE, "no DoG pyramid");
  const Pyramid& P = ctx->P;
  ExtState& E = ctx->ext;
  std::vector<unsigned> keys(n);
  std::vector<double> vals(n);
  for (size_t i = 0; i < n; ++i) {
    const sift_extremum& c = cand[i];
    if (c.octave < 0 || c.octave >= P.O) return set_err(ctx, SIFT_E_ARG, "candidate octave out of range");
    const Octave& oc = P.oct[c.octave];
    if (c.scale < 1 || c.scale > P.S || c.y < 1 || c.y > oc.h - 2 || c.x < 1 || c.x > oc.w - 2)
      return set_err(ctx, SIFT_E_ARG, "candidate outside the refinable interior");
    keys[i] = oc.key_off + (unsigned)(c.scale - 1) * (unsigned)oc.h * (unsigned)oc.w + (unsigned)c.y * oc.w + c.x;
    vals[i] = c.value;
  }
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(E.cand_key.ensure(std::max<size_t>(n, 1) * sizeof(unsigned)));
  HIPCHK(E.cand_val.ensure(std::max<size_t>(n, 1) * sizeof(double)));
  if (int rc = h2d_buffer(ctx, E.cand_key, keys.data(), n * sizeof(unsigned))) return rc;
  if (int rc = h2d_buffer(ctx, E.cand_val, vals.data(), n * sizeof(double))) return rc;
  const unsigned n32 = (unsigned)n;
  HIPCHK(hipMemcpyAsync(ctx->counters.as<unsigned>() + kCntN, &n32, sizeof(unsigned), hipMemcpyHostToDevice,
                        ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  E.n_cand = n;
  E.n_slots = n;
  E.slot_cap = (int)n;
  E.pending = false;
  E.has_keep = false;
  E.slots_rows = false;
  E.have_cand = true;
  return SIFT_OK;
}
