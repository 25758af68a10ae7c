// C ABI of what a sharded detection needs of one context: owned rows and the row origin of a band, keypoint
// origins, the exported base of the next octave, per-block keypoint counts and the merge of the parts' keypoint blocks.
#include "sift_ctx.h"

using namespace sift;

int sift_set_owned_rows(sift_ctx* ctx, int row_begin, int row_end) {
  if (!ctx) return SIFT_E_ARG;
  if (row_begin < 0) {
    ctx->shard.own_lo = ctx->shard.own_hi = -1;
    return SIFT_OK;
  }
  if (row_end >= 0 && row_end < row_begin) return set_err(ctx, SIFT_E_ARG, "row_end < row_begin");
  ctx->shard.own_lo = row_begin;
  ctx->shard.own_hi = row_end;
  return SIFT_OK;
}

int sift_set_row_origin(sift_ctx* ctx, int input_row0) {
  if (!ctx || input_row0 < 0) return SIFT_E_ARG;
  ctx->shard.row0 = input_row0;
  return SIFT_OK;
}

int sift_last_block_counts(sift_ctx* ctx, int64_t* counts, int cap, int* n_blocks) {
  if (!ctx) return SIFT_E_ARG;
  const int n = (int)ctx->ref.blk_counts.size();
  if (n_blocks) *n_blocks = n;
  if (!counts) return SIFT_OK;
  if (cap < n) return set_err(ctx, SIFT_E_CAPACITY, "destination too small (num_octaves * scales_per_octave)");
  for (int b = 0; b < n; ++b) counts[b] = ctx->ref.blk_counts[b];
  return SIFT_OK;
}

int sift_device_next_seed(sift_ctx* ctx, const double** d_seed, int* rows, int* cols) {
  if (!ctx || !d_seed) return SIFT_E_ARG;
  const ShardState& S = ctx->shard;
  if (!S.has_xseed) return set_err(ctx, SIFT_E_STATE, "no next-octave base (SIFT_F_EXPORT_NEXT_SEED)");
  *d_seed = S.xseed.as<const double>();
  if (rows) *rows = S.xseed_h;
  if (cols) *cols = S.xseed_w;
  return SIFT_OK;
}

int sift_next_seed(sift_ctx* ctx, double* dst, size_t cap, int* rows, int* cols) {
  if (!ctx) return SIFT_E_ARG;
  const ShardState& S = ctx->shard;
  if (!S.has_xseed) return set_err(ctx, SIFT_E_STATE, "no next-octave base (SIFT_F_EXPORT_NEXT_SEED)");
  if (rows) *rows = S.xseed_h;
  if (cols) *cols = S.xseed_w;
  if (!dst) return SIFT_OK;
  const size_t n = (size_t)S.xseed_h * S.xseed_w;
  if (cap < n) return set_err(ctx, SIFT_E_CAPACITY, "destination too small");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(dst, S.xseed.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_copy_next_seed_device(sift_ctx* ctx, double* d_dst, size_t cap, int row_begin, int row_end) {
  if (!ctx) return SIFT_E_ARG;
  const ShardState& S = ctx->shard;
  if (!S.has_xseed) return set_err(ctx, SIFT_E_STATE, "no next-octave base (SIFT_F_EXPORT_NEXT_SEED)");
  if (row_begin < 0 || row_end > S.xseed_h || row_begin > row_end) return set_err(ctx, SIFT_E_ARG, "bad row range");
  const size_t n = (size_t)(row_end - row_begin) * S.xseed_w;
  if (!d_dst || n == 0) return SIFT_OK;
  if (cap < n) return set_err(ctx, SIFT_E_CAPACITY, "destination too small");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(d_dst, S.xseed.as<double>() + (size_t)row_begin * S.xseed_w, n * sizeof(double),
                        hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_copy_keypoint_origins_device(sift_ctx* ctx, int32_t* d_dst, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (!ctx->shard.has_origins) return set_err(ctx, SIFT_E_STATE, "no keypoint origins (SIFT_F_KEYPOINT_ORIGINS)");
  if (n_out) *n_out = ctx->n_kp;
  if (!d_dst || ctx->n_kp == 0) return SIFT_OK;
  if (cap < 4 * ctx->n_kp) return set_err(ctx, SIFT_E_CAPACITY, "destination too small (4 per keypoint)");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(launch_decode_origins(ctx->P, ctx->shard.kp_key.as<unsigned>(), (int)ctx->n_kp, d_dst, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_keypoint_origins(sift_ctx* ctx, int32_t* out, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (!ctx->shard.has_origins) return set_err(ctx, SIFT_E_STATE, "no keypoint origins (SIFT_F_KEYPOINT_ORIGINS)");
  if (n_out) *n_out = ctx->n_kp;
  if (!out || ctx->n_kp == 0) return SIFT_OK;
  if (cap < 4 * ctx->n_kp) return set_err(ctx, SIFT_E_CAPACITY, "destination too small (4 per keypoint)");
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<unsigned> keys(ctx->n_kp);
  HIPCHK(hipMemcpyAsync(keys.data(), ctx->shard.kp_key.p, keys.size() * sizeof(unsigned), hipMemcpyDeviceToHost,
                        ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const Pyramid& P = ctx->P;
  for (size_t i = 0; i < keys.size(); ++i) {
    int b, o, s, y, x;
    decode_key(P, keys[i], b, o, s, y, x);
    out[4 * i + 0] = o;
    out[4 * i + 1] = s;
    out[4 * i + 2] = y + ((P.row0 * 2) >> o);  // whole-image octave row
    out[4 * i + 3] = x;
  }
  return SIFT_OK;
}

int sift_merge_keypoint_blocks_device(sift_ctx* ctx, const sift_keypoint* d_in, const int64_t* counts, int n_parts,
                                      int n_blocks, sift_keypoint* d_out) {
  if (!ctx || !counts || n_parts < 1 || n_blocks < 1 || n_parts > 1024 || n_blocks > 4096) return SIFT_E_ARG;
  // Every (part, block) run is contiguous in d_in and in d_out: the merge is
  // one copy per non-empty run (seg = src, dst, bytes; cstart = first chunk).
  const int np = n_parts, nb = n_blocks;
  constexpr long long kRec = sizeof(sift_keypoint), kChunk = kMergeChunk;
  std::vector<long long> part_start((size_t)np + 1, 0);
  for (int q = 0; q < np; ++q) {
    long long a = 0;
    for (int b = 0; b < nb; ++b) {
      const long long c = counts[(size_t)q * nb + b];
      a += c < 0 ? -c : c;  // negative: skipped records (padding)
    }
    part_start[q + 1] = part_start[q] + a;
  }
  std::vector<long long> in_at(part_start.begin(), part_start.end() - 1);  // next record of each part
  std::vector<long long> seg, cstart;
  long long o = 0, chunks = 0;
  for (int b = 0; b < nb; ++b)
    for (int q = 0; q < np; ++q) {
      const long long c = counts[(size_t)q * nb + b];
      if (c <= 0) {
        in_at[q] -= c;
        continue;
      }
      seg.push_back(in_at[q] * kRec);
      seg.push_back(o * kRec);
      seg.push_back(c * kRec);
      cstart.push_back(chunks);
      chunks += (c * kRec + kChunk - 1) / kChunk;
      in_at[q] += c;
      o += c;
    }
  if (o == 0) return SIFT_OK;
  if (!d_in || !d_out) return SIFT_E_ARG;
  const int nseg = (int)cstart.size();
  std::vector<long long> tab(seg);
  tab.insert(tab.end(), cstart.begin(), cstart.end());
  DBuf& dtab = ctx->shard.merge_tab;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(dtab.ensure(tab.size() * sizeof(long long)));
  // through the context's pinned staging (an asynchronous DMA; a pageable
  // source is copied through the runtime's own staging first)
  HIPCHK(ctx->hpl.ensure(tab.size() * sizeof(long long)));
  std::memcpy(ctx->hpl.p, tab.data(), tab.size() * sizeof(long long));
  HIPCHK(hipMemcpyAsync(dtab.p, ctx->hpl.p, tab.size() * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(launch_merge_blocks(reinterpret_cast<const Keypoint*>(d_in), dtab.as<long long>(),
                             dtab.as<long long>() + 3 * (size_t)nseg, nseg, chunks,
                             reinterpret_cast<Keypoint*>(d_out), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}
