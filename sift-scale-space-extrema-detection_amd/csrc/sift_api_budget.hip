// C ABI of the keypoint budget: the N strongest keypoints, overall or per grid cell (kernels: sift_budget.hip).
#include "sift_ctx.h"

using namespace sift;

static_assert(sizeof(sift_budget) == 16, "16-byte budget");
static_assert(sizeof(sift_keypoint) == sizeof(Keypoint), "keypoint records");
static_assert(kBudgetMaxCells == SIFT_BUDGET_MAX_CELLS, "budget constants of include/sift_hip.h");

namespace {

struct BudgetGrid {
  int ncx = 0, ncy = 0, cells = 0;  // all 0 without a grid
};

// The limits of include/sift_hip.h; nothing has been written when this fails.
int budget_check(sift_ctx* ctx, const void* kp, size_t n, int width, int height, const sift_budget* b, BudgetGrid* g) {
  if (!b) return set_err(ctx, SIFT_E_ARG, "null budget");
  if (!count_ok(n)) return set_err(ctx, SIFT_E_ARG, "too many keypoints");
  if (n && !kp) return set_err(ctx, SIFT_E_ARG, "null keypoint records");
  if (b->reserved != 0) return set_err(ctx, SIFT_E_ARG, "budget.reserved must be 0");
  if (b->cell_px < 0) return set_err(ctx, SIFT_E_ARG, "budget.cell_px must not be negative");
  if (b->cell_px > 0) {
    if (width <= 0 || height <= 0) return set_err(ctx, SIFT_E_ARG, "a grid needs a width and a height");
    const long long ncx = ((long long)width + b->cell_px - 1) / b->cell_px;
    const long long ncy = ((long long)height + b->cell_px - 1) / b->cell_px;
    if (ncx * ncy > kBudgetMaxCells) return set_err(ctx, SIFT_E_UNSUPPORTED, "more than SIFT_BUDGET_MAX_CELLS cells");
    g->ncx = (int)ncx;
    g->ncy = (int)ncy;
    g->cells = (int)(ncx * ncy);
  }
  return SIFT_OK;
}

// The selection over validated device records, timed and complete on return: *total = the kept count always;
// the ascending indices into d_index and the gathered records into kp_out, each when given and cap holds them.
int budget_run(sift_ctx* ctx, const Keypoint* d_kp, size_t n_rec, const sift_budget& b, const BudgetGrid& g,
               int32_t* d_index, Keypoint* kp_out, size_t cap, size_t* total_out) {
  BudgetState& B = ctx->budget;
  B.select_ms = 0;
  *total_out = 0;
  if (!n_rec) return SIFT_OK;
  const int n = (int)n_rec;
  const bool per_cell = b.cell_px > 0 && b.max_per_cell >= 0, overall = b.max_total >= 0;
  const int cells = per_cell ? g.cells : 1;
  HIPCHK(B.ev.ensure());
  HIPCHK(B.flag.ensure((size_t)(n + 1) * sizeof(unsigned)));
  HIPCHK(B.off.ensure((size_t)(n + 1) * sizeof(unsigned)));
  if (per_cell || overall) {
    HIPCHK(B.key.ensure((size_t)n * sizeof(unsigned long long)));
    HIPCHK(B.tkey.ensure((size_t)cells * sizeof(unsigned long long)));
    HIPCHK(B.ttail.ensure((size_t)cells * sizeof(unsigned)));
    HIPCHK(B.rem.ensure((size_t)cells * sizeof(unsigned)));
    HIPCHK(B.hist.ensure((size_t)cells * 256 * sizeof(unsigned)));
  }
  if (per_cell) HIPCHK(B.cell.ensure((size_t)n * sizeof(unsigned)));
  if (per_cell && overall) HIPCHK(B.surv.ensure((size_t)(n + 1) * sizeof(unsigned)));
  unsigned* flag = B.flag.as<unsigned>();
  HIPCHK(hipEventRecord(B.ev[0], ctx->stream));
  if (per_cell || overall) {
    unsigned long long* key = B.key.as<unsigned long long>();
    unsigned* surv = per_cell && overall ? B.surv.as<unsigned>() : nullptr;
    HIPCHK(launch_budget_keys(d_kp, n, per_cell ? b.cell_px : 0, g.ncx, g.ncy, key, B.cell.as<unsigned>(),
                              ctx->stream));
    HIPCHK(hipMemsetAsync(B.hist.p, 0, (size_t)cells * 256 * sizeof(unsigned), ctx->stream));
    if (per_cell)
      HIPCHK(launch_budget_select(key, B.cell.as<unsigned>(), nullptr, n, cells, (unsigned)b.max_per_cell,
                                  B.tkey.as<unsigned long long>(), B.ttail.as<unsigned>(), B.rem.as<unsigned>(),
                                  B.hist.as<unsigned>(), surv ? surv : flag, ctx->stream));
    if (overall)  // one cell over the survivors
      HIPCHK(launch_budget_select(key, nullptr, surv, n, 1, (unsigned)b.max_total, B.tkey.as<unsigned long long>(),
                                  B.ttail.as<unsigned>(), B.rem.as<unsigned>(), B.hist.as<unsigned>(), flag,
                                  ctx->stream));
  } else {
    HIPCHK(launch_budget_fill(flag, n, ctx->stream));
  }
  unsigned total = 0;
  if (int rc = ordered_total(ctx, flag, B.off.as<unsigned>(), n, &total)) return rc;
  *total_out = total;
  const bool fits = cap >= total;
  if (fits) HIPCHK(launch_budget_emit(flag, B.off.as<unsigned>(), n, total, d_index, d_kp, kp_out, ctx->stream));
  HIPCHK(hipEventRecord(B.ev[1], ctx->stream));
  HIPCHK(hipEventSynchronize(B.ev[1]));
  B.select_ms = event_ms(B.ev[0], B.ev[1]);
  if ((d_index || kp_out) && !fits) return set_err(ctx, SIFT_E_CAPACITY, "index buffer too small");
  return SIFT_OK;
}

void swap_buffers(DBuf& a, DBuf& b) {
  std::swap(a.p, b.p);
  std::swap(a.bytes, b.bytes);
}

}  // namespace

int sift_keypoint_select_device(sift_ctx* ctx, const sift_keypoint* d_kp, size_t n, int width, int height,
                                const sift_budget* budget, int32_t* d_index, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  BudgetGrid g;
  if (int rc = budget_check(ctx, d_kp, n, width, height, budget, &g)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  size_t total = 0;
  const int rc = budget_run(ctx, reinterpret_cast<const Keypoint*>(d_kp), n, *budget, g, d_index, nullptr, cap, &total);
  if (n_out && (rc == SIFT_OK || rc == SIFT_E_CAPACITY)) *n_out = total;
  return rc;
}

// budget_run over uploaded records, with the indices through ctx->budget.idx into host memory.
int sift_keypoint_select(sift_ctx* ctx, const sift_keypoint* kp, size_t n, int width, int height,
                         const sift_budget* budget, int32_t* index, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  BudgetGrid g;
  if (int rc = budget_check(ctx, kp, n, width, height, budget, &g)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  BudgetState& B = ctx->budget;
  if (int rc = h2d_buffer(ctx, B.in_kp, kp, n * sizeof(Keypoint))) return rc;
  if (index && n) HIPCHK(B.idx.ensure(std::max<size_t>(std::min(cap, n), 1) * sizeof(int32_t)));
  size_t total = 0;
  const int rc = budget_run(ctx, B.in_kp.as<Keypoint>(), n, *budget, g, index && n ? B.idx.as<int32_t>() : nullptr,
                            nullptr, cap, &total);
  if (n_out && (rc == SIFT_OK || rc == SIFT_E_CAPACITY)) *n_out = total;
  if (rc) return rc;
  if (index && total) HIPCHK(d2h_staged(ctx, index, B.idx.p, total * sizeof(int32_t)));
  return SIFT_OK;
}

int sift_limit_keypoints(sift_ctx* ctx, const sift_budget* budget, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  if (!stage_has(ctx, kNeedKp)) return set_err(ctx, SIFT_E_STATE, "no refinement: run sift_refine or a detection first");
  if (ctx->P.nimg > 1) return set_err(ctx, SIFT_E_UNSUPPORTED, "a budget for a batch");
  if (ctx->shard.row0 != 0 || ctx->shard.own_lo >= 0)
    return set_err(ctx, SIFT_E_UNSUPPORTED, "a budget with a row origin or owned rows");
  BudgetGrid g;
  const size_t n = ctx->n_kp;
  if (int rc = budget_check(ctx, ctx->kp.p, n, ctx->P.W, ctx->P.H, budget, &g)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  BudgetState& B = ctx->budget;
  HIPCHK(B.kp2.ensure(std::max<size_t>(n, 1) * sizeof(Keypoint)));
  HIPCHK(B.sel.ensure(std::max<size_t>(n, 1) * sizeof(int32_t)));
  B.have_sel = false;
  size_t total = 0;
  if (int rc = budget_run(ctx, ctx->kp.as<Keypoint>(), n, *budget, g, B.sel.as<int32_t>(), B.kp2.as<Keypoint>(), n,
                          &total))
    return rc;
  swap_buffers(ctx->kp, B.kp2);
  ctx->n_kp = total;
  B.n_sel = total;
  B.have_sel = true;
  // the new list has no orientations, descriptors, blocks or origins; the singular count and refine_ms remain true
  // of the detection behind it
  FeatState& F = ctx->feat;
  F.have_ori = F.have_desc = false;
  F.n_ori = F.n_desc_ok = 0;
  F.orient_ms = F.describe_ms = 0;
  ctx->shard.has_origins = false;
  ctx->ref.blk_counts.clear();
  if (n_out) *n_out = total;
  return SIFT_OK;
}

int sift_copy_keypoint_selection(sift_ctx* ctx, int32_t* index, size_t cap, size_t* n_out) {
  if (!ctx) return SIFT_E_ARG;
  const BudgetState& B = ctx->budget;
  if (!stage_has(ctx, kNeedKp) || !B.have_sel)
    return set_err(ctx, SIFT_E_STATE, "no selection: the list is not that of a sift_limit_keypoints");
  if (n_out) *n_out = B.n_sel;
  if (!index) return SIFT_OK;
  if (cap < B.n_sel) return set_err(ctx, SIFT_E_CAPACITY, "index buffer too small");
  HIPCHK(hipSetDevice(ctx->device));
  if (B.n_sel) HIPCHK(d2h_staged(ctx, index, B.sel.p, B.n_sel * sizeof(int32_t)));
  return SIFT_OK;
}

int sift_last_select_timing(sift_ctx* ctx, double* select_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (select_ms) *select_ms = ctx->budget.select_ms;
  return SIFT_OK;
}
