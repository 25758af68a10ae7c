// C ABI of libsift_hip.so (include/sift_hip.h): context lifetime, host registration, parameters and schedule, the
// helpers every stage shares (sift_ctx.h) and the last run's counts and timings.  The stages, all on one HIP stream,
// mirror the reference's worker stages (background.js:71 / :258 / :359 / :455): sift_api_pyramid / _extrema / _detect
// / _shard / _image.hip (detection) and sift_api_feature / _match / _verify / _refit.hip, over the helpers here.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <map>
#include <mutex>
#include <atomic>

#include "sift_ctx.h"

using namespace sift;

// Threads of a host copy of rows x width bytes: one below 4 MiB.
static int copy_threads(size_t rows, size_t width, int nt) { return rows * width < ((size_t)4 << 20) ? 1 : nt; }

// Row copy between host buffers on up to `nt` threads (host memory bandwidth
// of one core is well below what the DMA engines take from pinned memory).
static void par_copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows,
                          int nt) {
  par_for(rows, copy_threads(rows, width, nt), [&](size_t r0, size_t r1) {
    for (size_t r = r0; r < r1; ++r)
      std::memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
  });
}

// Host rows -> pinned staging -> device, pipelined: each of nt host threads
// copies its share of the rows in ~2 MiB pieces and queues each piece's DMA on
// `st` as soon as it is staged (disjoint ranges: their order does not matter;
// the caller's later launches on `st` follow every piece).
hipError_t sift::h2d_rows_staged(void* dev, void* stage, const void* src, size_t spitch, size_t width, size_t rows,
                                 int nt, hipStream_t st) {
  std::atomic<int> err{0};
  par_for(rows, copy_threads(rows, width, nt), [&](size_t r0, size_t r1) {
    const size_t piece = std::max<size_t>(1, ((size_t)2 << 20) / width);
    for (size_t a = r0; a < r1; a += piece) {
      const size_t b = std::min(r1, a + piece);
      for (size_t r = a; r < b; ++r) std::memcpy((char*)stage + r * width, (const char*)src + r * spitch, width);
      if (hipMemcpyAsync((char*)dev + a * width, (const char*)stage + a * width, (b - a) * width,
                         hipMemcpyHostToDevice, st) != hipSuccess)
        err = 1;
    }
  });
  return err ? hipErrorUnknown : hipSuccess;
}

// Host threads of the library's own copies (image staging, keypoint split,
// plane read-back): min(4, cores); SIFT_HOST_THREADS=n in experiments builds
// (1, 2 and 4 measured under the N-API pool: 4 is best).
int sift::host_threads() {
  static const int n = [] {
    const int v = exp_knob("SIFT_HOST_THREADS", 0);
    if (v >= 1 && v <= 64) return v;
    const unsigned h = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(4u, h ? h : 1u));
  }();
  return n;
}

int sift::check_params(const sift_params* p) {
  if (!p) return SIFT_E_ARG;
  if (p->num_octaves < 1 || p->num_octaves > kMaxOctaves) return SIFT_E_UNSUPPORTED;
  if (p->scales_per_octave < 1 || p->scales_per_octave + 3 > kMaxScales) return SIFT_E_UNSUPPORTED;
  if (!(p->min_blur > 0) || !(p->assumed_blur >= 0) || !(p->min_interpixel_distance > 0)) return SIFT_E_ARG;
  return SIFT_OK;
}

// Host ranges page-locked through sift_host_register: the runtime DMAs into
// them directly; anything else is treated as pageable.  Tracked here rather
// than probed with hipPointerGetAttributes, whose failure on pageable memory
// would have to be cleared with hipGetLastError -- and that would also
// swallow an earlier asynchronous error still pending on the thread.
static std::mutex g_reg_mu;
static std::map<uintptr_t, size_t> g_reg_ranges;  // start -> bytes

bool sift::host_registered(const void* p, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg_ranges.upper_bound(a);
  if (it == g_reg_ranges.begin()) return false;
  --it;
  return a >= it->first && a + bytes <= it->first + it->second;
}

// Device -> pageable host copy through pinned staging: chunks alternate
// between the two halves of ctx->hpl, so the DMA of chunk i+1 overlaps the
// (multi-threaded) host copy of chunk i.  A plain hipMemcpy into pageable
// memory runs at a fraction of the link rate; this keeps the link busy.
hipError_t sift::d2h_staged(sift_ctx* ctx, void* dst, const void* src, size_t bytes) {
  constexpr size_t kChunk = (size_t)8 << 20;
  if (bytes < ((size_t)1 << 20) || host_registered(dst, bytes)) {  // small or page-locked: one DMA straight into it
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
  }
  hipError_t e = ctx->hpl.ensure(2 * kChunk);
  if (e == hipSuccess) e = ctx->ev_pl.ensure();
  if (e != hipSuccess) return e;
  char* half[2] = {(char*)ctx->hpl.p, (char*)ctx->hpl.p + kChunk};
  const size_t n = (bytes + kChunk - 1) / kChunk;
  auto len = [&](size_t i) { return std::min(kChunk, bytes - i * kChunk); };
  auto issue = [&](size_t i) {
    hipError_t r = hipMemcpyAsync(half[i & 1], (const char*)src + i * kChunk, len(i), hipMemcpyDeviceToHost,
                                  ctx->stream);
    return r != hipSuccess ? r : hipEventRecord(ctx->ev_pl[i & 1], ctx->stream);
  };
  for (size_t i = 0; i < std::min<size_t>(n, 2) && e == hipSuccess; ++i) e = issue(i);
  for (size_t i = 0; i < n && e == hipSuccess; ++i) {
    e = hipEventSynchronize(ctx->ev_pl[i & 1]);
    if (e != hipSuccess) break;
    const size_t piece = 256 << 10, l = len(i), rows = l / piece;  // 256 KB rows split over the threads
    par_copy_rows((char*)dst + i * kChunk, piece, half[i & 1], piece, piece, rows, host_threads());
    if (l > rows * piece) std::memcpy((char*)dst + i * kChunk + rows * piece, half[i & 1] + rows * piece, l - rows * piece);
    if (i + 2 < n) e = issue(i + 2);
  }
  if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);  // nothing left writing into hpl
  return e;
}

// out = the exclusive prefix sums of in[0 .. n), on the context stream (scratch: ctx->temp).
hipError_t sift::exclusive_sum(sift_ctx* ctx, unsigned* in, unsigned* out, int n) {
  size_t tb = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, n, ctx->stream);
  if (e == hipSuccess) e = ctx->temp.ensure(tb);
  if (e != hipSuccess) return e;
  tb = ctx->temp.bytes;
  return hipcub::DeviceScan::ExclusiveSum(ctx->temp.p, tb, in, out, n, ctx->stream);
}

bool sift::count_ok(size_t n) { return n < (size_t)0x7fffffff; }  // a scan over n + 1 items fits an int

// Milliseconds between two completed events, 0 when the query fails.
double sift::event_ms(hipEvent_t a, hipEvent_t b) {
  double ms = 0;
  take_event_ms(&ms, a, b);
  return ms;
}

// ... into *ms, which keeps its value when the query fails (what the sift_last_* timings then report).
void sift::take_event_ms(double* ms, hipEvent_t a, hipEvent_t b) {
  float t = 0;
  if (hipEventElapsedTime(&t, a, b) == hipSuccess) *ms = t;
}

// Host bytes into a context buffer, queued on the stream (nothing for bytes == 0 or src == nullptr).
int sift::h2d_buffer(sift_ctx* ctx, DBuf& b, const void* src, size_t bytes) {
  if (!src || !bytes) return SIFT_OK;
  HIPCHK(b.ensure(bytes));
  HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SIFT_OK;
}

// The count half of an ordered, sort-free selection: offsets = the exclusive scan of counts[0 .. n] (counts[n] is a
// zero), and *total = offsets[n] read back through the pinned word, which sizes the output of the emit kernel that
// follows; the stream is idle on return.  counts == nullptr: the read-back of offsets[n] alone.
int sift::ordered_total(sift_ctx* ctx, unsigned* counts, unsigned* offsets, int n, unsigned* total) {
  unsigned* h = &static_cast<StageScratch*>(ctx->hscratch.p)->word;
  if (counts) HIPCHK(exclusive_sum(ctx, counts, offsets, n + 1));
  HIPCHK(hipMemcpyAsync(h, offsets + n, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *total = *h;
  return SIFT_OK;
}

// No detection is in flight and the context holds a keypoint list [, its orientation records [, their descriptors]].
bool sift::stage_has(const sift_ctx* c, StageNeed need) {
  return !c->detect_pending && !c->begin_pending && c->have_kp && (need < kNeedOri || c->feat.have_ori) &&
         (need < kNeedDesc || c->feat.have_desc);
}

static int ctx_create(int device, sift_ctx* share, sift_ctx** out) {
  if (!out) return SIFT_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return SIFT_E_HIP;
  if (device < 0 || device >= n) return SIFT_E_ARG;
  sift_ctx* ctx = new sift_ctx();
  ctx->device = device;
  ctx->own_stream = share == nullptr;
  if (hipSetDevice(device) != hipSuccess ||
      (share ? (ctx->stream = share->stream, false)
             : hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) ||
      ctx->h_counters.ensure(kCntAll * sizeof(unsigned)) != hipSuccess ||
      ctx->hscratch.ensure(sizeof(StageScratch)) != hipSuccess ||
      ctx->counters.ensure(kCntAll * sizeof(unsigned)) != hipSuccess) {
    delete ctx;
    return SIFT_E_HIP;
  }
  (void)ctx->ev.ensure();
  (void)ctx->pyr.ev_go.ensure();
  (void)ctx->ref.ev_heavy.ensure();
  *out = ctx;
  return SIFT_OK;
}

extern "C" {

int sift_abi_version(void) { return SIFT_ABI_VERSION; }

int sift_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return SIFT_E_ARG;
  if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) return SIFT_E_HIP;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  g_reg_ranges[reinterpret_cast<uintptr_t>(p)] = bytes;
  return SIFT_OK;
}

int sift_host_unregister(void* p) {
  if (!p) return SIFT_E_ARG;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg_ranges.erase(reinterpret_cast<uintptr_t>(p));
  }
  return hipHostUnregister(p) == hipSuccess ? SIFT_OK : SIFT_E_HIP;
}

int sift_params_default(sift_params* p) {
  if (!p) return SIFT_E_ARG;
  p->num_octaves = 5;         // worker.js:33
  p->scales_per_octave = 3;   // worker.js:34
  p->min_blur = 0.8;          // worker.js:35
  p->assumed_blur = 0.5;      // worker.js:36
  p->min_interpixel_distance = 0.5;  // worker.js:88
  p->flags = 0;
  return SIFT_OK;
}

int sift_octave_dims(int width, int height, int num_octaves, int* dims) {
  if (width < 1 || height < 1 || num_octaves < 1 || !dims) return SIFT_E_ARG;
  int h = 2 * height, w = 2 * width;  // background.js:84 (2x upsample)
  for (int o = 0; o < num_octaves; ++o) {
    if (o > 0) { h = (h + 1) / 2; w = (w + 1) / 2; }  // background.js:118
    dims[2 * o] = h;
    dims[2 * o + 1] = w;
  }
  return SIFT_OK;
}

int sift_schedule(const sift_params* p, double* blur, double* sigma) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!blur || !sigma) return SIFT_E_ARG;
  // background.js:89-177
  const int S = p->scales_per_octave, NS = S + 3;
  const double k = std::pow(2.0, 1.0 / S);
  double base_blur = p->min_blur;
  for (int o = 0; o < p->num_octaves; ++o) {
    for (int s = 0; s < NS; ++s) {
      if (o > 0 && s == 0) {
        base_blur = blur[(o - 1) * NS + S];
        blur[o * NS] = base_blur;
        sigma[o * NS] = 0.0;
      } else {
        const double target = base_blur * std::pow(k, (double)s);
        const double from = o == 0 ? p->assumed_blur : base_blur;
        blur[o * NS + s] = target;
        sigma[o * NS + s] = std::sqrt((target * target) - (from * from));
      }
    }
  }
  return SIFT_OK;
}

int sift_ctx_create(int device, sift_ctx** out) { return ctx_create(device, nullptr, out); }

int sift_ctx_create_shared(sift_ctx* share, sift_ctx** out) {
  if (!share || !out) return SIFT_E_ARG;
  return ctx_create(share->device, share, out);
}

int sift_ctx_destroy(sift_ctx* ctx) {
  if (!ctx) return SIFT_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx;
  return SIFT_OK;
}

const char* sift_last_error(sift_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void* sift_stream(sift_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int sift_synchronize(sift_ctx* ctx) {
  if (!ctx) return SIFT_E_ARG;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_set_flags(sift_ctx* ctx, int flags) {
  if (!ctx) return SIFT_E_ARG;
  ctx->p.flags = flags;
  return SIFT_OK;
}

int sift_last_counts(sift_ctx* ctx, size_t* nc, size_t* nl, size_t* nk, size_t* ns, size_t* ne) {
  if (!ctx) return SIFT_E_ARG;
  if (nc) *nc = ctx->ext.n_cand;
  if (nl) *nl = ctx->ext.n_low;
  if (nk) *nk = ctx->n_kp;
  if (ns) *ns = ctx->ref.n_sing;
  if (ne) *ne = ctx->ext.n_exact;
  return SIFT_OK;
}

int sift_last_timings(sift_ctx* ctx, sift_timings* t) {
  if (!ctx || !t) return SIFT_E_ARG;
  *t = ctx->tm;
  return SIFT_OK;
}

int sift_last_octave_timings(sift_ctx* ctx, double* ms, int cap, int* n_out) {
  if (!ctx) return SIFT_E_ARG;
  const int n = (int)ctx->pyr.oct_ms.size();
  if (n_out) *n_out = n;
  if (!ms) return SIFT_OK;
  if (cap < n) return set_err(ctx, SIFT_E_CAPACITY, "destination too small (one per octave)");
  for (int o = 0; o < n; ++o) ms[o] = ctx->pyr.oct_ms[o];
  return SIFT_OK;
}

int sift_last_pass_kernels(sift_ctx* ctx, char* buf, size_t cap, size_t* len) {
  if (!ctx) return SIFT_E_ARG;
  const std::vector<std::string>& kn = ctx->pyr.pass_kn;
  std::string t;
  for (size_t o = 0; o < kn.size(); ++o) {
    if (kn[o].empty()) continue;
    if (!t.empty()) t += "; ";
    t += "o" + std::to_string(o) + ": " + kn[o];
  }
  if (len) *len = t.size();
  if (!buf) return SIFT_OK;
  if (cap < t.size() + 1) return set_err(ctx, SIFT_E_CAPACITY, "destination too small");
  std::memcpy(buf, t.c_str(), t.size() + 1);
  return SIFT_OK;
}

}  // extern "C"
