// C ABI of the homography warp and of the 3 x 3 inverse that feeds it (kernels: sift_warp.hip).
#include "sift_ctx.h"

#pragma clang fp contract(off)

using namespace sift;

int sift_homography_inverse(const double h[9], double out[9]) {
  if (!out) return SIFT_E_ARG;
  for (int i = 0; i < 9; ++i) out[i] = 0.0;
  if (!h) return SIFT_E_ARG;
  double a[9];
  a[0] = h[4] * h[8] - h[5] * h[7];
  a[1] = h[2] * h[7] - h[1] * h[8];
  a[2] = h[1] * h[5] - h[2] * h[4];
  a[3] = h[5] * h[6] - h[3] * h[8];
  a[4] = h[0] * h[8] - h[2] * h[6];
  a[5] = h[2] * h[3] - h[0] * h[5];
  a[6] = h[3] * h[7] - h[4] * h[6];
  a[7] = h[1] * h[6] - h[0] * h[7];
  a[8] = h[0] * h[4] - h[1] * h[3];
  const double d = (h[0] * a[0] + h[1] * a[3]) + h[2] * a[6];
  if (d == 0.0 || !std::isfinite(d)) return SIFT_E_ARG;
  double r[9];
  for (int i = 0; i < 9; ++i) {
    r[i] = a[i] / d;
    if (!std::isfinite(r[i])) return SIFT_E_ARG;
  }
  for (int i = 0; i < 9; ++i) out[i] = r[i];
  return SIFT_OK;
}

namespace {

// One warp as every entry point sees it: a pixel is 4 bytes (a float, or an RGBA word), strides in pixels.
struct WarpCall {
  bool rgba;
  const void* src;
  int sw, sh;
  size_t sstride;
  const double* m;
  int mode;
  unsigned fill;  // the float's bits, or the four bytes
  void* dst;
  int dw, dh;
  size_t dstride;
  uint8_t* mask;
  size_t* n_valid;
};

inline bool px_ok(int w, int h) { return w > 0 && h > 0 && (size_t)w * (size_t)h < ((size_t)1 << 31); }

int warp_check(sift_ctx* ctx, const WarpCall& c, size_t sstride_given, size_t dstride_given) {
  if (!ctx) return SIFT_E_ARG;
  if (!c.src || !c.dst || !c.m) return set_err(ctx, SIFT_E_ARG, "null source, destination or matrix");
  if (c.sw <= 0 || c.sh <= 0 || c.dw <= 0 || c.dh <= 0) return set_err(ctx, SIFT_E_ARG, "empty source or destination");
  if (!px_ok(c.sw, c.sh) || !px_ok(c.dw, c.dh)) return set_err(ctx, SIFT_E_ARG, "width * height >= 2^31");
  if (c.rgba && (sstride_given % 4 || dstride_given % 4))
    return set_err(ctx, SIFT_E_ARG, "RGBA row stride not a multiple of 4");
  if (c.sstride < (size_t)c.sw || c.dstride < (size_t)c.dw) return set_err(ctx, SIFT_E_ARG, "row stride below the width");
  if (c.mode != SIFT_WARP_NEAREST && c.mode != SIFT_WARP_BILINEAR) return set_err(ctx, SIFT_E_ARG, "bad warp mode");
  if (c.dst == c.src) return set_err(ctx, SIFT_E_ARG, "the destination is the source");
  return SIFT_OK;
}

// The kernels over device memory, queued with their events and the count's read-back; not waited for.
int warp_enqueue(sift_ctx* ctx, const WarpCall& c, const void* d_src, size_t sstride, void* d_dst, size_t dstride,
                 uint8_t* d_mask) {
  WarpState& W = ctx->warp;
  HIPCHK(W.ev.ensure());
  unsigned* d_count = nullptr;
  if (c.n_valid) {
    HIPCHK(W.count.ensure((1 + kWarpMaxBlocks) * sizeof(unsigned)));
    d_count = W.count.as<unsigned>();
  }
  unsigned* d_partial = d_count ? d_count + 1 : nullptr;
  const bool bilinear = c.mode == SIFT_WARP_BILINEAR;
  HIPCHK(hipEventRecord(W.ev[0], ctx->stream));
  if (c.rgba) {
    HIPCHK(launch_warp_rgba(static_cast<const unsigned*>(d_src), c.sw, c.sh, sstride, c.m, bilinear, c.fill,
                            static_cast<unsigned*>(d_dst), c.dw, c.dh, dstride, d_mask, d_partial, d_count, ctx->stream));
  } else {
    float fill;
    std::memcpy(&fill, &c.fill, sizeof fill);
    HIPCHK(launch_warp_gray(static_cast<const float*>(d_src), c.sw, c.sh, sstride, c.m, bilinear, fill,
                            static_cast<float*>(d_dst), c.dw, c.dh, dstride, d_mask, d_partial, d_count, ctx->stream));
  }
  HIPCHK(hipEventRecord(W.ev[1], ctx->stream));
  if (d_count)
    HIPCHK(hipMemcpyAsync(&static_cast<StageScratch*>(ctx->hscratch.p)->word, d_count, sizeof(unsigned),
                          hipMemcpyDeviceToHost, ctx->stream));
  return SIFT_OK;
}

// Waits for the stream, then the timing and the count.
int warp_finish(sift_ctx* ctx, const WarpCall& c) {
  HIPCHK(hipStreamSynchronize(ctx->stream));
  take_event_ms(&ctx->warp.warp_ms, ctx->warp.ev[0], ctx->warp.ev[1]);
  if (c.n_valid) *c.n_valid = static_cast<StageScratch*>(ctx->hscratch.p)->word;
  return SIFT_OK;
}

int warp_device(sift_ctx* ctx, const WarpCall& c, size_t sstride_given, size_t dstride_given) {
  if (int rc = warp_check(ctx, c, sstride_given, dstride_given)) return rc;
  if (c.rgba && ((reinterpret_cast<uintptr_t>(c.src) | reinterpret_cast<uintptr_t>(c.dst)) & 3))
    return set_err(ctx, SIFT_E_ARG, "RGBA device image not 4-byte aligned");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = warp_enqueue(ctx, c, c.src, c.sstride, c.dst, c.dstride, c.mask)) return rc;
  return warp_finish(ctx, c);
}

// Host rows <-> a dense device image of w x h 4-byte pixels: one DMA when the host side is dense and page-locked.
hipError_t rows_copy(void* dst, size_t dpitch, const void* src, size_t spitch, int w, int h, const void* host,
                     size_t host_pitch, hipMemcpyKind kind, hipStream_t st) {
  const size_t row = (size_t)w * 4;
  if (host_pitch == row && host_registered(host, row * h)) return hipMemcpyAsync(dst, src, row * h, kind, st);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, row, h, kind, st);
}

int warp_host_queued(sift_ctx* ctx, const WarpCall& c) {
  WarpState& W = ctx->warp;
  const size_t srow = (size_t)c.sw * 4, drow = (size_t)c.dw * 4, npx = (size_t)c.dw * c.dh;
  HIPCHK(W.src.ensure(srow * c.sh));
  HIPCHK(W.dst.ensure(drow * c.dh));
  if (c.mask) HIPCHK(W.mask.ensure(npx));
  HIPCHK(rows_copy(W.src.p, srow, c.src, c.sstride * 4, c.sw, c.sh, c.src, c.sstride * 4, hipMemcpyHostToDevice,
                   ctx->stream));
  if (int rc = warp_enqueue(ctx, c, W.src.p, (size_t)c.sw, W.dst.p, (size_t)c.dw, c.mask ? W.mask.as<uint8_t>() : nullptr))
    return rc;
  HIPCHK(rows_copy(c.dst, c.dstride * 4, W.dst.p, drow, c.dw, c.dh, c.dst, c.dstride * 4, hipMemcpyDeviceToHost,
                   ctx->stream));
  if (c.mask) HIPCHK(hipMemcpyAsync(c.mask, W.mask.p, npx, hipMemcpyDeviceToHost, ctx->stream));
  return warp_finish(ctx, c);
}

int warp_host(sift_ctx* ctx, const WarpCall& c, size_t sstride_given, size_t dstride_given) {
  if (int rc = warp_check(ctx, c, sstride_given, dstride_given)) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  return host_image_exit(ctx, warp_host_queued(ctx, c));  // the caller's memory is free of DMA on every exit
}

unsigned fill_bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}
unsigned fill_bits(const uint8_t* f) {
  unsigned u = 0;
  if (f) std::memcpy(&u, f, sizeof u);
  return u;
}

}  // namespace

int sift_warp_gray_device(sift_ctx* ctx, const float* d_src, int src_w, int src_h, size_t src_stride_px,
                          const double m[9], int mode, float fill, float* d_dst, int dst_w, int dst_h,
                          size_t dst_stride_px, uint8_t* d_mask, size_t* n_valid) {
  return warp_device(ctx, WarpCall{false, d_src, src_w, src_h, src_stride_px, m, mode, fill_bits(fill), d_dst, dst_w,
                                   dst_h, dst_stride_px, d_mask, n_valid},
                     src_stride_px, dst_stride_px);
}

int sift_warp_gray(sift_ctx* ctx, const float* src, int src_w, int src_h, size_t src_stride_px, const double m[9],
                   int mode, float fill, float* dst, int dst_w, int dst_h, size_t dst_stride_px, uint8_t* mask,
                   size_t* n_valid) {
  return warp_host(ctx, WarpCall{false, src, src_w, src_h, src_stride_px, m, mode, fill_bits(fill), dst, dst_w, dst_h,
                                 dst_stride_px, mask, n_valid},
                   src_stride_px, dst_stride_px);
}

int sift_warp_rgba_device(sift_ctx* ctx, const uint8_t* d_src, int src_w, int src_h, size_t src_stride_bytes,
                          const double m[9], int mode, const uint8_t fill[4], uint8_t* d_dst, int dst_w, int dst_h,
                          size_t dst_stride_bytes, uint8_t* d_mask, size_t* n_valid) {
  if (ctx && !fill) return set_err(ctx, SIFT_E_ARG, "null fill");
  return warp_device(ctx, WarpCall{true, d_src, src_w, src_h, src_stride_bytes / 4, m, mode, fill_bits(fill), d_dst,
                                   dst_w, dst_h, dst_stride_bytes / 4, d_mask, n_valid},
                     src_stride_bytes, dst_stride_bytes);
}

int sift_warp_rgba(sift_ctx* ctx, const uint8_t* src, int src_w, int src_h, size_t src_stride_bytes, const double m[9],
                   int mode, const uint8_t fill[4], uint8_t* dst, int dst_w, int dst_h, size_t dst_stride_bytes,
                   uint8_t* mask, size_t* n_valid) {
  if (ctx && !fill) return set_err(ctx, SIFT_E_ARG, "null fill");
  return warp_host(ctx, WarpCall{true, src, src_w, src_h, src_stride_bytes / 4, m, mode, fill_bits(fill), dst, dst_w,
                                 dst_h, dst_stride_bytes / 4, mask, n_valid},
                   src_stride_bytes, dst_stride_bytes);
}

int sift_last_warp_timing(sift_ctx* ctx, double* warp_ms) {
  if (!ctx) return SIFT_E_ARG;
  if (warp_ms) *warp_ms = ctx->warp.warp_ms;
  return SIFT_OK;
}
