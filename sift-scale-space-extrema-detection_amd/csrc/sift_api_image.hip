// C ABI of the image products either side of the path: RGBA -> gray (and the RGBA entry points of the pyramid and
// the detection), pyramid planes -> display images.  Kernels: sift_image.hip.
#include "sift_ctx.h"

using namespace sift;

static int check_rgba(sift_ctx* ctx, const void* rgba, int W, int H, size_t stride_bytes) {
  if (!ctx) return SIFT_E_ARG;
  if (!rgba || W <= 0 || H <= 0) return set_err(ctx, SIFT_E_ARG, "null or empty RGBA image");
  if (stride_bytes < (size_t)W * 4 || stride_bytes % 4) return set_err(ctx, SIFT_E_ARG, "bad RGBA row stride");
  return SIFT_OK;
}

// Upload the RGBA rows (dense) and convert them into ctx->pyr.img on ctx's stream.
static int rgba_to_ctx_img(sift_ctx* ctx, const uint8_t* rgba, int W, int H, size_t stride_bytes,
                           bool alpha = false) {
  int rc = check_rgba(ctx, rgba, W, H, stride_bytes);
  if (rc) return rc;
  ImgState& I = ctx->img;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(I.rgba.ensure((size_t)W * H * 4));
  HIPCHK(ctx->pyr.img.ensure((size_t)W * H * sizeof(float)));
  if (stride_bytes == (size_t)W * 4 && host_registered(rgba, (size_t)W * H * 4))  // page-locked: one DMA
    HIPCHK(hipMemcpyAsync(I.rgba.p, rgba, (size_t)W * H * 4, hipMemcpyHostToDevice, ctx->stream));
  else
    HIPCHK(hipMemcpy2DAsync(I.rgba.p, (size_t)W * 4, rgba, stride_bytes, (size_t)W * 4, H, hipMemcpyHostToDevice,
                            ctx->stream));
  if (alpha) HIPCHK(I.alpha.ensure((size_t)W * H * sizeof(float)));
  HIPCHK(launch_rgba_to_gray(I.rgba.as<unsigned char>(), (size_t)W * 4, W, H, ctx->pyr.img.as<float>(),
                             alpha ? I.alpha.as<float>() : nullptr, ctx->stream));
  return SIFT_OK;
}

static int plane_image_common(sift_ctx* ctx, int kind, int o, int s, int mode, double coef, uint8_t* dst,
                              size_t cap_bytes, bool host) {
  if (!ctx || !dst) return SIFT_E_ARG;
  if (ctx->pyr.dog_source == kNone) return set_err(ctx, SIFT_E_STATE, "no pyramid");
  if (mode < SIFT_DISPLAY_PLAIN || mode > SIFT_DISPLAY_SAMPLED) return set_err(ctx, SIFT_E_ARG, "bad display mode");
  const float* src = nullptr;
  size_t plane = 0;
  const int rc = find_plane(ctx, kind, o, s, cap_bytes / 4, "destination too small (4 bytes per pixel)", &src, &plane);
  if (rc) return rc;
  ImgState& I = ctx->img;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(I.mm_parts.ensure((size_t)plane_image_parts((long long)plane) * sizeof(float2)));
  unsigned* out = reinterpret_cast<unsigned*>(dst);
  if (host) {
    HIPCHK(I.display.ensure(plane * 4));
    out = I.display.as<unsigned>();
  }
  HIPCHK(launch_plane_image(src, (long long)plane, mode, coef, I.mm_parts.as<float2>(), out, ctx->stream));
  if (host) HIPCHK(hipMemcpyAsync(dst, out, plane * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_rgba_to_gray_device(sift_ctx* ctx, const uint8_t* d_rgba, int width, int height, size_t stride_bytes,
                             float* d_gray, float* d_alpha) {
  int rc = check_rgba(ctx, d_rgba, width, height, stride_bytes);
  if (rc) return rc;
  if (!d_gray) return set_err(ctx, SIFT_E_ARG, "null gray destination");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(launch_rgba_to_gray(d_rgba, stride_bytes, width, height, d_gray, d_alpha, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_rgba_to_gray(sift_ctx* ctx, const uint8_t* rgba, int width, int height, size_t stride_bytes, float* gray,
                      float* alpha) {
  if (ctx && !gray) return set_err(ctx, SIFT_E_ARG, "null gray destination");
  int rc = rgba_to_ctx_img(ctx, rgba, width, height, stride_bytes, alpha != nullptr);
  if (rc) return rc;
  const size_t n = (size_t)width * height;
  if (alpha) HIPCHK(hipMemcpyAsync(alpha, ctx->img.alpha.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(gray, ctx->pyr.img.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SIFT_OK;
}

int sift_build_scale_space_rgba(sift_ctx* ctx, const uint8_t* rgba, int width, int height, size_t stride_bytes,
                                const sift_params* p, const double* sig) {
  int rc = rgba_to_ctx_img(ctx, rgba, width, height, stride_bytes);
  if (rc) return rc;
  return sift_build_scale_space_device(ctx, ctx->pyr.img.as<float>(), width, height, (size_t)width, p, sig);
}

int sift_detect_rgba(sift_ctx* ctx, const uint8_t* rgba, int width, int height, size_t stride_bytes,
                     const sift_params* p, sift_keypoint* out, size_t cap, size_t* n_out) {
  int rc = rgba_to_ctx_img(ctx, rgba, width, height, stride_bytes);
  if (rc) return rc;
  return sift_detect_device(ctx, ctx->pyr.img.as<float>(), width, height, (size_t)width, p, out, cap, n_out);
}

int sift_plane_image(sift_ctx* ctx, int kind, int octave, int scale, int mode, double coefficient, uint8_t* rgba,
                     size_t cap_bytes) {
  return plane_image_common(ctx, kind, octave, scale, mode, coefficient, rgba, cap_bytes, true);
}

int sift_plane_image_device(sift_ctx* ctx, int kind, int octave, int scale, int mode, double coefficient,
                            uint8_t* d_rgba, size_t cap_bytes) {
  return plane_image_common(ctx, kind, octave, scale, mode, coefficient, d_rgba, cap_bytes, false);
}
