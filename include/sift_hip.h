/*
 * sift_hip.h -- C ABI of the MI355X (gfx950) SIFT scale-space extrema path.
 *
 * This is the drop-in boundary for the reference's hot path
 * (bingjetli/sift-scale-space-extrema-detection).  The reference exposes the
 * path as a Web-Worker message protocol (src/worker.js:5-98 helpers,
 * background.js:14-50 dispatcher); every entry point below names the
 * reference function whose behaviour it reproduces.  Plain C types only: no
 * C++ or torch types cross this boundary.  The Node N-API addon
 * (sift-scale-space-extrema-detection_amd/napi/sift_napi.c) and the Python
 * ctypes binding bind exactly these symbols.
 *
 * Threading: one sift_ctx per host thread; a ctx is not re-entrant; distinct
 * ctxs are independent.  Every call is synchronous with respect to the ctx's
 * HIP stream unless its name ends in _async.
 *
 * Numerics: Gaussian weights and every convolution accumulate in fp64 (the
 * reference computes in JS Number = fp64); Gaussian and DoG planes are
 * handed out as fp32 (the ImageData-shaped Float32 contract); octave seeds
 * stay fp64 on device; extrema decisions and refinement are fp64 and exact
 * with respect to the fp64 pyramid (fp32 ties are re-decided in fp64).
 */
#ifndef SIFT_HIP_H
#define SIFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT_ABI_VERSION 10

/* Opaque context (one HIP stream + device-resident pyramids). */
struct sift_ctx;

/* Status codes.  Every function returns one of these. */
enum {
  SIFT_OK = 0,
  SIFT_E_ARG = -1,        /* invalid argument (null pointer, bad size, bad index)   */
  SIFT_E_HIP = -2,        /* HIP runtime error; see sift_last_error()               */
  SIFT_E_CAPACITY = -3,   /* output buffer too small; *n_out holds the needed count */
  SIFT_E_STATE = -4,      /* stage called before the stage it depends on            */
  SIFT_E_SINGULAR = -5,   /* refinement met a Hessian with |det| < DBL_EPSILON: the
                             reference throws a TypeError there (matrix2d.js:482 ->
                             :455); outputs for every other candidate are still
                             written and *n_singular counts the offenders           */
  SIFT_E_UNSUPPORTED = -6 /* configuration outside this build's limits              */
};

/* Plane kinds for sift_get_plane / sift_get_blur_level. */
enum { SIFT_PLANE_GAUSS = 0, SIFT_PLANE_DOG = 1 };

/* sift_params.flags */
enum {
  SIFT_F_SKIP_GAUSS_PLANES = 1 << 0, /* do not materialise Gaussian planes (seeds still kept) */
  SIFT_F_SKIP_DOG_PLANES = 1 << 1,   /* reserved: DoG planes are needed by refinement today   */
  SIFT_F_EXPORT_NEXT_SEED = 1 << 2,  /* also form the fp64 base of octave num_octaves (sift_next_seed) */
  SIFT_F_KEYPOINT_ORIGINS = 1 << 3,  /* record each keypoint's candidate (sift_keypoint_origins) */
  SIFT_F_FUSED_EXTREMA = 1 << 4,     /* detections: decide octave 0's extrema inside its Gaussian+DoG
                                        pass instead of re-reading its DoG planes (same results;
                                        measured slower on MI355X) */
  SIFT_F_LOW_CONTRAST_LIST = 1 << 5  /* also list the low-contrast extrema (sift_copy_low_contrast) */
};

/* Parameters of the pipeline.  Names and defaults follow
 * src/worker.js:29-98 (workerComputeGaussianScaleSpace / ...Refine...). */
typedef struct {
  int num_octaves;                /* number_of_octaves        default 5   (worker.js:33) */
  int scales_per_octave;          /* scales_per_octave        default 3   (worker.js:34) */
  double min_blur;                /* min_blur_level           default 0.8 (worker.js:35) */
  double assumed_blur;            /* assumed_blur             default 0.5 (worker.js:36) */
  double min_interpixel_distance; /* min_interpixel_distance  default 0.5 (worker.js:88) */
  int flags;                      /* SIFT_F_*                 default 0                  */
} sift_params;

/* One candidate extremum, reference order (octave, scale, y, x):
 * background.js:433-436 {scaleLevel, localExtremas:[{x, y, value}]}. */
typedef struct {
  int32_t octave;
  int32_t scale; /* scaleLevel: DoG index 1..S */
  int32_t x;
  int32_t y;
  double value; /* DoG value at (x, y) */
} sift_extremum;

/* One refined keypoint: background.js:619-628. */
typedef struct {
  int32_t octave;
  int32_t scale_level;
  int32_t local_x;
  int32_t local_y;
  double abs_x;
  double abs_y;
  double abs_sigma;
  double interp_value;
} sift_keypoint;

/* Per-stage device timings of the last call chain, milliseconds. */
typedef struct {
  double gauss_dog_ms; /* Gaussian + DoG kernels (all octaves)              */
  double extrema_ms;   /* extrema scan + ordering + exact tie resolution    */
  double refine_ms;    /* refinement + compaction                           */
  double h2d_ms;       /* input upload (0 for the device-pointer entry)     */
  double gauss_oct0_ms;/* octave 0's Gaussian + DoG launch alone (the        */
                       /* dominant, HBM-bound kernel; ABI version >= 2)     */
} sift_timings;

int sift_abi_version(void);
int sift_params_default(sift_params *p);

/* Context: owns one HIP stream and device-resident pyramids on `device`. */
int sift_ctx_create(int device, struct sift_ctx **out);
/* A context on the SAME stream as `share` (ABI version >= 2): its work is
 * ordered after everything already enqueued on `share`, so several
 * detections can be in flight (sift_detect_device_async) without their
 * kernels overlapping.  Destroy it before `share`. */
int sift_ctx_create_shared(struct sift_ctx *share, struct sift_ctx **out);
int sift_ctx_destroy(struct sift_ctx *ctx);
const char *sift_last_error(struct sift_ctx *ctx);

/* Offset sigma and blur level of every (octave, scale) for these params,
 * background.js:89-177.  Arrays are num_octaves*(scales_per_octave+3);
 * sigma 0 marks the un-blurred octave seed.  Pure host math. */
int sift_schedule(const sift_params *p, double *blur_levels, double *offset_sigmas);

/* Octave plane dims for a W x H input: dims[2o] = rows, dims[2o+1] = cols.
 * Pure host math (matrix2d.js:112-138 resize rules). */
int sift_octave_dims(int width, int height, int num_octaves, int *dims);

/* computeGaussianScaleSpace (background.js:71-237) fused with
 * computeDifferenceOfGaussians (background.js:258-354).  `img` is a gray
 * row-major Float32 host image (ImageData-shaped, stride in pixels).
 * `offset_sigmas` may be NULL (schedule computed here) or supply the
 * num_octaves*(S+3) offset sigmas computed by the caller (e.g. in JS with
 * Math.pow, so the schedule is bit-identical to the reference's). */
int sift_build_scale_space(struct sift_ctx *ctx, const float *img, int width, int height,
                           size_t stride_px, const sift_params *p, const double *offset_sigmas);

/* Same, with `d_img` already resident in device memory of ctx's device. */
int sift_build_scale_space_device(struct sift_ctx *ctx, const float *d_img, int width,
                                  int height, size_t stride_px, const sift_params *p,
                                  const double *offset_sigmas);

int sift_get_dims(struct sift_ctx *ctx, int octave, int *rows, int *cols);
int sift_get_blur_level(struct sift_ctx *ctx, int kind, int octave, int scale, double *blur);

/* Copy one plane to host memory owned by the caller (cap in pixels). */
int sift_get_plane(struct sift_ctx *ctx, int kind, int octave, int scale, float *dst,
                   size_t cap_px);

/* Replace the context's DoG pyramid with caller-supplied planes (for callers
 * that hand findCandidateKeypoints / refineCandidateKeypoints a pyramid this
 * context did not build).  `planes` is octave-major, (S+2) planes per
 * octave, each rows*cols fp32 in the dims sift_octave_dims gives. */
int sift_load_dog(struct sift_ctx *ctx, const float *planes, int width, int height,
                  const sift_params *p);

/* Replace the Gaussian pyramid with caller planes ((S+3) per octave) and
 * recompute the DoG from them: computeDifferenceOfGaussians on a foreign
 * scale space (background.js:258-354, sift.js:154-188). */
int sift_load_scale_space(struct sift_ctx *ctx, const float *planes, int width, int height,
                          const sift_params *p);

/* findCandidateKeypoints (background.js:359-450 + sift.js:212-316).
 * Strict 26-neighbour extrema of DoG scales 1..S with |v| >= 0.8*thr, in
 * reference order.  *n_low_contrast counts extrema failing 0.8*thr.
 * SIFT_E_CAPACITY: *n_out = required count, nothing written. */
int sift_find_extrema(struct sift_ctx *ctx, sift_extremum *out, size_t cap, size_t *n_out,
                      size_t *n_low_contrast);

/* The low-contrast extrema of the last extrema stage run with
 * SIFT_F_LOW_CONTRAST_LIST in its parameters (ABI version >= 5): strict
 * 26-neighbour extrema with |v| < 0.8*thr, the reference's
 * lowContrastKeypoints (sift.js:293-306), in its order (octave, scale, y, x)
 * with their DoG values.  SIFT_E_CAPACITY: *n_out = required count. */
int sift_copy_low_contrast(struct sift_ctx *ctx, sift_extremum *out, size_t cap, size_t *n_out);

/* Replace the sift_params.flags the context's current pyramid was built or
 * loaded with, for the stages that follow (ABI version >= 5): e.g.
 * SIFT_F_LOW_CONTRAST_LIST before sift_find_extrema on a built pyramid. */
int sift_set_flags(struct sift_ctx *ctx, int flags);

/* refineCandidateKeypoints (background.js:455-685) on the candidates of the
 * last sift_find_extrema (or sift_set_candidates).  Output keeps reference
 * order and duplicates. */
int sift_refine(struct sift_ctx *ctx, sift_keypoint *out, size_t cap, size_t *n_out,
                size_t *n_singular);

/* Copy the candidates / keypoints of the last find / refine / detect without
 * recomputing (cap in records; SIFT_E_CAPACITY if too small). */
int sift_copy_candidates(struct sift_ctx *ctx, sift_extremum *out, size_t cap, size_t *n_out);
int sift_copy_keypoints(struct sift_ctx *ctx, sift_keypoint *out, size_t cap, size_t *n_out);
/* The last keypoints as two field arrays (the JS typed result format):
 * ints[4i..4i+3] = octave, scale_level, local_x, local_y and reals[4i..4i+3]
 * = abs_sigma, abs_x, abs_y, interp_value of keypoint i, in the reference's
 * order (background.js:660-671).  Through the context's pinned staging. */
int sift_copy_keypoints_soa(struct sift_ctx *ctx, int32_t *ints, double *reals, size_t cap, size_t *n_out);

/* Page-lock a caller's host buffer for the device's DMA engines (ABI version
 * >= 8): plane and keypoint reads into a registered buffer are one
 * device -> host DMA instead of a staged copy through pinned memory.  For
 * buffers the caller recycles (the JS addon's result pool); unregister
 * before freeing.  Registration faults in and pins every page. */
int sift_host_register(void *p, size_t bytes);
int sift_host_unregister(void *p);

/* Override the two scalars refineCandidateKeypoints receives in its own
 * message (minBlurLevel, minInterpixelDistance: background.js:460-461,
 * :611-614) for the next sift_refine; build/load set them from sift_params. */
int sift_refine_params(struct sift_ctx *ctx, double min_blur_level, double min_interpixel_distance);

/* Use caller-supplied candidates (reference order) for the next sift_refine. */
int sift_set_candidates(struct sift_ctx *ctx, const sift_extremum *cand, size_t n);

/* Whole path in one call: build + extrema + refine.  Keypoints stay on
 * device when out == NULL (counts still returned). */
int sift_detect(struct sift_ctx *ctx, const float *img, int width, int height, size_t stride_px,
                const sift_params *p, sift_keypoint *out, size_t cap, size_t *n_out);
int sift_detect_device(struct sift_ctx *ctx, const float *d_img, int width, int height,
                       size_t stride_px, const sift_params *p, sift_keypoint *out, size_t cap,
                       size_t *n_out);

/* Counts of the last detect / find / refine: candidates, low-contrast
 * extrema, refined keypoints, singular Hessians, exact fp64 re-decisions. */
int sift_last_counts(struct sift_ctx *ctx, size_t *n_candidates, size_t *n_low_contrast,
                     size_t *n_keypoints, size_t *n_singular, size_t *n_exact);

/* Asynchronous one-call detection (ABI version >= 2): enqueue on the
 * context's stream and return; sift_detect_wait completes it (one host
 * synchronisation, capacity retries, counts) and copies the keypoints like
 * sift_detect.  One detection in flight per context: several contexts
 * (streams) keep the device busy while the host settles earlier images. */
int sift_detect_device_async(struct sift_ctx *ctx, const float *d_img, int width, int height,
                             size_t stride_px, const sift_params *p);
int sift_detect_wait(struct sift_ctx *ctx, sift_keypoint *out, size_t cap, size_t *n_out);

/* A batch of n_images independent device images of one geometry (ABI
 * version >= 6; BASELINE cfg 4's images per GPU): image b is width x height
 * at d_imgs + b * image_stride_px (row stride stride_px).  Each stage is ONE
 * launch over the whole batch -- a Gaussian+DoG launch per octave, one
 * extrema scan, one refinement -- with the planes image-major.  Per image the
 * results are exactly those of sift_detect_device on that image (the
 * reference's per-image path, background.js:71-685, run once per image); the
 * keypoints come out image-major, each image's in the reference's order, and
 * sift_last_block_counts gives n_images * num_octaves * scales_per_octave
 * block counts (image-major), so image b's count is the sum of its blocks.
 * Plain detection only: no low-contrast list, fused decisions, crops, owned
 * rows or exported seeds (SIFT_E_UNSUPPORTED); the candidate list of a batch
 * is not exposed.  _async enqueues it (sift_detect_wait completes it). */
int sift_detect_batch_device(struct sift_ctx *ctx, const float *d_imgs, int n_images, size_t image_stride_px,
                             int width, int height, size_t stride_px, const sift_params *p,
                             sift_keypoint *out, size_t cap, size_t *n_out);
/* The same batch from host images (image b at imgs + b * image_stride_px),
 * uploaded image by image into the context's device buffer. */
int sift_detect_batch(struct sift_ctx *ctx, const float *imgs, int n_images, size_t image_stride_px, int width,
                      int height, size_t stride_px, const sift_params *p, sift_keypoint *out, size_t cap,
                      size_t *n_out);
int sift_detect_batch_device_async(struct sift_ctx *ctx, const float *d_imgs, int n_images,
                                   size_t image_stride_px, int width, int height, size_t stride_px,
                                   const sift_params *p);

/* The same detection in two phases (ABI version >= 4): _begin enqueues the
 * Gaussian+DoG pass, _end the extrema scan and refinement; sift_detect_wait
 * completes it.  Between the two, sift_order_after can hold the second
 * phase back behind other contexts' work (bench.py --overlap phased: the
 * next image's octave 0 runs before this image's extrema scan, so the
 * HBM-bound phases of consecutive images alternate instead of contending). */
int sift_detect_begin_async(struct sift_ctx *ctx, const float *d_img, int width, int height, size_t stride_px,
                            const sift_params *p);
int sift_detect_end_async(struct sift_ctx *ctx);

/* Software pipelining of consecutive images on contexts with their own
 * streams (ABI version >= 3): the next work enqueued on ctx waits until
 * prev's last enqueued detection has passed `after`:
 *   SIFT_AFTER_OCTAVE0     its octave-0 Gaussian+DoG (HBM-write bound) -- the
 *                          next image's octave 0 then overlaps prev's small
 *                          octaves, extrema scan and refinement;
 *   SIFT_AFTER_GAUSSIAN    its whole Gaussian+DoG pass;
 *   SIFT_AFTER_REFINEMENT  its fast refinement (only the latency-bound tail
 *                          overlaps).
 * No-op for contexts sharing one stream (already in order). */
enum { SIFT_AFTER_OCTAVE0 = 0, SIFT_AFTER_GAUSSIAN = 1, SIFT_AFTER_REFINEMENT = 2 };
int sift_order_after(struct sift_ctx *ctx, const struct sift_ctx *prev, int after);

int sift_last_timings(struct sift_ctx *ctx, sift_timings *t);

/* Per-octave Gaussian+DoG launch times of the last build / detection, ms
 * (ABI version >= 5): ms[o] for o < *n_octaves (0 for octaves not built).
 * Launch o is timed from the end of launch o-1 on the same stream, so with
 * other streams' work overlapping it includes the wait for CUs. */
int sift_last_octave_timings(struct sift_ctx *ctx, double *ms, int cap, int *n_octaves);

/* The kernels the last build / detection launched for its Gaussian+DoG pass
 * (ABI version >= 9), one entry per octave: "o0: k_gauss_dog<octave0>; o1:
 * k_gauss_rw<12>; ..." -- what bench.py's roofline.kernel reports.  Writes
 * at most cap bytes including the terminating NUL; *len = the full length
 * (excluding the NUL); SIFT_E_CAPACITY when cap is too small. */
int sift_last_pass_kernels(struct sift_ctx *ctx, char *buf, size_t cap, size_t *len);

/* The launch plan of one octave's Gaussian+DoG pass as the last build /
 * detection launched it (ABI version >= 10): a read-only copy of what the
 * library decided, for tests that must prove which code they ran.  Nothing
 * here is an input, and the fields may grow with the kernels. */
enum { /* sift_gauss_plan_info.kernel: the instantiation */
  SIFT_GAUSS_K_STAGED8 = 0,       /* k_gauss_dog<octave0>, largest radius <= 8        */
  SIFT_GAUSS_K_STAGED16 = 1,      /* ... 9..16                                         */
  SIFT_GAUSS_K_STAGED8_FUSED = 2, /* the same two with fused extrema decisions        */
  SIFT_GAUSS_K_STAGED16_FUSED = 3,
  SIFT_GAUSS_K_TILES = 4,         /* k_gauss_dog<64>; also octave 0 on the fp64 base  */
  SIFT_GAUSS_K_SPLIT_TILES = 5,   /* k_gauss_vert + k_gauss_dog<64>                   */
  SIFT_GAUSS_K_WINDOW12 = 6,      /* k_gauss_rw<12>                                   */
  SIFT_GAUSS_K_WINDOW16 = 7,      /* k_gauss_rw<16>, <24>: experiments only           */
  SIFT_GAUSS_K_WINDOW24 = 8,
  SIFT_GAUSS_K_STREAMED12 = 9,    /* k_gauss_rw<12,true>: experiments only            */
  SIFT_GAUSS_K_STREAMED16 = 10,   /* k_gauss_rw<16,true>                              */
  SIFT_GAUSS_K_STREAMED24 = 11    /* k_gauss_rw<24,true>                              */
};
enum { /* sift_gauss_plan_info.path */
  SIFT_GAUSS_PATH_STAGED0 = 0,     /* octave 0 from the staged input region           */
  SIFT_GAUSS_PATH_BASE0 = 1,       /* octave 0 on a materialised fp64 upsample        */
  SIFT_GAUSS_PATH_TILES = 2,       /* 64 x 32 tiles                                   */
  SIFT_GAUSS_PATH_SPLIT_TILES = 3, /* split vertical pass, then 64 x 32 tiles         */
  SIFT_GAUSS_PATH_WINDOW = 4,      /* register-window tiles                           */
  SIFT_GAUSS_PATH_STREAMED = 5     /* ... with the window streamed per scale          */
};
#define SIFT_GAUSS_MAX_GROUPS 12
typedef struct sift_gauss_plan_info {
  int32_t kernel;             /* SIFT_GAUSS_K_*, as launched (a fused launch: the fused one) */
  int32_t path;               /* SIFT_GAUSS_PATH_*                                    */
  int32_t rw;                 /* k_gauss_rw: window radius 12 / 16 / 24; else 0       */
  int32_t tile_w, tile_rows;  /* output columns x rows per block (unfused)            */
  int32_t gx, gy;             /* tiles per row, tile rows, as launched (a fused launch
                                 steps by its own decided columns x rows)             */
  int32_t G;                  /* scale groups, as launched                            */
  int32_t gb[SIFT_GAUSS_MAX_GROUPS + 1]; /* group g computes scales gb[g] .. gb[g+1]-1 */
  int32_t sw;                 /* LDS strip row stride, doubles                        */
  int32_t zero;               /* a generic-radius body is present                     */
  int32_t keep_l64;           /* the octave keeps its fp64 Gaussian planes            */
  int32_t vsplit;             /* the split vertical pass ran first                    */
  int32_t xcd_band;           /* XCD-banded tile order                                */
  int32_t vec;                /* 16-byte plane stores, as launched                    */
  int32_t fused;              /* extrema decisions ran inside this launch             */
} sift_gauss_plan_info;
/* SIFT_E_STATE without a pyramid built by this library or for an octave the
 * last build did not launch; SIFT_E_ARG for an octave out of range. */
int sift_last_gauss_plan(struct sift_ctx *ctx, int octave, sift_gauss_plan_info *out);

/* Device-to-device copy of the last keypoints into caller device memory
 * (e.g. an RCCL all-gather send buffer), ordered on ctx's stream and
 * completed before return. */
int sift_copy_keypoints_device(struct sift_ctx *ctx, void *d_dst, size_t cap, size_t *n_out);

/* Raw device pointers (for in-process consumers that stay on device, e.g.
 * the RCCL all-gather of keypoints).  Valid until the next build/detect. */
int sift_device_keypoints(struct sift_ctx *ctx, const sift_keypoint **d_kp, size_t *n);
void *sift_stream(struct sift_ctx *ctx);

/* Row-band sharding of one image over several devices (ABI version >= 3;
 * SURVEY.md §8e cfg 5, no reference counterpart: the reference is one Web
 * Worker).  A shard runs the leading octaves on a crop of whole input rows
 * (sift_detect with num_octaves = K + 1, SIFT_F_EXPORT_NEXT_SEED and
 * SIFT_F_KEYPOINT_ORIGINS), keeps the keypoints whose candidate row it owns
 * and contributes its owned rows of the octave-(K+1) base; the base rows of
 * all shards make the whole base, from which sift_detect_from_seed runs the
 * trailing octaves.  The pipeline is translation invariant in y, so rows far
 * enough from a crop edge are bit-identical to the whole-image run. */

/* Input row of the first row of the images given to the following builds /
 * detections (a crop of whole rows of a taller image; default 0): keypoint
 * local_y / abs_y and origins are reported in the whole image's rows.  The
 * crop's first row must be a multiple of 2^(num_octaves - 1) (octave rows
 * stay whole). */
int sift_set_row_origin(struct sift_ctx *ctx, int input_row0);

/* Keep only the keypoints whose candidate lies in input rows [row_begin,
 * row_end) of the whole image (row_end < 0: to the bottom; row_begin < 0:
 * every keypoint, the default) in the following refinements / detections
 * (ABI version >= 5): a row band's share of a sharded image, decided by the
 * candidate's octave row as the band plan cuts it (octave 0: 2 r, octave o:
 * r >> (o - 1)).  Applied in the keypoint compaction on the device. */
int sift_set_owned_rows(struct sift_ctx *ctx, int row_begin, int row_end);

/* Kept keypoints per (octave, scale) block of the last refinement /
 * detection (ABI version >= 5): counts[o * S + s - 1], *n_blocks =
 * num_octaves * scales_per_octave.  Host memory; the keypoint list is in
 * block order, so these are its block boundaries
 * (sift_merge_keypoint_blocks_device). */
int sift_last_block_counts(struct sift_ctx *ctx, int64_t *counts, int cap, int *n_blocks);

/* The fp64 base of octave num_octaves formed by the last build with
 * SIFT_F_EXPORT_NEXT_SEED: rows x cols, row-major (host copy / device
 * pointer valid until the next build). */
int sift_next_seed(struct sift_ctx *ctx, double *dst, size_t cap, int *rows, int *cols);
int sift_device_next_seed(struct sift_ctx *ctx, const double **d_seed, int *rows, int *cols);

/* Detection of octaves octave_first .. num_octaves-1 of a width x height
 * input from the fp64 base of octave octave_first (>= 1; rows x cols as
 * sift_octave_dims gives, row-major, host or device memory).  Octave
 * indices, scales and absolute coordinates are those of the whole-image run. */
int sift_detect_from_seed(struct sift_ctx *ctx, int octave_first, const double *seed, int width, int height,
                          const sift_params *p, sift_keypoint *out, size_t cap, size_t *n_out);
int sift_detect_from_seed_device(struct sift_ctx *ctx, int octave_first, const double *d_seed, int width,
                                 int height, const sift_params *p, sift_keypoint *out, size_t cap,
                                 size_t *n_out);

/* Detection of a tail of octaves split over several devices (ABI version >= 5):
 * like sift_detect_from_seed_device, building octaves octave_first ..
 * p->num_octaves - 1 from the fp64 base of octave_first, but scanning only
 * octaves octave_scan_first .. p->num_octaves - 1 for extrema.  The octaves
 * before it are evaluated for their successor's base only (L[S] at even rows
 * and columns, bit-identical to the full build): they have no Gaussian or
 * DoG planes (sift_get_plane returns SIFT_E_STATE for them).  Rank j of a
 * row-band run builds the tail up to its octave and detects that one
 * octave. */
int sift_detect_from_seed_range_device(struct sift_ctx *ctx, int octave_first, int octave_scan_first,
                                       const double *d_seed, int width, int height, const sift_params *p,
                                       sift_keypoint *out, size_t cap, size_t *n_out);

/* Block-major merge of keypoint lists in device memory (ABI version >= 5):
 * d_in holds n_parts lists back to back; list q holds, in block order,
 * counts[q * n_blocks + b] keypoints of block b.  d_out receives block 0 of
 * every list in list order, then block 1, ...  With blocks = (octave, scale)
 * and lists = row bands in row order, this is the reference's candidate order
 * (octave, scale, y, x) without a sort.  A negative count skips that many
 * records of list q in d_in (padding, e.g. of an all-gather padded to the
 * largest list); they are not copied.  counts is host memory; completes
 * before return. */
int sift_merge_keypoint_blocks_device(struct sift_ctx *ctx, const sift_keypoint *d_in, const int64_t *counts,
                                      int n_parts, int n_blocks, sift_keypoint *d_out);

/* The candidate (octave, scale, y, x) of each keypoint of the last
 * detection/refinement run with SIFT_F_KEYPOINT_ORIGINS: 4 int32 per
 * keypoint, keypoint order (the reference's candidate order). */
int sift_keypoint_origins(struct sift_ctx *ctx, int32_t *out, size_t cap, size_t *n_out);

/* ---- Image products either side of the path (ABI version >= 4) ---------- */

/* ImageUtils_convertImageDataToMatrix2D({convertToGrayscale: true,
 * usePerceptualGrayscale: true}) (image-utils.js:27-152, called by
 * main.js:98-103) on device: gray = ((R*0.299) + (G*0.587) + (B*0.114)) / 255,
 * alpha = A / 255, evaluated in fp64 in that order and rounded once to fp32
 * (bit-identical to Float32Array.from(<the reference's gray Matrix2D>)).
 * `rgba` is ImageData.data (Uint8 R,G,B,A per pixel, row stride in bytes, a
 * multiple of 4); `gray` (required) and `alpha` (NULL = discardAlphaChannel)
 * are dense width*height fp32.  Host buffers here, device buffers in the
 * _device form (ordered on ctx's stream, completed before return). */
int sift_rgba_to_gray(struct sift_ctx *ctx, const uint8_t *rgba, int width, int height, size_t stride_bytes,
                      float *gray, float *alpha);
int sift_rgba_to_gray_device(struct sift_ctx *ctx, const uint8_t *d_rgba, int width, int height,
                             size_t stride_bytes, float *d_gray, float *d_alpha);

/* sift_build_scale_space / sift_detect from an RGBA ImageData (host): the
 * RGBA bytes are uploaded and converted on device (no host gray pass). */
int sift_build_scale_space_rgba(struct sift_ctx *ctx, const uint8_t *rgba, int width, int height,
                                size_t stride_bytes, const sift_params *p, const double *offset_sigmas);
int sift_detect_rgba(struct sift_ctx *ctx, const uint8_t *rgba, int width, int height, size_t stride_bytes,
                     const sift_params *p, sift_keypoint *out, size_t cap, size_t *n_out);

/* Preview ImageData of one plane of the context's pyramid, as the reference
 * posts them to its UI: ImageUtils_convertMatrix2DToImageData with a gray
 * channel (image-utils.js:171-217): p = Math.round(g * 255) stored as
 * (p, p, p, 255) with Uint8ClampedArray clamping, where g is
 *   SIFT_DISPLAY_PLAIN    the plane value (Gaussian images, background.js:139, :218)
 *   SIFT_DISPLAY_SIGMOID  1/(1+exp(coefficient*(-1*v))) (Matrix2D_sigmoidNormalize,
 *                         matrix2d.js:151; DoG chunks use 5, background.js:303)
 *   SIFT_DISPLAY_SAMPLED  (v-min)/(max-min) over the plane (Matrix2D_sampledNormalize,
 *                         matrix2d.js:169; DoG images, background.js:336, :387)
 * computed in fp64 from the fp32 plane.  The sampled mode's min and max are
 * the reference's scan: it starts at min = Number.MAX_SAFE_INTEGER = 2^53 - 1
 * and max = Number.MIN_SAFE_INTEGER = -(2^53 - 1) and moves them with strict
 * `value < min` / `value > max`, so NaNs never win, a plane with no value
 * below 2^53 - 1 keeps that minimum and one with none above -(2^53 - 1) that
 * maximum (a constant plane of 1e30 is white, not 0 / 0).  The plain and
 * sampled bytes equal the reference's for any plane, these included.  `rgba`
 * holds rows*cols*4 bytes (cap_bytes); host memory, or device memory in the
 * _device form (4-byte aligned; 16-byte aligned takes 16-byte stores). */
enum { SIFT_DISPLAY_PLAIN = 0, SIFT_DISPLAY_SIGMOID = 1, SIFT_DISPLAY_SAMPLED = 2 };
int sift_plane_image(struct sift_ctx *ctx, int kind, int octave, int scale, int mode, double coefficient,
                     uint8_t *rgba, size_t cap_bytes);
int sift_plane_image_device(struct sift_ctx *ctx, int kind, int octave, int scale, int mode,
                            double coefficient, uint8_t *d_rgba, size_t cap_bytes);

/* Device-resident forms for a shard driver that keeps everything on the GPU
 * (ABI version >= 4): the origins of sift_keypoint_origins decoded on
 * device into caller device memory (4 int32 per keypoint), and rows
 * [row_begin, row_end) of the octave-(num_octaves) base into caller device
 * memory.  Both complete before return. */
int sift_copy_keypoint_origins_device(struct sift_ctx *ctx, int32_t *d_dst, size_t cap, size_t *n_out);
int sift_copy_next_seed_device(struct sift_ctx *ctx, double *d_dst, size_t cap, int row_begin, int row_end);

/* ---- Orientation assignment and descriptors -------------------------------
 *
 * The reference stops at refinement (readme.md:11); these two stages follow
 * Rey-Otero & Delbracio, "Anatomy of the SIFT Method" (IPOL 2014), algorithms
 * 11 and 12, in fp64 on the context's fp32 Gaussian planes, in octave-local
 * pixel units (x = abs_x / 2^(octave-1), likewise y and sigma; plane =
 * SIFT_PLANE_GAUSS (octave, scale_level)).  Results are bit-identical from
 * run to run.  SIFT_ABI_VERSION stayed 9: a caller detects these entry points
 * by symbol (dlsym / hasattr), not by version.  The constants are fixed;
 * there is no setter. */
#define SIFT_ORI_LAMBDA 1.5      /* Gaussian window sigma = lambda * sigma; box radius 3 * that */
#define SIFT_ORI_BINS 36
#define SIFT_ORI_SMOOTH 6        /* circular (1,1,1)/3 passes over the histogram */
#define SIFT_ORI_PEAK_RATIO 0.8
#define SIFT_ORI_MAX_PEAKS 18    /* strict circular maxima of 36 bins */
#define SIFT_DESC_LAMBDA 6.0     /* Gaussian window sigma = lambda * sigma; cells are 3 sigma wide */
#define SIFT_DESC_CELLS 4        /* 4 x 4 cells */
#define SIFT_DESC_ORI 8          /* orientation bins per cell */
#define SIFT_DESC_CAP 0.2        /* clamp at cap * norm, then renormalise */
#define SIFT_DESC_BYTES 128      /* byte (i*4 + j)*8 + k: cell row i, cell column j, bin k */

/* One reference orientation of keypoint `keypoint` (its index in the list
 * sift_copy_keypoints returns): the histogram peak in bin `bin`, interpolated
 * to theta in [0, 2 pi).  Records are in keypoint order, then ascending bin;
 * a keypoint whose 3 * lambda * sigma box leaves [1, w-2] x [1, h-2] has none. */
typedef struct {
  int32_t keypoint;
  int32_t bin;
  double theta;
} sift_orientation; /* 16 bytes */

/* Orientations of the keypoints of the last refinement / detection.  Records
 * stay on the device when out == NULL (*n_out still returned).
 * SIFT_E_CAPACITY: *n_out = required count, nothing written.  SIFT_E_STATE:
 * no refinement yet, or the Gaussian planes were not materialised
 * (SIFT_F_SKIP_GAUSS_PLANES, sift_load_dog).  SIFT_E_UNSUPPORTED: a batch, a
 * row origin or owned rows set, or a seed-range detection whose leading
 * octaves have no planes. */
int sift_orient(struct sift_ctx *ctx, sift_orientation *out, size_t cap, size_t *n_out);

/* One 128-byte descriptor per record of the last sift_orient (SIFT_E_STATE
 * without one).  A record whose descriptor box leaves [1, w-2] x [1, h-2] is
 * not described: 128 zero bytes, described[r] = 0 (else 1).  desc == NULL
 * keeps the results on the device; `described` may be NULL; cap is in
 * records.  *n_out = records, *n_described = described records. */
int sift_describe(struct sift_ctx *ctx, uint8_t *desc, uint8_t *described, size_t cap, size_t *n_out,
                  size_t *n_described);

/* Device pointers of the last sift_orient + sift_describe results (n records;
 * valid until the next orient / describe / build / detect). */
int sift_device_features(struct sift_ctx *ctx, const sift_orientation **d_ori, const uint8_t **d_desc,
                         const uint8_t **d_described, size_t *n);

/* Device time of the last sift_orient (histograms, scan, emission) and
 * sift_describe, milliseconds. */
int sift_last_feature_timings(struct sift_ctx *ctx, double *orient_ms, double *describe_ms);

/* Use caller-supplied keypoints for the stages that follow (sift_orient,
 * sift_describe, sift_copy_keypoints), as sift_set_candidates does for the
 * refinement; detected by symbol like the entry points above.  Needs a
 * single-image pyramid with materialised Gaussian planes and no row origin or
 * owned rows (else SIFT_E_STATE / SIFT_E_UNSUPPORTED as sift_orient returns
 * them); no refinement is needed.  Each record's octave must have planes and
 * its scale_level lie in [0, scales_per_octave + 3), and n must be below
 * 2^31 - 1: else SIFT_E_ARG and the previous list stays.  Coordinates and
 * sigma are taken as they are: a keypoint whose box is not inside its plane
 * (NaN, infinite, non-positive sigma included) simply has no record.  Drops
 * the orientations and descriptors of the previous list, and resets what the
 * replaced refinement left behind rather than serving it stale: the singular
 * count and refine_ms read 0, sift_last_block_counts reports no blocks and the
 * keypoint origins return SIFT_E_STATE until the next refinement. */
int sift_set_keypoints(struct sift_ctx *ctx, const sift_keypoint *kp, size_t n);

/* Use caller-supplied orientation records (in the caller's order) for the next
 * sift_describe; sift_orient afterwards copies them back without recomputing.
 * Needs keypoints (a refinement or sift_set_keypoints).  Every record must
 * have 0 <= keypoint < the keypoint count, 0 <= bin < SIFT_ORI_BINS and a
 * finite theta in [0, 2 pi): else SIFT_E_ARG and the previous records stay.
 * Drops the descriptors of the previous records. */
int sift_set_orientations(struct sift_ctx *ctx, const sift_orientation *rec, size_t n);

/* ---- Brute-force descriptor matching ---------------------------------------
 *
 * Descriptors are rows of SIFT_DESC_BYTES (128) uint8.  For query row q and
 * train row t the squared L2 distance is d2(q, t) = sum_k (Q[q][k] - T[t][k])^2,
 * an integer in [0, 128 * 255^2 = 8323200].  A row may be masked out by a
 * `described`-style byte array (0 = the row does not take part; sift_describe
 * writes zero bytes for undescribed rows); a NULL mask means every row takes
 * part.  For every query row the stage returns the two smallest (d2, t) pairs
 * over the unmasked train rows in lexicographic order (d2, then train index):
 * among equal distances the lowest index wins, and `second` may be at the same
 * distance as `best`.  A missing neighbour has index -1 and d2 =
 * SIFT_MATCH_NONE_D2: both for a masked query row or no unmasked train row,
 * `second` alone for exactly one unmasked train row.  The arithmetic is
 * integer (int8 matrix cores): results are exact and do not depend on how the
 * work is split.  Like the feature stages, these entry points are detected by
 * symbol; SIFT_ABI_VERSION stayed 9. */
struct sift_match {
  int32_t best, second, d2_best, d2_second;
}; /* 16 bytes; a struct tag, as stat(2)'s: C has one namespace for typedefs and functions, and the
      host entry point below is sift_match too */
#define SIFT_MATCH_NONE_D2 INT32_MAX

/* One accepted pair of the selection below. */
typedef struct {
  int32_t query, train, d2, d2_second;
} sift_match_pair; /* 16 bytes */

/* Everything in device memory of ctx's device: n_query x 128 and n_train x 128
 * descriptor bytes (16-byte aligned), their masks (n bytes each, or NULL) and
 * d_out for n_query records.  Ordered on ctx's stream, complete on return.
 * Counts must be below 2^31 - 1 and pointers non-NULL for non-zero counts, else
 * SIFT_E_ARG with nothing written; a zero count is valid (n_train == 0: every
 * neighbour missing). */
int sift_match_device(struct sift_ctx *ctx, const uint8_t *d_query, const uint8_t *d_query_mask, size_t n_query,
                      const uint8_t *d_train, const uint8_t *d_train_mask, size_t n_train, struct sift_match *d_out);
/* The same with host buffers, through the context's own device buffers. */
int sift_match(struct sift_ctx *ctx, const uint8_t *query, const uint8_t *query_mask, size_t n_query,
               const uint8_t *train, const uint8_t *train_mask, size_t n_train, struct sift_match *out);

/* Query = the last sift_describe of ctx, train = that of train_ctx on the same
 * device (it may be ctx itself); the masks are their `described` arrays.  The
 * records stay on the device when out == NULL (*n_out still returned;
 * sift_device_matches).  SIFT_E_STATE without a describe on either side;
 * SIFT_E_CAPACITY: *n_out = required count, nothing written. */
int sift_match_features(struct sift_ctx *ctx, struct sift_ctx *train_ctx, struct sift_match *out, size_t cap, size_t *n_out);

/* Device pointer of the last sift_match / sift_match_features records of ctx
 * (valid until its next match). */
int sift_device_matches(struct sift_ctx *ctx, const struct sift_match **d_match, size_t *n);

/* The ordered, compacted list of accepted pairs of d_fwd (n_query records of a
 * query -> train match), ascending query index.  Query q is accepted when
 *   best >= 0, and
 *   ratio <= 0 (no ratio test), or second < 0, or
 *     (double)d2_best < (ratio * ratio) * (double)d2_second   (fp64, no contraction), and
 *   d_rev == NULL, or best < n_train and d_rev[best].best == q   (d_rev: the
 *     n_train records of the swapped, train -> query match: a mutual check).
 * ratio must be finite and < 1, or <= 0: else SIFT_E_ARG.  *n_out = accepted
 * pairs; d_pairs == NULL only counts; SIFT_E_CAPACITY when cap < *n_out, nothing
 * written.  Device memory of ctx's device; complete on return.  _host: the
 * same with host arrays. */
int sift_match_select(struct sift_ctx *ctx, const struct sift_match *d_fwd, size_t n_query, const struct sift_match *d_rev,
                      size_t n_train, double ratio, sift_match_pair *d_pairs, size_t cap, size_t *n_out);
int sift_match_select_host(struct sift_ctx *ctx, const struct sift_match *fwd, size_t n_query, const struct sift_match *rev,
                           size_t n_train, double ratio, sift_match_pair *pairs, size_t cap, size_t *n_out);

/* Device time of the last match (row preparation, match, split merge) and of
 * the last selection (flags, scan, count read-back, and the emission when pairs
 * were written), milliseconds. */
int sift_last_match_timings(struct sift_ctx *ctx, double *match_ms, double *select_ms);

/* ---- RANSAC homography verification of match pairs ------------------------
 *
 * A homography fitted to the putative pairs of the selection above, on the
 * device and bit-identical from run to run.  The definition uses only + - * /
 * and comparisons in fp64 with no contraction (no fused multiply-add) and no
 * sqrt, so that a plain restatement reproduces it bit for bit.  Like the stages
 * above, these entry points are detected by symbol; SIFT_ABI_VERSION stayed 9.
 *
 * Model: H is row-major h[0..8] and maps query to train: (u, v, w) = H (x, y, 1),
 * the image point is (u/w, v/w).
 *
 * Hypothesis k (0 <= k < K) for seed s (uint64) over n >= 4 pairs:
 *  1. Four distinct indices.  For draw i = 0..3:
 *       z = mix(s + (4 k + i + 1) * 0x9E3779B97F4A7C15)            (mod 2^64),
 *       mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *               0x94D049BB133111EB; z ^ (z >> 31)    (splitmix64's output mixer),
 *       r = ((z >> 32) * (n - i)) >> 32,
 *       then for every earlier chosen index c in ascending order: if (r >= c) r++.
 *     No rejection loop; the sample keeps draw order.
 *  2. The 8 x 9 system in the unknowns h[0..7], h[8] = 1.  Sample j with
 *     (x, y) -> (X, Y) gives
 *       row 2j   = [x, y, 1, 0, 0, 0, -X*x, -X*y | X],
 *       row 2j+1 = [0, 0, 0, x, y, 1, -Y*x, -Y*y | Y].
 *  3. Gaussian elimination with partial pivoting.  For column c = 0..7 the pivot
 *     row is the row r >= c of largest |A[r][c]| (p = c; a later row replaces it
 *     only when strictly larger, so a NaN never does), lowest r among equals.  A
 *     pivot that is zero or not finite makes the hypothesis invalid.  Swap the
 *     rows; for each r > c: f = A[r][c] / A[c][c], and for j = c+1..8:
 *     A[r][j] = A[r][j] - f * A[c][j].  Back substitution for c = 7..0:
 *     t = A[c][8]; for j = c+1..7 ascending: t = t - A[c][j] * h[j]; h[c] = t /
 *     A[c][c].  A non-finite h makes the hypothesis invalid.
 *     An invalid hypothesis has H = nine zeros and count -1.
 *  4. No coordinate normalisation.
 *
 * Inlier rule for a pair (x, y) -> (X, Y), a matrix h and t2 = thresh * thresh
 * (formed once on the host):
 *       u = (h0*x + h1*y) + h2, v = (h3*x + h4*y) + h5, w = (h6*x + h7*y) + h8,
 *       du = u - X*w, dv = v - Y*w,
 *       inlier iff w > 0 && (du*du + dv*dv) < t2 * (w*w).
 * No division; a NaN in a point or a coefficient compares false, so that pair
 * is never an inlier.
 *
 * Result: the count of a valid hypothesis is its number of inliers over all n
 * pairs; the best hypothesis has the largest count, lowest k among equals; the
 * inlier list holds the pair indices of the best hypothesis in ascending order.
 * If n < 4, K == 0 or every hypothesis is invalid the result is hypothesis = -1,
 * inliers = 0, nine zeros and an empty list, and the call is valid (with n < 4
 * or K == 0 no hypothesis is formed: sift_copy_homography_hypotheses gives 0).
 *
 * Limits: K <= SIFT_RANSAC_MAX_HYPOTHESES, n < 2^31 - 1, thresh finite and > 0,
 * pointers non-NULL where a count is non-zero: else SIFT_E_ARG, nothing written.
 *
 * Not here: symmetric transfer error, adaptive termination, fundamental or
 * essential matrices.  The least-squares refit over the inliers follows below. */
#define SIFT_RANSAC_MAX_HYPOTHESES 65536

/* A point of the query image and its putative partner in the train image, in
 * absolute input-pixel units (abs_x, abs_y of sift_keypoint). */
typedef struct {
  double qx, qy, tx, ty;
} sift_point_pair; /* 32 bytes */

typedef struct {
  double h[9];
  int32_t hypothesis; /* index k of the best hypothesis, -1: none */
  int32_t inliers;    /* its count */
} sift_homography; /* 80 bytes */

/* d_points[i] = the keypoint positions behind d_pairs[i] (n records of
 * sift_match_select): `query` / `train` index the orientation records of ctx /
 * train_ctx (the rows sift_match_features matched), whose `keypoint` indexes the
 * keypoint list.  An index outside its list gives four NaNs (such a pair is
 * never an inlier).  Device memory of ctx's device; complete on return.
 * SIFT_E_STATE without a sift_orient on either side. */
int sift_pair_points_device(struct sift_ctx *ctx, struct sift_ctx *train_ctx, const sift_match_pair *d_pairs, size_t n,
                            sift_point_pair *d_points);

/* RANSAC over n device point pairs: K hypotheses for `seed`, scored at `thresh`
 * (input pixels).  *model (host memory) receives the best hypothesis, *n_inliers
 * its count; d_inliers (device memory, cap indices) the inlier list, or NULL to
 * only count.  SIFT_E_CAPACITY when cap < *n_inliers: *model and *n_inliers are
 * set, the list is not written.  Complete on return. */
int sift_homography_ransac_device(struct sift_ctx *ctx, const sift_point_pair *d_points, size_t n, size_t K,
                                  uint64_t seed, double thresh, sift_homography *model, int32_t *d_inliers, size_t cap,
                                  size_t *n_inliers);
/* The same with host points and a host inlier list, through the context's own device buffers. */
int sift_homography_ransac(struct sift_ctx *ctx, const sift_point_pair *points, size_t n, size_t K, uint64_t seed,
                           double thresh, sift_homography *model, int32_t *inliers, size_t cap, size_t *n_inliers);

/* counts[k] = the inliers among the n pairs of the caller's matrix H[9 k ..
 * 9 k + 8] (k < K, h[8] as given), by the inlier rule alone.  Host arrays;
 * _device: device arrays, complete on return. */
int sift_homography_score(struct sift_ctx *ctx, const sift_point_pair *points, size_t n, const double *H, size_t K,
                          double thresh, int32_t *counts);
int sift_homography_score_device(struct sift_ctx *ctx, const sift_point_pair *d_points, size_t n, const double *d_H,
                                 size_t K, double thresh, int32_t *d_counts);

/* Every hypothesis (9 doubles each) and count (-1: invalid) of the last RANSAC
 * on ctx, into host memory; cap in hypotheses; either array may be NULL.
 * SIFT_E_STATE without one; SIFT_E_CAPACITY: *n_out = required count. */
int sift_copy_homography_hypotheses(struct sift_ctx *ctx, double *H, int32_t *counts, size_t cap, size_t *n_out);

/* Host pairs in (the output of sift_match_select_host between ctx and
 * train_ctx), point gather plus RANSAC on the device, host results out:
 * sift_pair_points_device followed by sift_homography_ransac. */
int sift_verify_features(struct sift_ctx *ctx, struct sift_ctx *train_ctx, const sift_match_pair *pairs, size_t n,
                         size_t K, uint64_t seed, double thresh, sift_homography *model, int32_t *inliers, size_t cap,
                         size_t *n_inliers);

/* Device time of the last RANSAC's stages, milliseconds: the hypotheses, their
 * scoring (sift_homography_score* sets this one alone), and the selection (best
 * hypothesis, flags, scan, count read-back, and the emission when written). */
int sift_last_verify_timings(struct sift_ctx *ctx, double *hypotheses_ms, double *score_ms, double *select_ms);

/* ---- Least-squares refit of the RANSAC inliers -------------------------------
 *
 * The best RANSAC model interpolates four noisy pairs; the refit fits a
 * homography to all of its inliers, rescores, and repeats while the inlier
 * count grows.  Like the stage above it uses only + - * /, comparisons and
 * negation in fp64 with no contraction, no sqrt and no library function, and it
 * is bit-identical from run to run: the one floating-point sum over a
 * data-dependent list is taken in a fixed tree (step 3).  These entry points
 * are detected by symbol; SIFT_ABI_VERSION stayed 9.
 *
 * Fit of a list I of m >= 4 pair indices (each < n; repeats are legal).  The
 * list order is the summation order; the refit passes ascending indices.
 *  1. Box normalisation, per image side.  Over the listed pairs lo_x, hi_x,
 *     lo_y, hi_y are the smallest and largest query coordinate that is not a
 *     NaN (a NaN when there is none); a bound that is a zero is taken as +0
 *     (lo = lo + 0.0).  Then
 *       cx = (lo_x + hi_x) * 0.5, cy = (lo_y + hi_y) * 0.5,
 *       w = hi_x - lo_x, g = hi_y - lo_y, dq = (g > w ? g : w) * 0.5.
 *     The train side gives cX, cY, dt in the same way.  The fit is invalid unless
 *     dq > 0 && dt > 0 and both are finite.  Normalised coordinates are
 *     x' = (x - cx) / dq, y' = (y - cy) / dq, X' = (X - cX) / dt, Y' = (Y - cY) / dt.
 *     Minimum and maximum are exact and do not depend on the order: this is why
 *     the normalisation uses the box and not a mean distance.
 *  2. Normal equations.  With the normalised point (written x, y, X, Y), the
 *     rows of RANSAC step 2:
 *       a = [x, y, 1, 0, 0, 0, -(X*x), -(X*y) | X],
 *       b = [0, 0, 0, x, y, 1, -(Y*x), -(Y*y) | Y].
 *     For 0 <= j <= k <= 8, j <= 7 (44 sums, in this row-major order) the term of
 *     pair i is t_i = a_j*a_k + b_j*b_k: both products rounded, then added, the
 *     zeros and ones multiplied like every other entry.  N[j][k] = N[k][j] = the
 *     sum of t_i, g[j] = N[j][8].
 *  3. Summation order: a fixed tree that depends on m alone.  The terms, in list
 *     order, are split into chunks of 64, the last one padded with +0.0.  A
 *     chunk's sum is the halving tree: for s = 32, 16, 8, 4, 2, 1: p[i] = p[i] +
 *     p[i + s] for i < s; the sum is p[0].  The ceil(m / 64) chunk sums are
 *     reduced by the same rule, and so on until one value is left (a single
 *     chunk sum is the result as it is).
 *  4. [N | g] is solved for h'[0..7] by exactly the elimination and back
 *     substitution of RANSAC step 3, pivot rule included; a zero or non-finite
 *     pivot or a non-finite h' makes the fit invalid.
 *  5. Denormalisation.  With Hn = [h'0 .. h'7, 1] row-major, for r = 0, 1, 2:
 *       G[r][0] = Hn[r][0] / dq, G[r][1] = Hn[r][1] / dq,
 *       G[r][2] = Hn[r][2] - (Hn[r][0]*cx + Hn[r][1]*cy) / dq;
 *     for c = 0, 1, 2:
 *       F[0][c] = dt*G[0][c] + cX*G[2][c], F[1][c] = dt*G[1][c] + cY*G[2][c],
 *       F[2][c] = G[2][c];
 *     h = F / F[2][2] element by element, so h[8] is exactly 1.  The fit is
 *     invalid if F[2][2] is zero or not finite, or if any h is not finite.
 *  An invalid fit gives nine zeros.  A list of fewer than four entries is an
 *  invalid fit that forms no box and no sums.
 *
 * Refit of a starting model H0 (any nine doubles, h[8] as given) over n pairs at
 * `thresh` with at most R = max_rounds rounds.  I_0 = the inliers of H0 by the
 * inlier rule above, ascending, c_0 = |I_0|.  Round r = 1 .. R:
 *   if c_{r-1} < 4, stop.  Fit I_{r-1}; if the fit is invalid, stop.  Apply the
 *   inlier rule to all n pairs: I_r, c_r.  If c_r < c_{r-1}, discard the round
 *   and stop.  Otherwise accept it, and stop after accepting if c_r == c_{r-1}
 *   or r == R.
 * The result is the last accepted matrix, its count, its ascending inlier list
 * and the number of accepted rounds; with none accepted it is H0 unchanged with
 * I_0.  The host compares integers only.  R == 0, n == 0 and a "none" model (all
 * zeros, so no inliers) are valid calls.
 *
 * Limits: 0 <= R <= SIFT_REFIT_MAX_ROUNDS, n < 2^31 - 1 (and m < 2^31 - 1),
 * thresh finite and > 0, pointers non-NULL where a count is non-zero, every
 * entry of a host list < n: else SIFT_E_ARG, nothing written.  A device list
 * cannot be checked on the host: an entry outside [0, n) is not read through,
 * and makes the fit invalid. */
#define SIFT_REFIT_MAX_ROUNDS 16

/* One fit of the list d_index[0 .. m) over n device point pairs; d_index == NULL
 * means the list 0 .. n-1 (m is not read).  h (host memory, nine doubles) and
 * *valid (1 / 0; may be NULL) receive the result; m < 4 is an invalid fit and
 * SIFT_OK.  Complete on return. */
int sift_homography_fit_device(struct sift_ctx *ctx, const sift_point_pair *d_points, size_t n, const int32_t *d_index,
                               size_t m, double *h, int *valid);
/* The same with host points and a host list, through the context's own device buffers. */
int sift_homography_fit(struct sift_ctx *ctx, const sift_point_pair *points, size_t n, const int32_t *index, size_t m,
                        double *h, int *valid);

/* box = cx, cy, dq, cX, cY, dt and the 44 sums (step 2's order) of the last fit
 * on ctx -- by the two calls above, or the last round a refit tried -- valid or
 * not; either array may be NULL.  SIFT_E_STATE without a fit, or after one of
 * fewer than four entries.  The fit keeps its own state: a RANSAC or a scoring
 * on ctx leaves these values as they are. */
int sift_copy_homography_fit_sums(struct sift_ctx *ctx, double *box, double *sums);

/* The refit of *start over n device point pairs.  *refined (host memory; it may
 * be start) receives the matrix and the count, with `hypothesis` copied from
 * *start; *rounds the accepted rounds; *n_inliers the count; d_inliers (device
 * memory, cap indices) the inlier list, or NULL to only count.
 * SIFT_E_CAPACITY when cap < *n_inliers: everything but the list is set.
 * rounds and n_inliers may be NULL.  Complete on return; the RANSAC state of ctx
 * (sift_copy_homography_hypotheses) is left as it is. */
int sift_homography_refit_device(struct sift_ctx *ctx, const sift_point_pair *d_points, size_t n,
                                 const sift_homography *start, double thresh, int max_rounds, sift_homography *refined,
                                 int32_t *rounds, int32_t *d_inliers, size_t cap, size_t *n_inliers);
/* The same with host points and a host inlier list. */
int sift_homography_refit(struct sift_ctx *ctx, const sift_point_pair *points, size_t n, const sift_homography *start,
                          double thresh, int max_rounds, sift_homography *refined, int32_t *rounds, int32_t *inliers,
                          size_t cap, size_t *n_inliers);

/* sift_verify_features followed by the refit of its model, on the points already
 * gathered on the device: host pairs in, host results out. */
int sift_verify_features_refit(struct sift_ctx *ctx, struct sift_ctx *train_ctx, const sift_match_pair *pairs, size_t n,
                               size_t K, uint64_t seed, double thresh, int max_rounds, sift_homography *model,
                               int32_t *rounds, int32_t *inliers, size_t cap, size_t *n_inliers);

/* Device time of the last refit, milliseconds, summed over the rounds it tried
 * (a discarded one included): the fits (box, sums, solve) and the rescoring
 * (flags, scan, read-back, emission).  Both 0 when no round was tried. */
int sift_last_refit_timings(struct sift_ctx *ctx, double *fit_ms, double *rescore_ms);

/* ---- Homography warp ----------------------------------------------------------
 *
 * The product at the far end of the path: an image resampled through a
 * homography, gray (fp32) or RGBA (4 x uint8).  Like the stages above it is
 * defined with + - * /, comparisons and floor in fp64 with no contraction and no
 * other library function, and it is bit-identical from run to run.  These entry
 * points are detected by symbol; SIFT_ABI_VERSION stayed 9.
 *
 * Inverse of h (row-major).  The adjugate a, term by term:
 *   a[0] = h4*h8 - h5*h7, a[1] = h2*h7 - h1*h8, a[2] = h1*h5 - h2*h4,
 *   a[3] = h5*h6 - h3*h8, a[4] = h0*h8 - h2*h6, a[5] = h2*h3 - h0*h5,
 *   a[6] = h3*h7 - h4*h6, a[7] = h1*h6 - h0*h7, a[8] = h0*h4 - h1*h3;
 *   d = (h0*a[0] + h1*a[3]) + h2*a[6];  out[i] = a[i] / d.
 * When d is zero or not finite, or any out[i] is not finite, there is no inverse:
 * nine zeros (the "none" model above, all zeros, is such a case).  It is the true
 * inverse, not the adjugate: the sign of the third row survives a mirroring h
 * (det < 0), and the rule below tests w > 0.
 *
 * The warp takes m[9], which maps a DESTINATION pixel to a SOURCE position; it
 * inverts nothing.  To bring the query image into the train frame, pass the
 * inverse of the model's h.  The matrix is not validated: NaN, infinite and huge
 * entries are defined by the rule (no pixel valid, or few).
 *
 * Per destination pixel (X, Y), 0 <= X < dst_w, 0 <= Y < dst_h as doubles, and a
 * source of sw x sh pixels p (pixel centres at integer coordinates, as abs_x and
 * abs_y of sift_keypoint are; pixel values converted to fp64):
 *   u = (m0*X + m1*Y) + m2, v = (m3*X + m4*Y) + m5, w = (m6*X + m7*Y) + m8;
 *   r = 1.0 / w, sx = u * r, sy = v * r                      (one division);
 *   valid iff w > 0 && sx >= 0 && sy >= 0 && sx <= sw-1 && sy <= sh-1
 *     (any NaN compares false; the test precedes every cast to an integer, and
 *     an invalid pixel reads nothing);
 *   x0 = min(floor(sx), max(sw-2, 0)), x1 = min(x0+1, sw-1), fx = sx - x0,
 *   gx = 1.0 - fx;  y0, y1, fy, gy likewise from sy and sh;
 *   top = p(y0,x0)*gx + p(y0,x1)*fx,  bot = p(y1,x0)*gx + p(y1,x1)*fx,
 *   val = top*gy + bot*fy            (every product rounded, then added).
 * The clamp of x0 makes sx == sw-1 legal, with fx = 1; a source one pixel wide
 * gives x0 = x1 = 0 and fx = 0.
 *  Gray: dst = (float)val, rounded once.  RGBA: each of the four channels is
 *  interpolated on its byte values, dst = floor(val + 0.5); val lies in
 *  [0, 255], so nothing clamps.  An invalid pixel receives the caller's fill:
 *  a float, bits as given, or four bytes.
 *  SIFT_WARP_NEAREST: xn = floor(sx + 0.5), yn = floor(sy + 0.5) under the same
 *  validity test and dst = p(yn, xn) unchanged, for masks and label images.
 *  Mask (optional): one byte per destination pixel, dense (dst_w * dst_h), 1 for
 *  a valid pixel and 0 for an invalid one.  *n_valid (optional): the number of
 *  valid pixels, an integer sum.
 * With m the identity or an integer translation gx or fx is exactly 0 or 1, and a
 * source without negative zeros or non-finite values comes back byte for byte
 * where it is valid.  A -0.0 comes back as +0.0 and inf * 0 is a NaN.
 *
 * Limits: ctx, source, destination, matrix (and the RGBA fill) non-NULL, every
 * dimension > 0, width * height < 2^31 on either side, strides >= the width, an
 * RGBA stride a multiple of 4, RGBA device images 4-byte aligned, a mode named
 * below, and a destination that is not the source (they must not overlap): else
 * SIFT_E_ARG, nothing written. */
enum { SIFT_WARP_NEAREST = 0, SIFT_WARP_BILINEAR = 1 };

/* Host math, no context.  SIFT_E_ARG with nine zeros in out when h has no
 * inverse (above), or when h is NULL. */
int sift_homography_inverse(const double h[9], double out[9]);

/* Device images, strides in pixels; m in host memory.  d_mask (device, dense) and
 * n_valid (host) may be NULL.  Ordered on ctx's stream and complete on return;
 * nothing is copied but the count, and not that when n_valid is NULL. */
int sift_warp_gray_device(struct sift_ctx *ctx, const float *d_src, int src_w, int src_h, size_t src_stride_px,
                          const double m[9], int mode, float fill, float *d_dst, int dst_w, int dst_h,
                          size_t dst_stride_px, uint8_t *d_mask, size_t *n_valid);
/* The same with host images, through the context's own device buffers; only the
 * dst_w pixels of each destination row are written.  A buffer that is dense and
 * page-locked (sift_host_register) moves in one DMA. */
int sift_warp_gray(struct sift_ctx *ctx, const float *src, int src_w, int src_h, size_t src_stride_px,
                   const double m[9], int mode, float fill, float *dst, int dst_w, int dst_h, size_t dst_stride_px,
                   uint8_t *mask, size_t *n_valid);
/* RGBA: four bytes per pixel, strides in bytes, fill = four bytes. */
int sift_warp_rgba_device(struct sift_ctx *ctx, const uint8_t *d_src, int src_w, int src_h, size_t src_stride_bytes,
                          const double m[9], int mode, const uint8_t fill[4], uint8_t *d_dst, int dst_w, int dst_h,
                          size_t dst_stride_bytes, uint8_t *d_mask, size_t *n_valid);
int sift_warp_rgba(struct sift_ctx *ctx, const uint8_t *src, int src_w, int src_h, size_t src_stride_bytes,
                   const double m[9], int mode, const uint8_t fill[4], uint8_t *dst, int dst_w, int dst_h,
                   size_t dst_stride_bytes, uint8_t *mask, size_t *n_valid);

/* Device time of the last warp's kernel on ctx, milliseconds. */
int sift_last_warp_timing(struct sift_ctx *ctx, double *warp_ms);

/* ---- Keypoint budget -------------------------------------------------------------
 *
 * The N strongest keypoints of a list, overall or per cell of a square grid over
 * the input, chosen on the device.  The definition uses integers alone (one fp64
 * division and a floor place a record in its cell), so it is exact, does not
 * depend on how the work is split, and is bit-identical from run to run.  The
 * list keeps its order: nothing is sorted by strength.  These entry points are
 * detected by symbol; SIFT_ABI_VERSION stayed 9.
 *
 * Strength key of record i: the 64 bits of interp_value with the sign bit
 * cleared, read as an unsigned integer; a NaN has key 0.  For everything that is
 * not a NaN this orders by |interp_value|: inf is the strongest; +0.0, -0.0 and
 * NaN are the weakest and equal to each other.  Record i PRECEDES record j when
 * key_i > key_j, or when key_i == key_j && i < j.
 *
 * Cell of record i, when cell_px > 0: ncx = ceil(width / cell_px), ncy =
 * ceil(height / cell_px); t = abs_x / (double)cell_px;
 *   ix = t >= 0 ? (t < ncx ? (int)floor(t) : ncx - 1) : 0
 * (the test comes before the cast; a NaN or a negative coordinate goes to column
 * 0); iy likewise from abs_y and ncy; cell = iy * ncx + ix.
 *
 * Selection, in two steps:
 *  1. If cell_px > 0 && max_per_cell >= 0, record i survives when fewer than
 *     max_per_cell records of its cell precede it.  Otherwise every record
 *     survives.
 *  2. If max_total >= 0, a survivor is kept when fewer than max_total SURVIVORS
 *     precede it.  Otherwise every survivor is kept.
 * The result is the ascending list of the kept indices.
 *
 * Limits: n < 2^31 - 1, reserved == 0, cell_px >= 0; with cell_px > 0, width > 0
 * and height > 0; pointers non-NULL where a count is non-zero: else SIFT_E_ARG.
 * With cell_px > 0, ncx * ncy <= SIFT_BUDGET_MAX_CELLS: else SIFT_E_UNSUPPORTED.
 * In both cases nothing is written.
 *
 * Not here: radius-based suppression, budgets per octave, budgets for a batch or
 * for sharded lists, output ordered by strength. */
typedef struct {
  int32_t max_total;     /* < 0: no overall limit */
  int32_t cell_px;       /* 0: no grid; > 0: square cells of cell_px input pixels */
  int32_t max_per_cell;  /* < 0: no per-cell limit; read only when cell_px > 0 */
  int32_t reserved;      /* must be 0 */
} sift_budget;           /* 16 bytes */
#define SIFT_BUDGET_MAX_CELLS 16384

/* The selection over n device records of a width x height input: *n_out = the
 * kept count, d_index (device memory, cap indices) the ascending list, or NULL
 * to only count.  SIFT_E_CAPACITY when cap < *n_out, nothing written.  Any device
 * array of sift_keypoint will do; of the context only scratch and the timing
 * change.  Ordered on ctx's stream, complete on return. */
int sift_keypoint_select_device(struct sift_ctx *ctx, const sift_keypoint *d_kp, size_t n, int width, int height,
                                const sift_budget *budget, int32_t *d_index, size_t cap, size_t *n_out);
/* The same with host arrays, through the context's own device buffers. */
int sift_keypoint_select(struct sift_ctx *ctx, const sift_keypoint *kp, size_t n, int width, int height,
                         const sift_budget *budget, int32_t *index, size_t cap, size_t *n_out);

/* The selection applied to the context's keypoint list in place, with the
 * pyramid's input size as width and height: the kept records are gathered in
 * order into a second buffer, which becomes the list (*n_out = its count; a
 * pointer that sift_device_keypoints gave before is no longer the list).
 * Needs a settled keypoint list (a refinement, a detection or
 * sift_set_keypoints: else SIFT_E_STATE) but no Gaussian planes;
 * SIFT_E_UNSUPPORTED for a batch, a row origin or owned rows, as sift_orient.
 * Drops the orientations and descriptors; sift_last_block_counts reports no
 * blocks and the keypoint origins return SIFT_E_STATE afterwards, as after
 * sift_set_keypoints.  The singular count and refine_ms stay: they remain true
 * of the detection.  A second call selects from the already limited list. */
int sift_limit_keypoints(struct sift_ctx *ctx, const sift_budget *budget, size_t *n_out);

/* The indices into the previous list that the last sift_limit_keypoints kept
 * (host memory; index == NULL only counts; SIFT_E_CAPACITY: *n_out = required
 * count).  SIFT_E_STATE when there was no such call, or after a new refinement,
 * detection or sift_set_keypoints. */
int sift_copy_keypoint_selection(struct sift_ctx *ctx, int32_t *index, size_t cap, size_t *n_out);

/* Device time of the last selection on ctx through any of the forms above,
 * milliseconds: the keys, the narrowing passes, the flags, the scan, the count
 * read-back and the emission. */
int sift_last_select_timing(struct sift_ctx *ctx, double *select_ms);

/* ---- Guided descriptor matching ---------------------------------------------------
 *
 * The descriptor match restricted by a homography: for every query row, the
 * nearest and second-nearest descriptor among the train rows whose position lies
 * within `radius` input pixels of the projection H x of the query row's position.
 * The result is a lexicographic minimum of integer keys over a set that the
 * rules below fix, so it is exact, does not depend on the grid or on how the work
 * is split, and is bit-identical from run to run.  It is written as struct
 * sift_match records: sift_match_select, sift_pair_points_device, the RANSAC and
 * the refit follow unchanged.  These entry points are detected by symbol;
 * SIFT_ABI_VERSION stayed 10.
 *
 * Inputs: query and train rows of SIFT_DESC_BYTES uint8 (16-byte aligned in
 * device memory), optional byte masks as in sift_match, one sift_point per row,
 * h[9] row-major mapping query positions to train positions (as the RANSAC's;
 * not validated), radius (finite, > 0, input pixels), and train_width,
 * train_height > 0, which only shape the grid: train points outside the image
 * take part like any other.  All arithmetic is fp64 without contraction, + - * /,
 * comparisons and floor alone.
 *
 * Projection of query row q at (x, y), by the warp's rule:
 *   u = (h0*x + h1*y) + h2, v = (h3*x + h4*y) + h5, w = (h6*x + h7*y) + h8,
 *   rinv = 1.0 / w, px = u * rinv, py = v * rinv.
 * The row is PROJECTED iff it is unmasked, w > 0, and px and py are finite
 * (px - px == 0.0 and py - py == 0.0); a NaN anywhere compares false.
 *
 * Candidates, with r2 = radius * radius formed once on the host: train row t at
 * (tx, ty) is a candidate of a projected row q iff t is unmasked and
 *   (dx*dx + dy*dy) <= r2,  dx = tx - px, dy = ty - py
 * (each product rounded, then added).  A NaN train coordinate never passes.
 *
 * Result, per query row: the two smallest (d2, t) over its candidates in
 * lexicographic order, d2 the integer squared distance of sift_match: the lowest
 * train index wins among equal distances, and `second` may be at the distance of
 * `best`.  A missing neighbour is (-1, SIFT_MATCH_NONE_D2) exactly as in
 * sift_match: both for a masked or unprojected row and for a row without a
 * candidate, `second` alone for a row with exactly one.
 *
 * Grid.  It is internal and changes no record; it is stated because n_visited
 * below is defined by it.  cell_px is the smallest integer
 *   c >= max(1, min(ceil(radius), max(train_width, train_height)))
 * with ceil(W / c) * ceil(H / c) <= SIFT_GUIDED_MAX_CELLS; ncx = ceil(W / c), ncy =
 * ceil(H / c).  The column of a coordinate a is the budget's clamped rule:
 *   t = a / (double)c;  col(a) = t >= 0 ? (t < ncx ? (int)floor(t) : ncx - 1) : 0
 * (the test comes before the cast); rows likewise with ncy.  An unmasked train
 * row with two non-NaN coordinates is filed in cell (row(ty), col(tx)).  A
 * projected query row VISITS the train rows filed in columns
 * col(px - radius) - 1 .. col(px + radius) + 1 and rows row(py - radius) - 1 ..
 * row(py + radius) + 1, both clamped to the grid.  The margin of one cell is
 * there because the rounded distance test can admit a point a few ulp beyond
 * radius and col is only monotone; DESIGN.md section 18 proves that every
 * candidate is visited, for huge and overflowing coordinates and radii too.
 *
 * Limits: counts below 2^31 - 1; pointers non-NULL where a count is non-zero, h
 * non-NULL; device descriptors 16-byte aligned; radius finite and > 0;
 * train_width > 0 and train_height > 0: else SIFT_E_ARG with nothing written.
 * n_query == 0 and n_train == 0 are valid (no train rows: every neighbour
 * missing).
 *
 * Not here: gates on scale or orientation, a fundamental-matrix or epipolar band,
 * a symmetric both-ways call, batches.  A mutual check is done the existing way:
 * run the guided match again with the two sets swapped and the matrix of
 * sift_homography_inverse, and pass its records as d_rev to sift_match_select. */
typedef struct {
  double x, y;
} sift_point; /* 16 bytes */
#define SIFT_GUIDED_MAX_CELLS (1 << 20)
typedef struct {
  int32_t cell_px, ncx, ncy, reserved; /* the grid; reserved is 0 */
  int64_t n_projected;                 /* projected query rows */
  int64_t n_visited;                   /* sum over projected rows of visited train rows */
  int64_t n_candidates;                /* sum over projected rows of candidates */
} sift_guided_info;                    /* 40 bytes */

/* Everything in device memory of ctx's device but h; d_out for n_query records.
 * Ordered on ctx's stream, complete on return.  Writes d_out alone: the context's
 * last match (sift_device_matches) stays what it was. */
int sift_match_guided_device(struct sift_ctx *ctx, const uint8_t *d_query, const uint8_t *d_query_mask,
                             const sift_point *d_query_xy, size_t n_query, const uint8_t *d_train,
                             const uint8_t *d_train_mask, const sift_point *d_train_xy, size_t n_train, int train_width,
                             int train_height, const double h[9], double radius, struct sift_match *d_out);
/* The same with host arrays, through the context's own device buffers; the
 * records become the context's last match, as sift_match's. */
int sift_match_guided(struct sift_ctx *ctx, const uint8_t *query, const uint8_t *query_mask, const sift_point *query_xy,
                      size_t n_query, const uint8_t *train, const uint8_t *train_mask, const sift_point *train_xy,
                      size_t n_train, int train_width, int train_height, const double h[9], double radius,
                      struct sift_match *out);

/* Query = the last sift_describe of ctx, train = that of train_ctx on the same
 * device, rows and masks exactly as sift_match_features; a row's position is
 * abs_x, abs_y of the keypoint its orientation record names (the gather of
 * sift_pair_points_device), and the train size is train_ctx's input size.  The
 * records become ctx's last match and stay on the device when out == NULL.
 * SIFT_E_STATE without a describe on either side, SIFT_E_ARG across devices,
 * SIFT_E_CAPACITY as sift_match_features. */
int sift_match_features_guided(struct sift_ctx *ctx, struct sift_ctx *train_ctx, const double h[9], double radius,
                               struct sift_match *out, size_t cap, size_t *n_out);

/* The grid and the three sums of the last guided match on ctx through any form
 * (SIFT_E_STATE without one), and its device time in milliseconds: the filing
 * (cells, scan, fill) and the match. */
int sift_last_guided_info(struct sift_ctx *ctx, sift_guided_info *out);
int sift_last_guided_timings(struct sift_ctx *ctx, double *grid_ms, double *match_ms);

/* Wait for all work queued on ctx's stream. */
int sift_synchronize(struct sift_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* SIFT_HIP_H */
