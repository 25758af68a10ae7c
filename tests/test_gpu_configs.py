"""Parity at BASELINE.json's full configurations, on the GPU.

* cfg 3 -- 3840x2160, 4 octaves x 5 scales (the configuration the bench's
  metric is quoted on): the whole path against the CPU oracle, both in its
  separable form and in the reference's own 2D-kernel summation order
  (sift.js:72-149); identical candidate lists and order, identical
  low-contrast counts, identical keypoint lists and order with (x, y, sigma)
  within 1e-4.
* cfg 5 geometry -- 6 octaves x 5 scales: octave 4/5 radii (94 / 188) exceed
  the plane height at 8K (and at 960x540, the cheap stand-in); the generic-
  radius path with its wide LDS strip against the oracle; and the 8K image
  itself, whole against the 8-shard device-resident row-band run, bit for bit,
  and against the oracle.

The oracle runs on the GPU box's host cores (OpenMP; its results do not
depend on the thread count).  The reference semantics matched here are
background.js:71-237 (Gaussian scale space), :258-354 (DoG), :359-450 +
sift.js:212-316 (extrema), background.js:455-685 (refinement).
"""
import time

import numpy as np
import pytest

import oracle as orc
import sift_amd
from parity_util import as_keypoints, check_candidates, check_keypoints, host_threads, oracle_params
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu


def ctx_octaves(p):
    return p.num_octaves


def _vs_oracle(ctx, img, p, mode, low_rtol=0.0):
    """low_rtol == 0: the low-contrast list (F_LOW_CONTRAST_LIST) must equal
    the oracle's too (positions exact, values within fp32 rounding)."""
    t0 = time.perf_counter()
    p = sift_amd.make_params(p.num_octaves, p.scales_per_octave, p.min_blur, p.assumed_blur,
                             p.min_interpixel_distance, p.flags | sift_amd.F_LOW_CONTRAST_LIST)
    kp = ctx.detect(img, p).copy()
    cand = ctx.candidates()
    counts = ctx.counts()
    low = ctx.low_contrast()
    t1 = time.perf_counter()
    r = orc.OracleRun(img, oracle_params(p), mode, threads=host_threads(), keep_gauss=False)
    t2 = time.perf_counter()
    print("\n%dx%d O%d S%d: GPU %.2f s, oracle (%s, %d threads) %.1f s: %d candidates, %d keypoints, %d low, "
          "%d exact fp64 re-decisions"
          % (img.shape[1], img.shape[0], p.num_octaves, p.scales_per_octave, t1 - t0,
             {orc.CONV_2D: "2D", orc.CONV_SEPARABLE: "separable"}.get(mode, "gpu order"), host_threads(), t2 - t1,
             cand.shape[0], kp.shape[0],
             r.n_low, counts["exact"]))
    if kp.shape[0] == r.refined.shape[0]:
        got = np.stack([kp["abs_sigma"], kp["abs_x"], kp["abs_y"]], 1)
        print("max |d(sigma, x, y)| = %.3g, max |d interp_value| = %.3g" % (
            float(np.abs(got - r.refined[:, 4:7]).max(initial=0.0)),
            float(np.abs(kp["interp_value"] - r.refined[:, 7]).max(initial=0.0))))
    check_candidates(cand, r.candidates())
    check_keypoints(kp, r.refined)
    assert low.shape[0] == counts["low_contrast"]
    if low_rtol > 0.0:  # report the low-contrast set difference (positions)
        def pos(a):
            return set(map(tuple, np.asarray(a).tolist()))
        g = pos(np.stack([low["octave"], low["scale"], low["x"], low["y"]], 1))
        rl = r.low_contrast()
        o_ = pos(rl[:, :4].astype(np.int64))
        print("low-contrast: GPU %d, oracle %d, only GPU %d, only oracle %d (per octave %s / %s)" % (
            len(g), len(o_), len(g - o_), len(o_ - g),
            np.bincount([t[0] for t in g - o_], minlength=ctx_octaves(p)).tolist(),
            np.bincount([t[0] for t in o_ - g], minlength=ctx_octaves(p)).tolist()))
    assert abs(counts["low_contrast"] - r.n_low) <= low_rtol * r.n_low, (counts["low_contrast"], r.n_low)
    if low_rtol == 0.0:
        check_candidates(low, r.low_contrast())
    assert counts["singular"] == r.n_singular == 0
    return kp, r


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", [orc.CONV_SEPARABLE, orc.CONV_2D], ids=["separable", "reference_2d"])
def test_cfg3_4k_o4_s5_matches_oracle(gpu_ctx, mode):
    """The metric's configuration (BASELINE cfg 3), the bench's own image."""
    img = blob_image(3840, 2160, seed=42)
    kp, _ = _vs_oracle(gpu_ctx, img, sift_amd.make_params(4, 5), mode)
    assert kp.shape[0] > 400000


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", [orc.CONV_SEPARABLE, orc.CONV_2D], ids=["separable", "reference_2d"])
def test_cfg5_radii_960x540_o6_s5_matches_oracle(gpu_ctx, mode):
    """6 octaves x 5 scales: octave-4/5 radii 94 and 188, as at 8K, exceed
    their planes (68 and 34 rows here): clamped generic-radius passes."""
    img = blob_image(960, 540, seed=5)
    p = sift_amd.make_params(6, 5)
    from sift_amd.shard import octave_radii
    rad = octave_radii(p)
    assert max(rad[4]) == 94 and max(rad[5]) == 188
    dims = sift_amd.octave_dims(960, 540, 6)
    assert max(rad[5]) > dims[5][0] and max(rad[4]) > dims[4][0]
    _vs_oracle(gpu_ctx, img, p, mode)


@pytest.fixture(scope="module")
def img8k():
    return blob_image(7680, 4320, seed=8)


@pytest.mark.timeout(600)
def test_cfg5_8k_o6_s5_whole_vs_8_row_band_shards(gpu_ctx, img8k):
    """BASELINE cfg 5 geometry: the 8-shard device-resident row-band run
    (crops for octaves 0..K, the gathered base for the tail, ordered merge)
    equals the whole-image run bit for bit."""
    import torch
    from sift_amd.shard import detect_sharded_device_local
    p = sift_amd.make_params(6, 5)
    whole = gpu_ctx.detect(img8k, p).copy()
    d_img = torch.from_numpy(img8k).to("cuda:0")
    merged, plan = detect_sharded_device_local(gpu_ctx, d_img, p, 8)
    got = as_keypoints(merged)
    print("\n8K O6 S5: %d keypoints, plan %s" % (whole.shape[0], plan))
    assert len(plan.bands) == 8 and plan.has_tail
    assert got.shape == whole.shape
    assert got.tobytes() == whole.tobytes()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", [orc.CONV_SEPARABLE, orc.CONV_SEPARABLE_FMA_VH, orc.CONV_2D],
                         ids=["separable", "gpu_order", "reference_2d"])
def test_cfg5_8k_o6_s5_matches_oracle(gpu_ctx, img8k, mode):
    """The whole 8K image against the oracle.  Candidates and keypoints must
    be identical in all three summation orders, the reference's own 2D-kernel
    order (sift.js:96-128) included.  The low-contrast list is exact against
    the oracle in the HIP path's own operation order (columns then rows, fma
    chains); against the rows-first and the 2D order its count may differ by
    a few of ~435 K -- low-contrast extrema in flat regions whose 26
    neighbours tie to the last fp64 bit, which each summation order breaks its
    own way -- and the test prints the set difference per octave."""
    kp, _ = _vs_oracle(gpu_ctx, img8k, sift_amd.make_params(6, 5), mode,
                       low_rtol=0.0 if mode == orc.CONV_SEPARABLE_FMA_VH else 1e-5)
    assert kp.shape[0] > 1000000


@pytest.mark.timeout(600)
@pytest.mark.parametrize("W,H,O,S,seed", [(640, 480, 5, 5, 3), (333, 517, 4, 3, 4), (1920, 1080, 4, 5, 42),
                                         (3840, 2160, 4, 5, 42), (1280, 720, 3, 3, 5)])
def test_planes_bit_exact_in_gpu_order(gpu_ctx, W, H, O, S, seed):
    """Every Gaussian and DoG plane is the fp32 rounding of the oracle's fp64
    value computed in the HIP path's operation order, bit for bit."""
    img = blob_image(W, H, seed=seed)
    p = sift_amd.make_params(O, S)
    gpu_ctx.build_scale_space(img, p)
    r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE_FMA_VH, threads=host_threads())
    for o, (h, w) in enumerate(r.dims):
        for s in range(S + 3):
            np.testing.assert_array_equal(gpu_ctx.plane(sift_amd.PLANE_GAUSS, o, s), r.gauss[o][s].astype(np.float32))
        for s in range(S + 2):
            np.testing.assert_array_equal(gpu_ctx.plane(sift_amd.PLANE_DOG, o, s), r.dog[o][s].astype(np.float32))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("W,H", [(1920, 1080), (160, 120)], ids=["1920x1080", "160x120"])
def test_pass_kernels_record(gpu_ctx, W, H):
    """sift_last_pass_kernels names each octave's launches (bench.py's
    roofline.kernel): O4 S5 runs octave 0's staged tile kernel, octave 1
    (radii <= 12) the register-window kernel, octave 2 (radii <= 24) the
    streamed one and octave 3 (radius 47) the split vertical pass + tiles.
    Radii depend on octave and scale only, so 160x120 (octave 3: 40x30) takes
    the same launches; there octave 3's planes are also checked against the
    oracle in the HIP path's operation order, bit for bit."""
    p = sift_amd.make_params(4, 5)
    img = blob_image(W, H, seed=3)
    gpu_ctx.build_scale_space(img, p)
    parts = dict(e.split(": ", 1) for e in gpu_ctx.pass_kernels().split("; "))
    assert sorted(parts) == ["o0", "o1", "o2", "o3"], parts
    assert parts["o0"].startswith("k_gauss_dog<octave0"), parts
    assert parts["o1"] == "k_gauss_rw<12>", parts
    assert parts["o2"] == "k_gauss_rw<24,true>", parts
    assert parts["o3"] == "k_gauss_vert + k_gauss_dog<64>", parts
    if (W, H) == (160, 120):
        from sift_amd.shard import octave_radii
        assert max(octave_radii(p)[3]) == 47
        r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE_FMA_VH, threads=host_threads())
        assert tuple(r.dims[3]) == (30, 40)
        for s in range(p.scales_per_octave + 3):
            np.testing.assert_array_equal(gpu_ctx.plane(sift_amd.PLANE_GAUSS, 3, s), r.gauss[3][s].astype(np.float32))
        for s in range(p.scales_per_octave + 2):
            np.testing.assert_array_equal(gpu_ctx.plane(sift_amd.PLANE_DOG, 3, s), r.dog[3][s].astype(np.float32))


_SPLIT = "k_gauss_vert + k_gauss_dog<64>"
_PASS_PATHS = [
    # (O, S, min_blur), largest radius per octave, launches per octave
    ((4, 5, 0.8), [6, 12, 23, 47],
     ["k_gauss_dog<octave0>", "k_gauss_rw<12>", "k_gauss_rw<24,true>", _SPLIT]),
    ((5, 3, 0.8), [7, 14, 29, 58, 116],
     ["k_gauss_dog<octave0>", "k_gauss_rw<16,true>", "k_gauss_dog<64>", _SPLIT, _SPLIT]),
    ((4, 2, 0.8), [9, 19, 37, 74],
     ["k_gauss_dog<octave0>", "k_gauss_rw<24,true>", "k_gauss_dog<64>", _SPLIT]),
    ((3, 3, 2.5), [24, 45, 90],
     ["k_upsample_base + k_gauss_dog<octave0,fp64 base>", _SPLIT, _SPLIT]),
]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("params,rmax,kernels", _PASS_PATHS, ids=["O4S5", "O5S3", "O4S2", "O3S3mb2.5"])
def test_pass_kernels_every_path(gpu_ctx, params, rmax, kernels):
    """One 160x120 image per launch path of the Gaussian pass: octave 0 staged
    with either strip stride (largest radius <= 8, 9..16) or on the
    materialised fp64 base (> 16); octaves >= 1 through the register window
    (<= 12), the streamed window (13..24, RW 16 and 24), the 64-column tiles
    (25..39) and the split vertical pass + tiles (>= 40; >= 90 also keeps the
    fp64 planes).  The radii are asserted so that a schedule change cannot
    move a case onto another path; every Gaussian and DoG plane equals the
    oracle's in the HIP path's operation order, bit for bit."""
    from sift_amd.shard import octave_radii
    p = sift_amd.make_params(*params)
    assert [max(r) for r in octave_radii(p)] == rmax
    img = blob_image(160, 120, seed=3)
    gpu_ctx.build_scale_space(img, p)
    parts = dict(e.split(": ", 1) for e in gpu_ctx.pass_kernels().split("; "))
    assert parts == {"o%d" % o: k for o, k in enumerate(kernels)}, parts
    r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE_FMA_VH, threads=host_threads())
    S = p.scales_per_octave
    for o in range(p.num_octaves):
        for s in range(S + 3):
            np.testing.assert_array_equal(gpu_ctx.plane(sift_amd.PLANE_GAUSS, o, s), r.gauss[o][s].astype(np.float32),
                                          err_msg="gauss o%d s%d" % (o, s))
        for s in range(S + 2):
            np.testing.assert_array_equal(gpu_ctx.plane(sift_amd.PLANE_DOG, o, s), r.dog[o][s].astype(np.float32),
                                          err_msg="dog o%d s%d" % (o, s))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("W,H,O,S,seed", [(3840, 2160, 4, 5, 42), (333, 517, 4, 3, 4), (64, 48, 3, 3, 5)])
def test_fused_extrema_flag_same_results(gpu_ctx, W, H, O, S, seed):
    """SIFT_F_FUSED_EXTREMA (octave 0's decisions inside its Gaussian pass):
    candidates, low-contrast count and keypoints identical to the scan."""
    img = blob_image(W, H, seed=seed)
    a = gpu_ctx.detect(img, sift_amd.make_params(O, S)).copy()
    ca, na = gpu_ctx.candidates(), gpu_ctx.counts()
    b = gpu_ctx.detect(img, sift_amd.make_params(O, S, flags=sift_amd.F_FUSED_EXTREMA)).copy()
    cb, nb = gpu_ctx.candidates(), gpu_ctx.counts()
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    assert na["low_contrast"] == nb["low_contrast"] and na["candidates"] == nb["candidates"]


def test_fused_extrema_exact_keys_on_saturated_image(gpu_ctx):
    """k_exact_extrema in key mode, list positions from the bitmap geometry,
    with real work: fused octave-0 decisions list ambiguous pixel keys, and in
    that one launch octave 0 has 60-column words from column 1 while octaves
    1 and 2 have 62-column words from column 0.  The saturated image (clipped
    share 0.486) has 2,544 input pixels whose 15x15 neighbourhood is constant;
    each gives 4 octave-0 pixels x 3 scales of exactly-zero DoG: 30,528
    guaranteed fp32 ties, all interior.  The plain detection runs first: it
    grows the ambiguous-key capacity past the tie count, so the fused run does
    not overflow and fall back to the unfused retry."""
    W, H, O, S = 200, 150, 3, 3
    img = blob_image(W, H, seed=1)
    img = (np.clip(np.rint((img - 0.5) * 3.0 * 4096 + 2048), 0, 4096) / 4096).astype(np.float32)
    assert (img == 0).mean() + (img == 1).mean() > 0.4
    a = gpu_ctx.detect(img, sift_amd.make_params(O, S)).copy()
    ca, na = gpu_ctx.candidates(), gpu_ctx.counts()
    p = sift_amd.make_params(O, S, flags=sift_amd.F_FUSED_EXTREMA)
    b = gpu_ctx.detect(img, p).copy()
    cb, nb = gpu_ctx.candidates(), gpu_ctx.counts()
    print("\nsaturated %dx%d O%d S%d: %d candidates, %d keypoints, exact re-decisions plain %d, fused %d"
          % (W, H, O, S, ca.shape[0], a.shape[0], na["exact"], nb["exact"]))
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    assert na["exact"] == nb["exact"]
    assert na["exact"] >= 10000 and nb["exact"] >= 10000  # a third of the derived minimum: not a vacuous run
    r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE_FMA_VH, threads=host_threads())
    check_candidates(cb, r.candidates())
    check_keypoints(b, r.refined)


@pytest.mark.timeout(300)
def test_capacity_growth_on_dense_extrema():
    """A fresh context starts from a geometry estimate of its candidate,
    ambiguous-key and low-contrast capacities; a noisy 3-pixel
    dot lattice image has more extrema than that estimate (1 per 9 input
    pixels at every scale), so the extrema stage overflows, grows and runs again (the
    retry path), and the results still equal the oracle's in the HIP path's
    operation order.  A second detection on the grown context runs without
    a retry and gives the same bytes."""
    rng = np.random.default_rng(5)
    H, W = 960, 1280
    y, x = np.mgrid[0:H, 0:W]
    img = (0.5 + 0.4 * ((x % 3 == 1) & (y % 3 == 1)) + 0.01 * rng.random((H, W))).astype(np.float32)
    ctx = sift_amd.Context(0)
    try:
        p = sift_amd.make_params(3, 3, flags=sift_amd.F_LOW_CONTRAST_LIST)
        kp = ctx.detect(img, p).copy()
        cand, low, counts = ctx.candidates(), ctx.low_contrast(), ctx.counts()
        r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE_FMA_VH, threads=host_threads())
        print("\ndot lattice 1280x960 O3 S3: %d candidates, %d low, %d keypoints, %d exact re-decisions"
              % (cand.shape[0], low.shape[0], kp.shape[0], counts["exact"]))
        assert cand.shape[0] > 3 * 6451200 // 192  # above the initial estimate: the retry ran
        check_candidates(cand, r.candidates())
        check_candidates(low, r.low_contrast())
        check_keypoints(kp, r.refined)
        again = ctx.detect(img, p).copy()
        assert again.tobytes() == kp.tobytes()
    finally:
        ctx.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("W,H,O,S,gain", [(1920, 1080, 4, 5, 2.0), (640, 480, 6, 3, 3.0)])
def test_saturated_image_exact_words(gpu_ctx, W, H, O, S, gain):
    """Clipped (saturated) regions make whole rows of flat DoG values tie in
    fp32: every such pixel is ambiguous, and the scan lists whole ambiguous
    words that k_exact_words re-decides in fp64 (62 pixels per wave).  The
    candidates, the low-contrast list and the keypoints must equal the
    oracle's in the HIP path's operation order, and the ambiguous pixels must
    be many (the case this path is for).  640x480 O6: octaves 4 and 5 keep
    their fp64 planes (radii above 90): the l64 branch."""
    img = blob_image(W, H, seed=1)
    img = (np.clip(np.rint((img - 0.5) * gain * 4096 + 2048), 0, 4096) / 4096).astype(np.float32)
    assert (img == 0).mean() + (img == 1).mean() > 0.02
    p = sift_amd.make_params(O, S, flags=sift_amd.F_LOW_CONTRAST_LIST)
    kp = gpu_ctx.detect(img, p).copy()
    cand, low, counts = gpu_ctx.candidates(), gpu_ctx.low_contrast(), gpu_ctx.counts()
    r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE_FMA_VH, threads=host_threads())
    print("\nsaturated %dx%d O%d S%d: %d candidates, %d low, %d keypoints, %d exact re-decisions"
          % (W, H, O, S, cand.shape[0], low.shape[0], kp.shape[0], counts["exact"]))
    assert counts["exact"] > 10000
    check_candidates(cand, r.candidates())
    check_candidates(low, r.low_contrast())
    check_keypoints(kp, r.refined)
    assert counts["low_contrast"] == r.n_low
