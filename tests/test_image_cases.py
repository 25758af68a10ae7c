"""The image products' case tables (image_cases.py) held to the reference and
to the numpy restatement, and shown able to fail (CPU).

Every table equals the fixture tests/golden/image_products.npz (outputs of
the reference's own functions, tests/golden/make_image_golden.py) where the
fixture holds its inputs, and the restatement oracle/image_products.py
everywhere.  For every table a named wrong kernel, modelled in numpy, gives
at least one other byte, so that the GPU test of the same table
(test_gpu_image_edges.py) is not vacuous.

The sampled normalisation's scan starts at +-(2^53 - 1)
(matrix2d.js:174-175).  A scan started at +-inf -- the restatement and the
kernel as they stood before they were put right, image_cases.
wrong_sampled_inf_start -- differs from the reference on the planes of
EXTREMES_INF_START_WRONG (test_inf_start_scan_is_rejected) and on no others.

Round-half-even in place of Math.round cannot be told apart in the plain
mode by any fp32 input: the only tie there is 0.5 * 255 = 127.5 (see
image_cases), which both take to 128.  The ramps of the sampled mode put 255
values on ties and reject it.
"""
import os
import re

import numpy as np
import pytest

import image_cases as ic
import image_products as ip

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "sift-scale-space-extrema-detection_amd", "csrc", "sift_image.hip")
FORMS = ((0, "plain"), (1, "sigmoid"), (2, "sampled"))


def _img(v, mode, c=1.0):
    return ip.plane_image(np.asarray(v).reshape(1, -1), mode, c).reshape(-1, 4)


# ---- the fixture holds the tables' inputs ----------------------------------
def test_fixture_holds_the_tables():
    g = ic.gold()
    assert g["s_in"].tobytes() == ic.sigmoid_input().tobytes()
    assert g["s_coefs"].tobytes() == np.array(ic.SIGMOID_COEFS).tobytes()
    ramp = np.concatenate([[0.0], np.arange(1.0, 510.0, 2.0), [510.0]]).astype(np.float32)
    assert g["x_ramp"].tobytes() == ramp.tobytes()
    assert g["x_ramp_shift"].tobytes() == (ramp + 1000).tobytes()
    assert g["x_ramp_scale"].tobytes() == (ramp * np.float32(2.0 ** -10)).tobytes()
    for name in ic.EXTREMES + ic.RAMPS:
        v, forms = ic.fixture_plane(name)
        assert v.dtype == np.float32 and all(f.shape == (v.size, 4) for f in forms.values()), name
    # the planes the extreme table is about: no value at or below 2^53 - 1, or none at or above -(2^53 - 1)
    for name in ic.EXTREMES:
        v = ic.fixture_plane(name)[0].astype(np.float64)
        v = v[~np.isnan(v)]
        keeps = v.size > 0 and (not (v <= ip.MAX_SAFE_INTEGER).any() or not (v >= -ip.MAX_SAFE_INTEGER).any())
        assert keeps == (name in ic.EXTREMES_KEEP_START), name
    assert set(ic.EXTREMES_INF_START_WRONG) < set(ic.EXTREMES_KEEP_START)
    p53 = ic.fixture_plane("p53_mixed")[0]
    for nb in (np.nextafter(np.float32(2.0 ** 53), np.float32(0)), np.nextafter(np.float32(2.0 ** 53), np.float32(np.inf))):
        assert nb in p53 and -nb in p53


# ---- sampled mode: the start values of the scan ------------------------------
@pytest.mark.parametrize("mode,form", FORMS)
@pytest.mark.parametrize("name", ic.EXTREMES + ic.RAMPS)
def test_restatement_equals_reference_on_extreme_planes(name, mode, form):
    v, forms = ic.fixture_plane(name)
    np.testing.assert_array_equal(_img(v, mode, float(ic.gold()["coef"])), forms[form])


@pytest.mark.parametrize("name", ic.EXTREMES + ic.RAMPS)
def test_fixture_planes_keep_the_sigmoid_off_ties(name):
    """The GPU test compares the sigmoid form of these planes too (coefficient
    5, V8's exp in the fixture): the condition of test_sigmoid_table."""
    d, exact = ic.sigmoid_tie_distance(ic.fixture_plane(name)[0], float(ic.gold()["coef"]))
    assert (d[~exact] >= ic.TIE_MARGIN).all()


def test_reference_bytes_of_the_planes_above_2_53():
    """The reference's own bytes, as a reader can check them by hand."""
    want = {"big_const": [255] * 4, "big_pos": [127, 255, 191, 127], "big_neg": [128, 0, 64, 128],
            "e16": [12, 255, 134, 12], "all_nan": [0] * 4, "p53_const": [255] * 4}
    for name, b in want.items():
        np.testing.assert_array_equal(ic.fixture_plane(name)[1]["sampled"][:, 0], b, err_msg=name)


def test_inf_start_scan_is_rejected():
    """Wrong kernel: min / max started at +-inf.  It differs from the
    reference on the planes that keep a start value and have a range small
    enough for it to show (EXTREMES_INF_START_WRONG), and on no others."""
    differs = []
    for name in ic.EXTREMES:
        v, forms = ic.fixture_plane(name)
        got = ic.as_image(ic.display_bytes(ic.wrong_sampled_inf_start(v)))
        if not np.array_equal(got, forms["sampled"]):
            differs.append(name)
    assert tuple(differs) == ic.EXTREMES_INF_START_WRONG


# ---- gray: the whole cube -----------------------------------------------------
def test_gray_cube():
    g = ic.gold()
    gray, alpha = ic.cube_expected()
    rgba = ic.cube_rgba()
    assert rgba.shape == (ic.CUBE_SIDE, ic.CUBE_SIDE, 4)
    flat = rgba.reshape(-1, 4)
    idx = flat[:, 0].astype(np.int64) | (flat[:, 1].astype(np.int64) << 8) | (flat[:, 2].astype(np.int64) << 16)
    assert np.array_equal(idx, np.arange(1 << 24))                       # every (R, G, B), once
    assert np.array_equal(np.unique(flat[:: 257, 3]), np.arange(256))     # every alpha
    # the restatement on the image itself
    rg, ra = ip.rgba_to_gray(rgba)
    assert np.array_equal(rg.astype(np.float32), gray) and np.array_equal(ra.astype(np.float32), alpha)
    # the reference's pixels, looked up in the table
    px = g["rgba"].reshape(-1, 4).astype(np.int64)
    at = px[:, 0] | (px[:, 1] << 8) | (px[:, 2] << 16)
    np.testing.assert_array_equal(gray.ravel()[at], g["gray"].ravel().astype(np.float32))
    np.testing.assert_array_equal((px[:, 3] / 255.0).astype(np.float32), g["alpha"].ravel().astype(np.float32))
    # other fp64 evaluations: the same fp32 on the whole domain
    for name, v in ic.cube_gray_variants():
        assert np.array_equal(v.ravel(), gray.ravel()), name
    # wrong kernel: fp32 evaluation (6 476 852 pixels differ)
    n = int((ic.wrong_gray_fp32() != gray).sum())
    assert n == 6476852


# ---- plain mode -------------------------------------------------------------------
def test_plain_specials():
    v = ic.plain_specials()
    assert v.dtype == np.float32 and v.size == 1552
    want = ic.as_image(ic.exact_plain_bytes(v))
    np.testing.assert_array_equal(_img(v, 0), want)
    np.testing.assert_array_equal(ic.gold()["s_plain"].reshape(-1, 4)[:v.size], want)
    np.testing.assert_array_equal(ic.as_image(ic.display_bytes(v)), want)
    # the table reaches every byte and both ends of the clamp
    assert np.array_equal(np.unique(want[:, 0]), np.arange(256))
    # the only tie: 0.5
    t = v.astype(np.float64) * 255.0
    fin = np.isfinite(t)
    ties = v[fin][(t[fin] - np.floor(t[fin]) == 0.5) & (t[fin] > 0) & (t[fin] < 255)]
    assert set(ties.tolist()) == {0.5}
    # wrong kernels
    assert (ic.display_bytes(v, store="wrap") != want[:, 0]).sum() >= 2      # 256/255, 300, 3e38
    assert (ic.display_bytes(v, nan_byte=255) != want[:, 0]).sum() == 1      # NaN
    assert np.array_equal(ic.display_bytes(v, rounding="even"), want[:, 0])  # see the module docstring
    # a rounding that moves any (k + 0.5) / 255 neighbour across its boundary
    assert (ic.display_bytes(np.nextafter(v, np.float32(np.inf))) != want[:, 0]).sum() >= 256


# ---- sampled mode: ties --------------------------------------------------------------
@pytest.mark.parametrize("name", ic.RAMPS)
def test_ramp_ties(name):
    v, forms = ic.fixture_plane(name)
    want = forms["sampled"]
    t = ic.sampled(v) * 255.0
    assert v.size == 257 and int((t - np.floor(t) == 0.5).sum()) == 255   # every odd value sits on k + 0.5
    np.testing.assert_array_equal(ic.as_image(ic.display_bytes(ic.sampled(v))), want)
    np.testing.assert_array_equal(want[:, 0], np.concatenate([[0], np.arange(1, 256), [255]]))
    # wrong kernels: multiplying by 1 / range (23 bytes on the ramp), round-half-even (every even k + 0.5)
    n = int((ic.display_bytes(ic.sampled(v, reciprocal=True)) != want[:, 0]).sum())
    assert n == 23
    assert (ic.display_bytes(ic.sampled(v), rounding="even") != want[:, 0]).sum() >= 127


# ---- sampled mode: where the minimum and the maximum sit ---------------------------------
def test_partial_count_is_the_kernels():
    src = open(SRC).read()
    assert re.search(r"constexpr int kMMThreads = 256;", src)
    assert "(n / 4 + kMMThreads * 8 - 1) / (kMMThreads * 8)" in src and "std::min(1024LL, want)" in src
    for n, p in ((1, 1), (8192, 1), (8195, 1), (8196, 2), (16387, 2), (16388, 3), (8388608, 1024), (4096 * 2050, 1024)):
        assert ic.minmax_parts(n) == p, n
    assert (4096 * 2050 // 4 + 2047) // 2048 > 1024       # the cap is what limits the large plane
    sizes = [int(np.prod(ic.plane_dims(*g))) for g in ic.POSITION_GEOMS]
    assert sizes == ic.POSITION_SIZES
    assert {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 8191, 8192, 8193, 8196, 16383, 16385} < set(sizes)
    assert max(sizes) > 8388608
    for g in ic.POSITION_GEOMS:   # octave 0 planes are even by even
        assert g[2] == 1 or (ic.plane_dims(*g)[0] % 2 == 0 and ic.plane_dims(*g)[1] % 2 == 0)


@pytest.mark.parametrize("n", ic.POSITION_SIZES)
def test_position_planes(n):
    pos = ic.positions(n)
    n4, P = n // 4, ic.minmax_parts(n)
    assert 0 in pos and n - 1 in pos and (n4 * 4 in pos or n % 4 == 0) and (n4 == 0 or n4 * 4 - 1 in pos)
    last = ic.last_partial_mask(n)
    assert last.size == n and last.any()
    if n4:
        lo, hi = 4 * (P - 1) * 256, 4 * min(P * 256, n4) - 1
        assert lo in pos and hi in pos and last[lo] and last[hi] and (lo == 0 or not last[lo - 1])
    tail = np.arange(n) >= 4 * n4
    planes = ic.position_planes(n)
    assert sorted(p[0] for p in planes) == sorted(pos) == sorted(p[1] for p in planes)
    caught = {"tail": 0, "last": 0}
    for imin, imax, v in planes:
        assert v.argmin() == imin and v.argmax() == imax
        assert n == 1 or ((v == v[imin]).sum() == 1 and (v == v[imax]).sum() == 1)
        want = _img(v, 2)[:, 0]
        # wrong kernels: a scan that skips the tail, one that skips the last partial
        for key, skipped in (("tail", tail), ("last", last)):
            if n > 1 and (skipped[imin] or skipped[imax]):   # one pixel is 0 / 0 or NaN, byte 0, whatever the scan
                got = ic.display_bytes(ic.wrong_sampled_inf_start(v, keep=~skipped))
                assert (got != want).any(), (n, key, imin, imax)
                caught[key] += 1
    assert n == 1 or (caught["last"] >= 2 and (caught["tail"] >= 2 or n % 4 == 0)), caught


# ---- sigmoid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(len(ic.SIGMOID_COEFS)))
def test_sigmoid_table(j):
    """numpy's exp, V8's and the device's may differ in the last place.  Every
    input of the table either has an exp that is the same double in all of
    them (argument 0 or within 2^-54 of it, where 1 + a rounds to 1; +-inf;
    NaN) or puts g * 255 at least TIE_MARGIN = 1e-9 from a tie, about 10^4
    times the effect of such a difference: the bytes are then the same, and
    the GPU test compares them with no input left out.  (The reference's
    bytes for the inputs of the first kind are in the fixture like the rest:
    the smallest denormal at coefficient 5 gives exp = 1, g * 255 = 127.5,
    byte 128.)"""
    c = ic.SIGMOID_COEFS[j]
    v = ic.sigmoid_input()
    want = ic.gold()["s_sigmoid_%d" % j].reshape(-1, 4)
    np.testing.assert_array_equal(_img(v, 1, c), want)
    d, exact = ic.sigmoid_tie_distance(v, c)
    assert (d[~exact] >= ic.TIE_MARGIN).all(), (c, v[~exact][d[~exact] < ic.TIE_MARGIN])
    x = v.astype(np.float64)
    if np.isfinite(c) and c != 0:     # the random plane and the grey levels are all of the second kind
        assert (~exact).sum() >= v.size - 9
        # wrong kernel: exp(c * v), the -1 dropped
        assert (_img(v, 1, -c)[:, 0] != want[:, 0]).sum() > v.size // 2
    elif c == 0:                      # g = 1 / (1 + 1) everywhere but at the infinities and NaN (0 * inf)
        assert (want[np.isfinite(x), 0] == 128).all() and (want[~np.isfinite(x), 0] == 0).all()
    elif np.isnan(c):
        assert (want[:, 0] == 0).all()
    else:                             # inf: a step function, NaN at 0
        assert (want[x > 0, 0] == 255).all() and (want[x < 0, 0] == 0).all() and (want[x == 0, 0] == 0).all()
