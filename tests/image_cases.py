"""Case tables of the image products (csrc/sift_image.hip): inputs, and where
they can be stated without the code under test, the expected bytes.

test_image_cases.py (CPU) holds every table to the fixture
tests/golden/image_products.npz (outputs of the reference's own functions) and
to the numpy restatement oracle/image_products.py, and shows for every table a
named wrong kernel, modelled in numpy, that the table rejects.
test_gpu_image_edges.py holds k_rgba_to_gray, k_minmax_partial and
k_plane_image to the tables.  Every comparison is array equality.

Tables
  gray cube     all 2^24 (R, G, B) as one 4096 x 4096 RGBA image, alpha through
                all 256 values: the whole input domain of k_rgba_to_gray.
  specials      plain mode: signed zeros, denormals, infinities, NaN, 0.5 (the
                one fp32 value whose v * 255 is a tie: 255 = 3 * 5 * 17, so
                (2m + 1) / 510 is a binary fraction only for 2m + 1 = 255 and
                its odd multiples, and those lie beyond the clamp), the fp32
                nearest every (k + 0.5) / 255 with two steps either side,
                every k / 255, and the clamp's two ends.  Expected bytes by
                exact rational arithmetic (exact_plain_bytes).
  ramps         sampled mode: 0, 1, 3, ..., 509, 510, whose odd values the
                normalisation puts exactly on k + 0.5, shifted and scaled.
  extremes      sampled mode: the fixture's planes around the scan's start
                values +-(2^53 - 1), infinities and NaNs.
  positions     sampled mode: a unique minimum and maximum at every edge of
                the reduction (float4 body / tail, partial count, last
                partial), for plane sizes either side of every step.
  sigmoid       coefficients 5, 1, 0, -5, 1e308, inf, NaN on the specials and
                a random plane; bytes from the reference (V8's exp).
"""
import functools
import os
from fractions import Fraction

import numpy as np

import image_products as ip

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_products.npz")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------
# Geometry: a plane of n pixels as (W, H, octave) of an input image
# ---------------------------------------------------------------------------
def plane_dims(W, H, octave):
    """(rows, cols) of octave `octave` of a W x H input (sift_octave_dims)."""
    h, w = 2 * H, 2 * W
    for _ in range(octave):
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def geom_for(n):
    """A (W, H, octave) whose plane has n pixels: octave 1 of an n x 1 input
    (its planes, n floats apart, are 16-byte aligned only when n % 4 == 0)."""
    return (int(n), 1, 1)


def pyramid_flat(geom, planes):
    """planes (each rows*cols of geom's octave) as the DoG planes of that
    octave, zeros in the octaves above it: (flat fp32, O, S) for
    sift_load_dog; at least 3 planes (S >= 1), the last repeated."""
    W, H, o = geom
    planes = [np.ascontiguousarray(p, dtype=F32).ravel() for p in planes]
    while len(planes) < 3:
        planes.append(planes[-1])
    nd = len(planes)
    h, w = plane_dims(W, H, o)
    assert all(p.size == h * w for p in planes), (geom, [p.size for p in planes])
    head = [np.zeros(nd * np.prod(plane_dims(W, H, k)), dtype=F32) for k in range(o)]
    return np.concatenate(head + planes), o + 1, nd - 2


# ---------------------------------------------------------------------------
# Gray: the whole cube
# ---------------------------------------------------------------------------
CUBE_SIDE = 4096


@functools.lru_cache(maxsize=None)
def cube_rgba():
    """Pixel i of the 4096 x 4096 image: R = i & 255, G = (i >> 8) & 255,
    B = i >> 16, A = (R + G + B) & 255 (every alpha value, against every R)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    a = np.empty((1 << 24, 4), dtype=np.uint8)
    a[:, 0] = i & 255
    a[:, 1] = (i >> 8) & 255
    a[:, 2] = i >> 16
    a[:, 3] = a[:, 0] + a[:, 1] + a[:, 2]
    a = a.reshape(CUBE_SIDE, CUBE_SIDE, 4)
    a.setflags(write=False)
    return a


def _cube_terms():
    v = np.arange(256, dtype=np.float64)
    return v[None, None, :], v[None, :, None], v[:, None, None]  # R fastest, then G, then B


@functools.lru_cache(maxsize=None)
def cube_expected():
    """(gray, alpha) fp32 4096 x 4096 of cube_rgba(): the reference's formula
    in its order in fp64 (image-utils.js:107, :114), rounded once to fp32.
    This is a table over the whole input domain, not a sample: a kernel that
    equals it converts every possible pixel as the reference does."""
    r, g, b = _cube_terms()
    gray = ((((r * 0.299) + (g * 0.587)) + (b * 0.114)) / 255.0).astype(F32).reshape(CUBE_SIDE, CUBE_SIDE)
    alpha = (cube_rgba()[..., 3].astype(np.float64) / 255.0).astype(F32)
    gray.setflags(write=False)
    alpha.setflags(write=False)
    return gray, alpha


def cube_gray_variants():
    """fp64 evaluations a kernel might choose instead: another association,
    a reciprocal multiply.  Each gives the same fp32 on the whole cube (the
    CPU test asserts it), so the table does not distinguish them and need not."""
    r, g, b = _cube_terms()
    yield "G+B first", (((r * 0.299) + ((g * 0.587) + (b * 0.114))) / 255.0).astype(F32)
    yield "reciprocal", ((((r * 0.299) + (g * 0.587)) + (b * 0.114)) * (1.0 / 255.0)).astype(F32)


def wrong_gray_fp32():
    """Wrong kernel: the formula evaluated in fp32."""
    r, g, b = (t.astype(F32) for t in _cube_terms())
    return ((((r * F32(0.299)) + (g * F32(0.587))) + (b * F32(0.114))) / F32(255.0)).reshape(CUBE_SIDE, CUBE_SIDE)


# ---------------------------------------------------------------------------
# Plain mode specials
# ---------------------------------------------------------------------------
def _steps(v, k):
    """v moved k fp32 steps (k < 0: down)."""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return v


@functools.lru_cache(maxsize=None)
def plain_specials():
    tiny = np.nextafter(F32(0), F32(1), dtype=F32)
    v = [F32(0.0), F32(-0.0), tiny, -tiny, F32(np.inf), F32(-np.inf), F32(np.nan)]
    v += [_steps(0.5, -1), F32(0.5), _steps(0.5, 1)]
    for k in range(256):
        v += [_steps((k + 0.5) / 255.0, d) for d in (-2, -1, 0, 1, 2)]
    v += [F32(k / 255.0) for k in range(256)]
    v += [F32(1.0), _steps(1.0, 1), F32(256.0 / 255.0), F32(-1e-30), F32(300.0), F32(3e38)]
    a = np.array(v, dtype=F32)
    a.setflags(write=False)
    return a


def exact_plain_bytes(v):
    """Math.round(v * 255) through Uint8ClampedArray, in exact rational
    arithmetic (v * 255 is exact in fp64 too: 24 + 8 bits): floor(x + 1/2),
    clamped to [0, 255]; NaN -> 0."""
    out = np.zeros(v.size, dtype=np.uint8)
    for i, x in enumerate(np.asarray(v, dtype=np.float64).ravel()):
        if np.isnan(x):
            p = 0
        elif np.isinf(x):
            p = 255 if x > 0 else 0
        else:
            q = Fraction(x) * 255 + Fraction(1, 2)
            p = min(255, max(0, q.numerator // q.denominator))
        out[i] = p
    return out


def as_image(p):
    """bytes p -> (p, p, p, 255)."""
    p = np.asarray(p, dtype=np.uint8)
    out = np.empty(p.shape + (4,), dtype=np.uint8)
    out[..., 0] = out[..., 1] = out[..., 2] = p
    out[..., 3] = 255
    return out


def display_bytes(g, rounding="js", store="clamp", nan_byte=0):
    """The display conversion of normalised values g (fp64) -- the
    restatement with rounding 'js', store 'clamp', nan_byte 0; the other
    settings are the wrong kernels:
      rounding 'even'  round-half-even (rint) for Math.round;
      store 'wrap'     conversion to an integer cut to its low byte for the clamp;
      nan_byte 255     NaN shown white."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = g * 255.0
        p = np.rint(t) if rounding == "even" else ip.js_round(t)
        if store == "wrap":
            fin = np.where(np.isfinite(p), p, 0.0)
            b = (np.clip(fin, -2.0 ** 62, 2.0 ** 62).astype(np.int64) & 255).astype(np.uint8)
            b = np.where(np.isposinf(p), 255, b).astype(np.uint8)
        else:
            b = ip.to_uint8_clamped(p)
    return np.where(np.isnan(g), np.uint8(nan_byte), b).astype(np.uint8)


# ---------------------------------------------------------------------------
# Sampled mode
# ---------------------------------------------------------------------------
RAMPS = ("ramp", "ramp_shift", "ramp_neg_shift", "ramp_scale", "ramp_scale_up")
# The fixture's planes around the start values of the reference's scan; those of them that keep a start value
# (no element below 2^53 - 1, or none above its negative); and those of these on which a scan started at +-inf
# gives other bytes (in three of the others the difference, 1 in a range of 2^53 and more, moves no byte, and a plane
# of +inf alone is NaN either way).
EXTREMES = ("big_const", "big_pos", "big_neg", "e16", "all_nan", "pos_inf", "neg_inf", "both_inf", "inf_only",
            "nan_first", "p53_const", "p53_above", "p53_below_neg", "p53_from_below", "p53_mixed", "p53_pos_mixed",
            "p53_above_nan")
EXTREMES_KEEP_START = ("big_const", "big_pos", "big_neg", "e16", "inf_only", "p53_const", "p53_above",
                       "p53_below_neg", "p53_above_nan")
EXTREMES_INF_START_WRONG = ("big_const", "big_pos", "big_neg", "e16", "p53_const")


def fixture_plane(name):
    """(fp32 vector, {form: (n, 4) bytes}) of the fixture's plane x_<name>."""
    g = gold()
    return g["x_" + name], {f: g["x_%s_%s" % (name, f)].reshape(-1, 4) for f in ("plain", "sigmoid", "sampled")}


def sampled(v, mn=None, mx=None, reciprocal=False):
    """(v - min) / (max - min) in fp64, min / max by the reference's rule
    unless given; reciprocal: the wrong kernel that multiplies by 1 / range."""
    x = np.asarray(v, dtype=np.float64)
    if mn is None:
        seen = x[~np.isnan(x)]
        mn = min(seen.min(), ip.MAX_SAFE_INTEGER) if seen.size else ip.MAX_SAFE_INTEGER
        mx = max(seen.max(), -ip.MAX_SAFE_INTEGER) if seen.size else -ip.MAX_SAFE_INTEGER
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (x - mn) * (1.0 / (mx - mn)) if reciprocal else (x - mn) / (mx - mn)


def wrong_sampled_inf_start(v, keep=None):
    """Wrong kernel: the scan started at +inf / -inf (min and max of the
    non-NaN values, the start values only for a plane of NaNs), optionally
    over the elements keep (a mask) only: normalised values."""
    x = np.asarray(v, dtype=np.float64)
    s = x if keep is None else x[keep]
    s = s[~np.isnan(s)]
    mn = s.min() if s.size else np.inf
    mx = s.max() if s.size else -np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (x - mn) / (mx - mn)


MM_THREADS = 256


def minmax_parts(n):
    """Blocks of k_minmax_partial for n pixels (plane_image_parts): eight
    float4 per lane, at most 1024."""
    return max(1, min(1024, (n // 4 + MM_THREADS * 8 - 1) // (MM_THREADS * 8)))


def last_partial_mask(n):
    """Elements the last block of k_minmax_partial reads: float4 k belongs to
    block (k // 256) % parts, the tail (fewer than 4 elements) to block 0."""
    P, n4 = minmax_parts(n), n // 4
    k = np.arange(n4)
    m = np.repeat((k // MM_THREADS) % P == P - 1, 4)
    return np.concatenate([m, np.full(n - 4 * n4, P == 1)])


def positions(n):
    """Where the reduction can drop an element: the ends, both sides of the
    float4 body's end, the first and last element of the last block's first
    stride."""
    P, n4 = minmax_parts(n), n // 4
    cand = [0, n - 1, 4 * n4, 4 * n4 - 1, 4 * (P - 1) * MM_THREADS, 4 * min(P * MM_THREADS, n4) - 1]
    out = []
    for c in cand:
        if 0 <= c < n and c not in out:
            out.append(c)
    return out


# Plane sizes either side of: one float4, the wave and block widths, one lane's first float4 (1024), the step from
# one partial to two (n // 4 = 2049: 8196) and on, and the cap of 1024 partials (n > 8 388 608).  (W, H, octave).
POSITION_GEOMS = [(1, 1, 1), (2, 1, 1), (3, 1, 1), (1, 1, 0), (5, 1, 1), (15, 17, 1), (8, 8, 0), (257, 1, 1),
                  (1023, 1, 1), (41, 25, 1), (8191, 1, 1), (64, 32, 0), (2731, 3, 1), (683, 3, 0), (16383, 1, 1),
                  (3277, 5, 1), (2048, 1025, 0)]
POSITION_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 8191, 8192, 8193, 8196, 16383, 16385, 4096 * 2050]


@functools.lru_cache(maxsize=4)
def position_planes(n):
    """[(imin, imax, plane)]: mid-range noise with the unique minimum -1 at
    imin and the unique maximum 2 at imax; every position of positions(n)
    holds the minimum once and the maximum once."""
    pos = positions(n)
    noise = np.random.default_rng(n).uniform(0.25, 0.75, size=n).astype(F32)
    out = []
    for j, imin in enumerate(pos):
        imax = pos[(j + 1) % len(pos)]
        v = noise.copy()
        v[imax] = 2.0
        v[imin] = -1.0   # n == 1: the one element is both, 0 / 0
        v.setflags(write=False)
        out.append((imin, imax, v))
    return out


# ---------------------------------------------------------------------------
# Sigmoid
# ---------------------------------------------------------------------------
SIGMOID_COEFS = (5.0, 1.0, 0.0, -5.0, 1e308, float("inf"), float("nan"))
SIGMOID_SEED = 20
SIGMOID_RANDOM = 2048
TIE_MARGIN = 1e-9
# exp's argument a with |a| <= 2^-54: 1 + a rounds to 1, and fdlibm (V8), glibc (numpy) and the
# device library all return exactly 1 there, as they do for a = 0.
EXP_IS_ONE = 2.0 ** -54


@functools.lru_cache(maxsize=None)
def sigmoid_input():
    """The plain specials, then a seeded random plane in [-1, 1]."""
    r = np.random.default_rng(SIGMOID_SEED).uniform(-1.0, 1.0, size=SIGMOID_RANDOM).astype(F32)
    a = np.concatenate([plain_specials(), r])
    a.setflags(write=False)
    return a


def sigmoid_tie_distance(v, c):
    """(distance of g * 255 from the nearest k + 0.5, mask of the inputs whose
    exp is the same double in every implementation): exp's argument 0 (or
    within EXP_IS_ONE of it), +-inf or NaN."""
    x = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = c * (-1.0 * x)
        t = ip.sigmoid_normalize(x, c) * 255.0
    exact = np.isnan(a) | np.isinf(a) | (np.abs(a) <= EXP_IS_ONE)
    return np.abs(t - np.floor(t) - 0.5), exact
