#!/usr/bin/env python3
"""Golden fixtures for the image products.

Runs only in the build container (needs /root/reference and Node): drives
run_image_reference.mjs, which calls the reference's own
ImageUtils_convertImageDataToMatrix2D, Matrix2D_sigmoidNormalize,
Matrix2D_sampledNormalize and ImageUtils_convertMatrix2DToImageData, and
packs inputs and outputs into tests/golden/image_products.npz (data only).

Inputs: an RGBA image holding every byte value in every channel plus random
pixels, and an fp32 matrix with values in [-0.3, 1.3], exact k/255 and
(k+0.5)/255 grey levels (Math.round boundaries), huge magnitudes (clamping,
sigmoid saturation) and zeros; the same matrix without the saturating values
(the sampled normalisation then spreads over all levels); a constant matrix
pins the sampled normalisation's 0/0 case.

Extreme planes (EXTREMES, arrays x_<name> with x_<name>_plain / _sigmoid /
_sampled): Matrix2D_sampledNormalize starts its scan at min =
Number.MAX_SAFE_INTEGER and max = Number.MIN_SAFE_INTEGER (matrix2d.js:174-175),
so planes wholly above 2^53 - 1 or wholly below -(2^53 - 1) keep a start value;
with them all-NaN planes, infinities, a NaN first element, the fp32 neighbours
of 2^53 among ordinary values, and the integer ramp 0, 1, 3, ..., 509, 510
whose odd values the sampled mode puts exactly on k + 0.5 (shifted by a
constant and scaled by a power of two as well).  Each runs as a 1 x n matrix.
The plain specials of tests/image_cases.py followed by its random plane
(s_in) run once per sigmoid coefficient of that module (s_coefs, s_sigmoid_<j>;
s_plain and s_sampled from the last run).

A rerun keeps every array the file already holds bit for bit (asserted before
the file is replaced).

usage: python tests/golden/make_image_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")):
    sys.path.insert(0, _p)
import image_cases  # noqa: E402  (tests/image_cases.py: the tables whose reference bytes this file records)
OUT = os.path.join(HERE, "image_products.npz")
W, H = 37, 23            # RGBA image (ragged width: not a multiple of 4)
MW, MH = 74, 46          # matrix = the octave-0 plane of a W x H input
COEF = 5.0               # background.js:303


def rgba_input():
    rng = np.random.default_rng(1234)
    a = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    v = np.arange(256, dtype=np.uint8)
    flat = a.reshape(-1, 4)
    for c in range(4):
        flat[:256, c] = np.roll(v, 37 * c)
    return a


def matrix_input(const=False, moderate=False):
    if const:
        return np.full((MH, MW), 0.25, dtype=np.float32)
    rng = np.random.default_rng(99)
    m = rng.uniform(-0.3, 1.3, size=(MH, MW)).astype(np.float32)
    flat = m.reshape(-1)
    k = np.arange(256)
    flat[:256] = (k / 255.0).astype(np.float32)
    flat[256:512] = ((k + 0.5) / 255.0).astype(np.float32)
    flat[512:520] = np.array([0.0, -0.0, 1e30, -1e30, 300.0, -300.0, 0.5 / 255, 254.5 / 255], dtype=np.float32)
    if moderate:  # no saturating values: the sampled normalisation spreads over all levels
        flat[514:518] = 0.5
    return m


P53 = float(2 ** 53)
NAN, INF = float("nan"), float("inf")


def extreme_inputs():
    """name -> fp32 vector.  2^53 - 2^29 and 2^53 + 2^30 are 2^53's fp32 neighbours."""
    lo, hi = P53 - 2.0 ** 29, P53 + 2.0 ** 30
    ramp = np.concatenate([[0.0], np.arange(1.0, 510.0, 2.0), [510.0]])
    x = {
        "big_const": [1e30] * 4,
        "big_pos": [1e30, 2e30, 1.5e30, 1e30],
        "big_neg": [-1e30, -2e30, -1.5e30, -1e30],
        "e16": [1e16, 3e16, 2e16, 1e16],
        "all_nan": [NAN] * 4,
        "pos_inf": [0.25, INF, -0.5, 1.0, 0.75, 0.0],
        "neg_inf": [0.25, -INF, -0.5, 1.0, 0.75, 0.0],
        "both_inf": [INF, 0.25, -INF, 1.0, 0.75, 0.0],
        "inf_only": [INF, INF, INF, INF],
        "nan_first": [NAN, 0.1, 0.9, 0.5, NAN, 0.3],
        "p53_const": [P53] * 4,
        "p53_above": [P53, hi, 2.0 * P53, 3.0 * P53, hi, P53],
        "p53_below_neg": [-P53, -hi, -2.0 * P53, -3.0 * P53, -hi, -P53],
        "p53_from_below": [lo, P53, hi, 2.0 * P53, lo, 3.0 * P53],
        "p53_mixed": [0.25, lo, P53, hi, -1.5, 100.0, -lo, -P53, -hi, 7.0],
        "p53_pos_mixed": [0.25, lo, P53, hi, 1.5, 100.0, 3.0 * 2.0 ** 50, 7.0],
        "p53_above_nan": [NAN, hi, P53, 2.0 * P53, NAN, hi],
        "ramp": ramp,
        "ramp_shift": ramp + 1000.0,
        "ramp_neg_shift": ramp - 77.0,
        "ramp_scale": ramp * 2.0 ** -10,
        "ramp_scale_up": ramp * 2.0 ** 40,
    }
    out = {}
    for k, v in x.items():
        a = np.asarray(v, dtype=np.float64)
        out[k] = a.astype(np.float32)
        if k.startswith(("p53", "ramp")):  # these values are fp32 numbers as written
            assert np.array_equal(out[k].astype(np.float64), a, equal_nan=True), k
    assert out["ramp"].size == 257
    return out


def js_number(c):
    """A double as a string JavaScript's unary + reads back to the same double."""
    return "NaN" if c != c else ("-" if c < 0 else "") + "Infinity" if abs(c) == INF else repr(float(c))


def run(rgba, mat, tmp, tag, coef=COEF):
    rp, mp = os.path.join(tmp, "rgba.u8"), os.path.join(tmp, "m.f32")
    od = os.path.join(tmp, tag)
    os.makedirs(od)
    MH, MW = mat.shape
    rgba.tofile(rp)
    mat.tofile(mp)
    cmd = ["node", "--experimental-loader", os.path.join(HERE, "ref_loader.mjs"),
           os.path.join(HERE, "run_image_reference.mjs"), rp, str(W), str(H), mp, str(MW), str(MH), js_number(coef), od]
    subprocess.run(cmd, check=True, cwd=HERE, stderr=subprocess.DEVNULL)
    rd = lambda n, t: np.fromfile(os.path.join(od, n), dtype=t)  # noqa: E731
    return {
        "gray": rd("gray.f64", np.float64).reshape(H, W),
        "alpha": rd("alpha.f64", np.float64).reshape(H, W),
        "plain": rd("plain.u8", np.uint8).reshape(MH, MW, 4),
        "sigmoid": rd("sigmoid.u8", np.uint8).reshape(MH, MW, 4),
        "sampled": rd("sampled.u8", np.uint8).reshape(MH, MW, 4),
    }


def main():
    rgba = rgba_input()
    m = matrix_input()
    mm = matrix_input(moderate=True)
    mc = matrix_input(const=True)
    with tempfile.TemporaryDirectory() as tmp:
        r = run(rgba, m, tmp, "a")
        rm = run(rgba, mm, tmp, "m")
        rc = run(rgba, mc, tmp, "c")
        extra = {}
        for name, v in extreme_inputs().items():
            rx = run(rgba, v.reshape(1, -1), tmp, "x_" + name)
            extra["x_" + name] = v
            for form in ("plain", "sigmoid", "sampled"):
                extra["x_%s_%s" % (name, form)] = rx[form]
        # tests/image_cases.py: the plain specials and the sigmoid input, one run per coefficient
        sv = image_cases.sigmoid_input()
        extra["s_in"] = np.array(sv)
        extra["s_coefs"] = np.array(image_cases.SIGMOID_COEFS, dtype=np.float64)
        for j, c in enumerate(image_cases.SIGMOID_COEFS):
            rs = run(rgba, sv.reshape(1, -1), tmp, "s%d" % j, coef=c)
            extra["s_sigmoid_%d" % j] = rs["sigmoid"]
        extra["s_plain"], extra["s_sampled"] = rs["plain"], rs["sampled"]
    old = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    NEW = OUT[:-4] + ".new.npz"
    np.savez_compressed(NEW, rgba=rgba, matrix=m, matrix_mod=mm, matrix_const=mc, coef=np.float64(COEF),
                        mod_plain=rm["plain"], mod_sigmoid=rm["sigmoid"], mod_sampled=rm["sampled"],
                        gray=r["gray"], alpha=r["alpha"], plain=r["plain"], sigmoid=r["sigmoid"],
                        sampled=r["sampled"], const_plain=rc["plain"], const_sampled=rc["sampled"],
                        const_sigmoid=rc["sigmoid"], **extra)
    new = np.load(NEW)
    try:
        for k, v in old.items():  # a rerun changes nothing the file already held
            assert new[k].dtype == v.dtype and new[k].shape == v.shape and new[k].tobytes() == v.tobytes(), k
    except (AssertionError, KeyError):
        os.remove(NEW)
        raise
    os.replace(NEW, OUT)
    print("wrote", OUT, "(%d arrays, %d kept bit for bit)" % (len(new.files), len(old)))


if __name__ == "__main__":
    main()
