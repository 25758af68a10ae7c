"""Plain numpy statement of the orientation and descriptor stages
(include/sift_hip.h, sift_orient / sift_describe): Rey-Otero & Delbracio,
"Anatomy of the SIFT Method", algorithms 11 and 12, in fp64 and octave-local
pixel units on fp32 Gaussian planes.  Test infrastructure only.

planes[o][s] is the (h, w) float32 plane (octave o, scale s) -- a list of
lists or a dict of dicts; keypoints is a sift_amd.KEYPOINT_DTYPE array.

Besides its results each function returns an ambiguity mask: the decisions
that sit within MARGIN of a discontinuity of the definition, where two
correct fp64 evaluations may legitimately differ.
"""
import numpy as np

LAMBDA_ORI = 1.5
N_BINS = 36
N_SMOOTH = 6
PEAK_RATIO = 0.8
LAMBDA_DESC = 6.0
N_CELLS = 4
N_ORI = 8
DESC_CAP = 0.2
MARGIN = 1e-9
TWO_PI = 2.0 * np.pi

ORIENTATION_DTYPE = np.dtype([("keypoint", "<i4"), ("bin", "<i4"), ("theta", "<f8")])


def rnd(t):
    return np.floor(t + 0.5)


def _near_half_integer(t):
    """t + 0.5 within MARGIN of an integer: rnd(t) is undecided."""
    t = np.asarray(t, dtype=np.float64) + 0.5
    return np.abs(t - np.rint(t)) < MARGIN


def _frame(planes, k):
    o, s = int(k["octave"]), int(k["scale_level"])
    delta = 2.0 ** (o - 1)
    P = np.asarray(planes[o][s])
    assert P.dtype == np.float32
    return P, float(k["abs_x"]) / delta, float(k["abs_y"]) / delta, float(k["abs_sigma"]) / delta


def _box(P, x, y, r):
    """(u0, u1, v0, v1) if the box lies within [1, w-2] x [1, h-2], else None; and whether a bound is undecided."""
    h, w = P.shape
    bounds = np.array([x - r, x + r, y - r, y + r])
    amb = bool(_near_half_integer(bounds).any())
    u0, u1, v0, v1 = (int(b) for b in rnd(bounds))
    if u0 >= 1 and v0 >= 1 and u1 <= w - 2 and v1 <= h - 2:
        return (u0, u1, v0, v1), amb
    return None, amb


def _gradients(P, u0, u1, v0, v1):
    """gx, gy (fp64) over the box, and the pixel coordinate grids u, v."""
    P64 = P.astype(np.float64)
    gx = (P64[v0:v1 + 1, u0 + 1:u1 + 2] - P64[v0:v1 + 1, u0 - 1:u1]) / 2.0
    gy = (P64[v0 + 1:v1 + 2, u0:u1 + 1] - P64[v0 - 1:v1, u0:u1 + 1]) / 2.0
    v, u = np.mgrid[v0:v1 + 1, u0:u1 + 1]
    return gx, gy, u.astype(np.float64), v.astype(np.float64)


def orientation_histogram(P, x, y, sg):
    """The raw 36-bin histogram of one keypoint, or None when its box leaves
    the plane; and whether a box bound or a sample's bin is undecided."""
    box, amb = _box(P, x, y, 3.0 * LAMBDA_ORI * sg)
    if box is None:
        return None, amb
    gx, gy, u, v = _gradients(P, *box)
    dx, dy = u - x, v - y
    c = np.exp(-(dx * dx + dy * dy) / (2.0 * ((LAMBDA_ORI * sg) * (LAMBDA_ORI * sg)))) * np.sqrt(gx * gx + gy * gy)
    a = np.arctan2(gy, gx)
    a = np.where(a < 0.0, a + TWO_PI, a)
    t = 36.0 * a / TWO_PI
    bins = rnd(t).astype(np.int64) % N_BINS
    tie = (np.abs(gx) == np.abs(gy)) & (gx != 0.0)
    tie_bin = np.where(gy > 0.0, np.where(gx > 0.0, 5, 14), np.where(gx < 0.0, 23, 32))
    bins = np.where(tie, tie_bin, bins)
    amb = amb or bool((_near_half_integer(t) & ~tie).any())
    return np.bincount(bins.ravel(), weights=c.ravel(), minlength=N_BINS), amb


def peaks(hist):
    """[(bin, theta)] of a raw histogram after smoothing, ascending bin; and whether a peak decision is undecided."""
    h = hist
    for _ in range(N_SMOOTH):
        h = (np.roll(h, 1) + h + np.roll(h, -1)) / 3.0
    hm, hp = np.roll(h, 1), np.roll(h, -1)
    mx = h.max()
    is_peak = (h > hm) & (h > hp) & (h >= PEAK_RATIO * mx)
    amb = bool((np.abs(h - PEAK_RATIO * mx) < MARGIN * mx).any())
    high = h >= (PEAK_RATIO - MARGIN) * mx
    amb = amb or bool((high & ((np.abs(h - hm) < MARGIN * mx) | (np.abs(h - hp) < MARGIN * mx))).any())
    out = []
    for k in np.nonzero(is_peak)[0]:
        th = TWO_PI * float(k) / 36.0 + (np.pi / 36.0) * (hm[k] - hp[k]) / (hm[k] - 2.0 * h[k] + hp[k])
        if th < 0.0:
            th += TWO_PI
        if th >= TWO_PI:
            th -= TWO_PI
        out.append((int(k), float(th)))
    return out, amb


def orient(planes, keypoints, params=None):
    """(records ORIENTATION_DTYPE in keypoint order then bin, ambiguous bool
    [n_keypoints]).  params is accepted for symmetry with the detection
    stages; the constants of these stages are fixed."""
    recs = []
    amb = np.zeros(len(keypoints), dtype=bool)
    for i, k in enumerate(keypoints):
        P, x, y, sg = _frame(planes, k)
        hist, amb[i] = orientation_histogram(P, x, y, sg)
        if hist is None:
            continue
        pk, a = peaks(hist)
        amb[i] |= a
        recs.extend((i, b, th) for b, th in pk)
    return np.array(recs, dtype=ORIENTATION_DTYPE), amb


def describe(planes, keypoints, orientations):
    """(desc uint8 [n, 128], described bool [n], ambiguous bool [n, 128]) for
    the given orientation records (their theta is taken as it is)."""
    n = len(orientations)
    desc = np.zeros((n, 128), dtype=np.uint8)
    described = np.zeros(n, dtype=bool)
    amb = np.zeros((n, 128), dtype=bool)
    centres = (np.arange(N_CELLS) - 1.5) * 3.0
    for r, rec in enumerate(orientations):
        P, x, y, sg = _frame(planes, keypoints[int(rec["keypoint"])])
        theta = float(rec["theta"])
        box, _ = _box(P, x, y, np.sqrt(2.0) * LAMBDA_DESC * sg * 5.0 / 4.0)
        if box is None:
            continue
        described[r] = True
        gx, gy, u, v = _gradients(P, *box)
        dx, dy = u - x, v - y
        ct, st = np.cos(theta), np.sin(theta)
        xh = (dx * ct + dy * st) / sg
        yh = (-dx * st + dy * ct) / sg
        keep = np.maximum(np.abs(xh), np.abs(yh)) < 7.5
        gx, gy, dx, dy, xh, yh = (a[keep] for a in (gx, gy, dx, dy, xh, yh))
        c = np.exp(-(dx * dx + dy * dy) / (2.0 * ((LAMBDA_DESC * sg) * (LAMBDA_DESC * sg)))) * \
            np.sqrt(gx * gx + gy * gy)
        a = np.mod(np.arctan2(gy, gx) - theta, TWO_PI)
        wx = np.maximum(1.0 - np.abs(xh[:, None] - centres[None, :]) / 3.0, 0.0)  # [pixel, j]
        wy = np.maximum(1.0 - np.abs(yh[:, None] - centres[None, :]) / 3.0, 0.0)  # [pixel, i]
        d = np.abs(a[:, None] - TWO_PI * np.arange(N_ORI)[None, :] / 8.0)
        d = np.minimum(d, TWO_PI - d)
        wk = np.maximum(1.0 - d * 8.0 / TWO_PI, 0.0)                               # [pixel, k]
        f = np.einsum("pi,pj,pk->ijk", wy * c[:, None], wx, wk).ravel()
        nrm = np.sqrt(np.sum(f * f))
        if nrm == 0.0:
            continue
        f = np.minimum(f, DESC_CAP * nrm)
        q = 512.0 * f / np.sqrt(np.sum(f * f))
        desc[r] = np.minimum(np.floor(q), 255.0).astype(np.uint8)
        near = np.rint(q)
        amb[r] = (near >= 1.0) & (np.abs(q - near) < MARGIN)
    return desc, described, amb
