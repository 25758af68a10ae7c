"""Hand-built inputs of the orientation / descriptor stages: planes and
keypoints that reach the paths detector-found keypoints never do (the tie
rule, zero gradients, saturated bytes, border decisions, octave 0, large and
one-pixel boxes, many peaks, long keypoint lists), with the counts the numpy
statement (tests/feature_ref.py) gives on each.  tests/test_feature_ref.py
re-derives every count on the CPU; tests/test_gpu_feature_edges.py feeds the
same inputs to the kernels through sift_set_keypoints / sift_set_orientations.
Test infrastructure only.

Every case but "e" uses one geometry: a 96 x 80 image, 3 octaves, 3 scales,
i.e. six planes per octave of 192 x 160, 96 x 80 and 48 x 40 (w x h).
"""
import numpy as np

import feature_ref as fr
import sift_amd

W, H, O, S = 96, 80, 3, 3
NS = S + 3
TWO_PI = 2.0 * np.pi


def keypoints_at(points, octave=1, scale=1):
    """KEYPOINT_DTYPE records at octave-local (x, y, sigma) of octave `octave` (delta = 2^(octave-1))."""
    delta = 2.0 ** (octave - 1)
    kp = np.zeros(len(points), dtype=sift_amd.KEYPOINT_DTYPE)
    for i, (x, y, sg) in enumerate(points):
        kp[i] = (octave, scale, int(round(x)), int(round(y)), x * delta, y * delta, sg * delta, 0.0)
    return kp


def ramp(a, b, h=64, w=64):
    v, u = np.mgrid[0:h, 0:w]
    return (a * u + b * v).astype(np.float32)


def smooth_plane(h, w, seed):
    """A smooth fp32 plane with gradients of every direction: random low-frequency waves."""
    rng = np.random.RandomState(seed)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    P = np.zeros((h, w))
    for _ in range(24):
        fx, fy = rng.uniform(-0.25, 0.25, 2)
        P += rng.uniform(0.2, 1.0) * np.sin(fx * u + fy * v + rng.uniform(0, 2 * np.pi))
    return (P / 8.0).astype(np.float32)


def dims(width=W, height=H, octaves=O):
    """[(h, w)] per octave."""
    d = sift_amd.octave_dims(width, height, octaves)
    if (width, height, octaves) == (W, H, O):
        assert d == [(160, 192), (80, 96), (40, 48)], d
    return d


def filled(fn, width=W, height=H, octaves=O, scales=S):
    """planes[o][s] = fn(o, s, h, w)."""
    return [[np.ascontiguousarray(fn(o, s, h, w), dtype=np.float32) for s in range(scales + 3)]
            for o, (h, w) in enumerate(dims(width, height, octaves))]


def concat(parts):
    return np.concatenate(parts) if parts else np.zeros(0, dtype=sift_amd.KEYPOINT_DTYPE)


# ---- (a) integer ramps: one record each, at the bin centre -------------------
RAMPS = ((1, 0), (0, 1), (1, 1), (-1, 1), (-1, -1), (1, -1), (2, -2))
RAMP_BINS = (0, 9, 5, 14, 23, 32, 32)
# octave-local (x, y, sigma): non-integer, every box bound away from a half-integer, descriptor box inside
RAMP_POINTS = {0: (96.3, 79.8, 2.3), 1: (48.3, 39.8, 1.9), 2: (24.4, 19.8, 1.6)}


def ramp_slots(first):
    """RAMPS index of scale level s: seven ramps, six levels, so two plane sets ("a0": first = 0, "a1": first = 6)."""
    return [(first + s) % len(RAMPS) for s in range(NS)]


def _ramps(first):
    slots = ramp_slots(first)
    planes = filled(lambda o, s, h, w: ramp(*RAMPS[slots[s]], h=h, w=w))
    kp = concat([keypoints_at([RAMP_POINTS[o]], o, s) for o in range(O) for s in range(NS)])
    return planes, kp


# ---- (b) border decisions ----------------------------------------------------
def _borders():
    """sigma = 2: the orientation box has r = 9, so a keypoint has a record iff
    9.5 <= x < w - 10.5 and 9.5 <= y < h - 10.5 (rnd(x - 9) >= 1, rnd(x + 9) <=
    w - 2).  Per octave and side, two keypoints just inside and two just
    outside (the x = 9.4 / 10.6 and y = 53.4 / 53.6 of the 64-pixel CPU test,
    restated); then, on octaves 0 and 1, the descriptor's larger box (R =
    21.2): x = 22.0 is described, x = 21.0 has a record that is not (octave 2
    is too small for any sigma = 2 descriptor)."""
    planes = filled(lambda o, s, h, w: ramp(1, 0, h=h, w=w))
    parts = []
    for o, (h, w) in enumerate(dims()):
        cx, cy = w / 2 + 0.3, h / 2 + 0.2
        pts = [(9.6, cy), (10.6, cy), (9.4, cy), (9.2, cy),                  # left: in, in, out, out
               (w - 10.6, cy), (w - 11.6, cy), (w - 10.4, cy), (w - 9.7, cy),  # right
               (cx, 9.7), (cx, 10.6), (cx, 9.3), (cx, 8.8),                   # top
               (cx, h - 10.6), (cx, h - 11.4), (cx, h - 10.4), (cx, h - 9.6)]  # bottom
        if o < 2:
            pts += [(22.0, cy), (21.0, cy)]
        for i, (x, y) in enumerate(pts):
            parts.append(keypoints_at([(x, y, 2.0)], o, i % NS))
    return planes, concat(parts)


BORDER_HAS_RECORD = ([1, 1, 0, 0] * 4 + [1, 1]) * 2 + [1, 1, 0, 0] * 4


# ---- (c) degenerate gradients ------------------------------------------------
STEP_KEYPOINT = 6  # index in case "c"
STEP_BYTES = [(4 * i + 3) * 8 for i in range(4)]  # cell (i, 3), bin 0


def degenerate_records():
    """theta = 0 for every keypoint of case "c" (none has a record of its own)."""
    recs = np.zeros(STEP_KEYPOINT + 1, dtype=fr.ORIENTATION_DTYPE)
    recs["keypoint"] = np.arange(STEP_KEYPOINT + 1)
    return recs


def _degenerate():
    """Constant planes everywhere (no record for any keypoint: atan2(0, 0), an
    all-zero histogram) but (octave 1, scale 1): zero with one vertical step,
    P[:, 60:] = 1.  The step's keypoint is at (47.4, 47.6, 2) rather than the
    (47.5, 47.5, 2) whose orientation box bound x - 9 = 38.5 is a half-integer
    (flagged).  With theta = 0 its only gradients (columns 59 and 60, angle 0)
    fall into cell column 3, bin 0 of the four cell rows: four non-zero values,
    all clamped to 0.2 * norm, so each is exactly half the second norm, q = 256
    exactly, and the byte is min(256, 255)."""
    def plane(o, s, h, w):
        P = np.full((h, w), 0.25 * (s + 1), dtype=np.float32)
        if (o, s) == (1, 1):
            P[:] = 0.0
            P[:, 60:] = 1.0
        return P
    kp = concat([keypoints_at([(90.4, 80.3, 2.0)], 0, 0), keypoints_at([(100.2, 70.6, 0.7)], 0, 5),
                 keypoints_at([(47.4, 39.6, 1.5)], 1, 0), keypoints_at([(30.3, 41.2, 1.0)], 1, 3),
                 keypoints_at([(24.3, 19.8, 1.2)], 2, 2), keypoints_at([(20.3, 21.4, 0.6)], 2, 4),
                 keypoints_at([(47.4, 47.6, 2.0)], 1, 1)])
    return planes_checked(filled(plane)), kp


def planes_checked(planes):
    assert all(np.isfinite(P).all() for octv in planes for P in octv)
    return planes


# ---- (d) random keypoints on smooth planes: the bulk comparison -----------------
def _random():
    planes = filled(lambda o, s, h, w: smooth_plane(h, w, 100 + 10 * o + s))
    rng = np.random.RandomState(42)
    parts = []
    for o, (h, w) in enumerate(dims()):
        for _ in range(150):
            x = rng.uniform(0, w - 1)
            y = rng.uniform(0, h - 1)
            sg = rng.uniform(0.5, 2.0 if o == 2 else 4.0)
            s = rng.randint(0, NS)
            parts.append(keypoints_at([(x, y, sg)], o, s))
    return planes, concat(parts)


# ---- (e) large and one-pixel boxes: a geometry of its own -----------------------
E_GEOM = (100, 100, 1, 3)  # one octave of 200 x 200 planes


def _large():
    """sigma = 8: the orientation box is 73 x 73 pixels (83 or 84 per lane) and
    the descriptor box 171 x 171.  sigma = 0.1: the orientation box is the
    single pixel (50, 60)."""
    w_, h_, o_, s_ = E_GEOM
    planes = filled(lambda o, s, h, w: smooth_plane(h, w, 200 + s), w_, h_, o_, s_)
    kp = concat([keypoints_at([(100.3, 99.6, 8.0)], 0, 2), keypoints_at([(50.02, 60.03, 0.1)], 0, 4)])
    return planes, kp


# ---- (g) many peaks -------------------------------------------------------------
def _four_peaks():
    """r cos(4 phi) / 8 about (47.5, 47.5): four gradient lobes.  The keypoint is off the centre -- the centred one
    has four exactly equal peaks, which the reference flags."""
    def plane(o, s, h, w):
        v, u = np.mgrid[0:h, 0:w].astype(np.float64)
        dx, dy = u - 47.5, v - 47.5
        return np.hypot(dx, dy) * np.cos(4.0 * np.arctan2(dy, dx)) / 8.0
    return filled(plane), keypoints_at([(47.8, 47.3, 2.5)], 1, 2)


# ---- (h) the scan and the emission at size ---------------------------------------
# sift_orient's exclusive scan is hipcub::DeviceScan::ExclusiveSum over n + 1 counts.  rocPRIM's default tile for
# 4-byte values is 256 threads x 16 items = 4096 (a tuned configuration may differ): 25 411 is six of those and a
# ragged remainder, and still three and a remainder if the tile in use is twice that.
H_COUNT = 25411
H_DISTINCT = (17, 18, 15)  # keypoints of "d" with 0, 1 and 2 records


def many_from(ref_d):
    """(indices into case d's keypoints [H_COUNT], the 50 distinct ones): a fixed shuffled repetition."""
    per = np.bincount(ref_d["ori"]["keypoint"], minlength=len(ref_d["amb"]))
    ok = ~ref_d["amb"]
    distinct = np.concatenate([np.nonzero(ok & (per == c))[0][:n] for c, n in enumerate(H_DISTINCT)])
    assert len(distinct) == sum(H_DISTINCT)
    return distinct[np.random.RandomState(7).randint(0, len(distinct), H_COUNT)], distinct


# ---- (j) unusable geometry among usable ------------------------------------------
J_BAD = {3: ("abs_x", np.nan), 8: ("abs_y", np.inf), 11: ("abs_sigma", 0.0), 12: ("abs_sigma", -1.5),
         20: ("abs_sigma", 1e30), 24: ("abs_x", -np.inf), 25: ("abs_sigma", np.nan)}
J_COUNT = 26


def unusable():
    """The first small-sigma keypoints of "d", some made unusable: none of
    those may yield a record (the kernels compare in fp64 before any cast),
    the rest keep theirs."""
    planes, kp = _random()
    kp = kp[(kp["abs_sigma"] / 2.0 ** (kp["octave"] - 1.0) < 1.2) & (kp["abs_sigma"] > 0)][:J_COUNT].copy()
    assert len(kp) == J_COUNT
    for i, (field, value) in J_BAD.items():
        kp[field][i] = value
    return planes, kp


# name: (builder, (width, height, octaves, scales),
#        counts of the reference: records, keypoints without a record, keypoints with several, described records,
#        bytes equal to 255)
CASES = {
    "a0": (lambda: _ramps(0), (W, H, O, S), (18, 0, 0, 18, 0)),
    "a1": (lambda: _ramps(6), (W, H, O, S), (18, 0, 0, 18, 0)),
    "b": (_borders, (W, H, O, S), (28, 24, 0, 2, 0)),
    "c": (_degenerate, (W, H, O, S), (0, 7, 0, 0, 0)),
    "d": (_random, (W, H, O, S), (288, 177, 15, 137, 0)),
    "e": (_large, E_GEOM, (3, 0, 1, 3, 0)),
    "g": (_four_peaks, (W, H, O, S), (4, 0, 1, 4, 0)),
}
_built = {}
_refs = {}


def case(name):
    """dict(planes, kp, geom, params, counts) of a case, built once and read-only."""
    if name not in _built:
        build, geom, counts = CASES[name]
        planes, kp = build()
        planes_checked(planes)
        for P in [kp] + [P for octv in planes for P in octv]:
            P.setflags(write=False)
        _built[name] = dict(planes=planes, kp=kp, geom=geom, counts=counts,
                            params=sift_amd.make_params(geom[2], geom[3]))
    return _built[name]


def reference(name):
    """feature_ref on a case, once: dict(ori, amb, desc, described, flag), read-only."""
    if name not in _refs:
        c = case(name)
        ori, amb = fr.orient(c["planes"], c["kp"])
        desc, described, flag = fr.describe(c["planes"], c["kp"], ori)
        for a in (ori, amb, desc, described, flag):
            a.setflags(write=False)
        _refs[name] = dict(ori=ori, amb=amb, desc=desc, described=described, flag=flag)
    return _refs[name]


def counts_of(kp, ref):
    per = np.bincount(ref["ori"]["keypoint"], minlength=len(kp))
    return (len(ref["ori"]), int((per == 0).sum()), int((per > 1).sum()), int(ref["described"].sum()),
            int((ref["desc"] == 255).sum()))


def with_theta(recs, theta):
    out = np.array(recs, dtype=fr.ORIENTATION_DTYPE)
    out["theta"] = theta
    return out


def quarter_turn(planes, kp, recs, widths):
    """np.rot90 of every plane (P'[i][j] = P[j][w-1-i]): (x, y) -> (y, w-1-x), theta -> theta - pi/2."""
    turned = [[np.ascontiguousarray(np.rot90(P)) for P in octv] for octv in planes]
    k = kp.copy()
    delta = 2.0 ** (kp["octave"] - 1.0)
    k["abs_x"] = kp["abs_y"]
    k["abs_y"] = ((np.asarray(widths)[kp["octave"]] - 1) - kp["abs_x"] / delta) * delta
    k["local_x"], k["local_y"] = kp["local_y"], np.asarray(widths)[kp["octave"]] - 1 - kp["local_x"]
    r = np.array(recs, dtype=fr.ORIENTATION_DTYPE)
    th = np.mod(recs["theta"] - np.pi / 2, TWO_PI)
    r["theta"] = np.where(th >= TWO_PI, 0.0, th)
    r["bin"] = (recs["bin"] - 9) % 36
    return turned, k, r
