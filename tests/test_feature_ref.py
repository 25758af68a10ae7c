"""The numpy statement of the orientation / descriptor stages
(tests/feature_ref.py) against properties it cannot pass by accident, and the
binding's side of the new entry points.  No GPU."""
import numpy as np

import feature_ref as fr
import sift_amd


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


def test_binding_declares_the_feature_entry_points():
    L = sift_amd.lib()
    for name in ("sift_orient", "sift_describe", "sift_device_features", "sift_last_feature_timings"):
        assert hasattr(L, name), name
        assert name in sift_amd.ABI_SYMBOLS
    assert sift_amd.ORIENTATION_DTYPE.itemsize == 16
    assert sift_amd.ORIENTATION_DTYPE == fr.ORIENTATION_DTYPE
    for method in ("orient", "describe", "device_features", "feature_timings"):
        assert callable(getattr(sift_amd.Context, method))


def test_linear_ramps_give_their_gradient_direction():
    kp = keypoints_at([(30.25, 31.3, 2.0)])
    for (a, b), theta in (((1, 0), 0.0), ((0, 1), np.pi / 2)):
        recs, amb = fr.orient({1: {1: ramp(a, b)}}, kp)
        assert len(recs) == 1 and not amb.any()
        assert recs["keypoint"][0] == 0
        d = abs(recs["theta"][0] - theta)
        assert min(d, 2 * np.pi - d) < 1e-12
    # |gx| == |gy|: t = 4.5 exactly, a bin edge; the tie rule puts it in bin 5
    recs, amb = fr.orient({1: {1: ramp(1, 1)}}, kp)
    assert len(recs) == 1 and not amb.any()
    assert recs["bin"][0] == 5
    for (a, b), bin_ in (((-1, 1), 14), ((-1, -1), 23), ((1, -1), 32)):
        recs, _ = fr.orient({1: {1: ramp(a, b)}}, kp)
        assert [int(x) for x in recs["bin"]] == [bin_]


def test_keypoint_near_the_border_yields_no_record():
    P = ramp(1, 0)
    sg = 2.0  # r = 9: the box of x = 9.4 starts at column rnd(0.4) = 0 < 1
    recs, _ = fr.orient({1: {1: P}}, keypoints_at([(9.4, 32.0, sg), (10.6, 32.0, sg), (32.0, 53.6, sg),
                                                   (32.0, 53.4, sg)]))
    assert [int(k) for k in recs["keypoint"]] == [1, 3]
    # described needs the larger box: R = sqrt(2) * 6 * sg * 5/4 = 21.2 at sg = 2
    kp = keypoints_at([(32.0, 32.0, 2.0), (21.0, 32.0, 2.0)])
    recs, _ = fr.orient({1: {1: P}}, kp)
    assert len(recs) == 2
    desc, described, _ = fr.describe({1: {1: P}}, kp, recs)
    assert described.tolist() == [True, False]
    assert desc[0].any() and not desc[1].any()


def test_octave_scales_the_frame():
    """The same plane read as octave 2 (delta = 2) with doubled absolute coordinates gives the same records."""
    P = smooth_plane(80, 90, 3)
    pts = [(40.3, 38.7, 1.9), (30.1, 45.2, 2.4)]
    r1, _ = fr.orient({1: {2: P}}, keypoints_at(pts, 1, 2))
    r2, _ = fr.orient({2: {2: P}}, keypoints_at(pts, 2, 2))
    assert len(r1) >= 2
    assert r1.tobytes() == r2.tobytes()


def test_quarter_turn_of_the_plane_turns_the_records():
    h, w = 96, 112
    P = smooth_plane(h, w, 7)
    rng = np.random.RandomState(11)
    pts = [(rng.uniform(30, w - 31), rng.uniform(30, h - 31), rng.uniform(1.6, 2.6)) for _ in range(12)]
    kp = keypoints_at(pts)
    # np.rot90: P'[i][j] = P[j][w-1-i], so (x, y) -> (y, w-1-x) and every gradient angle drops by pi/2
    Pr = np.ascontiguousarray(np.rot90(P))
    kpr = keypoints_at([(y, (w - 1) - x, sg) for x, y, sg in pts])
    recs, amb = fr.orient({1: {1: P}}, kp)
    recs_r, amb_r = fr.orient({1: {1: Pr}}, kpr)
    ok = ~(amb | amb_r)
    assert ok.sum() >= 10
    n_checked = 0
    for i in np.nonzero(ok)[0]:
        a = recs[recs["keypoint"] == i]
        b = recs_r[recs_r["keypoint"] == i]
        assert len(a) == len(b) >= 1
        # the turn moves bin k to k - 9 (mod 36): compare as sets of angles
        want = np.sort(np.mod(a["theta"] - np.pi / 2, 2 * np.pi))
        got = np.sort(b["theta"])
        d = np.abs(want - got)
        assert np.minimum(d, 2 * np.pi - d).max() < 1e-9
        assert sorted((int(k) - 9) % 36 for k in a["bin"]) == sorted(int(k) for k in b["bin"])
        n_checked += len(a)
    assert n_checked >= 10
    # descriptors: the same bytes for the turned record, apart from flagged bytes
    desc, described, flag = fr.describe({1: {1: P}}, kp, recs)
    desc_r, described_r, flag_r = fr.describe({1: {1: Pr}}, kpr, recs_r)
    assert described.sum() >= 8
    n_desc = 0
    for i in np.nonzero(ok)[0]:
        ia = np.nonzero(recs["keypoint"] == i)[0]
        ib = np.nonzero(recs_r["keypoint"] == i)[0]
        ia = ia[np.argsort((recs["bin"][ia] - 9) % 36)]
        ib = ib[np.argsort(recs_r["bin"][ib])]
        for ra, rb in zip(ia, ib):
            assert described[ra] == described_r[rb]
            free = ~(flag[ra] | flag_r[rb])
            assert (desc[ra][free] == desc_r[rb][free]).all()
            assert np.abs(desc[ra].astype(int) - desc_r[rb].astype(int)).max() <= 1
            n_desc += int(described[ra])
    assert n_desc >= 8


def test_descriptor_is_normalised_and_capped():
    P = smooth_plane(96, 96, 5)
    kp = keypoints_at([(48.2, 47.6, 2.0)])
    recs, _ = fr.orient({1: {1: P}}, kp)
    desc, described, _ = fr.describe({1: {1: P}}, kp, recs)
    assert described.all()
    f = desc.astype(np.float64) / 512.0
    # after the 0.2 cap and renormalisation every entry is at most 0.2 n / n2 and the norm is just under 1
    nrm = np.sqrt((f * f).sum(axis=1))
    assert ((nrm > 0.9) & (nrm <= 1.0)).all()
    assert desc.max() <= 255
