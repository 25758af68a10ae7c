"""The numpy statement of the orientation / descriptor stages
(tests/feature_ref.py) against properties it cannot pass by accident, and the
binding's side of the new entry points.  No GPU."""
import numpy as np
import pytest

import feature_cases as fc
import feature_ref as fr
import sift_amd
from feature_cases import keypoints_at, ramp, smooth_plane


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


def test_binding_declares_the_keypoint_and_orientation_seams():
    L = sift_amd.lib()
    for name in ("sift_set_keypoints", "sift_set_orientations"):
        assert hasattr(L, name), name
        assert name in sift_amd.ABI_SYMBOLS
    for method in ("set_keypoints", "set_orientations"):
        assert callable(getattr(sift_amd.Context, method))


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_edge_cases_give_their_counts_within_the_flag_caps(name):
    """Every case of tests/feature_cases.py on the reference alone: the exact
    counts written next to it, and ambiguity flags within the caps of
    tests/test_gpu_features.py (1 % of the keypoints, 0.1 % of the bytes --
    none at all below 100 keypoints / 1000 bytes)."""
    c, ref = fc.case(name), fc.reference(name)
    got = fc.counts_of(c["kp"], ref)
    print("case %s: %d keypoints; records, no record, multi-peak, described, bytes at 255 = %s; "
          "%d flagged keypoints, %d flagged bytes" % (name, len(c["kp"]), got, int(ref["amb"].sum()),
                                                      int(ref["flag"].sum())))
    assert got == c["counts"]
    assert ref["amb"].sum() <= 0.01 * len(c["kp"])
    assert ref["flag"].sum() <= 0.001 * ref["flag"].size
    assert not ref["desc"][~ref["described"]].any()


def test_edge_case_properties_hold_on_the_reference():
    """What tests/test_gpu_feature_edges.py relies on beyond the counts."""
    for name, first in (("a0", 0), ("a1", 6)):
        c, ref = fc.case(name), fc.reference(name)
        want = np.array([fc.RAMP_BINS[i] for i in fc.ramp_slots(first)] * fc.O)
        assert (ref["ori"]["keypoint"] == np.arange(len(want))).all() and (ref["ori"]["bin"] == want).all()
        assert np.abs(ref["ori"]["theta"] - want * np.pi / 18).max() < 1e-9
        diagonal = want % 9 != 0
        assert ((ref["desc"][diagonal] > 0).sum(axis=1) == 32).all() and (ref["desc"][diagonal].max(axis=1) == 128).all()
    c, ref = fc.case("b"), fc.reference("b")
    assert (np.bincount(ref["ori"]["keypoint"], minlength=len(c["kp"])) == fc.BORDER_HAS_RECORD).all()
    x = c["kp"]["abs_x"] / 2.0 ** (c["kp"]["octave"] - 1.0)
    assert (ref["described"] == (x[ref["ori"]["keypoint"]] == 22.0)).all()
    # degenerate gradients, with theta = 0 supplied: constant planes are described with zero bytes, the step
    # saturates exactly four
    c, recs = fc.case("c"), fc.degenerate_records()
    desc, described, flag = fr.describe(c["planes"], c["kp"], recs)
    assert described.all() and not desc[:fc.STEP_KEYPOINT].any() and not flag[:fc.STEP_KEYPOINT].any()
    assert np.nonzero(desc[fc.STEP_KEYPOINT])[0].tolist() == fc.STEP_BYTES
    assert (desc[fc.STEP_KEYPOINT][fc.STEP_BYTES] == 255).all()
    assert np.nonzero(flag[fc.STEP_KEYPOINT])[0].tolist() == fc.STEP_BYTES  # q = 256 exactly
    c, ref = fc.case("d"), fc.reference("d")
    octave = c["kp"]["octave"][ref["ori"]["keypoint"]]
    assert [int(ref["described"][octave == o].sum()) for o in range(fc.O)] == [79, 31, 27]
    assert np.bincount(ref["ori"]["keypoint"]).max() == 2
    ref = fc.reference("g")
    assert (np.diff(ref["ori"]["bin"]) > 0).all() and len(ref["ori"]) == 4
    idx, distinct = fc.many_from(fc.reference("d"))
    assert len(idx) == fc.H_COUNT and len(set(idx.tolist())) == len(distinct) == 50
