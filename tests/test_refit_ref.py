"""The numpy restatement of the least-squares refit (tests/refit_ref.py) held
against itself, against numpy's own least squares and against planted data; and
the presence of the new entry points in the binding and the library.  No GPU."""
import numpy as np
import pytest

import ransac_ref as rr
import refit_ref as rf
import sift_amd

SIZES = [4, 5, 63, 64, 65, 4097]
NEW_SYMBOLS = ("sift_homography_fit_device", "sift_homography_fit", "sift_copy_homography_fit_sums",
               "sift_homography_refit_device", "sift_homography_refit", "sift_verify_features_refit",
               "sift_last_refit_timings")

# Transfer error at the frame's corners and centre of the fit of planted(64, 1.0, 0.0, 3) against PLANTED_H, as the
# restatement gives it (both forms: they agree bitwise), and the bound of the test: ten times that.
EXACT_MEASURED_PX = 5.63e-13
EXACT_TOL_PX = 10 * EXACT_MEASURED_PX
# Largest transfer error between the fit and np.linalg.lstsq of the same normalised 2m x 8 system over LSTSQ_CASES
# (1.0e-12, 3.2e-12, 3.6e-12, 3.3e-12 px; the normal matrix's condition number is 25 .. 27), and the bound: 1000 x.
LSTSQ_MEASURED_PX = 3.65e-12
LSTSQ_TOL_PX = 1000 * LSTSQ_MEASURED_PX
LSTSQ_CASES = [(64, 0.5, 1), (300, 1.0, 2), (3000, 0.75, 3), (4097, 1.0, 4)]


def test_new_entry_points_are_bound_and_exported():
    assert set(NEW_SYMBOLS) <= set(sift_amd.ABI_SYMBOLS)
    L = sift_amd.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ("fit_homography", "homography_fit_sums", "refit_homography", "verify_features_refit",
                 "refit_timings"):
        assert hasattr(sift_amd.Context, name), name


@pytest.mark.parametrize("m", SIZES)
def test_tree_sum_of_ones(m):
    assert rf.tree_sum(np.ones(m)) == m == rf.tree_sum_scalar(np.ones(m))
    assert rf.tree_sum(np.ones((3, m))).tolist() == [m] * 3


def test_tree_sum_is_the_stated_tree():
    """65 terms: the first chunk's halving tree, then (chunk 0 + 0 ...) + (chunk 1 + 0 ...) at the second level."""
    v = np.random.default_rng(0).uniform(-1.0, 1.0, 65)
    p = v[:64].copy()
    for s in (32, 16, 8, 4, 2, 1):
        p[:s] = p[:s] + p[s:2 * s]
    want = p[0] + v[64]
    assert rf.tree_sum(v) == want == rf.tree_sum_scalar(v)
    assert rf.tree_sum(v[:1]) == v[0] and rf.tree_sum(v[:0]) == 0.0


@pytest.mark.parametrize("m", SIZES)
def test_scalar_and_vector_forms_agree_bitwise(m):
    pts, _, _ = rr.planted(m, 1.0, 0.5, m)
    a, b = rf.fit_ref(pts, None, "scalar"), rf.fit_ref(pts, None, "vector")
    assert a[1] and b[1]
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert b[0][2, 2] == 1.0
    idx = np.random.default_rng(m).permutation(m)[:max(4, m // 2)]      # a list in its own order
    a, b = rf.fit_ref(pts, idx, "scalar"), rf.fit_ref(pts, idx, "vector")
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()


def test_the_order_of_the_list_is_part_of_the_definition():
    pts, _, _ = rr.planted(300, 1.0, 1.0, 5)
    perm = np.random.default_rng(6).permutation(300)
    a, b = rf.fit_ref(pts, np.arange(300)), rf.fit_ref(pts, perm)
    assert a[2].tobytes() == b[2].tobytes()                              # the box is order-free
    assert (a[3] != b[3]).any()                                          # the sums are not (18 of 44 differ here)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-12, atol=1e-12)


def test_exact_data_returns_the_planted_matrix():
    pts, H_true, _ = rr.planted(64, 1.0, 0.0, 3)
    for form in ("scalar", "vector"):
        H, ok, _, _ = rf.fit_ref(pts, None, form)
        err = rf.corner_error(H, H_true)
        print("exact data, %s form: %.3e px" % (form, err))
        assert ok and err < EXACT_TOL_PX


def lstsq_fit(pts):
    """np.linalg.lstsq of the 2m x 8 system in the fit's own normalised coordinates, denormalised like the fit."""
    _, _, box, _ = rf.fit_ref(pts)
    cx, cy, dq, cX, cY, dt = box
    x, y = (pts["qx"] - cx) / dq, (pts["qy"] - cy) / dq
    X, Y = (pts["tx"] - cX) / dt, (pts["ty"] - cY) / dt
    m = len(pts)
    A, b = np.zeros((2 * m, 8)), np.zeros(2 * m)
    A[0::2, 0], A[0::2, 1], A[0::2, 2], A[0::2, 6], A[0::2, 7], b[0::2] = x, y, 1.0, -X * x, -X * y, X
    A[1::2, 3], A[1::2, 4], A[1::2, 5], A[1::2, 6], A[1::2, 7], b[1::2] = x, y, 1.0, -Y * x, -Y * y, Y
    hn = np.linalg.lstsq(A, b, rcond=None)[0]
    h, ok = rf._denormalise([np.float64(v) for v in hn], [np.float64(v) for v in box])
    assert ok
    return h.reshape(3, 3), np.linalg.cond(A.T @ A)


@pytest.mark.parametrize("m,noise,seed", LSTSQ_CASES)
def test_normal_equations_against_lstsq(m, noise, seed):
    pts, _, _ = rr.planted(m, 1.0, noise, seed)
    H, ok, _, _ = rf.fit_ref(pts)
    Hl, cond = lstsq_fit(pts)
    err = rf.corner_error(H, Hl)
    print("m = %d: %.3e px from lstsq, condition number %.1f" % (m, err, cond))
    assert ok and err < LSTSQ_TOL_PX and cond < 100.0


def test_round_rule_on_a_noisy_case():
    pts, H_true, _ = rr.planted(1000, 0.3, 1.0, 1)
    H0, best, inl0, _, _ = rr.ransac_homography(pts, 256, 7, 3.0)
    assert best >= 0
    R = 4
    for form in ("vector", "scalar"):
        H, inl, rounds, counts = rf.refit_ref(pts, H0, 3.0, R, form)
        assert counts[0] == len(inl0) and counts == [34, 149, 300, 300]
        assert all(b >= a for a, b in zip(counts, counts[1:]))           # no round was discarded here
        assert rounds == len(counts) - 1 and (counts[rounds] == counts[rounds - 1] or rounds == R)
        assert len(inl) == counts[rounds] and (np.diff(inl) > 0).all() and inl.dtype == np.int32
        assert rf.corner_error(H, H_true) < 0.5 < 50.0 < rf.corner_error(H0, H_true)   # 0.27 px from 68.6 px
    one = rf.refit_ref(pts, H0, 3.0, 1)
    assert one[2] == 1 and one[3] == [34, 149]
    assert one[0].tobytes() == rf.fit_ref(pts, inl0)[0].tobytes()


def collinear_points(n=60):
    t = np.linspace(0.0, 1.0, n)
    pts = np.zeros(n, dtype=rr.POINT_PAIR_DTYPE)
    pts["qx"], pts["qy"] = 100.0 + 3000.0 * t, 200.0 + 1500.0 * t
    hom = np.stack([pts["qx"], pts["qy"], np.ones(n)], 1) @ rr.PLANTED_H.T
    pts["tx"], pts["ty"] = hom[:, 0] / hom[:, 2], hom[:, 1] / hom[:, 2]
    return pts


def test_degenerate_inputs():
    same = np.zeros(10, dtype=rr.POINT_PAIR_DTYPE)
    same[:] = (5.0, 6.0, 7.0, 8.0)
    for form in ("scalar", "vector"):
        H, ok, box, _ = rf.fit_ref(same, None, form)
        assert not ok and not H.any() and box[2] == 0.0 and box[5] == 0.0
    line = collinear_points()
    H, inl, rounds, counts = rf.refit_ref(line, rr.PLANTED_H, 3.0, 4)
    assert counts[0] == 60 and rounds == 0 and len(inl) == 60            # invalid, or rejected by its count
    assert H.tobytes() == rr.PLANTED_H.tobytes()
    pts, _, _ = rr.planted(200, 0.5, 0.5, 9)
    assert not rf.fit_ref(pts[:3])[1] and not rf.fit_ref(pts, [1, 2, 3])[1]
    H0 = rr.ransac_homography(pts, 64, 1, 3.0)[0]
    H, inl, rounds, counts = rf.refit_ref(pts, H0, 3.0, 0)
    assert rounds == 0 and H.tobytes() == H0.tobytes() and counts == [len(inl)] and len(inl) > 50
    H, inl, rounds, counts = rf.refit_ref(pts, np.zeros((3, 3)), 3.0, 4)
    assert rounds == 0 and not H.any() and len(inl) == 0 and counts == [0]
    H, inl, rounds, counts = rf.refit_ref(pts[:3], H0, 3.0, 4)
    assert rounds == 0 and H.tobytes() == H0.tobytes() and counts == [len(inl)]


def test_nan_pairs_never_reach_a_sum():
    pts, _, _ = rr.planted(300, 0.6, 0.5, 12)
    H0 = rr.ransac_homography(pts, 64, 2, 3.0)[0]
    bad = pts.copy()
    holes = np.flatnonzero(rr.inliers_ref(pts, H0.reshape(1, 9), 3.0)[0])[:5]
    for i, f in zip(holes, ("qx", "qy", "tx", "ty", "qx")):
        bad[f][i] = np.nan
    H, inl, rounds, counts = rf.refit_ref(bad, H0, 3.0, 4)
    assert rounds >= 1 and np.isfinite(H).all() and not set(holes.tolist()) & set(inl.tolist())
