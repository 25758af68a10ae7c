"""CPU checks of the RANSAC homography definition (tests/ransac_ref.py, the
restatement of include/sift_hip.h that the GPU tests compare against): its two
forms agree bitwise, and the properties the definition promises hold."""
import os
import re

import numpy as np
import pytest

import ransac_ref as rr
import sift_amd
from sift_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sift_pair_points_device", "sift_homography_ransac_device", "sift_homography_ransac",
               "sift_homography_score", "sift_homography_score_device", "sift_copy_homography_hypotheses",
               "sift_verify_features", "sift_last_verify_timings")


def points_of(rows):
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    p = np.zeros(len(a), dtype=rr.POINT_PAIR_DTYPE)
    p["qx"], p["qy"], p["tx"], p["ty"] = a.T
    return p


def test_the_mixer_is_the_one_of_synth():
    v = np.array([0, 1, 12345, 2**63 + 17, 2**64 - 1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        want = synth._splitmix64(v - np.uint64(rr.GOLDEN))
    np.testing.assert_array_equal(rr.mix_ref(v), want)
    assert [rr.mix_scalar(int(x)) for x in v] == [int(x) for x in want]


@pytest.mark.parametrize("n", [4, 5, 64, 10**6])
def test_samples_are_distinct_in_range_and_the_two_forms_agree(n):
    for seed in (0, 7, 2**64 - 1):
        s = rr.samples_ref(seed, 300, n)
        assert s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 4 for row in s.tolist())
        if n == 4:
            assert (np.sort(s, axis=1) == np.arange(4)).all()
            assert len({tuple(r) for r in s.tolist()}) > 10      # and not one permutation alone
        for k in (0, 1, 17, 299):
            assert rr.sample_scalar(seed, k, n) == s[k].tolist()


def test_the_two_forms_agree_bitwise():
    pts, _, _ = rr.planted(12, 0.5, 0.5, 3)
    pts[[5, 7, 9, 11]] = pts[3]                               # some samples draw two copies: invalid hypotheses
    H, valid = rr.hypotheses_ref(pts, 64, 5)
    assert 0 < valid.sum() < 64
    for k in range(64):
        h, ok = rr.hypothesis_scalar(pts, 5, k)
        assert ok == valid[k]
        assert h.tobytes() == H[k].tobytes(), k
    got = rr.ransac_homography(pts, 64, 5, 3.0)
    want = rr.ransac_scalar(pts, 64, 5, 3.0)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] >= 0
    np.testing.assert_array_equal(got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes()
    np.testing.assert_array_equal(got[4], want[4])
    assert (got[4][~valid] == -1).all() and (got[4][valid] >= 0).all()
    assert (np.diff(got[2]) > 0).all() and len(got[2]) == got[4][got[1]]


def test_an_integer_affine_map_comes_back_exactly():
    q = np.array([[0, 0], [8, 0], [0, 4], [8, 4]], dtype=np.float64)
    M = np.array([[2.0, 1.0, 3.0], [-1.0, 4.0, 5.0]])
    t = q @ M[:, :2].T + M[:, 2]
    pts = points_of(np.concatenate([q, t], axis=1))
    for k in range(24):
        for h, ok in (rr.hypothesis_scalar(pts, 1, k), [a[k] for a in rr.hypotheses_ref(pts, 24, 1)]):
            assert ok
            np.testing.assert_array_equal(h, [2.0, 1.0, 3.0, -1.0, 4.0, 5.0, 0.0, 0.0, 1.0])


def test_two_identical_pairs_in_a_sample_make_it_invalid():
    pts, _, _ = rr.planted(4, 1.0, 0.0, 9)
    pts[2] = pts[0]
    H, valid = rr.hypotheses_ref(pts, 16, 0)
    assert not valid.any() and not H.any()
    assert all(not rr.hypothesis_scalar(pts, 0, k)[1] for k in range(16))
    h, best, inl, _, counts = rr.ransac_homography(pts, 16, 0, 3.0)
    assert best == -1 and len(inl) == 0 and not h.any() and (counts == -1).all()
    assert rr.ransac_scalar(pts, 16, 0, 3.0)[1] == -1


def test_the_comparison_is_strict():
    ident = np.eye(3).reshape(1, 9)
    pts = points_of([[10.0, 20.0, 13.0, 24.0]])               # residual exactly 3-4-5
    above = np.nextafter(5.0, 6.0)
    assert rr.score_ref(pts, ident, 5.0)[0] == 0 and rr.score_ref(pts, ident, above)[0] == 1
    assert not rr.inlier_scalar(ident[0], 10.0, 20.0, 13.0, 24.0, 25.0)
    assert rr.inlier_scalar(ident[0], 10.0, 20.0, 13.0, 24.0, above * above)
    behind = -np.eye(3).reshape(1, 9)                         # w = -1: zero residual, never an inlier
    same = points_of([[10.0, 20.0, 10.0, 20.0]])
    assert rr.score_ref(same, ident, 5.0)[0] == 1 and rr.score_ref(same, behind, 5.0)[0] == 0
    nan = points_of([[np.nan, 20.0, 10.0, 20.0]])
    assert rr.score_ref(nan, ident, 5.0)[0] == 0


@pytest.mark.parametrize("n,share,K,seed", [(500, 0.6, 256, 1), (5000, 0.3, 1024, 2)])
def test_the_planted_model_is_found(n, share, K, seed):
    """The cases of tests/test_gpu_verify.py are not vacuous: the reference's
    best hypothesis gathers at least 0.9 of the planted inliers."""
    pts, _, is_in = rr.planted(n, share, 0.5, seed)
    _, best, inl, _, counts = rr.ransac_homography(pts, K, seed, 3.0)
    assert best >= 0 and len(inl) == counts[best]
    assert len(inl) >= 0.9 * is_in.sum()
    assert is_in[inl].sum() >= 0.9 * is_in.sum()


def test_small_and_empty_inputs():
    pts, _, _ = rr.planted(3, 1.0, 0.0, 1)
    for p, K in ((pts, 8), (pts[:0], 8), (rr.planted(10, 1.0, 0.0, 1)[0], 0)):
        h, best, inl, H, counts = rr.ransac_homography(p, K, 0, 3.0)
        assert best == -1 and not h.any() and len(inl) == 0 and len(H) == 0 and len(counts) == 0


def test_pair_points_ref():
    kp = np.zeros(3, dtype=sift_amd.KEYPOINT_DTYPE)
    kp["abs_x"], kp["abs_y"] = [1.0, 2.0, 3.0], [10.0, 20.0, 30.0]
    ori = np.zeros(4, dtype=sift_amd.ORIENTATION_DTYPE)
    ori["keypoint"] = [0, 0, 2, 1]
    pairs = np.zeros(3, dtype=sift_amd.PAIR_DTYPE)
    pairs["query"], pairs["train"] = [1, 2, 4], [3, 0, 0]
    got = rr.pair_points_ref(pairs, ori, kp, ori, kp)
    assert tuple(got[0]) == (1.0, 10.0, 2.0, 20.0) and tuple(got[1]) == (3.0, 30.0, 1.0, 10.0)
    assert all(np.isnan(v) for v in got[2].tolist())


def test_the_new_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "sift_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in sift_amd.ABI_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert rr.POINT_PAIR_DTYPE == sift_amd.POINT_PAIR_DTYPE and sift_amd.POINT_PAIR_DTYPE.itemsize == 32
    assert sift_amd.RANSAC_MAX_HYPOTHESES == rr.MAX_HYPOTHESES
