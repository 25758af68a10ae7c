"""RANSAC homography verification on the device (sift_homography_*,
sift_pair_points_device, sift_verify_features) against
its numpy definition (tests/ransac_ref.py).

The definition is exact -- fp64 + - * / without contraction, integer counts --
so every comparison is array equality: the bytes of every H, every count, the
best index, the inlier list.  Shapes are the smallest that reach each way the
kernels can go wrong: one pair, the 64-lane and 1024-pair block edges, one and
several hypothesis tiles of 64 with a partial last one, more than one pair
block adding into one counter.
"""
import ctypes

import numpy as np
import pytest

import match_ref as mr
import ransac_ref as rr
import sift_amd
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

_planted = {}
IDENT = np.eye(3).reshape(1, 9)


def points_of(rows):
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    p = np.zeros(len(a), dtype=sift_amd.POINT_PAIR_DTYPE)
    p["qx"], p["qy"], p["tx"], p["ty"] = a.T
    return p


def planted_case(ctx, n, share, K, seed):
    """The points, the GPU result with its hypotheses, and the reference, once per case."""
    key = (n, share, K, seed)
    if key not in _planted:
        pts, _, is_in = rr.planted(n, share, 0.5, seed)
        got = ctx.ransac_homography(pts, K, seed, 3.0)
        hyp = ctx.homography_hypotheses()
        _planted[key] = dict(pts=pts, is_in=is_in, got=got, hyp=hyp, ref=rr.ransac_homography(pts, K, seed, 3.0))
    return _planted[key]


def assert_result(got, ref):
    H, best, inl = got
    assert H.tobytes() == ref[0].tobytes()
    assert best == ref[1]
    assert inl.dtype == np.int32
    np.testing.assert_array_equal(inl, ref[2])


def assert_none(got):
    H, best, inl = got
    assert best == -1 and H.shape == (3, 3) and not H.any() and len(inl) == 0


# ---- the score seam ------------------------------------------------------------
def test_the_comparison_is_strict_and_w_must_be_positive(gpu_ctx):
    pair = points_of([[10.0, 20.0, 13.0, 24.0]])              # residual exactly 3-4-5
    assert gpu_ctx.score_homographies(pair, IDENT, 5.0).tolist() == [0]
    assert gpu_ctx.score_homographies(pair, IDENT, np.nextafter(5.0, 6.0)).tolist() == [1]
    same = points_of([[10.0, 20.0, 10.0, 20.0]])
    assert gpu_ctx.score_homographies(same, IDENT, 5.0).tolist() == [1]
    assert gpu_ctx.score_homographies(same, -IDENT, 5.0).tolist() == [0]      # h[8] = -1: w = -1, zero residual
    w0 = np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0, 0]])                          # w == 0
    assert gpu_ctx.score_homographies(same, w0, 5.0).tolist() == [0]
    assert gpu_ctx.score_homographies(points_of([[0.0, 0.0, 0.0, 0.0]]), w0, 5.0).tolist() == [0]


def test_nan_and_inf_count_zero(gpu_ctx):
    pts, _, _ = rr.planted(130, 1.0, 0.0, 4)
    H = np.repeat(rr.PLANTED_H.reshape(1, 9), 20, axis=0)
    for j in range(9):
        H[j, j] = np.nan
        H[9 + j, j] = np.inf
    H[18, 8] = -np.inf
    got = gpu_ctx.score_homographies(pts, H, 3.0)
    np.testing.assert_array_equal(got, rr.score_ref(pts, H, 3.0))
    assert (got[:9] == 0).all() and got[19] == 130
    bad = pts.copy()
    for i, f in enumerate(bad.dtype.names):
        bad[f][10 * i] = np.nan
        bad[f][10 * i + 5] = np.inf
    got = gpu_ctx.score_homographies(bad, H[19:], 3.0)
    assert got.tolist() == [122] == rr.score_ref(bad, H[19:], 3.0).tolist()
    allnan = np.full(4 * 70, np.nan).view(sift_amd.POINT_PAIR_DTYPE)
    assert gpu_ctx.score_homographies(allnan, H[19:], 3.0).tolist() == [0]


@pytest.mark.parametrize("K", [1, 63, 65, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_score_tile_edges(gpu_ctx, n, K):
    pts, _, _ = rr.planted(n, 0.5, 2.0, 100 + n)
    rng = np.random.default_rng(200 + K)
    H = np.repeat(rr.PLANTED_H.reshape(1, 9), K, axis=0)
    H[:, [2, 5]] += rng.uniform(-3.0, 3.0, (K, 2))            # shifted by up to the threshold either way
    want = rr.score_ref(pts, H, 3.0)
    if n >= 63 and K >= 63:
        assert 0 < want.max() < n and len(set(want.tolist())) > 3             # neither all nor none
    np.testing.assert_array_equal(gpu_ctx.score_homographies(pts, H, 3.0), want)


# ---- the hypotheses ------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 64, 257])
@pytest.mark.parametrize("n", [4, 5, 64, 1000])
def test_hypotheses(gpu_ctx, n, K):
    pts, _, _ = rr.planted(n, 0.7, 0.5, 300 + n)
    for seed in (0, 2**64 - 12345):
        got = gpu_ctx.ransac_homography(pts, K, seed, 3.0)
        H, counts = gpu_ctx.homography_hypotheses()
        ref = rr.ransac_homography(pts, K, seed, 3.0)
        assert H.shape == (K, 3, 3) and H.tobytes() == ref[3].tobytes()
        np.testing.assert_array_equal(counts, ref[4])
        assert_result(got, ref)


def test_duplicated_pairs_make_invalid_hypotheses(gpu_ctx):
    pts, _, _ = rr.planted(12, 0.5, 0.5, 3)
    pts[[5, 7, 9, 11]] = pts[3]
    got = gpu_ctx.ransac_homography(pts, 64, 5, 3.0)
    H, counts = gpu_ctx.homography_hypotheses()
    ref = rr.ransac_homography(pts, 64, 5, 3.0)
    assert 0 < (ref[4] == -1).sum() < 64
    assert H.tobytes() == ref[3].tobytes()
    np.testing.assert_array_equal(counts, ref[4])
    assert not H[counts == -1].any() and (H[counts >= 0][:, 2, 2] == 1.0).all()
    assert_result(got, ref)


# ---- RANSAC ----------------------------------------------------------------------
CASES = [(500, 0.6, 256, 1), (5000, 0.3, 1024, 2)]


@pytest.mark.parametrize("n,share,K,seed", CASES)
def test_ransac_equals_the_reference(gpu_ctx, n, share, K, seed):
    c = planted_case(gpu_ctx, n, share, K, seed)
    ref = c["ref"]
    assert ref[1] >= 0 and len(ref[2]) >= 0.9 * c["is_in"].sum()          # not a vacuous case
    assert_result(c["got"], ref)
    H, counts = c["hyp"]
    assert H.tobytes() == ref[3].tobytes()
    np.testing.assert_array_equal(counts, ref[4])
    inl = c["got"][2]
    assert (np.diff(inl) > 0).all() and len(inl) == counts[c["got"][1]]


@pytest.mark.parametrize("n,share,K,seed", CASES)
def test_ransac_is_repeatable_and_follows_the_seed(gpu_ctx, n, share, K, seed):
    c = planted_case(gpu_ctx, n, share, K, seed)
    again = gpu_ctx.ransac_homography(c["pts"], K, seed, 3.0)
    H2, counts2 = gpu_ctx.homography_hypotheses()
    for a, b in zip(again, c["got"]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert H2.tobytes() == c["hyp"][0].tobytes() and counts2.tobytes() == c["hyp"][1].tobytes()
    other = gpu_ctx.ransac_homography(c["pts"], K, seed + 1000, 3.0)
    assert_result(other, rr.ransac_homography(c["pts"], K, seed + 1000, 3.0))
    assert other[1] != c["got"][1] and other[1] >= 0


# ---- edges -----------------------------------------------------------------------
def test_small_inputs(gpu_ctx):
    pts, _, _ = rr.planted(4, 1.0, 0.0, 11)
    assert_none(gpu_ctx.ransac_homography(pts[:0], 16, 0, 3.0))
    assert len(gpu_ctx.homography_hypotheses()[1]) == 0
    assert_none(gpu_ctx.ransac_homography(pts[:3], 16, 0, 3.0))
    assert_none(gpu_ctx.ransac_homography(pts, 0, 0, 3.0))
    assert len(gpu_ctx.homography_hypotheses()[1]) == 0
    got = gpu_ctx.ransac_homography(pts, 16, 0, 3.0)
    ref = rr.ransac_homography(pts, 16, 0, 3.0)
    assert_result(got, ref)
    assert got[1] == 0 and got[2].tolist() == [0, 1, 2, 3]
    assert len(gpu_ctx.score_homographies(pts, IDENT[:0], 3.0)) == 0
    assert gpu_ctx.score_homographies(pts[:0], IDENT, 3.0).tolist() == [0]


def test_identical_pairs_return_none(gpu_ctx):
    pts = points_of(np.tile([[100.0, 200.0, 110.0, 190.0]], (70, 1)))
    assert_none(gpu_ctx.ransac_homography(pts, 100, 3, 3.0))
    H, counts = gpu_ctx.homography_hypotheses()
    assert len(counts) == 100 and (counts == -1).all() and not H.any()
    assert_none(rr.ransac_homography(pts, 100, 3, 3.0)[:3])


def test_count_alone_capacity_and_bad_arguments(gpu_ctx):
    L, h = sift_amd.lib(), gpu_ctx._h
    c = planted_case(gpu_ctx, *CASES[0])
    pts, ref = c["pts"], c["ref"]
    n_ref = len(ref[2])
    p = pts.ctypes.data_as(ctypes.c_void_p)
    m, n = sift_amd.Homography(), ctypes.c_size_t(99)
    mp = ctypes.byref(m)
    assert L.sift_homography_ransac(h, p, 500, 256, 1, 3.0, mp, None, 0, ctypes.byref(n)) == 0    # a count alone
    assert n.value == n_ref and m.hypothesis == ref[1] and m.inliers == n_ref
    assert np.array(m.h).tobytes() == ref[0].tobytes()
    assert gpu_ctx.verify_timings()["select_ms"] > 0
    out = np.full(500, 7, dtype=np.int32)
    o = out.ctypes.data_as(ctypes.c_void_p)
    n.value = 99
    rc = L.sift_homography_ransac(h, p, 500, 256, 1, 3.0, mp, o, n_ref - 1, ctypes.byref(n))
    assert rc == sift_amd.SIFT_E_CAPACITY and n.value == n_ref and (out == 7).all()
    assert L.sift_homography_ransac(h, p, 500, 256, 1, 3.0, mp, o, n_ref, ctypes.byref(n)) == 0
    np.testing.assert_array_equal(out[:n_ref], ref[2])
    assert (out[n_ref:] == 7).all()

    sentinel = sift_amd.Homography((ctypes.c_double * 9)(*[5.0] * 9), 77, 88)
    m, n.value = sentinel, 99
    mp = ctypes.byref(m)
    out[:] = 7
    counts = np.full(4, 7, dtype=np.int32)
    cp = counts.ctypes.data_as(ctypes.c_void_p)
    Hs = np.repeat(IDENT, 4, axis=0)
    hp = Hs.ctypes.data_as(ctypes.c_void_p)
    E = sift_amd.SIFT_E_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.sift_homography_ransac(h, p, 500, 256, 1, bad, mp, o, 500, ctypes.byref(n)) == E
        assert L.sift_homography_ransac_device(h, p, 500, 256, 1, bad, mp, o, 500, ctypes.byref(n)) == E
        assert L.sift_homography_score(h, p, 500, hp, 4, bad, cp) == E
        assert L.sift_homography_score_device(h, p, 500, hp, 4, bad, cp) == E
        assert L.sift_verify_features(h, h, p, 500, 256, 1, bad, mp, o, 500, ctypes.byref(n)) == E
    for fn in (L.sift_homography_ransac, L.sift_homography_ransac_device):
        assert fn(h, p, 500, 65537, 1, 3.0, mp, o, 500, ctypes.byref(n)) == E
        assert fn(h, p, 2**31 - 1, 256, 1, 3.0, mp, o, 500, ctypes.byref(n)) == E
        assert fn(h, None, 500, 256, 1, 3.0, mp, o, 500, ctypes.byref(n)) == E
        assert fn(h, p, 500, 256, 1, 3.0, None, o, 500, ctypes.byref(n)) == E
        assert fn(None, p, 500, 256, 1, 3.0, mp, o, 500, ctypes.byref(n)) == E
    for fn in (L.sift_homography_score, L.sift_homography_score_device):
        assert fn(h, p, 500, hp, 65537, 3.0, cp) == E
        assert fn(h, None, 500, hp, 4, 3.0, cp) == E
        assert fn(h, p, 500, None, 4, 3.0, cp) == E
        assert fn(h, p, 500, hp, 4, 3.0, None) == E
    assert L.sift_verify_features(h, None, p, 500, 256, 1, 3.0, mp, o, 500, ctypes.byref(n)) == E
    assert L.sift_pair_points_device(h, None, p, 500, p) == E
    assert L.sift_copy_homography_hypotheses(None, None, None, 0, None) == E
    assert n.value == 99 and (out == 7).all() and (counts == 7).all()
    assert (m.hypothesis, m.inliers) == (77, 88) and list(m.h) == [5.0] * 9
    with sift_amd.Context(0) as fresh:
        assert L.sift_copy_homography_hypotheses(fresh._h, None, None, 0, ctypes.byref(n)) == sift_amd.SIFT_E_STATE
        assert L.sift_pair_points_device(fresh._h, fresh._h, None, 0, None) == sift_amd.SIFT_E_STATE
        rc = L.sift_verify_features(fresh._h, fresh._h, p, 500, 256, 1, 3.0, mp, o, 500, ctypes.byref(n))
        assert rc == sift_amd.SIFT_E_STATE
    Hh = np.zeros((255, 9))
    rc = L.sift_copy_homography_hypotheses(h, Hh.ctypes.data_as(ctypes.c_void_p), None, 255, ctypes.byref(n))
    assert rc == sift_amd.SIFT_E_CAPACITY and n.value == 256 and not Hh.any()


def test_device_forms_equal_the_host_forms(gpu_ctx):
    import torch
    L, h = sift_amd.lib(), gpu_ctx._h
    c = planted_case(gpu_ctx, *CASES[1])
    pts, ref = c["pts"], c["ref"]
    n_ref = len(ref[2])
    d_pts = torch.from_numpy(pts.view(np.float64).reshape(-1, 4).copy()).cuda()
    d_inl = torch.full((5000,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m, n = sift_amd.Homography(), ctypes.c_size_t()
    rc = L.sift_homography_ransac_device(h, d_pts.data_ptr(), 5000, 1024, 2, 3.0, ctypes.byref(m), d_inl.data_ptr(),
                                         5000, ctypes.byref(n))
    assert rc == 0 and n.value == n_ref and m.hypothesis == ref[1] and m.inliers == n_ref
    assert np.array(m.h).tobytes() == ref[0].tobytes()
    inl = d_inl.cpu().numpy()
    np.testing.assert_array_equal(inl[:n_ref], ref[2])
    assert (inl[n_ref:] == 7).all()
    rc = L.sift_homography_ransac_device(h, d_pts.data_ptr(), 5000, 1024, 2, 3.0, ctypes.byref(m), d_inl.data_ptr(),
                                         n_ref - 1, ctypes.byref(n))
    assert rc == sift_amd.SIFT_E_CAPACITY and n.value == n_ref
    t = gpu_ctx.verify_timings()
    assert t["hypotheses_ms"] > 0 and t["score_ms"] > 0 and t["select_ms"] > 0

    d_H = torch.from_numpy(ref[3].copy()).cuda()
    d_counts = torch.full((1024,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.sift_homography_score_device(h, d_pts.data_ptr(), 5000, d_H.data_ptr(), 1024, 3.0, d_counts.data_ptr()) == 0
    want = rr.score_ref(pts, ref[3], 3.0)
    np.testing.assert_array_equal(d_counts.cpu().numpy(), want)
    np.testing.assert_array_equal(gpu_ctx.score_homographies(pts, ref[3], 3.0), want)
    np.testing.assert_array_equal(np.where(ref[4] >= 0, want, -1), ref[4])


# ---- end to end ---------------------------------------------------------------------
def test_end_to_end(gpu_ctx):
    """Two 256 x 256 crops of blob_image(288, 288, seed=1), the second one 8
    pixels to the right and 16 down: multiples of 2^(O-1) = 4, so that every
    octave's grid lines up and interior features repeat exactly."""
    p = sift_amd.make_params(3, 4)
    big = blob_image(288, 288, seed=1)
    a, b = big[:256, :256], big[16:272, 8:264]
    K, seed, thresh = 512, 9, 3.0
    with sift_amd.Context(0) as other:
        feats = []
        for ctx, img in ((gpu_ctx, a), (other, b)):
            kp = ctx.detect(np.ascontiguousarray(img), p)
            ori = ctx.orient()
            ctx.describe()
            feats.append((kp, ori))
        (kpa, oria), (kpb, orib) = feats
        fwd, rev = gpu_ctx.match_features(other), other.match_features(gpu_ctx)
        pairs = gpu_ctx.select_matches(fwd, rev, 0.8)
        assert len(pairs) > 50

        patched = pairs.copy()
        patched["query"][3] = len(oria)
        patched["train"][5] = -1
        want_pts = rr.pair_points_ref(patched, oria, kpa, orib, kpb)
        got_pts = gpu_ctx.pair_points(other, patched)
        np.testing.assert_array_equal(got_pts.view(np.float64), want_pts.view(np.float64))
        assert np.isnan(got_pts.view(np.float64).reshape(-1, 4)[[3, 5]]).all()
        assert np.isfinite(np.delete(got_pts.view(np.float64).reshape(-1, 4), [3, 5], axis=0)).all()

        pts = rr.pair_points_ref(pairs, oria, kpa, orib, kpb)
        got = gpu_ctx.verify_features(other, pairs, K, seed, thresh)
        ref = rr.ransac_homography(pts, K, seed, thresh)
        assert_result(got, ref)
        assert_result(gpu_ctx.ransac_homography(pts, K, seed, thresh), ref)
        H, best, inl = got
        assert best >= 0 and len(inl) > len(pairs) / 2
        for x, y in ((0.0, 0.0), (255.0, 0.0), (0.0, 255.0), (255.0, 255.0)):
            u, v, w = H @ np.array([x, y, 1.0])
            assert np.hypot(u / w - (x - 8.0), v / w - (y - 16.0)) < thresh
        t = gpu_ctx.verify_timings()
        assert t["hypotheses_ms"] > 0 and t["score_ms"] > 0 and t["select_ms"] > 0
        with sift_amd.Context(0) as fresh:
            with pytest.raises(sift_amd.SiftError) as e:
                gpu_ctx.verify_features(fresh, pairs, K, seed, thresh)
            assert e.value.code == sift_amd.SIFT_E_STATE


# ---- the mechanisms the feature, match and verify stages share -------------------------
def test_selection_and_inliers_at_the_scan_edges(gpu_ctx):
    """Selection and RANSAC at the 256-item edges of the flag grids and of the
    n + 1 scan.  Every second query is a train row, so that the ratio test accepts
    some records and rejects the others; every planted pair is an inlier, so the
    total is n.  Sizes descending, then ascending, on the one context: the pinned
    count word and the grown flag / offset buffers are reused by a smaller list."""
    cases = {}
    for nq, n in ((1, 4), (255, 255), (256, 256), (257, 257)):
        query = np.random.default_rng(400 + nq).integers(0, 256, (nq, 128), dtype=np.uint8)
        train = np.random.default_rng(500 + nq).integers(0, 256, (300, 128), dtype=np.uint8)
        k = (nq + 1) // 2
        train[:k] = query[::2]
        fwd = gpu_ctx.match(query, train)
        want = {r: mr.select_ref(fwd, None, r) for r in (0.0, 0.8)}
        assert len(want[0.0]) == nq and len(want[0.8]) == k
        pts, _, _ = rr.planted(n, 1.0, 0.0, 600 + n)
        ref = rr.ransac_homography(pts, 64, 600 + n, 3.0)
        assert ref[1] >= 0 and len(ref[2]) == n
        cases[nq] = (fwd, want, pts, ref, n)
    for nq in (257, 256, 255, 1, 255, 256, 257):
        fwd, want, pts, ref, n = cases[nq]
        for ratio in (0.0, 0.8):
            got = gpu_ctx.select_matches(fwd, None, ratio)
            assert got.dtype == want[ratio].dtype and got.tobytes() == want[ratio].tobytes(), (nq, ratio)
        assert_result(gpu_ctx.ransac_homography(pts, 64, 600 + n, 3.0), ref)


def test_stages_keep_their_own_state(gpu_ctx):
    """Feature, match and verify results and timings on one context survive the
    other stages' calls (which share one pinned read-back and one scan scratch)."""
    L, h = sift_amd.lib(), gpu_ctx._h
    p = sift_amd.make_params(3, 4)
    with sift_amd.Context(0) as other:
        for ctx, seed in ((gpu_ctx, 1), (other, 2)):
            ctx.detect(blob_image(256, 256, seed=seed), p)
            ctx.orient()
            ctx.describe()
        ori, (desc, ok) = gpu_ctx.orient(), gpu_ctx.describe()
        fwd, rev = gpu_ctx.match_features(other), other.match_features(gpu_ctx)
        pairs = gpu_ctx.select_matches(fwd, rev, 0.0)
        assert len(ori) > 100 and ok.sum() > 100 and len(pairs) >= 4
        model = gpu_ctx.verify_features(other, pairs, 128, 5, 3.0)
        assert len(gpu_ctx.homography_hypotheses()[1]) == 128
        ft, mt, vt = gpu_ctx.feature_timings(), gpu_ctx.match_timings(), gpu_ctx.verify_timings()
        assert min(ft.values()) > 0 and min(mt.values()) > 0 and min(vt.values()) > 0

        n = ctypes.c_size_t(99)                                               # a count alone
        f = fwd.ctypes.data_as(ctypes.c_void_p)
        assert L.sift_match_select_host(h, f, len(fwd), None, len(rev), 0.0, None, 0, ctypes.byref(n)) == 0
        assert n.value == len(mr.select_ref(fwd, None, 0.0)) >= len(pairs)
        assert gpu_ctx.match_timings()["match_ms"] == mt["match_ms"]
        assert gpu_ctx.feature_timings() == ft and gpu_ctx.verify_timings() == vt

        pts, _, _ = rr.planted(4, 1.0, 0.0, 11)
        assert_result(gpu_ctx.ransac_homography(pts, 16, 0, 3.0), rr.ransac_homography(pts, 16, 0, 3.0))
        assert gpu_ctx.match_timings()["match_ms"] == mt["match_ms"]
        assert len(gpu_ctx.homography_hypotheses()[1]) == 16                  # that run's K, not the earlier one's
        vt4 = gpu_ctx.verify_timings()

        assert gpu_ctx.orient().tobytes() == ori.tobytes()                    # served from the context
        assert gpu_ctx.feature_timings() == ft
        desc2, ok2 = gpu_ctx.describe()
        assert desc2.tobytes() == desc.tobytes() and ok2.tobytes() == ok.tobytes()
        assert gpu_ctx.match_features(other).tobytes() == fwd.tobytes()
        assert gpu_ctx.verify_timings() == vt4
        again = gpu_ctx.verify_features(other, pairs, 128, 5, 3.0)
        for a, b in zip(again, model):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
