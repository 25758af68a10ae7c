"""The least-squares homography fit and the refit of the RANSAC inliers on the
device (sift_homography_fit*, sift_homography_refit*, sift_verify_features_refit;
DESIGN.md section 14) against their numpy definition (tests/refit_ref.py).

The definition fixes every rounding and the order of every addition, so every
comparison is on bytes: the matrix, the box, each of the 44 sums, the rounds and
the inlier list.  The sizes are the edges of the summation tree: one partial
chunk, exactly one chunk, one more; 4096 = 64^2 and 262145 = 64^3 + 1, where a
second and a third level begin and where padding appears at each level.
"""
import ctypes

import numpy as np
import pytest

import ransac_ref as rr
import refit_ref as rf
import sift_amd
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

DP = ctypes.POINTER(ctypes.c_double)
_cases = {}


def assert_fit(ctx, got, ref):
    """A fit_homography result and the context's box and sums against fit_ref's."""
    H, ok = got
    assert ok == ref[1]
    assert H.tobytes() == ref[0].tobytes()
    box, sums = ctx.homography_fit_sums()
    assert box.tobytes() == ref[2].tobytes(), (box, ref[2])
    wrong = [rf.PAIRS[q] for q in np.flatnonzero(sums.view(np.uint64) != ref[3].view(np.uint64))]
    assert not wrong, "sums (j, k) that differ: %s" % wrong


def assert_refit(got, ref):
    H, rounds, inl = got
    assert H.tobytes() == ref[0].tobytes()
    assert rounds == ref[2]
    assert inl.dtype == np.int32 and inl.tobytes() == ref[1].tobytes()


def device_points(pts):
    import torch
    d = torch.from_numpy(pts.view(np.float64).reshape(-1, 4).copy()).cuda()
    torch.cuda.synchronize()
    return d


def fit_device(ctx, d_pts, n, d_idx=None, m=0):
    h, ok = np.zeros(9), ctypes.c_int(7)
    rc = sift_amd.lib().sift_homography_fit_device(ctx._h, d_pts.data_ptr() if n else None, n,
                                                   None if d_idx is None else d_idx.data_ptr(), m,
                                                   h.ctypes.data_as(DP), ctypes.byref(ok))
    assert rc == 0
    return h.reshape(3, 3), bool(ok.value)


def refit_case(n, share, K, seed, noise, data_seed):
    """Points, the reference RANSAC model and the reference refit, once per case."""
    key = (n, share, K, seed, noise, data_seed)
    if key not in _cases:
        pts, H_true, _ = rr.planted(n, share, noise, data_seed)
        ran = rr.ransac_homography(pts, K, seed, 3.0)
        _cases[key] = dict(pts=pts, H_true=H_true, ransac=ran, ref=rf.refit_ref(pts, ran[0], 3.0, 4))
    return _cases[key]


# ---- the fit seam -----------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 5, 63, 64, 65, 4095, 4096, 4097, 262145])
def test_fit_at_the_edges_of_the_tree(gpu_ctx, m):
    pts, H_true, _ = rr.planted(m, 1.0, 0.5, 700 + m % 1000)
    ref = rf.fit_ref(pts)
    assert ref[1] and (m < 63 or rf.corner_error(ref[0], H_true) < 1.0)       # a real fit, not a degenerate one
    assert_fit(gpu_ctx, gpu_ctx.fit_homography(pts), ref)


def test_index_lists(gpu_ctx):
    n = 1000
    pts, _, _ = rr.planted(n, 1.0, 0.5, 21)
    whole = gpu_ctx.fit_homography(pts)
    explicit = gpu_ctx.fit_homography(pts, np.arange(n))
    assert explicit[1] and explicit[0].tobytes() == whole[0].tobytes()
    rng = np.random.default_rng(22)
    lists = dict(third=np.arange(0, n, 3), descending=np.arange(n)[::-1], repeated=rng.integers(0, n, 700),
                 permuted=rng.permutation(n), four=np.array([5, 900, 17, 333]))
    for name, idx in lists.items():
        ref = rf.fit_ref(pts, idx)
        assert ref[1], name
        assert_fit(gpu_ctx, gpu_ctx.fit_homography(pts, idx), ref)
    # the order is part of the definition: the permuted list's sums are not the ascending list's
    assert rf.fit_ref(pts, lists["permuted"])[3].tobytes() != rf.fit_ref(pts)[3].tobytes()


def test_repeatable_and_device_form_equals_host_form(gpu_ctx):
    import torch
    n = 5000
    pts, _, _ = rr.planted(n, 1.0, 0.5, 23)
    idx = np.random.default_rng(24).permutation(n)[:4321].astype(np.int32)
    a = gpu_ctx.fit_homography(pts, idx)
    sa = gpu_ctx.homography_fit_sums()
    b = gpu_ctx.fit_homography(pts, idx)
    sb = gpu_ctx.homography_fit_sums()
    assert a[1] and b[1] and a[0].tobytes() == b[0].tobytes()
    assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes()
    d_pts = device_points(pts)
    d_idx = torch.from_numpy(idx.copy()).cuda()
    torch.cuda.synchronize()
    c = fit_device(gpu_ctx, d_pts, n, d_idx, len(idx))
    sc = gpu_ctx.homography_fit_sums()
    assert c[1] and c[0].tobytes() == a[0].tobytes() and sc[1].tobytes() == sa[1].tobytes()
    assert_fit(gpu_ctx, c, rf.fit_ref(pts, idx))
    assert_fit(gpu_ctx, fit_device(gpu_ctx, d_pts, n), rf.fit_ref(pts))       # d_index == NULL: 0 .. n-1


def test_a_device_list_entry_outside_the_pairs_is_not_read(gpu_ctx):
    import torch
    n = 200
    pts, _, _ = rr.planted(n, 1.0, 0.5, 25)
    d_pts = device_points(pts)
    for bad in (n, -1, 2**31 - 1):
        idx = np.arange(100, dtype=np.int32)
        idx[70] = bad
        d_idx = torch.from_numpy(idx).cuda()
        torch.cuda.synchronize()
        H, ok = fit_device(gpu_ctx, d_pts, n, d_idx, 100)
        assert not ok and not H.any()
    d_idx = torch.arange(100, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert_fit(gpu_ctx, fit_device(gpu_ctx, d_pts, n, d_idx, 100), rf.fit_ref(pts, np.arange(100)))


def test_degenerate_fits(gpu_ctx):
    L, h = sift_amd.lib(), gpu_ctx._h
    pts, _, _ = rr.planted(100, 1.0, 0.5, 26)
    gpu_ctx.fit_homography(pts)
    for few in (pts[:0], pts[:3]):
        H, ok = gpu_ctx.fit_homography(few)
        assert not ok and not H.any()
        assert L.sift_copy_homography_fit_sums(h, None, None) == sift_amd.SIFT_E_STATE   # it formed no sums
    H, ok = gpu_ctx.fit_homography(pts, [1, 2, 3])
    assert not ok and not H.any()
    same = np.zeros(70, dtype=sift_amd.POINT_PAIR_DTYPE)
    same[:] = (100.0, 200.0, 110.0, 190.0)
    H, ok = gpu_ctx.fit_homography(same)
    assert not ok and not H.any() and not rf.fit_ref(same)[1]
    box, _ = gpu_ctx.homography_fit_sums()
    assert box.tolist() == [100.0, 200.0, 0.0, 110.0, 190.0, 0.0]
    allnan = np.full(4 * 70, np.nan).view(sift_amd.POINT_PAIR_DTYPE)
    H, ok = gpu_ctx.fit_homography(allnan)
    assert not ok and not H.any()


# ---- the refit ----------------------------------------------------------------------
# (n, inlier share, K, RANSAC seed, noise, seed of the planted data): the two CASES of tests/test_gpu_verify.py, the
# same shape with 30 % inliers and noise 1.0 (where 256 hypotheses find 6 inliers and the refit cannot help), and the
# case of tests/test_refit_ref.py, whose counts go 34 -> 149 -> 300 -> 300.
REFIT_CASES = [(500, 0.6, 256, 1, 0.5, 1), (5000, 0.3, 1024, 2, 0.5, 2), (1000, 0.3, 256, 7, 1.0, 7),
               (1000, 0.3, 256, 7, 1.0, 1)]
GROWING = REFIT_CASES[3]


@pytest.mark.parametrize("n,share,K,seed,noise,data_seed", REFIT_CASES)
def test_refit_equals_the_reference(gpu_ctx, n, share, K, seed, noise, data_seed):
    c = refit_case(n, share, K, seed, noise, data_seed)
    H0, best, inl0, _, _ = c["ransac"]
    got0 = gpu_ctx.ransac_homography(c["pts"], K, seed, 3.0)
    assert got0[0].tobytes() == H0.tobytes() and best >= 0
    got = gpu_ctx.refit_homography(c["pts"], got0[0], 3.0, 4)
    assert_refit(got, c["ref"])
    assert (np.diff(got[2]) > 0).all() and len(got[2]) >= len(inl0)
    assert rf.corner_error(got[0], c["H_true"]) < rf.corner_error(H0, c["H_true"])
    again = gpu_ctx.refit_homography(c["pts"], got0[0], 3.0, 4)
    for a, b in zip(again, got):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_the_refit_cases_are_not_vacuous():
    c = refit_case(*GROWING)
    H, inl, rounds, counts = c["ref"]
    assert rounds >= 2 and len(inl) > len(c["ransac"][2]) and counts == [34, 149, 300, 300]


def test_rounds(gpu_ctx):
    c = refit_case(*GROWING)
    pts, (H0, _, inl0, _, _) = c["pts"], c["ransac"]
    H, rounds, inl = gpu_ctx.refit_homography(pts, H0, 3.0, 0)
    assert rounds == 0 and H.tobytes() == H0.tobytes() and inl.tobytes() == inl0.tobytes()
    assert gpu_ctx.refit_timings() == dict(fit_ms=0.0, rescore_ms=0.0)
    assert_refit(gpu_ctx.refit_homography(pts, H0, 3.0, 1), rf.refit_ref(pts, H0, 3.0, 1))
    t = gpu_ctx.refit_timings()
    assert t["fit_ms"] > 0 and t["rescore_ms"] > 0
    assert gpu_ctx.refit_homography(pts, H0, 3.0, 1)[0].tobytes() == rf.fit_ref(pts, inl0)[0].tobytes()
    assert_refit(gpu_ctx.refit_homography(pts, H0, 3.0, 16), rf.refit_ref(pts, H0, 3.0, 16))
    H0s = H0 * 2.0                                                            # h[8] as given: the same inliers
    assert_refit(gpu_ctx.refit_homography(pts, H0s, 3.0, 0), rf.refit_ref(pts, H0s, 3.0, 0))
    assert_refit(gpu_ctx.refit_homography(pts, H0s, 3.0, 4), rf.refit_ref(pts, H0s, 3.0, 4))


def test_a_refit_that_loses_inliers_is_rejected(gpu_ctx):
    """50 pairs on one line that PLANTED_H maps exactly, and 50 scattered outliers.  The normal matrix of collinear
    points is singular up to rounding, so the fit is whatever the rounding leaves: on this line it is valid but keeps
    none of the 50 inliers (counts 50 -> 0 in the reference), the round is discarded and the start comes back.  (Other
    lines give a fit that keeps all 50 and is accepted; this one was chosen on the CPU because the reference rejects.)"""
    t = np.linspace(0.0, 1.0, 50)
    pts, _, _ = rr.planted(100, 0.0, 0.0, 31)
    pts["qx"][::2], pts["qy"][::2] = 500.0 + 2500.0 * t, 1800.0 - 1500.0 * t
    hom = np.stack([pts["qx"][::2], pts["qy"][::2], np.ones(50)], 1) @ rr.PLANTED_H.T
    pts["tx"][::2], pts["ty"][::2] = hom[:, 0] / hom[:, 2], hom[:, 1] / hom[:, 2]
    ref = rf.refit_ref(pts, rr.PLANTED_H, 3.0, 4)
    assert ref[2] == 0 and ref[3] == [50, 0] and ref[1].tolist() == list(range(0, 100, 2))   # the reference rejects
    got = gpu_ctx.refit_homography(pts, rr.PLANTED_H, 3.0, 4)
    assert_refit(got, ref)
    assert got[0].tobytes() == rr.PLANTED_H.tobytes()
    t = gpu_ctx.refit_timings()
    assert t["fit_ms"] > 0 and t["rescore_ms"] > 0                            # the discarded round was tried


def test_small_inputs_none_model_and_nan_pairs(gpu_ctx):
    pts, _, _ = rr.planted(300, 0.6, 0.5, 12)
    H0 = rr.ransac_homography(pts, 64, 2, 3.0)[0]
    for sub in (pts[:0], pts[:3]):
        got = gpu_ctx.refit_homography(sub, H0, 3.0, 4)
        assert_refit(got, rf.refit_ref(sub, H0, 3.0, 4))
        assert got[1] == 0 and got[0].tobytes() == H0.tobytes()
        assert gpu_ctx.refit_timings() == dict(fit_ms=0.0, rescore_ms=0.0)
    H, rounds, inl = gpu_ctx.refit_homography(pts, np.zeros((3, 3)), 3.0, 4)  # a "none" model
    assert rounds == 0 and not H.any() and len(inl) == 0
    bad = pts.copy()
    holes = np.flatnonzero(rr.inliers_ref(pts, H0.reshape(1, 9), 3.0)[0])[:5]
    for i, f in zip(holes, ("qx", "qy", "tx", "ty", "qx")):
        bad[f][i] = np.nan
    ref = rf.refit_ref(bad, H0, 3.0, 4)
    got = gpu_ctx.refit_homography(bad, H0, 3.0, 4)
    assert_refit(got, ref)
    assert got[1] >= 1 and np.isfinite(got[0]).all() and not set(holes.tolist()) & set(got[2].tolist())
    _, sums = gpu_ctx.homography_fit_sums()
    assert np.isfinite(sums).all()                                            # no NaN pair reached a sum


def test_count_alone_capacity_and_bad_arguments(gpu_ctx):
    L, h = sift_amd.lib(), gpu_ctx._h
    c = refit_case(*REFIT_CASES[0])
    pts, ref, H0 = c["pts"], c["ref"], c["ransac"][0]
    n, n_ref = len(pts), len(ref[1])
    p = pts.ctypes.data_as(ctypes.c_void_p)
    start = sift_amd.Homography((ctypes.c_double * 9)(*H0.reshape(9)), 41, 0)
    sp = ctypes.byref(start)
    m, cnt, r = sift_amd.Homography(), ctypes.c_size_t(99), ctypes.c_int32(99)
    mp, cp, rp = ctypes.byref(m), ctypes.byref(cnt), ctypes.byref(r)
    assert L.sift_homography_refit(h, p, n, sp, 3.0, 4, mp, rp, None, 0, cp) == 0          # a count alone
    assert cnt.value == n_ref == m.inliers and r.value == ref[2] and m.hypothesis == 41
    assert np.array(m.h).tobytes() == ref[0].tobytes()
    out = np.full(n, 7, dtype=np.int32)
    o = out.ctypes.data_as(ctypes.c_void_p)
    cnt.value = 99
    rc = L.sift_homography_refit(h, p, n, sp, 3.0, 4, mp, rp, o, n_ref - 1, cp)
    assert rc == sift_amd.SIFT_E_CAPACITY and cnt.value == n_ref and (out == 7).all()
    assert np.array(m.h).tobytes() == ref[0].tobytes() and r.value == ref[2]
    assert L.sift_homography_refit(h, p, n, sp, 3.0, 4, mp, rp, o, n_ref, cp) == 0
    assert out[:n_ref].tobytes() == ref[1].tobytes() and (out[n_ref:] == 7).all()
    assert L.sift_homography_refit(h, p, n, sp, 3.0, 4, sp, None, None, 0, None) == 0      # refined may be start
    assert np.array(start.h).tobytes() == ref[0].tobytes() and start.hypothesis == 41 and start.inliers == n_ref
    start = sift_amd.Homography((ctypes.c_double * 9)(*H0.reshape(9)), 41, 0)
    sp = ctypes.byref(start)

    m = sift_amd.Homography((ctypes.c_double * 9)(*[5.0] * 9), 77, 88)
    mp = ctypes.byref(m)
    cnt.value, r.value = 99, 99
    out[:] = 7
    E = sift_amd.SIFT_E_ARG
    refits = (L.sift_homography_refit, L.sift_homography_refit_device)
    for fn in refits:
        for rounds in (-1, 17):
            assert fn(h, p, n, sp, 3.0, rounds, mp, rp, o, n, cp) == E
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(h, p, n, sp, bad, 4, mp, rp, o, n, cp) == E
        assert fn(h, p, 2**31 - 1, sp, 3.0, 4, mp, rp, o, n, cp) == E
        assert fn(h, None, n, sp, 3.0, 4, mp, rp, o, n, cp) == E
        assert fn(h, p, n, None, 3.0, 4, mp, rp, o, n, cp) == E
        assert fn(h, p, n, sp, 3.0, 4, None, rp, o, n, cp) == E
        assert fn(None, p, n, sp, 3.0, 4, mp, rp, o, n, cp) == E
    for rounds, thresh in ((-1, 3.0), (17, 3.0), (4, 0.0), (4, float("nan"))):
        assert L.sift_verify_features_refit(h, h, p, n, 256, 1, thresh, rounds, mp, rp, o, n, cp) == E
    assert L.sift_verify_features_refit(h, None, p, n, 256, 1, 3.0, 4, mp, rp, o, n, cp) == E
    hh, ok = np.full(9, 5.0), ctypes.c_int(7)
    hp, okp = hh.ctypes.data_as(DP), ctypes.byref(ok)
    for bad in (n, -1):
        idx = np.arange(10, dtype=np.int32)
        idx[4] = bad
        assert L.sift_homography_fit(h, p, n, idx.ctypes.data_as(ctypes.c_void_p), 10, hp, okp) == E
    for fn in (L.sift_homography_fit, L.sift_homography_fit_device):
        assert fn(h, None, n, None, 0, hp, okp) == E
        assert fn(h, p, n, None, 0, None, okp) == E
        assert fn(h, p, 2**31 - 1, None, 0, hp, okp) == E
        assert fn(None, p, n, None, 0, hp, okp) == E
    assert L.sift_copy_homography_fit_sums(None, None, None) == E
    assert L.sift_last_refit_timings(None, None, None) == E
    assert cnt.value == 99 and r.value == 99 and (out == 7).all() and (hh == 5.0).all() and ok.value == 7
    assert (m.hypothesis, m.inliers) == (77, 88) and list(m.h) == [5.0] * 9
    with sift_amd.Context(0) as fresh:
        assert L.sift_copy_homography_fit_sums(fresh._h, None, None) == sift_amd.SIFT_E_STATE
        rc = L.sift_verify_features_refit(fresh._h, fresh._h, p, n, 256, 1, 3.0, 4, mp, rp, o, n, cp)
        assert rc == sift_amd.SIFT_E_STATE
        assert fresh.refit_timings() == dict(fit_ms=0.0, rescore_ms=0.0)


def test_device_form_equals_the_host_form(gpu_ctx):
    import torch
    L, h = sift_amd.lib(), gpu_ctx._h
    c = refit_case(*REFIT_CASES[1])
    pts, ref, H0 = c["pts"], c["ref"], c["ransac"][0]
    n, n_ref = len(pts), len(ref[1])
    d_pts = device_points(pts)
    d_inl = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    start = sift_amd.Homography((ctypes.c_double * 9)(*H0.reshape(9)), 3, 0)
    m, cnt, r = sift_amd.Homography(), ctypes.c_size_t(), ctypes.c_int32()
    rc = L.sift_homography_refit_device(h, d_pts.data_ptr(), n, ctypes.byref(start), 3.0, 4, ctypes.byref(m),
                                        ctypes.byref(r), d_inl.data_ptr(), n, ctypes.byref(cnt))
    assert rc == 0 and cnt.value == n_ref == m.inliers and r.value == ref[2] and m.hypothesis == 3
    assert np.array(m.h).tobytes() == ref[0].tobytes()
    inl = d_inl.cpu().numpy()
    assert inl[:n_ref].tobytes() == ref[1].tobytes() and (inl[n_ref:] == 7).all()
    d_inl.fill_(7)
    torch.cuda.synchronize()
    rc = L.sift_homography_refit_device(h, d_pts.data_ptr(), n, ctypes.byref(start), 3.0, 4, ctypes.byref(m),
                                        ctypes.byref(r), d_inl.data_ptr(), n_ref - 1, ctypes.byref(cnt))
    assert rc == sift_amd.SIFT_E_CAPACITY and cnt.value == n_ref and (d_inl.cpu().numpy() == 7).all()
    assert_refit(gpu_ctx.refit_homography(pts, H0, 3.0, 4), ref)


# ---- end to end -----------------------------------------------------------------------
def test_verify_features_refit_end_to_end(gpu_ctx):
    """The two crops of tests/test_gpu_verify.py::test_end_to_end, same parameters."""
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
        pts = rr.pair_points_ref(pairs, oria, kpa, orib, kpb)
        H, best, rounds, inl = gpu_ctx.verify_features_refit(other, pairs, K, seed, thresh, 4)
        H0, best0, inl0 = gpu_ctx.verify_features(other, pairs, K, seed, thresh)
        ref0 = rr.ransac_homography(pts, K, seed, thresh)
        assert H0.tobytes() == ref0[0].tobytes() and best == best0 == ref0[1] >= 0
        ref = rf.refit_ref(pts, ref0[0], thresh, 4)
        assert_refit((H, rounds, inl), ref)
        assert_refit(gpu_ctx.refit_homography(pts, H0, thresh, 4), ref)
        assert len(inl) >= len(inl0) > len(pairs) / 2
        for x, y in ((0.0, 0.0), (255.0, 0.0), (0.0, 255.0), (255.0, 255.0)):
            u, v, w = H @ np.array([x, y, 1.0])
            assert np.hypot(u / w - (x - 8.0), v / w - (y - 16.0)) < thresh
        with sift_amd.Context(0) as fresh:
            with pytest.raises(sift_amd.SiftError) as e:
                gpu_ctx.verify_features_refit(fresh, pairs, K, seed, thresh, 4)
            assert e.value.code == sift_amd.SIFT_E_STATE


# ---- state ----------------------------------------------------------------------------
def test_refit_and_ransac_keep_their_own_state(gpu_ctx):
    c = refit_case(*REFIT_CASES[0])
    pts, K, seed = c["pts"], REFIT_CASES[0][2], REFIT_CASES[0][3]
    H0, _, _ = gpu_ctx.ransac_homography(pts, K, seed, 3.0)
    hyp = gpu_ctx.homography_hypotheses()
    vt = gpu_ctx.verify_timings()
    gpu_ctx.refit_homography(pts, H0, 3.0, 4)
    H2, counts2 = gpu_ctx.homography_hypotheses()
    assert H2.tobytes() == hyp[0].tobytes() and counts2.tobytes() == hyp[1].tobytes() and len(counts2) == K
    assert gpu_ctx.verify_timings() == vt
    other, _, _ = rr.planted(777, 1.0, 0.5, 41)
    ref = rf.fit_ref(other)
    got = gpu_ctx.fit_homography(other)
    rt = gpu_ctx.refit_timings()
    gpu_ctx.ransac_homography(pts, 64, seed, 3.0)                             # a RANSAC and a scoring in between
    gpu_ctx.score_homographies(pts, H0.reshape(1, 9), 3.0)
    assert_fit(gpu_ctx, got, ref)                                             # the fit's box and sums are intact
    assert gpu_ctx.refit_timings() == rt and min(rt.values()) >= 0.0
