"""Guided descriptor matching on the device (sift_match_guided*, DESIGN.md
section 18) against its numpy definition (tests/guided_ref.py).

The records are a lexicographic minimum of integer keys over a set that fp64
comparisons with fixed roundings define, and the three info sums are integers:
every comparison is array equality of all four fields and of the sums; there is
nothing to tolerate.  The cases are the smallest that reach each way the
kernels can go wrong: the 64-lane rounds of the position test and of the
candidate queue, the `<=` of the radius, cell borders and margins, the edges of
the image and of the grid, unprojected rows and non-finite numbers, ties, masks
and the cell cap.
"""
import ctypes

import numpy as np
import pytest

import guided_ref as gr
import match_ref as mr
import sift_amd
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

NONE = (-1, -1, mr.NONE_D2, mr.NONE_D2)
EYE = np.eye(3)
DP = ctypes.POINTER(ctypes.c_double)
_persp = {}


def assert_same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for f in got.dtype.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def random_rows(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 128), dtype=np.uint8)


def check(ctx, query, qxy, train, txy, size, h, radius, qm=None, tm=None):
    """The device records and info of one call, after comparing both with the reference."""
    got = ctx.match_guided(query, qxy, train, txy, size, h, radius, qm, tm)
    info = ctx.guided_info()
    want, want_info = gr.info_ref(query, qxy, train, txy, size[0], size[1], h, radius, qm, tm)
    assert_same(got, want)
    assert info == want_info
    return got, info


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (2, 1), (65, 1023), (0, 5), (5, 0)])
def test_a_degenerate_grid_is_the_brute_force_match(gpu_ctx, nq, nt):
    rng = np.random.default_rng(10 * nq + nt)
    query, train = random_rows(100 + nq, nq), random_rows(200 + nt, nt)
    qxy, txy = rng.uniform(0, 100, (nq, 2)), rng.uniform(0, 100, (nt, 2))
    got, info = check(gpu_ctx, query, qxy, train, txy, (100, 100), EYE, 1e9)
    assert_same(got, mr.match_ref(query, train))
    assert_same(got, gpu_ctx.match(query, train))
    assert (info["cell_px"], info["ncx"], info["ncy"]) == (100, 1, 1)
    assert info["n_projected"] == nq and info["n_visited"] == info["n_candidates"] == nq * nt
    if nt == 0:
        assert all(tuple(r) == NONE for r in got)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 63, 64, 65, 129])
def test_candidate_counts_at_the_edges_of_a_wave(gpu_ctx, k, spread):
    """One query at the centre of cell (8, 8) of the 16 x 16 grid of a 256 x 256 image, radius 16: k train rows
    inside the disc, in that cell alone or over the nine cells the disc reaches, and 200 outside it."""
    rng = np.random.default_rng(1000 + 2 * k + spread)
    centre = np.array([136.0, 136.0])
    ang, rad = rng.uniform(0, 2 * np.pi, k), rng.uniform(0, 7.9 if not spread else 15.9, k)
    inside = centre + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    if spread and k >= 9:
        inside[:9] = centre + np.array([(dx, dy) for dx in (-10, 0, 10) for dy in (-10, 0, 10)], dtype=np.float64)
    far = rng.uniform(0, 256, (4000, 2))
    far = far[np.hypot(*(far - centre).T) > 16.5][:200]
    txy = np.concatenate([inside, far])
    order = rng.permutation(len(txy))
    txy = txy[order]
    train = random_rows(1200 + k, len(txy))
    query = random_rows(1300 + k, 1)
    got, info = check(gpu_ctx, query, centre[None], train, txy, (256, 256), EYE, 16.0)
    assert (info["cell_px"], info["ncx"], info["ncy"]) == (16, 16, 16)
    assert info["n_candidates"] == k and info["n_projected"] == 1
    assert (got["best"][0] >= 0) == (k >= 1) and (got["second"][0] >= 0) == (k >= 2)
    cells = set(map(tuple, (inside // 16).astype(int)))
    assert len(cells) == 9 if spread and k >= 9 else not k or spread or cells == {(8, 8)}


# 3 ---------------------------------------------------------------------------------------------------------------
NA = float(np.nextafter(5.0, 6.0))
MUST = [(3.0, 4.0), (-4.0, 3.0), (5.0, 0.0), (0.0, -5.0)]
DECOYS = [(4.0, 4.0), (7.5, 0.0), (-7.5, 0.0), (0.0, 7.5), (0.0, -7.5)]      # outside; the last four in margin cells
AXIS_DECOYS = [(NA, 0.0), (-NA, 0.0), (0.0, NA), (0.0, -NA)]                  # one ulp beyond the radius


@pytest.mark.parametrize("p,decoys", [((48.5, 47.5), DECOYS), ((50.0, 50.0), DECOYS), ((52.25, 44.75), DECOYS),
                                       ((2.0, 2.5), DECOYS + AXIS_DECOYS)])
def test_the_radius_is_less_or_equal(gpu_ctx, p, decoys):
    """r = 5 on 5-pixel cells.  From (48.5, 47.5) each of the four points at distance exactly 5 lies across a cell
    border; from (50, 50) they lie on borders.  The decoys carry the query's own bytes, so any that was admitted
    would win at distance 0.  (2, 2.5) makes p + nextafter(5, 6) exact in fp64."""
    p = np.array(p)
    query = random_rows(31, 1)
    dxy = p + np.array(decoys)
    if len(decoys) > len(DECOYS):
        assert dxy[5, 0] - p[0] == NA and p[0] - dxy[6, 0] == NA and dxy[7, 1] - p[1] == NA and p[1] - dxy[8, 1] == NA
    must = p + np.array(MUST)
    if tuple(p) == (48.5, 47.5):
        assert ((must // 5 != p // 5).any(1)).all()
    train = np.concatenate([random_rows(32, 4), np.repeat(query, len(decoys), 0)])
    got, info = check(gpu_ctx, query, p[None], train, np.concatenate([must, dxy]), (100, 100), EYE, 5.0)
    assert info["cell_px"] == 5 and info["n_candidates"] == 4 and info["n_visited"] >= 4
    assert got["d2_best"][0] > 0 and {got["best"][0], got["second"][0]} <= {0, 1, 2, 3}
    for j in range(4):                                   # each one alone, in front of the decoys and behind them
        for first in (True, False):
            txy = np.concatenate([must[j:j + 1], dxy] if first else [dxy, must[j:j + 1]])
            rows = np.concatenate([train[j:j + 1], train[4:]] if first else [train[4:], train[j:j + 1]])
            got, info = check(gpu_ctx, query, p[None], rows, txy, (100, 100), EYE, 5.0)
            assert tuple(got[0])[:2] == (0 if first else len(decoys), -1) and info["n_candidates"] == 1


# 4 ---------------------------------------------------------------------------------------------------------------
def test_edges_of_the_image(gpu_ctx):
    W, H, r = 131, 257, 6.0
    rng = np.random.default_rng(4)
    qxy = np.array([(-3.0, -3.0), (W + 2.0, H / 2), (W - 1.0, H - 1.0), (0.0, 0.0), (W + 0.0, H + 0.0), (65.0, 128.0)])
    planted = np.array([(-4.0, -2.0), (-8.5, -3.0), (W + 3.5, H / 2 + 1), (W + 7.0, H / 2), (W - 1.0, H - 1.0),
                        (W + 4.0, H + 3.0), (-0.0, -5.5)])
    txy = np.concatenate([planted, rng.uniform(-10, 1, (150, 2)), rng.uniform((-10, -10), (W + 10, H + 10), (900, 2)),
                          rng.uniform((W - 8, H - 8), (W + 10, H + 10), (150, 2))])
    train, query = random_rows(41, len(txy)), random_rows(42, len(qxy))
    got, info = check(gpu_ctx, query, qxy, train, txy, (W, H), EYE, r)
    assert (info["cell_px"], info["ncx"], info["ncy"]) == (6, 22, 43) and W % 6 and H % 6
    assert (got["best"][:5] >= 0).all() and info["n_projected"] == 6
    cand0 = np.flatnonzero(gr.candidates(-3.0, -3.0, txy, np.ones(len(txy), bool), r))
    assert 0 in cand0 and 1 in cand0                       # train points at negative coordinates
    cand1 = np.flatnonzero(gr.candidates(W + 2.0, H / 2, txy, np.ones(len(txy), bool), r))
    assert 2 in cand1 and 3 in cand1                       # ... and beyond W


# 5 ---------------------------------------------------------------------------------------------------------------
def test_unprojected_rows_and_bad_numbers(gpu_ctx):
    rng = np.random.default_rng(5)
    nq, nt = 300, 500
    query, train = random_rows(51, nq), random_rows(52, nt)
    qxy, txy = rng.uniform(0, 100, (nq, 2)), rng.uniform(0, 100, (nt, 2))
    qxy[0] = (20.0, 50.0)                                   # w == 0 under the matrix below
    half = [1, 0, 0, 0, 1, 0, 0.05, 0, -1.0]                # w = 0.05 x - 1: > 0 right of x = 20 only
    got, info = check(gpu_ctx, query, qxy, train, txy, (100, 100), half, 30.0)
    front = 0.05 * qxy[:, 0] - 1.0 > 0
    assert 0 < info["n_projected"] == front.sum() < nq and info["n_candidates"] > 0
    assert all(tuple(r) == NONE for r in got[~front]) and tuple(got[0]) == NONE

    bad = np.eye(3)
    bad[0, 1] = np.nan
    for h in (bad, np.zeros(9)):
        got, info = check(gpu_ctx, query, qxy, train, txy, (100, 100), h, 30.0)
        assert all(tuple(r) == NONE for r in got)
        assert (info["n_projected"], info["n_visited"], info["n_candidates"]) == (0, 0, 0)

    qxy2, txy2 = qxy.copy(), txy.copy()
    qxy2[1], qxy2[2], qxy2[3], qxy2[4] = (np.nan, 5), (5, np.nan), (np.inf, 5), (5, -np.inf)
    txy2[::7, 0] = np.nan
    txy2[3::7, 1] = np.nan
    txy2[5] = (np.inf, 50.0)
    train2 = train.copy()
    train2[::7] = query[10]                                 # the NaN rows would win for query 10
    got, info = check(gpu_ctx, query, qxy2, train2, txy2, (100, 100), EYE, 25.0)
    assert all(tuple(got[q]) == NONE for q in (1, 2, 3, 4)) and info["n_projected"] == nq - 4
    assert got["best"][10] >= 0 and got["best"][10] % 7 != 0 and not np.isin(got["best"], np.arange(0, nt, 7)).any()

    qxy3 = qxy.copy()
    qxy3[7] = (1e300, 40.0)
    qxy3[8] = (-1e300, 1e300)
    got, info = check(gpu_ctx, query, qxy3, train2, txy2, (100, 100), EYE, 1e300)
    filed = int((~np.isnan(txy2).any(1)).sum())
    assert info["n_projected"] == nq and info["n_visited"] == info["n_candidates"] == nq * filed
    assert got["best"][7] >= 0 and got["best"][8] >= 0     # dx * dx = inf <= r2 = inf
    got, info = check(gpu_ctx, query, qxy3, train2, txy2, (100, 100), EYE, 30.0)
    assert tuple(got[7]) == NONE and tuple(got[8]) == NONE  # projected, and nothing near


# 6 ---------------------------------------------------------------------------------------------------------------
def test_ties_take_the_lowest_indices_across_cells(gpu_ctx):
    rng = np.random.default_rng(6)
    nt = 120
    train = random_rows(61, nt)
    txy = rng.uniform(0, 128, (nt, 2))
    at = {10: (45.0, 50.0), 50: (50.0, 50.0), 90: (57.0, 50.0)}          # columns 5, 6 and 7 of 8-pixel cells
    for i, p in at.items():
        train[i], txy[i] = train[10], p
    assert len({int(p[0] // 8) for p in at.values()}) == 3
    query, qxy = train[10:11].copy(), np.array([(50.0, 50.0)])
    got, info = check(gpu_ctx, query, qxy, train, txy, (128, 128), EYE, 8.0)
    assert tuple(got[0]) == (10, 50, 0, 0) and info["cell_px"] == 8
    got, _ = check(gpu_ctx, query, qxy, train[::-1].copy(), txy[::-1].copy(), (128, 128), EYE, 8.0)
    assert tuple(got[0]) == (nt - 1 - 90, nt - 1 - 50, 0, 0)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_masks(gpu_ctx):
    rng = np.random.default_rng(7)
    train = random_rows(8, 700)
    zero_rows = np.arange(0, 700, 7)
    train[zero_rows] = 0
    tm = np.ones(700, np.uint8)
    tm[zero_rows] = 0                                       # the rows that would otherwise win
    query = rng.integers(0, 4, (70, 128), dtype=np.uint8)
    qm = np.ones(70, np.uint8)
    qm[[0, 13, 31, 32, 69]] = 0
    qxy, txy = rng.uniform(20, 44, (70, 2)), rng.uniform(0, 64, (700, 2))
    unmasked, _ = check(gpu_ctx, query, qxy, train, txy, (64, 64), EYE, 20.0)
    assert np.isin(unmasked["best"], zero_rows).all()
    got, info = check(gpu_ctx, query, qxy, train, txy, (64, 64), EYE, 20.0, qm, tm)
    assert not np.isin(got["best"], zero_rows).any() and (got["best"][qm != 0] >= 0).all()
    assert info["n_projected"] == 65
    for q in (0, 13, 31, 32, 69):
        assert tuple(got[q]) == NONE
    one = np.zeros(700, np.uint8)
    one[333] = 1
    got, info = check(gpu_ctx, query, qxy, train, txy, (64, 64), EYE, 1e9, None, one)
    assert (got["best"] == 333).all() and (got["second"] == -1).all() and info["n_visited"] == 70
    got, info = check(gpu_ctx, query, qxy, train, txy, (64, 64), EYE, 20.0, None, np.zeros(700, np.uint8))
    assert all(tuple(r) == NONE for r in got) and info["n_visited"] == 0


# 8, 9 ------------------------------------------------------------------------------------------------------------
PERSP = np.array([[1.02, 0.01, -3.0], [-0.015, 0.99, 4.0], [2e-5, -1e-5, 1.0]])


def persp(ctx):
    """Case 8's data, its device records and info, and the reference, once."""
    if not _persp:
        rng = np.random.default_rng(8)
        nq, nt = 2000, 3000
        query, train = random_rows(81, nq), random_rows(82, nt)
        qxy, txy = rng.uniform((0, 0), (1024, 768), (nq, 2)), rng.uniform((0, 0), (1024, 768), (nt, 2))
        qm, tm = rng.integers(0, 20, nq) != 0, rng.integers(0, 20, nt) != 0
        got = ctx.match_guided(query, qxy, train, txy, (1024, 768), PERSP, 12.0, qm, tm)
        info = ctx.guided_info()
        ref, ref_info = gr.info_ref(query, qxy, train, txy, 1024, 768, PERSP, 12.0, qm, tm)
        _persp.update(query=query, train=train, qxy=qxy, txy=txy, qm=qm, tm=tm, got=got, info=info, ref=ref,
                      ref_info=ref_info)
    return _persp


def test_a_perspective_homography(gpu_ctx):
    c = persp(gpu_ctx)
    assert_same(c["got"], c["ref"])
    assert c["info"] == c["ref_info"]
    n_best, n_second = (c["ref"]["best"] >= 0).sum(), (c["ref"]["second"] >= 0).sum()
    assert 0 < n_second < n_best < 2000                     # rows with no, one and several candidates
    again = gpu_ctx.match_guided(c["query"], c["qxy"], c["train"], c["txy"], (1024, 768), PERSP, 12.0, c["qm"],
                                 c["tm"])
    assert again.tobytes() == c["got"].tobytes() and gpu_ctx.guided_info() == c["info"]
    t = gpu_ctx.guided_timings()
    assert t["grid_ms"] > 0 and t["match_ms"] > 0


def test_the_grid_prunes(gpu_ctx):
    c = persp(gpu_ctx)
    info = c["info"]
    assert (info["cell_px"], info["ncx"], info["ncy"]) == gr.grid_ref(1024, 768, 12.0) == (12, 86, 64)
    assert info["n_visited"] == c["ref_info"]["n_visited"] >= info["n_candidates"] > 0
    # a condition, not a measurement: at most 5 x 5 cells of 12 px, below 0.5 % of the image
    assert info["n_visited"] * 16 < info["n_projected"] * 3000


# 10 --------------------------------------------------------------------------------------------------------------
def test_the_cell_cap(gpu_ctx):
    rng = np.random.default_rng(10)
    n = 500
    txy = rng.uniform(0, 40000, (n, 2))
    txy[100:110] = txy[100] + rng.uniform(-1.5, 1.5, (10, 2))            # a cluster
    qxy = txy[rng.permutation(n)] + rng.uniform(-1.1, 1.1, (n, 2))
    query, train = random_rows(101, n), random_rows(102, n)
    got, info = check(gpu_ctx, query, qxy, train, txy, (40000, 40000), EYE, 1.0)
    assert (info["cell_px"], info["ncx"], info["ncy"]) == (40, 1000, 1000)
    assert info["ncx"] * info["ncy"] <= sift_amd.GUIDED_MAX_CELLS
    assert 0 < (got["best"] >= 0).sum() < n and (got["second"] >= 0).any()


# 11 --------------------------------------------------------------------------------------------------------------
def test_arguments(gpu_ctx):
    import torch
    L, ctx = sift_amd.lib(), gpu_ctx._h
    rng = np.random.default_rng(11)
    query, train = random_rows(111, 40), random_rows(112, 300)
    qxy, txy = rng.uniform(0, 50, (40, 2)), rng.uniform(0, 50, (300, 2))
    hm = np.eye(3).reshape(9)
    h = hm.ctypes.data_as(DP)
    too_many = 2**31 - 1
    E = sift_amd.SIFT_E_ARG

    def bad_calls(fn, q, qx, t, tx, o):
        assert fn(ctx, None, None, qx, 40, t, None, tx, 300, 50, 50, h, 5.0, o) == E
        assert fn(ctx, q, None, None, 40, t, None, tx, 300, 50, 50, h, 5.0, o) == E
        assert fn(ctx, q, None, qx, 40, None, None, tx, 300, 50, 50, h, 5.0, o) == E
        assert fn(ctx, q, None, qx, 40, t, None, None, 300, 50, 50, h, 5.0, o) == E
        assert fn(ctx, q, None, qx, 40, t, None, tx, 300, 50, 50, h, 5.0, None) == E
        assert fn(ctx, q, None, qx, 40, t, None, tx, 300, 50, 50, None, 5.0, o) == E
        assert fn(ctx, q, None, qx, too_many, t, None, tx, 300, 50, 50, h, 5.0, o) == E
        assert fn(ctx, q, None, qx, 40, t, None, tx, too_many, 50, 50, h, 5.0, o) == E
        for radius in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            assert fn(ctx, q, None, qx, 40, t, None, tx, 300, 50, 50, h, radius, o) == E
        for w, hh in ((0, 50), (50, 0), (-1, 50), (50, -7)):
            assert fn(ctx, q, None, qx, 40, t, None, tx, 300, w, hh, h, 5.0, o) == E
        assert fn(None, q, None, qx, 40, t, None, tx, 300, 50, 50, h, 5.0, o) == E

    out = np.full(40, 7, dtype=sift_amd.MATCH_DTYPE)
    host = [a.ctypes.data_as(ctypes.c_void_p) for a in (query, qxy, train, txy, out)]
    bad_calls(L.sift_match_guided, *host)
    assert (out.view(np.int32) == 7).all()

    dev = [torch.from_numpy(a).cuda() for a in (query, qxy, train, txy)]
    pad_q = torch.zeros(40 * 128 + 16, dtype=torch.uint8, device="cuda")
    d_out = torch.full((40 * 4,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs = [a.data_ptr() for a in dev] + [d_out.data_ptr()]
    bad_calls(L.sift_match_guided_device, *ptrs)
    fn = L.sift_match_guided_device                                        # misaligned rows, either side
    assert fn(ctx, pad_q.data_ptr() + 1, None, ptrs[1], 40, ptrs[2], None, ptrs[3], 300, 50, 50, h, 5.0, ptrs[4]) == E
    assert fn(ctx, ptrs[0], None, ptrs[1], 40, pad_q.data_ptr() + 8, None, ptrs[3], 40, 50, 50, h, 5.0, ptrs[4]) == E
    assert (d_out.cpu().numpy() == 7).all()

    assert L.sift_match_features_guided(ctx, None, h, 5.0, None, 0, None) == E
    assert L.sift_last_guided_info(ctx, None) == E and L.sift_last_guided_info(None, None) == E
    assert L.sift_last_guided_timings(None, None, None) == E
    with sift_amd.Context(0) as fresh:
        assert L.sift_last_guided_info(fresh._h, ctypes.byref(sift_amd.GuidedInfo())) == sift_amd.SIFT_E_STATE
        assert fresh.guided_timings() == dict(grid_ms=0.0, match_ms=0.0)

    # the device form equals the host form, writes d_out alone and leaves the last match what it was
    before = gpu_ctx.match(query[:3], train)
    assert fn(ctx, ptrs[0], None, ptrs[1], 40, ptrs[2], None, ptrs[3], 300, 50, 50, h, 5.0, ptrs[4]) == 0
    got = d_out.cpu().numpy().view(sift_amd.MATCH_DTYPE)
    assert gpu_ctx.device_matches()[1] == 3
    want, _, _ = gr.guided_ref(query, qxy, train, txy, hm, 5.0)
    assert_same(got, want)
    assert_same(gpu_ctx.match_guided(query, qxy, train, txy, (50, 50), hm, 5.0), want)
    assert gpu_ctx.device_matches()[1] == 40 and len(before) == 3


# 12 --------------------------------------------------------------------------------------------------------------
def features(ctx):
    kp, ori = ctx.keypoints(), ctx.orient()
    desc, ok = ctx.describe()
    return desc, ok, np.stack([kp["abs_x"][ori["keypoint"]], kp["abs_y"][ori["keypoint"]]], 1)


def test_end_to_end(gpu_ctx):
    import torch
    L = sift_amd.lib()
    p = sift_amd.make_params(3, 4)
    img = blob_image(256, 256, seed=1)
    shift = np.array([[1.0, 0, 5], [0, 1.0, 3], [0, 0, 1.0]])            # x + 5, y + 3
    with sift_amd.Context(0) as other:
        gpu_ctx.detect(img, p)                                            # a list without descriptors
        for a in (other, gpu_ctx):
            with pytest.raises(sift_amd.SiftError) as e:
                a.match_features_guided(other, shift, 3.0)
            assert e.value.code == sift_amd.SIFT_E_STATE
        d1, ok1, xy1 = features(gpu_ctx)
        with pytest.raises(sift_amd.SiftError) as e:
            gpu_ctx.match_features_guided(other, shift, 3.0)              # the train side has none yet
        assert e.value.code == sift_amd.SIFT_E_STATE
        other.detect(np.roll(img, (3, 5), axis=(0, 1)), p)
        d2, ok2, xy2 = features(other)
        assert ok1.sum() > 100 and ok2.sum() > 100

        got = gpu_ctx.match_features_guided(other, shift, 3.0)
        info = gpu_ctx.guided_info()
        want, want_info = gr.info_ref(d1, xy1, d2, xy2, 256, 256, shift, 3.0, ok1, ok2)
        assert_same(got, want)
        assert info == want_info and (got["best"] >= 0).sum() > 50

        d_fwd, n = gpu_ctx.device_matches()
        assert n == len(d1)
        d_pairs = torch.zeros(max(n, 1) * 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cnt = ctypes.c_size_t()
        assert L.sift_match_select(gpu_ctx._h, d_fwd, n, None, len(d2), 0.8, d_pairs.data_ptr(), n,
                                   ctypes.byref(cnt)) == 0
        pairs = d_pairs.cpu().numpy().view(sift_amd.PAIR_DTYPE)[:cnt.value]
        assert_same(pairs, mr.select_ref(want, None, 0.8))
        assert len(pairs) > 20
        pts = gpu_ctx.pair_points(other, pairs)
        np.testing.assert_array_equal(pts["qx"], xy1[pairs["query"], 0])
        np.testing.assert_array_equal(pts["ty"], xy2[pairs["train"], 1])
        H, hyp, rounds, inl = gpu_ctx.verify_features_refit(other, pairs, hypotheses=256, seed=1)
        assert hyp >= 0 and len(inl) >= 4 and np.isfinite(H).all()

        wide = gpu_ctx.match_features_guided(other, shift, 1e9)
        assert_same(wide, gpu_ctx.match_features(other))
        assert_same(wide, mr.match_ref(d1, d2, ok1, ok2))
