"""The keypoint budget on the device against its numpy restatement
(tests/budget_ref.py): every check is array equality of the kept index list."""
import ctypes

import numpy as np
import pytest

import budget_ref as br
import sift_amd
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

T = 2048                        # records one block handles (kBudgetTile, sift_kernels.h)
LDS_CELLS = 16                  # up to here the bins are kept in LDS (kBudgetLdsCells); above: global adds
SENTINEL = -0x5A5A5A5B
INT_MAX = 2**31 - 1
NAN, INF = float("nan"), float("inf")
VP = ctypes.c_void_p


def make_kp(values, xs=None, ys=None):
    kp = np.zeros(len(values), dtype=sift_amd.KEYPOINT_DTYPE)
    kp["interp_value"] = values
    kp["abs_x"] = 0.0 if xs is None else xs
    kp["abs_y"] = 0.0 if ys is None else ys
    return kp


def tied_values(rng, n):
    """Normal values, a third of them drawn from a small pool so that ties and special values occur."""
    pool = np.array([0.0, -0.0, NAN, INF, -INF, 5e-324, 1.0, -1.0, 0.25, -0.25])
    v = rng.normal(size=n)
    some = rng.random(n) < 0.33
    v[some] = pool[rng.integers(0, len(pool), int(some.sum()))]
    return v


def raw_host(ctx, kp, w, h, bud, cap=None, want_index=True, reserved=0, null_kp=False):
    """sift_keypoint_select on a sentinel-filled buffer: (rc, n_out, buffer)."""
    L = sift_amd.lib()
    k = np.ascontiguousarray(kp, dtype=sift_amd.KEYPOINT_DTYPE)
    n = k.shape[0]
    b = sift_amd.Budget(bud[0], bud[1], bud[2], reserved)
    cap = n if cap is None else cap
    buf = np.full(max(cap, n, 1) + 3, SENTINEL, dtype=np.int32)
    n_out = ctypes.c_size_t(12345)
    rc = L.sift_keypoint_select(ctx._h, None if null_kp or n == 0 else k.ctypes.data_as(VP), n, w, h, ctypes.byref(b),
                                buf.ctypes.data_as(VP) if want_index else None, cap, ctypes.byref(n_out))
    return rc, n_out.value, buf


def raw_device(ctx, kp, w, h, bud, cap=None, want_index=True):
    """sift_keypoint_select_device on torch's device memory: (rc, n_out, buffer)."""
    import torch
    L = sift_amd.lib()
    k = np.ascontiguousarray(kp, dtype=sift_amd.KEYPOINT_DTYPE)
    n = k.shape[0]
    b = sift_amd.Budget(bud[0], bud[1], bud[2], 0)
    cap = n if cap is None else cap
    d_kp = torch.from_numpy(k.view(np.uint8).reshape(-1).copy()).cuda()
    d_idx = torch.full((max(cap, n, 1) + 3,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n_out = ctypes.c_size_t(12345)
    rc = L.sift_keypoint_select_device(ctx._h, d_kp.data_ptr() if n else None, n, w, h, ctypes.byref(b),
                                       d_idx.data_ptr() if want_index else None, cap, ctypes.byref(n_out))
    return rc, n_out.value, d_idx.cpu().numpy()


def check(ctx, kp, w, h, bud, what="", run=raw_host):
    want = br.select(kp, w, h, bud)
    rc, m, buf = run(ctx, kp, w, h, bud)
    assert rc == 0, (what, bud, sift_amd.lib().sift_last_error(ctx._h))
    assert m == len(want), (what, bud, m, len(want))
    np.testing.assert_array_equal(buf[:m], want, err_msg="%s %s" % (what, bud))
    assert (buf[m:] == SENTINEL).all(), (what, bud)  # entries past *n_out are untouched
    return want


def quotas_at_every_threshold(k):
    """For every distinct key: the quotas that put the threshold at the first, a middle and the last of its records."""
    out = set()
    for v in np.unique(k):
        above, cnt = int((k > v).sum()), int((k == v).sum())
        out.update((above + 1, above + (cnt + 1) // 2, above + cnt))
    return sorted(out)


# ---- sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_sizes_and_totals(gpu_ctx, n):
    kp = make_kp(tied_values(np.random.default_rng(n), n))
    for max_total in (0, 1, n - 1, n, n + 1, INT_MAX, -1):
        check(gpu_ctx, kp, 64, 64, (max_total, 0, -1), "n=%d" % n)
    check(gpu_ctx, kp, 64, 64, (max(n // 3, 1), 0, -1), "n=%d device" % n, run=raw_device)


# ---- the radix passes, one by one ----------------------------------------------------------------------------------
BYTE_VALUES = (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF)
BASES = (0x3FE5A5A5A5A5A5A5,    # an ordinary number whichever byte changes
         0x7FF0000000000000)    # inf: a non-zero byte below the exponent makes a NaN, whose key is 0


def byte_keypoints(rng, base, byte, n=300):
    """n records whose interp_value bits equal `base` except in `byte` (0 = the top one), with random signs."""
    shift = 8 * (7 - byte)
    vals = [v for v in BYTE_VALUES if byte > 0 or v <= 0x7F]
    b = np.array(vals, dtype=np.uint64)[rng.integers(0, len(vals), n)]
    bits = (np.uint64(base) & ~(np.uint64(0xFF) << np.uint64(shift))) | (b << np.uint64(shift))
    bits |= rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)
    return bits.view(np.float64)


@pytest.mark.parametrize("byte", range(8))
@pytest.mark.parametrize("base", BASES)
def test_each_key_byte_decides(gpu_ctx, base, byte):
    rng = np.random.default_rng(100 + byte)
    v = byte_keypoints(rng, base, byte)
    kp = make_kp(v, rng.uniform(0, 40, len(v)), rng.uniform(0, 40, len(v)))
    k = br.keys(kp)
    assert len(np.unique(k)) >= 2
    for q in quotas_at_every_threshold(k):                  # one cell: the LDS bins
        check(gpu_ctx, kp, 40, 40, (q, 0, -1), "byte %d" % byte)
    assert br.grid(40, 40, 8)[0] ** 2 > LDS_CELLS            # 25 cells: the global bins
    for per_cell in (1, 3, 7):
        check(gpu_ctx, kp, 40, 40, (-1, 8, per_cell), "byte %d" % byte)


# ---- ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.75, NAN])
def test_all_keys_equal(gpu_ctx, value):
    n = 3 * T + 5
    rng = np.random.default_rng(5)
    kp = make_kp(np.full(n, value), rng.uniform(0, 64, n), rng.uniform(0, 64, n))
    for q in (1, T - 1, T, T + 1, 2 * T + 3, n - 1):
        want = check(gpu_ctx, kp, 64, 64, (q, 0, -1), "equal keys")
        np.testing.assert_array_equal(want, np.arange(q))
    check(gpu_ctx, kp, 64, 64, (-1, 16, 3), "equal keys, 16 cells")
    check(gpu_ctx, kp, 64, 64, (-1, 8, 3), "equal keys, 64 cells")
    check(gpu_ctx, kp, 64, 64, (T + 1, 8, 40), "equal keys, both steps")


@pytest.mark.parametrize("stronger", [0, 7])
def test_tie_run_across_a_block_boundary(gpu_ctx, stronger):
    n = 2 * T + 9
    rng = np.random.default_rng(6)
    v = rng.uniform(0.1, 0.2, n)
    v[T - 10:T + 10] = -0.5                                 # the run: records T-10 .. T+9
    v[rng.choice(np.r_[0:T - 10, T + 10:n], stronger, replace=False)] = 0.9
    kp = make_kp(v)
    for inside in (1, 9, 10, 11, 12, 19, 20):               # the quota ends inside the run, either side of the boundary
        want = check(gpu_ctx, kp, 8, 8, (stronger + inside, 0, -1), "tie run")
        assert sorted(set(want) & set(range(T - 10, T + 10))) == list(range(T - 10, T - 10 + inside))


# ---- the grid ------------------------------------------------------------------------------------------------------
def grid_kp(seed, n, w, h):
    rng = np.random.default_rng(seed)
    xs, ys = rng.uniform(-1.0, w + 1.0, n), rng.uniform(-1.0, h + 1.0, n)
    xs[rng.random(n) < 0.02] = NAN
    ys[rng.random(n) < 0.02] = NAN
    return make_kp(tied_values(rng, n), xs, ys)


@pytest.mark.parametrize("w,h,cell_px,what", [
    (16, 12, 16, "one cell"), (16, 12, 100, "one cell, larger than the frame"), (16, 12, 1, "192 cells of 1 px"),
    (20, 12, 8, "a partial last column and row"), (33, 17, 8, "5 x 3 cells, 15: the LDS bins"),
    (33, 25, 8, "5 x 4 cells, 20: the global bins")])
def test_grids(gpu_ctx, w, h, cell_px, what):
    kp = grid_kp(w * h + cell_px, 700, w, h)
    for per_cell in (0, 1, 2, 5, INT_MAX, -1):
        check(gpu_ctx, kp, w, h, (-1, cell_px, per_cell), what)
    for max_total, per_cell in ((0, 1), (1, 1), (10, 1), (10, 3), (150, 2), (5, -1), (5, 0)):
        check(gpu_ctx, kp, w, h, (max_total, cell_px, per_cell), what)
    check(gpu_ctx, kp, w, h, (37, cell_px, 2), what + " device", run=raw_device)


def test_cell_border_coordinates(gpu_ctx):
    w, h, c = br.BORDER_FRAME
    coords = np.array([x for x, _ in br.BORDER_X] * 3)
    v = np.r_[np.full(len(br.BORDER_X), 1.0), np.full(len(br.BORDER_X), 2.0), np.full(len(br.BORDER_X), 3.0)]
    for kp in (make_kp(v, coords, np.zeros(len(v))), make_kp(v, np.zeros(len(v)), coords),
               make_kp(v, coords, coords[::-1].copy())):
        for per_cell in (0, 1, 2, 4, -1):
            check(gpu_ctx, kp, w, h, (-1, c, per_cell), "borders")
        check(gpu_ctx, kp, w, h, (6, c, 2), "borders")


def test_step_two_tie_between_survivors_of_different_cells(gpu_ctx):
    xs = [1.0, 9.0, 2.0, 10.0, 3.0, 11.0]                   # cells 0, 1, 0, 1, 0, 1 of a 16 x 8 frame
    kp = make_kp([5.0, 5.0, 9.0, 1.0, 5.0, 5.0], xs, [0.0] * 6)
    assert check(gpu_ctx, kp, 16, 8, (-1, 8, 2)).tolist() == [0, 1, 2, 5]
    assert check(gpu_ctx, kp, 16, 8, (2, 8, 2)).tolist() == [0, 2]
    assert check(gpu_ctx, kp, 16, 8, (3, 8, 2)).tolist() == [0, 1, 2]
    assert check(gpu_ctx, kp, 16, 8, (4, 8, 1)).tolist() == [1, 2]


def test_cell_count_at_the_limit_and_above(gpu_ctx):
    assert br.grid(128, 128, 1) == (128, 128) and 128 * 128 == br.MAX_CELLS
    kp = grid_kp(9, 3 * T + 5, 128, 128)
    check(gpu_ctx, kp, 128, 128, (-1, 1, 1), "16384 cells")
    check(gpu_ctx, kp, 128, 128, (T, 1, 2), "16384 cells")
    assert 145 * 113 == br.MAX_CELLS + 1
    for run in (raw_host, raw_device):
        for w, h in ((145, 113), (129, 128)):
            rc, m, buf = run(gpu_ctx, kp, w, h, (-1, 1, 1))
            assert rc == sift_amd.SIFT_E_UNSUPPORTED and m == 12345 and (buf == SENTINEL).all()
            rc, m, buf = run(gpu_ctx, kp, w, h, (5, 1, -1))  # the cells are counted even when no step reads them
            assert rc == sift_amd.SIFT_E_UNSUPPORTED and m == 12345 and (buf == SENTINEL).all()
    check(gpu_ctx, kp, 145, 113, (T, 0, 1), "no grid: the frame is not read")


# ---- buffers and arguments -----------------------------------------------------------------------------------------
def test_capacity_count_only_and_arguments(gpu_ctx):
    kp = grid_kp(11, 500, 64, 64)
    bud = (40, 16, 5)
    want = br.select(kp, 64, 64, bud)
    assert len(want) == 40
    for run in (raw_host, raw_device):
        rc, m, buf = run(gpu_ctx, kp, 64, 64, bud, cap=len(want) - 1)
        assert rc == sift_amd.SIFT_E_CAPACITY and m == len(want) and (buf == SENTINEL).all()
        rc, m, buf = run(gpu_ctx, kp, 64, 64, bud, cap=len(want))
        assert rc == 0 and m == len(want) and (buf[:m] == want).all() and (buf[m:] == SENTINEL).all()
        rc, m, buf = run(gpu_ctx, kp, 64, 64, bud, cap=0, want_index=False)
        assert rc == 0 and m == len(want) and (buf == SENTINEL).all()
    E_ARG = sift_amd.SIFT_E_ARG
    rc, m, buf = raw_host(gpu_ctx, kp, 64, 64, bud, reserved=1)
    assert rc == E_ARG and m == 12345 and (buf == SENTINEL).all()
    assert raw_host(gpu_ctx, kp, 64, 64, (40, -1, 5))[0] == E_ARG
    assert raw_device(gpu_ctx, kp, 64, 64, (40, -8, 5))[0] == E_ARG
    assert raw_host(gpu_ctx, kp, 64, 64, bud, null_kp=True)[0] == E_ARG
    assert raw_host(gpu_ctx, kp, 0, 64, bud)[0] == E_ARG and raw_host(gpu_ctx, kp, 64, -3, bud)[0] == E_ARG
    L = sift_amd.lib()
    n_out = ctypes.c_size_t(12345)
    assert L.sift_keypoint_select(gpu_ctx._h, kp.ctypes.data_as(VP), len(kp), 64, 64, None, None, 0,
                                  ctypes.byref(n_out)) == E_ARG
    assert L.sift_keypoint_select(None, kp.ctypes.data_as(VP), len(kp), 64, 64, None, None, 0, None) == E_ARG
    assert n_out.value == 12345


def test_host_and_device_forms_agree_and_repeat(gpu_ctx):
    kp = grid_kp(12, 3 * T + 5, 200, 120)
    for bud in ((T + 7, 0, -1), (-1, 16, 3), (300, 16, 3), (-1, 0, -1)):
        a = raw_host(gpu_ctx, kp, 200, 120, bud)
        b = raw_device(gpu_ctx, kp, 200, 120, bud)
        c = raw_device(gpu_ctx, kp, 200, 120, bud)
        assert a[0] == b[0] == c[0] == 0 and a[1] == b[1] == c[1]
        assert a[2].tobytes() == b[2].tobytes() == c[2].tobytes()
        np.testing.assert_array_equal(a[2][:a[1]], br.select(kp, 200, 120, bud))
    got = gpu_ctx.select_keypoints(kp, 200, 120, max_total=300, cell_px=16, max_per_cell=3)
    np.testing.assert_array_equal(got, br.select(kp, 200, 120, (300, 16, 3)))
    assert got.dtype == np.int32 and gpu_ctx.select_timing() > 0.0


# ---- the context's own list ----------------------------------------------------------------------------------------
W = H = 256
PARAMS = dict(num_octaves=3, scales_per_octave=4)


@pytest.fixture(scope="module")
def detected():
    """(image, parameters, the detection's keypoints): computed once, left unchanged."""
    img = blob_image(W, H, seed=3)
    p = sift_amd.make_params(**PARAMS)
    with sift_amd.Context(0) as ctx:
        kp = ctx.detect(img, p).copy()
    assert len(kp) > 1000
    return img, p, kp


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("bud", [dict(max_total=200), dict(cell_px=32, max_per_cell=2),
                                 dict(max_total=50, cell_px=32, max_per_cell=2)])
def test_limit_keypoints_in_place(detected, bud):
    img, p, kp0 = detected
    want = br.select(kp0, W, H, br.budget(**bud))
    assert 0 < len(want) < len(kp0)
    with sift_amd.Context(0) as ctx, sift_amd.Context(0) as other:
        ctx.detect(img, p)
        before = ctx.counts(), ctx.timings()["refine_ms"]
        assert ctx.limit_keypoints(**bud) == len(want)
        assert same_bytes(ctx.keypoints(), kp0[want])
        np.testing.assert_array_equal(ctx.keypoint_selection(), want)
        assert ctx.counts()["keypoints"] == len(want) and ctx.counts()["singular"] == before[0]["singular"]
        assert ctx.timings()["refine_ms"] == before[1] and ctx.select_timing() > 0.0
        assert len(ctx.block_counts()) == 0
        ori, (desc, ok) = ctx.orient(), ctx.describe()
        other.build_scale_space(img, p)
        other.set_keypoints(kp0[want])
        ori2, (desc2, ok2) = other.orient(), other.describe()
        assert len(ori) > 0 and same_bytes(ori, ori2) and same_bytes(desc, desc2) and same_bytes(ok, ok2)
        # a second call selects from the limited list, and drops the features of the first
        kp1 = kp0[want]
        want2 = br.select(kp1, W, H, br.budget(max_total=17))
        assert ctx.limit_keypoints(max_total=17) == 17
        assert same_bytes(ctx.keypoints(), kp1[want2])
        np.testing.assert_array_equal(ctx.keypoint_selection(), want2)
        other.set_keypoints(kp1[want2])
        assert same_bytes(ctx.orient(), other.orient())
        # no limit keeps the list as it is
        assert ctx.limit_keypoints() == 17
        np.testing.assert_array_equal(ctx.keypoint_selection(), np.arange(17))
        assert ctx.limit_keypoints(max_total=0) == 0 and len(ctx.keypoints()) == 0 and len(ctx.orient()) == 0


def expect(code, fn, *a, **k):
    with pytest.raises(sift_amd.SiftError) as e:
        fn(*a, **k)
    assert e.value.code == code


def test_limit_keypoints_states(detected):
    img, p, kp0 = detected
    E_STATE, E_UNSUP = sift_amd.SIFT_E_STATE, sift_amd.SIFT_E_UNSUPPORTED
    with sift_amd.Context(0) as ctx:
        expect(E_STATE, ctx.limit_keypoints, max_total=5)         # before any refinement
        expect(E_STATE, ctx.keypoint_selection)
        ctx.build_scale_space(img, p)
        expect(E_STATE, ctx.limit_keypoints, max_total=5)         # a pyramid alone is not a list
        po = sift_amd.make_params(flags=sift_amd.F_KEYPOINT_ORIGINS, **PARAMS)
        ctx.detect(img, po)
        assert len(ctx.keypoint_origins()) == len(kp0)
        expect(E_STATE, ctx.keypoint_selection)                   # a list, but not a limited one
        L = sift_amd.lib()
        bad = sift_amd.Budget(5, 0, -1, 1)
        assert L.sift_limit_keypoints(ctx._h, ctypes.byref(bad), None) == sift_amd.SIFT_E_ARG
        assert L.sift_limit_keypoints(ctx._h, None, None) == sift_amd.SIFT_E_ARG
        assert same_bytes(ctx.keypoints(), kp0)                   # nothing was changed
        assert ctx.limit_keypoints(max_total=100) == 100
        expect(E_STATE, ctx.keypoint_origins)                     # the origins were those of the whole list
        assert len(ctx.keypoint_selection()) == 100
        ctx.detect(img, po)                                       # a new detection: the selection is gone
        expect(E_STATE, ctx.keypoint_selection)
        assert len(ctx.keypoint_origins()) == len(kp0)
        ctx.limit_keypoints(max_total=100)
        ctx.set_keypoints(kp0[:10])                               # ... and so after caller keypoints
        expect(E_STATE, ctx.keypoint_selection)
        assert ctx.limit_keypoints(max_total=4) == 4              # caller keypoints are a list
        np.testing.assert_array_equal(ctx.keypoint_selection(), br.select(kp0[:10], W, H, br.budget(4)))
        # a skipped Gaussian pyramid is no obstacle
        ctx.detect(img, sift_amd.make_params(flags=sift_amd.F_SKIP_GAUSS_PLANES, **PARAMS))
        assert ctx.limit_keypoints(cell_px=64, max_per_cell=1) == len(br.select(kp0, W, H, br.budget(None, 64, 1)))
        ctx.detect_batch(np.stack([img, img]), p)
        expect(E_UNSUP, ctx.limit_keypoints, max_total=5)
        ctx.set_row_origin(4)
        ctx.detect(img, p)
        expect(E_UNSUP, ctx.limit_keypoints, max_total=5)
        ctx.set_row_origin(0)
        ctx.set_owned_rows(0, 128)
        ctx.detect(img, p)
        expect(E_UNSUP, ctx.limit_keypoints, max_total=5)
        ctx.set_owned_rows(-1)
        ctx.detect(img, p)
        assert ctx.limit_keypoints(max_total=5) == 5
