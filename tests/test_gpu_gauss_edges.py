"""The Gaussian + DoG pass at every radius of every kernel, every tile edge
and every scale-group seam (tables: gauss_cases.py; CPU half:
test_gauss_cases.py).

Every case builds a pyramid, reads the launch plan back
(sift_last_gauss_plan) and asserts that each octave ran the kernel, window
radius, grid, scale groups, store width and fp64-plane choice the case was
built for, then compares EVERY Gaussian and DoG plane of EVERY octave with the
oracle's CONV_SEPARABLE_FMA_VH plane rounded to fp32, with
assert_array_equal: there is no tolerance in this file.  The octave after the
one under test is always built, so its planes check the seed stores.

The last test collects what the module launched -- (path, radius) tokens from
the plan records and the library's own radii, counted only for planes with an
interior tile and edge tiles on all four sides -- and asserts the required
set, so a case that silently stops running its path fails there.  It needs the
whole module to have run.
"""
import numpy as np
import pytest

import gauss_cases as gc
import sift_amd
from parity_util import host_threads
from sift_amd.shard import octave_radii

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("kernel", "path", "rw", "tile_w", "tile_rows", "gx", "gy", "G", "keep_l64", "vsplit", "vec", "fused")
PATH_OF = {(k, p): name for name, (k, p, _, _, _) in gc.PATHS.items()}
LAUNCHED = set()      # tokens of planes with an interior tile, over the whole module
GEOMETRY_RAN = set()  # (family, w, h, fused)
GROUPS_RAN = set()    # (family, G)


def _sched_id(s):
    return "O%dS%dmb%g" % s


def _run(ctx, img, sched, fused=False, count=False):
    """Build (fused: detect with F_FUSED_EXTREMA), hold the reported plan of
    every octave to the restated one, compare every plane with the oracle.
    Returns (plans, dims, radii)."""
    O, S, mb = sched
    NS = S + 3
    p = sift_amd.make_params(O, S, mb, gc.ASSUMED_BLUR, flags=sift_amd.F_FUSED_EXTREMA if fused else 0)
    if fused:
        ctx.detect(img, p)
    else:
        ctx.build_scale_space(img, p)
    rad = octave_radii(p)
    dims = [ctx.dims(o) for o in range(O)]
    plans = [ctx.gauss_plan(o) for o in range(O)]
    want = gc.expected_plans(dims, rad, S, fused)
    for o in range(O):
        got = {k: plans[o][k] for k in PLAN_KEYS}
        assert got == want[o], "octave %d (%d x %d, radii %s): launched %s, the case needs %s" % (
            o, dims[o][1], dims[o][0], rad[o], got, want[o])
        gb = plans[o]["gb"]
        assert len(gb) == plans[o]["G"] + 1 and gb[0] == 0 and gb[-1] == NS and all(
            a < b for a, b in zip(gb, gb[1:])), gb
    odims, gauss, dog = gc.oracle_planes(img, O, S, mb, threads=host_threads())
    assert [tuple(d) for d in odims] == [tuple(d) for d in dims]
    for o in range(O):
        name = PATH_OF[(plans[o]["kernel"] - (2 if plans[o]["fused"] else 0), plans[o]["path"])]
        what = "%s%s octave %d (%d x %d, gx %d gy %d G %d gb %s)" % (
            name, " fused" if plans[o]["fused"] else "", o, dims[o][1], dims[o][0], plans[o]["gx"], plans[o]["gy"],
            plans[o]["G"], plans[o]["gb"])
        for s in range(NS):
            np.testing.assert_array_equal(ctx.plane(sift_amd.PLANE_GAUSS, o, s), gauss[o][s].astype(np.float32),
                                          err_msg="%s: Gaussian scale %d, radius %d" % (what, s, rad[o][s]))
        for s in range(NS - 1):
            np.testing.assert_array_equal(ctx.plane(sift_amd.PLANE_DOG, o, s), dog[o][s].astype(np.float32),
                                          err_msg="%s: DoG %d = L%d - L%d, radii %d and %d" % (
                                              what, s, s, s + 1, rad[o][s], rad[o][s + 1]))
        if count and plans[o]["gx"] >= 3 and plans[o]["gy"] >= 3:
            toks = gc.tokens(name, rad[o])
            LAUNCHED.update({(t[0] + "_fused",) + t[1:] for t in toks} if plans[o]["fused"] else toks)
    return plans, dims, rad


# ---------------------------------------------------------------------------
# The radius sweep.
# ---------------------------------------------------------------------------
SWEEP_TILES = (400, 200)   # octaves 0, 1, 2: 800 x 400, 400 x 200, 200 x 100 -- at least 4 x 4 tiles of 64 x 32


def _rw_image(paths):
    """Input whose deepest k_gauss_rw octave is 700 x 30: at least 3 tiles of 224 / 192 columns x 8 rows."""
    deepest = max(o for o, p in enumerate(paths) if p in gc.RW_PATHS)
    return 700 << (deepest - 1), 30 << (deepest - 1)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sched,paths", gc.RADIUS_TABLE, ids=[_sched_id(s) for s, _ in gc.RADIUS_TABLE])
def test_radius_sweep_tiles(gpu_ctx, sched, paths):
    """Octave 0 (staged or on the fp64 base) and the 64 x 32 tile and split
    paths of octaves >= 1, every plane with an interior tile."""
    img = gc.noise_image(*SWEEP_TILES, seed=101 + 7 * sched[1])
    plans, _, _ = _run(gpu_ctx, img, sched, count=True)
    assert tuple(PATH_OF[(g["kernel"], g["path"])] for g in plans) == tuple(paths)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sched,paths", [(s, p) for s, p in gc.RADIUS_TABLE if set(p) & set(gc.RW_PATHS)],
                         ids=[_sched_id(s) for s, p in gc.RADIUS_TABLE if set(p) & set(gc.RW_PATHS)])
def test_radius_sweep_rw(gpu_ctx, sched, paths):
    """The k_gauss_rw octaves on planes at least 3 tiles wide and 24 rows high."""
    W, H = _rw_image(paths)
    img = gc.noise_image(W, H, seed=211 + 7 * sched[1])
    plans, dims, _ = _run(gpu_ctx, img, sched, count=True)
    assert tuple(PATH_OF[(g["kernel"], g["path"])] for g in plans) == tuple(paths)
    for o, p in enumerate(paths):
        if p in gc.RW_PATHS:
            assert dims[o][1] >= 3 * plans[o]["tile_w"] and dims[o][0] >= 24
            assert plans[o]["gx"] >= 3 and plans[o]["gy"] >= 3


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sched,paths", [(s, p) for s, p in gc.RADIUS_TABLE if p[0] != "base0"],
                         ids=[_sched_id(s) for s, p in gc.RADIUS_TABLE if p[0] != "base0"])
def test_radius_sweep_fused_octave0(gpu_ctx, sched, paths):
    """The staged octave 0 again with its extrema decisions fused: the same
    planes, and the same candidates as the plain detection."""
    img = gc.noise_image(*SWEEP_TILES, seed=101 + 7 * sched[1])
    O, S, mb = sched
    gpu_ctx.detect(img, sift_amd.make_params(O, S, mb, gc.ASSUMED_BLUR))
    plain = gpu_ctx.candidates().copy()
    assert gpu_ctx.gauss_plan(0)["fused"] == 0
    plans, _, _ = _run(gpu_ctx, img, sched, fused=True, count=True)
    assert plans[0]["fused"] == 1 and plans[0]["kernel"] == gc.PATHS[paths[0]][0] + 2
    fused = gpu_ctx.candidates()
    print("\n%s: %d candidates" % (_sched_id(sched), plain.shape[0]))
    assert fused.tobytes() == plain.tobytes()


# ---------------------------------------------------------------------------
# The geometry sweep.
# ---------------------------------------------------------------------------
def _geom_id(c):
    return "%s-w%dT%+d-h%dT%+d" % (c[0], c[1][0], c[1][1], c[2][0], c[2][1])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", gc.geometry_cases(), ids=_geom_id)
def test_geometry_sweep(gpu_ctx, case):
    """One plane at a tile edge of its family; the size is the case's offset
    from the tile size the launch reports.  Octave-0 cases run plain and, where
    the plan can fuse, with F_FUSED_EXTREMA (tiles of 60 x 30 decided pixels)."""
    family, wmd, hmd = case
    sched, o, path = gc.GEOMETRY_SCHEDULES[family]
    W, H = gc.geometry_input(family, wmd, hmd)
    img = gc.noise_image(W, H, seed=31 * W + H)
    for fused in (False, True):
        if fused and not gc.can_fuse(path, 2 * H, 2 * W):
            continue
        plans, dims, _ = _run(gpu_ctx, img, sched, fused=fused)
        g = plans[o]
        assert PATH_OF[(g["kernel"] - (2 if fused else 0), g["path"])] == path
        h, w = dims[o]
        assert (w, h) == (gc.size(wmd, g["tile_w"]), gc.size(hmd, g["tile_rows"]))
        if fused:
            assert (g["gx"], g["gy"]) == (max(1, -(-(w - 2) // gc.FUSED_X)), -(-(h - 2) // gc.FUSED_Y))
        assert len(plans) > o + 1  # the next octave's planes were compared: the seed stores
        GEOMETRY_RAN.add((family, w, h, fused))


# ---------------------------------------------------------------------------
# The scale-group sweep.
# ---------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", gc.group_cases(), ids=lambda c: "%s-h%d-G%d" % c)
def test_scale_group_sweep(gpu_ctx, case):
    """Narrow tall planes whose tile count gives 1 < G < NS: the groups, their
    boundaries and the L[s-1] each group recomputes at its seam."""
    family, h, G = case
    sched = gc.GROUP_SCHEDULES[family]
    img = gc.noise_image(gc.GROUP_WIDTH, h, seed=h)
    plans, dims, _ = _run(gpu_ctx, img, sched)
    g = plans[1]
    assert dims[1] == (h, gc.GROUP_WIDTH) and PATH_OF[(g["kernel"], g["path"])] == family
    assert g["G"] == G and any(0 < b < sched[1] + 3 for b in g["gb"]), g
    GROUPS_RAN.add((family, G))


def test_plan_record_arguments_and_state(gpu_ctx):
    import ctypes
    L = sift_amd.lib()
    info = sift_amd.GaussPlanInfo()
    gpu_ctx.build_scale_space(gc.noise_image(20, 12, seed=1), sift_amd.make_params(2, 5))
    assert L.sift_last_gauss_plan(None, 0, ctypes.byref(info)) == sift_amd.SIFT_E_ARG
    assert L.sift_last_gauss_plan(gpu_ctx._h, 0, None) == sift_amd.SIFT_E_ARG
    assert L.sift_last_gauss_plan(gpu_ctx._h, -1, ctypes.byref(info)) == sift_amd.SIFT_E_ARG
    assert L.sift_last_gauss_plan(gpu_ctx._h, 2, ctypes.byref(info)) == sift_amd.SIFT_E_ARG
    names = dict(e.split(": ", 1) for e in gpu_ctx.pass_kernels().split("; "))
    assert names == {"o0": "k_gauss_dog<octave0>", "o1": "k_gauss_rw<12>"}
    assert (gpu_ctx.gauss_plan(0)["kernel"], gpu_ctx.gauss_plan(1)["kernel"]) == (gc.K_STAGED8, gc.K_WINDOW12)
    with sift_amd.Context(0) as fresh:
        assert L.sift_last_gauss_plan(fresh._h, 0, ctypes.byref(info)) == sift_amd.SIFT_E_STATE


def test_the_module_launched_every_required_path_and_radius():
    fused = {(t[0] + "_fused", t[1]) for t in gc.REQUIRED if t[0] in ("staged8", "staged16")}
    missing = (gc.REQUIRED | fused) - LAUNCHED
    assert not missing, "never launched on a plane with an interior tile: %s" % sorted(missing, key=str)
    want = set()
    for family, wmd, hmd in gc.geometry_cases():
        _, o, path = gc.GEOMETRY_SCHEDULES[family]
        w, h = gc.size(wmd, gc.PATHS[path][3]), gc.size(hmd, gc.PATHS[path][4])
        want.add((family, w, h, False))
        if gc.can_fuse(path, h, w):
            want.add((family, w, h, True))
    assert GEOMETRY_RAN == want
    assert GROUPS_RAN == {(f, G) for f, _, G in gc.group_cases()}
