"""CPU half of the Gaussian-pass case tables (gauss_cases.py): the restated
schedule is the library's and the oracle's, the committed radius table covers
every (path, radius) the shipping plan can reach, every geometry and
scale-group case sits where it claims, and the oracle -- trusted by
test_gpu_gauss_edges.py at radii no other test runs it at -- agrees with an
independent numpy blur at every radius of the table."""
import numpy as np
import pytest

import gauss_cases as gc
import oracle as orc
import sift_amd
from sift_amd.shard import octave_radii

ALL_SCHEDULES = sorted({s for s, _ in gc.RADIUS_TABLE} | {s for s, _, _ in gc.GEOMETRY_SCHEDULES.values()} |
                       set(gc.GROUP_SCHEDULES.values()) | {(4, 5, 0.8), (5, 3, 0.8), (3, 4, 1.0), (3, 6, 1.1)})


@pytest.mark.parametrize("sched", ALL_SCHEDULES, ids=lambda s: "O%dS%dmb%g" % s)
def test_radii_restatement_is_the_librarys_and_the_oracles(sched):
    O, S, mb = sched
    blur, sigma = gc.schedule(O, S, mb)
    ob, osig = orc.schedule(orc.make_params(O, S, mb, gc.ASSUMED_BLUR))
    np.testing.assert_array_equal(np.array(blur), ob)
    np.testing.assert_array_equal(np.array(sigma), osig)
    assert gc.radii(O, S, mb) == octave_radii(sift_amd.make_params(O, S, mb, gc.ASSUMED_BLUR))


def test_radius_table_is_within_the_issue_limits_and_claims_its_paths():
    assert len(gc.RADIUS_TABLE) == len({s for s, _ in gc.RADIUS_TABLE})
    for (O, S, mb), paths in gc.RADIUS_TABLE:
        assert 1 <= O <= 3 and 1 <= S <= 9 and mb >= 0.55
        rad = gc.radii(O, S, mb)
        assert gc.schedule_fits(rad)
        assert tuple(paths) == gc.schedule_paths(O, S, mb)
        for o in range(O):  # the claim again from the thresholds, spelled out
            rmax = max(rad[o])
            want = {"staged8": o == 0 and rmax <= 8, "staged16": o == 0 and 9 <= rmax <= 16,
                    "base0": o == 0 and rmax > 16, "rw12": o >= 1 and rmax <= 12,
                    "rws16": o >= 1 and 13 <= rmax <= 16, "rws24": o >= 1 and 17 <= rmax <= 24,
                    "tiles": o >= 1 and 25 <= rmax <= 39, "split": o >= 1 and rmax >= 40}
            assert want[paths[o]], (O, S, mb, o, rmax, paths[o])


def test_radius_table_covers_every_reachable_path_and_radius():
    got = set()
    for (O, S, mb), paths in gc.RADIUS_TABLE:
        rad = gc.radii(O, S, mb)
        for o in range(O):
            got |= gc.tokens(paths[o], rad[o])
    assert not gc.REQUIRED - got, sorted(gc.REQUIRED - got, key=str)
    # the required set itself, in the issue's words
    req = gc.REQUIRED
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "staged8"} == set(range(1, 9))
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "staged16"} == set(range(1, 17))
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "rw12"} == set(range(1, 13))
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "rws16"} == set(range(2, 17))
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "rws24"} == set(range(3, 25))
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "tiles"} >= set(range(5, 13))
    assert {r for p, r in (t for t in req if len(t) == 2) if p == "split"} == set(range(8, 13))
    for name in ("tiles_gen2", "tiles_gen", "split_gen2", "split_gen"):
        assert {m for p, m in (t for t in req if len(t) == 2) if p == name} == {0, 1, 2, 3}
    assert {m for p, m in (t for t in req if len(t) == 2) if p == "tiles_rmax_parity"} == {0, 1}
    assert ("split_keep_l64",) in req
    assert {t[1:] for t in req if t[0] == "base0"} == {(b, m) for b in ("le12", "13_16", "17_32", "gt32")
                                                       for m in range(4)}


def test_greedy_generator_reproduces_the_committed_table():
    assert gc.greedy_cover() == [(s, tuple(p)) for s, p in gc.RADIUS_TABLE]


def test_geometry_cases_sit_on_their_paths_and_edges():
    for family, ((O, S, mb), o, path) in gc.GEOMETRY_SCHEDULES.items():
        assert family == path and O > o + 0 and O >= o + 2  # the octave after the one under test is built
        rad = gc.radii(O, S, mb)
        tw, th = gc.PATHS[path][3], gc.PATHS[path][4]
        widths, heights = set(), set()
        for wmd, hmd in gc.geometry_planes(family):
            W, H = gc.geometry_input(family, wmd, hmd)
            dims = orc.octave_dims(W, H, O)
            h, w = dims[o]
            assert (w, h) == (gc.size(wmd, tw), gc.size(hmd, th))
            assert gc.plan_path(o, max(rad[o]), w) == path, (family, w, h)
            widths.add(w)
            heights.add(h)
        if family in gc.RW_PATHS:
            assert widths >= {2, 3, 5, tw - 1, tw, tw + 1, tw + 4, 2 * tw + 2} and heights >= {1, 7, 8, 9, 17}
            assert (tw, th) == ((192, 8) if family == "rws24" else (224, 8))
        elif family in ("tiles", "split"):
            assert widths >= {1, 2, 63, 64, 65, 68, 130, 192} and heights >= {1, 31, 32, 33, 63, 64, 65, 96}
        else:
            assert widths >= {2, 62, 64, 66, 68, 130} and heights >= {2, 30, 32, 34, 66}
        # every residue of the width mod 4 (octave 0 is 2W wide: the even ones)
        assert {w % 4 for w in widths} == ({0, 2} if o == 0 else {0, 1, 2, 3}), family


def test_scale_group_cases_split_strictly_between_one_and_all():
    for family, h, G in gc.group_cases():
        O, S, mb = gc.GROUP_SCHEDULES[family]
        assert S == 3
        rad = gc.radii(O, S, mb)
        dims = orc.octave_dims(gc.GROUP_WIDTH, h, O)
        assert dims[1] == (h, gc.GROUP_WIDTH)
        e = gc.expected_plan(1, rad[1], h, gc.GROUP_WIDTH, S + 3)
        assert e["kernel"] == gc.PATHS[family][0] and e["gx"] == 1
        assert e["G"] == G and 1 < G < S + 3
        thr = 600 if family in gc.RW_PATHS else 400
        assert e["gy"] * (G - 1) < thr <= e["gy"] * G


U = 2.0 ** -53


def _pass_bound(r):
    """Absolute error bound of one plane of the oracle's separable fma blur
    against exact arithmetic, for inputs in [0, 1] and n = 2 r + 1
    non-negative weights that sum to 1 (unit roundoff u = 2^-53):
    * each weight: the exponent ((a a) / (s s)) * -0.5 carries 3 roundings on
      a magnitude of at most 4.5 (|a| <= 3 s + 0.5), so exp() is off by
      <= 13.5 u relative plus its own 1 u; the sum of n positive terms adds
      <= n u, the division 1 u: (n + 17) u relative, and sum(w x) <= 1;
    * each pass: an fma chain of n steps, one rounding each on a partial sum
      <= 1: n u.
    One pass is within (2 n + 17) u, vertical then horizontal within twice
    that (the horizontal pass averages the vertical one's error, it does not
    amplify it)."""
    n = 2 * r + 1
    return 2 * (2 * n + 17) * U


@pytest.mark.parametrize("sched", [s for s, _ in gc.RADIUS_TABLE], ids=lambda s: "O%dS%dmb%g" % s)
def test_oracle_matches_numpy_blur_at_every_table_radius(sched):
    """The oracle's CONV_SEPARABLE_FMA_VH planes against gauss_cases.numpy_pyramid
    (longdouble weights from the reference's formula, clamped indexing,
    vertical then horizontal), every plane of every octave of the schedule on
    a 9 x 7 image.  Tolerance: _pass_bound of the plane's radius, plus the
    bound of the plane its octave base was sampled from (a blur with
    normalised non-negative weights passes an input error on unamplified).
    The longdouble side's own error, ~n 2^-64, is three orders below it."""
    O, S, mb = sched
    img = gc.noise_image(9, 7, seed=17)
    dims, gauss, _ = gc.oracle_planes(img, O, S, mb)
    ref = gc.numpy_pyramid(img, O, S, mb)
    rad = gc.radii(O, S, mb)
    base_err = 0.0
    for o in range(O):
        for s in range(S + 3):
            tol = base_err + (0.0 if rad[o][s] == 0 else _pass_bound(rad[o][s]))
            err = float(np.abs(gauss[o][s].astype(np.longdouble) - ref[o][s]).max())
            assert err <= tol, "octave %d scale %d radius %d: |oracle - numpy| = %.3g > %.3g" % (
                o, s, rad[o][s], err, tol)
        base_err += _pass_bound(rad[o][S])


def test_every_table_radius_is_checked_against_numpy():
    seen = {r for (O, S, mb), _ in gc.RADIUS_TABLE for ro in gc.radii(O, S, mb) for r in ro}
    assert seen >= set(range(1, 40))
