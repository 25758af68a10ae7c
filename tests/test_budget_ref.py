"""The numpy restatement of the keypoint budget (tests/budget_ref.py) against a
plain loop over the definition's "precedes" and against a hand-written table;
and the five entry points in the header, the binding and the library."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import budget_ref as br
import sift_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sift_keypoint_select_device", "sift_keypoint_select", "sift_limit_keypoints",
           "sift_copy_keypoint_selection", "sift_last_select_timing")
NAN, INF = float("nan"), float("inf")
DENORMAL = 5e-324


def make_kp(values, xs=None, ys=None):
    kp = np.zeros(len(values), dtype=sift_amd.KEYPOINT_DTYPE)
    kp["interp_value"] = values
    kp["abs_x"] = 0.0 if xs is None else xs
    kp["abs_y"] = 0.0 if ys is None else ys
    return kp


# ---- the definition as a loop -------------------------------------------------------------------------------------
def loop_key(v):
    if math.isnan(v):
        return 0
    return struct.unpack("<Q", struct.pack("<d", v))[0] & 0x7FFFFFFFFFFFFFFF


def loop_axis(a, cell_px, nc):
    t = a / float(cell_px)
    if not t >= 0:
        return 0
    return int(math.floor(t)) if t < nc else nc - 1


def loop_select(kp, width, height, bud):
    max_total, cell_px, max_per_cell = bud
    n = len(kp)
    key = [loop_key(float(v)) for v in kp["interp_value"]]

    def precedes(i, j):
        return key[i] > key[j] or (key[i] == key[j] and i < j)

    surv = list(range(n))
    if cell_px > 0 and max_per_cell >= 0:
        ncx, ncy = -(-width // cell_px), -(-height // cell_px)
        cell = [loop_axis(float(kp["abs_y"][i]), cell_px, ncy) * ncx + loop_axis(float(kp["abs_x"][i]), cell_px, ncx)
                for i in range(n)]
        surv = [i for i in range(n)
                if sum(1 for j in range(n) if cell[j] == cell[i] and precedes(j, i)) < max_per_cell]
    if max_total >= 0:
        surv = [i for i in surv if sum(1 for j in surv if precedes(j, i)) < max_total]
    return np.array(surv, dtype=np.int32)


def special_values(rng, n):
    pool = np.array([0.0, -0.0, NAN, INF, -INF, DENORMAL, -DENORMAL, 1.0, -1.0, 0.5, 0.03, -0.03, 2.0])
    v = pool[rng.integers(0, len(pool), n)]
    some = rng.random(n) < 0.4
    v[some] = rng.normal(size=int(some.sum()))
    return v


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 60))
    w, h = 23, 17
    xs = rng.uniform(-3, w + 3, n)
    ys = rng.uniform(-3, h + 3, n)
    xs[rng.random(n) < 0.1] = NAN
    kp = make_kp(special_values(rng, n), xs, ys)
    for bud in (br.budget(), br.budget(0), br.budget(1), br.budget(n // 2), br.budget(n), br.budget(n + 1),
                br.budget(None, 5, 0), br.budget(None, 5, 1), br.budget(None, 5, 2), br.budget(7, 5, 2),
                br.budget(3, 100, 5), br.budget(4, 1, 1), br.budget(None, 5, None), br.budget(2, 5, None)):
        np.testing.assert_array_equal(br.select(kp, w, h, bud), loop_select(kp, w, h, bud), err_msg=str(bud))


# ---- the table ----------------------------------------------------------------------------------------------------
def test_keys_of_signs_zeros_nan_inf_and_a_denormal():
    v = np.array([1.5, -1.5, 0.0, -0.0, NAN, INF, -INF, DENORMAL, -DENORMAL, -NAN])
    k = br.keys(make_kp(v))
    assert k.dtype == np.uint64
    assert k[0] == k[1] == 0x3FF8000000000000
    assert k[2] == k[3] == k[4] == k[9] == 0
    assert k[5] == k[6] == 0x7FF0000000000000
    assert k[7] == k[8] == 1
    assert k[5] > k[0] > k[7] > k[2]


TABLE = [
    # values, max_total, kept
    ([1.0, -2.0, 3.0, -4.0], 2, [2, 3]),                       # by magnitude, either sign
    ([0.0, -0.0, NAN, DENORMAL], 1, [3]),                      # a denormal beats every zero and NaN
    ([0.0, -0.0, NAN, DENORMAL], 3, [0, 1, 3]),                # the zeros and the NaN tie: the lowest indices win
    ([NAN, 0.0, -0.0], 2, [0, 1]),                             # a NaN is not weaker than a zero
    ([1.0, INF, -INF, 1e308], 2, [1, 2]),                      # inf is the strongest
    ([2.0, 5.0, -5.0, 5.0, 1.0], 2, [1, 2]),                   # a tie at the quota: index order
    ([2.0, 5.0, -5.0, 5.0, 1.0], 3, [1, 2, 3]),
    ([2.0, 5.0, -5.0, 5.0, 1.0], 4, [0, 1, 2, 3]),
    ([7.0, 7.0, 7.0], 0, []),
    ([7.0, 7.0, 7.0], 5, [0, 1, 2]),
    ([7.0, 7.0, 7.0], -1, [0, 1, 2]),
]


@pytest.mark.parametrize("values,max_total,kept", TABLE)
def test_table_of_strengths_and_ties(values, max_total, kept):
    got = br.select(make_kp(values), 10, 10, (max_total, 0, -1))
    assert got.dtype == np.int32
    assert got.tolist() == kept


def test_cell_borders():
    assert br.BORDER_FRAME == (20, 12, 8)
    xs = np.array([x for x, _ in br.BORDER_X])
    want = np.array([c for _, c in br.BORDER_X])
    kp = make_kp(np.ones(len(xs)), xs, np.zeros(len(xs)))
    np.testing.assert_array_equal(br.cells(kp, 20, 12, 8), want)
    kp = make_kp(np.ones(len(xs)), np.zeros(len(xs)), xs)  # the same on y: rows 0, 1, and the clamp to the last row
    np.testing.assert_array_equal(br.cells(kp, 20, 12, 8), np.minimum(want, 1) * 3)
    assert br.grid(20, 12, 8) == (3, 2) and br.grid(16, 12, 1) == (16, 12) and br.grid(16, 16, 8) == (2, 2)


def test_per_cell_then_total_ties_between_cells():
    # two cells of 8 px on a 16 x 8 frame; cell 0 holds records 0, 2, 4, cell 1 holds 1, 3, 5
    xs = [1.0, 9.0, 2.0, 10.0, 3.0, 11.0]
    v = [5.0, 5.0, 9.0, 1.0, 5.0, 5.0]
    kp = make_kp(v, xs, [0.0] * 6)
    assert br.select(kp, 16, 8, br.budget(None, 8, 2)).tolist() == [0, 1, 2, 5]    # 4 and 3 fall in step 1
    assert br.select(kp, 16, 8, br.budget(2, 8, 2)).tolist() == [0, 2]             # 9, then the first of the 5s
    assert br.select(kp, 16, 8, br.budget(3, 8, 2)).tolist() == [0, 1, 2]          # the tie crosses the cells
    assert br.select(kp, 16, 8, br.budget(3, 8, None)).tolist() == [0, 1, 2]       # no step 1: 4 could not enter anyway
    assert br.select(kp, 16, 8, br.budget(4, 8, 1)).tolist() == [1, 2]
    assert br.select(kp, 16, 8, br.budget(None, 8, 0)).tolist() == []


# ---- the interface ------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "sift_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = sift_amd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", sift_amd.LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sift_amd.ABI_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r" T %s\b" % name, out), name
    assert "SIFT_BUDGET_MAX_CELLS 16384" in header and sift_amd.BUDGET_MAX_CELLS == br.MAX_CELLS == 16384
    for method in ("select_keypoints", "limit_keypoints", "keypoint_selection", "select_timing"):
        assert callable(getattr(sift_amd.Context, method)), method
    import ctypes
    assert ctypes.sizeof(sift_amd.Budget) == 16
    b = sift_amd.make_budget(None, 32, 2)
    assert (b.max_total, b.cell_px, b.max_per_cell, b.reserved) == (-1, 32, 2, 0)
