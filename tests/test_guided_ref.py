"""The numpy statement of guided matching (tests/guided_ref.py) against the same definition written with two
loops, against the brute-force reference when the radius covers everything, and the grid rule at its cell cap."""
import numpy as np
import pytest

import guided_ref as gr
import match_ref as mr


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for f in got.dtype.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def small_case(seed, nq, nt, size=64.0):
    rng = np.random.default_rng(seed)
    query = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    train = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    if nt > 3 and nq > 2:
        train[3] = train[1] = query[2]                     # a tie at distance 0
    qxy, txy = rng.uniform(-4, size + 4, (nq, 2)), rng.uniform(-4, size + 4, (nt, 2))
    qm, tm = rng.integers(0, 8, nq) != 0, rng.integers(0, 8, nt) != 0
    return query, qxy, train, txy, qm, tm


@pytest.mark.parametrize("seed,nq,nt,radius", [(1, 7, 40, 20.0), (2, 12, 25, 9.5), (3, 5, 1, 100.0), (4, 1, 60, 30.0),
                                                (5, 9, 0, 3.0), (6, 0, 9, 3.0)])
def test_numpy_statement_equals_the_loops(seed, nq, nt, radius):
    query, qxy, train, txy, qm, tm = small_case(seed, nq, nt)
    h = [1.01, 0.02, -1.5, -0.015, 0.99, 2.0, 1e-4, -2e-4, 1.0]
    got, n_proj, n_cand = gr.guided_ref(query, qxy, train, txy, h, radius, qm, tm)
    want, w_proj, w_cand = gr.guided_loops(query, qxy, train, txy, h, radius, qm, tm)
    same(got, want)
    assert (n_proj, n_cand) == (w_proj, w_cand)
    got, n_proj, n_cand = gr.guided_ref(query, qxy, train, txy, h, radius)
    want, w_proj, w_cand = gr.guided_loops(query, qxy, train, txy, h, radius)
    same(got, want)
    assert (n_proj, n_cand) == (w_proj, w_cand) and n_proj == nq


def test_unprojected_rows_and_bad_numbers_in_both_statements():
    query, qxy, train, txy, qm, tm = small_case(7, 10, 30)
    qxy[0] = (np.nan, 3.0)
    qxy[1] = (np.inf, 3.0)
    qxy[2] = (1e300, 5.0)
    txy[4] = (np.nan, 1.0)
    txy[5] = (2.0, np.nan)
    for h in ([1, 0, 0, 0, 1, 0, 0.05, 0, -1.0],           # w > 0 only right of x = 20
              [1, 0, 0, 0, 1, 0, 0, 0, 0], [0] * 9, [1, 0, np.nan, 0, 1, 0, 0, 0, 1]):
        for radius in (15.0, 1e300):
            got, n_proj, n_cand = gr.guided_ref(query, qxy, train, txy, h, radius)
            want, w_proj, w_cand = gr.guided_loops(query, qxy, train, txy, h, radius)
            same(got, want)
            assert (n_proj, n_cand) == (w_proj, w_cand)
            assert got["best"][0] == -1 and got["best"][1] == -1
            assert not np.isin(got["best"], (4, 5)).any()
    got, n_proj, _ = gr.guided_ref(query, qxy, train, txy, [1, 0, 0, 0, 1, 0, 0.05, 0, -1.0], 15.0)
    assert 0 < n_proj < 10
    got, n_proj, n_cand = gr.guided_ref(query, qxy, train, txy, np.eye(3), 1e300)
    assert n_proj == 8 and n_cand == 8 * 28 and got["best"][2] >= 0   # 1e300: dx * dx = inf <= r2 = inf


@pytest.mark.parametrize("masked", [False, True])
def test_a_radius_over_everything_is_the_brute_force_match(masked):
    query, qxy, train, txy, qm, tm = small_case(8, 70, 300, size=500.0)
    if not masked:
        qm = tm = None
    got, n_proj, n_cand = gr.guided_ref(query, qxy, train, txy, np.eye(3), 1e9, qm, tm)
    same(got, mr.match_ref(query, train, qm, tm))
    nq_in = 70 if qm is None else int(qm.sum())
    nt_in = 300 if tm is None else int(tm.sum())
    assert (n_proj, n_cand) == (nq_in, nq_in * nt_in)
    assert gr.visited_ref(qxy, txy, 500, 400, np.eye(3), 1e9, qm, tm) == nq_in * nt_in
    assert gr.grid_ref(500, 400, 1e9) == (500, 1, 1)


def test_the_grid_reaches_the_cell_cap_and_stays_within_it():
    assert gr.grid_ref(1024, 768, 12) == (12, 86, 64)
    assert gr.grid_ref(1024, 768, 11.01) == (12, 86, 64)
    assert gr.grid_ref(1024, 1024, 1) == (1, 1024, 1024)                # exactly MAX_CELLS
    assert gr.grid_ref(1025, 1024, 0.5) == (2, 513, 512)
    assert gr.grid_ref(3, 7, 1e300) == (7, 1, 1)
    for w, h, r in [(40000, 40000, 1), (3840, 2160, 0.25), (2**31 - 1, 1, 1), (2**31 - 1, 2**31 - 1, 3), (1, 1, 1)]:
        c, ncx, ncy = gr.grid_ref(w, h, r)
        assert ncx * ncy <= gr.MAX_CELLS and c >= 1
        assert (ncx, ncy) == (-(-w // c), -(-h // c))
        if c > max(1, min(int(np.ceil(r)), max(w, h))):                  # the cap decided: one less is too many
            assert -(-w // (c - 1)) * -(-h // (c - 1)) > gr.MAX_CELLS
    assert gr.grid_ref(40000, 40000, 1) == (40, 1000, 1000)


def test_axis_is_the_clamped_rule():
    a = np.array([-1e300, -0.5, -0.0, 0.0, 11.999, 12.0, 1023.9, 1024.0, 1e300, np.inf, -np.inf, np.nan])
    np.testing.assert_array_equal(gr.axis(a, 12, 86), [0, 0, 0, 0, 0, 1, 85, 85, 85, 85, 0, 0])


def test_visited_counts_the_cells_of_the_stated_rule():
    # 10-pixel cells on 100 x 100, one train point in every cell centre; radius 10 around (55, 55) reaches columns
    # col(45) - 1 .. col(65) + 1 = 3 .. 7, and likewise rows: 25 cells
    c = np.arange(10) * 10 + 5.0
    txy = np.stack(np.meshgrid(c, c), -1).reshape(-1, 2)
    assert gr.grid_ref(100, 100, 10) == (10, 10, 10)
    assert gr.visited_ref(np.array([[55.0, 55.0]]), txy, 100, 100, np.eye(3), 10) == 25
    assert gr.visited_ref(np.array([[-30.0, 55.0]]), txy, 100, 100, np.eye(3), 10) == 2 * 5   # columns 0 .. 1
    assert gr.visited_ref(np.array([[99.0, 99.0]]), txy, 100, 100, np.eye(3), 10) == 3 * 3    # 7 .. 9 both ways
    tm = np.ones(100, np.uint8)
    tm[55] = 0                                             # the centre cell's point masked: not filed
    assert gr.visited_ref(np.array([[55.0, 55.0]]), txy, 100, 100, np.eye(3), 10, None, tm) == 24
