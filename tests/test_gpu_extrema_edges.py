"""The extrema scan at every edge of its geometry, every S (GPU).

Caller-supplied planes (sift_load_dog: the fp32 planes are the data, the
scan's exact_planes path, k_extrema -> k_emit): extrema_cases.build_table
plants an isolated extremum, or an extremum and the one neighbour that
defeats it -- a tie, one fp32 step either way, NaN, in each of the 26
positions -- on both sides of every scan-word, strip and scale-group
boundary, on the plane's first and last interior column, row and scale and
on the contrast threshold and its fp32 predecessor, on a zero background
that holds nothing.  Geometries: w in {16, 31, 32, 62, 63, 64, 125, 126,
250, 1980, 3980} (a word whose only column is the border, a word with one
interior column, 65 words per row: k_emit's second chunk), h - 2 in {1, 2,
3, 4, 6, 14, 15, 30, 31, 32, 64}, launches of fewer than 8 blocks, of 8 and 16,
and of 17 and 33 (xcd_band with and without a remainder), S in {1, 2, 3, 5,
6, 7, 8, 9} (every instantiation of x_scan, both unequal splits of the
scales).  Noise tables (33 levels: ties everywhere, 45 % of the extrema
below the threshold, |v| on the threshold itself) reach every interior
column, row and scale of a three-octave pyramid.  Every list
equals the C oracle's on the same values: same records, same order, same
value bits.  test_extrema_cases.py (CPU) proves what the inputs hold.

Built pyramids (fp32 roundings of fp64 values: ambiguous words,
k_exact_words, and the decisions fused into k_gauss_dog): noise images of
91 x 46 whose extrema, by the oracle, fall on every fused-tile, scan-word
and strip edge of octave 0 at every scale, for S = 1..9, against the oracle
in the HIP path's summation order with the project's existing checks.
"""
import numpy as np
import pytest

import extrema_cases as xc
import oracle as orc
import sift_amd
from parity_util import check_candidates, check_keypoints, oracle_params
from sift_amd.shard import octave_radii

pytestmark = pytest.mark.gpu

TABLE_IDS = ["%dx%dO%d-S%d" % (g + (S,)) for g, S in xc.TABLES]
NOISE_IDS = ["S%d-seed%d" % (S, seed) for _, S, seed in xc.NOISE_TABLES]

_oracle = {}


def _oracle_lists(T, flat):
    """The oracle's lists of a table's values as (N,5) records (computed once)."""
    key = (T.geom, T.S, getattr(T, "seed", None), flat is not None)   # flat: the table's one finite copy
    if key not in _oracle:
        a = T.arrays() if flat is None else flat
        (crec, cval), (lrec, lval) = orc.extrema_lists(orc.make_params(T.O, T.S), T.W, T.H, a.astype(np.float64))
        _oracle[key] = (orc.as_records(crec, cval), orc.as_records(lrec, lval), crec, cval)
    return _oracle[key]


def _same_list(got, ref):
    """Same length, records, order; the values bit for bit (they are the fp32 plane values)."""
    check_candidates(got, ref, value_rtol=0)
    assert np.ascontiguousarray(got["value"]).tobytes() == np.ascontiguousarray(ref[:, 4]).tobytes()


def _scan(ctx, T, flat=None):
    """Both instantiations of k_extrema on a table; returns the bytes of what the context gave."""
    a = T.arrays() if flat is None else flat
    cref, lref, _, _ = _oracle_lists(T, flat)
    ctx.load_dog(a, T.W, T.H, sift_amd.make_params(T.O, T.S, flags=sift_amd.F_LOW_CONTRAST_LIST))
    cand, low = ctx.find_extrema()
    _same_list(cand, cref)
    lc = ctx.low_contrast()
    assert lc.shape[0] == low == lref.shape[0]
    _same_list(lc, lref)
    # without the list: k_extrema<false>
    ctx.load_dog(a, T.W, T.H, sift_amd.make_params(T.O, T.S))
    cand2, low2 = ctx.find_extrema()
    assert cand2.tobytes() == cand.tobytes() and low2 == low
    with pytest.raises(sift_amd.SiftError):
        ctx.low_contrast()
    return cand.tobytes() + lc.tobytes()


@pytest.mark.parametrize("geom,S", xc.TABLES, ids=TABLE_IDS)
def test_plant_table_equals_oracle(gpu_ctx, geom, S):
    _scan(gpu_ctx, xc.build_table(geom, S))


@pytest.mark.parametrize("geom,S,seed", xc.NOISE_TABLES, ids=NOISE_IDS)
def test_noise_table_equals_oracle(gpu_ctx, geom, S, seed):
    _scan(gpu_ctx, xc.noise_table(geom, S, seed))


def test_sparse_after_dense_on_one_context():
    """Stale bitmap words, row counts, or a block order that skips a unit: a
    dense pyramid (about 11,000 extrema, 11 blocks), then sparse tables of a
    smaller, a wider and a taller geometry at other S on the same context.
    Each result equals the oracle's and the bytes a fresh context gives."""
    dense = xc.noise_table(xc.NOISE_GEOM, 9, 1)
    assert max(len(xc.noise_table(*k).lists()[0][1]) for k in xc.NOISE_TABLES) == len(dense.lists()[0][1])
    seq = [dense, xc.build_table((31, 16, 3), 1), xc.build_table((1990, 3, 1), 7), xc.build_table((63, 33, 2), 9),
           xc.build_table((2, 2, 1), 1)]
    with sift_amd.Context(0) as ctx:
        got = [_scan(ctx, T) for T in seq]
    for T, g in zip(seq, got):
        with sift_amd.Context(0) as fresh:
            assert _scan(fresh, T) == g


def test_refine_accepts_the_table(gpu_ctx):
    """The hand-over of the ordered list, the keep flags and the deferred
    values: refine() after a plant table (its NaN, Inf and FLT_MAX entries
    zeroed) keeps what oracle_refine keeps of the same candidates."""
    T = xc.build_table((63, 33, 2), 7)
    flat = T.finite_copy()
    assert np.isfinite(flat).all() and (flat != T.arrays()).sum() > 100
    cref, _, crec, cval = _oracle_lists(T, flat)
    gpu_ctx.load_dog(flat, T.W, T.H, sift_amd.make_params(T.O, T.S))
    cand, _ = gpu_ctx.find_extrema()
    _same_list(cand, cref)
    kp, sing = gpu_ctx.refine()
    r = orc.OracleRun.__new__(orc.OracleRun)
    r.W, r.H, r.p = T.W, T.H, orc.make_params(T.O, T.S)
    r.dog_flat = flat.astype(np.float64)
    out, osing = r.refine(crec, cval)
    assert sing == osing and kp.shape[0] == out.shape[0] > 100
    ints = np.stack([kp["octave"], kp["scale_level"], kp["local_x"], kp["local_y"]], axis=1)
    np.testing.assert_array_equal(ints, out[:, :4].astype(np.int64))


# ---------------------------------------------------------------------------
# Built pyramids
# ---------------------------------------------------------------------------
FUSED_NAME = "k_gauss_dog<octave0,fused extrema>"
BASE0_NAME = "k_upsample_base + k_gauss_dog<octave0,fp64 base>"
_runs = {}


def _edge_run(S, seed):
    """Image and oracle run (the HIP path's summation order), once per (S, seed)."""
    if (S, seed) not in _runs:
        img = xc.edge_image(seed)
        _runs[(S, seed)] = (img, orc.OracleRun(img, orc.make_params(xc.EDGE_O, S), orc.CONV_SEPARABLE_FMA_VH))
    return _runs[(S, seed)]


@pytest.mark.parametrize("S", range(1, 10))
def test_native_scan_edges(gpu_ctx, S):
    """k_extrema on built planes (ties and near-threshold values go through
    the ambiguous words to k_exact_words), every S: candidates, low-contrast
    list and count, keypoints equal the oracle's."""
    p = sift_amd.make_params(xc.EDGE_O, S, flags=sift_amd.F_LOW_CONTRAST_LIST)
    for seed in xc.EDGE_SEEDS[S]:
        img, r = _edge_run(S, seed)
        kp = gpu_ctx.detect(img, p).copy()
        cand, low, counts = gpu_ctx.candidates(), gpu_ctx.low_contrast(), gpu_ctx.counts()
        check_candidates(cand, r.candidates())
        check_candidates(low, r.low_contrast())
        assert low.shape[0] == counts["low_contrast"] == r.n_low
        check_keypoints(kp, r.refined)


@pytest.mark.parametrize("S", range(1, 10))
def test_fused_edges(gpu_ctx, S):
    """SIFT_F_FUSED_EXTREMA: octave 0's decisions inside its Gaussian pass
    (60-column words from column 1, 30-row tiles) give the scan's bytes.
    The plan fuses the staged octave 0 (largest radius <= 16); at S = 1 the
    radius is 19, octave 0 runs on the fp64 base and the scan decides it:
    the pass record says which of the two ran."""
    plain, fused = sift_amd.make_params(xc.EDGE_O, S), sift_amd.make_params(xc.EDGE_O, S, flags=sift_amd.F_FUSED_EXTREMA)
    rmax = max(octave_radii(plain)[0])
    assert (rmax <= 16) == (S >= 2), rmax
    for seed in xc.EDGE_SEEDS[S]:
        img, r = _edge_run(S, seed)
        a = gpu_ctx.detect(img, plain).copy()
        ca, na = gpu_ctx.candidates(), gpu_ctx.counts()
        o0 = dict(e.split(": ", 1) for e in gpu_ctx.pass_kernels().split("; "))["o0"]
        assert "fused" not in o0, o0
        b = gpu_ctx.detect(img, fused).copy()
        cb, nb = gpu_ctx.candidates(), gpu_ctx.counts()
        f0 = dict(e.split(": ", 1) for e in gpu_ctx.pass_kernels().split("; "))["o0"]
        assert f0 == (FUSED_NAME if S >= 2 else BASE0_NAME), f0
        assert (S >= 2) or f0 == o0
        assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
        assert na["low_contrast"] == nb["low_contrast"] == r.n_low and na["candidates"] == nb["candidates"]
        check_candidates(cb, r.candidates())
        check_keypoints(b, r.refined)
