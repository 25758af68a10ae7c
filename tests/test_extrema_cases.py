"""The extrema scan's test inputs are what they claim to be (CPU).

* the restated scan (extrema_cases.reference_lists) equals the C oracle on
  every plant table and noise table: records, order and values bit for bit
  -- it only labels inputs, so it must label them right;
* every plant ends as built (candidate / low / none);
* coverage: every plant family on every geometry that has room for it, every
  expected class, the three kinds of block count, the widths and heights the
  geometries were chosen for; every interior column, row and scale of the
  noise pyramids; every tile / word / strip edge of the built pyramids'
  octave 0.  These assertions depend on the reference alone; they keep
  test_gpu_extrema_edges.py from passing on inputs that test nothing;
* the tables can fail: a scan that is wrong in one rule labels at least one
  plant differently (test_the_table_tells_wrong_scans_apart).
"""
import re

import numpy as np
import pytest

import extrema_cases as xc
import oracle as orc

TABLE_IDS = ["%dx%dO%d-S%d" % (g + (S,)) for g, S in xc.TABLES]
NOISE_IDS = ["S%d-seed%d" % (S, seed) for _, S, seed in xc.NOISE_TABLES]
THRESHOLD_LABELS = {"thr.%s%s" % (n, sg) for sg in "+-" for n in
                    ("t_up", "below", "denormal", "flt_min", "flt_max", "inf", "inf_equal", "inf_equal_s", "zero")}


def _same_lists(a, b):
    for (ra, va), (rb, vb) in zip(a, b):
        assert ra.shape == rb.shape
        np.testing.assert_array_equal(ra, rb)
        assert np.asarray(va, dtype=np.float64).tobytes() == np.asarray(vb, dtype=np.float64).tobytes()


def _oracle_lists(T):
    return orc.extrema_lists(orc.make_params(T.O, T.S), T.W, T.H, T.arrays().astype(np.float64))


def _roomy(T):
    """Every geometry but the three tiny ones -- (4,4), (10,10) and (6,14) as
    octave 0 -- which hold a handful of footprints per three scales: they
    are there for their heights (h - 2 = 1, 2, 3) and get what fits."""
    h, w = T.dims[0]
    return (h - 2) * (w - 2) >= 200


@pytest.mark.parametrize("geom,S", xc.TABLES, ids=TABLE_IDS)
def test_reference_equals_oracle_on_plant_table(geom, S):
    T = xc.build_table(geom, S)
    _same_lists(T.lists(), _oracle_lists(T))


@pytest.mark.parametrize("geom,S,seed", xc.NOISE_TABLES, ids=NOISE_IDS)
def test_reference_equals_oracle_on_noise_table(geom, S, seed):
    N = xc.noise_table(geom, S, seed)
    _same_lists(N.lists(), _oracle_lists(N))


@pytest.mark.parametrize("geom,S", xc.TABLES, ids=TABLE_IDS)
def test_plants_end_as_built(geom, S):
    T = xc.build_table(geom, S)
    lab = xc.labels_of(T.lists())
    wrong = [(p, lab.get(p[1:5], "none")) for p in T.plants if lab.get(p[1:5], "none") != p[5]]
    assert not wrong, wrong[:5]
    assert len({p[1:5] for p in T.plants}) == len(T.plants)
    if _roomy(T):
        assert {p[5] for p in T.plants} == {"candidate", "low", "none"}
    # the background holds nothing: every extremum lies inside a plant's footprint
    rec = np.concatenate([r for r, _ in T.lists()])
    assert all(T.taken[o][s, y, x] for o, s, x, y in rec.tolist())


def test_thresholds_are_the_fp32_neighbours_of_the_fp64_one():
    for S in range(1, 10):
        t, thr = xc.fp32_threshold(S), 0.8 * xc.contrast_threshold(S)
        assert t.dtype == np.float32 and float(t) > thr > float(np.nextafter(t, np.float32(0)))
    assert [xc.scale_groups(S) for S in (5, 6, 7, 8, 9)] == [[1, 6], [1, 4, 7], [1, 5, 8], [1, 5, 9], [1, 6, 10]]


def test_geometries_cover_the_widths_heights_and_block_counts():
    dims = {d for g, S in xc.TABLES for d in xc.build_table(g, S).dims}
    assert {w for _, w in dims} >= {16, 31, 32, 62, 63, 64, 125, 126, 250, 3980}
    assert {h - 2 for h, _ in dims} >= {1, 2, 3, 4, 14, 15, 30, 31, 32, 64}
    assert {S for _, S in xc.TABLES} == {1, 2, 3, 5, 6, 7, 8, 9}
    nb = {xc.build_table(g, S).blocks for g, S in xc.TABLES}
    assert any(b < 8 for b in nb), nb
    assert any(b >= 8 and b % 8 == 0 for b in nb), nb
    assert any(b > 8 and b % 8 != 0 for b in nb), nb
    assert any((w + xc.WORD - 1) // xc.WORD > 64 for _, w in dims), "k_emit's second chunk"
    # both unequal splits of the scales (s_first = 1 + g per + min(g, rem) with rem != 0)
    assert {S for _, S in xc.TABLES if S > 5 and S % 2} == {7, 9}


@pytest.mark.parametrize("geom,S", xc.TABLES, ids=TABLE_IDS)
def test_plant_families_are_present(geom, S):
    T = xc.build_table(geom, S)
    labels = {p[0] for p in T.plants}
    at = {}
    for p in T.plants:
        at.setdefault(p[1], []).append(p)
    if not _roomy(T):
        assert len(T.plants) >= 1
        return
    assert THRESHOLD_LABELS <= labels
    for o, (h, w) in enumerate(T.dims):
        # an isolated maximum and minimum (pos.*) at every special column, row and scale of every octave
        pos = [p for p in at[o] if p[0].startswith("pos.")]

        def both(axis, v):
            got = {p[0].rsplit(".", 1)[1] for p in pos if p[axis] == v}
            return got == {"max", "min"}

        nw = (w + xc.WORD - 1) // xc.WORD
        for fam, cols in xc.position_columns(w, h, o).items():
            for x in cols:
                assert both(4, x), (o, "column", x)
        for rows in xc.special_rows(h).values():
            for y in rows:
                assert both(3, y), (o, "row", y)
        for sc in xc.special_scales(S).values():
            for s in sc:
                assert both(2, s), (o, "scale", s)
        # every scan-word boundary of a wide plane has a plant centre on at least one side
        cols = {p[4] for p in at[o]}
        for k in range(1, nw):
            if xc.WORD * k <= w - 2:
                assert {xc.WORD * k - 1, xc.WORD * k} & cols, (o, k)
    # the neighbour family's contexts
    h0, w0 = T.dims[0]
    want = {"scale1", "scaleS", "interior"}
    if any(xc.special_columns(w)["word"] for _, w in T.dims):
        want |= {"col62k-1", "col62k"}
    if any(y % xc.STRIP == 0 for h, _ in T.dims for y in xc.special_rows(h)["strip"]):
        want |= {"row30k"}
    if any(y % xc.STRIP == 1 for h, _ in T.dims for y in xc.special_rows(h)["strip"]):
        want |= {"row30k+1"}
    if S > xc.MAX_GROUP:
        want |= {"group_last", "group_first"}
    # (a plane that the constrained contexts fill leaves no room for the unconstrained one)
    assert want - {"interior"} <= set(T.contexts) <= want, (set(T.contexts), want)
    for name, idx in T.contexts.items():
        assert len(idx) == len(set(idx)) >= 1, (name, len(idx))
    for p in T.plants:   # a context's plants are where the context says
        m = re.match(r"nbr\.([^.]+)\.", p[0])
        if m:
            c, (_, o, s, y, x, _) = m.group(1), p
            g = xc.special_scales(S)["group"]
            assert {"col62k-1": x % xc.WORD == xc.WORD - 1, "col62k": x % xc.WORD == 0 and x > 0,
                    "row30k": y % xc.STRIP == 0, "row30k+1": y % xc.STRIP == 1 and y > 1, "scale1": s == 1,
                    "scaleS": s == S, "group_last": s in g[0::2], "group_first": s in g[1::2], "interior": True}[c], p
    # the lattice: 31 bits in every full word of two rows of octave 0, scale 1
    if h0 >= 32 and w0 >= xc.WORD:
        rec = np.concatenate([r for r, _ in T.lists()])
        for y in (11, 13):
            xs = rec[(rec[:, 0] == 0) & (rec[:, 1] == 1) & (rec[:, 3] == y), 2]
            for k in range(w0 // xc.WORD):
                full = xc.WORD * (k + 1) <= w0 - 1   # all 62 columns interior (word 0 lacks column 0)
                n = int(((xs >= xc.WORD * k) & (xs < xc.WORD * (k + 1))).sum())
                assert n == 31 or not full, (y, k, n)
            assert len(set(T.planes[0][1, y, 1:w0 - 1:2].tolist())) == len(range(1, w0 - 1, 2)), "distinct values"
    # more than 64 words: extrema in words 0, 63, 64 and the last of one row (two scales where S has two)
    nw0 = (w0 + xc.WORD - 1) // xc.WORD
    if nw0 > 64:
        rec = np.concatenate([r for r, _ in T.lists()])
        for s in {1, S}:
            words = set((rec[(rec[:, 1] == s) & (rec[:, 3] == 2), 2] // xc.WORD).tolist())
            assert words >= {0, 63, 64, nw0 - 1}, (s, sorted(words))


def test_neighbour_family_is_complete_over_the_tables():
    """All 26 offsets x {max, min} x 4 neighbour values in every context: the
    union over the tables (no single table has room for 208 plants on one
    column), and in one table for the unconstrained ones."""
    union = {}
    for g, S in xc.TABLES:
        for name, idx in xc.build_table(g, S).contexts.items():
            union.setdefault(name, set()).update(idx)
    assert set(union) == {"interior", "col62k-1", "col62k", "row30k", "row30k+1", "scale1", "scaleS", "group_last",
                          "group_first"}
    for name, idx in union.items():
        assert idx == set(range(len(xc.COMBOS))), (name, len(idx))
    assert len(xc.COMBOS) == 26 * 2 * 4
    for S in xc.S_FEW:
        T = xc.build_table((63, 33, 2), S)
        for name in ("interior", "scale1", "scaleS") + (("group_last", "group_first") if S > 5 else ()):
            assert len(T.contexts[name]) == len(xc.COMBOS), (S, name)


@pytest.mark.parametrize("S", xc.S_ALL)
def test_noise_tables_reach_every_position(S):
    got, want = set(), set()
    for seed in xc.NOISE_SEEDS[S]:
        N = xc.noise_table(xc.NOISE_GEOM, S, seed)
        (rec, val), (low, lval) = N.lists()
        assert rec.shape[0] > 100 and low.shape[0] > 100, "both lists"
        assert 0.25 < low.shape[0] / (rec.shape[0] + low.shape[0]) < 0.75
        assert (np.abs(val) == float(N.t)).any(), "|v| on the threshold itself"
        for o, s, x, y in np.concatenate([rec, low]).tolist():
            got |= {(o, "x", x), (o, "y", y), (o, "s", s)}
        # ties: a large share of neighbour pairs are equal
        p = N.planes[0]
        assert (p[:, :, 1:] == p[:, :, :-1]).mean() > 0.02
    for o, (h, w) in enumerate(N.dims):
        want |= {(o, "x", x) for x in range(1, w - 1)} | {(o, "y", y) for y in range(1, h - 1)}
        want |= {(o, "s", s) for s in range(1, S + 1)}
    assert want <= got, sorted(want - got)[:10]


@pytest.mark.parametrize("S", range(1, 10))
def test_edge_images_reach_every_edge(S):
    """Built pyramids (the HIP path's summation order): the chosen images'
    extrema hit every edge column, edge row and scale of octave 0."""
    p = orc.make_params(xc.EDGE_O, S)
    cols, rows, scales = set(), set(), set()
    assert 1 <= len(xc.EDGE_SEEDS[S]) <= 6
    for seed in xc.EDGE_SEEDS[S]:
        r = orc.OracleRun(xc.edge_image(seed), p, orc.CONV_SEPARABLE_FMA_VH)
        assert r.dims[0] == (92, 182)
        c, y, s = xc.edge_hits(r, S)
        cols, rows, scales = cols | c, rows | y, scales | s
    assert cols == set(xc.EDGE_COLUMNS) and rows == set(xc.EDGE_ROWS) and scales == set(range(1, S + 1))
    assert set(xc.EDGE_COLUMNS) == {1, 59, 60, 61, 62, 63, 64, 119, 120, 121, 122, 123, 124, 125, 126, 179, 180}


# one wrong rule each
WRONG_SCANS = ([("ge", dict(ge=True))] + [("drop%d" % k, dict(drop=k)) for k in range(26)] +
               [("nan_drop", dict(nan_drop=True)), ("thr_gt", dict(thr_gt=True)), ("ftz", dict(ftz=True))])
# every geometry at the S with the most contexts, the two small ones at S = 1 as well
_WRONG_ON = [(g, 7) for g in xc.GEOMETRIES] + [(g, 1) for g in xc.GEOMETRIES[:2]]


@pytest.mark.parametrize("name,wrong", WRONG_SCANS, ids=[n for n, _ in WRONG_SCANS])
def test_the_table_tells_wrong_scans_apart(name, wrong):
    """The restated scan with one rule wrong -- ties taken as extrema, one of
    the 26 neighbours not looked at, NaN neighbours skipped, the fp32
    threshold comparison strict, denormals flushed -- labels at least one
    plant differently from how it was built, on every table that holds a
    plant of the rule: a kernel with that rule fails
    test_gpu_extrema_edges.py there.  (No GPU involved.)"""
    told = 0
    for geom, S in _WRONG_ON:
        T = xc.build_table(geom, S)
        if not _roomy(T):
            continue
        if "drop" in wrong:   # tables with a plant whose neighbour at that offset defeats its centre
            pat = re.compile(r"nbr\.[^.]+\.%d\.(max|min)\.(equal|ulp_defeats|nan)$" % wrong["drop"])
            if not any(pat.match(p[0]) for p in T.plants):
                continue
        if "nan_drop" in wrong and not any(p[0].endswith(".nan") for p in T.plants):
            continue
        lab = xc.labels_of(T.lists(**wrong))
        changed = [p for p in T.plants if lab.get(p[1:5], "none") != p[5]]
        assert changed, (geom, S)
        told += 1
    assert told >= 5, told
