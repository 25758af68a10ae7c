"""The refinement's test inputs are what they claim to be (CPU).

* the restated chain (refine_cases.trace) equals oracle_refine on a blob
  image and on the decision table: same outcomes, kept records and singular
  count -- it is only used to label inputs, so it must label them right;
* every sweep of the table has both outcomes of its decision, the flip lies
  between two consecutive values, and every single case ends as built;
* every stored steered image (tests/golden/refine_steered.npz) still meets
  its acceptance conditions when recomputed from the committed pixels, so a
  regenerated or hand-edited fixture cannot quietly go vacuous.
"""
import os

import numpy as np
import pytest

import oracle as orc
import refine_cases as rc
from sift_amd.synth import blob_image


@pytest.fixture(scope="module", params=[3, 5, 6])
def table(request):
    return rc.build_table(request.param)


def _table_run(T):
    flat, rec, val = T.arrays()
    r = orc.OracleRun.__new__(orc.OracleRun)
    r.W, r.H, r.p = rc.TABLE_W, rc.TABLE_H, orc.make_params(rc.TABLE_O, T.S)
    r.dog_flat = flat.astype(np.float64)
    return r, rec, val


def test_trace_equals_oracle_on_blob_image():
    img = blob_image(96, 64, seed=7)
    p = orc.make_params(4, 3)
    r = orc.OracleRun(img, p, orc.CONV_SEPARABLE)
    tr, kept, sing = rc.trace_list(r.dog, r.dims, r.cand_rec, r.cand_val, 3)
    assert kept.shape[0] == r.refined.shape[0] > 50
    np.testing.assert_array_equal(kept[:, :4], r.refined[:, :4])
    np.testing.assert_allclose(kept[:, 4:], r.refined[:, 4:], rtol=1e-15, atol=0)
    assert sing == r.n_singular
    assert {t.outcome for t in tr} >= {"keep", "low_contrast", "edge"}


def test_trace_equals_oracle_on_table(table):
    r, rec, val = _table_run(table)
    out, sing = r.refine(rec, val)
    planes = [p.astype(np.float64) for p in table.planes]
    tr, kept, tsing = rc.trace_list(planes, table.dims, rec, val, table.S)
    assert tsing == sing > 0
    assert kept.shape == out.shape
    np.testing.assert_array_equal(kept[:, :4], out[:, :4])
    np.testing.assert_allclose(kept[:, 4:], out[:, 4:], rtol=1e-15, atol=0)


def test_table_shape_and_sweeps(table):
    n = len(table.rec)
    nb = (n + 255) // 256
    assert nb > 8 and nb % 8 != 0, "the list must run xcd_block with a remainder"
    assert set(table.sweeps) == {"alpha0+", "alpha0-", "alpha1+", "alpha1-", "alpha2+", "alpha2-", "edge", "det-",
                                 "det+", "omega"}
    for name, (idx, probe) in table.sweeps.items():
        assert len(idx) >= 64, name
        lab = [probe(table.trace(i)) for i in idx]
        assert any(lab) and not all(lab), name
        assert sum(a != b for a, b in zip(lab, lab[1:])) == 1, (name, "one flip between consecutive values")
        # the swept quantity moves by consecutive representable values
        if name == "omega":
            v = np.array([table.val[i] for i in idx])
            assert np.all(np.abs(np.diff(v.view(np.int64))) == 1)
    # sweeps whose two sides end differently in the kept list
    for name in ("edge", "det-", "det+", "omega"):
        outs = {table.trace(i).outcome for i in table.sweeps[name][0]}
        assert len(outs) == 2, (name, outs)
    for name in ("alpha0+", "alpha0-", "alpha1+", "alpha1-", "alpha2+", "alpha2-"):
        moves = {table.trace(i).moves for i in table.sweeps[name][0]}
        assert moves == {0, 1}, (name, moves)


def test_table_single_cases(table):
    for name, want in table.expect.items():
        t = table.trace(table.cases[name][0])
        assert t.outcome == want, (name, t.outcome)
        if name.startswith("chain_"):
            k = int(name[-1])
            assert t.moves == k, (name, t.moves)
            if want == "keep":  # the record carries the final position
                o, s, x, y = table.rec[table.cases[name][0]]
                ax = "syx".index(name[6])
                fin = [s, y, x]
                fin[ax] += k
                assert [t.kept[1], t.kept[3], t.kept[2]] == fin
    # ties toward +inf: m - 1.5 -> m - 1, m + 1.5 -> m + 2, m + 2.5 -> m + 3
    for name in table.expect:
        if name.startswith("tie"):
            ax, gi = int(name[3]), float(name[5:])
            i = table.cases[name][0]
            o, s, x, y = table.rec[i]
            t = table.trace(i)
            assert t.steps[0].alpha[ax] == gi
            land = {1.5: 2, -1.5: -1, 2.5: 3}[gi]
            assert (t.kept[1], t.kept[3], t.kept[2])[ax] == (s, y, x)[ax] + land
    if table.S == 6:  # five moves along s arrive on a bowl that a start next to it keeps
        assert table.expect["chain_s5"] == "five_moves" and table.expect["chain_s4"] == "keep"
        o, s, x, y = table.rec[table.cases["chain_s5"][0]]
        t = table.trace(table.cases["chain_s5"][0])
        assert [st.pos for st in t.steps] == [(s + k, y, x) for k in range(5)]
        assert rc.trace(table.planes[o].astype(np.float64), o, s + 5, y, x, 1.0, 6).outcome == "keep"
    want = {"tie1_+1.5", "tie1_-1.5", "tie1_+2.5", "tie2_+1.5", "tie2_-1.5", "tie2_+2.5", "tie0_+1.5", "tie0_-1.5"}
    assert want <= set(table.expect)
    for ax in range(3):
        for nm in ("inner", "first", "last"):
            assert "face%d_%s" % (ax, nm) in table.expect
        for sg in ("+1", "-1"):
            assert "huge%d%s" % (ax, sg) in table.expect and "inf%d%s" % (ax, sg) in table.expect
            t = table.trace(table.cases["huge%d%s" % (ax, sg)][0])
            assert abs(abs(float(t.steps[0].alpha[ax])) / 1e30 - 1) < 1e-6



def _half_down(v):
    return np.ceil(v - 0.5)


def _half_even(v):
    return np.round(v)


@pytest.mark.parametrize("name,value", [
    ("js_round", _half_down), ("js_round", _half_even),
    ("ALPHA_MAX", 0.6 * (1 + 3e-7)), ("ALPHA_MAX", 0.6 * (1 - 3e-7)),
    ("EDGE_THR", 12.1 * (1 + 3e-7)), ("EDGE_THR", 12.1 * (1 - 3e-7)),
    ("DBL_EPSILON", rc.DBL_EPSILON * (1 + 1e-6)), ("DBL_EPSILON", rc.DBL_EPSILON * (1 - 1e-6)),
    ("contrast_threshold", lambda S, f=rc.contrast_threshold: float(rc.f64_step(f(S), 8))),
    ("contrast_threshold", lambda S, f=rc.contrast_threshold: float(rc.f64_step(f(S), -8))),
])
def test_table_notices_a_wrong_rule(monkeypatch, name, value):
    """The restated chain with one rule slightly off -- another tie rule
    (ties to even or downwards; positions are positive, so rounding half away
    from zero IS the reference's rule on every reachable input), a
    threshold moved by a few fp32 steps of the swept entry (eight fp64 steps
    for thr) -- no longer gives the oracle's list on the table: a kernel with
    that rule fails test_gpu_refine_edges.py."""
    T = rc.build_table(3)
    r, rec, val = _table_run(T)
    out, sing = r.refine(rec, val)
    monkeypatch.setattr(rc, name, value)
    planes = [p.astype(np.float64) for p in T.planes]
    _, kept, tsing = rc.trace_list(planes, T.dims, rec, val, T.S)
    assert tsing != sing or kept.shape != out.shape or not np.array_equal(kept, out)


# ---------------------------------------------------------------------------
# tests/golden/refine_steered.npz
# ---------------------------------------------------------------------------
# kind -> images the fixture must hold of it (both sides of the threshold among them)
STEERED_KINDS = {"omega": 4, "pixthr": 4, "alpha": 4, "edge": 4, "round": 1}
_STEERED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_steered.npz")


@pytest.fixture(scope="module")
def steered():
    z = np.load(_STEERED)
    items = []
    for i in range(int(z["n"])):
        O, S = (int(v) for v in z["params_%d" % i])
        rows = [(str(k), tuple(int(v) for v in t), float(m), float(b)) for k, t, m, b in
                zip(z["kind_%d" % i], z["target_%d" % i], z["margin_%d" % i], z["bound_%d" % i])]
        items.append((z["img_%d" % i], O, S, rows))
    return items


def test_steered_fixture_is_small():
    assert os.path.getsize(_STEERED) < 1000000


def test_steered_images_meet_their_conditions(steered):
    """Recomputed from the committed pixels: margin <= bound / 2, margin >=
    1e-12 of the threshold, no earlier decision of the chain inside its own
    bound, and the same lists under both separable orders (rc.accept)."""
    for img, O, S, rows in steered:
        assert img.dtype == np.float32 and img.shape[0] * img.shape[1] <= 96 * 64
        for kind, tgt, margin, bound in rows:
            a = rc.accept(img, O, S, tgt, kind)
            assert a is not None, (kind, tgt)
            # the stored figures, up to another libm's last bits: the side and the bound hold
            assert abs(a[1] / bound - 1) < 1e-6 and abs(a[0] - margin) < 1e-3 * bound, (kind, tgt, a, margin, bound)
            assert (a[0] > 0) == (margin > 0) and abs(a[0]) <= a[1] / 2


def test_steered_targets_cover_the_issue(steered):
    rows = [(r, O) for img, O, S, rr in steered for r in rr]

    def sides(kind):
        return (sum(1 for r, _ in rows if r[0] == kind and r[2] > 0),
                sum(1 for r, _ in rows if r[0] == kind and r[2] < 0))

    for kind in STEERED_KINDS:
        above, below = sides(kind)
        assert above + below >= STEERED_KINDS[kind] and above >= 1 and below >= 1, (kind, above, below)
    assert any(r[1][0] >= 2 for r, _ in rows), "a target at octave >= 2"
    assert any(len(rr) == 2 for _, _, _, rr in steered), "one image with two steered targets"
    # a 0.8 thr target is a candidate on one side and a low-contrast extremum on the other, and one image
    # holds a target on each side, so one detection exercises the split
    both_sides = False
    for img, O, S, rr in steered:
        r = rc.oracle_run(img, O, S)
        for kind, tgt, margin, bound in rr:
            if kind == "pixthr":
                in_cand = (r.cand_rec == np.array(tgt, dtype=np.int32)).all(axis=1).any()
                in_low = (r.low_rec == np.array(tgt, dtype=np.int32)).all(axis=1).any()
                assert in_cand == (margin >= 0) and in_low == (margin < 0)
        pm = [m for kind, _, m, _ in rr if kind == "pixthr"]
        both_sides |= len(pm) == 2 and min(pm) < 0 < max(pm)
    assert both_sides, "one image with a 0.8 thr target on each side"
    # every bracket of a refinement decision: its two sides leave different keypoint lists (kept on one side
    # only, or another kept record), so a wrong decision on either image changes what the GPU test compares
    groups = {}
    for img, O, S, rr in steered:
        kind, tgt, margin, _ = rr[0]
        if kind != "pixthr":
            groups.setdefault((kind, tgt, O), {})[margin > 0] = rc.final_result(rc.oracle_run(img, O, S), S, tgt)
    assert {k[0] for k in groups} == {k for k in STEERED_KINDS if k != "pixthr"}
    for key, ends in groups.items():
        assert len(ends) == 2 and ends[True] != ends[False], (key, ends)
    assert int(np.load(_STEERED)["n"]) == rc.N_STEERED
