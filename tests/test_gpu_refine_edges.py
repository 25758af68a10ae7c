"""Refinement at its thresholds, and the exact fallback (GPU).

Decision table (caller-supplied planes, the EXACT instantiation of
k_refine_fast): refine_cases.build_table puts every decision of refine_step
within one representable value of its threshold -- sweeps of consecutive
fp32 plane values / fp64 candidate values -- and constructs rounding ties,
moves onto every face of the interior and chains of one to five moves.  The
fp32 planes are the data, so every result equals the oracle's on the same
values: same kept set and order, same integers, the four reals to 1e-14
relative, the same singular count.

Native planes (tests/golden/refine_steered.npz, made on the CPU by
tests/golden/make_refine_steered.py): 25 images of 96 x 64 in which one
decision of one target candidate lies within half the error bound the fast
pass carries for it -- |omega| on thr (10 images, one pair at octave 2, one
pair with a second target on |alpha| = 0.6), an extremum's |value| on
0.8 thr (5, one of them with a target on each side), max |alpha_i| on 0.6
(6 with the pair above), edgeness on 12.1 (4), a move's rounding on k + 0.5
(2).  The images come in pairs, one on each side of the threshold, whose
keypoint lists differ in the target's record.  One detection per image
through the stage API: lists equal the oracle's, the refinement's exact
count covers the targets on top of the polish entries the mirror predicts,
the one-call path gives the same bytes, and every kept keypoint that is a
steered target or whose mirrored output bound exceeds 2 SIFT_KP_TOL equals
the oracle within TIGHT_TOL.  Two unsteered images add keypoints that only
the polish path makes exact.

TIGHT_TOL, measured on the CPU from the oracle alone: the largest
difference between the oracle's two separable summation orders
(CONV_SEPARABLE, CONV_SEPARABLE_FMA_VH) over exactly those keypoints of all
27 images is 3.04e-12 (sigma of an octave-2 keypoint, output bound 8.7e-5);
times 100: 3.1e-10.  The exact pass (sift_exact.h) differs from either
order only by summation order; the fast pass leaves 1e-6..1e-5 on such
keypoints, so a skipped exact or polish pass fails.
"""
import os

import numpy as np
import pytest

import oracle as orc
import refine_cases as rc
import sift_amd
from parity_util import check_candidates, check_keypoints, oracle_params
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

TIGHT_TOL = 3.1e-10
assert TIGHT_TOL <= 1e-8

_tables = {}


def _table(S):
    """The table, its oracle results and the kept candidates' indices (computed once per S)."""
    if S not in _tables:
        T = rc.build_table(S)
        flat, rec, val = T.arrays()
        r = orc.OracleRun.__new__(orc.OracleRun)
        r.W, r.H, r.p = rc.TABLE_W, rc.TABLE_H, orc.make_params(rc.TABLE_O, S)
        r.dog_flat = flat.astype(np.float64)
        out, sing = r.refine(rec, val)
        tr, kept, tsing = rc.trace_list([p.astype(np.float64) for p in T.planes], T.dims, rec, val, S)
        kept_idx = [i for i, t in enumerate(tr) if t.outcome == "keep"]
        assert len(kept_idx) == out.shape[0] and tsing == sing
        cand = np.zeros(rec.shape[0], dtype=sift_amd.EXTREMUM_DTYPE)
        cand["octave"], cand["scale"], cand["x"], cand["y"], cand["value"] = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], val
        _tables[S] = (T, flat, cand, out, sing, kept_idx)
    return _tables[S]


def _check_exact(kp, sing, out, osing):
    assert sing == osing
    assert kp.shape[0] == out.shape[0]
    ints = np.stack([kp["octave"], kp["scale_level"], kp["local_x"], kp["local_y"]], axis=1)
    np.testing.assert_array_equal(ints, out[:, :4].astype(np.int64))
    got = np.stack([kp["abs_sigma"], kp["abs_x"], kp["abs_y"], kp["interp_value"]], axis=1)
    np.testing.assert_allclose(got, out[:, 4:], rtol=1e-14, atol=0)


@pytest.mark.parametrize("S", [3, 5, 6])
def test_decision_table_equals_oracle(gpu_ctx, S):
    """Every sweep and single case in one candidate list of 2100 (nine blocks:
    xcd_block with a remainder), S = 3, 5 and 6 (thr depends on S; S = 6 has
    room for five moves along s onto a keepable bowl)."""
    T, flat, cand, out, osing, kept_idx = _table(S)
    assert osing >= 2 * (rc.SWEEP_LEN // 2 - 1), "both |det| sweeps reach the singular side"
    gpu_ctx.load_dog(flat, rc.TABLE_W, rc.TABLE_H, sift_amd.make_params(rc.TABLE_O, S))
    gpu_ctx.set_candidates(cand)
    kp, sing = gpu_ctx.refine()
    _check_exact(kp, sing, out, osing)
    # the same list again: the same bytes
    kp2, sing2 = gpu_ctx.refine()
    assert sing2 == sing and kp2.tobytes() == kp.tobytes()


def test_decision_table_origins(gpu_ctx):
    """F_KEYPOINT_ORIGINS: a keypoint's origin is its candidate, not the
    position its chain ended on (the table's chains move up to four pixels)."""
    T, flat, cand, out, osing, kept_idx = _table(3)
    gpu_ctx.load_dog(flat, rc.TABLE_W, rc.TABLE_H,
                     sift_amd.make_params(rc.TABLE_O, 3, flags=sift_amd.F_KEYPOINT_ORIGINS))
    gpu_ctx.set_candidates(cand)
    kp, sing = gpu_ctx.refine()
    _check_exact(kp, sing, out, osing)
    org = gpu_ctx.keypoint_origins()
    want = np.stack([cand["octave"], cand["scale"], cand["y"], cand["x"]], axis=1)[kept_idx]
    np.testing.assert_array_equal(org, want)
    moved = (org[:, 1] != kp["scale_level"]) | (org[:, 2] != kp["local_y"]) | (org[:, 3] != kp["local_x"])
    assert moved.sum() >= 6 * (rc.SWEEP_LEN // 2 - 1), "the moved sides of the alpha sweeps and the chains"


# ---------------------------------------------------------------------------
# Native planes steered onto the bounds, and the exact / polish paths
# ---------------------------------------------------------------------------
_STEERED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_steered.npz")
_z = []


def _steered(i):
    if not _z:
        _z.append(np.load(_STEERED))
    Z = _z[0]
    assert int(Z["n"]) == rc.N_STEERED
    kinds = [str(k) for k in Z["kind_%d" % i]]
    return Z["img_%d" % i], int(Z["params_%d" % i][0]), int(Z["params_%d" % i][1]), kinds, \
        [tuple(int(v) for v in t) for t in Z["target_%d" % i]]


def _check_native(gpu_ctx, img, O, S, kinds=(), targets=(), min_polish=0):
    """One detection through the stage API against the oracle; the exact path
    must have taken every steered target and written exact records."""
    p = sift_amd.make_params(O, S, flags=sift_amd.F_LOW_CONTRAST_LIST)
    r = orc.OracleRun(img, oracle_params(p), orc.CONV_SEPARABLE)
    H, W = img.shape
    gpu_ctx.build_scale_space(img, p)
    cand, low = gpu_ctx.find_extrema()
    n_amb = gpu_ctx.counts()["exact"]          # the extrema stage's near-threshold / tie list
    check_candidates(cand, r.candidates())
    assert low == r.n_low
    check_candidates(gpu_ctx.low_contrast(), r.low_contrast())
    kp, sing = gpu_ctx.refine()
    n_unc = gpu_ctx.counts()["exact"] - n_amb  # the refinement adds its uncertain AND polish entries
    check_keypoints(kp, r.refined)
    assert sing == r.n_singular
    assert n_amb >= sum(k == "pixthr" for k in kinds), (n_amb, kinds)
    # kept keypoints the exact pass must have written: steered targets, and output bounds above the polish bar
    tr, kept, _ = rc.trace_list(r.dog, r.dims, r.cand_rec, r.cand_val, S, native=True)
    kept_tr = [t for t in tr if t.outcome == "keep"]
    assert len(kept_tr) == r.refined.shape[0]
    ref_targets = {t for k, t in zip(kinds, targets) if k != "pixthr"}
    polish = [j for j, t in enumerate(kept_tr) if t.polish]
    assert len(polish) >= min_polish, "the mirror of the output bound predicts polish entries here"
    # the count net of polish: polish entries go through the same list, so the targets must come on top of
    # those the mirror predicts (the ones clear of the bar; a target is uncertain, never a polish entry)
    assert not any(kept_tr[j].origin in ref_targets for j in polish)
    sure_polish = sum(float(kept_tr[j].steps[-1].bounds["out"]) > 1.01 * rc.KP_TOL for j in polish)
    assert n_unc >= len(ref_targets) + sure_polish, (n_unc, len(ref_targets), sure_polish, kinds)
    bar = rc.KP_TOL if min_polish else 2 * rc.KP_TOL
    tight = [j for j, t in enumerate(kept_tr)
             if t.origin in ref_targets or float(t.steps[-1].bounds["out"]) > bar]
    if min_polish:   # every predicted entry is clear of the bar, so the kernel's own bound agrees
        assert all(abs(float(kept_tr[j].steps[-1].bounds["out"]) / rc.KP_TOL - 1) > 0.01 for j in polish)
        assert set(polish) <= set(tight)
    got = np.stack([kp["abs_sigma"], kp["abs_x"], kp["abs_y"], kp["interp_value"]], axis=1)
    np.testing.assert_allclose(got[tight], r.refined[tight, 4:], rtol=0, atol=TIGHT_TOL)
    # the one-call path: the same bytes as the stage chain
    kp1 = gpu_ctx.detect(img, p)
    assert kp1.tobytes() == kp.tobytes()
    return len(tight)


@pytest.mark.parametrize("i", range(rc.N_STEERED))
def test_steered_image(gpu_ctx, i):
    """One stored image: its target's decision lies inside the fast pass's
    bound, so the exact path decides it -- as the oracle does."""
    img, O, S, kinds, targets = _steered(i)
    _check_native(gpu_ctx, img, O, S, kinds, targets)


@pytest.mark.parametrize("W,H,O,S,seed,noise", [(96, 64, 4, 3, 7, None), (128, 128, 5, 3, 5, 0.01)])
def test_polish_entries_are_exact(gpu_ctx, W, H, O, S, seed, noise):
    """Unsteered images in which kept keypoints' output bounds exceed
    SIFT_KP_TOL (every decision certain): the polish path rewrites them from
    exact fp64 patches."""
    img = blob_image(W, H, seed=seed) if noise is None else blob_image(W, H, seed=seed, noise=noise)
    assert _check_native(gpu_ctx, img, O, S, min_polish=2) >= 2
