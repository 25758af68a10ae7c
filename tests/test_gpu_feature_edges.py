"""k_orient / k_orient_emit / k_describe on hand-built inputs
(tests/feature_cases.py) through sift_set_keypoints and sift_set_orientations,
against the numpy statement of their definition (tests/feature_ref.py).

Every input of the kernels is the test's, so the expected counts are exact:
tests/test_feature_ref.py derives them on the CPU.  Bounds as in
tests/test_gpu_features.py: the same (keypoint, bin) records off the
reference's ambiguity mask, circular |d theta| <= 1e-6, `described` equal,
bytes equal off the flagged ones and within 1 on those; flags capped at 1 % of
the keypoints and 0.1 % of the bytes, which below 100 keypoints / 1000 bytes
means none.  One stated exemption: the four saturated bytes of the step plane
(case "c") are flagged because q = 256 exactly, and there both sides must
still give 255.
"""
import ctypes

import numpy as np
import pytest

import feature_cases as fc
import feature_ref as fr
import sift_amd
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * np.pi
_gpu = {}
_many = {}


def load(ctx, planes, geom):
    w, h, O, S = geom
    ctx.load_scale_space(sift_amd.flatten_pyramid(planes), w, h, sift_amd.make_params(O, S))


def features(ctx, planes, geom, kp, recs=None):
    """load -> set_keypoints -> orient (or set_orientations(recs)) -> describe: (ori, desc, described)."""
    load(ctx, planes, geom)
    ctx.set_keypoints(kp)
    if recs is not None:
        ctx.set_orientations(recs)
    ori = ctx.orient()
    desc, described = ctx.describe()
    return ori, desc, described


def run_case(ctx, name):
    """A case on the GPU, and the reference's descriptors of the GPU's records, once."""
    if name not in _gpu:
        c = fc.case(name)
        ori, desc, described = features(ctx, c["planes"], c["geom"], c["kp"])
        ref_desc, ref_described, flag = fr.describe(c["planes"], c["kp"], ori)
        for a in (ori, desc, described, ref_desc, ref_described, flag):
            a.setflags(write=False)
        _gpu[name] = dict(ori=ori, desc=desc, described=described, ref_desc=ref_desc, ref_described=ref_described,
                          flag=flag)
    return _gpu[name]


def circular(a, b):
    d = np.abs(a - b)
    return np.minimum(d, TWO_PI - d)


def assert_records(ori, ref, amb, n):
    """The existing orientation bounds; returns max |d theta|."""
    got_per, ref_per = np.bincount(ori["keypoint"], minlength=n), np.bincount(ref["keypoint"], minlength=n)
    assert amb.sum() <= 0.01 * n
    assert (ori["keypoint"] >= 0).all() and (ori["keypoint"] < n).all()
    assert (np.diff(ori["keypoint"]) >= 0).all()
    assert ((ori["theta"] >= 0) & (ori["theta"] < TWO_PI)).all()
    assert (got_per[~amb] == ref_per[~amb]).all()
    a, b = ori[~amb[ori["keypoint"]]], ref[~amb[ref["keypoint"]]]
    assert (a["keypoint"] == b["keypoint"]).all() and (a["bin"] == b["bin"]).all()
    d = circular(a["theta"], b["theta"])
    assert (d <= 1e-6).all()
    return float(d.max()) if len(d) else 0.0


def assert_bytes(desc, described, ref_desc, ref_described, flag, exempt=None):
    """The existing descriptor bounds; `exempt` marks flagged bytes that are outside the cap but must be equal."""
    capped = flag if exempt is None else flag & ~exempt
    assert capped.sum() <= 0.001 * flag.size
    assert (described == ref_described).all()
    assert not desc[~described].any()
    diff = np.abs(desc.astype(np.int32) - ref_desc.astype(np.int32))
    assert (diff[~capped] == 0).all()
    assert (diff[capped] <= 1).all()
    return int((diff > 0).sum())


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_orientations_match_the_reference(gpu_ctx, name):
    c, ref, g = fc.case(name), fc.reference(name), run_case(gpu_ctx, name)
    n, ori = len(c["kp"]), g["ori"]
    per = np.bincount(ori["keypoint"], minlength=n)
    n_rec, n_none, n_multi = c["counts"][:3]
    dmax = assert_records(ori, ref["ori"], ref["amb"], n)
    print("case %s: %d keypoints, %d records, %d without, %d multi-peak, max circular |d theta| = %.3e"
          % (name, n, len(ori), int((per == 0).sum()), int((per > 1).sum()), dmax))
    assert not ref["amb"].any()  # (tests/test_feature_ref.py) so the counts are exact
    assert (len(ori), int((per == 0).sum()), int((per > 1).sum())) == (n_rec, n_none, n_multi)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_descriptors_match_the_reference_on_the_gpu_orientations(gpu_ctx, name):
    c, g = fc.case(name), run_case(gpu_ctx, name)
    n_diff = assert_bytes(g["desc"], g["described"], g["ref_desc"], g["ref_described"], g["flag"])
    print("case %s: %d of %d records described, %d flagged bytes, %d bytes differ"
          % (name, int(g["described"].sum()), len(g["ori"]), int(g["flag"].sum()), n_diff))
    assert int(g["described"].sum()) == c["counts"][3]
    assert int((g["desc"] == 255).sum()) == c["counts"][4]


@pytest.mark.parametrize("name,first", [("a0", 0), ("a1", 6)])
def test_integer_ramps_land_on_their_bin_centres(gpu_ctx, name, first):
    """Every pixel of a diagonal ramp takes the tie branch of k_orient; theta
    is the bin centre k pi / 18 because the interpolation term (pi/36) (hm -
    hp) / (hm - 2 h + hp) has a numerator of a few ulp of h: below 1e-15 rad."""
    g = run_case(gpu_ctx, name)
    want = np.array([fc.RAMP_BINS[i] for i in fc.ramp_slots(first)] * fc.O)
    assert (g["ori"]["keypoint"] == np.arange(len(want))).all()
    assert g["ori"]["bin"].tolist() == want.tolist()
    d = circular(g["ori"]["theta"], want * np.pi / 18)
    print("case %s: max |theta - k pi / 18| = %.3e" % (name, d.max()))
    assert (d <= 1e-9).all()
    diagonal = want % 9 != 0
    assert ((g["desc"][diagonal] > 0).sum(axis=1) == 32).all()
    assert (g["desc"][diagonal].max(axis=1) == 128).all()


def test_border_decisions(gpu_ctx):
    c, g = fc.case("b"), run_case(gpu_ctx, "b")
    per = np.bincount(g["ori"]["keypoint"], minlength=len(c["kp"]))
    assert per.tolist() == fc.BORDER_HAS_RECORD
    x = c["kp"]["abs_x"] / 2.0 ** (c["kp"]["octave"] - 1.0)
    assert (g["described"] == (x[g["ori"]["keypoint"]] == 22.0)).all()
    assert g["desc"][g["described"]].any(axis=1).all() and not g["desc"][~g["described"]].any()


def test_degenerate_gradients(gpu_ctx):
    c = fc.case("c")
    g = run_case(gpu_ctx, "c")
    assert len(g["ori"]) == 0 and g["desc"].shape == (0, 128)
    recs = fc.degenerate_records()
    ori, desc, described = features(gpu_ctx, c["planes"], c["geom"], c["kp"], recs)
    assert ori.tobytes() == recs.tobytes()  # copied back, not recomputed (that would give no record)
    ref_desc, ref_described, flag = fr.describe(c["planes"], c["kp"], recs)
    step = fc.STEP_KEYPOINT
    assert described.all()
    assert not desc[:step].any()  # all-zero gradients: nrm == 0, zero bytes, nothing NaN-derived
    # the step: four values clamped to 0.2 * norm, q = 256 exactly -> 255.  The reference flags exactly these four
    # (4 of 128 is over the 0.1 % cap): exempt from the cap, and held to equality instead of +-1.
    exempt = np.zeros_like(flag)
    exempt[step, fc.STEP_BYTES] = True
    assert (flag == exempt).all()
    assert_bytes(desc, described, ref_desc, ref_described, flag, exempt)
    assert np.nonzero(desc[step])[0].tolist() == fc.STEP_BYTES and (desc[step][fc.STEP_BYTES] == 255).all()


def described_records_of_d(gpu_ctx):
    g = run_case(gpu_ctx, "d")
    recs = np.array(g["ori"][g["described"]])
    assert len(recs) == fc.case("d")["counts"][3]
    return recs


@pytest.mark.parametrize("theta", [0.0, np.pi / 4, np.pi / 2, np.pi, 3 * np.pi / 2, np.nextafter(TWO_PI, 0), 1e-300],
                         ids=["0", "pi_4", "pi_2", "pi", "3pi_2", "below_2pi", "1e-300"])
def test_chosen_thetas(gpu_ctx, theta):
    """k_describe's per-cell bounding box and the two-step wrap of atan2 - theta at the thetas blobs never give.
    (Bytes cannot tell the second `a += 2 pi` from its absence: `(int)tf & 7` maps a negative bin to the same bin
    and t - floor(t) is the same fraction, so only last-bit rounding moves.)"""
    c = fc.case("d")
    recs = fc.with_theta(described_records_of_d(gpu_ctx), theta)
    ori, desc, described = features(gpu_ctx, c["planes"], c["geom"], c["kp"], recs)
    assert ori.tobytes() == recs.tobytes()
    ref_desc, ref_described, flag = fr.describe(c["planes"], c["kp"], recs)
    n_diff = assert_bytes(desc, described, ref_desc, ref_described, flag)
    print("theta %r: %d records, %d flagged bytes, %d bytes differ" % (theta, len(recs), int(flag.sum()), n_diff))
    assert described.all() and desc.any(axis=1).all()


def test_quarter_turn_of_the_planes_turns_the_descriptors(gpu_ctx):
    """The rot90 property of tests/test_feature_ref.py, on the GPU: the
    quarter-turned planes with the moved keypoints and theta - pi/2 give the
    same bytes."""
    c = fc.case("d")
    recs = described_records_of_d(gpu_ctx)
    widths = [w for _, w in fc.dims()]
    turned, kpr, recs_r = fc.quarter_turn(c["planes"], c["kp"], recs, widths)
    _, desc, described = features(gpu_ctx, c["planes"], c["geom"], c["kp"], recs)
    _, desc_r, described_r = features(gpu_ctx, turned, (fc.H, fc.W, fc.O, fc.S), kpr, recs_r)
    _, _, flag = fr.describe(c["planes"], c["kp"], recs)
    _, ref_described_r, flag_r = fr.describe(turned, kpr, recs_r)
    assert described.all() and described_r.all() and ref_described_r.all()  # all 137 are compared
    free = ~(flag | flag_r)
    assert (~free).sum() <= 0.001 * free.size
    diff = np.abs(desc.astype(np.int32) - desc_r.astype(np.int32))
    print("quarter turn: %d descriptors, %d flagged bytes, %d bytes differ" % (len(recs), int((~free).sum()),
                                                                               int((diff > 0).sum())))
    assert (diff[free] == 0).all() and diff.max() <= 1


def test_four_peaks_in_ascending_bins(gpu_ctx):
    ref, g = fc.reference("g"), run_case(gpu_ctx, "g")
    assert g["ori"]["keypoint"].tolist() == [0] * 4
    assert g["ori"]["bin"].tolist() == ref["ori"]["bin"].tolist() == sorted(ref["ori"]["bin"].tolist())
    assert (circular(g["ori"]["theta"], ref["ori"]["theta"]) <= 1e-6).all()  # slot j holds the j-th peak's angle
    assert (np.diff(g["ori"]["theta"]) > 1.0).all()  # four lobes a quarter turn apart: no slot repeated


def many(gpu_ctx):
    """Case (h): 25 411 keypoints, a fixed shuffled repetition of 50 of case d's."""
    if not _many:
        d, ref = fc.case("d"), fc.reference("d")
        idx, distinct = fc.many_from(ref)
        kp = d["kp"][idx]
        ori, desc, described = features(gpu_ctx, d["planes"], d["geom"], kp)
        for a in (idx, kp, ori, desc, described):
            a.setflags(write=False)
        _many.update(idx=idx, distinct=distinct, kp=kp, ori=ori, desc=desc, described=described)
    return _many


def test_scan_and_emission_at_size(gpu_ctx):
    """Every record's (keypoint, bin, theta) -- hence every offset of the exclusive scan -- and the record count, over
    several scan tiles; the reference is evaluated once per distinct keypoint."""
    m, ref = many(gpu_ctx), fc.reference("d")
    idx, ori = m["idx"], m["ori"]
    per_d = np.bincount(ref["ori"]["keypoint"], minlength=len(ref["amb"]))
    first_d = np.concatenate([[0], np.cumsum(per_d)])
    per = per_d[idx]
    n_out = int(per.sum())
    assert sorted(set(per.tolist())) == [0, 1, 2]
    assert len(ori) == n_out
    want_kp = np.repeat(np.arange(fc.H_COUNT), per)
    slot = np.arange(n_out) - np.repeat(np.cumsum(per) - per, per)  # 0, or 0 1 within a keypoint
    want = ref["ori"][first_d[idx[want_kp]] + slot]
    assert (ori["keypoint"] == want_kp).all()
    assert (ori["bin"] == want["bin"]).all()
    d = circular(ori["theta"], want["theta"])
    print("scan at size: %d keypoints, %d records, max circular |d theta| = %.3e" % (fc.H_COUNT, n_out, d.max()))
    assert (d <= 1e-6).all()
    # a keypoint's records do not depend on where it stands in the list: bit-identical repeats
    src = first_d[idx[want_kp]] + slot
    _, first_at, inverse = np.unique(src, return_index=True, return_inverse=True)
    rep = first_at[inverse]  # the first occurrence of each record's (distinct keypoint, peak)
    assert (ori["theta"] == ori["theta"][rep]).all()
    # descriptors, with stride (as case D of tests/test_gpu_features.py), on the GPU's records
    sel = np.arange(0, n_out, 97)
    d_case = fc.case("d")
    ref_desc, ref_described, flag = fr.describe(d_case["planes"], m["kp"], ori[sel])
    assert_bytes(m["desc"][sel], m["described"][sel], ref_desc, ref_described, flag)
    assert ref_described.any() and not ref_described.all()
    # and every repeat of a record has the bytes of its first occurrence
    assert (m["desc"] == m["desc"][rep]).all() and (m["described"] == m["described"][rep]).all()


def test_buffers_regrow_between_lists_of_different_size(gpu_ctx):
    m, small = many(gpu_ctx), fc.case("a0")
    d = fc.case("d")

    def big(ctx):
        return tuple(a.tobytes() for a in features(ctx, d["planes"], d["geom"], m["kp"]))

    def little(ctx):
        return tuple(a.tobytes() for a in features(ctx, small["planes"], small["geom"], small["kp"]))

    with sift_amd.Context(0) as fresh:
        little_0 = little(fresh)
    with sift_amd.Context(0) as ctx:
        big_0 = big(ctx)  # on a fresh context
        assert little(ctx) == little_0
        assert big(ctx) == big_0
    assert big_0 == (m["ori"].tobytes(), m["desc"].tobytes(), m["described"].tobytes())
    g = run_case(gpu_ctx, "a0")
    assert little_0 == (g["ori"].tobytes(), g["desc"].tobytes(), g["described"].tobytes())


def test_describe_needs_orientations_of_the_new_list(gpu_ctx):
    c = fc.case("a0")
    features(gpu_ctx, c["planes"], c["geom"], c["kp"])
    gpu_ctx.set_keypoints(c["kp"][:5])
    n = ctypes.c_size_t()
    assert gpu_ctx._L.sift_describe(gpu_ctx._h, None, None, 0, ctypes.byref(n), None) == sift_amd.SIFT_E_STATE
    assert gpu_ctx._L.sift_device_features(gpu_ctx._h, None, None, None, ctypes.byref(n)) == sift_amd.SIFT_E_STATE
    assert len(gpu_ctx.orient()) == 5


def test_keypoints_round_trip(gpu_ctx):
    c = fc.case("d")
    load(gpu_ctx, c["planes"], c["geom"])
    gpu_ctx.set_keypoints(c["kp"])
    assert gpu_ctx.keypoints().tobytes() == c["kp"].tobytes()
    assert gpu_ctx.counts()["keypoints"] == len(c["kp"])
    gpu_ctx.set_keypoints(c["kp"][:0])
    assert len(gpu_ctx.keypoints()) == 0 and len(gpu_ctx.orient()) == 0
    assert gpu_ctx.describe()[0].shape == (0, 128)


def test_bad_records_are_rejected_and_change_nothing(gpu_ctx):
    c, L, h = fc.case("a0"), gpu_ctx._L, gpu_ctx._h
    ori, _, _ = features(gpu_ctx, c["planes"], c["geom"], c["kp"])
    n_kp = len(c["kp"])

    def set_ori(**field):
        r = np.array(ori[:3])
        for k, v in field.items():
            r[k][1] = v
        return L.sift_set_orientations(h, r.ctypes.data_as(ctypes.c_void_p), len(r))

    def set_kp(**field):
        k = np.array(c["kp"][:4])
        for name, v in field.items():
            k[name][2] = v
        return L.sift_set_keypoints(h, k.ctypes.data_as(ctypes.c_void_p), len(k))

    for bad in (dict(keypoint=n_kp), dict(keypoint=-1), dict(theta=TWO_PI), dict(theta=np.nan), dict(theta=np.inf),
                dict(theta=-1e-300), dict(bin=36), dict(bin=-1)):
        assert set_ori(**bad) == sift_amd.SIFT_E_ARG, bad
        assert gpu_ctx.orient().tobytes() == ori.tobytes()
    for bad in (dict(octave=-1), dict(octave=fc.O), dict(scale_level=fc.S + 3), dict(scale_level=-1)):
        assert set_kp(**bad) == sift_amd.SIFT_E_ARG, bad
        assert gpu_ctx.keypoints().tobytes() == c["kp"].tobytes()
        assert gpu_ctx.orient().tobytes() == ori.tobytes()
    assert L.sift_set_keypoints(h, None, 1) == sift_amd.SIFT_E_ARG
    assert L.sift_set_orientations(h, None, 1) == sift_amd.SIFT_E_ARG
    assert set_ori() == sift_amd.SIFT_OK and len(gpu_ctx.orient()) == 3
    assert set_kp() == sift_amd.SIFT_OK and len(gpu_ctx.keypoints()) == 4


def test_contexts_the_feature_stages_do_not_serve():
    """sift_set_keypoints returns what sift_orient would on the same context."""
    c = fc.case("a0")
    kp, L = np.array(c["kp"]), sift_amd.lib()
    p = sift_amd.make_params(fc.O, fc.S)

    def set_kp(ctx):
        return L.sift_set_keypoints(ctx._h, kp.ctypes.data_as(ctypes.c_void_p), len(kp))

    with sift_amd.Context(0) as ctx:
        assert set_kp(ctx) == sift_amd.SIFT_E_STATE  # no pyramid
        load(ctx, c["planes"], c["geom"])
        recs = np.zeros(1, dtype=sift_amd.ORIENTATION_DTYPE)
        assert L.sift_set_orientations(ctx._h, recs.ctypes.data_as(ctypes.c_void_p), 1) == sift_amd.SIFT_E_STATE
        n_dog = sum(h * w for h, w in fc.dims()) * (fc.S + 2)
        ctx.load_dog(np.zeros(n_dog, dtype=np.float32), fc.W, fc.H, p)
        assert set_kp(ctx) == sift_amd.SIFT_E_STATE  # no Gaussian planes
        ctx.detect(blob_image(fc.W, fc.H, seed=1), sift_amd.make_params(fc.O, fc.S, flags=sift_amd.F_SKIP_GAUSS_PLANES))
        assert set_kp(ctx) == sift_amd.SIFT_E_STATE
        ctx.detect_batch(np.stack([blob_image(fc.W, fc.H, seed=1), blob_image(fc.W, fc.H, seed=2)]), p)
        assert set_kp(ctx) == sift_amd.SIFT_E_UNSUPPORTED
        ctx.set_row_origin(2)
        load(ctx, c["planes"], c["geom"])
        assert set_kp(ctx) == sift_amd.SIFT_E_UNSUPPORTED
        ctx.set_row_origin(0)
        load(ctx, c["planes"], c["geom"])
        assert set_kp(ctx) == sift_amd.SIFT_OK


def test_set_keypoints_drops_the_refinement_by_products():
    p = sift_amd.make_params(fc.O, fc.S, flags=sift_amd.F_KEYPOINT_ORIGINS)
    with sift_amd.Context(0) as ctx:
        kp = ctx.detect(blob_image(fc.W, fc.H, seed=1), p)
        assert len(kp) > 4 and len(ctx.keypoint_origins()) == len(kp) and ctx.block_counts().sum() == len(kp)
        ctx.set_keypoints(kp[:4])
        n = ctypes.c_size_t()
        assert ctx._L.sift_keypoint_origins(ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_E_STATE
        assert len(ctx.block_counts()) == 0
        assert ctx.counts()["singular"] == 0 and ctx.counts()["keypoints"] == 4
        assert ctx.timings()["refine_ms"] == 0
        assert ctx.keypoints().tobytes() == kp[:4].tobytes()
        assert (np.diff(ctx.orient()["keypoint"]) >= 0).all()


def test_unusable_geometry_yields_no_record(gpu_ctx):
    """NaN, infinite, zero, negative and absurd coordinates or sigma: local_frame / inner_box reject each in fp64
    before any cast or address; the keypoints around them keep their records."""
    planes, kp = fc.unusable()
    geom = (fc.W, fc.H, fc.O, fc.S)
    bad = np.zeros(len(kp), dtype=bool)
    bad[list(fc.J_BAD)] = True
    good = np.nonzero(~bad)[0]
    ref, amb = fr.orient(planes, kp[good])
    assert not amb.any() and len(ref) >= 8
    ori, desc, described = features(gpu_ctx, planes, geom, kp)
    assert not bad[ori["keypoint"]].any()
    assert (ori["keypoint"] == good[ref["keypoint"]]).all() and (ori["bin"] == ref["bin"]).all()
    assert (circular(ori["theta"], ref["theta"]) <= 1e-6).all()
    ref_desc, ref_described, flag = fr.describe(planes, kp, ori)
    assert_bytes(desc, described, ref_desc, ref_described, flag)
    # k_describe on records that point at the unusable keypoints: not described, zero bytes
    recs = np.zeros(len(kp), dtype=sift_amd.ORIENTATION_DTYPE)
    recs["keypoint"] = np.arange(len(kp))
    recs["theta"] = 1.0
    _, desc, described = features(gpu_ctx, planes, geom, kp, recs)
    assert not described[bad].any() and not desc[bad].any()
    ref_desc, ref_described, flag = fr.describe(planes, kp[good], fc.with_theta(recs[:len(good)], 1.0))
    assert_bytes(desc[good], described[good], ref_desc, ref_described, flag)
    assert ref_described.any()
