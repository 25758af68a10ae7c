"""sift_orient / sift_describe on the GPU against the numpy statement of their
definition (tests/feature_ref.py), on the GPU's own planes and keypoints.

The descriptor stage is checked on the GPU's own orientation records, as
sift_set_candidates lets the refinement be checked on the GPU's candidates.

Bounds.  theta: both sides sum their histograms in fp64 in different orders,
so the smoothed bins differ by ~1e-14 relative; a peak the reference does not
flag has |h[k-1] - 2 h[k] + h[k+1]| > 1e-9 max h, so the interpolated offset
(pi/36) (h[k-1] - h[k+1]) / (...) moves by less than (pi/36) * 1e-5 < 1e-6 rad.
Bytes: equal, except where the reference flags 512 f / n2 within 1e-9 of an
integer, where they may differ by 1.  Flags are capped (1 % of the keypoints,
0.1 % of the bytes per case) so the exceptions cannot swallow the check.
"""
import ctypes

import numpy as np
import pytest

import feature_ref as fr
import sift_amd
from sift_amd.synth import blob_image, constant_image

pytestmark = pytest.mark.gpu

# name: (width, height, blob_image arguments, octaves, scales, descriptor stride,
#        counts of the reference on the CPU oracle's planes: keypoints, border-rejected, records, multi-peak
#        keypoints, described (None = not recorded) -- each asserted to at least half)
CASES = {
    "A": (64, 48, dict(seed=1, noise=0.1), 3, 3, 1, (76, 23, 56, 3, 15)),
    "B": (128, 96, dict(seed=2, noise=0.1), 4, 5, 1, (650, 113, 701, 140, 537)),
    "C": (256, 192, dict(seed=11, noise=0.02, n_blobs=600), 4, 3, 1, (34, None, 31, None, 15)),
    "D": (131, 257, dict(seed=5, noise=0.1), 4, 6, 4, (1999, None, 2489, None, 2068)),
}
_cache = {}


def gpu_planes(ctx, p):
    return [[ctx.plane(sift_amd.PLANE_GAUSS, o, s) for s in range(p.scales_per_octave + 3)]
            for o in range(p.num_octaves)]


def run_case(ctx, name):
    """detect + orient + describe on the GPU and the reference on the GPU's planes, once per case."""
    if name not in _cache:
        w, h, kw, O, S, stride, counts = CASES[name]
        p = sift_amd.make_params(O, S)
        kp = ctx.detect(blob_image(w, h, **kw), p)
        planes = gpu_planes(ctx, p)
        ori = ctx.orient()
        desc, described = ctx.describe()
        ref_ori, amb = fr.orient(planes, kp, p)
        sel = np.arange(0, len(ori), stride)
        ref_desc, ref_described, flag = fr.describe(planes, kp, ori[sel])
        for a in (kp, ori, desc, described, ref_ori, amb, sel, ref_desc, ref_described, flag):
            a.setflags(write=False)
        _cache[name] = dict(kp=kp, ori=ori, desc=desc, described=described, ref_ori=ref_ori, amb=amb, sel=sel,
                            ref_desc=ref_desc, ref_described=ref_described, flag=flag, counts=counts, stride=stride)
    return _cache[name]


def per_keypoint(recs, n):
    return np.bincount(recs["keypoint"], minlength=n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_orientations_match_the_reference(gpu_ctx, name):
    c = run_case(gpu_ctx, name)
    kp, ori, ref, amb = c["kp"], c["ori"], c["ref_ori"], c["amb"]
    n = len(kp)
    n_kp, n_rej, n_rec, n_multi, _ = c["counts"]
    got_per, ref_per = per_keypoint(ori, n), per_keypoint(ref, n)
    print("case %s: %d keypoints, %d records (reference %d), %d flagged keypoints, %d rejected, %d multi-peak"
          % (name, n, len(ori), len(ref), int(amb.sum()), int((got_per == 0).sum()), int((got_per > 1).sum())))
    assert 2 * n >= n_kp and 2 * len(ori) >= n_rec
    if n_rej is not None:
        assert 2 * int((got_per == 0).sum()) >= n_rej
        assert 2 * int((got_per > 1).sum()) >= n_multi
    assert amb.sum() <= 0.01 * n
    assert (ori["keypoint"] >= 0).all() and (ori["keypoint"] < n).all()
    assert (np.diff(ori["keypoint"]) >= 0).all()
    assert got_per.max() <= 18
    assert ((ori["theta"] >= 0) & (ori["theta"] < 2 * np.pi)).all()
    keep_got, keep_ref = ~amb[ori["keypoint"]], ~amb[ref["keypoint"]]
    a, b = ori[keep_got], ref[keep_ref]
    assert (got_per[~amb] == ref_per[~amb]).all()
    assert (a["keypoint"] == b["keypoint"]).all() and (a["bin"] == b["bin"]).all()
    d = np.abs(a["theta"] - b["theta"])
    d = np.minimum(d, 2 * np.pi - d)
    print("case %s: max circular |d theta| = %.3e" % (name, d.max() if len(d) else 0.0))
    assert (d <= 1e-6).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_descriptors_match_the_reference_on_the_gpu_orientations(gpu_ctx, name):
    c = run_case(gpu_ctx, name)
    sel, flag = c["sel"], c["flag"]
    desc, described = c["desc"][sel], c["described"][sel]
    n_desc = c["counts"][4]
    print("case %s: %d of %d compared records described, %d flagged bytes"
          % (name, int(described.sum()), len(sel), int(flag.sum())))
    assert 2 * c["stride"] * int(described.sum()) >= n_desc
    assert flag.sum() <= 0.001 * flag.size
    assert (described == c["ref_described"]).all()
    assert not desc[~described].any()
    diff = np.abs(desc.astype(np.int32) - c["ref_desc"].astype(np.int32))
    print("case %s: %d bytes differ, %d of them unflagged" % (name, int((diff > 0).sum()), int((diff[~flag] > 0).sum())))
    assert (diff[~flag] == 0).all()
    assert (diff[flag] <= 1).all()


def test_two_runs_are_byte_identical(gpu_ctx):
    w, h, kw, O, S = CASES["B"][:5]
    img, p = blob_image(w, h, **kw), sift_amd.make_params(O, S)
    runs = []
    for _ in range(2):
        gpu_ctx.detect(img, p)
        ori = gpu_ctx.orient()
        desc, described = gpu_ctx.describe()
        runs.append((ori.tobytes(), desc.tobytes(), described.tobytes()))
    assert runs[0] == runs[1]
    c = run_case(gpu_ctx, "B")
    assert runs[0] == (c["ori"].tobytes(), c["desc"].tobytes(), c["described"].tobytes())
    with sift_amd.Context(0) as other:  # another context, another stream
        other.detect(img, p)
        ori = other.orient()
        desc, described = other.describe()
    assert runs[0] == (ori.tobytes(), desc.tobytes(), described.tobytes())


def test_stage_chain_equals_detect(gpu_ctx):
    w, h, kw, O, S = CASES["A"][:5]
    img, p = blob_image(w, h, **kw), sift_amd.make_params(O, S)
    c = run_case(gpu_ctx, "A")
    gpu_ctx.build_scale_space(img, p)
    gpu_ctx.find_extrema()
    kp, _ = gpu_ctx.refine()
    ori = gpu_ctx.orient()
    desc, described = gpu_ctx.describe()
    assert kp.tobytes() == c["kp"].tobytes()
    assert ori.tobytes() == c["ori"].tobytes()
    assert desc.tobytes() == c["desc"].tobytes() and (described == c["described"]).all()


def test_no_keypoints_is_ok_with_zero_records(gpu_ctx):
    kp = gpu_ctx.detect(constant_image(32, 32), sift_amd.make_params(3, 3))
    assert len(kp) == 0
    L, n, nd = gpu_ctx._L, ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.sift_orient(gpu_ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_OK and n.value == 0
    n.value = 7
    assert L.sift_describe(gpu_ctx._h, None, None, 0, ctypes.byref(n), ctypes.byref(nd)) == sift_amd.SIFT_OK
    assert (n.value, nd.value) == (0, 0)
    assert len(gpu_ctx.orient()) == 0
    desc, described = gpu_ctx.describe()
    assert desc.shape == (0, 128) and described.shape == (0,)


def test_capacity_one_too_small(gpu_ctx):
    w, h, kw, O, S = CASES["A"][:5]
    gpu_ctx.detect(blob_image(w, h, **kw), sift_amd.make_params(O, S))
    L, n, nd = gpu_ctx._L, ctypes.c_size_t(), ctypes.c_size_t()
    assert L.sift_orient(gpu_ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_OK
    need = n.value
    assert need > 1
    out = np.zeros(need, dtype=sift_amd.ORIENTATION_DTYPE)
    out["keypoint"] = -1
    n.value = 0
    assert L.sift_orient(gpu_ctx._h, out.ctypes.data_as(ctypes.c_void_p), need - 1, ctypes.byref(n)) == \
        sift_amd.SIFT_E_CAPACITY
    assert n.value == need and (out["keypoint"] == -1).all()
    desc = np.full((need, 128), 0xAB, dtype=np.uint8)
    n.value = 0
    assert L.sift_describe(gpu_ctx._h, desc.ctypes.data_as(ctypes.c_void_p), None, need - 1, ctypes.byref(n),
                           ctypes.byref(nd)) == sift_amd.SIFT_E_CAPACITY
    assert n.value == need and (desc == 0xAB).all()
    assert L.sift_describe(gpu_ctx._h, desc.ctypes.data_as(ctypes.c_void_p), None, need, ctypes.byref(n),
                           ctypes.byref(nd)) == sift_amd.SIFT_OK
    assert n.value == need and 0 < nd.value <= need


def test_state_errors():
    img, n = blob_image(64, 48, seed=1), ctypes.c_size_t()
    with sift_amd.Context(0) as ctx:
        L = ctx._L
        assert L.sift_orient(ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_E_STATE  # no refinement yet
        assert L.sift_describe(ctx._h, None, None, 0, ctypes.byref(n), None) == sift_amd.SIFT_E_STATE
        ctx.build_scale_space(img, sift_amd.make_params(3, 3))
        ctx.find_extrema()
        assert L.sift_orient(ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_E_STATE  # still none
        ctx.refine()
        assert L.sift_describe(ctx._h, None, None, 0, ctypes.byref(n), None) == sift_amd.SIFT_E_STATE  # before orient
        assert L.sift_device_features(ctx._h, None, None, None, ctypes.byref(n)) == sift_amd.SIFT_E_STATE
        assert len(ctx.orient()) > 0
        ctx.detect(img, sift_amd.make_params(3, 3, flags=sift_amd.F_SKIP_GAUSS_PLANES))
        assert L.sift_orient(ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_E_STATE  # no Gaussian planes


def test_batch_is_unsupported(gpu_ctx):
    imgs = np.stack([blob_image(64, 48, seed=1), blob_image(64, 48, seed=2)])
    kp = gpu_ctx.detect_batch(imgs, sift_amd.make_params(3, 3))
    assert len(kp) > 0
    n = ctypes.c_size_t()
    assert gpu_ctx._L.sift_orient(gpu_ctx._h, None, 0, ctypes.byref(n)) == sift_amd.SIFT_E_UNSUPPORTED
    assert gpu_ctx._L.sift_describe(gpu_ctx._h, None, None, 0, ctypes.byref(n), None) == sift_amd.SIFT_E_UNSUPPORTED


def test_device_pointers_hold_the_host_copies(gpu_ctx):
    hip = ctypes.CDLL("libamdhip64.so")  # the HIP runtime libsift_hip.so uses
    w, h, kw, O, S = CASES["A"][:5]
    gpu_ctx.detect(blob_image(w, h, **kw), sift_amd.make_params(O, S))
    ori = gpu_ctx.orient()
    desc, described = gpu_ctx.describe()
    d_ori, d_desc, d_ok, n = gpu_ctx.device_features()
    assert n == len(ori) > 0 and d_ori and d_desc and d_ok
    t = gpu_ctx.feature_timings()
    assert t["orient_ms"] > 0 and t["describe_ms"] > 0

    def device_bytes(ptr, nbytes):
        host = np.empty(nbytes, dtype=np.uint8)
        assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes),
                             2) == 0  # device to host
        return host.tobytes()

    assert device_bytes(d_ori, 16 * n) == ori.tobytes()
    assert device_bytes(d_desc, 128 * n) == desc.tobytes()
    assert device_bytes(d_ok, n) == described.astype(np.uint8).tobytes()
