"""State and argument checks of the detection entry points (sift_find_extrema, sift_refine, the sift_detect*
family, sift_order_after): what each returns on a fresh context, with a detection in flight, for a bad batch or a
short buffer, and which earlier results a new detection invalidates.  Every case is an early return or a small
complete detection (64x48, 3 octaves, 3 scales)."""
import ctypes

import numpy as np
import pytest
import torch

import sift_amd
from sift_amd import SIFT_E_ARG, SIFT_E_CAPACITY, SIFT_E_STATE, SIFT_E_UNSUPPORTED, SIFT_OK
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

W, H = 64, 48
_shared = {}


def params():
    return sift_amd.make_params(3, 3)


def shared(gpu_ctx):
    """The image on the host and on the device, and its keypoints from one synchronous detect_device on a context
    of its own (read-only; gpu_ctx only orders the device's initialisation)."""
    if not _shared:
        img = np.ascontiguousarray(blob_image(W, H, seed=1, noise=0.1), dtype=np.float32)
        d_img = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        with sift_amd.Context(0) as c:
            assert c.detect_device(d_img.data_ptr(), W, H, params()) > 0
            kp = c.keypoints()
        img.setflags(write=False)
        kp.setflags(write=False)
        _shared.update(img=img, d_img=d_img, kp=kp)
    return _shared


@pytest.fixture
def ctx(gpu_ctx):
    """A fresh context (gpu_ctx first: it initialises the device in the order the suite needs)."""
    with sift_amd.Context(0) as c:
        yield c


def test_fresh_context_refuses_every_stage(ctx):
    L, h, n = sift_amd.lib(), ctx._h, ctypes.c_size_t()
    r, c = ctypes.c_int(), ctypes.c_int()
    plane = np.zeros(4 * W * H, dtype=np.float32)
    calls = {
        "sift_find_extrema": lambda: L.sift_find_extrema(h, None, 0, ctypes.byref(n), None),
        "sift_refine": lambda: L.sift_refine(h, None, 0, ctypes.byref(n), None),
        "sift_detect_wait": lambda: L.sift_detect_wait(h, None, 0, ctypes.byref(n)),
        "sift_detect_end_async": lambda: L.sift_detect_end_async(h),
        "sift_copy_candidates": lambda: L.sift_copy_candidates(h, None, 0, ctypes.byref(n)),
        "sift_copy_low_contrast": lambda: L.sift_copy_low_contrast(h, None, 0, ctypes.byref(n)),
        "sift_next_seed": lambda: L.sift_next_seed(h, None, 0, ctypes.byref(r), ctypes.byref(c)),
        "sift_get_plane": lambda: L.sift_get_plane(h, sift_amd.PLANE_DOG, 0, 0,
                                                   plane.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), plane.size),
    }
    for name, call in calls.items():
        assert call() == SIFT_E_STATE, name


def test_second_async_detection_is_refused_and_the_first_completes(gpu_ctx, ctx):
    s, L, p = shared(gpu_ctx), sift_amd.lib(), params()
    ctx.detect_device_async(s["d_img"].data_ptr(), W, H, p)
    assert L.sift_detect_device_async(ctx._h, s["d_img"].data_ptr(), W, H, W, ctypes.byref(p)) == SIFT_E_STATE
    assert ctx.detect_wait() == len(s["kp"])
    assert ctx.keypoints().tobytes() == s["kp"].tobytes()
    assert L.sift_detect_wait(ctx._h, None, 0, None) == SIFT_E_STATE


def test_detection_begun_refuses_another_and_still_completes(gpu_ctx, ctx):
    s, L, p = shared(gpu_ctx), sift_amd.lib(), params()
    ctx.detect_begin_async(s["d_img"].data_ptr(), W, H, p)
    assert L.sift_detect_device_async(ctx._h, s["d_img"].data_ptr(), W, H, W, ctypes.byref(p)) == SIFT_E_STATE
    ctx.detect_end_async()
    assert ctx.detect_wait() == len(s["kp"])
    assert ctx.keypoints().tobytes() == s["kp"].tobytes()
    assert L.sift_detect_wait(ctx._h, None, 0, None) == SIFT_E_STATE


def test_batch_arguments_and_candidates_of_a_batch(gpu_ctx, ctx):
    s, L, p, n = shared(gpu_ctx), sift_amd.lib(), params(), ctypes.c_size_t()
    d2 = torch.stack([s["d_img"], s["d_img"]]).contiguous()
    torch.cuda.synchronize()

    def batch(n_images, image_stride):
        return L.sift_detect_batch_device(ctx._h, d2.data_ptr(), n_images, image_stride, W, H, W, ctypes.byref(p),
                                          None, 0, ctypes.byref(n))

    assert batch(0, W * H) == SIFT_E_ARG
    assert batch(2, W * H - 1) == SIFT_E_ARG
    assert batch(2, W * H) == SIFT_OK
    assert n.value == 2 * len(s["kp"])
    assert list(ctx.batch_counts(2)) == [len(s["kp"])] * 2
    assert L.sift_copy_candidates(ctx._h, None, 0, ctypes.byref(n)) == SIFT_E_UNSUPPORTED


def test_short_keypoint_buffer_reports_the_count(gpu_ctx, ctx):
    s, L, p, n = shared(gpu_ctx), sift_amd.lib(), params(), ctypes.c_size_t()
    want = len(s["kp"])
    out = np.zeros(want, dtype=sift_amd.KEYPOINT_DTYPE)
    img = s["img"].ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = L.sift_detect(ctx._h, img, W, H, W, ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p), want - 1,
                       ctypes.byref(n))
    assert rc == SIFT_E_CAPACITY and n.value == want
    assert not out.view(np.uint8).any()
    rc = L.sift_detect(ctx._h, img, W, H, W, ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p), want,
                       ctypes.byref(n))
    assert rc == SIFT_OK and out.tobytes() == s["kp"].tobytes()


def test_new_detection_invalidates_the_feature_results(gpu_ctx, ctx):
    s, L, p, n, nd = shared(gpu_ctx), sift_amd.lib(), params(), ctypes.c_size_t(), ctypes.c_size_t()
    assert ctx.detect(s["img"], p).tobytes() == s["kp"].tobytes()
    ori = ctx.orient()
    desc, _ = ctx.describe()
    assert len(ori) > 0 and len(desc) == len(ori)
    ctx.detect(s["img"], p)
    assert L.sift_describe(ctx._h, None, None, 0, ctypes.byref(n), ctypes.byref(nd)) == SIFT_E_STATE
    assert ctx.orient().tobytes() == ori.tobytes()
    assert ctx.describe()[0].tobytes() == desc.tobytes()
    # the stages one by one on that pyramid find what the detection found
    cand, _ = ctx.find_extrema()
    assert len(cand) >= len(s["kp"])
    kp, _ = ctx.refine()
    assert kp.tobytes() == s["kp"].tobytes()
    assert L.sift_describe(ctx._h, None, None, 0, ctypes.byref(n), ctypes.byref(nd)) == SIFT_E_STATE


def test_order_after_arguments(gpu_ctx, ctx):
    L = sift_amd.lib()
    for after in (sift_amd.AFTER_REFINEMENT + 1, -1):
        assert L.sift_order_after(ctx._h, gpu_ctx._h, after) == SIFT_E_ARG
    assert L.sift_order_after(ctx._h, ctx._h, sift_amd.AFTER_GAUSSIAN) == SIFT_OK
    assert L.sift_order_after(ctx._h, gpu_ctx._h, sift_amd.AFTER_GAUSSIAN) == SIFT_OK
