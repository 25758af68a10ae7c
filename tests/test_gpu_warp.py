"""The homography warp on the device against its numpy restatement
(tests/warp_ref.py): destination, mask and count, compared on bytes."""
import ctypes
import mmap

import numpy as np
import pytest

import sift_amd
import warp_ref as wr
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

E_ARG = sift_amd.SIFT_E_ARG
SENTINEL = 0xA5
TILE_H = 16                     # rows of a block's tile (sift_warp.hip); its width is 64
DP = ctypes.POINTER(ctypes.c_double)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def is_rgba(src):
    return src.ndim == 3


def fill_arg(src, fill):
    """(the ctypes argument, the object that keeps it alive)"""
    if is_rgba(src):
        f = np.broadcast_to(np.asarray(fill, dtype=np.uint8), (4,)).copy()
        return f.ctypes.data_as(ctypes.c_void_p), f
    f = sift_amd.float_fill(fill if isinstance(fill, np.float32) else np.float32(fill))
    return f, f


def padded(img, pad_px, value=0):
    """img with pad_px more pixels in every row, the padding holding `value`
    bytes: float32 (rows, w + pad) or uint8 (rows, (w + pad) * 4)."""
    h, w = img.shape[:2]
    out = np.full((h, (w + pad_px) * 4), value, dtype=np.uint8)
    if is_rgba(img):
        out[:, :w * 4] = img.reshape(h, w * 4)
        return out
    out = out.view(np.float32)
    out[:, :w] = img
    return out


def sentinel_dst(src, oh, ow, pad_px):
    buf = np.full((oh, (ow + pad_px) * 4), SENTINEL, dtype=np.uint8)
    return buf if is_rgba(src) else buf.view(np.float32)


def split_dst(src, buf, oh, ow):
    """(the image part of a padded destination, the bytes of its padding)"""
    if is_rgba(src):
        return np.ascontiguousarray(buf[:, :ow * 4]).reshape(oh, ow, 4), buf[:, ow * 4:]
    return np.ascontiguousarray(buf[:, :ow]), buf[:, ow:].view(np.uint8)


def run_host(ctx, src, m, shape, mode=wr.BILINEAR, fill=0, spad=0, dpad=0, want_mask=True, want_count=True):
    """The host entry points on padded buffers: (dst, mask or None, n or None,
    padding untouched)."""
    L = sift_amd.lib()
    oh, ow = shape
    sh, sw = src.shape[:2]
    s, d = padded(src, spad), sentinel_dst(src, oh, ow, dpad)
    mm = np.ascontiguousarray(m, dtype=np.float64).reshape(9)
    mask = np.full((oh, ow), SENTINEL, dtype=np.uint8) if want_mask else None
    n = ctypes.c_size_t(12345)
    f, keep = fill_arg(src, fill)
    per = 4 if is_rgba(src) else 1
    fn = L.sift_warp_rgba if is_rgba(src) else L.sift_warp_gray
    rc = fn(ctx._h, s.ctypes.data_as(ctypes.c_void_p), sw, sh, (sw + spad) * per, mm.ctypes.data_as(DP), mode, f,
            d.ctypes.data_as(ctypes.c_void_p), ow, oh, (ow + dpad) * per,
            mask.ctypes.data_as(ctypes.c_void_p) if want_mask else None, ctypes.byref(n) if want_count else None)
    assert rc == 0, sift_amd.lib().sift_last_error(ctx._h)
    img, pad = split_dst(src, d, oh, ow)
    return img, mask, (n.value if want_count else None), bool((pad == SENTINEL).all())


def run_device(ctx, src, m, shape, mode=wr.BILINEAR, fill=0, spad=0, dpad=0, want_mask=True, want_count=True):
    """The same through the device entry points, on torch's device memory."""
    import torch
    L = sift_amd.lib()
    oh, ow = shape
    sh, sw = src.shape[:2]
    d_s = torch.from_numpy(padded(src, spad)).cuda()
    d_d = torch.from_numpy(sentinel_dst(src, oh, ow, dpad)).cuda()
    d_m = torch.full((oh, ow), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mm = np.ascontiguousarray(m, dtype=np.float64).reshape(9)
    n = ctypes.c_size_t(12345)
    f, keep = fill_arg(src, fill)
    per = 4 if is_rgba(src) else 1
    fn = L.sift_warp_rgba_device if is_rgba(src) else L.sift_warp_gray_device
    rc = fn(ctx._h, d_s.data_ptr(), sw, sh, (sw + spad) * per, mm.ctypes.data_as(DP), mode, f, d_d.data_ptr(), ow, oh,
            (ow + dpad) * per, d_m.data_ptr() if want_mask else None, ctypes.byref(n) if want_count else None)
    assert rc == 0, sift_amd.lib().sift_last_error(ctx._h)
    img, pad = split_dst(src, d_d.cpu().numpy(), oh, ow)
    return img, (d_m.cpu().numpy() if want_mask else None), (n.value if want_count else None), \
        bool((pad == SENTINEL).all())


def check(got, want, what):
    img, mask, n, pad_ok = got
    assert same_bytes(img, want[0]), what
    assert mask is None or same_bytes(mask, want[1]), what
    assert n is None or n == want[2], what
    assert pad_ok, what


def binding(ctx, src, m, shape, mode, fill):
    f = ctx.warp_rgba if is_rgba(src) else ctx.warp_gray
    return f(src, m, shape, mode, fill) + (True,)


# ---- the small cases: every source into every destination through every map ----------------
def test_every_small_case(gpu_ctx):
    """Sources 1x1, 1x5, 5x1, 2x2 and 67x35 into 3x2, 9x7 and 130x70 through the
    identity, integer and half-pixel shifts, scales that put the last column
    at sx == sw-1, a rotation with perspective, a horizon inside the
    destination, an inverted mirroring, all NaN, and 1e300 with m8 = 1e-300."""
    n = 0
    for name, src, m, shape, mode, fill in wr.small_cases():
        check(binding(gpu_ctx, src, m, shape, mode, fill), wr.warp(src, m, shape, mode, fill), name)
        n += 1
    assert n > 200


# ---- tile edges, strides, device forms ------------------------------------------------------
EDGE_MAPS = {
    "rot_persp": wr.rotation(5.0, 33.0, 17.0, 1e-3, -2e-3),
    "shift_half": wr.shift(0.5, 0.5),
}


@pytest.mark.parametrize("kind", ["gray", "rgba"])
@pytest.mark.parametrize("oh", [1, TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1])
def test_tile_edges_with_padded_rows(gpu_ctx, kind, oh):
    """Destination widths and heights at and either side of the 64 x 16 tile,
    source and destination rows longer than the images; the destination's
    padding keeps its sentinel; host and device forms give the same bytes."""
    src = wr.gray_image(35, 67, 5) if kind == "gray" else wr.rgba_image(35, 67, 5)
    fill = np.float32(3.25) if kind == "gray" else (5, 6, 7, 8)
    for ow in (63, 64, 65, 127, 129):
        for name, m in EDGE_MAPS.items():
            for mode in (wr.BILINEAR, wr.NEAREST):
                want = wr.warp(src, m, (oh, ow), mode, fill)
                what = (kind, oh, ow, name, mode)
                check(run_host(gpu_ctx, src, m, (oh, ow), mode, fill, spad=3, dpad=5), want, what)
                check(run_device(gpu_ctx, src, m, (oh, ow), mode, fill, spad=3, dpad=5), want, what)


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_scale_that_ends_on_the_last_pixel(gpu_ctx, kind):
    """0.5x: destination column 132 sits at sx == 66 == sw-1 and row 68 at
    sy == sh-1, so fx = fy = 1 on the clamped x0, y0; column 133 is invalid."""
    src = wr.gray_image(35, 67, 6) if kind == "gray" else wr.rgba_image(35, 67, 6)
    want = wr.warp(src, wr.scale(0.5), (70, 134), wr.BILINEAR, 0)
    assert want[1][68, 132] == 1 and want[1][68, 133] == 0 and want[1][69, 132] == 0
    last = src[34, 66]
    assert want[0][68, 132].tobytes() == last.tobytes()
    check(run_device(gpu_ctx, src, wr.scale(0.5), (70, 134), wr.BILINEAR, 0, dpad=2), want, kind)


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_identity_and_integer_shift_copy_exactly(gpu_ctx, kind):
    h, w = 150, 200
    src = wr.gray_image(h, w, 7) if kind == "gray" else wr.rgba_image(h, w, 7)
    dst, mask, n, _ = binding(gpu_ctx, src, np.eye(3), (h, w), wr.BILINEAR, 0)
    assert same_bytes(dst, src) and mask.all() and n == h * w
    m = sift_amd.homography_inverse([[1, 0, 16], [0, 1, 8], [0, 0, 1]])
    dst, mask, n, _ = binding(gpu_ctx, src, m, (h, w), wr.BILINEAR, 0)
    assert same_bytes(np.ascontiguousarray(dst[8:, 16:]), np.ascontiguousarray(src[:-8, :-16]))
    assert n == (h - 8) * (w - 16)
    check((dst, mask, n, True), wr.warp(src, m, (h, w)), kind)


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_many_tiles_with_a_horizon(gpu_ctx, kind):
    """1024 x 768 into 1030 x 770 with w = 0 crossing the destination: over 40 %
    of the pixels have w <= 0 and read nothing."""
    src = wr.gray_image(768, 1024, 8) if kind == "gray" else wr.rgba_image(768, 1024, 8)
    want = wr.warp(src, wr.HORIZON, (770, 1030), wr.BILINEAR, 1)
    assert 0.25 < want[2] / (770 * 1030) < 0.4
    check(run_device(gpu_ctx, src, wr.HORIZON, (770, 1030), wr.BILINEAR, 1), want, kind)
    check(binding(gpu_ctx, src, wr.HORIZON, (770, 1030), wr.BILINEAR, 1), want, kind)


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_more_tiles_than_blocks(gpu_ctx, kind):
    """A destination one pixel wide and 70 001 rows tall is 4 376 tiles: more than
    the 4 096 blocks of a launch, so blocks take a second tile, and the count is
    the sum of 4 096 per-block words."""
    src = wr.gray_image(35, 67, 15) if kind == "gray" else wr.rgba_image(35, 67, 15)
    m = [0, 0, 3.3, 0, 0.0005, 0, 0, 0, 1]
    want = wr.warp(src, m, (70001, 1), wr.BILINEAR, 4)
    assert want[2] == 68001 and want[1][-1, 0] == 0
    check(run_device(gpu_ctx, src, m, (70001, 1), wr.BILINEAR, 4, dpad=1), want, kind)


def test_mirroring_matrix_through_the_library_inverse(gpu_ctx):
    m = sift_amd.homography_inverse(wr.MIRROR)
    assert np.linalg.det(wr.MIRROR) < 0 and same_bytes(m, wr.inverse(wr.MIRROR))
    src = wr.gray_image(35, 67, 9)
    want = wr.warp(src, m, (40, 70))
    assert 0 < want[2] < 40 * 70
    check(binding(gpu_ctx, src, m, (40, 70), wr.BILINEAR, 0.0), want, "mirror")


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_matrices_that_are_not_homographies(gpu_ctx, kind):
    """All NaN: no pixel is valid.  1e300 with m8 = 1e-300: pixel (0, 0) overflows
    and is invalid, the others land between source pixels 1 and 2; a cast to an
    integer before the validity test would index outside the source here."""
    src = wr.gray_image(35, 67, 10) if kind == "gray" else wr.rgba_image(35, 67, 10)
    fill = np.float32(9.0) if kind == "gray" else (9, 9, 9, 9)
    for mode in (wr.BILINEAR, wr.NEAREST):
        dst, mask, n, pad = run_device(gpu_ctx, src, np.full(9, np.nan), (70, 130), mode, fill, dpad=1)
        assert n == 0 and not mask.any() and (dst == 9).all() and pad
        want = wr.warp(src, wr.huge_matrix(), (70, 130), mode, fill)
        assert want[1][0, 0] == 0 and want[2] == 70 * 130 - 1
        check(run_device(gpu_ctx, src, wr.huge_matrix(), (70, 130), mode, fill), want, (kind, mode))
        for bad in (np.full(9, np.inf), np.full(9, -1e308), [1e308, 1e308, 1e308, 0, 1, 0, 0, 0, 1e-308],
                    [1e-308, 0, 0, 0, 1e-308, 0, 0, 0, 1e-308]):   # subnormal entries: near the identity
            check(run_device(gpu_ctx, src, bad, (17, 65), mode, fill), wr.warp(src, bad, (17, 65), mode, fill), kind)


def test_fill_keeps_its_bits(gpu_ctx):
    src = wr.gray_image(5, 6, 11)
    for bits in (0x7fc12345, 0xffc00001, 0x80000000):
        fill = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        want = wr.warp(src, wr.shift(-2.0, -1.0), (7, 9), wr.BILINEAR, fill)
        assert (want[0].view(np.uint32)[want[1] == 0] == bits).all() and 0 < want[2] < 63
        check(binding(gpu_ctx, src, wr.shift(-2.0, -1.0), (7, 9), wr.BILINEAR, fill), want, hex(bits))
        check(run_device(gpu_ctx, src, wr.shift(-2.0, -1.0), (7, 9), wr.NEAREST, fill),
              wr.warp(src, wr.shift(-2.0, -1.0), (7, 9), wr.NEAREST, fill), hex(bits))
    zeros = np.array([[-0.0, 1.0], [2.0, 3.0]], dtype=np.float32)
    dst = binding(gpu_ctx, zeros, np.eye(3), (2, 2), wr.BILINEAR, 0.0)[0]
    assert dst[0, 0].tobytes() == np.float32(0.0).tobytes()       # -0.0 * 1 + 1 * 0 is +0.0
    dst = binding(gpu_ctx, zeros, np.eye(3), (2, 2), wr.NEAREST, 0.0)[0]
    assert same_bytes(dst, zeros)                                    # nearest copies


def test_rgba_rounding_fill_and_stride(gpu_ctx):
    for v in (0, 255):                                               # the rounding ends
        src = np.full((5, 6, 4), v, dtype=np.uint8)
        dst, _, n, _ = run_host(gpu_ctx, src, wr.shift(0.3, 0.7), (4, 5), spad=2, dpad=1)
        assert n == 20 and (dst == v).all()
    cb = wr.checkerboard(20, 70)
    want = wr.warp(cb, wr.shift(0.5, 0.0), (20, 70), wr.BILINEAR, (1, 2, 3, 4))
    assert (want[0][:, :69, 1] == 128).all() and (want[0][:, 69] == (1, 2, 3, 4)).all()   # x.5 goes up; the fill
    check(run_host(gpu_ctx, cb, wr.shift(0.5, 0.0), (20, 70), wr.BILINEAR, (1, 2, 3, 4), spad=7, dpad=3), want, "cb")
    check(run_device(gpu_ctx, cb, wr.shift(0.5, 0.0), (20, 70), wr.BILINEAR, (1, 2, 3, 4), spad=7, dpad=3), want, "cb")
    want = wr.warp(cb, wr.shift(0.5, 0.5), (19, 69))
    check(binding(gpu_ctx, cb, wr.shift(0.5, 0.5), (19, 69), wr.BILINEAR, (0, 0, 0, 0)), want, "cb both ways")


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_nearest_at_the_half(gpu_ctx, kind):
    """sx = k + 0.5 exactly goes up."""
    src = wr.gray_image(20, 70, 12) if kind == "gray" else wr.rgba_image(20, 70, 12)
    dst, mask, n, _ = binding(gpu_ctx, src, wr.shift(0.5, 0.5), (19, 69), wr.NEAREST, 0)
    assert same_bytes(dst, np.ascontiguousarray(src[1:, 1:])) and n == 19 * 69
    check((dst, mask, n, True), wr.warp(src, wr.shift(0.5, 0.5), (19, 69), wr.NEAREST, 0), kind)


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_optional_outputs_and_repeat(gpu_ctx, kind):
    """mask == NULL and n_valid == NULL are accepted and change nothing else;
    two runs are bytewise identical."""
    src = wr.gray_image(35, 67, 13) if kind == "gray" else wr.rgba_image(35, 67, 13)
    m = EDGE_MAPS["rot_persp"]
    want = wr.warp(src, m, (70, 130), wr.BILINEAR, 2)
    for run in (run_host, run_device):
        for want_mask in (True, False):
            for want_count in (True, False):
                check(run(gpu_ctx, src, m, (70, 130), wr.BILINEAR, 2, 1, 1, want_mask, want_count), want, kind)
    a = run_device(gpu_ctx, src, m, (70, 130), wr.BILINEAR, 2)
    b = run_device(gpu_ctx, src, m, (70, 130), wr.BILINEAR, 2)
    assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1]) and a[2] == b[2]
    assert gpu_ctx.warp_timing() > 0


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_page_locked_host_buffers(gpu_ctx, kind):
    L = sift_amd.lib()
    sh, sw, oh, ow = 35, 67, 70, 130
    img = wr.gray_image(sh, sw, 14) if kind == "gray" else wr.rgba_image(sh, sw, 14)
    m = EDGE_MAPS["rot_persp"]
    want = wr.warp(img, m, (oh, ow), wr.BILINEAR, 2)
    bufs = [mmap.mmap(-1, sh * sw * 4), mmap.mmap(-1, oh * ow * 4), mmap.mmap(-1, oh * ow)]  # page-aligned
    src = np.frombuffer(bufs[0], dtype=img.dtype).reshape(img.shape)
    dst = np.frombuffer(bufs[1], dtype=img.dtype).reshape((oh, ow) + img.shape[2:])
    mask = np.frombuffer(bufs[2], dtype=np.uint8).reshape(oh, ow)
    src[:] = img
    ptrs = [src.ctypes.data, dst.ctypes.data, mask.ctypes.data]
    for q, b in zip(ptrs, bufs):
        assert L.sift_host_register(ctypes.c_void_p(q), len(b)) == 0
    try:
        n = ctypes.c_size_t()
        f, keep = fill_arg(img, 2)
        per = 4 if kind == "rgba" else 1
        fn = L.sift_warp_rgba if kind == "rgba" else L.sift_warp_gray
        mm = np.ascontiguousarray(m, dtype=np.float64).reshape(9)
        rc = fn(gpu_ctx._h, ctypes.c_void_p(ptrs[0]), sw, sh, sw * per, mm.ctypes.data_as(DP), wr.BILINEAR, f,
                ctypes.c_void_p(ptrs[1]), ow, oh, ow * per, ctypes.c_void_p(ptrs[2]), ctypes.byref(n))
        assert rc == 0
        check((dst.copy(), mask.copy(), n.value, True), want, kind)
    finally:
        for q in ptrs:
            L.sift_host_unregister(ctypes.c_void_p(q))
        del src, dst, mask


# ---- rejected calls ----------------------------------------------------------------------------
def test_bad_arguments_write_nothing(gpu_ctx):
    import torch
    L, h = sift_amd.lib(), gpu_ctx._h
    sw, sh, ow, oh = 8, 6, 9, 7
    m = np.eye(3).reshape(9)
    mp = m.ctypes.data_as(DP)
    fill4 = np.zeros(4, dtype=np.uint8)
    f4 = fill4.ctypes.data_as(ctypes.c_void_p)
    big = 1 << 16                                                    # big * (big / 2) == 2^31

    def gray_calls(src, dst):
        """(why, arguments) with every argument good but one."""
        good = [h, src, sw, sh, sw, mp, wr.BILINEAR, ctypes.c_float(1.0), dst, ow, oh, ow, None, None]

        def but(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return a
        return [("ctx", but(_0=None)), ("src", but(_1=None)), ("dst", but(_8=None)), ("m", but(_5=None)),
                ("src_w", but(_2=0)), ("src_h", but(_3=-1)), ("dst_w", but(_9=0)), ("dst_h", but(_10=-3)),
                ("src stride", but(_4=sw - 1)), ("dst stride", but(_11=ow - 1)),
                ("src 2^31", but(_2=big, _3=big // 2, _4=big)), ("dst 2^31", but(_9=big, _10=big // 2, _11=big)),
                ("mode", but(_6=2)), ("mode", but(_6=-1)), ("dst == src", but(_8=src))]

    def rgba_calls(src, dst):
        good = [h, src, sw, sh, sw * 4, mp, wr.BILINEAR, f4, dst, ow, oh, ow * 4, None, None]

        def but(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return a
        return [("ctx", but(_0=None)), ("src", but(_1=None)), ("dst", but(_8=None)), ("m", but(_5=None)),
                ("fill", but(_7=None)),
                ("src_w", but(_2=0)), ("src_h", but(_3=-1)), ("dst_w", but(_9=0)), ("dst_h", but(_10=-3)),
                ("src stride", but(_4=sw * 4 - 4)), ("dst stride", but(_11=ow * 4 - 4)),
                ("src stride % 4", but(_4=sw * 4 + 2)), ("dst stride % 4", but(_11=ow * 4 + 1)),
                ("src 2^31", but(_2=big, _3=big // 2, _4=big * 4)),
                ("dst 2^31", but(_9=big, _10=big // 2, _11=big * 4)),
                ("mode", but(_6=2)), ("dst == src", but(_8=src))]

    # host forms: numpy buffers, big enough for the largest good geometry
    src_g, dst_g = np.ones((sh, sw), dtype=np.float32), np.full((oh, ow), 7.0, dtype=np.float32)
    for why, a in gray_calls(src_g.ctypes.data, dst_g.ctypes.data):
        assert L.sift_warp_gray(*a) == E_ARG, why
    assert (dst_g == 7.0).all()
    src_r, dst_r = np.ones((sh, sw, 4), dtype=np.uint8), np.full((oh, ow, 4), SENTINEL, dtype=np.uint8)
    for why, a in rgba_calls(src_r.ctypes.data, dst_r.ctypes.data):
        assert L.sift_warp_rgba(*a) == E_ARG, why
    assert (dst_r == SENTINEL).all()
    # device forms
    d_src = torch.ones((sh, sw), dtype=torch.float32, device="cuda")
    d_dst = torch.full((oh, ow), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for why, a in gray_calls(d_src.data_ptr(), d_dst.data_ptr()):
        assert L.sift_warp_gray_device(*a) == E_ARG, why
    assert bool((d_dst == 7.0).all())
    d_src = torch.ones((sh, sw, 4), dtype=torch.uint8, device="cuda")
    d_dst = torch.full((oh, ow, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for why, a in rgba_calls(d_src.data_ptr(), d_dst.data_ptr()) + \
            [("alignment", [h, d_src.data_ptr() + 1, sw - 1, sh, sw * 4, mp, wr.BILINEAR, f4, d_dst.data_ptr(), ow, oh,
                            ow * 4, None, None])]:
        assert L.sift_warp_rgba_device(*a) == E_ARG, why
    assert bool((d_dst == SENTINEL).all())
    assert L.sift_last_warp_timing(None, None) == E_ARG
    # the context still works
    check(binding(gpu_ctx, src_g, np.eye(3), (oh, ow), wr.BILINEAR, 0.0), wr.warp(src_g, np.eye(3), (oh, ow)), "after")


# ---- end to end ----------------------------------------------------------------------------------
def test_end_to_end_alignment(gpu_ctx, capsys):
    """The two crops of test_gpu_verify.py::test_end_to_end through the whole
    chain: detect, describe, match, verify with refit, invert, warp the query
    into the train frame.  b[Y, X] = a[Y + 16, X + 8], so the overlap is 248
    columns by 240 rows at the destination's top left.

    The count's bounds: a model that is within `thresh` = 3 pixels of the true
    shift at every point (asserted at the corners below, as test_end_to_end
    does) moves each of the two borders that cross the destination by at most 3
    pixels, so the valid region holds the (248 - 3) x (240 - 3) rectangle and
    lies inside the (248 + 3) x (240 + 3) one."""
    p = sift_amd.make_params(3, 4)
    big = blob_image(288, 288, seed=1)
    a, b = np.ascontiguousarray(big[:256, :256]), np.ascontiguousarray(big[16:272, 8:264])
    K, seed, thresh = 512, 9, 3.0
    with sift_amd.Context(0) as other:
        for ctx, img in ((gpu_ctx, a), (other, b)):
            ctx.detect(img, p)
            ctx.orient()
            ctx.describe()
        pairs = gpu_ctx.select_matches(gpu_ctx.match_features(other), other.match_features(gpu_ctx), 0.8)
        H, best, rounds, inl = gpu_ctx.verify_features_refit(other, pairs, K, seed, thresh)
    assert best >= 0 and len(inl) > len(pairs) / 2
    for x, y in ((0.0, 0.0), (255.0, 0.0), (0.0, 255.0), (255.0, 255.0)):
        u, v, w = H @ np.array([x, y, 1.0])
        assert np.hypot(u / w - (x - 8.0), v / w - (y - 16.0)) < thresh
    m = sift_amd.homography_inverse(H)
    assert m is not None and same_bytes(m, wr.inverse(H))
    dst, mask, n = gpu_ctx.warp_gray(a, m, b.shape)
    check((dst, mask, n, True), wr.warp(a, m, b.shape), "end to end")
    assert (248 - 3) * (240 - 3) <= n <= (248 + 3) * (240 + 3)
    ok = mask == 1
    aligned = float(np.abs(dst.astype(np.float64) - b)[ok].mean())
    unaligned = float(np.abs(a.astype(np.float64) - b)[ok].mean())
    with capsys.disabled():
        print("\nend to end: n_valid = %d, mean |warped - b| = %.6g, mean |a - b| = %.6g over the valid pixels"
              % (n, aligned, unaligned))
    assert aligned < unaligned
