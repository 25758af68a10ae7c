"""CPU checks of the warp's restatement (tests/warp_ref.py): its two forms agree
on bytes, the exact-copy consequences of the definition hold, and the
library's host-only inverse equals the restated one."""
import numpy as np
import pytest

import sift_amd
import warp_ref as wr


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


MATRICES = {
    "identity": np.eye(3),
    "shift": [[1, 0, 16], [0, 1, 8], [0, 0, 1]],
    "mirror": wr.MIRROR,
    "horizon": wr.HORIZON,
    "rotation": wr.rotation(5.0, 100.0, 50.0, 1e-5, -2e-5),
    "singular": [[1, 2, 3], [2, 4, 6], [0, 1, 1]],
    "zeros": np.zeros((3, 3)),
    "nan": np.full((3, 3), np.nan),
    "inf": [[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]],
    "overflow": np.full((3, 3), 1e200) + np.eye(3) * 1e200,
    "tiny": np.eye(3) * 1e-200,
}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_library_inverse_equals_the_restated_one(name):
    H = np.array(MATRICES[name], dtype=np.float64)
    want, got = wr.inverse(H), sift_amd.homography_inverse(H)
    if want is None:
        assert got is None
    else:
        assert same_bytes(got, want)


def test_inverse_of_singular_and_none_models():
    for name in ("singular", "zeros", "nan", "inf", "tiny"):
        assert wr.inverse(MATRICES[name]) is None, name
        assert sift_amd.homography_inverse(MATRICES[name]) is None, name
    assert wr.inverse(wr.MIRROR)[2, 2] > 0 > np.linalg.det(wr.MIRROR)


def test_inverse_of_the_shift_is_exact():
    inv = sift_amd.homography_inverse(MATRICES["shift"])
    assert same_bytes(inv + 0.0, wr.shift(-16.0, -8.0))  # + 0.0: a -0.0 entry equals the +0.0 of the translation
    assert same_bytes(wr.inverse(MATRICES["shift"]), inv)


def test_inverse_twice_is_close():
    H = np.array(MATRICES["rotation"])
    back = sift_amd.homography_inverse(sift_amd.homography_inverse(H))
    assert np.abs(back - H).max() <= 1e-12 * np.abs(H).max()


def test_two_restatements_agree_on_every_small_case():
    n = 0
    for name, src, m, shape, mode, fill in wr.small_cases():
        a, b = wr.warp(src, m, shape, mode, fill), wr.warp_loop(src, m, shape, mode, fill)
        assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1]) and a[2] == b[2], name
        n += 1
    assert n > 200


def test_small_cases_reach_what_they_are_for():
    """The cases the GPU test leans on do what their names say."""
    src = wr.gray_image(35, 67, 1)
    _, mask, n = wr.warp(src, wr.scale(0.5), (70, 133))          # the last valid column sits at sx == sw - 1
    assert mask[0, 132] == 1 and mask[0, :].sum() == 133 and n == 69 * 133
    _, mask, n = wr.warp(src, wr.HORIZON, (770, 1030))
    X, Y = np.meshgrid(np.arange(1030.0), np.arange(770.0))
    assert ((wr.HORIZON[6] * X + wr.HORIZON[7] * Y) + wr.HORIZON[8] <= 0).mean() > 0.4 and n > 0
    _, mask, n = wr.warp(src, np.full(9, np.nan), (7, 9))
    assert n == 0 and not mask.any()
    _, mask, n = wr.warp(src, wr.huge_matrix(), (7, 9))
    assert mask[0, 0] == 0 and 0 < n < 63
    _, mask, n = wr.warp(src, wr.inverse(wr.MIRROR), (70, 130))
    assert 0 < n < 70 * 130


@pytest.mark.parametrize("kind", ["gray", "rgba"])
def test_identity_and_integer_shift_copy_exactly(kind):
    h, w = 768, 1024
    src = wr.gray_image(h, w, 3) if kind == "gray" else wr.rgba_image(h, w, 3)
    dst, mask, n = wr.warp(src, np.eye(3), (h, w))
    assert same_bytes(dst, src) and mask.all() and n == h * w
    m = wr.inverse([[1, 0, 16], [0, 1, 8], [0, 0, 1]])
    fill = np.float32(-1.0) if kind == "gray" else (9, 8, 7, 6)
    dst, mask, n = wr.warp(src, m, (h, w), wr.BILINEAR, fill)
    assert same_bytes(np.ascontiguousarray(dst[8:, 16:]), np.ascontiguousarray(src[:-8, :-16]))
    assert n == (h - 8) * (w - 16) and mask[8:, 16:].all() and not mask[:8].any() and not mask[:, :16].any()
    want_fill = np.float32(-1.0) if kind == "gray" else np.array([9, 8, 7, 6], dtype=np.uint8)
    assert (dst[:8] == want_fill).all() and (dst[:, :16] == want_fill).all()


def test_fill_bits_and_zero_signs():
    src = np.array([[-0.0, 1.0], [2.0, 3.0]], dtype=np.float32)
    nan = np.array([0x7fc12345], dtype=np.uint32).view(np.float32)[0]
    for f in (wr.warp, wr.warp_loop):
        dst, mask, n = f(src, np.eye(3), (3, 3), wr.BILINEAR, nan)
        assert n == 4 and dst[0, 0].tobytes() == np.float32(0.0).tobytes()    # -0.0 comes back as +0.0
        assert (dst.view(np.uint32)[mask == 0] == 0x7fc12345).all()
        dst, mask, n = f(src, np.eye(3), (3, 3), wr.NEAREST, np.float32(-0.0))
        assert dst[0, 0].tobytes() == np.float32(-0.0).tobytes()               # nearest copies the pixel unchanged
        assert (dst.view(np.uint32)[mask == 0] == 0x80000000).all()


def test_rounding_ends_and_halves():
    for v in (0, 255):
        src = np.full((5, 6, 4), v, dtype=np.uint8)
        dst, _, n = wr.warp(src, wr.shift(0.3, 0.7), (4, 5))
        assert n == 20 and (dst == v).all()
    cb = wr.checkerboard(6, 7)
    dst, mask, _ = wr.warp(cb, wr.shift(0.5, 0.0), (6, 6))
    assert mask.all()
    assert (dst[..., 0] == 11).all() and (dst[..., 1] == 128).all() and (dst[..., 2] == 255).all()  # x.5 goes up
    src = np.arange(12, dtype=np.float32).reshape(3, 4)
    dst, _, _ = wr.warp(src, wr.shift(0.5, 0.5), (2, 3), wr.NEAREST)
    assert same_bytes(dst, np.ascontiguousarray(src[1:, 1:]))   # sx = k + 0.5 goes up
