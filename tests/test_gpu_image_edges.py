"""The image products at every edge of their kernels (GPU).

k_rgba_to_gray: the whole (R, G, B) cube with every alpha, through the device
and the host entry point, equal to image_cases.cube_expected bit for bit; the
device form on torch device memory over widths 1..65, heights that keep the
launch in one block and that cross it, row strides from dense to two 16-byte
steps of padding (the padding holds 0xFF), and the RGBA, gray and alpha bases
at byte offsets 0, 4, 8, 12 independently (every choice between the 16-byte
and the scalar path, gray aligned with alpha not among them), alpha NULL;
every destination inside a sentinel-filled buffer whose other bytes must
stay.  Host images with padded rows through sift_rgba_to_gray,
sift_build_scale_space_rgba and sift_detect_rgba.

k_minmax_partial / k_plane_image: caller planes (sift_load_dog,
sift_load_scale_space) of the tables of image_cases.py -- the plain specials,
the sigmoid table at every coefficient, the ramps whose sampled values are
ties, the fixture's planes around the scan's start values +-(2^53 - 1) (the
sampled mode of these is what a scan started at +-inf gets wrong), and a
unique minimum and maximum at every edge of the reduction for plane sizes
either side of each of its steps, up to the cap of 1024 partials -- against
the reference's bytes (tests/golden/image_products.npz) and the numpy
restatement; planes that are not 16-byte aligned (odd sizes, scale >= 1);
sift_plane_image_device into a sentinel-filled buffer at byte offsets 0, 4,
8, 12, its capacity at 4n and 4n - 4; the smallest plane after the largest
on one context.  test_image_cases.py (CPU) proves what the tables hold and
that each can fail.  Every comparison is array equality.
"""
import ctypes

import numpy as np
import pytest

import image_cases as ic
import image_products as ip
import sift_amd

pytestmark = pytest.mark.gpu

SENT = 0xA5
VP = ctypes.c_void_p
FP = ctypes.POINTER(ctypes.c_float)


def _torch():
    import torch
    return torch


def _ok(ctx, rc, what):
    assert rc == sift_amd.SIFT_OK, (what, rc, sift_amd.lib().sift_last_error(ctx._h).decode())


# ---------------------------------------------------------------------------
# k_rgba_to_gray
# ---------------------------------------------------------------------------
def test_gray_cube_device_and_host(gpu_ctx):
    """All 2^24 (R, G, B), every alpha: the device form on device memory, then
    the host form (one upload, k_rgba_to_gray on the context's dense copy)."""
    torch = _torch()
    rgba = ic.cube_rgba()
    gray, alpha = ic.cube_expected()
    n = ic.CUBE_SIDE
    d_src = torch.from_numpy(rgba.copy()).cuda()   # the table is read-only, which torch warns about
    d_g = torch.full((n, n), -7.0, dtype=torch.float32, device="cuda")
    d_a = torch.full((n, n), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _ok(gpu_ctx, sift_amd.lib().sift_rgba_to_gray_device(gpu_ctx._h, d_src.data_ptr(), n, n, 4 * n, d_g.data_ptr(),
                                                        d_a.data_ptr()), "device")
    assert np.array_equal(d_g.cpu().numpy(), gray) and np.array_equal(d_a.cpu().numpy(), alpha)
    del d_src, d_g, d_a
    g, a = gpu_ctx.rgba_to_gray(rgba, alpha=True)
    assert np.array_equal(g, gray) and np.array_equal(a, alpha)


GRAY_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 64, 65)
GRAY_HEIGHTS = (1, 2, 129)     # 5 x 129: 2 quads a row, 258 lanes, the second block
OFFSETS = (0, 4, 8, 12)
# (RGBA, gray, alpha) base offsets: every triple, then every pair with alpha NULL
GRAY_BASES = [(r, g, a) for r in OFFSETS for g in OFFSETS for a in OFFSETS] + \
             [(r, g, None) for r in OFFSETS for g in OFFSETS]


def _strides(W):
    up = (4 * W + 15) // 16 * 16
    return (4 * W, 4 * W + 4, 4 * W + 8, 4 * W + 12, up, up + 16)


def _gray_launch(ctx, rgba, stride, off_r, off_g, off_a):
    """One sift_rgba_to_gray_device call on rows `stride` bytes apart from byte
    off_r of a 0xFF-filled source, gray / alpha at bytes off_g / off_a of
    sentinel-filled buffers: (gray, alpha or None), the sentinels checked."""
    torch = _torch()
    H, W = rgba.shape[:2]
    src = np.full(off_r + H * stride + 16, 0xFF, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(src[off_r:], shape=(H, W * 4), strides=(stride, 1))
    rows[:] = rgba.reshape(H, W * 4)
    d_src = torch.from_numpy(src).cuda()
    nb = 4 * W * H
    d_g = torch.full((nb + 32,), SENT, dtype=torch.uint8, device="cuda")
    d_a = torch.full((nb + 32,), SENT, dtype=torch.uint8, device="cuda") if off_a is not None else None
    torch.cuda.synchronize()
    rc = sift_amd.lib().sift_rgba_to_gray_device(ctx._h, d_src.data_ptr() + off_r, W, H, stride, d_g.data_ptr() + off_g,
                                                 d_a.data_ptr() + off_a if d_a is not None else None)
    _ok(ctx, rc, (W, H, stride, off_r, off_g, off_a))
    out = []
    for d, off in ((d_g, off_g), (d_a, off_a)):
        if d is None:
            out.append(None)
            continue
        b = d.cpu().numpy()
        assert (b[:off] == SENT).all() and (b[off + nb:] == SENT).all(), (W, H, stride, off_r, off_g, off_a)
        out.append(b[off:off + nb].copy().view(np.float32).reshape(H, W))
    return out


@pytest.mark.parametrize("H", GRAY_HEIGHTS)
def test_gray_device_geometry(gpu_ctx, H):
    """Widths x strides of this height, the base offsets taken in turn so
    that the three heights go through every (RGBA, gray, alpha) triple and
    every pair with alpha NULL at least twice (180 launches, 80 choices)."""
    t = GRAY_HEIGHTS.index(H) * len(GRAY_WIDTHS) * 6
    assert len(GRAY_HEIGHTS) * len(GRAY_WIDTHS) * 6 >= 2 * len(GRAY_BASES)
    for W in GRAY_WIDTHS:
        rgba = np.random.default_rng(1000 * W + H).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        rg, ra = (x.astype(np.float32) for x in ip.rgba_to_gray(rgba))
        for stride in _strides(W):
            off_r, off_g, off_a = GRAY_BASES[t % len(GRAY_BASES)]
            t += 1
            g, a = _gray_launch(gpu_ctx, rgba, stride, off_r, off_g, off_a)
            what = (W, H, stride, off_r, off_g, off_a)
            assert g.tobytes() == rg.tobytes(), what
            assert a is None or a.tobytes() == ra.tobytes(), what


def test_gray_aligned_alpha_unaligned(gpu_ctx):
    """The branch of the 16-byte path that stores alpha by elements: RGBA rows
    and gray 16-byte aligned, alpha at 4, 8 and 12; and its mirror (gray off
    16 bytes sends the whole quad down the scalar path)."""
    rgba = np.random.default_rng(3).integers(0, 256, size=(5, 8, 4), dtype=np.uint8)
    rg, ra = (x.astype(np.float32) for x in ip.rgba_to_gray(rgba))
    for off_g, off_a in ((0, 4), (0, 8), (0, 12), (4, 0), (12, 0)):
        g, a = _gray_launch(gpu_ctx, rgba, 32, 0, off_g, off_a)
        assert g.tobytes() == rg.tobytes() and a.tobytes() == ra.tobytes(), (off_g, off_a)


def test_host_rgba_with_padded_rows(gpu_ctx):
    """Rows cut out of a wider host image (hipMemcpy2DAsync into the dense
    copy): gray, alpha, planes and keypoints equal those of the dense copy."""
    L = sift_amd.lib()
    H, W, WF = 120, 161, 200
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:WF]
    base = 128 + 90 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rng.integers(-20, 21, size=(H, WF))
    wide = np.full((H, WF, 4), 0xFF, dtype=np.uint8)
    for c, k in enumerate((1.0, 0.8, 1.2)):
        wide[:, 17:17 + W, c] = np.clip(base[:, 17:17 + W] * k, 0, 255).astype(np.uint8)
    wide[:, 17:17 + W, 3] = rng.integers(0, 256, size=(H, W))
    view = wide[:, 17:17 + W]
    dense = np.ascontiguousarray(view)
    assert not view.flags["C_CONTIGUOUS"] and view.strides[0] == 4 * WF
    ptr = VP(view.ctypes.data)
    rg, ra = (x.astype(np.float32) for x in ip.rgba_to_gray(dense))

    g = np.full((H, W), -7, dtype=np.float32)
    a = np.full((H, W), -7, dtype=np.float32)
    _ok(gpu_ctx, L.sift_rgba_to_gray(gpu_ctx._h, ptr, W, H, 4 * WF, g.ctypes.data_as(FP), a.ctypes.data_as(FP)), "gray")
    assert g.tobytes() == rg.tobytes() and a.tobytes() == ra.tobytes()
    g2 = np.full((H, W), -7, dtype=np.float32)
    _ok(gpu_ctx, L.sift_rgba_to_gray(gpu_ctx._h, ptr, W, H, 4 * WF, g2.ctypes.data_as(FP), None), "gray, no alpha")
    assert g2.tobytes() == rg.tobytes()

    p = sift_amd.make_params(3, 3)
    _ok(gpu_ctx, L.sift_build_scale_space_rgba(gpu_ctx._h, ptr, W, H, 4 * WF, ctypes.byref(p), None), "build")
    got = [gpu_ctx.plane(k, o, s).copy() for k, o, s in ((sift_amd.PLANE_GAUSS, 0, 0), (sift_amd.PLANE_DOG, 1, 2),
                                                         (sift_amd.PLANE_GAUSS, 2, 5))]
    gpu_ctx.build_scale_space_rgba(dense, p)
    for x, (k, o, s) in zip(got, ((sift_amd.PLANE_GAUSS, 0, 0), (sift_amd.PLANE_DOG, 1, 2), (sift_amd.PLANE_GAUSS, 2, 5))):
        assert x.tobytes() == gpu_ctx.plane(k, o, s).tobytes(), (k, o, s)

    n = ctypes.c_size_t()
    rc = L.sift_detect_rgba(gpu_ctx._h, ptr, W, H, 4 * WF, ctypes.byref(p), None, 0, ctypes.byref(n))
    assert rc in (sift_amd.SIFT_OK, sift_amd.SIFT_E_SINGULAR), rc
    k1 = gpu_ctx.keypoints().copy()
    k2 = gpu_ctx.detect_rgba(dense, p)
    assert k1.shape[0] == n.value == k2.shape[0] > 0 and k1.tobytes() == k2.tobytes()
    assert k1.tobytes() == gpu_ctx.detect(rg, p).tobytes()


# ---------------------------------------------------------------------------
# k_minmax_partial, k_plane_image
# ---------------------------------------------------------------------------
def _load(ctx, geom, planes):
    """planes as the DoG planes of geom's octave (sift_load_dog); the plane
    size read back."""
    flat, O, S = ic.pyramid_flat(geom, planes)
    ctx.load_dog(flat, geom[0], geom[1], sift_amd.make_params(O, S))
    assert ctx.dims(geom[2]) == ic.plane_dims(*geom)
    return geom[2]


def _image(ctx, o, s, mode, c=1.0, kind=sift_amd.PLANE_DOG):
    return ctx.plane_image(kind, o, s, mode, c).reshape(-1, 4)


def _same(got, want, what):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), \
        (what, np.flatnonzero((got != want).any(axis=1))[:8], got[(got != want).any(axis=1)][:4])


def test_specials_and_sigmoid_table(gpu_ctx):
    """The plain specials followed by the random plane (3600 values): plain
    against exact arithmetic, sigmoid at all seven coefficients and sampled
    against the reference's bytes; DoG planes at scale 0 (aligned) and, one
    element shorter, at scale 1 of an odd-sized octave (not aligned)."""
    g = ic.gold()
    v = ic.sigmoid_input()
    o = _load(gpu_ctx, ic.geom_for(v.size), [v])
    _same(_image(gpu_ctx, o, 0, 0)[:ic.plain_specials().size], ic.as_image(ic.exact_plain_bytes(ic.plain_specials())),
          "plain, exact")
    _same(_image(gpu_ctx, o, 0, 0), g["s_plain"].reshape(-1, 4), "plain")
    _same(_image(gpu_ctx, o, 0, 2), g["s_sampled"].reshape(-1, 4), "sampled")
    for j, c in enumerate(ic.SIGMOID_COEFS):
        _same(_image(gpu_ctx, o, 0, 1, c), g["s_sigmoid_%d" % j].reshape(-1, 4), ("sigmoid", c))
    u = v[:-1]                          # 3599 floats a plane: scale 1 starts 12 bytes past a 16-byte boundary
    o = _load(gpu_ctx, ic.geom_for(u.size), [u[::-1], u])
    _same(_image(gpu_ctx, o, 1, 0), g["s_plain"].reshape(-1, 4)[:-1], "plain, unaligned")
    for j, c in enumerate(ic.SIGMOID_COEFS):
        _same(_image(gpu_ctx, o, 1, 1, c), g["s_sigmoid_%d" % j].reshape(-1, 4)[:-1], ("sigmoid, unaligned", c))
    _same(_image(gpu_ctx, o, 1, 2), ip.plane_image(u.reshape(1, -1), 2).reshape(-1, 4), "sampled, unaligned")


def test_specials_as_gaussian_planes(gpu_ctx):
    """The same through sift_load_scale_space and the Gaussian kind."""
    g = ic.gold()
    v = ic.sigmoid_input()
    W, H, o = ic.geom_for(v.size)
    S = 1
    flat = np.concatenate([np.zeros((S + 3) * 4 * v.size, np.float32)] + [v, v[::-1], v, v])
    gpu_ctx.load_scale_space(flat, W, H, sift_amd.make_params(2, S))
    assert gpu_ctx.dims(o) == (1, v.size)
    for s in (0, 2):
        _same(_image(gpu_ctx, o, s, 0, kind=sift_amd.PLANE_GAUSS), g["s_plain"].reshape(-1, 4), "plain")
        _same(_image(gpu_ctx, o, s, 2, kind=sift_amd.PLANE_GAUSS), g["s_sampled"].reshape(-1, 4), "sampled")
        _same(_image(gpu_ctx, o, s, 1, 5.0, kind=sift_amd.PLANE_GAUSS), g["s_sigmoid_0"].reshape(-1, 4), "sigmoid")


def _by_size(names):
    out = {}
    for name in names:
        out.setdefault(ic.fixture_plane(name)[0].size, []).append(name)
    return sorted(out.items())


@pytest.mark.parametrize("n,names", _by_size(ic.EXTREMES + ic.RAMPS), ids=["n%d" % k for k, _ in _by_size(ic.EXTREMES + ic.RAMPS)])
def test_extreme_planes_and_ramps(gpu_ctx, n, names):
    """The fixture's planes, all three modes, against the reference's bytes.
    The sampled mode of the planes that keep a start value of the reference's
    scan (image_cases.EXTREMES_INF_START_WRONG) is what a scan started at
    +-inf gets wrong; the ramps put 255 values on ties (an odd-sized octave:
    every plane but the first is off 16-byte alignment)."""
    c = float(ic.gold()["coef"])
    o = _load(gpu_ctx, ic.geom_for(n), [ic.fixture_plane(name)[0] for name in names])
    for s, name in enumerate(names):
        forms = ic.fixture_plane(name)[1]
        for mode, form in ((2, "sampled"), (0, "plain"), (1, "sigmoid")):
            _same(_image(gpu_ctx, o, s, mode, c), forms[form], (name, form))


SMALL_GEOMS = [g for g in ic.POSITION_GEOMS if np.prod(ic.plane_dims(*g)) < 100000]


@pytest.mark.parametrize("geom", SMALL_GEOMS, ids=["%dx%dO%d" % g for g in SMALL_GEOMS])
def test_minmax_positions(gpu_ctx, geom):
    """The unique minimum and maximum at each edge of the reduction in turn,
    one plane each (so the planes of an odd size start at every alignment)."""
    n = int(np.prod(ic.plane_dims(*geom)))
    planes = ic.position_planes(n)
    o = _load(gpu_ctx, geom, [p[2] for p in planes])
    for s, (imin, imax, v) in enumerate(planes):
        _same(_image(gpu_ctx, o, s, 2), ip.plane_image(v.reshape(1, -1), 2).reshape(-1, 4), (n, imin, imax))
        _same(_image(gpu_ctx, o, s, 0), ip.plane_image(v.reshape(1, -1), 0).reshape(-1, 4), (n, "plain"))


def test_capped_partials_then_the_smallest_plane():
    """4096 x 2050 pixels: 1024 partials of 2050 float4 each (the cap; uncapped
    it would be 1025), the minimum and maximum at the plane's ends and at the
    ends of the last partial's first stride.  Then, on the same context, one
    pixel, five pixels and a ramp: the partial and display buffers are reused."""
    geom = ic.POSITION_GEOMS[-1]
    n = int(np.prod(ic.plane_dims(*geom)))
    assert n == ic.POSITION_SIZES[-1] > 8388608 and ic.minmax_parts(n) == 1024
    planes = ic.position_planes(n)
    with sift_amd.Context(0) as ctx:
        o = _load(ctx, geom, [p[2] for p in planes])
        for s, (imin, imax, v) in enumerate(planes):
            _same(_image(ctx, o, s, 2), ip.plane_image(v.reshape(1, -1), 2).reshape(-1, 4), (n, imin, imax))
        for m in (1, 5):
            small = ic.position_planes(m)
            o = _load(ctx, ic.geom_for(m), [p[2] for p in small])
            for s, (imin, imax, v) in enumerate(small):
                _same(_image(ctx, o, s, 2), ip.plane_image(v.reshape(1, -1), 2).reshape(-1, 4), (m, imin, imax))
        v, forms = ic.fixture_plane("ramp")
        o = _load(ctx, ic.geom_for(v.size), [v])
        _same(_image(ctx, o, 0, 2), forms["sampled"], "ramp")


def _device_image(ctx, o, s, mode, c, n, off, cap=None):
    """sift_plane_image_device at byte `off` of a sentinel-filled device
    buffer: (return code, the 4n bytes, whether every other byte kept the sentinel)."""
    torch = _torch()
    d = torch.full((4 * n + 32,), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = sift_amd.lib().sift_plane_image_device(ctx._h, sift_amd.PLANE_DOG, o, s, mode, float(c), d.data_ptr() + off,
                                                4 * n if cap is None else cap)
    b = d.cpu().numpy()
    return rc, b[off:off + 4 * n].reshape(-1, 4), bool((b[:off] == SENT).all() and (b[off + 4 * n:] == SENT).all())


def _device_cases():
    v = ic.sigmoid_input()
    g = ic.gold()
    want = {0: g["s_plain"].reshape(-1, 4), 1: g["s_sigmoid_0"].reshape(-1, 4), 2: g["s_sampled"].reshape(-1, 4)}
    yield "specials", ic.geom_for(v.size), [(v, want)]
    r, forms = ic.fixture_plane("ramp")
    rs, forms_s = ic.fixture_plane("ramp_shift")
    yield "ramp", ic.geom_for(r.size), [(x, {0: f["plain"], 1: f["sigmoid"], 2: f["sampled"]})
                                        for x, f in ((r, forms), (rs, forms_s))]
    for n in (5, 1025, 8193):
        geom = ic.POSITION_GEOMS[ic.POSITION_SIZES.index(n)]
        yield "positions-%d" % n, geom, [(p[2], {m: ip.plane_image(p[2].reshape(1, -1), m).reshape(-1, 4) for m in (0, 2)})
                                         for p in ic.position_planes(n)[:4]]


@pytest.mark.parametrize("case", ["specials", "ramp", "positions-5", "positions-1025", "positions-8193"])
def test_plane_image_device(gpu_ctx, case):
    """The device form: the destination at byte offsets 0, 4, 8, 12 of a
    sentinel-filled buffer (16-byte stores only at 0, and only from an aligned
    plane), capacity exactly 4n; 4n - 4 is refused with nothing written."""
    name, geom, planes = next(c for c in _device_cases() if c[0] == case)
    n = int(np.prod(ic.plane_dims(*geom)))
    o = _load(gpu_ctx, geom, [p[0] for p in planes])
    for s, (v, want) in enumerate(planes):
        for mode, w in sorted(want.items()):
            for off in OFFSETS:
                rc, got, kept = _device_image(gpu_ctx, o, s, mode, 5.0, n, off)
                _ok(gpu_ctx, rc, (case, s, mode, off))
                assert kept, (case, s, mode, off)
                _same(got, w, (case, s, mode, off))
        rc, got, kept = _device_image(gpu_ctx, o, s, 2, 1.0, n, 4 * (s % 4), cap=4 * n - 4)
        assert rc == sift_amd.SIFT_E_CAPACITY and kept and (got == SENT).all(), (case, s, rc)
