"""numpy restatement of the homography warp and of the 3 x 3 inverse
(include/sift_hip.h, "Homography warp"), in two forms: `warp` is vectorised,
`warp_loop` is a plain Python loop over np.float64 scalars.  numpy's elementwise
+ - * / on float64 round every operation and never contract, which is the
definition.  Also the small cases that both test files run."""
import numpy as np

NEAREST, BILINEAR = 0, 1
F64 = np.float64


def inverse(H):
    """float64 [3, 3], or None when H has no inverse by the definition."""
    h = [F64(x) for x in np.asarray(H, dtype=F64).reshape(9)]
    with np.errstate(all="ignore"):
        a = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
             h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
             h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
        d = (h[0] * a[0] + h[1] * a[3]) + h[2] * a[6]
        if d == 0.0 or not np.isfinite(d):
            return None
        out = np.array([x / d for x in a], dtype=F64)
    return out.reshape(3, 3) if np.isfinite(out).all() else None


def _fill_like(src, fill):
    """fill in the destination's dtype with its bits kept: float32 for a gray
    source, four bytes for an RGBA one."""
    if src.ndim == 2:
        return np.asarray(fill, dtype=np.float32).reshape(())
    return np.broadcast_to(np.asarray(fill, dtype=np.uint8), (4,)).copy()


def warp(src, m, out_shape, mode=BILINEAR, fill=0.0):
    """src: float32 (h, w) or uint8 (h, w, 4).  Returns (dst, mask uint8, n_valid)."""
    src = np.asarray(src)
    m = np.asarray(m, dtype=F64).reshape(9)
    sh, sw = src.shape[:2]
    oh, ow = out_shape
    X = np.arange(ow, dtype=F64)[None, :]
    Y = np.arange(oh, dtype=F64)[:, None]
    with np.errstate(all="ignore"):
        u = (m[0] * X + m[1] * Y) + m[2]
        v = (m[3] * X + m[4] * Y) + m[5]
        w = (m[6] * X + m[7] * Y) + m[8]
        r = 1.0 / w
        sx, sy = u * r, v * r
        valid = (w > 0) & (sx >= 0) & (sy >= 0) & (sx <= sw - 1) & (sy <= sh - 1)
    sx = np.where(valid, sx, 0.0)  # the validity test precedes every cast to an integer
    sy = np.where(valid, sy, 0.0)
    if mode == NEAREST:
        xn = np.floor(sx + 0.5).astype(np.int64)
        yn = np.floor(sy + 0.5).astype(np.int64)
        res = src[yn, xn]
    else:
        x0 = np.minimum(np.floor(sx), F64(max(sw - 2, 0)))
        y0 = np.minimum(np.floor(sy), F64(max(sh - 2, 0)))
        fx, fy = sx - x0, sy - y0
        gx, gy = 1.0 - fx, 1.0 - fy
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
        if src.ndim == 3:
            fx, fy, gx, gy = (k[..., None] for k in (fx, fy, gx, gy))
        p = src.astype(F64)
        with np.errstate(all="ignore"):
            top = p[y0, x0] * gx + p[y0, x1] * fx
            bot = p[y1, x0] * gx + p[y1, x1] * fx
            val = top * gy + bot * fy
            res = val.astype(np.float32) if src.ndim == 2 else np.floor(val + 0.5).astype(np.uint8)
    f = _fill_like(src, fill)
    if src.ndim == 2:  # through the bits: a NaN fill keeps its payload
        dst = np.where(valid, res.view(np.uint32), f.view(np.uint32)).view(np.float32)
    else:
        dst = np.where(valid[..., None], res, f)
    return np.ascontiguousarray(dst), valid.astype(np.uint8), int(valid.sum())


def warp_loop(src, m, out_shape, mode=BILINEAR, fill=0.0):
    """The same, one pixel and one operation at a time."""
    src = np.asarray(src)
    m = [F64(x) for x in np.asarray(m, dtype=F64).reshape(9)]
    sh, sw = src.shape[:2]
    oh, ow = out_shape
    f = _fill_like(src, fill)
    dst = np.empty((oh, ow) + src.shape[2:], dtype=src.dtype)
    mask = np.zeros((oh, ow), dtype=np.uint8)
    one, half = F64(1.0), F64(0.5)

    def axis(s, n):
        i0 = min(np.floor(s), F64(max(n - 2, 0)))
        fr = s - i0
        return int(i0), min(int(i0) + 1, n - 1), fr, one - fr

    def lerp(p00, p01, p10, p11, fx, gx, fy, gy):
        top = F64(p00) * gx + F64(p01) * fx
        bot = F64(p10) * gx + F64(p11) * fx
        return top * gy + bot * fy

    with np.errstate(all="ignore"):
        for iy in range(oh):
            for ix in range(ow):
                X, Y = F64(ix), F64(iy)
                u = (m[0] * X + m[1] * Y) + m[2]
                v = (m[3] * X + m[4] * Y) + m[5]
                w = (m[6] * X + m[7] * Y) + m[8]
                r = one / w
                sx, sy = u * r, v * r
                if not (w > 0 and sx >= 0 and sy >= 0 and sx <= sw - 1 and sy <= sh - 1):
                    dst[iy, ix] = f
                    continue
                mask[iy, ix] = 1
                if mode == NEAREST:
                    dst[iy, ix] = src[int(np.floor(sy + half)), int(np.floor(sx + half))]
                    continue
                x0, x1, fx, gx = axis(sx, sw)
                y0, y1, fy, gy = axis(sy, sh)
                if src.ndim == 2:
                    dst[iy, ix] = np.float32(lerp(src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1], fx, gx, fy, gy))
                else:
                    for c in range(4):
                        val = lerp(src[y0, x0, c], src[y0, x1, c], src[y1, x0, c], src[y1, x1, c], fx, gx, fy, gy)
                        dst[iy, ix, c] = int(np.floor(val + half))
    if src.ndim == 2:  # the fill's bits, which an assignment of a NaN scalar need not keep
        dst.view(np.uint32)[mask == 0] = f.view(np.uint32)
    return dst, mask, int(mask.sum())


# ---- matrices and the small cases -------------------------------------------------------
IDENTITY = np.eye(3)
HORIZON = np.array([1, .1, 3, -.05, 1, 2, -.002, .0005, 1], dtype=F64)  # w = 0 crosses a 1030 x 770 destination
MIRROR = np.array([[-1.0, 0.02, 60.0], [0.03, 1.0, -2.0], [1e-4, -2e-4, 1.0]])  # det < 0


def shift(dx, dy):
    """Destination (X, Y) reads the source at (X + dx, Y + dy)."""
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])


def scale(s):
    return np.array([[s, 0.0, 0.0], [0.0, s, 0.0], [0.0, 0.0, 1.0]])


def rotation(deg, cx, cy, px=0.0, py=0.0):
    """Rotation about (cx, cy) with the perspective row (px, py, 1)."""
    t = np.deg2rad(deg)
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [px, py, 1.0]])


def gray_image(h, w, seed):
    """Finite fp32 values without negative zeros."""
    return np.random.default_rng(seed).random((h, w), dtype=np.float32) + np.float32(0.25)


def rgba_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def checkerboard(h, w):
    """Bytes k and k + 1 alternating, so that a half-pixel shift lands on x.5."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = ((yy + xx) % 2).astype(np.uint8)
    return np.stack([base + 10, base * 255, base + 254, 255 - base * 255], axis=-1).astype(np.uint8)


def huge_matrix():
    """Entries of 1e300 with m8 = 1e-300: at (0, 0) r = 1e300 and sx = u * r
    overflows to inf (invalid); elsewhere r is near 1e-300 / (X + Y) and
    sx = sy = (X + Y + 1) / (X + Y) up to rounding, valid where the source has
    three pixels each way."""
    m = np.full(9, 1e300)
    m[8] = 1e-300
    return m


SMALL_SOURCES = ((1, 1), (5, 1), (1, 5), (2, 2), (35, 67))  # (h, w): 1x1, 1x5, 5x1, 2x2, 67x35 as w x h
SMALL_DESTS = ((2, 3), (70, 130), (7, 9))                     # (h, w): 3x2 and 130x70 among them


def small_maps(sh, sw, oh, ow):
    """name -> m for a source of sw x sh into a destination of ow x oh."""
    return {
        "identity": IDENTITY,
        "shift_int": shift(-2.0, -1.0),
        "shift_half": shift(0.5, 0.5),
        "fit": np.array([[(sw - 1) / max(ow - 1, 1), 0, 0], [0, (sh - 1) / max(oh - 1, 1), 0], [0, 0, 1.0]]),
        "half_scale": scale(0.5),
        "rot_persp": rotation(5.0, (sw - 1) / 2, (sh - 1) / 2, 1e-3, -2e-3),
        "horizon": HORIZON,
        "mirror_inv": inverse(MIRROR),
        "nan": np.full(9, np.nan),
        "huge": huge_matrix(),
    }


def small_cases():
    """(name, src, m, out_shape, mode, fill): every small source into every small
    destination through every map, gray and RGBA, bilinear; nearest for the
    maps that land between pixels."""
    for si, (sh, sw) in enumerate(SMALL_SOURCES):
        for di, (oh, ow) in enumerate(SMALL_DESTS):
            for name, m in small_maps(sh, sw, oh, ow).items():
                modes = (BILINEAR, NEAREST) if name in ("shift_half", "fit", "rot_persp", "huge") else (BILINEAR,)
                for mode in modes:
                    tag = "%dx%d->%dx%d:%s:%d" % (sw, sh, ow, oh, name, mode)
                    yield "gray:" + tag, gray_image(sh, sw, 10 * si + di), m, (oh, ow), mode, np.float32(-7.5)
                    yield "rgba:" + tag, rgba_image(sh, sw, 10 * si + di), m, (oh, ow), mode, (1, 2, 3, 4)
