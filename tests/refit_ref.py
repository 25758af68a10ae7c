"""The least-squares homography refit of include/sift_hip.h, restated in numpy.

Like tests/ransac_ref.py the definition uses only + - * /, comparisons and
negation in fp64 with no fused multiply-add, and every sum over pairs is taken
in one fixed tree that depends on the length of the list alone, so these
functions reproduce the device results bit for bit.  The definition is written
twice: with Python loops over np.float64 scalars and the tree as an explicit
loop (form="scalar"), and vectorised (form="vector");
tests/test_refit_ref.py holds the two against each other bitwise.
"""
import numpy as np

import ransac_ref as rr

CHUNK = 64
MAX_ROUNDS = 16
# (j, k) of the 44 sums in the order sift_copy_homography_fit_sums returns them:
# the upper triangle of the 8 x 8 normal matrix, row-major, with column 8 (g).
PAIRS = [(j, k) for j in range(8) for k in range(j, 9)]
F64 = np.float64


# ---- the summation tree ---------------------------------------------------------
def tree_sum_scalar(terms):
    """The sum of `terms` in the fixed tree: chunks of 64 in list order, the last
    padded with +0.0, each summed by halving (p[i] += p[i + s], s = 32 .. 1);
    the chunk sums are reduced by the same rule until one value is left."""
    v = [F64(t) for t in terms]
    if not v:
        return F64(0.0)
    while True:
        out = []
        for a in range(0, len(v), CHUNK):
            p = v[a:a + CHUNK]
            p = p + [F64(0.0)] * (CHUNK - len(p))
            s = CHUNK // 2
            while s:
                for i in range(s):
                    p[i] = p[i] + p[i + s]
                s //= 2
            out.append(p[0])
        v = out
        if len(v) == 1:
            return v[0]


def tree_sum(terms):
    """tree_sum_scalar along the last axis of an array."""
    v = np.asarray(terms, dtype=F64)
    if v.shape[-1] == 0:
        return np.zeros(v.shape[:-1])
    while True:
        m = v.shape[-1]
        c = -(-m // CHUNK)
        p = np.zeros(v.shape[:-1] + (c * CHUNK,))
        p[..., :m] = v
        p = p.reshape(v.shape[:-1] + (c, CHUNK))
        s = CHUNK // 2
        while s:
            p = p[..., :s] + p[..., s:2 * s]
            s //= 2
        v = p[..., 0]
        if c == 1:
            return v[..., 0]


# ---- one fit --------------------------------------------------------------------
def _bounds_scalar(vals):
    """(lo, hi) of the values that are not NaN (NaN, NaN without one); a zero bound is +0."""
    lo = hi = None
    for v in vals:
        v = F64(v)
        if v == v:
            lo = v if lo is None or v < lo else lo
            hi = v if hi is None or v > hi else hi
    if lo is None:
        return F64(np.nan), F64(np.nan)
    return lo + F64(0.0), hi + F64(0.0)


def _bounds_vector(vals):
    v = np.asarray(vals, dtype=F64)
    v = v[~np.isnan(v)]
    if not len(v):
        return F64(np.nan), F64(np.nan)
    return v.min() + F64(0.0), v.max() + F64(0.0)


def _side(xs, ys, bounds):
    """(centre x, centre y, half of the longer box side) of one image side."""
    lx, hx = bounds(xs)
    ly, hy = bounds(ys)
    half = F64(0.5)
    w, h = hx - lx, hy - ly
    return (lx + hx) * half, (ly + hy) * half, (h if h > w else w) * half


def _solve_scalar(A):
    """RANSAC step 3 on an 8 x 9 list of lists: (h' [8], valid)."""
    with np.errstate(all="ignore"):
        for c in range(8):
            p, best = c, abs(A[c][c])
            for r in range(c + 1, 8):
                m = abs(A[r][c])
                if m > best:
                    p, best = r, m
            if not (best > 0.0 and np.isfinite(best)):
                return None, False
            A[p], A[c] = A[c], A[p]
            for r in range(c + 1, 8):
                f = A[r][c] / A[c][c]
                for j in range(c + 1, 9):
                    A[r][j] = A[r][j] - f * A[c][j]
        h = [F64(0.0)] * 8
        for c in range(7, -1, -1):
            t = A[c][8]
            for j in range(c + 1, 8):
                t = t - A[c][j] * h[j]
            h[c] = t / A[c][c]
            if not np.isfinite(h[c]):
                return None, False
    return h, True


def _solve_vector(A):
    """The same on a float64 [8, 9] array, a row at a time."""
    A = np.array(A, dtype=F64)
    with np.errstate(all="ignore"):
        for c in range(8):
            col = np.abs(A[c:, c])
            best = col[0]
            p = c
            for r in range(1, 8 - c):
                if col[r] > best:
                    p, best = c + r, col[r]
            if not (best > 0.0 and np.isfinite(best)):
                return None, False
            A[[p, c]] = A[[c, p]]
            f = A[c + 1:, c] / A[c, c]
            A[c + 1:, c + 1:] = A[c + 1:, c + 1:] - f[:, None] * A[c, c + 1:][None, :]
        h = np.zeros(8)
        for c in range(7, -1, -1):
            t = A[c, 8]
            for j in range(c + 1, 8):
                t = t - A[c, j] * h[j]
            h[c] = t / A[c, c]
            if not np.isfinite(h[c]):
                return None, False
    return [F64(v) for v in h], True


def _denormalise(hn, box):
    """Step 5: (h float64 [9], valid) from h'[0..7] and the box."""
    cx, cy, dq, cX, cY, dt = box
    Hn = [[hn[0], hn[1], hn[2]], [hn[3], hn[4], hn[5]], [hn[6], hn[7], F64(1.0)]]
    with np.errstate(all="ignore"):
        G = [[r[0] / dq, r[1] / dq, r[2] - (r[0] * cx + r[1] * cy) / dq] for r in Hn]
        F = [[dt * G[0][c] + cX * G[2][c] for c in range(3)],
             [dt * G[1][c] + cY * G[2][c] for c in range(3)],
             [G[2][c] for c in range(3)]]
        d = F[2][2]
        if not (d != 0.0 and np.isfinite(d)):
            return np.zeros(9), False
        h = np.array([F[r][c] / d for r in range(3) for c in range(3)], dtype=F64)
    if not np.isfinite(h).all():
        return np.zeros(9), False
    return h, True


def fit_ref(points, index=None, form="vector"):
    """(H float64 [3, 3], valid, box float64 [6] = cx, cy, dq, cX, cY, dt, sums
    float64 [44] in PAIRS order) of the fit of the listed pairs (index None: all,
    in order).  An invalid fit has H = zeros; a list of fewer than four pairs forms
    no box and no sums (zeros)."""
    n = len(points)
    idx = np.arange(n) if index is None else np.asarray(index, dtype=np.int64)
    m = len(idx)
    if m < 4:
        return np.zeros((3, 3)), False, np.zeros(6), np.zeros(44)
    if ((idx < 0) | (idx >= n)).any():
        raise IndexError("index outside the points")
    scalar = form == "scalar"
    x, y, X, Y = (np.asarray(points[f], dtype=F64)[idx] for f in ("qx", "qy", "tx", "ty"))
    bounds = _bounds_scalar if scalar else _bounds_vector
    with np.errstate(all="ignore"):
        cx, cy, dq = _side(x, y, bounds)
        cX, cY, dt = _side(X, Y, bounds)
        box = np.array([cx, cy, dq, cX, cY, dt], dtype=F64)
        if scalar:
            one, zero = F64(1.0), F64(0.0)
            terms = [[] for _ in PAIRS]
            for i in range(m):
                u, v = (x[i] - cx) / dq, (y[i] - cy) / dq
                U, V = (X[i] - cX) / dt, (Y[i] - cY) / dt
                a = [u, v, one, zero, zero, zero, -(U * u), -(U * v), U]
                b = [zero, zero, zero, u, v, one, -(V * u), -(V * v), V]
                for t, (j, k) in zip(terms, PAIRS):
                    t.append(a[j] * a[k] + b[j] * b[k])
            sums = np.array([tree_sum_scalar(t) for t in terms], dtype=F64)
        else:
            u, v = (x - cx) / dq, (y - cy) / dq
            U, V = (X - cX) / dt, (Y - cY) / dt
            one, zero = np.ones(m), np.zeros(m)
            a = [u, v, one, zero, zero, zero, -(U * u), -(U * v), U]
            b = [zero, zero, zero, u, v, one, -(V * u), -(V * v), V]
            sums = tree_sum(np.stack([a[j] * a[k] + b[j] * b[k] for j, k in PAIRS]))
    if not (dq > 0.0 and dt > 0.0 and np.isfinite(dq) and np.isfinite(dt)):
        return np.zeros((3, 3)), False, box, sums
    A = [[F64(0.0)] * 9 for _ in range(8)]
    for s, (j, k) in zip(sums, PAIRS):
        A[j][k] = F64(s)
        if k < 8:
            A[k][j] = F64(s)
    hn, ok = (_solve_scalar if scalar else _solve_vector)(A)
    if not ok:
        return np.zeros((3, 3)), False, box, sums
    h, ok = _denormalise(hn, [F64(v) for v in box])
    return h.reshape(3, 3), ok, box, sums


# ---- the rounds -----------------------------------------------------------------
def refit_ref(points, H0, thresh, max_rounds, form="vector"):
    """(H float64 [3, 3], inlier indices int32 ascending, accepted rounds, counts
    [c0, c1, ...] of the start and of every round tried, the discarded one
    included) by the round rule of include/sift_hip.h."""
    assert 0 <= max_rounds <= MAX_ROUNDS
    H = np.array(H0, dtype=F64).reshape(3, 3)
    inl = np.flatnonzero(rr.inliers_ref(points, H.reshape(1, 9), thresh)[0]).astype(np.int32)
    counts, rounds = [len(inl)], 0
    for r in range(1, max_rounds + 1):
        if len(inl) < 4:
            break
        Hr, ok, _, _ = fit_ref(points, inl, form)
        if not ok:
            break
        new = np.flatnonzero(rr.inliers_ref(points, Hr.reshape(1, 9), thresh)[0]).astype(np.int32)
        counts.append(len(new))
        if len(new) < len(inl):
            break
        same = len(new) == len(inl)
        H, inl, rounds = Hr, new, r
        if same:
            break
    return H, inl, rounds, counts


def corner_error(H, H_true=rr.PLANTED_H, frame=rr.FRAME):
    """The largest transfer error, in pixels, of the frame's corners and centre under H against H_true."""
    w, h = frame
    worst = 0.0
    for x, y in ((0.0, 0.0), (w, 0.0), (0.0, h), (w, h), (w / 2, h / 2)):
        p = np.array([x, y, 1.0])
        a, b = np.asarray(H).reshape(3, 3) @ p, np.asarray(H_true).reshape(3, 3) @ p
        worst = max(worst, float(np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2])))
    return worst
