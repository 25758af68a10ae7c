"""The RANSAC homography stage of include/sift_hip.h, restated in numpy.

The definition uses only + - * / and comparisons in fp64 with no fused
multiply-add, so these functions reproduce the device results bit for bit: the
GPU tests compare with assert_array_equal.  The definition is written twice:
once with Python ints and np.float64 scalars, one hypothesis at a time
(sample_scalar, hypothesis_scalar, inlier_scalar), and once vectorised over the
hypotheses (samples_ref, hypotheses_ref, score_ref); tests/test_ransac_ref.py
holds the two against each other.
"""
import numpy as np

POINT_PAIR_DTYPE = np.dtype([("qx", "<f8"), ("qy", "<f8"), ("tx", "<f8"), ("ty", "<f8")])

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_HYPOTHESES = 65536
FRAME = (3840.0, 2160.0)


# ---- one hypothesis at a time: Python ints, np.float64 scalars ---------------
def mix_scalar(z):
    """splitmix64's output mixer (sift_amd/synth.py: _splitmix64(x) = mix(x + GOLDEN))."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_scalar(seed, k, n):
    """The four distinct indices of hypothesis k over n >= 4 pairs, in draw order."""
    chosen = []
    for i in range(4):
        z = mix_scalar((seed + (4 * k + i + 1) * GOLDEN) & M64)
        r = ((z >> 32) * (n - i)) >> 32
        for c in sorted(chosen):
            if r >= c:
                r += 1
        chosen.append(r)
    return chosen


def hypothesis_scalar(points, seed, k):
    """(h float64 [9], valid) of hypothesis k."""
    one, zero = np.float64(1.0), np.float64(0.0)
    A = [[zero] * 9 for _ in range(8)]
    for j, s in enumerate(sample_scalar(seed, k, len(points))):
        x, y, X, Y = (np.float64(points[f][s]) for f in ("qx", "qy", "tx", "ty"))
        A[2 * j] = [x, y, one, zero, zero, zero, -X * x, -X * y, X]
        A[2 * j + 1] = [zero, zero, zero, x, y, one, -Y * x, -Y * y, Y]
    invalid = (np.zeros(9), False)
    with np.errstate(all="ignore"):
        for c in range(8):
            p, best = c, abs(A[c][c])
            for r in range(c + 1, 8):
                m = abs(A[r][c])
                if m > best:
                    p, best = r, m
            if not (best > 0.0 and np.isfinite(best)):
                return invalid
            A[p], A[c] = A[c], A[p]
            for r in range(c + 1, 8):
                f = A[r][c] / A[c][c]
                for j in range(c + 1, 9):
                    A[r][j] = A[r][j] - f * A[c][j]
        h = [zero] * 9
        h[8] = one
        for c in range(7, -1, -1):
            t = A[c][8]
            for j in range(c + 1, 8):
                t = t - A[c][j] * h[j]
            h[c] = t / A[c][c]
            if not np.isfinite(h[c]):
                return invalid
    return np.array(h, dtype=np.float64), True


def inlier_scalar(h, x, y, X, Y, t2):
    h = [np.float64(v) for v in h]
    x, y, X, Y, t2 = (np.float64(v) for v in (x, y, X, Y, t2))
    with np.errstate(all="ignore"):
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        w = (h[6] * x + h[7] * y) + h[8]
        du, dv = u - X * w, v - Y * w
        return bool(w > 0.0) and bool((du * du + dv * dv) < t2 * (w * w))


def ransac_scalar(points, K, seed, thresh):
    """(h [9], best k, inlier indices, H [K, 9], counts [K]) by the scalar forms alone (small cases)."""
    n = len(points)
    t2 = np.float64(thresh) * np.float64(thresh)
    H, counts, lists = np.zeros((K, 9)), np.full(K, -1, np.int32), {}
    if n >= 4:
        for k in range(K):
            H[k], ok = hypothesis_scalar(points, seed, k)
            if ok:
                lists[k] = [i for i in range(n) if inlier_scalar(H[k], *(points[f][i] for f in points.dtype.names), t2)]
                counts[k] = len(lists[k])
    else:
        H, counts = H[:0], counts[:0]
    best = -1
    for k in range(len(counts)):
        if counts[k] >= 0 and (best < 0 or counts[k] > counts[best]):
            best = k
    if best < 0:
        return np.zeros(9), -1, np.zeros(0, np.int32), H, counts
    return H[best].copy(), best, np.array(lists[best], np.int32), H, counts


# ---- vectorised over the hypotheses -----------------------------------------
def mix_ref(z):
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def samples_ref(seed, K, n):
    """int64 [K, 4]: the samples of hypotheses 0 .. K-1."""
    k = np.arange(K, dtype=np.uint64)
    out = np.zeros((K, 4), dtype=np.int64)
    with np.errstate(over="ignore"):
        for i in range(4):
            z = mix_ref(np.uint64(seed & M64) + (np.uint64(4) * k + np.uint64(i + 1)) * np.uint64(GOLDEN))
            r = (((z >> np.uint64(32)) * np.uint64(n - i)) >> np.uint64(32)).astype(np.int64)
            earlier = np.sort(out[:, :i], axis=1)
            for j in range(i):
                r = r + (r >= earlier[:, j])
            out[:, i] = r
    return out


def hypotheses_ref(points, K, seed):
    """(H float64 [K, 9], valid bool [K]); an invalid hypothesis is nine zeros."""
    n = len(points)
    s = samples_ref(seed, K, n)
    x, y, X, Y = (np.asarray(points[f], dtype=np.float64)[s] for f in ("qx", "qy", "tx", "ty"))  # [K, 4]
    A = np.zeros((K, 8, 9))
    A[:, 0::2, 0], A[:, 0::2, 1], A[:, 0::2, 2] = x, y, 1.0
    A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = -X * x, -X * y, X
    A[:, 1::2, 3], A[:, 1::2, 4], A[:, 1::2, 5] = x, y, 1.0
    A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = -Y * x, -Y * y, Y
    ar = np.arange(K)
    valid = np.ones(K, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(8):
            p = np.full(K, c)
            best = np.abs(A[:, c, c])
            for r in range(c + 1, 8):
                m = np.abs(A[:, r, c])
                gt = m > best
                p, best = np.where(gt, r, p), np.where(gt, m, best)
            valid &= (best > 0.0) & np.isfinite(best)
            rows_p, rows_c = A[ar, p].copy(), A[:, c].copy()
            A[ar, p] = rows_c
            A[:, c] = rows_p
            for r in range(c + 1, 8):
                f = A[:, r, c] / A[:, c, c]
                A[:, r, c + 1:] = A[:, r, c + 1:] - f[:, None] * A[:, c, c + 1:]
        h = np.zeros((K, 9))
        h[:, 8] = 1.0
        for c in range(7, -1, -1):
            t = A[:, c, 8].copy()
            for j in range(c + 1, 8):
                t = t - A[:, c, j] * h[:, j]
            h[:, c] = t / A[:, c, c]
            valid &= np.isfinite(h[:, c])
    h[~valid] = 0.0
    return h, valid


def inliers_ref(points, H, thresh):
    """bool [K, n]: pair i is an inlier of H[k] (H: [K, 9] or [K, 3, 3], h[8] as given)."""
    h = np.asarray(H, dtype=np.float64).reshape(-1, 9)[:, :, None]
    x, y, X, Y = (np.asarray(points[f], dtype=np.float64)[None, :] for f in ("qx", "qy", "tx", "ty"))
    t2 = np.float64(thresh) * np.float64(thresh)
    with np.errstate(all="ignore"):
        u = (h[:, 0] * x + h[:, 1] * y) + h[:, 2]
        v = (h[:, 3] * x + h[:, 4] * y) + h[:, 5]
        w = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
        du, dv = u - X * w, v - Y * w
        return (w > 0.0) & ((du * du + dv * dv) < t2 * (w * w))


def score_ref(points, H, thresh, chunk=64):
    """int32 [K]: the inlier counts of the matrices H."""
    h = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    out = np.zeros(len(h), dtype=np.int32)
    for a in range(0, len(h), chunk):
        out[a:a + chunk] = inliers_ref(points, h[a:a + chunk], thresh).sum(axis=1)
    return out


def ransac_homography(points, K, seed, thresh):
    """(H float64 [3, 3], best k or -1, inlier indices int32, all H [K, 9], counts int32 [K] with -1 = invalid)."""
    n = len(points)
    if n < 4 or K == 0:
        return np.zeros((3, 3)), -1, np.zeros(0, np.int32), np.zeros((0, 9)), np.zeros(0, np.int32)
    H, valid = hypotheses_ref(points, K, seed)
    counts = np.where(valid, score_ref(points, H, thresh), -1).astype(np.int32)
    best = int(np.argmax(counts))  # the first of the largest: lowest k among equals
    if counts[best] < 0:
        return np.zeros((3, 3)), -1, np.zeros(0, np.int32), H, counts
    inl = np.flatnonzero(inliers_ref(points, H[best:best + 1], thresh)[0]).astype(np.int32)
    return H[best].reshape(3, 3).copy(), best, inl, H, counts


def pair_points_ref(pairs, q_ori, q_kp, t_ori, t_kp):
    """POINT_PAIR_DTYPE [n]: (abs_x, abs_y) of the keypoints behind each pair's
    orientation records; four NaNs where an index is outside its list."""
    out = np.full(len(pairs), np.nan, dtype=POINT_PAIR_DTYPE)
    for f in out.dtype.names:
        out[f] = np.nan
    for i, (q, t) in enumerate(zip(pairs["query"], pairs["train"])):
        if not (0 <= q < len(q_ori) and 0 <= t < len(t_ori)):
            continue
        kq, kt = q_ori["keypoint"][q], t_ori["keypoint"][t]
        if not (0 <= kq < len(q_kp) and 0 <= kt < len(t_kp)):
            continue
        out[i] = (q_kp["abs_x"][kq], q_kp["abs_y"][kq], t_kp["abs_x"][kt], t_kp["abs_y"][kt])
    return out


PLANTED_H = np.array([[0.98, -0.05, 30.0], [0.04, 1.01, -20.0], [1.0e-5, -5.0e-6, 1.0]])


def planted(n, inlier_share, noise, seed):
    """(points POINT_PAIR_DTYPE [n], H_true [3, 3], planted bool [n]): round(n *
    inlier_share) pairs follow PLANTED_H in a 3840 x 2160 frame with uniform
    noise of +-`noise` pixels on the train point, the rest are uniform
    outliers; the two kinds are interleaved by a permutation."""
    rng = np.random.default_rng(seed)
    n_in = int(round(n * inlier_share))
    q = rng.uniform(0.0, 1.0, (n, 2)) * FRAME
    t = rng.uniform(0.0, 1.0, (n, 2)) * FRAME
    hom = np.concatenate([q, np.ones((n, 1))], axis=1) @ PLANTED_H.T
    proj = hom[:, :2] / hom[:, 2:3] + rng.uniform(-noise, noise, (n, 2))
    is_in = np.zeros(n, dtype=bool)
    is_in[rng.permutation(n)[:n_in]] = True
    t[is_in] = proj[is_in]
    pts = np.zeros(n, dtype=POINT_PAIR_DTYPE)
    pts["qx"], pts["qy"], pts["tx"], pts["ty"] = q[:, 0], q[:, 1], t[:, 0], t[:, 1]
    return pts, PLANTED_H.copy(), is_in
