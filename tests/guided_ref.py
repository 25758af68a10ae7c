"""numpy statement of guided descriptor matching (include/sift_hip.h, DESIGN.md
section 18): projection, candidates and top-2, and the grid behind n_visited.

Everything positional is float64 with one rounding per operation, which is
what numpy's elementwise operators and Python's floats do; every distance is an
integer.  guided_loops is the definition once more with Python scalars and two
loops, for small cases.
"""
import math

import numpy as np

from match_ref import MATCH_DTYPE, NONE_D2

MAX_CELLS = 1 << 20


def _xy(a, n):
    a = np.asarray(a)
    if a.dtype.names:
        a = np.stack([a["x"], a["y"]], 1)
    return np.asarray(a, dtype=np.float64).reshape(n, 2)


def _mask(m, n):
    return np.ones(n, bool) if m is None else np.asarray(m).reshape(n) != 0


def project(query_xy, h, query_mask=None):
    """(projected [n] bool, px, py) of the query rows."""
    h = np.asarray(h, dtype=np.float64).reshape(9)
    xy = _xy(query_xy, len(query_xy))
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        w = (h[6] * x + h[7] * y) + h[8]
        rinv = 1.0 / w
        px, py = u * rinv, v * rinv
        ok = _mask(query_mask, len(xy)) & (w > 0.0) & (px - px == 0.0) & (py - py == 0.0)
    return ok, px, py


def candidates(px, py, train_xy, train_mask, radius):
    """bool [n_train]: the candidates of one projected row at (px, py)."""
    with np.errstate(all="ignore"):
        r2 = np.float64(radius) * np.float64(radius)              # formed once; inf for a huge radius
        dx, dy = train_xy[:, 0] - px, train_xy[:, 1] - py
        return train_mask & ((dx * dx + dy * dy) <= r2)          # a NaN compares false


def guided_ref(query, query_xy, train, train_xy, h, radius, query_mask=None, train_mask=None):
    """(records MATCH_DTYPE [n_query], n_projected, n_candidates)."""
    query = np.asarray(query, dtype=np.uint8).reshape(-1, 128).astype(np.int64)
    train = np.asarray(train, dtype=np.uint8).reshape(-1, 128).astype(np.int64)
    nq, nt = len(query), len(train)
    txy, tm = _xy(train_xy, nt), _mask(train_mask, nt)
    ok, px, py = project(query_xy, h, query_mask)
    out = np.zeros(nq, dtype=MATCH_DTYPE)
    out["best"] = out["second"] = -1
    out["d2_best"] = out["d2_second"] = NONE_D2
    n_cand = 0
    for q in np.flatnonzero(ok):
        c = np.flatnonzero(candidates(px[q], py[q], txy, tm, radius))
        n_cand += len(c)
        if len(c) == 0:
            continue
        d2 = ((train[c] - query[q]) ** 2).sum(1)
        order = np.lexsort((c, d2))[:2]                           # by d2, then train index
        out["best"][q], out["d2_best"][q] = c[order[0]], d2[order[0]]
        if len(order) > 1:
            out["second"][q], out["d2_second"][q] = c[order[1]], d2[order[1]]
    return out, int(ok.sum()), int(n_cand)


def guided_loops(query, query_xy, train, train_xy, h, radius, query_mask=None, train_mask=None):
    """The definition with Python scalars and two loops (small cases): the same triple."""
    h = [float(a) for a in np.asarray(h, dtype=np.float64).reshape(9)]
    qxy, txy = _xy(query_xy, len(query)), _xy(train_xy, len(train))
    r2 = float(radius) * float(radius)
    out = np.zeros(len(query), dtype=MATCH_DTYPE)
    n_proj = n_cand = 0
    for q in range(len(query)):
        pairs = []
        x, y = float(qxy[q, 0]), float(qxy[q, 1])
        w = (h[6] * x + h[7] * y) + h[8]
        if (query_mask is None or query_mask[q]) and w > 0.0:     # 1.0 / w is only formed for w > 0
            rinv = 1.0 / w
            px, py = ((h[0] * x + h[1] * y) + h[2]) * rinv, ((h[3] * x + h[4] * y) + h[5]) * rinv
            if px - px == 0.0 and py - py == 0.0:
                n_proj += 1
                for t in range(len(train)):
                    dx, dy = float(txy[t, 0]) - px, float(txy[t, 1]) - py
                    if (train_mask is None or train_mask[t]) and (dx * dx + dy * dy) <= r2:
                        pairs.append((sum((int(a) - int(b)) ** 2 for a, b in zip(query[q], train[t])), t))
        n_cand += len(pairs)
        pairs = sorted(pairs)[:2] + [(NONE_D2, -1)] * 2
        out[q] = (pairs[0][1], pairs[1][1], pairs[0][0], pairs[1][0])
    return out, n_proj, n_cand


def grid_ref(width, height, radius):
    """(cell_px, ncx, ncy): the smallest c from max(1, min(ceil(radius), max(W, H))) up that keeps the cells
    within MAX_CELLS."""
    c = max(1, min(math.ceil(radius), max(width, height)))
    while -(-width // c) * -(-height // c) > MAX_CELLS:
        c += 1
    return c, -(-width // c), -(-height // c)


def axis(a, c, nc):
    """The clamped column (or row) of coordinates a: the test comes before the cast."""
    with np.errstate(all="ignore"):
        t = np.asarray(a, dtype=np.float64) / np.float64(c)
        inside = (t >= 0.0) & (t < nc)
        return np.where(t >= 0.0, np.where(inside, np.floor(np.where(inside, t, 0.0)), nc - 1), 0).astype(np.int64)


def visited_ref(query_xy, train_xy, width, height, h, radius, query_mask=None, train_mask=None):
    """n_visited: over the projected rows, the train rows filed in the cells the row visits."""
    c, ncx, ncy = grid_ref(width, height, radius)
    txy = _xy(train_xy, len(train_xy))
    filed = _mask(train_mask, len(txy)) & ~np.isnan(txy[:, 0]) & ~np.isnan(txy[:, 1])
    ix, iy = axis(txy[filed, 0], c, ncx), axis(txy[filed, 1], c, ncy)
    ok, px, py = project(query_xy, h, query_mask)
    r = np.float64(radius)
    with np.errstate(all="ignore"):
        x0 = np.maximum(axis(px - r, c, ncx) - 1, 0)
        x1 = np.minimum(axis(px + r, c, ncx) + 1, ncx - 1)
        y0 = np.maximum(axis(py - r, c, ncy) - 1, 0)
        y1 = np.minimum(axis(py + r, c, ncy) + 1, ncy - 1)
    total = 0
    for q in np.flatnonzero(ok):
        total += int(((ix >= x0[q]) & (ix <= x1[q]) & (iy >= y0[q]) & (iy <= y1[q])).sum())
    return total


def info_ref(query, query_xy, train, train_xy, width, height, h, radius, query_mask=None, train_mask=None):
    """(records, info dict as Context.guided_info())."""
    rec, n_proj, n_cand = guided_ref(query, query_xy, train, train_xy, h, radius, query_mask, train_mask)
    c, ncx, ncy = grid_ref(width, height, radius)
    return rec, dict(cell_px=c, ncx=ncx, ncy=ncy, n_projected=n_proj,
                     n_visited=visited_ref(query_xy, train_xy, width, height, h, radius, query_mask, train_mask),
                     n_candidates=n_cand)
