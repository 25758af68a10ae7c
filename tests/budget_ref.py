"""numpy restatement of the keypoint budget of include/sift_hip.h (sift_budget):
the strength key, the grid cell and the two-step selection.  It sorts
(np.lexsort per cell, then over the survivors); the device selects with a radix
select and sorts nothing, so the two share no method."""
import numpy as np

ABS_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)
INF_BITS = np.uint64(0x7FF0000000000000)
MAX_CELLS = 16384

# Coordinates at the cell borders of a 20 x 12 frame with 8 px cells -- ncx = 3 (the last column 4 px wide), ncy = 2
# (the last row 4 px high) -- and the column each belongs to, written by hand.
_BELOW_8 = float(np.nextafter(8.0, 0.0))
_NAN, _INF = float("nan"), float("inf")
BORDER_FRAME = (20, 12, 8)
BORDER_X = [(0.0, 0), (_BELOW_8, 0), (8.0, 1), (15.999, 1), (16.0, 2), (19.5, 2), (20.0, 2), (1e9, 2), (_INF, 2),
            (-0.0, 0), (-1e-300, 0), (-5.0, 0), (-_INF, 0), (_NAN, 0)]


def budget(max_total=None, cell_px=0, max_per_cell=None):
    """(max_total, cell_px, max_per_cell) as the C struct stores them: None -> -1."""
    return (-1 if max_total is None else int(max_total), int(cell_px),
            -1 if max_per_cell is None else int(max_per_cell))


def keys(kp):
    """uint64 [n]: the bits of interp_value without the sign; a NaN has key 0."""
    v = np.ascontiguousarray(kp["interp_value"], dtype=np.float64)
    k = v.view(np.uint64) & ABS_MASK
    return np.where(k > INF_BITS, np.uint64(0), k)


def grid(width, height, cell_px):
    return -(-int(width) // int(cell_px)), -(-int(height) // int(cell_px))


def _axis(a, cell_px, nc):
    with np.errstate(invalid="ignore"):
        t = np.asarray(a, dtype=np.float64) / float(cell_px)
        inside = t < nc
        pos = t >= 0
    f = np.floor(np.where(pos & inside, t, 0.0)).astype(np.int64)  # the test comes before the cast
    return np.where(pos, np.where(inside, f, nc - 1), 0)


def cells(kp, width, height, cell_px):
    """int64 [n]: iy * ncx + ix; a NaN or a negative coordinate goes to column / row 0."""
    ncx, ncy = grid(width, height, cell_px)
    return _axis(kp["abs_y"], cell_px, ncy) * ncx + _axis(kp["abs_x"], cell_px, ncx)


def _strongest(idx, k, quota):
    """The `quota` members of idx that precede the others: key descending, index ascending."""
    order = np.lexsort((idx, ~k[idx]))  # the last key is the primary one; ~k descends where k ascends
    return idx[order[:quota]]


def select(kp, width, height, bud):
    """int32 [m]: the ascending indices the budget keeps."""
    max_total, cell_px, max_per_cell = bud
    n = len(kp)
    k = keys(kp)
    surv = np.arange(n, dtype=np.int64)
    if cell_px > 0 and max_per_cell >= 0:
        c = cells(kp, width, height, cell_px)
        parts = [_strongest(np.flatnonzero(c == v), k, max_per_cell) for v in np.unique(c)]
        surv = np.sort(np.concatenate(parts)) if parts else surv[:0]
    if max_total >= 0:
        surv = np.sort(_strongest(surv, k, max_total))
    return surv.astype(np.int32)
