"""Case tables of the Gaussian + DoG pass (CPU, numpy only): which sigma
schedules and which plane sizes put every radius body of every kernel, every
tile edge and every scale-group seam under a plane comparison.

Only the sigma schedule decides which radius-specialised body runs, and only
the plane size decides which tile edge code runs, so the tables are lists of
(O, S, min_blur) and of plane sizes.  Everything here restates the library:

* schedule / radii: sift_schedule and the radius rule r = round(3 sigma)
  (test_gauss_cases.py holds them to sift_amd.shard.octave_radii and to
  oracle.schedule).
* plan_path / expected_plan: the thresholds of gauss_plan
  (csrc/sift_gauss_plan.hip).  The GPU tests do not trust them: they read the
  launch back through sift_last_gauss_plan and compare.
* tokens: what one octave of one schedule exercises, as hashable tokens;
  REQUIRED is the set the radius table must cover (asserted on the CPU from
  the restatement, on the GPU from the launches).
* RADIUS_TABLE: the committed greedy cover, each schedule with the path it
  claims per octave.  `python tests/gauss_cases.py --regen` prints the table
  the generator gives now; paste it here when a plan threshold moves
  (DESIGN.md section 17).
* geometry and scale-group tables: plane sizes as (multiples of the tile
  size, offset) so that a changed tile size moves the cases with it.

Paths (the names used in every table):
  staged8 / staged16   octave 0 from the staged input, largest radius <= 8 / 9..16
  base0                octave 0 on the fp64 upsample (largest radius > 16), k_gauss_dog<64>
  rw12                 k_gauss_rw<12>        octaves >= 1, largest radius <= 12
  rws16 / rws24        k_gauss_rw<16,true> / <24,true>   13..16 / 17..24
  tiles                k_gauss_dog<64>       25..39 (and planes one column wide)
  split                k_gauss_vert + k_gauss_dog<64>    >= 40; >= 90 keeps the fp64 planes

Not covered, because the shipping plan cannot select them: k_gauss_rw<16>,
k_gauss_rw<24> and k_gauss_rw<12,true> (experiment knobs only), batches and
k_seed_*.
"""
import math

import numpy as np

ASSUMED_BLUR = 0.5
MAX_LDS = 160 * 1024

# GaussKernel / GaussPath enumerators (include/sift_hip.h: SIFT_GAUSS_K_*, SIFT_GAUSS_PATH_*)
K_STAGED8, K_STAGED16, K_STAGED8_FUSED, K_STAGED16_FUSED, K_TILES, K_SPLIT_TILES = range(6)
K_WINDOW12, K_STREAMED16, K_STREAMED24 = 6, 10, 11
P_STAGED0, P_BASE0, P_TILES, P_SPLIT, P_WINDOW, P_STREAMED = range(6)

# path -> (kernel, plan path, rw, tile_w, tile_rows)
PATHS = {
    "staged8": (K_STAGED8, P_STAGED0, 0, 64, 32),
    "staged16": (K_STAGED16, P_STAGED0, 0, 64, 32),
    "base0": (K_TILES, P_BASE0, 0, 64, 32),
    "rw12": (K_WINDOW12, P_WINDOW, 12, 224, 8),
    "rws16": (K_STREAMED16, P_STREAMED, 16, 224, 8),
    "rws24": (K_STREAMED24, P_STREAMED, 24, 192, 8),
    "tiles": (K_TILES, P_TILES, 0, 64, 32),
    "split": (K_SPLIT_TILES, P_SPLIT, 0, 64, 32),
}
RW_PATHS = ("rw12", "rws16", "rws24")
FUSED_X, FUSED_Y = 60, 30   # a fused launch steps by its decided columns x rows (kFX x kFY)


def js_round(x):
    f = math.floor(x)
    return int(f + 1) if x - f >= 0.5 else int(f)


def schedule(O, S, min_blur, assumed_blur=ASSUMED_BLUR):
    """(blur, sigma) per (octave, scale); background.js:89-177."""
    NS = S + 3
    k = 2.0 ** (1.0 / S)
    blur = [[0.0] * NS for _ in range(O)]
    sigma = [[0.0] * NS for _ in range(O)]
    base = min_blur
    for o in range(O):
        for s in range(NS):
            if o > 0 and s == 0:
                base = blur[o - 1][S]
                blur[o][0] = base
            else:
                target = base * k ** float(s)
                src = assumed_blur if o == 0 else base
                blur[o][s] = target
                sigma[o][s] = math.sqrt(target * target - src * src)
    return blur, sigma


def radii(O, S, min_blur, assumed_blur=ASSUMED_BLUR):
    """Blur radius per (octave, scale); 0 for the un-blurred octave seed."""
    _, sigma = schedule(O, S, min_blur, assumed_blur)
    return [[0 if (o > 0 and s == 0) else js_round(3.0 * sigma[o][s]) for s in range(S + 3)] for o in range(O)]


def plan_path(o, rmax, w=64):
    """The launch path of octave o with largest radius rmax and w columns (gauss_plan)."""
    if o == 0:
        return "staged8" if rmax <= 8 else "staged16" if rmax <= 16 else "base0"
    keep_l64 = rmax >= 90
    if w >= 2 and not keep_l64 and rmax <= 24:
        return "rw12" if rmax <= 12 else "rws16" if rmax <= 16 else "rws24"
    return "split" if rmax >= 40 else "tiles"


def strip_stride(path, rmax):
    """LDS strip row stride of a k_gauss_dog launch, doubles (gauss_plan)."""
    if path == "staged8":
        return 2 * 15 + 8 + 6
    if path == "staged16":
        return 2 * 15 + 16 + 6
    sw = 64 + 2 * rmax + (4 if rmax <= 12 else 12)
    return sw + 2 if sw % 4 == 0 else sw


def schedule_fits(rad):
    """Every octave's strip fits the LDS (else the build is refused)."""
    for o, r in enumerate(rad):
        p = plan_path(o, max(r))
        if p not in RW_PATHS and p not in ("staged8", "staged16") and 8 * 32 * strip_stride(p, max(r)) > MAX_LDS:
            return False
    return True


def groups(path, gx, gy, NS, o):
    """Scale groups of the launch (gauss_plan)."""
    if o == 0:
        return 1
    thr = 600 if path in RW_PATHS else 400
    G = 1
    while G < NS and gx * gy * G < thr:
        G += 1
    return G


def expected_plan(o, rad_o, h, w, NS, px_before=0, fused=False):
    """What sift_last_gauss_plan must report for octave o (h x w, radii rad_o;
    px_before: pixels of one plane of every earlier octave -- the octave's
    planes start NS and NS - 1 times that many floats into their buffers, and
    the 16-byte stores need them aligned)."""
    rmax = max(rad_o)
    path = plan_path(o, rmax, w)
    kernel, ppath, rw, tw, th = PATHS[path]
    gx, gy = -(-w // tw), -(-h // th)
    G = groups(path, gx, gy, NS, o)
    if fused:
        kernel += K_STAGED8_FUSED - K_STAGED8
        gx = -(-(w - 2) // FUSED_X) if w > 2 else 1
        gy = -(-(h - 2) // FUSED_Y)
    return dict(kernel=kernel, path=ppath, rw=rw, tile_w=tw, tile_rows=th, gx=gx, gy=gy, G=G,
                keep_l64=int(o >= 1 and rmax >= 90), vsplit=int(path == "split"),
                vec=int(w % 4 == 0 and (NS * px_before) % 4 == 0 and ((NS - 1) * px_before) % 4 == 0),
                fused=int(fused))


def expected_plans(dims, rad, S, fused=False):
    """expected_plan of every octave of a pyramid (dims: [(h, w)]); fused: octave 0's launch."""
    out, px = [], 0
    for o, (h, w) in enumerate(dims):
        out.append(expected_plan(o, rad[o], h, w, S + 3, px, fused and o == 0))
        px += h * w
    return out


def can_fuse(path, h, w):
    return path in ("staged8", "staged16") and h >= 3 and w >= 3


# ---------------------------------------------------------------------------
# What an octave exercises, and what the radius table must cover.
# ---------------------------------------------------------------------------
def _base0_band(r):
    return "le12" if r <= 12 else "13_16" if r <= 16 else "17_32" if r <= 32 else "gt32"


def tokens(path, rad_o):
    """Coverage tokens of one octave on `path` with radii rad_o."""
    out = set()
    rmax = max(rad_o)
    for r in rad_o:
        if r == 0:
            continue  # the octave seed: a copy
        if path in ("staged8", "staged16") or path in RW_PATHS:
            out.add((path, r))
        elif path == "base0":
            out.add(("base0", _base0_band(r), r % 4))
        else:
            if r <= 12 or path == "tiles":
                out.add((path, r))                   # r <= 12: unrolled vert_glob2 / horz_full
            if 12 < r <= 32:
                out.add((path + "_gen2", r % 4))     # vert_glob_gen2 (split: k_gauss_vert), horz_full_gen
            elif r > 32:
                out.add((path + "_gen", r % 4))      # vert_glob_gen
    if path == "tiles":
        out.add(("tiles_rmax_parity", rmax % 2))     # the strip stride adjustment
    if path == "split" and rmax >= 90:
        out.add(("split_keep_l64",))
    return out


def required_tokens():
    req = set()
    req |= {("staged8", r) for r in range(1, 9)}
    req |= {("staged16", r) for r in range(1, 17)}
    req |= {("rw12", r) for r in range(1, 13)}
    req |= {("rws16", r) for r in range(2, 17)}
    req |= {("rws24", r) for r in range(3, 25)}
    req |= {("tiles", r) for r in range(5, 40)}   # generic radii too: the strip stride follows the radius
    req |= {("tiles_gen2", m) for m in range(4)} | {("tiles_gen", m) for m in range(4)}
    req |= {("tiles_rmax_parity", m) for m in range(2)}
    req |= {("split", r) for r in range(8, 13)}
    req |= {("split_gen2", m) for m in range(4)} | {("split_gen", m) for m in range(4)}
    req.add(("split_keep_l64",))
    req |= {("base0", band, m) for band in ("le12", "13_16", "17_32", "gt32") for m in range(4)}
    return req


REQUIRED = required_tokens()


def schedule_paths(O, S, min_blur):
    return tuple(plan_path(o, max(r)) for o, r in enumerate(radii(O, S, min_blur)))


def schedule_tokens(O, S, min_blur):
    rad = radii(O, S, min_blur)
    out = set()
    for o in range(O):
        out |= tokens(plan_path(o, max(rad[o])), rad[o])
    return out


def greedy_cover():
    """The radius table: schedules (3, S, 0.55 + 0.05 i) taken greedily, most
    new required tokens first, ties to the smaller (S, min_blur)."""
    universe = []
    for S in range(1, 10):
        for i in range(50):
            mb = (55 + 5 * i) / 100.0
            if schedule_fits(radii(3, S, mb)):
                universe.append(((3, S, mb), schedule_tokens(3, S, mb) & REQUIRED))
    left = set(REQUIRED)
    table = []
    while left:
        best = max(universe, key=lambda e: len(e[1] & left))  # max keeps the first of equals
        if not best[1] & left:
            raise RuntimeError("no schedule reaches %s" % sorted(left, key=str))
        left -= best[1]
        table.append((best[0], schedule_paths(*best[0])))
    return sorted(table)


# (O, S, min_blur), the path each octave claims
RADIUS_TABLE = [
    ((3, 1, 0.55), ('staged16', 'tiles', 'split')),
    ((3, 1, 0.85), ('base0', 'split', 'split')),
    ((3, 1, 1.1), ('base0', 'split', 'split')),
    ((3, 1, 1.45), ('base0', 'split', 'split')),
    ((3, 1, 1.5), ('base0', 'split', 'split')),
    ((3, 1, 2.75), ('base0', 'split', 'split')),
    ((3, 2, 0.7), ('staged8', 'rws16', 'tiles')),
    ((3, 2, 0.75), ('staged16', 'rws24', 'tiles')),
    ((3, 2, 1.25), ('staged16', 'tiles', 'split')),
    ((3, 4, 1.2), ('staged16', 'rws24', 'tiles')),
    ((3, 7, 1.5), ('staged16', 'rws24', 'split')),
    ((3, 7, 2.2), ('staged16', 'tiles', 'split')),
    ((3, 8, 0.55), ('staged8', 'rw12', 'rws16')),
    ((3, 8, 0.95), ('staged8', 'rw12', 'tiles')),
    ((3, 8, 1.3), ('staged16', 'rws24', 'tiles')),
    ((3, 8, 1.85), ('staged16', 'rws24', 'split')),
    ((3, 9, 0.9), ('staged8', 'rw12', 'rws24')),
    ((3, 9, 1.0), ('staged8', 'rws16', 'tiles')),
    ((3, 9, 1.2), ('staged8', 'rws16', 'tiles')),
    ((3, 9, 1.55), ('staged16', 'rws24', 'tiles')),
    ((3, 9, 2.9), ('base0', 'tiles', 'split')),
]


# ---------------------------------------------------------------------------
# Geometry: planes at the tile edges.  A size is (m, d): m tiles + d.
# ---------------------------------------------------------------------------
def size(md, tile):
    return md[0] * tile + md[1]


# family -> (O, S, min_blur), octave under test, its claimed path.  The octave
# after the one under test is built too: its base is the seed store.
GEOMETRY_SCHEDULES = {
    "rw12": ((3, 5, 0.8), 1, "rw12"),
    "rws16": ((3, 3, 0.8), 1, "rws16"),
    "rws24": ((3, 2, 0.8), 1, "rws24"),
    "tiles": ((3, 3, 1.6), 1, "tiles"),
    "split": ((3, 3, 2.5), 1, "split"),
    "staged8": ((2, 5, 0.8), 0, "staged8"),
    "staged16": ((2, 2, 0.8), 0, "staged16"),
    "base0": ((2, 3, 2.5), 0, "base0"),
}

# k_gauss_rw: TW (224 or 192) columns x 8 rows; plane = input size
RW_WIDTHS = [(0, 2), (0, 3), (0, 5), (1, -1), (1, 0), (1, 1), (1, 4), (2, 2)]   # at height 1 tile + 1
RW_HEIGHTS = [(0, 1), (0, 7), (1, 0), (1, 1), (2, 1)]                            # at width 1 tile + 1
# 64 x 32 tiles on octaves >= 1 (k_gauss_vert: 64-row blocks); plane = input size
TILE_WIDTHS = [(0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (1, 4), (2, 2)]          # at height 1 tile + 1
TILE_HEIGHTS = [(0, 1), (1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1)]        # at width 1 tile + 1
TILE_INTERIOR = ((3, 0), (3, 0))                                                 # 192 x 96: an interior tile
# octave 0: plane = 2W x 2H, so even sizes only (width residues 0 and 2 mod 4)
OCT0_WIDTHS = [(0, 2), (1, -2), (1, 0), (1, 2), (1, 4), (2, 2)]                  # at height 1 tile + 2
OCT0_HEIGHTS = [(0, 2), (1, -2), (1, 0), (1, 2), (2, 2)]                         # at width 1 tile + 2


def geometry_planes(family):
    """[(wmd, hmd)] of the family: plane sizes in (tiles, offset) form."""
    if family in RW_PATHS:
        return [(w, (1, 1)) for w in RW_WIDTHS] + [((1, 1), h) for h in RW_HEIGHTS]
    if family in ("tiles", "split"):
        return ([(w, (1, 1)) for w in TILE_WIDTHS] + [((1, 1), h) for h in TILE_HEIGHTS] + [TILE_INTERIOR])
    return [(w, (1, 2)) for w in OCT0_WIDTHS] + [((1, 2), h) for h in OCT0_HEIGHTS]


def geometry_cases():
    """[(family, wmd, hmd)] for every family."""
    return [(f, w, h) for f in GEOMETRY_SCHEDULES for (w, h) in geometry_planes(f)]


def geometry_input(family, wmd, hmd):
    """Input (W, H) that gives the octave under test the plane (wmd, hmd)."""
    _, o, path = GEOMETRY_SCHEDULES[family]
    tw, th = PATHS[path][3], PATHS[path][4]
    w, h = size(wmd, tw), size(hmd, th)
    if o == 0:
        assert w % 2 == 0 and h % 2 == 0
        return w // 2, h // 2
    return w, h


# ---------------------------------------------------------------------------
# Scale groups: narrow tall planes whose tile count puts G strictly between
# 1 and NS.  S = 3 (NS = 6); width 8, so gx = 1; the octave under test is 1.
# ---------------------------------------------------------------------------
GROUP_WIDTH = 8
GROUP_SCHEDULES = {
    "rw12": (3, 3, 0.65),
    "rws16": (3, 3, 0.8),
    "tiles": (3, 3, 1.6),
    "split": (3, 3, 2.5),
}
# family -> [(octave-1 height, G)]: G stops rising once gx gy G reaches 600
# (k_gauss_rw, 8-row tiles) or 400 (32-row tiles)
GROUP_HEIGHTS = {
    "rw12": [(2400, 2), (1600, 3), (1200, 4), (960, 5)],
    "rws16": [(2400, 2), (1600, 3), (1200, 4), (960, 5)],
    "tiles": [(6400, 2), (4288, 3), (3200, 4), (2560, 5)],
    "split": [(6400, 2), (4288, 3), (3200, 4), (2560, 5)],
}


def group_cases():
    return [(f, h, G) for f in GROUP_SCHEDULES for (h, G) in GROUP_HEIGHTS[f]]


# ---------------------------------------------------------------------------
# Inputs and references.
# ---------------------------------------------------------------------------
def noise_image(W, H, seed):
    """Random multiples of 1/4096 in [0, 1]: no symmetry that could hide a swapped tap or neighbour."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4097, size=(H, W)) / 4096.0).astype(np.float32)


def oracle_planes(img, O, S, min_blur, threads=1):
    """(dims, gauss, dog) of the oracle in the HIP path's operation order
    (CONV_SEPARABLE_FMA_VH): fp64 planes per octave, [scale][h][w].  The
    pyramid only -- no extrema, no refinement."""
    import ctypes

    import oracle as orc
    img = np.ascontiguousarray(img, dtype=np.float32)
    H, W = img.shape
    p = orc.make_params(O, S, min_blur, ASSUMED_BLUR)
    dims = orc.octave_dims(W, H, O)
    px = sum(h * w for h, w in dims)
    dp = ctypes.POINTER(ctypes.c_double)
    L = orc.lib()
    gauss = np.zeros(px * (S + 3))
    dog = np.zeros(px * (S + 2))
    orc.set_threads(threads)
    try:
        L.oracle_scale_space(img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), W, H, ctypes.byref(p),
                             orc.CONV_SEPARABLE_FMA_VH, gauss.ctypes.data_as(dp))
        L.oracle_dog(ctypes.byref(p), W, H, gauss.ctypes.data_as(dp), dog.ctypes.data_as(dp))
    finally:
        orc.set_threads(1)
    return dims, orc.split_pyramid(gauss, dims, S + 3), orc.split_pyramid(dog, dims, S + 2)


def numpy_blur(plane, sigma):
    """Independent statement of one blur in longdouble: weights exp(-i^2 / (2
    sigma^2)) / sum over i = -r..r with r = round(3 sigma) (sift.js:38-44),
    clamped indexing, vertical then horizontal."""
    r = js_round(3.0 * sigma)
    i = np.arange(-r, r + 1).astype(np.longdouble)
    w = np.exp(-(i * i) / (2 * np.longdouble(sigma) * np.longdouble(sigma)))
    w = w / w.sum()
    a = np.asarray(plane, dtype=np.longdouble)
    h, wd = a.shape
    v = np.zeros_like(a)
    for k in range(2 * r + 1):
        v += w[k] * a[np.clip(np.arange(h) + k - r, 0, h - 1), :]
    out = np.zeros_like(a)
    for k in range(2 * r + 1):
        out += w[k] * v[:, np.clip(np.arange(wd) + k - r, 0, wd - 1)]
    return out


def numpy_pyramid(img, O, S, min_blur):
    """Gaussian planes [octave][scale] in longdouble through numpy_blur:
    2x nearest upsample, every scale blurred from the octave base, next base =
    plane S at even rows and columns (background.js:84-118)."""
    _, sigma = schedule(O, S, min_blur)
    base = np.repeat(np.repeat(np.asarray(img, dtype=np.longdouble), 2, axis=0), 2, axis=1)
    out = []
    for o in range(O):
        planes = [base if (o > 0 and s == 0) else numpy_blur(base, sigma[o][s]) for s in range(S + 3)]
        out.append(planes)
        base = planes[S][::2, ::2]
    return out


def _print_table():
    print("RADIUS_TABLE = [")
    for sched, paths in greedy_cover():
        print("    (%r, %r)," % (sched, paths))
    print("]")


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--regen"]:
        _print_table()
    else:
        print("usage: python tests/gauss_cases.py --regen")
