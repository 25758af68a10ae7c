"""Inputs that put the extrema scan on every edge of its geometry, and a
restatement of SIFT_findExtremas that labels them (CPU, numpy only).

* reference_lists: strict 26-neighbour max / min on fp64 copies of the
  planes, border excluded, scales 1..S; |v| >= 0.8 thr -> candidate list,
  else low-contrast list; order octave, scale, y, x.  The C oracle
  (oracle.extrema_lists) stays the judge of results; this function labels
  inputs and proves coverage (test_extrema_cases.py holds it to the oracle,
  bit for bit).  Its keyword arguments are deliberately WRONG scans, used
  only to show that the tables tell them apart.
* build_table(geom, S): one caller-supplied DoG pyramid per geometry on a
  zero background (all ties: no extremum) plus labelled plants
  (label, octave, s, y, x, expected), expected in {candidate, low, none}.
  Plants are independent because their footprints -- the 3 x 3 x 3 box
  around the centre, clipped to the plane -- do not overlap: a plant writes
  only inside its own box, and a centre is decided by its own box alone.
  (A 5 x 5 footprint in y and x would also keep the labels of a plant's
  NEIGHBOURS independent; those are not expectations of the table, the
  reference labels them, and 3 x 3 packs three times as many plants.)  The
  builder refuses a plant whose footprint is taken (Table.fits) and asserts
  the rule when it writes (Table.plant).
* noise_table(geom, S, seed): integers in [-16, 16] times t / 16 -- many
  ties, and |v| == t exactly for |k| = 16.  A strict extremum of 26 uniform
  neighbours is almost always one of the outermost levels: P(centre = k and
  all 26 below) = (1/33) ((k + 16) / 33)^26, which puts 55 % of the extrema
  on |k| = 16, 24 % on 15, 10 % on 14.  With t / 8 (threshold at |k| = 8)
  the low-contrast list stays empty; with t / 16 it takes 45 %.
* edge_image(seed) / EDGE_SEEDS: small noise images whose built pyramids put
  extrema on every fused-tile / scan-word / strip edge of octave 0
  (test_extrema_cases.py proves it from the oracle).

Words, strips and groups (csrc/sift_kernels.h, sift_extrema.hip): a scan
word is 62 columns from column 0, a fused word 60 columns from column 1, a
strip 30 rows from row 1, a scale group at most 5 scales (S > 5 splits:
6 = 3+3, 7 = 4+3, 8 = 4+4, 9 = 5+4).

What does not fit: the neighbour family is 26 offsets x {max, min} x 4
neighbour values = 208 plants per context (interior, centre at column
62k-1 / 62k, row 30k / 30k+1, scale 1 / S / either side of the group
boundary), 27 plane values of footprint each.  A fixed column or row leaves
one line of centres per three scales, so no single table holds 208 plants
on, say, column 61.  Every table therefore takes as many as fit, starting
from an index that depends on (geometry, S) and dealing the constrained
contexts in turn; test_extrema_cases.py asserts that every table holds
every context its geometry has, and that the tables together hold all 208
of every context.
"""
import itertools

import numpy as np

from refine_cases import contrast_threshold

WORD = 62          # kXW
FUSED_WORD = 60    # kFX (from column 1)
STRIP = 30         # kXRows, kFY
MAX_GROUP = 5      # kXMaxGroup
FLT_MIN = np.float32(1.17549435e-38)
FLT_MAX = np.finfo(np.float32).max
DENORMAL = np.float32(1e-45)   # the smallest positive fp32 denormal

OFFSETS = [(ds, dy, dx) for ds in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (ds, dy, dx) != (0, 0, 0)]
KINDS = ("equal", "ulp_defeats", "ulp_keeps", "nan")
# the neighbour family of one context: (offset index, sign of the centre, neighbour value)
COMBOS = [(k, sign, kind) for kind in KINDS for sign in (+1, -1) for k in range(26)]

#                 W     H  O
GEOMETRIES = [(31, 16, 3),     # (32,62), (16,31), (8,16)
              (32, 17, 2),     # (34,64), (17,32)
              (63, 33, 2),     # (66,126), (33,63)
              (125, 17, 2),    # (34,250), (17,125)
              (1990, 3, 1),    # (6,3980): 65 words per row -- k_emit's second chunk
              (2, 2, 1),       # (4,4): a single interior 2 x 2
              (990, 3, 1),     # (6,1980): 32 words -- 8 blocks at S <= 5, 16 at S = 7, 9
              (5, 5, 2),       # (10,10), (5,5): three interior rows
              (7, 3, 2)]       # (6,14), (3,7): one interior row
S_ALL = (1, 2, 3, 5, 6, 7, 8, 9)
S_FEW = (1, 7, 9)
TABLES = [(g, S) for g in GEOMETRIES[:2] for S in S_ALL] + [(g, S) for g in GEOMETRIES[2:] for S in S_FEW]

NOISE_GEOM = (95, 47, 3)       # (94,190), (47,95), (24,48)
# seeds per S: their tables together hold an extremum in every interior column and row and at every scale of every
# octave (test_extrema_cases.py asserts it; S >= 5 needs one table, the sparser pyramids below it more)
NOISE_SEEDS = {1: (1, 2, 3, 4), 2: (1, 2, 3), 3: (1, 2), 5: (1,), 6: (1,), 7: (1,), 8: (1,), 9: (1,)}
NOISE_TABLES = [(NOISE_GEOM, S, seed) for S in S_ALL for seed in NOISE_SEEDS[S]]


def fp32_threshold(S):
    """t_up: the smallest fp32 whose value is >= 0.8 thr."""
    t = 0.8 * contrast_threshold(S)
    f = np.float32(t)
    if float(f) < t:
        f = np.nextafter(f, np.float32(np.inf))
    assert float(f) >= t > float(np.nextafter(f, np.float32(0)))
    return f


def scale_groups(S):
    """First scale of every group of k_extrema, and S + 1."""
    ng = (S + MAX_GROUP - 1) // MAX_GROUP
    per, rem = S // ng, S % ng
    return [1 + g * per + min(g, rem) for g in range(ng)] + [S + 1]


def block_count(dims, S):
    """Blocks of the k_extrema launch: one wave per unit, four per block."""
    ng = (S + MAX_GROUP - 1) // MAX_GROUP
    units = sum(ng * ((w + WORD - 1) // WORD) * ((h - 2 + STRIP - 1) // STRIP) for h, w in dims if h >= 3 and w >= 3)
    return (units + 3) // 4


# ---------------------------------------------------------------------------
# The reference scan
# ---------------------------------------------------------------------------
def reference_lists(planes, dims, S, ge=False, drop=None, nan_drop=False, thr_gt=False, ftz=False):
    """((rec (N,4) int32 [o, s, x, y], value (N,)), (low_rec, low_value)) of
    the octave planes `planes` (one (S+2, h, w) array per octave).

    The keyword arguments are wrong scans (test_the_table_tells_wrong_scans_apart):
    ge -- ties count as extrema; drop -- neighbour OFFSETS[drop] is not
    looked at; nan_drop -- a NaN neighbour is skipped (fmax / fmin); thr_gt
    -- the kernel's fp32 threshold comparison |v| >= t_up written as > (0.8
    thr is no fp32 value, so in fp64 the two agree on every fp32 plane);
    ftz -- denormal plane values read as zero."""
    pix_thr = 0.8 * contrast_threshold(S)
    t_up = float(fp32_threshold(S))
    out = ([], [], [], [])
    for o, (h, w) in enumerate(dims):
        D = np.array(planes[o], dtype=np.float64)
        assert D.shape == (S + 2, h, w)
        if h < 3 or w < 3:
            continue
        if ftz:
            D = np.where(np.abs(D) < float(FLT_MIN), np.copysign(0.0, D), D)
        for s in range(1, S + 1):
            c = D[s, 1:h - 1, 1:w - 1]
            is_max = np.ones(c.shape, dtype=bool)
            is_min = np.ones(c.shape, dtype=bool)
            with np.errstate(invalid="ignore"):
                for k, (ds, dy, dx) in enumerate(OFFSETS):
                    if k == drop:
                        continue
                    v = D[s + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                    below, above = (v <= c, v >= c) if ge else (v < c, v > c)
                    if nan_drop:
                        below, above = below | np.isnan(v), above | np.isnan(v)
                    is_max &= below
                    is_min &= above
            ys, xs = np.nonzero(is_max | is_min)   # raster order
            v = c[ys, xs]
            cand = (np.abs(v) > t_up) if thr_gt else (np.abs(v) >= pix_thr)
            rec = np.stack([np.full(ys.shape, o), np.full(ys.shape, s), xs + 1, ys + 1], axis=1)
            out[0].append(rec[cand])
            out[1].append(v[cand])
            out[2].append(rec[~cand])
            out[3].append(v[~cand])

    def cat(parts, shape, dt):
        return np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dtype=dt)

    return ((cat(out[0], (0, 4), np.int32), cat(out[1], (0,), np.float64)),
            (cat(out[2], (0, 4), np.int32), cat(out[3], (0,), np.float64)))


def labels_of(lists):
    """{(o, s, y, x): 'candidate' | 'low'} of a pair of lists; anything else is 'none'."""
    (rec, _), (low, _) = lists
    lab = {(int(r[0]), int(r[1]), int(r[3]), int(r[2])): "candidate" for r in rec}
    lab.update({(int(r[0]), int(r[1]), int(r[3]), int(r[2])): "low" for r in low})
    return lab


# ---------------------------------------------------------------------------
# The plant table
# ---------------------------------------------------------------------------
class Table:
    """One caller DoG pyramid.  planes[o]: (S + 2, h, w) float32; plants:
    (label, o, s, y, x, expected); contexts[name]: the COMBOS indices placed."""

    def __init__(self, geom, S):
        import oracle as orc
        self.geom, self.S = geom, S
        self.W, self.H, self.O = geom
        self.dims = orc.octave_dims(*geom)
        self.planes = [np.zeros((S + 2, h, w), dtype=np.float32) for h, w in self.dims]
        self.taken = [np.zeros((S + 2, h, w), dtype=bool) for h, w in self.dims]
        self.plants = []
        self.contexts = {}
        self.t = fp32_threshold(S)
        self.blocks = block_count(self.dims, S)

    def _box(self, o, s, y, x):
        h, w = self.dims[o]
        return (o, slice(s - 1, s + 2), slice(max(y - 1, 0), min(y + 2, h)), slice(max(x - 1, 0), min(x + 2, w)))

    def fits(self, o, s, y, x):
        h, w = self.dims[o]
        if not (1 <= s <= self.S and 1 <= y <= h - 2 and 1 <= x <= w - 2):
            return False
        o, ss, ys, xs = self._box(o, s, y, x)
        return not self.taken[o][ss, ys, xs].any()

    def plant(self, label, o, s, y, x, centre, neighbours=(), expected=None):
        """Centre value and neighbour values [(ds, dy, dx, v)] at a free footprint."""
        assert self.fits(o, s, y, x), ("footprints overlap", label, o, s, y, x)
        _, ss, ys, xs = self._box(o, s, y, x)
        self.taken[o][ss, ys, xs] = True
        self.planes[o][s, y, x] = np.float32(centre)
        for ds, dy, dx, v in neighbours:
            assert max(abs(ds), abs(dy), abs(dx)) == 1
            self.planes[o][s + ds, y + dy, x + dx] = np.float32(v)
        if expected is None:
            expected = "candidate" if abs(np.float32(centre)) >= self.t else "low"
        self.plants.append((label, o, s, y, x, expected))

    def spots(self, octaves=None, scales=None, rows=None, cols=None):
        """Free centres, a 3-pixel / 3-scale grid first (it packs), then the rest."""
        for o in (range(self.O) if octaves is None else octaves):
            h, w = self.dims[o]
            if h < 3 or w < 3:
                continue
            sl = [s for s in (scales if scales is not None else
                              list(range(1, self.S + 1, 3)) + [s for s in range(1, self.S + 1) if s % 3 != 1])
                  if 1 <= s <= self.S]
            yl = [y for y in (rows if rows is not None else
                              list(range(1, h - 1, 3)) + [y for y in range(1, h - 1) if y % 3 != 1])
                  if 1 <= y <= h - 2]
            xl = [x for x in (cols if cols is not None else
                              list(range(1, w - 1, 3)) + [x for x in range(1, w - 1) if x % 3 != 1])
                  if 1 <= x <= w - 2]
            for s, y, x in itertools.product(sl, yl, xl):
                if self.fits(o, s, y, x):
                    yield o, s, y, x

    def arrays(self):
        return np.concatenate([p.ravel() for p in self.planes])

    def lists(self, **wrong):
        return reference_lists(self.planes, self.dims, self.S, **wrong)

    def finite_copy(self):
        """The flat planes with NaN, Inf and FLT_MAX entries zeroed (for the refinement smoke check)."""
        a = self.arrays().copy()
        a[~np.isfinite(a) | (np.abs(a) >= FLT_MAX)] = 0.0
        return a


def special_columns(w):
    """{family: columns}: the plane's first and last interior column, both
    sides of every scan-word and fused-word boundary, bits 31|32 of a word."""
    inside = lambda c: sorted(x for x in set(c) if 1 <= x <= w - 2)   # noqa: E731
    nw = (w + WORD - 1) // WORD
    few = sorted(set(range(min(nw, 3))) | {nw - 1})   # the first words and the last (wide planes)
    return {"edge": inside([1, w - 2]),
            "word": inside([WORD * k - 1 for k in range(1, nw)] + [WORD * k for k in range(1, nw)]),
            "fused": inside([FUSED_WORD * k + d for k in [j + 1 for j in few] for d in (0, 1)]),
            "bit31": inside([WORD * k + b for k in few for b in (31, 32)])}


def special_rows(h):
    inside = lambda c: sorted(y for y in set(c) if 1 <= y <= h - 2)   # noqa: E731
    ks = range(1, (h + STRIP - 1) // STRIP + 1)
    return {"edge": inside([1, h - 2]), "strip": inside([STRIP * k + d for k in ks for d in (0, 1)])}


def special_scales(S):
    g = scale_groups(S)
    return {"edge": sorted({1, S}), "group": sorted(s for b in g[1:-1] for s in (b - 1, b))}


def _neighbour_plant(T, ctx, i, pos):
    k, sign, kind = COMBOS[i]
    c = np.float32(sign) * np.float32(2) * T.t
    toward = np.float32(sign * np.inf)          # above a maximum / below a minimum defeats it
    v = {"equal": c, "ulp_defeats": np.nextafter(c, toward), "ulp_keeps": np.nextafter(c, -toward),
         "nan": np.float32(np.nan)}[kind]
    T.plant("nbr.%s.%d.%s.%s" % (ctx, k, "max" if sign > 0 else "min", kind), *pos, centre=c,
            neighbours=[OFFSETS[k] + (v,)], expected="candidate" if kind == "ulp_keeps" else "none")
    T.contexts.setdefault(ctx, []).append(i)


def context_spots(T):
    """{context: generator of free centres} of the neighbour family, per geometry."""
    ctx = {}
    per_o = lambda f: [(o, f(*T.dims[o])) for o in range(T.O)]   # noqa: E731

    def chain(items, key):
        return itertools.chain.from_iterable(T.spots(octaves=[o], **{key: v}) for o, v in items if v)

    word = per_o(lambda h, w: special_columns(w)["word"])
    strip = per_o(lambda h, w: special_rows(h)["strip"])
    if any(v for _, v in word):
        ctx["col62k-1"] = chain([(o, [x for x in v if x % WORD == WORD - 1]) for o, v in word], "cols")
        ctx["col62k"] = chain([(o, [x for x in v if x % WORD == 0]) for o, v in word], "cols")
    if any(v for _, v in strip):
        ctx["row30k"] = chain([(o, [y for y in v if y % STRIP == 0]) for o, v in strip], "rows")
        ctx["row30k+1"] = chain([(o, [y for y in v if y % STRIP == 1]) for o, v in strip], "rows")
    ctx["scale1"] = T.spots(scales=[1])
    ctx["scaleS"] = T.spots(scales=[T.S])
    grp = special_scales(T.S)["group"]
    if grp:
        ctx["group_last"] = T.spots(scales=grp[0::2])
        ctx["group_first"] = T.spots(scales=grp[1::2])
    return ctx


def position_columns(w, h, o):
    """The special columns that get an isolated maximum and minimum in octave
    o of height h.  Fused words exist in octave 0 only.  On planes of more
    than 8 words: the first three scan-word boundaries and the last (the
    neighbour family's column contexts are dealt over all of them).  A plane
    of fewer than 12 interior rows has two lines of footprints per three
    scales, which columns 60, 61 and 62 cannot share with both signs: no
    fused columns there, and one side of each word boundary, alternating."""
    nw = (w + WORD - 1) // WORD
    sc = special_columns(w)
    if o or h - 2 < 12:
        sc["fused"] = []
    if nw > 8:
        sc["word"] = [x for x in sc["word"] if (x + 1) // WORD in (1, 2, 3, nw - 1)]
    if h - 2 < 12:
        sc["word"] = [x for x in sc["word"] if (x % WORD == 0) == (((x + 1) // WORD) % 2 == 0)]
        sc["bit31"] = [x for x in sc["bit31"] if (x % WORD == 31) == ((x // WORD) % 2 == 0)]   # the same for bits 31|32
    return sc


def _positions(T):
    """An isolated maximum and minimum on every special column, row and scale of every octave."""
    for o, (h, w) in enumerate(T.dims):
        if h < 3 or w < 3:
            continue
        # the corners of scale 1 (of scale S too, where its footprints clear scale 1's): four plants that
        # stand on both edge columns and both edge rows with both signs -- all a small plane has room for
        for s, flip in ((1, 1), (T.S, -1)) if T.S >= 4 else ((1, 1),):
            for y, x, sign in ((1, 1, 1), (h - 2, 1, -1), (1, w - 2, -1), (h - 2, w - 2, 1)):
                if T.fits(o, s, y, x):
                    c = np.float32(sign * flip) * T.t * np.float32(2.5)
                    T.plant("pos.corner.o%d.%d.%d.%d.%s" % (o, s, y, x, "max" if sign * flip > 0 else "min"),
                            o, s, y, x, centre=c)
        wanted = [("col." + f, "cols", v) for f, cols in position_columns(w, h, o).items() for v in cols]
        wanted += [("row." + f, "rows", v) for f, rows in special_rows(h).items() for v in rows]
        wanted += [("scale." + f, "scales", v) for f, sc in special_scales(T.S).items() for v in sc]
        merged = {}   # a column of two families (61: word and fused) gets one pair of plants, named for both
        for fam, key, v in wanted:
            merged.setdefault((key, v), []).append(fam)
        # scales first, then rows, then columns: a plant also stands on whatever its free coordinates
        # happen to be, and a small plane has room only if such plants are counted
        order = {"scales": 0, "rows": 1, "cols": 2}
        wanted = sorted((("+".join(f), key, v) for (key, v), f in merged.items()), key=lambda q: order[q[1]])
        axis = {"scales": 2, "rows": 3, "cols": 4}
        for j, (fam, key, v) in enumerate(wanted):
            for sign in (+1, -1):
                end = ".max" if sign > 0 else ".min"
                if any(p[0].startswith("pos.") and p[0].endswith(end) and p[1] == o and p[axis[key]] == v
                       for p in T.plants):
                    continue
                pos = next(T.spots(octaves=[o], **{key: [v]}), None)
                if pos is not None:   # distinct magnitudes between 2 t and 3 t
                    c = np.float32(sign) * T.t * np.float32(2 + (j % 64) / 64.0)
                    T.plant("pos.%s.o%d.%d%s" % (fam, o, v, end), *pos, centre=c)


def _threshold(T):
    t, inf = T.t, np.float32(np.inf)
    below = np.nextafter(t, np.float32(0))
    cases = []
    for sg, nm in ((+1, "+"), (-1, "-")):
        f = np.float32(sg)
        cases += [("thr.t_up" + nm, f * t, (), "candidate"), ("thr.below" + nm, f * below, (), "low"),
                  ("thr.denormal" + nm, f * DENORMAL, (), "low"), ("thr.flt_min" + nm, f * FLT_MIN, (), "low"),
                  ("thr.flt_max" + nm, f * FLT_MAX, (), "candidate"), ("thr.inf" + nm, f * inf, (), "candidate"),
                  ("thr.inf_equal" + nm, f * inf, [(0, 0, 1, f * inf)], "none"),
                  ("thr.inf_equal_s" + nm, f * inf, [(1, 0, 0, f * inf)], "none"),
                  # a zero of one sign over 26 zeros of the other: all ties
                  ("thr.zero" + nm, f * np.float32(0), [d + (-f * np.float32(0),) for d in OFFSETS], "none")]
    spots = T.spots()
    for label, c, nb, exp in cases:
        pos = next(spots, None)
        if pos is not None:
            T.plant(label, *pos, centre=c, neighbours=nb, expected=exp)


def _dense(T):
    """A lattice of distinct peaks at odd x on two odd rows of octave 0, scale 1
    (31 bits per full word); on planes wider than 64 words, peaks in words 0,
    63, 64 and the last word of one row at two scales (k_emit's second chunk
    continues a non-zero base)."""
    h, w = T.dims[0]
    nw = (w + WORD - 1) // WORD
    n = 0
    if h >= 32 and w >= WORD:
        for y in (11, 13):
            for x in range(1, w - 1, 2):
                # written directly: the lattice is one block of footprints (rows 10..14, scales 0..2)
                T.planes[0][1, y, x] = T.t * np.float32(0.5 + (n % 40) / 16.0) * np.float32(1 + n * 2.0 ** -12)
                T.plants.append(("dense.lattice.%d.%d" % (y, x), 0, 1, y, x,
                                 "candidate" if T.planes[0][1, y, x] >= T.t else "low"))
                n += 1
        assert not T.taken[0][0:3, 10:15, :].any()
        T.taken[0][0:3, 10:15, :] = True
    if nw > 64:
        for j, s in enumerate(sorted({1, T.S})):
            for wd in sorted({0, 63, 64, nw - 1}):
                x = WORD * wd + 4 + 3 * j
                if T.fits(0, s, 2, x):
                    T.plant("dense.chunk.s%d.w%d" % (s, wd), 0, s, 2, x, centre=T.t * np.float32(2 + n / 16.0))
                    n += 1


_tables = {}


def build_table(geom, S):
    """The plant table of one geometry at S scales (cached; treat as read-only)."""
    if (geom, S) in _tables:
        return _tables[(geom, S)]
    T = Table(geom, S)
    _dense(T)
    _positions(T)
    _threshold(T)
    # the neighbour family: the constrained contexts in turn, from a start that depends on the table
    rot = (37 * TABLES.index((geom, S)) if (geom, S) in TABLES else 0) % len(COMBOS)
    live = context_spots(T)
    for j in range(len(COMBOS)):
        i = (rot + j) % len(COMBOS)
        for name in list(live):
            pos = next(live[name], None)
            if pos is None:
                del live[name]
            else:
                _neighbour_plant(T, name, i, pos)
    spots = T.spots()
    for j in range(len(COMBOS)):   # an interior position: whatever is left
        pos = next(spots, None)
        if pos is None:
            break
        _neighbour_plant(T, "interior", (rot + j) % len(COMBOS), pos)
    _tables[(geom, S)] = T
    return T


# ---------------------------------------------------------------------------
# Quantised noise on caller planes
# ---------------------------------------------------------------------------
class NoiseTable:
    def __init__(self, geom, S, seed):
        import oracle as orc
        self.geom, self.S, self.seed = geom, S, seed
        self.W, self.H, self.O = geom
        self.dims = orc.octave_dims(*geom)
        self.t = fp32_threshold(S)
        self.blocks = block_count(self.dims, S)
        rng = np.random.default_rng(seed)
        q = self.t / np.float32(16)   # exact: |k| = 16 is the threshold itself
        self.planes = [(rng.integers(-16, 17, size=(S + 2, h, w)).astype(np.float32) * q) for h, w in self.dims]

    def arrays(self):
        return np.concatenate([p.ravel() for p in self.planes])

    def lists(self, **wrong):
        return reference_lists(self.planes, self.dims, self.S, **wrong)


_noise = {}


def noise_table(geom, S, seed):
    if (geom, S, seed) not in _noise:
        _noise[(geom, S, seed)] = NoiseTable(geom, S, seed)
    return _noise[(geom, S, seed)]


# ---------------------------------------------------------------------------
# Built pyramids: small noise images whose extrema fall on every edge
# ---------------------------------------------------------------------------
EDGE_W, EDGE_H, EDGE_O = 91, 46, 2    # octave 0: 92 x 182
EDGE_COLUMNS = [1] + list(range(59, 65)) + list(range(119, 127)) + [179, 180]
EDGE_ROWS = [1, 30, 31, 60, 61, 90]
# default_rng seeds per S, chosen greedily on the CPU from seeds 1000..1199 (test_extrema_cases.py asserts that
# the oracle's extrema of these images, CONV_SEPARABLE_FMA_VH, hit every edge column, edge row and scale)
EDGE_SEEDS = {1: (1000, 1008, 1040, 1086, 1090), 2: (1024, 1094, 1104), 3: (1026, 1028), 4: (1003, 1094),
              5: (1001, 1048), 6: (1000, 1004), 7: (1019,), 8: (1003,), 9: (1019,)}


def edge_image(seed):
    return np.random.default_rng(seed).random((EDGE_H, EDGE_W), dtype=np.float32)


def edge_hits(r, S):
    """(columns, rows, scales) of the edge set that the oracle run's extrema of octave 0 hit."""
    rec = np.concatenate([r.cand_rec, r.low_rec])
    rec = rec[rec[:, 0] == 0]
    return (set(EDGE_COLUMNS) & set(rec[:, 2].tolist()), set(EDGE_ROWS) & set(rec[:, 3].tolist()),
            set(range(1, S + 1)) & set(rec[:, 1].tolist()))
