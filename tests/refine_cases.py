"""Inputs that put every decision of the refinement at its threshold, and a
restatement of one refinement chain that labels them (CPU, numpy only).

* refine_step / trace: one refinement chain on an fp64 DoG octave, in
  oracle_refine's operation order (np.float64 scalars: every operation is
  rounded once, nothing is contracted).  With `native=True` every step also
  carries the first-order error bounds the fast pass on fp32 planes computes
  (csrc/sift_refine.h): delta, Edet, Ea, Eo, the edge interval, the rounding
  margin and the output bound.  The C oracle stays the judge of results; the
  trace only labels and selects inputs, and the bounds are only used to show
  that an input lies inside one, never as an expected value
  (test_refine_cases.py holds the trace to oracle_refine).
* build_table: the decision table of test_gpu_refine_edges.py -- one
  caller-supplied DoG pyramid (64 x 64, two octaves) and one candidate list
  holding sweeps of consecutive fp32 plane values / fp64 candidate values
  across every threshold, rounding ties, moves onto every face of the
  refinable interior and move chains of one to five moves.

Two cases of the reference's decision list cannot be reached from finite
fp32 planes and are therefore not in the table:
* tr^2/det2 = NaN (det2 == 0 with tr == 0): tr == 0 means h33 == -h22, so
  det2 = -(h22^2 + h23^2) is zero only for h22 = h33 = h23 = 0 (fp32 inputs
  cannot underflow an fp64 square), and then rows 2 and 3 of the Hessian are
  multiples of (1, 0, 0): det == 0, the chain ends as singular before the
  edge test.
* alpha = +-inf: with |det| >= DBL_EPSILON and fp32 entries |H^-1| < 1e45
  and |g| < 3.5e38, far from fp64 overflow.  The table holds |alpha| = 1e30
  in every component and both signs, and an infinite neighbour in every
  direction (g = +-inf, which makes alpha NaN): all of them leave the
  interior.
Rounding ties: positions are positive, so a kernel that rounds half away
from zero agrees with the reference (ties toward +inf) on every reachable
input; the ties catch rounding to even, downwards and truncation.
The scale axis has S interior positions, so its chains are as long as they
fit: one and two moves at S = 3, one to four at S = 5, and at S = 6 the full
set -- one to four moves then keep, and five moves arriving on a keepable
bowl at s = 6, discarded by the move limit alone.  (At S = 5 the five-move
case is five moving positions whose last move would also leave through the
top, which a six-move limit would discard too; S = 6 is the one that tells.)
"""
import types

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
KP_TOL = 2e-5          # SIFT_KP_TOL
VALUE_TOL = 1e-7       # kValueTol
EDGE_THR = ((10 + 1) * (10 + 1)) / 10.0
ALPHA_MAX = 0.6
OUTCOMES = ("keep", "low_contrast", "edge", "moved_out", "five_moves", "singular")

F = np.float64


def contrast_threshold(S):
    return float(((F(2.0) ** F(1.0 / S) - 1) / (F(2.0) ** F(1.0 / 3) - 1)) * 0.015)


def js_round(v):
    f = np.floor(v)
    return f + 1.0 if v - f >= 0.5 else f


def round_margin(v):
    return abs((v - np.floor(v)) - 0.5)


def _to_index(v):
    """(int) of a rounded position; anything non-finite or huge is outside."""
    if not np.isfinite(v) or abs(v) > 2.0 ** 30:
        return -(2 ** 31)
    return int(v)


def refine_step(d, o, s, m, n, value, delta, dval, S, ND, h, w, thr, last, sig0):
    """One iteration on the 3x3x3 patch d[k][a][c] (scale s-1+k, row m-1+a,
    column n-1+c).  delta / dval > 0: the fp32-plane error bounds as well."""
    kSafe = 2.0
    d = np.asarray(d, dtype=F)
    R = types.SimpleNamespace(uncertain=False, why=0, imprecise=False, pos=(s, m, n), s=s, m=m, n=n,
                              omega=None, edgeness=None, alpha=None, bounds={}, margins={})
    with np.errstate(all="ignore"):
        cc = d[1, 1, 1]
        g0 = (d[2, 1, 1] - d[0, 1, 1]) / 2
        g1 = (d[1, 2, 1] - d[1, 0, 1]) / 2
        g2 = (d[1, 1, 2] - d[1, 1, 0]) / 2
        h11 = d[2, 1, 1] + d[0, 1, 1] - (2 * cc)
        h22 = d[1, 2, 1] + d[1, 0, 1] - (2 * cc)
        h33 = d[1, 1, 2] + d[1, 1, 0] - (2 * cc)
        h12 = (d[2, 2, 1] - d[2, 0, 1] - d[0, 2, 1] + d[0, 0, 1]) / 4
        h13 = (d[2, 1, 2] - d[2, 1, 0] - d[0, 1, 2] + d[0, 1, 0]) / 4
        h23 = (d[1, 2, 2] - d[1, 2, 0] - d[1, 0, 2] + d[1, 0, 0]) / 4
        M = [[h11, h12, h13], [h12, h22, h23], [h13, h23, h33]]
        mn = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                r0, r1 = (1 if i == 0 else 0), (1 if i == 2 else 2)
                c0, c1 = (1 if j == 0 else 0), (1 if j == 2 else 2)
                mn[i][j] = (M[r0][c0] * M[r1][c1]) - (M[r0][c1] * M[r1][c0])
        det = ((M[0][0] * mn[0][0]) - (M[0][1] * mn[0][1])) + (M[0][2] * mn[0][2])
        R.g, R.H, R.det = (g0, g1, g2), M, det
        dG, dH = delta, 4 * delta
        if delta > 0:
            cof1 = sum(abs(mn[i][j]) for i in range(3) for j in range(3))
            hmax = max(abs(M[i][j]) for i in range(3) for j in range(3))
            Edet = kSafe * (cof1 * dH + 9 * (2 * hmax + dH) * dH * dH) + 1e-300
            R.bounds["det"] = Edet
            R.margins["det"] = abs(abs(det) - DBL_EPSILON)
            if R.margins["det"] <= Edet:
                R.uncertain, R.why = True, R.why | 1
        if abs(det) < DBL_EPSILON:
            R.state = "singular"
            return R
        ninv = [[None] * 3 for _ in range(3)]
        inv_norm = F(0)
        for i in range(3):
            rs = F(0)
            for j in range(3):
                cof = mn[j][i] * -1.0 if ((i + j) & 1) else mn[j][i]
                ninv[i][j] = (cof / det) * -1
                rs = rs + abs(ninv[i][j])
            inv_norm = max(inv_norm, rs)
        gv = (g0, g1, g2)
        a = []
        for i in range(3):
            r = F(0)
            for j in range(3):
                r = r + ninv[i][j] * gv[j]
            a.append(r)
        R.alpha = tuple(a)
        a1 = abs(a[0]) + abs(a[1]) + abs(a[2])
        Ea = 0.0
        if delta > 0:
            kappa = inv_norm * 3 * dH
            if kappa >= 0.5:
                R.uncertain, R.why = True, R.why | 2
                Ea = 1e300
            else:
                Ea = kSafe * inv_norm * (dG + 3 * dH * a1) / (1 - kappa) + 1e-300
            R.bounds["alpha"] = Ea
            R.margins["alpha"] = min(abs(abs(x) - ALPHA_MAX) for x in a)
            if R.margins["alpha"] <= Ea:
                R.uncertain, R.why = True, R.why | 2
        if abs(a[0]) < ALPHA_MAX and abs(a[1]) < ALPHA_MAX and abs(a[2]) < ALPHA_MAX:
            omega = value + (((0.5 * a[0]) * g0) + ((0.5 * a[1]) * g1) + ((0.5 * a[2]) * g2))
            R.omega = omega
            if delta > 0:
                kappa = inv_norm * 3 * dH
                r = [dG + dH * abs(a[j]) + dG * (a1 - abs(a[j])) for j in range(3)]
                e = [kSafe * (abs(ninv[i][0]) * r[0] + abs(ninv[i][1]) * r[1] + abs(ninv[i][2]) * r[2]) / (1 - kappa)
                     for i in range(3)]
                dlt = 2.0 ** (o - 1)
                e_xy = dlt * max(e[1], e[2])
                e_sig = dlt * sig0 * 3.04 * (0.6931471805599453 / S) * e[0]
                e_val = kSafe * (dval + 0.5 * (e[0] * abs(g0) + e[1] * abs(g1) + e[2] * abs(g2) +
                                               (a1 + e[0] + e[1] + e[2]) * dG))
                R.bounds["out"] = max(e_xy, e_sig)
                R.bounds["out_value"] = e_val
                R.imprecise = bool(max(e_xy, e_sig) > KP_TOL or e_val > VALUE_TOL)
            if delta > 0 or dval > 0:
                Eo = kSafe * (dval + 0.5 * (Ea * (abs(g0) + abs(g1) + abs(g2)) + (a1 + 3 * Ea) * dG)) + 1e-300
                R.bounds["omega"] = Eo
                R.margins["omega"] = abs(abs(omega) - thr)
                if R.margins["omega"] <= Eo:
                    R.uncertain, R.why = True, R.why | 4
            if abs(omega) < thr:
                R.state = "low_contrast"
                return R
            tr = (0 + h22) + h33
            dt = (h22 * h33) - (h23 * h23)
            edgeness = (tr * tr) / dt
            R.tr, R.dt, R.edgeness = tr, dt, edgeness
            if delta > 0:
                Etr = kSafe * 2 * dH
                Edt = kSafe * ((abs(h22) + abs(h33)) * dH + 2 * abs(h23) * dG + dH * dH + dG * dG) + 1e-300
                if abs(dt) <= Edt:
                    R.uncertain, R.why = True, R.why | 8
                else:
                    t_hi, t_lo = abs(tr) + Etr, max(0.0, abs(tr) - Etr)
                    d_lo, d_hi = abs(dt) - Edt, abs(dt) + Edt
                    if dt > 0:
                        e_lo, e_hi = t_lo * t_lo / d_hi, t_hi * t_hi / d_lo
                    else:
                        e_lo, e_hi = -(t_hi * t_hi / d_lo), -(t_lo * t_lo / d_hi)
                    R.bounds["edge"] = (e_hi - e_lo) / 2   # half-width of the interval
                    R.bounds["edge_interval"] = (e_lo, e_hi)
                    R.margins["edge"] = abs(edgeness - EDGE_THR)
                    if e_lo <= EDGE_THR <= e_hi:
                        R.uncertain, R.why = True, R.why | 16
            if edgeness > EDGE_THR:
                R.state = "edge"
                return R
            R.state = "keep"
            return R
        if last:
            R.state = "five_moves"
            return R
        vs, vm, vn = s + a[0], m + a[1], n + a[2]
        if delta > 0:
            R.bounds["round"] = Ea
            R.margins["round"] = min(round_margin(vs), round_margin(vm), round_margin(vn))
            if round_margin(vs) <= Ea or round_margin(vm) <= Ea or round_margin(vn) <= Ea:
                out_s = js_round(vs + Ea) < 1 or js_round(vs - Ea) >= ND - 1
                out_m = js_round(vm + Ea) < 1 or js_round(vm - Ea) >= h - 1
                out_n = js_round(vn + Ea) < 1 or js_round(vn - Ea) >= w - 1
                if not (out_s or out_m or out_n):
                    R.uncertain, R.why = True, R.why | 32
        R.s, R.m, R.n = _to_index(js_round(vs)), _to_index(js_round(vm)), _to_index(js_round(vn))
        if R.s < 1 or R.s >= ND - 1 or R.m < 1 or R.m >= h - 1 or R.n < 1 or R.n >= w - 1:
            R.state = "moved_out"
            return R
        R.state = "moved"
        return R


def trace(D, o, s, y, x, value, S, min_blur=0.8, mid=0.5, native=False):
    """The chain of candidate (o, s, x, y) with `value` on the octave's DoG
    planes D (ND, h, w) fp64.  Returns a namespace: steps (refine_step results,
    one per iteration), outcome (one of OUTCOMES), moves, and for a kept
    keypoint `kept`: the oracle's 8-tuple [o, s, x, y, sigma, X, Y, omega].
    native: the fast pass's bounds on fp32-rounded planes at every step."""
    ND, h, w = D.shape
    thr = contrast_threshold(S)
    value = F(value)
    dval = abs(value) * 2.0 ** -24 if native else 0.0
    steps = []
    T = types.SimpleNamespace(steps=steps, outcome=None, kept=None, origin=(o, s, x, y))
    for it in range(5):
        d = np.array(D[s - 1:s + 2, y - 1:y + 2, x - 1:x + 2], dtype=F)
        delta = 0.0
        if native:
            used = [abs(d[k, a, c]) for k in range(3) for a in range(3) for c in range(3)
                    if not (k != 1 and a != 1 and c != 1)]
            delta = max(used) * (2.0 ** -24 + 2.0 ** -40)
        R = refine_step(d, o, s, y, x, value, delta, dval, S, ND, h, w, thr, it == 4, min_blur / mid)
        R.delta = delta
        steps.append(R)
        if R.state != "moved":
            T.outcome = R.state
            break
        s, y, x = R.s, R.m, R.n
    else:
        T.outcome = "five_moves"  # the fifth move landed inside: the reference's loop ends
    T.moves = len(steps) - 1 if T.outcome in ("keep", "low_contrast", "edge", "singular") else len(steps)
    if T.outcome == "keep":
        R = steps[-1]
        with np.errstate(all="ignore"):
            dl = F(2.0) ** (o - 1)
            Y = dl * (R.alpha[1] + R.m)
            X = dl * (R.alpha[2] + R.n)
            sig = (dl / mid) * min_blur * F(2.0) ** ((R.alpha[0] + R.s) / S)
        T.kept = (o, R.s, R.n, R.m, float(sig), float(X), float(Y), float(R.omega))
    T.uncertain = any(R.uncertain for R in steps)
    T.polish = (not T.uncertain) and T.outcome == "keep" and steps[-1].imprecise
    return T


def trace_list(dog, dims, rec, val, S, native=False, **kw):
    """trace() of every candidate of an oracle list on the octave planes `dog`
    (oracle.split_pyramid).  Returns the traces, the kept (M, 8) array in
    list order and the singular count -- what oracle_refine returns."""
    tr = [trace(dog[int(r[0])], int(r[0]), int(r[1]), int(r[3]), int(r[2]), v, S, native=native, **kw)
          for r, v in zip(rec, val)]
    kept = np.array([t.kept for t in tr if t.outcome == "keep"], dtype=np.float64).reshape(-1, 8)
    return tr, kept, sum(t.outcome == "singular" for t in tr)


# ---------------------------------------------------------------------------
# The decision table on caller-supplied planes
# ---------------------------------------------------------------------------
TABLE_W = TABLE_H = 64
TABLE_O = 2
SWEEP_LEN = 64


def f32_step(v, k):
    """The fp32 value k representable steps above v (ordered by value)."""
    i = int(np.float32(v).view(np.int32))
    i = i if i >= 0 else -(i & 0x7fffffff)
    i += k
    i = i if i >= 0 else (-i) | 0x80000000
    return np.uint32(i & 0xffffffff).view(np.float32)


def f64_step(v, k):
    i = int(np.float64(v).view(np.int64))
    i = i if i >= 0 else -(i & 0x7fffffffffffffff)
    i += k
    i = i if i >= 0 else (-i) | 0x8000000000000000
    return np.uint64(i & 0xffffffffffffffff).view(np.float64)


def _bisect(pred, step, lo, n_max):
    """Smallest k in (0, n_max] with pred(step(lo, k)) != pred(lo)."""
    p0 = pred(step(lo, 0))
    a, b = 0, n_max
    assert pred(step(lo, b)) != p0, "the bracket holds no flip"
    while b - a > 1:
        c = (a + b) // 2
        if pred(step(lo, c)) == p0:
            a = c
        else:
            b = c
    return b


class Table:
    """One pyramid and one candidate list.  planes[o]: (ND, h, w) float32."""

    def __init__(self, S):
        import oracle as orc
        self.S, self.ND = S, S + 2
        self.dims = orc.octave_dims(TABLE_W, TABLE_H, TABLE_O)
        self.planes = [np.zeros((self.ND, h, w), dtype=np.float32) for h, w in self.dims]
        self.written = [np.zeros((self.ND, h, w), dtype=bool) for h, w in self.dims]
        self.rec, self.val = [], []
        self.cases = {}     # name -> list of candidate indices
        self.sweeps = {}    # name -> (indices, probe): probe(trace) -> bool, both values must occur
        self.expect = {}    # name -> expected outcome(s) of single cases, by the builder's intent

    def put(self, o, s, y, x, v):
        v = np.float32(v)
        if self.written[o][s, y, x]:
            old = self.planes[o][s, y, x]
            assert old == v or (np.isnan(old) and np.isnan(v)), ("conflicting writes", o, s, y, x, old, v)
        self.planes[o][s, y, x] = v
        self.written[o][s, y, x] = True

    def patch(self, o, s, y, x, cc=0.0, g=(0, 0, 0), hd=(-1, -1, -1), h12=0.0, h13=0.0, h23=0.0):
        """The entries that give gradient g and Hessian (hd, h12, h13, h23) at (s, y, x)."""
        self.put(o, s, y, x, cc)
        for ax, (ds, dy, dx) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            self.put(o, s + ds, y + dy, x + dx, cc + hd[ax] / 2.0 + g[ax])
            self.put(o, s - ds, y - dy, x - dx, cc + hd[ax] / 2.0 - g[ax])
        if h12:
            self.put(o, s + 1, y + 1, x, 4.0 * h12)
        if h13:
            self.put(o, s + 1, y, x + 1, 4.0 * h13)
        if h23:
            self.put(o, s, y + 1, x + 1, 4.0 * h23)

    def bowl(self, o, s, y, x, f):
        """A keepable peak: centre f + 1, its six neighbours f (H = -2 I, g = 0)."""
        self.put(o, s, y, x, f + 1.0)
        for ds, dy, dx in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            self.put(o, s + ds, y + dy, x + dx, f)
            self.put(o, s - ds, y - dy, x - dx, f)

    def cand(self, name, o, s, y, x, value):
        self.cases.setdefault(name, []).append(len(self.rec))
        self.rec.append((o, s, x, y))
        self.val.append(float(value))
        return len(self.rec) - 1

    def trace(self, i):
        o, s, x, y = self.rec[i]
        return trace(self.planes[o].astype(np.float64), o, s, y, x, self.val[i], self.S)

    def arrays(self):
        flat = np.concatenate([p.ravel() for p in self.planes])
        return flat, np.array(self.rec, dtype=np.int32).reshape(-1, 4), np.array(self.val, dtype=np.float64)


def _probe_trace(T, o, s, y, x, value):
    return trace(T.planes[o].astype(np.float64), o, s, y, x, value, T.S)


def _entry_sweep(T, name, sites, o, s, entry, lo, n_max, probe, value, setup):
    """SWEEP_LEN patches (one per site, built by setup(y, x)) that differ in
    one entry: consecutive fp32 values around the one where probe flips."""
    y0, x0 = sites[0]
    setup(y0, x0)
    es, ey, ex = s + entry[0], y0 + entry[1], x0 + entry[2]

    def pred(v):
        T.planes[o][es, ey, ex] = v
        return probe(_probe_trace(T, o, s, y0, x0, value))

    k = _bisect(pred, f32_step, np.float32(lo), n_max)
    idx = []
    for j, (y, x) in enumerate(sites):
        if j:
            setup(y, x)
        T.planes[o][s + entry[0], y + entry[1], x + entry[2]] = f32_step(np.float32(lo), k - SWEEP_LEN // 2 + j)
        idx.append(T.cand(name, o, s, y, x, value))
    T.sweeps[name] = (idx, probe)


def build_table(S):
    """The table at S scales per octave (S = 3: ND = 5; S = 5 and 6 move thr;
    S = 6 gives the scale axis room for five moves onto a bowl)."""
    T = Table(S)
    w0 = T.dims[0][1]
    # --- sweeps of one patch entry: sites on a 4-pixel pitch in octave 0, at s = 2
    sites = [(y, x) for y in range(4, 84, 4) for x in range(4, w0 - 3, 4)]
    nxt = iter(range(0, len(sites), SWEEP_LEN))

    def take():
        b = next(nxt)
        return sites[b:b + SWEEP_LEN]

    axes = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    for ax in range(3):
        for sign in (+1, -1):
            g = [0.0, 0.0, 0.0]
            g[ax] = sign * 0.59
            # H = -I, alpha = g: raising the entry on the +axis side raises g and lowers |h| -> alpha grows
            ent = tuple(sign * c for c in axes[ax])
            _entry_sweep(T, "alpha%d%s" % (ax, "+" if sign > 0 else "-"), take(), 0, 2, ent,
                         -0.5 + 0.59, 1 << 22,
                         lambda t, ax=ax: bool(abs(t.steps[0].alpha[ax]) < 0.6), 1.0,
                         lambda y, x, g=tuple(g): T.patch(0, 2, y, x, g=g))
    # edgeness across 12.1: h22 = -1, h33 = -10 gives exactly 121/10; raise one row neighbour
    _entry_sweep(T, "edge", take(), 0, 2, (0, 1, 0), -0.5 - 0.001, 1 << 20,
                 lambda t: bool(t.steps[0].edgeness > EDGE_THR), 1.0,
                 lambda y, x: T.patch(0, 2, y, x, hd=(-1, -1, -10)))
    # |det| across DBL_EPSILON, both signs: H = -+ h I with h^3 near 2.22e-16
    hh = DBL_EPSILON ** (1.0 / 3)
    for sign, nm in ((-1, "det-"), (+1, "det+")):
        lo = sign * hh / 2 * (0.97 if sign > 0 else 1.03)
        _entry_sweep(T, nm, take(), 0, 2, (1, 0, 0), lo, 1 << 22,
                     lambda t: t.steps[0].state == "singular", 1.0,
                     lambda y, x, sign=sign: T.patch(0, 2, y, x, hd=(sign * hh,) * 3))
    # --- single cases in octave 1 (64 x 64), every one in a region of its own
    _singles(T)
    # --- |omega| across thr by the candidate's value (consecutive fp64 values on one patch): the rest of the
    # list, which brings it to 2100 candidates = 9 blocks of 256 (more than 8, and a remainder modulo 8)
    o, s, y, x = 0, 2, 96, 16
    T.patch(o, s, y, x, g=(0, 0.25, 0))
    thr = contrast_threshold(S)
    lo = f64_step(thr - 0.5 * 0.25 * 0.25, -4096)
    k = _bisect(lambda v: _probe_trace(T, o, s, y, x, v).outcome == "keep", f64_step, lo, 8192)
    n_om = TABLE_N - len(T.rec)
    assert n_om >= 2 * SWEEP_LEN
    idx = [T.cand("omega", o, s, y, x, f64_step(lo, k - n_om // 2 + j)) for j in range(n_om)]
    T.sweeps["omega"] = (idx, lambda t: bool(abs(t.steps[-1].omega) < thr))
    return T


TABLE_N = 2100


def _at(p, ax, k):
    q = list(p)
    q[ax] += k
    return q


def _move_case(T, name, p, ax, gi, land, want):
    """H = -I and g = gi along ax at p (octave 1): alpha = gi exactly, the
    reference lands `land` pixels along; a keepable bowl there if want == keep."""
    g = [0.0, 0.0, 0.0]
    g[ax] = gi
    T.patch(1, p[0], p[1], p[2], g=tuple(g))
    if want == "keep":
        q = _at(p, ax, land)
        W, P = T.written[1], T.planes[1]
        near = _at(q, ax, -1 if land > 0 else 1)
        if W[tuple(q)]:
            f = float(P[tuple(q)]) - 1.0
        elif W[tuple(near)]:
            f = float(P[tuple(near)])
        else:
            f = 0.0
        T.bowl(1, q[0], q[1], q[2], f)
    T.expect[name] = want
    T.cand(name, 1, p[0], p[1], p[2], 1.0)


def _chain(T, name, p, ax, moves, c, value, want, bowl=True):
    """D = c 3^-j along ax from p (octave 1): alpha = +1 along ax at `moves`
    positions, then a keepable bowl (centre vc = c 3^-(moves+1), curvature
    4 vc in every direction).  bowl=False: the line just continues (the last
    move leaves the interior)."""
    line = [tuple(_at(p, ax, j)) for j in range(moves + 1)]
    vc = c * 3.0 ** -(moves + 1)
    a = 2.0 * vc
    b = _at(p, ax, -1)
    T.put(1, b[0], b[1], b[2], c)
    for j, q in enumerate(line):
        v = c * 3.0 ** -(j + 1)
        T.put(1, q[0], q[1], q[2], v)
        if j == moves and not bowl:
            break
        for k in range(3):
            for sgn in (-1, 1):
                b = _at(q, k, sgn)
                if k == ax and (sgn < 0 or j < moves):
                    continue  # on the line
                T.put(1, b[0], b[1], b[2], 3.0 * vc if k == ax else v + a)
    T.expect[name] = want
    T.cand(name, 1, p[0], p[1], p[2], value)


def _singles(T):
    S, ND = T.S, T.ND
    h1, w1 = T.dims[1]
    thr = contrast_threshold(S)
    # move chains of 1..4 moves then keep (the record carries the final position), 5 moves discard
    for k in range(1, 6):
        want = "keep" if k < 5 else "five_moves"
        _chain(T, "chain_x%d" % k, [2, 6 * k, 8], 2, k, 9.0, 1.0, want)
        _chain(T, "chain_y%d" % k, [2, 8, 24 + 6 * k], 1, k, 9.0, 1.0, want)
        if k <= S - 1:
            _chain(T, "chain_s%d" % k, [1, 40, 2 + 6 * k], 0, k, 9.0, 1.0, want)
    if S == 5:  # five interior positions only: five movers, the fifth move would leave through the top
        _chain(T, "chain_s5", [1, 40, 32], 0, 5, 9.0, 1.0, "five_moves", bowl=False)
    # omega uses the candidate's value after a move: the landing pixel holds a third of the start's
    _chain(T, "omega_origin_keep", [2, 36, 44], 2, 1, 0.06, 0.02, "keep")       # 0.02 >= thr > 0.0067
    _chain(T, "omega_origin_low", [2, 36, 54], 2, 1, 0.3, 0.9 * thr, "low_contrast")  # landing 0.033 >= thr
    # det2 < 0 keeps (negative edgeness passes); det2 == 0 with tr != 0 discards (+inf)
    T.patch(1, 2, 46, 8, hd=(-1, -1, 1))
    T.expect["edge_negative"] = "keep"
    T.cand("edge_negative", 1, 2, 46, 8, 1.0)
    T.patch(1, 2, 46, 14, hd=(-1, -1, -1), h12=1.0, h23=1.0)
    T.expect["edge_inf"] = "edge"
    T.cand("edge_inf", 1, 2, 46, 14, 1.0)
    # rounding ties go toward +inf: alpha = +1.5 -> +2, -1.5 -> -1, +2.5 -> +3
    col = iter(range(20, 60, 4))
    for ax in range(3):
        for gi, land in ((1.5, 2), (-1.5, -1), (2.5, 3)):
            s0 = 2 if ax else (1 if gi > 0 else 3)
            if ax == 0 and s0 + land > ND - 2:
                continue  # no room on the scale axis at this S
            p = [s0, 50, next(col)] if ax != 2 else [2, {1.5: 30, -1.5: 34, 2.5: 44}[gi], 58]
            _move_case(T, "tie%d_%+.1f" % (ax, gi), p, ax, gi, land, "keep")
    # faces of the interior: onto the last interior index (continues, keeps), index 0 and the last index
    for ax, last, spots in ((0, ND - 1, ([0, 56, 8], [0, 56, 14], [0, 56, 20])),
                            (1, h1 - 1, ([2, 0, 26], [2, 0, 30], [2, 0, 34])),
                            (2, w1 - 1, ([2, 16, 0], [2, 20, 0], [2, 24, 0]))):
        for (nm, start, gi, want), p in zip((("inner", last - 3, 2.0, "keep"), ("first", 2, -2.0, "moved_out"),
                                             ("last", last - 2, 2.0, "moved_out")), spots):
            p = list(p)
            p[ax] = start
            _move_case(T, "face%d_%s" % (ax, nm), p, ax, gi, 2 if gi > 0 else -2, want)
    # |alpha| = 1e30 and an infinite neighbour, every component and sign: they leave the interior, no fault
    col = iter(range(20, 64, 3))
    for ax in range(3):
        for sign in (1, -1):
            x = next(col)
            g, hd = [0.0, 0.0, 0.0], [-1e3, -1e3, -1e3]
            g[ax], hd[ax] = sign * 1e18, 0.0
            T.patch(1, 2, 44, x, cc=5e-13, g=tuple(g), hd=tuple(hd))
            T.expect["huge%d%+d" % (ax, sign)] = "moved_out"
            T.cand("huge%d%+d" % (ax, sign), 1, 2, 44, x, 1.0)
    col = iter(range(38, 64, 4))
    for ax in range(3):
        for sign in (1, -1):
            x = next(col)
            T.patch(1, 2, 56, x)
            b = _at([2, 56, x], ax, 1)
            T.written[1][tuple(b)] = False
            T.put(1, b[0], b[1], b[2], sign * np.inf)
            T.expect["inf%d%+d" % (ax, sign)] = "moved_out"
            T.cand("inf%d%+d" % (ax, sign), 1, 2, 56, x, 1.0)


# ---------------------------------------------------------------------------
# Native planes steered onto the bounds (tests/golden/refine_steered.npz):
# what the generator accepts and test_refine_cases.py re-checks
# ---------------------------------------------------------------------------
N_STEERED = 25   # images in tests/golden/refine_steered.npz (test_refine_cases.py holds it to the file)


def oracle_run(img, O, S, mode=1):
    """OracleRun of img (mode 1: CONV_SEPARABLE, 2: CONV_SEPARABLE_FMA_VH)."""
    import oracle as orc
    return orc.OracleRun(img, orc.make_params(O, S), mode)


def target_trace(r, S, tgt):
    """Native trace of candidate tgt = (o, s, x, y), or None if it is no candidate."""
    hit = np.nonzero((r.cand_rec == np.array(tgt, dtype=np.int32)).all(axis=1))[0]
    if hit.size == 0:
        return None
    o, s, x, y = tgt
    return trace(r.dog[o], o, s, y, x, r.cand_val[hit[0]], S, native=True)


def final_result(r, S, tgt):
    """What candidate tgt leaves in the keypoint list: its kept (o, s, x, y), or None."""
    t = target_trace(r, S, tgt)
    return None if t is None or t.kept is None else tuple(t.kept[:4])


def decision_margin(r, S, tgt, kind):
    """(signed distance from the threshold, mirrored bound, threshold, why bits
    of the chain up to and including the targeted step) of the target's decision."""
    thr = contrast_threshold(S)
    o, s, x, y = tgt
    if kind == "pixthr":
        v = abs(float(r.dog[o][s, y, x]))
        pt = 0.8 * thr
        ulp = float(np.spacing(np.float32(pt)))
        ext = ((r.cand_rec == np.array(tgt, dtype=np.int32)).all(axis=1).any() or
               (r.low_rec == np.array(tgt, dtype=np.int32)).all(axis=1).any())
        return (v - pt, ulp / 2, pt, 0) if ext else None
    t = target_trace(r, S, tgt)
    if t is None:
        return None
    why = 0
    for st in t.steps:
        if kind == "omega" and st.omega is not None:
            return float(abs(st.omega) - thr), float(st.bounds["omega"]), thr, why | (st.why & 3)
        if kind == "edge" and st.edgeness is not None and "edge" in st.bounds:
            return float(st.edgeness - EDGE_THR), float(st.bounds["edge"]), EDGE_THR, why | (st.why & 15)
        if kind == "alpha" and st is t.steps[0] and st.alpha is not None:
            m = max(abs(a) for a in st.alpha)
            return float(m - 0.6), float(st.bounds["alpha"]), 0.6, st.why & 1
        if kind == "round" and st is t.steps[0] and st.state == "moved":
            v = [p + a for p, a in zip((st.pos[0], st.pos[1], st.pos[2]), st.alpha)]
            k = int(np.argmin([round_margin(c) for c in v]))
            lim = r.dog[o].shape[k]   # both roundings must stay inside the interior
            ea = float(st.bounds["round"])
            if not (1 <= js_round(v[k] - ea) and js_round(v[k] + ea) < lim - 1):
                return None
            return float((v[k] - np.floor(v[k])) - 0.5), float(st.bounds["round"]), 0.5, st.why & 3
        why |= st.why
    return None


def same_lists(img, O, S):
    a, b = oracle_run(img, O, S, 1), oracle_run(img, O, S, 2)
    return (np.array_equal(a.cand_rec, b.cand_rec) and np.array_equal(a.low_rec, b.low_rec) and
            np.array_equal(a.refined[:, :4], b.refined[:, :4]))


def accept(img, O, S, tgt, kind):
    """The three acceptance conditions; returns (margin, bound) or None."""
    d = decision_margin(oracle_run(img, O, S), S, tgt, kind)
    if d is None:
        return None
    q, bound, thr, why = d
    if why:   # an earlier decision of the chain is inside its own bound: it would fire first
        return None
    if not (abs(q) <= bound / 2 and abs(q) >= 1e-12 * thr):
        return None
    if not same_lists(img, O, S):
        return None
    return q, bound
