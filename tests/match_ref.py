"""numpy statement of the descriptor match and of the selection rule
(include/sift_hip.h).

Descriptors are rows of 128 uint8.  d2(q, t) = sum_k (Q[q][k] - T[t][k])^2.
For every unmasked query row: the two smallest (d2, t) over the unmasked train
rows in lexicographic order; a missing neighbour is (-1, NONE_D2).  d2 comes
from one float64 matrix product of the rows shifted by -128 (|q'|^2 + |t'|^2 -
2 q'.t'): every partial sum is an integer below 2^53, so the product is exact
whatever order BLAS adds in.
"""
import numpy as np

MATCH_DTYPE = np.dtype([("best", "<i4"), ("second", "<i4"), ("d2_best", "<i4"), ("d2_second", "<i4")])
PAIR_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("d2", "<i4"), ("d2_second", "<i4")])
NONE_D2 = 2**31 - 1
D2_MAX = 128 * 255 * 255


def d2_matrix(query, train):
    """int64 [n_query, n_train] squared distances."""
    q = np.asarray(query, dtype=np.float64) - 128.0
    t = np.asarray(train, dtype=np.float64) - 128.0
    d = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * (q @ t.T)
    return d.astype(np.int64)


def match_ref(query, train, query_mask=None, train_mask=None, block=1024):
    query = np.asarray(query, dtype=np.uint8).reshape(-1, 128)
    train = np.asarray(train, dtype=np.uint8).reshape(-1, 128)
    nq, nt = query.shape[0], train.shape[0]
    qm = np.ones(nq, bool) if query_mask is None else np.asarray(query_mask) != 0
    tm = np.ones(nt, bool) if train_mask is None else np.asarray(train_mask) != 0
    out = np.zeros(nq, dtype=MATCH_DTYPE)
    out["best"] = out["second"] = -1
    out["d2_best"] = out["d2_second"] = NONE_D2
    tidx = np.flatnonzero(tm)
    if nq == 0 or len(tidx) == 0:
        return out
    tt = train[tidx]
    for q0 in range(0, nq, block):
        d = d2_matrix(query[q0:q0 + block], tt)
        for i in range(d.shape[0]):
            if not qm[q0 + i]:
                continue
            row = d[i]
            if len(row) > 2:  # the candidates: everything at or below the second smallest distance
                cand = np.flatnonzero(row <= np.partition(row, 1)[1])
            else:
                cand = np.arange(len(row))
            order = cand[np.lexsort((tidx[cand], row[cand]))]  # by d2, then train index
            r = out[q0 + i]
            r["best"], r["d2_best"] = tidx[order[0]], row[order[0]]
            if len(order) > 1:
                r["second"], r["d2_second"] = tidx[order[1]], row[order[1]]
    return out


def match_loops(query, train, query_mask=None, train_mask=None):
    """The definition with Python ints and two loops (small cases)."""
    out = np.zeros(len(query), dtype=MATCH_DTYPE)
    for q in range(len(query)):
        pairs = []
        if query_mask is None or query_mask[q]:
            for t in range(len(train)):
                if train_mask is None or train_mask[t]:
                    pairs.append((sum((int(a) - int(b)) ** 2 for a, b in zip(query[q], train[t])), t))
        pairs = sorted(pairs)[:2] + [(NONE_D2, -1)] * 2
        out[q] = (pairs[0][1], pairs[1][1], pairs[0][0], pairs[1][0])
    return out


def merge_ref(parts, offsets):
    """Top-2 records of train pieces (piece p's indices offset by offsets[p]) merged by (d2, index)."""
    n = len(parts[0])
    d = np.concatenate([np.stack([p["d2_best"], p["d2_second"]], 1) for p in parts], 1).astype(np.int64)
    i = np.concatenate([np.stack([np.where(p["best"] >= 0, p["best"] + o, -1),
                                  np.where(p["second"] >= 0, p["second"] + o, -1)], 1)
                        for p, o in zip(parts, offsets)], 1).astype(np.int64)
    key = np.where(i >= 0, d * 2**32 + i, np.iinfo(np.int64).max)
    order = np.argsort(key, axis=1, kind="stable")[:, :2]
    rows = np.arange(n)[:, None]
    out = np.zeros(n, dtype=MATCH_DTYPE)
    out["best"], out["second"] = i[rows, order][:, 0], i[rows, order][:, 1]
    out["d2_best"], out["d2_second"] = d[rows, order][:, 0], d[rows, order][:, 1]
    return out


def select_ref(fwd, rev=None, ratio=0.8):
    """Accepted pairs in ascending query index.  Query q is accepted when
    best >= 0; and ratio <= 0, or second < 0, or float64(d2_best) < (ratio *
    ratio) * float64(d2_second); and rev is None or rev[best].best == q."""
    ok = fwd["best"] >= 0
    if ratio > 0:
        r2 = np.float64(ratio) * np.float64(ratio)
        ok &= (fwd["second"] < 0) | (fwd["d2_best"].astype(np.float64) < r2 * fwd["d2_second"].astype(np.float64))
    if rev is not None:
        q = np.arange(len(fwd))
        back = np.full(len(fwd), -2, dtype=np.int64)
        inside = ok & (fwd["best"] < len(rev))
        back[inside] = rev["best"][fwd["best"][inside]]
        ok &= back == q
    out = np.zeros(int(ok.sum()), dtype=PAIR_DTYPE)
    out["query"] = np.flatnonzero(ok)
    out["train"], out["d2"], out["d2_second"] = fwd["best"][ok], fwd["d2_best"][ok], fwd["d2_second"][ok]
    return out
