"""Brute-force descriptor matching on the device (sift_match*, DESIGN.md
section 12) against its numpy definition (tests/match_ref.py).

The arithmetic is integer, so every comparison is array equality of all four
fields; there is nothing to tolerate.  Shapes are the smallest that reach each
way the kernel can go wrong: one and two rows, the 32-row fragment and 256-row
chunk edges, more than one 512-query block, and train sets long enough to be
split over blocks and merged.
"""
import ctypes

import numpy as np
import pytest

import match_ref as mr
import sift_amd
from sift_amd.synth import blob_image

pytestmark = pytest.mark.gpu

NONE = (-1, -1, mr.NONE_D2, mr.NONE_D2)
_big = {}


def assert_same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for f in got.dtype.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)


def random_rows(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 128), dtype=np.uint8)


def big(ctx):
    """Case 6's data, its GPU matches both ways and their references, once.
    Uniform random rows; every second query is a random train row plus noise
    of a few levels, so that the ratio test and the mutual check of case 7
    accept some pairs and reject others."""
    if not _big:
        rng = np.random.default_rng(60)
        train = rng.integers(0, 256, (12000, 128), dtype=np.uint8)
        query = rng.integers(0, 256, (5000, 128), dtype=np.uint8)
        src = rng.integers(0, 12000, 2500)
        noise = rng.integers(-40, 41, (2500, 128))
        query[::2] = np.clip(train[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        _big.update(query=query, train=train, fwd=ctx.match(query, train), rev=ctx.match(train, query),
                    ref_fwd=mr.match_ref(query, train), ref_rev=mr.match_ref(train, query))
        for a in _big.values():
            a.setflags(write=False)
    return _big


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (2, 1), (31, 33), (33, 31), (64, 257), (65, 1023)])
def test_tile_edges(gpu_ctx, nq, nt):
    query, train = random_rows(100 + nq, nq), random_rows(200 + nt, nt)
    assert_same(gpu_ctx.match(query, train), mr.match_ref(query, train))


def test_k_order_and_every_k_step(gpu_ctx):
    train = np.zeros((128, 128), np.uint8)
    train[np.arange(128), np.arange(128)] = 200
    perm = (5 * np.arange(128) + 3) % 128
    query = np.zeros((128, 128), np.uint8)
    query[np.arange(128), perm] = 200
    got = gpu_ctx.match(query, train)
    np.testing.assert_array_equal(got["best"], perm)
    np.testing.assert_array_equal(got["d2_best"], 0)
    np.testing.assert_array_equal(got["second"], np.where(perm == 0, 1, 0))
    np.testing.assert_array_equal(got["d2_second"], 80000)
    assert_same(got, mr.match_ref(query, train))


def test_sign_and_range(gpu_ctx):
    alt = np.tile(np.array([0, 255], np.uint8), 64)
    rows = np.stack([np.full(128, v, np.uint8) for v in (0, 255, 127, 128)] + [alt, alt[::-1]])
    got = gpu_ctx.match(rows, rows[::-1].copy())
    assert_same(got, mr.match_ref(rows, rows[::-1].copy()))
    far = gpu_ctx.match(rows[0:1], rows[1:2])          # all 0 against all 255
    assert tuple(far[0]) == (0, -1, 8323200, mr.NONE_D2)
    near = gpu_ctx.match(rows[2:3], rows[3:4])         # 127 against 128: a wrong ^ 0x80 gives 128 * 255^2
    assert tuple(near[0]) == (0, -1, 128, mr.NONE_D2)
    both = gpu_ctx.match(rows[4:5], rows[[5, 4]])      # alternating against its reverse, then itself
    assert tuple(both[0]) == (1, 0, 0, 8323200)


def test_ties_take_the_lowest_indices_across_the_split(gpu_ctx):
    base = random_rows(4, 1000)
    train = np.concatenate([base, base, base])         # copies at i, i + 1000, i + 2000
    got = gpu_ctx.match(base, train)
    np.testing.assert_array_equal(got["best"], np.arange(1000))
    np.testing.assert_array_equal(got["second"], np.arange(1000) + 1000)
    np.testing.assert_array_equal(got["d2_best"], 0)
    np.testing.assert_array_equal(got["d2_second"], 0)
    back = gpu_ctx.match(base[::-1].copy(), train[::-1].copy())   # the copies in the other order
    np.testing.assert_array_equal(back["best"], np.arange(1000))
    np.testing.assert_array_equal(back["second"], np.arange(1000) + 1000)


def test_masks(gpu_ctx):
    rng = np.random.default_rng(7)
    train = random_rows(8, 700)
    zero_rows = np.arange(0, 700, 7)
    train[zero_rows] = 0
    tm = np.ones(700, np.uint8)
    tm[zero_rows] = 0                                   # the rows that would otherwise win
    query = rng.integers(0, 4, (70, 128), dtype=np.uint8)
    qm = np.ones(70, np.uint8)
    qm[[0, 13, 31, 32, 69]] = 0
    unmasked = gpu_ctx.match(query, train)
    assert np.isin(unmasked["best"], zero_rows).all()
    got = gpu_ctx.match(query, train, qm, tm)
    assert_same(got, mr.match_ref(query, train, qm, tm))
    assert not np.isin(got["best"], zero_rows).any()
    for q in (0, 13, 31, 32, 69):
        assert tuple(got[q]) == NONE
    one = np.zeros(700, np.uint8)
    one[333] = 1
    got = gpu_ctx.match(query, train, None, one)
    assert (got["best"] == 333).all() and (got["second"] == -1).all() and (got["d2_second"] == mr.NONE_D2).all()
    assert_same(got, mr.match_ref(query, train, None, one))
    got = gpu_ctx.match(query, train, None, np.zeros(700, np.uint8))
    assert all(tuple(r) == NONE for r in got)
    got = gpu_ctx.match(query, train[:0])
    assert len(got) == 70 and all(tuple(r) == NONE for r in got)
    assert len(gpu_ctx.match(query[:0], train)) == 0
    assert len(gpu_ctx.match(query[:0], train[:0])) == 0


def test_split_and_merge(gpu_ctx):
    b = big(gpu_ctx)
    assert_same(b["fwd"], b["ref_fwd"])
    assert_same(b["rev"], b["ref_rev"])
    cuts = (0, 3000, 7777, 12000)
    parts = [gpu_ctx.match(b["query"], b["train"][lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
    assert_same(mr.merge_ref(parts, cuts[:-1]), b["fwd"])


def split(nq, nt):
    """(query blocks, chunks per split, splits) of match_split (csrc/sift_kernels.h), restated so that the two
    cases below fail loudly, not vacuously, if the rule changes under them."""
    blocks, chunks = -(-nq // 512), -(-nt // 256)
    want = min(chunks, -(-1024 // blocks))
    per = -(-chunks // want)
    return blocks, per, -(-chunks // per)


def test_two_chunks_per_block_with_ties_and_a_mask_across_the_chunk_edge(gpu_ctx):
    """A block walks two chunks: the per-chunk key reset, and the fold into a top-2 that already holds the first
    chunk's entries.  Split s owns rows [512 s, 512 s + 512); its chunk edge is at 512 s + 256."""
    nq, nt = 5000, 30000
    assert split(nq, nt) == (10, 2, 59)
    rng = np.random.default_rng(61)
    train = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    query = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    tm = (rng.integers(0, 16, nt) != 0).astype(np.uint8)
    expect = {}
    for j, s in enumerate((0, 3, 29, 58)):               # a pair on either side of the edge inside one split
        e = 512 * s + 256
        train[e] = train[e - 1]
        tm[[e - 1, e]] = 1
        query[40 * j + 1] = train[e]
        expect[40 * j + 1] = (e - 1, e, 0, 0)
    for j, s in enumerate((1, 17, 40)):                  # the copy at the edge masked: the next one counts
        e = 512 * s + 256
        train[e] = train[e + 1] = train[e - 1]
        tm[[e - 1, e, e + 1]] = 1, 0, 1
        query[40 * j + 7] = train[e]
        expect[40 * j + 7] = (e - 1, e + 1, 0, 0)
    for j, s in enumerate((5, 33)):                      # first chunk, second chunk, and the next split
        a, b, c = 512 * s + 100, 512 * s + 300, 512 * (s + 1) + 5
        train[b] = train[c] = train[a]
        tm[[a, b, c]] = 1
        query[40 * j + 13] = train[c]
        expect[40 * j + 13] = (a, b, 0, 0)
    got = gpu_ctx.match(query, train, None, tm)
    for q, want in expect.items():
        assert tuple(got[q]) == want, q
    assert_same(got, mr.match_ref(query, train, None, tm))


def test_one_split_of_several_chunks_writes_the_result_directly(gpu_ctx):
    """What every large query set takes: at least 1024 query blocks, so one split walks every chunk and writes the
    result without a merge.  The queries repeat 1000 distinct rows, so the reference is that of the distinct
    rows, looked up."""
    nq, nt = 1024 * 512 - 100, 700
    assert split(nq, nt) == (1024, 3, 1)
    rng = np.random.default_rng(62)
    distinct = rng.integers(0, 256, (1000, 128), dtype=np.uint8)
    train = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    tm = np.ones(nt, np.uint8)
    train[255] = train[256] = distinct[3]                # ties across the first chunk edge
    train[511] = train[512] = train[699] = distinct[5]   # across the second, and a third copy in the tail
    train[100] = train[600] = distinct[9]                # first and last chunk
    train[300] = train[650] = distinct[11]               # the earlier copy masked
    tm[300] = 0
    tm[rng.integers(0, nt, 40)] = 0
    tm[[255, 256, 511, 512, 699, 100, 600, 650]] = 1
    idx = (7 * np.arange(nq) + 3) % 1000
    qm = np.ones(nq, np.uint8)
    qm[::997] = 0
    ref = mr.match_ref(distinct, train, None, tm)
    assert tuple(ref[3]) == (255, 256, 0, 0) and tuple(ref[5]) == (511, 512, 0, 0)
    assert tuple(ref[9]) == (100, 600, 0, 0) and ref[11]["best"] == 650 and ref[11]["d2_second"] > 0
    want = ref[idx]
    want[qm == 0] = NONE
    assert_same(gpu_ctx.match(distinct[idx], train, qm, tm), want)


@pytest.mark.parametrize("ratio", [0.0, 0.8])
@pytest.mark.parametrize("mutual", [False, True])
def test_selection(gpu_ctx, ratio, mutual):
    b = big(gpu_ctx)
    rev = b["rev"] if mutual else None
    want = mr.select_ref(b["ref_fwd"], b["ref_rev"] if mutual else None, ratio)
    got = gpu_ctx.select_matches(b["fwd"], rev, ratio)
    assert 0 < len(want) < len(b["fwd"]) or ratio == 0.0 and not mutual
    assert_same(got, want)
    assert (np.diff(got["query"]) > 0).all()


@pytest.mark.parametrize("ratio", [1.0, 1.5, float("nan"), float("inf")])
def test_selection_rejects_a_bad_ratio(gpu_ctx, ratio):
    b = big(gpu_ctx)
    with pytest.raises(sift_amd.SiftError) as e:
        gpu_ctx.select_matches(b["fwd"], None, ratio)
    assert e.value.code == sift_amd.SIFT_E_ARG


def test_device_forms_equal_the_host_forms(gpu_ctx):
    import torch
    b = big(gpu_ctx)
    L, h = sift_amd.lib(), gpu_ctx._h
    query, train = b["query"][:65], b["train"][:1023]
    qm = (np.arange(65) % 5 != 0).astype(np.uint8)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (query, qm, train)]
    d_out = torch.zeros(65 * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.sift_match_device(h, dev[0].data_ptr(), dev[1].data_ptr(), 65, dev[2].data_ptr(), None, 1023,
                             d_out.data_ptr())
    assert rc == 0
    got = d_out.cpu().numpy().view(sift_amd.MATCH_DTYPE)
    assert_same(got, gpu_ctx.match(query, train, qm))
    assert_same(got, mr.match_ref(query, train, qm))

    fwd = torch.from_numpy(b["fwd"].view(np.int32).copy()).cuda()
    rev = torch.from_numpy(b["rev"].view(np.int32).copy()).cuda()
    d_pairs = torch.zeros(5000 * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = ctypes.c_size_t()
    rc = L.sift_match_select(h, fwd.data_ptr(), 5000, rev.data_ptr(), 12000, 0.8, d_pairs.data_ptr(), 5000,
                             ctypes.byref(n))
    assert rc == 0
    want = mr.select_ref(b["ref_fwd"], b["ref_rev"], 0.8)
    assert n.value == len(want)
    assert_same(d_pairs.cpu().numpy().view(sift_amd.PAIR_DTYPE)[:n.value], want)
    assert (d_pairs.cpu().numpy()[4 * n.value:] == 0).all()
    rc = L.sift_match_select(h, fwd.data_ptr(), 5000, rev.data_ptr(), 12000, 0.8, d_pairs.data_ptr(), n.value - 1,
                             ctypes.byref(n))
    assert rc == sift_amd.SIFT_E_CAPACITY and n.value == len(want)


def test_end_to_end(gpu_ctx):
    p = sift_amd.make_params(3, 4)
    with sift_amd.Context(0) as other:
        with pytest.raises(sift_amd.SiftError) as e:
            other.match_features(other)
        assert e.value.code == sift_amd.SIFT_E_STATE
        feats = []
        for ctx, seed in ((gpu_ctx, 1), (other, 2)):
            ctx.detect(blob_image(256, 256, seed=seed), p)
            ctx.orient()
            feats.append(ctx.describe())
        (d1, ok1), (d2, ok2) = feats
        assert ok1.sum() > 100 and ok2.sum() > 100 and not ok1.all()
        got = gpu_ctx.match_features(other)
        assert_same(got, mr.match_ref(d1, d2, ok1, ok2))
        assert gpu_ctx.match_timings()["match_ms"] > 0
        assert gpu_ctx.device_matches()[1] == len(d1)
        own = gpu_ctx.match_features(gpu_ctx)
        assert_same(own, mr.match_ref(d1, d1, ok1, ok1))
        r = np.flatnonzero(ok1)
        assert (own["d2_best"][r] == 0).all() and (own["best"][r] <= r).all()
        assert (d1[own["best"][r]] == d1[r]).all()
        assert all(tuple(m) == NONE for m in own[~ok1])
        with sift_amd.Context(0) as fresh:
            with pytest.raises(sift_amd.SiftError) as e:
                gpu_ctx.match_features(fresh)
            assert e.value.code == sift_amd.SIFT_E_STATE


def test_arguments(gpu_ctx):
    L, h = sift_amd.lib(), gpu_ctx._h
    query, train = random_rows(90, 40), random_rows(91, 300)
    out = np.full(40, 7, dtype=sift_amd.MATCH_DTYPE)
    q, t, o = (a.ctypes.data_as(ctypes.c_void_p) for a in (query, train, out))
    too_many = 2**31 - 1
    for fn in (L.sift_match, L.sift_match_device):
        assert fn(h, None, None, 40, t, None, 300, o) == sift_amd.SIFT_E_ARG
        assert fn(h, q, None, 40, None, None, 300, o) == sift_amd.SIFT_E_ARG
        assert fn(h, q, None, 40, t, None, 300, None) == sift_amd.SIFT_E_ARG
        assert fn(h, q, None, too_many, t, None, 300, o) == sift_amd.SIFT_E_ARG
        assert fn(h, q, None, 40, t, None, too_many, o) == sift_amd.SIFT_E_ARG
    n = ctypes.c_size_t(99)
    for fn in (L.sift_match_select, L.sift_match_select_host):
        assert fn(h, None, 40, None, 300, 0.8, o, 40, ctypes.byref(n)) == sift_amd.SIFT_E_ARG
        assert fn(h, o, too_many, None, 300, 0.8, o, 40, ctypes.byref(n)) == sift_amd.SIFT_E_ARG
        assert fn(h, o, 40, None, too_many, 0.8, o, 40, ctypes.byref(n)) == sift_amd.SIFT_E_ARG
    assert n.value == 99 and (out.view(np.int32) == 7).all()       # nothing half-written
    assert L.sift_match_features(h, None, None, 0, None) == sift_amd.SIFT_E_ARG
    first = gpu_ctx.match(query, train)
    second = gpu_ctx.match(query, train)
    assert first.tobytes() == second.tobytes()
    assert_same(first, mr.match_ref(query, train))


def test_last_match_and_selection_state(gpu_ctx):
    L, h = sift_amd.lib(), gpu_ctx._h
    query, train = random_rows(92, 40), random_rows(93, 300)
    fwd = gpu_ctx.match(query, train)
    assert gpu_ctx.device_matches()[1] == 40
    assert len(gpu_ctx.match(query[:0], train)) == 0
    assert gpu_ctx.device_matches()[1] == 0              # the last match has no records, not the one before
    n = ctypes.c_size_t()
    f = fwd.ctypes.data_as(ctypes.c_void_p)
    assert L.sift_match_select_host(h, f, 40, None, 300, 0.0, None, 0, ctypes.byref(n)) == 0   # a count alone
    assert n.value == 40 and gpu_ctx.match_timings()["select_ms"] > 0
    out = np.full(40, 7, dtype=sift_amd.PAIR_DTYPE)
    rc = L.sift_match_select_host(h, f, 40, None, 300, 0.0, out.ctypes.data_as(ctypes.c_void_p), 39, ctypes.byref(n))
    assert rc == sift_amd.SIFT_E_CAPACITY and n.value == 40 and (out.view(np.int32) == 7).all()
    assert gpu_ctx.match_timings()["select_ms"] > 0
