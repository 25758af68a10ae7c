"""CPU checks of the match definition (tests/match_ref.py) and of the ABI
surface of the matching stage.  No compute calls (no GPU needed)."""
import numpy as np

import match_ref as mr
import sift_amd

MATCH_SYMBOLS = ("sift_match_device", "sift_match", "sift_match_features", "sift_device_matches",
                 "sift_match_select", "sift_match_select_host", "sift_last_match_timings")


def small_case():
    rng = np.random.default_rng(5)
    train = rng.integers(0, 256, (9, 128), dtype=np.uint8)
    train[4] = train[1]              # duplicates: ties at every distance
    train[7] = train[1]
    train[8] = 0
    query = rng.integers(0, 256, (7, 128), dtype=np.uint8)
    query[0] = train[1]              # d2 = 0 three times
    query[3] = train[7]
    query[5] = 255                   # far from everything, 8323200 from row 8
    query[6] = 0
    qm = np.array([1, 1, 0, 1, 1, 1, 1], dtype=np.uint8)
    tm = np.array([1, 0, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    return query, train, qm, tm


def test_match_ref_equals_the_double_loop():
    query, train, qm, tm = small_case()
    for a, b in ((None, None), (qm, None), (None, tm), (qm, tm)):
        got, want = mr.match_ref(query, train, a, b), mr.match_loops(query, train, a, b)
        for f in mr.MATCH_DTYPE.names:
            np.testing.assert_array_equal(got[f], want[f])
    full = mr.match_ref(query, train)
    assert tuple(full[0]) == (1, 4, 0, 0)                    # lowest two of the copies at 1, 4, 7
    assert tuple(mr.match_ref(query, train, None, tm)[0]) == (4, 7, 0, 0)
    assert full[5]["d2_best"] < mr.D2_MAX and mr.d2_matrix(query[5:6], train[8:9])[0, 0] == mr.D2_MAX == 8323200
    assert tuple(mr.match_ref(query, train, qm)[2]) == (-1, -1, mr.NONE_D2, mr.NONE_D2)


def test_match_ref_missing_neighbours():
    query, train, _, _ = small_case()
    one = np.zeros(9, np.uint8)
    one[6] = 1
    r = mr.match_ref(query, train, None, one)
    assert (r["best"] == 6).all() and (r["second"] == -1).all() and (r["d2_second"] == mr.NONE_D2).all()
    none = mr.match_ref(query, train, None, np.zeros(9, np.uint8))
    assert (none["best"] == -1).all() and (none["d2_best"] == mr.NONE_D2).all()
    assert len(mr.match_ref(query[:0], train)) == 0
    assert (mr.match_ref(query, train[:0])["best"] == -1).all()


def test_merge_ref_of_pieces_equals_the_whole():
    query, train, qm, tm = small_case()
    whole = mr.match_ref(query, train, qm, tm)
    cuts = (0, 2, 5, 9)
    parts = [mr.match_ref(query, train[a:b], qm, tm[a:b]) for a, b in zip(cuts, cuts[1:])]
    merged = mr.merge_ref(parts, cuts[:-1])
    for f in mr.MATCH_DTYPE.names:
        np.testing.assert_array_equal(merged[f], whole[f])


def test_selection_rule_on_a_table():
    N = mr.NONE_D2
    fwd = np.array([(2, 0, 65, 100),     # 0: 65 < 0.64 * 100 is false: rejected by the ratio
                    (1, 3, 63, 100),     # 1: passes the ratio; rev[1].best == 1
                    (-1, -1, N, N),      # 2: no neighbour
                    (0, -1, 5, N),       # 3: no second: no ratio test; rev[0].best == 3
                    (3, 1, 0, 0),        # 4: 0 < 0 false
                    (3, 2, 10, 1000)],   # 5: passes the ratio; rev[3].best == 4: not mutual
                   dtype=mr.MATCH_DTYPE)
    rev = np.array([(3, 0, 5, 9), (1, 0, 63, 70), (0, 1, 65, 66), (4, 5, 0, 10)], dtype=mr.MATCH_DTYPE)
    assert mr.select_ref(fwd, None, 0.8)["query"].tolist() == [1, 3, 5]
    assert mr.select_ref(fwd, None, 0.0)["query"].tolist() == [0, 1, 3, 4, 5]
    assert mr.select_ref(fwd, rev, 0.0)["query"].tolist() == [0, 1, 3, 4]
    got = mr.select_ref(fwd, rev, 0.8)
    assert got["query"].tolist() == [1, 3] and got["train"].tolist() == [1, 0]
    assert got["d2"].tolist() == [63, 5] and got["d2_second"].tolist() == [100, N]


def test_library_exports_the_match_entry_points():
    L = sift_amd.lib()
    for name in MATCH_SYMBOLS:
        assert name in sift_amd.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert sift_amd.MATCH_DTYPE == mr.MATCH_DTYPE and sift_amd.PAIR_DTYPE == mr.PAIR_DTYPE
    assert sift_amd.MATCH_DTYPE.itemsize == 16 and sift_amd.PAIR_DTYPE.itemsize == 16
    assert sift_amd.MATCH_NONE_D2 == mr.NONE_D2
    for m in ("match", "match_features", "select_matches", "match_timings"):
        assert callable(getattr(sift_amd.Context, m))
