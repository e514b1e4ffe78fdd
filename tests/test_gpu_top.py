"""The k best hits per query, selected on the device (miopalSearchTop / miopalSearchBatchTop, DeviceDatabase.search_top /
search_batch_top, Aligner.top_hits / top_hits_many) against the full result arrays of the plain search ordered by
(score descending, index ascending), against the CPU checker on small sets, and against
sorted(aligner.align(...), key=score, reverse=True)."""
import json
import os
import threading

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
BOUNDARY_LENGTHS = [1, 7, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 59, 60, 61, 63, 64]


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def db_set(capi):
    rng = np.random.default_rng(11)
    # above the small-search bound; empty targets and a 35 000-residue target (side kernel)
    lengths = rng.integers(20, 400, size=5000)
    lengths[[3, 1000]] = 0
    lengths[-1] = 35000
    res, off = _data.random_db(rng, lengths)
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off
    db.close()


@pytest.fixture(scope="module")
def short_db(capi):
    """1M targets of 3-8 residues without W, Y or F, a few W-bearing ones among them: a query `W` scores 0 (SW)
    against nearly all of them."""
    rng = np.random.default_rng(5)
    allowed = np.array([i for i, c in enumerate(_data.NCBI[:20]) if c not in "WYF"], dtype=np.uint8)
    lengths = rng.integers(3, 9, size=1_000_000)
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    res = allowed[rng.integers(0, len(allowed), size=int(off[-1]))]
    w = _data.NCBI.index("W")
    for t in (17, 123_456, 500_001, 999_990):
        res[off[t] + 1] = w
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off
    db.close()


def ordered(full, start, k, min_score=None):
    score = full["score"]
    order = np.lexsort((np.arange(len(score)), -score.astype(np.int64)))
    if min_score is not None:
        order = order[score[order] >= min_score]
    return order[:k]


def check_top(got, full, start, k, mode, min_score=None):
    order = ordered(full, start, k, min_score)
    c = len(order)
    count = got["count"]
    assert int(count) == c, (int(count), c)
    assert np.array_equal(got["target"][:c], start + order)
    assert np.array_equal(got["score"][:c], full["score"][order])
    assert np.all(got["target"][c:] == -1) and np.all(got["score"][c:] == -1)
    if mode == "end":
        assert np.array_equal(got["end_q"][:c], full["end_q"][order])
        assert np.array_equal(got["end_t"][:c], full["end_t"][order])
        assert np.all(got["end_q"][c:] == -1) and np.all(got["end_t"][c:] == -1)


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("mode", ["score", "end"])
def test_every_mode_and_k(db_set, algo, mode):
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    full = db.search(query, B62, 3, 1, mode, algo)
    for k in (0, 1, 7, 100, 4096):
        got = db.search_top(query, B62, 3, 1, mode, algo, k=k)
        assert got["target"].shape == (k,)
        check_top(got, full, 0, k, mode)
    # k around the length of a slice (with the 35 000-residue target in it)
    start, end = 1999, 5000
    sub = db.search(query, B62, 3, 1, mode, algo, start, end)
    n = end - start
    for k in (n - 1, n, n + 5):
        check_top(db.search_top(query, B62, 3, 1, mode, algo, start, end, k=k), sub, start, k, mode)


def test_small_sets_against_the_checker(capi):
    rng = np.random.default_rng(3)
    res, off = _data.random_db(rng, rng.integers(0, 60, size=300))
    db = capi.DeviceDatabase(res, off, 24)
    query = _data.random_protein(rng, 40)
    for algo in ("sw", "nw", "hw", "ov"):
        want = _oracle.search(query, res, off, B62, 3, 1, "end", algo)
        for k in (1, 13, 300):
            check_top(db.search_top(query, B62, 3, 1, "end", algo, k=k), want, 0, k, "end")
    db.close()


def test_ties_across_the_boundary_duplicates(capi):
    rng = np.random.default_rng(9)
    distinct = [_data.random_protein(rng, int(L)) for L in (50, 80, 120, 200, 33)]
    seqs = [distinct[i % 5] for i in range(10_000)]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    res = np.concatenate(seqs)
    db = capi.DeviceDatabase(res, off, 24)
    query = distinct[2][10:70]
    for algo in ("sw", "nw"):
        for mode in ("score", "end"):
            full = db.search(query, B62, 3, 1, mode, algo)
            for k in (1, 100, 2001, 4096):
                check_top(db.search_top(query, B62, 3, 1, mode, algo, k=k), full, 0, k, mode)
    db.close()


def test_ties_at_scale_zero_scores(short_db):
    db, res, off = short_db
    query = np.array([_data.NCBI.index("W")], dtype=np.uint8)
    full = db.search(query, B62, 3, 1, "end", "sw")
    assert np.count_nonzero(full["score"] == 0) > 900_000
    for k in (1, 3, 4, 5, 100, 4096):
        check_top(db.search_top(query, B62, 3, 1, "end", "sw", k=k), full, 0, k, "end")
    # a slice that does not start on a 16-byte boundary
    sub = db.search(query, B62, 3, 1, "score", "sw", 123_455, 700_003)
    check_top(db.search_top(query, B62, 3, 1, "score", "sw", 123_455, 700_003, k=777), sub, 123_455, 777, "score")


def test_nw_scores_across_the_sign(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(2)
    query = np.array(res[off[10]:off[11]], dtype=np.uint8)   # one positive optimum, most scores negative
    full = db.search(query, B62, 3, 1, "score", "nw")
    assert full["score"].min() < -4096 and full["score"].max() > 0
    for k in (1, 50, 4096):
        check_top(db.search_top(query, B62, 3, 1, "score", "nw", k=k), full, 0, k, "score")
    for ms in (-1, 0, int(np.sort(full["score"])[-30])):
        check_top(db.search_top(query, B62, 3, 1, "score", "nw", k=100, min_score=ms), full, 0, 100, "score", ms)
    del rng


def test_min_score(db_set):
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    for mode, algo in (("score", "sw"), ("end", "hw")):
        full = db.search(query, B62, 3, 1, mode, algo)
        s = np.sort(full["score"])[::-1]
        for k in (1, 100, 4096):
            kth = int(s[min(k, len(s)) - 1])
            for ms in (int(s[-1]) - 1, kth, int(s[0]) + 1):
                got = db.search_top(query, B62, 3, 1, mode, algo, k=k, min_score=ms)
                want = min(k, int(np.count_nonzero(full["score"] >= ms)))
                assert got["count"] == want
                check_top(got, full, 0, k, mode, ms)


def test_slices_small_search_long_queries(db_set, tuning):
    db, res, off = db_set
    rng = np.random.default_rng(4)
    long_target = int(np.argmax(np.diff(off)[:-1]))
    queries = [_data.encode(_data.README_QUERY), _data.random_protein(rng, 300), _data.random_protein(rng, 2000),
               np.array(res[off[long_target]:off[long_target + 1]], dtype=np.uint8)]
    for q in queries:
        for start, end in ((0, 5000), (7, 4093), (1234, 1300), (4990, 5000)):
            for mode in ("score", "end"):
                full = db.search(q, B62, 3, 1, mode, "sw", start, end)
                check_top(db.search_top(q, B62, 3, 1, mode, "sw", start, end, k=25), full, start, 25, mode)
    tuning.delenv("MIOPAL_NO_SMALL_SEARCH", raising=False)
    q = queries[0]
    for start, end in ((100, 140), (3, 4)):
        full = db.search(q, B62, 3, 1, "end", "nw", start, end)
        check_top(db.search_top(q, B62, 3, 1, "end", "nw", start, end, k=9), full, start, 9, "end")


def test_headline_size(capi):
    rng = np.random.default_rng(1)
    n = 1_000_000
    off = np.arange(n + 1, dtype=np.int64) * 300
    res = rng.integers(0, 20, size=n * 300, dtype=np.uint8)
    db = capi.DeviceDatabase(res, off, 24)
    query = _data.encode(_data.README_QUERY)
    for mode in ("score", "end"):
        full = db.search(query, B62, 3, 1, mode, "sw")
        check_top(db.search_top(query, B62, 3, 1, mode, "sw", k=100), full, 0, 100, mode)
    db.close()


def test_batch_rows_equal_single_searches(short_db, db_set):
    rng = np.random.default_rng(6)
    db, res, off = short_db
    lengths = BOUNDARY_LENGTHS + [65, 300, 0]
    queries = [_data.random_protein(rng, L) for L in lengths]
    queries[3] = np.array([_data.NCBI.index("W")], dtype=np.uint8)
    start, end = 10_001, 610_000   # several chunks of rows
    for mode in ("score", "end"):
        got = db.search_batch_top(queries, B62, 3, 1, mode, "sw", start, end, k=50)
        routing = db.last_batch_routing()
        db.search_batch(queries, B62, 3, 1, mode, "sw", start, end)
        assert routing == db.last_batch_routing()
        for i, q in enumerate(queries):
            single = db.search_top(q, B62, 3, 1, mode, "sw", start, end, k=50)
            row = {key: got[key][i] for key in got}
            for key in single:
                assert np.array_equal(np.asarray(row[key]), np.asarray(single[key])), (i, key)
            full = db.search(q, B62, 3, 1, mode, "sw", start, end)
            check_top(row, full, start, 50, mode)
    # NW / HW on the mixed database, one chunk
    db2, res2, off2 = db_set
    for algo in ("nw", "hw"):
        got = db2.search_batch_top(queries, B62, 3, 1, "end", algo, k=30)
        for i, q in enumerate(queries):
            full = db2.search(q, B62, 3, 1, "end", algo)
            check_top({key: got[key][i] for key in got}, full, 0, 30, "end")


def test_threads_on_one_handle(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(8)
    queries = [_data.random_protein(rng, int(L)) for L in (30, 53, 120, 300)]
    want = [db.search(q, B62, 3, 1, "end", "sw") for q in queries]
    errors = []

    def work(i):
        try:
            for _ in range(3):
                check_top(db.search_top(queries[i], B62, 3, 1, "end", "sw", k=64), want[i], 0, 64, "end")
        except Exception as e:   # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def sorted_align(aligner, query, database, mode, algorithm, k, min_score=None, **kw):
    results = sorted(aligner.align(query, database, mode=mode, algorithm=algorithm, **kw), key=lambda r: r.score,
                     reverse=True)
    return [r for r in results if min_score is None or r.score >= min_score][:k]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y) and x == y, (x, y)
        if hasattr(x, "alignment"):
            assert x.alignment == y.alignment and x.query_start == y.query_start and x.target_start == y.target_start


def test_aligner_top_hits(capi):
    import pyopal_amd
    rng = np.random.default_rng(12)
    seqs = ["".join(rng.choice(list(_data.NCBI[:20]), size=int(L))) for L in rng.integers(1, 200, size=3000)]
    seqs[5] = _data.README_QUERY
    seqs[9] = _data.README_QUERY[:30]
    database = pyopal_amd.Database(seqs)
    aligner = pyopal_amd.Aligner()
    queries = [_data.README_QUERY, _data.README_QUERY[5:40], "W", seqs[100]]
    for mode in ("score", "end", "full"):
        for algo in ("sw", "nw"):
            for q in queries:
                same(aligner.top_hits(q, database, 12, mode=mode, algorithm=algo),
                     sorted_align(aligner, q, database, mode, algo, 12))
            many = aligner.top_hits_many(queries, database, 7, mode=mode, algorithm=algo, start=3, end=2500)
            for q, got in zip(queries, many):
                same(got, sorted_align(aligner, q, database, mode, algo, 7, start=3, end=2500))
    ms = sorted_align(aligner, queries[0], database, "score", "sw", 20)[-1].score
    same(aligner.top_hits(queries[0], database, 50, min_score=ms),
         sorted_align(aligner, queries[0], database, "score", "sw", 50, ms))


@pytest.mark.parametrize("vid", ["G3", "G4"])
def test_reference_examples(capi, vid):
    import pyopal_amd
    vectors = json.load(open(os.path.join(HERE, "golden", "reference_vectors.json")))["vectors"]
    v = next(x for x in vectors if x["id"] == vid)
    database = pyopal_amd.Database(v["targets"])
    aligner = pyopal_amd.Aligner(v["matrix"], gap_open=v["gap_open"], gap_extend=v["gap_extend"])
    for mode in ("score", "end", "full"):
        for k in (1, 2, len(v["targets"]), 10):
            got = aligner.top_hits(v["query"], database, k, mode=mode, algorithm=v["algorithm"])
            same(got, sorted_align(aligner, v["query"], database, mode, v["algorithm"], k))
            assert aligner.top_hits_many([v["query"]], database, k, mode=mode, algorithm=v["algorithm"]) == [got]
    best = aligner.top_hits(v["query"], database, 1, algorithm=v["algorithm"])[0]
    known = [(s, -i) for i, s in enumerate(v["score"]) if s is not None]
    if len(known) == len(v["score"]):
        assert best.score == max(known)[0]


# ---- arms of the selection that the searches above do not reach (tests/test_gpu_select_rows.py drives the same arms on
# synthetic rows): a second group of 1024 rows, the third histogram round, rows of more than 2^20 entries ----

@pytest.mark.parametrize("algo", ["sw", "hw"])
@pytest.mark.parametrize("mode", ["score", "end"])
def test_batch_above_one_group_of_rows(capi, algo, mode):
    """1100 queries in ONE chunk of the batch: the selection takes its rows in groups of 1024, so rows 1024.. come
    from its second sequence of launches."""
    rng = np.random.default_rng(1100)
    res, off = _data.random_db(rng, rng.integers(20, 201, size=300))
    db = capi.DeviceDatabase(res, off, 24)
    lengths = [BOUNDARY_LENGTHS[i % len(BOUNDARY_LENGTHS)] for i in range(1100)]
    for at, length in ((5, 65), (700, 0), (1023, 65), (1024, 0), (1030, 65), (1099, 0)):   # the single-query path
        lengths[at] = length
    queries = [_data.random_protein(rng, L) for L in lengths]
    got = db.search_batch_top(queries, B62, 3, 1, mode, algo, k=20)
    routing = db.last_batch_routing()
    full = db.search_batch(queries, B62, 3, 1, mode, algo)
    assert routing == db.last_batch_routing()
    # which lengths the batch kernels take under this model (a 64-row class does not fit their LDS table with 24 letters)
    single = set()
    for length in sorted(set(lengths)):
        db.search_batch([queries[lengths.index(length)]], B62, 3, 1, mode, algo)
        if db.last_batch_routing()[2]:
            single.add(length)
    assert {0, 65} <= single and not single & set(BOUNDARY_LENGTHS[:17])
    batch = sum(length not in single for length in lengths)
    assert sum(length not in single for length in lengths[1024:]) >= 50
    # every pair of the batch queries settled by the batch kernels or by their int32 pass, and in ONE chunk: as many
    # launches of the batch kernels (one per class of query rows and chunk) as for 21 queries that hold every length
    assert routing[2] == len(queries) - batch and routing[0] > 0 and routing[0] + routing[1] == batch * 300
    assert lengths[21:42] == BOUNDARY_LENGTHS
    db.search_batch(queries[21:42], B62, 3, 1, mode, algo)
    assert db.last_batch_routing()[3] == routing[3]
    for i in range(len(queries)):
        row = {key: got[key][i] for key in got}
        check_top(row, {key: full[key][i] for key in full}, 0, 20, mode)
    db.close()


def test_three_histogram_rounds_through_a_search(db_set):
    """NW with gaps of 600 against a 35 000-residue target: the scores span more than 2^24, which takes all three
    histogram rounds (12 + 12 + 8 bits)."""
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    full = db.search(query, B62, 600, 600, "score", "nw")
    assert int(full["score"].max()) - int(full["score"].min()) >= 2 ** 24
    for k in (1, 50, 4096):
        check_top(db.search_top(query, B62, 600, 600, "score", "nw", k=k), full, 0, k, "score")
    ms = int(np.sort(full["score"])[len(full["score"]) // 2])
    for k in (50, 4096):
        check_top(db.search_top(query, B62, 600, 600, "score", "nw", k=k, min_score=ms), full, 0, k, "score", ms)
    ends = db.search(query, B62, 600, 600, "end", "nw")
    check_top(db.search_top(query, B62, 600, 600, "end", "nw", k=50), ends, 0, 50, "end")


@pytest.fixture(scope="module")
def long_short_db(capi):
    """short_db's recipe with 1 100 000 targets: rows of 269 blocks of 4096 scores (68 of 16 384)."""
    rng = np.random.default_rng(55)
    allowed = np.array([i for i, c in enumerate(_data.NCBI[:20]) if c not in "WYF"], dtype=np.uint8)
    lengths = rng.integers(3, 9, size=1_100_000)
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    res = allowed[rng.integers(0, len(allowed), size=int(off[-1]))]
    w = _data.NCBI.index("W")
    for t in (17, 123_456, 500_001, 999_990, 1_050_000, 1_099_999):
        res[off[t] + 1] = w
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off
    db.close()


def test_rows_of_more_than_a_million_entries(long_short_db):
    db, res, off = long_short_db
    query = np.array([_data.NCBI.index("W")], dtype=np.uint8)
    full = db.search(query, B62, 3, 1, "end", "sw")
    assert np.count_nonzero(full["score"] == 0) > 1_000_000 and np.count_nonzero(full["score"] > 0) >= 6
    for k in (1, 5, 4096):
        check_top(db.search_top(query, B62, 3, 1, "end", "sw", k=k), full, 0, k, "end")
    # a slice of more than 2^20 targets that does not start on a 16-byte boundary
    start, end = 3, 1_080_000
    sub = db.search(query, B62, 3, 1, "end", "sw", start, end)
    for k in (5, 4096):
        check_top(db.search_top(query, B62, 3, 1, "end", "sw", start, end, k=k), sub, start, k, "end")
