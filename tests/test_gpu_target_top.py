"""The m best queries of every target, selected on the device (miopalSearchBatchTargetTop;
DeviceDatabase.search_batch_target_top; Aligner.best_queries / best_queries_arrays) against the dense batched search of
the same inputs reduced with numpy on the host, against the CPU checker on a small set, and against Aligner.align_many /
align_pairs. Thresholds are quantiles of the DENSE result (and INT_MIN): none depends on the code under test, and every
family of cases asserts that counts of 0, counts strictly between 0 and m and counts of m all occur."""
import ctypes
import threading

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix
from test_gpu_select_columns import reference

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
INT_MIN = -(2 ** 31)
BATCH_LENGTHS = [0, 1, 8, 9, 60, 61, 64, 65, 150]
KEYS = ("count", "query", "score", "end_q", "end_t")


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
def small_set(capi):
    """300 targets of 0-59 residues: below the small-search bound"""
    rng = np.random.default_rng(3)
    res, off = _data.random_db(rng, rng.integers(0, 60, size=300))
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off
    db.close()


def thresholds_of(score):
    """INT_MIN, the 50 % and 99 % quantiles of the dense scores, and one above their maximum"""
    s = np.sort(score, axis=None)
    return [INT_MIN, int(s[len(s) // 2]), int(s[(len(s) * 99) // 100]), int(s[-1]) + 1]


def reduce_dense(dense, m, threshold):
    """The reference: column t of the dense [queries][targets] arrays - entries >= threshold, by (-score, query), the
    first m. One sort key per cell (the scores of a search are far from 2^40), argpartition instead of a full sort."""
    score = dense["score"].astype(np.int64)
    rows, n = score.shape
    assert rows < 2 ** 20 and np.abs(score).max(initial=0) < 2 ** 40
    keep = score >= threshold
    key = np.where(keep, -score * 2 ** 20 + np.arange(rows)[:, None], 2 ** 62)
    top = np.argpartition(key, m - 1, axis=0)[:m] if rows > m else np.broadcast_to(np.arange(rows)[:, None], key.shape)
    cols = np.arange(n)[None, :]
    top = np.take_along_axis(top, np.argsort(key[top, cols], axis=0), axis=0)
    count = np.minimum(m, keep.sum(axis=0)).astype(np.int32)
    has = (np.arange(top.shape[0])[:, None] < count[None, :]).T
    out = {"count": count}
    for name, source in (("query", None), ("score", dense["score"]), ("end_q", dense.get("end_q")),
                         ("end_t", dense.get("end_t"))):
        if name != "query" and source is None:
            continue
        full = np.full((n, m), -1, dtype=np.int32)
        values = top if source is None else source[top, cols]
        full[:, :top.shape[0]][has] = values.T[has]
        out[name] = full
    return out


def same(got, want, what):
    for key in KEYS:
        assert (key in got) == (key in want), (what, key)
        if key in want:
            assert got[key].dtype == np.int32 and got[key].shape == want[key].shape, (what, key)
            assert np.array_equal(got[key], want[key]), (what, key)


class Seen:
    """which kinds of count a family of cases has produced"""

    def __init__(self):
        self.none = self.some = self.all = False

    def add(self, count, m):
        self.none |= bool((count == 0).any())
        self.some |= bool(((count > 0) & (count < m)).any())
        self.all |= bool((count == m).any())

    def everything(self):
        return self.none and self.some and self.all


def test_the_fast_reduction_is_the_reference():
    rng = np.random.default_rng(1)
    for rows, n, m in ((1, 7, 3), (3, 50, 3), (9, 200, 8), (40, 33, 1), (40, 33, 8)):
        dense = {key: rng.integers(-4, 5, size=(rows, n)).astype(np.int32) for key in ("score", "end_q", "end_t")}
        for threshold in (INT_MIN, -1, 3, 6):
            same(reduce_dense(dense, m, threshold),
                 reference(dense["score"], m, threshold, None, dense["end_q"], dense["end_t"]), (rows, n, m, threshold))


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("mode", ["score", "end"])
def test_equals_the_reduced_dense_batch(db_set, algo, mode):
    db, res, off = db_set
    rng = np.random.default_rng(6)
    queries = [_data.random_protein(rng, L) for L in BATCH_LENGTHS]
    dense = db.search_batch(queries, B62, 3, 1, mode, algo)
    routing = db.last_batch_routing()
    # both the batch kernels and the single-query path (lengths 0, 65 and 150 at least) feed the fold
    assert routing[2] > 0 and routing[0] > 0
    seen = Seen()
    for threshold in thresholds_of(dense["score"]):
        for m in (1, 3, 8):
            got = db.search_batch_target_top(queries, B62, 3, 1, mode, algo, 0, None, m, threshold)
            assert db.last_batch_routing() == routing
            same(got, reduce_dense(dense, m, threshold), (threshold, m))
            seen.add(got["count"], m)
    assert seen.everything()
    # no threshold: every query is a candidate
    got = db.search_batch_target_top(queries, B62, 3, 1, mode, algo, m=8)
    assert np.all(got["count"] == 8)
    same(got, reduce_dense(dense, 8, INT_MIN), "no bound")


def test_slice(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(16)
    queries = [_data.random_protein(rng, L) for L in BATCH_LENGTHS]
    seen = Seen()
    for algo, mode in (("sw", "end"), ("nw", "score"), ("hw", "end")):
        dense = db.search_batch(queries, B62, 3, 1, mode, algo, 1999, 5000)
        routing = db.last_batch_routing()
        for threshold in thresholds_of(dense["score"])[:3]:
            got = db.search_batch_target_top(queries, B62, 3, 1, mode, algo, 1999, 5000, 4, threshold)
            assert db.last_batch_routing() == routing
            assert got["count"].shape == (3001,)
            same(got, reduce_dense(dense, 4, threshold), (algo, mode, threshold))
            seen.add(got["count"], 4)
    assert seen.everything()


def test_fewer_queries_than_m(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(26)
    queries = [_data.random_protein(rng, L) for L in (12, 70, 30)]
    dense = db.search_batch(queries, B62, 3, 1, "end", "sw")
    seen = Seen()
    for threshold in thresholds_of(dense["score"]):
        got = db.search_batch_target_top(queries, B62, 3, 1, "end", "sw", m=8, min_score=threshold)
        same(got, reduce_dense(dense, 8, threshold), threshold)
        assert got["count"].max() <= 3 and np.all(got["query"][:, 3:] == -1) and np.all(got["end_t"][:, 3:] == -1)
        seen.add(got["count"], 3)
    assert seen.everything()
    # one query, m = 1 and m = 8: its own scores where they pass
    one = db.search_batch_target_top(queries[:1], B62, 3, 1, "score", "sw", m=8, min_score=thresholds_of(dense["score"][0])[1])
    passed = dense["score"][0] >= thresholds_of(dense["score"][0])[1]
    assert np.array_equal(one["count"], passed.astype(np.int32)) and 0 < passed.sum() < len(passed)
    assert np.array_equal(one["score"][:, 0], np.where(passed, dense["score"][0], -1))


def test_duplicate_queries_tie_to_the_lower_index(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(36)
    a, b, c = (_data.random_protein(rng, L) for L in (20, 33, 90))
    queries = [a, a, a, b, b, c, c]
    for algo, mode in (("sw", "end"), ("hw", "score")):
        dense = db.search_batch(queries, B62, 3, 1, mode, algo)
        for m in (2, 4, 8):
            got = db.search_batch_target_top(queries, B62, 3, 1, mode, algo, m=m)
            same(got, reduce_dense(dense, m, INT_MIN), (algo, mode, m))
        # the copies of a query score alike and have neighbouring indices: wherever a later copy is named, the one
        # before it stands right in front of it
        got = db.search_batch_target_top(queries, B62, 3, 1, mode, algo, m=8)
        for first, later in ((0, 1), (1, 2), (3, 4), (5, 6)):
            t, j = np.nonzero(got["query"] == later)
            assert len(t) > 0 and np.all(j > 0) and np.all(got["query"][t, j - 1] == first)
            assert np.all(got["score"][t, j - 1] == got["score"][t, j])


def test_more_than_one_chunk(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(46)
    lengths = rng.integers(4, 13, size=1700)
    first_of_second = 2 ** 23 // 5000   # the chunk bound of the batch (kBatchChunkPairs)
    assert len(lengths) > first_of_second
    lengths[first_of_second:] = 12   # (the queries of the second chunk are among the strongest)
    queries = [_data.random_protein(rng, int(L)) for L in lengths]
    dense = db.search_batch(queries, B62, 3, 1, "end", "hw")
    routing = db.last_batch_routing()
    seen = Seen()
    s = np.sort(dense["score"], axis=None)
    # (above all but about three scores per target on average; and no bound)
    for threshold in (int(s[len(s) - 3 * 5000]), INT_MIN):
        got = db.search_batch_target_top(queries, B62, 3, 1, "end", "hw", m=8, min_score=threshold)
        assert db.last_batch_routing() == routing
        same(got, reduce_dense(dense, 8, threshold), threshold)
        seen.add(got["count"], 8)
    assert seen.everything()
    # queries of the second chunk are named as well as those of the first
    assert (got["query"] >= first_of_second).any() and (got["query"][:, 0] < first_of_second).any()


def test_small_set_against_the_checker(small_set, tuning):
    db, res, off = small_set
    tuning.delenv("MIOPAL_NO_SMALL_SEARCH", raising=False)
    rng = np.random.default_rng(4)
    queries = [_data.random_protein(rng, L) for L in (0, 1, 9, 40, 64, 65, 150)]
    seen = Seen()
    for algo in ("sw", "nw", "hw", "ov"):
        rows = [_oracle.search(q, res, off, B62, 3, 1, "end", algo) for q in queries]
        dense = {key: np.stack([r[key] for r in rows]).astype(np.int32) for key in ("score", "end_q", "end_t")}
        for threshold in thresholds_of(dense["score"])[:3]:
            got = db.search_batch_target_top(queries, B62, 3, 1, "end", algo, m=3, min_score=threshold)
            same(got, reduce_dense(dense, 3, threshold), (algo, threshold))
            seen.add(got["count"], 3)
        routing = db.last_batch_routing()
        assert routing[0] == 0 and routing[1] > 0 and routing[3] == 0   # everything one wavefront per pair
    assert seen.everything()


def test_empty_slice_and_no_queries(db_set, capi):
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    for mode in ("score", "end"):
        got = db.search_batch_target_top([query, query[:5]], B62, 3, 1, mode, "sw", 40, 40, 2)
        assert got["count"].shape == (0,) and got["query"].shape == (0, 2) and ("end_q" in got) == (mode == "end")
        # no queries: every target of the slice without a candidate, nothing launched
        got = db.search_batch_target_top([], B62, 3, 1, mode, "sw", 10, 50, 3)
        assert db.last_batch_routing() == (0, 0, 0, 0)
        assert got["count"].tolist() == [0] * 40
        for key in got:
            if key != "count":
                assert got[key].shape == (40, 3) and np.all(got[key] == -1), key
    # the C call itself on an empty slice: 0, nothing written
    offsets = np.array([0, len(query)], dtype=np.int64)
    marks = [np.full(8, 77, dtype=np.int32) for _ in range(5)]
    rc = capi.lib().miopalSearchBatchTargetTop(db.handle, query.ctypes.data, offsets.ctypes.data, 1, 3, 1, B62.ctypes.data,
                                               24, 1, 3, 40, 40, 2, INT_MIN, *[a.ctypes.data for a in marks])
    assert rc == 0 and all(np.all(a == 77) for a in marks)
    # m and the outputs are checked behind the queries, before any work; a failing call writes nothing
    for m, missing in ((0, ()), (9, ()), (2, (0,)), (2, (1,)), (2, (3,))):
        args = [None if i in missing else a.ctypes.data for i, a in enumerate(marks)]
        rc = capi.lib().miopalSearchBatchTargetTop(db.handle, query.ctypes.data, offsets.ctypes.data, 1, 3, 1,
                                                   B62.ctypes.data, 24, 1, 3, 0, 2, m, INT_MIN, *args)
        assert rc == 101 and all(np.all(a == 77) for a in marks), (m, missing)
    # (the end arrays are only needed for end locations)
    args = [a.ctypes.data for a in marks[:3]] + [None, None]
    rc = capi.lib().miopalSearchBatchTargetTop(db.handle, query.ctypes.data, offsets.ctypes.data, 1, 3, 1, B62.ctypes.data,
                                               24, 0, 3, 0, 2, 2, INT_MIN, *args)
    assert rc == 0 and marks[0][:2].tolist() == [1, 1] and marks[1][:4].tolist() == [0, -1, 0, -1]
    rc = capi.lib().miopalSearchBatchTargetTop(db.handle, query.ctypes.data, offsets.ctypes.data, 1, 3, 1, B62.ctypes.data,
                                               24, 2, 3, 0, 2, 2, INT_MIN, *args)
    assert rc == capi.OPAL_ERR_INVALID_MODE


def test_threads_on_one_handle(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(8)
    cases = []
    for i, (mode, algo, m) in enumerate((("end", "sw", 8), ("score", "hw", 1), ("end", "nw", 3), ("score", "sw", 2))):
        queries = [_data.random_protein(rng, int(L)) for L in (30, 53, 120, 8, 64, 300)[i:]]
        dense = db.search_batch(queries, B62, 3, 1, mode, algo)
        threshold = thresholds_of(dense["score"])[1 + i % 2]
        cases.append((queries, mode, algo, m, threshold, reduce_dense(dense, m, threshold)))
    errors = []

    def work(i):
        queries, mode, algo, m, threshold, want = cases[i]
        try:
            for _ in range(3):
                same(db.search_batch_target_top(queries, B62, 3, 1, mode, algo, m=m, min_score=threshold), want, i)
        except Exception as e:   # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def same_objects(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y) and x == y, (x, y)
        if hasattr(x, "alignment"):
            assert x.alignment == y.alignment and x.query_start == y.query_start and x.target_start == y.target_start
            assert x.cigar() == y.cigar()


@pytest.fixture(scope="module")
def python_case(capi):
    import pyopal_amd
    rng = np.random.default_rng(12)
    seqs = ["".join(rng.choice(list(_data.NCBI[:20]), size=int(L))) for L in rng.integers(1, 200, size=700)]
    seqs[5] = _data.README_QUERY
    seqs[9] = _data.README_QUERY[:30]
    queries = [_data.README_QUERY[5:40], "W", seqs[100][:50], _data.README_QUERY[:30], seqs[9], seqs[200] + seqs[201]]
    return pyopal_amd.Aligner(), pyopal_amd.Database(seqs), queries


def test_aligner_best_queries(python_case):
    import pyopal_amd
    aligner, database, queries = python_case
    for mode, kind in (("score", pyopal_amd.ScoreResult), ("end", pyopal_amd.EndResult)):
        for algo in ("sw", "hw"):
            for start, end in ((0, 700), (3, 650)):
                per_query = aligner.align_many(queries, database, mode=mode, algorithm=algo, start=start, end=end)
                scores = np.array([[r.score for r in row] for row in per_query])
                for m, threshold in ((1, None), (3, thresholds_of(scores)[1]), (8, thresholds_of(scores)[2])):
                    got = aligner.best_queries(queries, database, m, mode=mode, algorithm=algo, min_score=threshold,
                                               start=start, end=end)
                    assert len(got) == end - start
                    lengths = set()
                    for t, row in enumerate(got):
                        order = sorted((q for q in range(len(queries)) if threshold is None or scores[q, t] >= threshold),
                                       key=lambda q: (-scores[q, t], q))[:m]
                        assert [q for q, _ in row] == order, (t, row)
                        same_objects([r for _, r in row], [per_query[q][t] for q in order])
                        assert all(type(r) is kind and r.target_index == start + t for _, r in row)
                        lengths.add(len(row))
                    assert len(lengths) > 1 or threshold is None


def test_aligner_full_equals_align_pairs_of_the_chosen(python_case):
    import pyopal_amd
    aligner, database, queries = python_case
    for algo in ("sw", "nw"):
        chosen = aligner.best_queries(queries, database, 2, algorithm=algo, start=3, end=650)
        scores = np.array([r.score for row in chosen for _, r in row])
        threshold = int(np.sort(scores)[len(scores) // 2])
        chosen = aligner.best_queries(queries, database, 2, algorithm=algo, min_score=threshold, start=3, end=650)
        got = aligner.best_queries(queries, database, 2, mode="full", algorithm=algo, min_score=threshold, start=3, end=650)
        assert {len(row) for row in got} == {0, 1, 2}
        assert [[q for q, _ in row] for row in got] == [[q for q, _ in row] for row in chosen]
        pairs = [(q, 3 + t) for t, row in enumerate(got) for q, _ in row]
        want = aligner.align_pairs(queries, database, pairs, mode="full", algorithm=algo)
        flat = [r for row in got for _, r in row]
        assert all(type(r) is pyopal_amd.FullResult for r in flat)
        same_objects(flat, want)
        # the arrays: the pair list row-major over (target, rank)
        arrays = aligner.best_queries_arrays(queries, database, 2, mode="full", algorithm=algo, min_score=threshold,
                                             start=3, end=650)
        assert arrays["count"].tolist() == [len(row) for row in got] and "end_q" not in arrays
        assert arrays["pairs"]["query"].tolist() == [q for q, _ in pairs]
        assert arrays["pairs"]["target"].tolist() == [t for _, t in pairs]
        assert arrays["pairs"]["score"].tolist() == [r.score for r in want]
        assert arrays["pairs"]["start_t"].tolist() == [r.target_start for r in want]
        assert int(arrays["pairs"]["aln_off"][-1]) == len(arrays["pairs"]["aln_flat"]) == sum(len(r.alignment) for r in want)
