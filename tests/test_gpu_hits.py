"""Every hit at or above a threshold, compacted on the device (miopalSearchHits / miopalSearchPssmHits /
miopalSearchBatchHits; DeviceDatabase.search_hits / search_pssm_hits / search_batch_hits; Aligner.hits / hits_many /
hits_pssm) against the plain search of the same inputs filtered on the host, against the CPU checker on a small set,
and against the filtered Aligner.align. Thresholds are quantiles of the PLAIN search's scores: no case is vacuous and
none depends on the code under test."""
import ctypes
import threading

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
INT_MIN = -(2 ** 31)
BATCH_LENGTHS = [0, 1, 8, 9, 60, 61, 64, 65, 150]


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
    """the 0 %, 50 % and 99 % quantiles of the plain search's scores, and one above its maximum"""
    s = np.sort(score)
    return [int(s[0]), int(s[len(s) // 2]), int(s[(len(s) * 99) // 100]), int(s[-1]) + 1]


def check_hits(got, full, start, threshold, mode):
    keep = np.nonzero(full["score"] >= threshold)[0]
    assert got["count"] == len(keep), (got["count"], len(keep))
    assert got["target"].dtype == np.int64 and np.array_equal(got["target"], start + keep)
    assert got["score"].dtype == np.int32 and np.array_equal(got["score"], full["score"][keep])
    if mode == "end":
        assert np.array_equal(got["end_q"], full["end_q"][keep]) and np.array_equal(got["end_t"], full["end_t"][keep])
    else:
        assert "end_q" not in got and "end_t" not in got
    return len(keep)


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("mode", ["score", "end"])
def test_hits_equal_the_filtered_search(db_set, algo, mode):
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    for start, end in ((0, 5000), (1999, 5000)):
        full = db.search(query, B62, 3, 1, mode, algo, start, end)
        routing = db.last_routing()
        counts = []
        for threshold in thresholds_of(full["score"]):
            counts.append(check_hits(db.search_hits(query, B62, 3, 1, mode, algo, start, end, threshold), full, start,
                                     threshold, mode))
            assert db.last_routing() == routing
        n = end - start
        assert counts[0] == n and n // 4 < counts[1] < n and 0 < counts[2] < n // 10 and counts[3] == 0
        # no threshold: every target
        assert check_hits(db.search_hits(query, B62, 3, 1, mode, algo, start, end), full, start, INT_MIN, mode) == n


def test_small_set_against_the_checker(small_set):
    db, res, off = small_set
    query = _data.random_protein(np.random.default_rng(4), 40)
    for algo in ("sw", "nw", "hw", "ov"):
        want = _oracle.search(query, res, off, B62, 3, 1, "end", algo)
        for threshold in thresholds_of(want["score"]):
            check_hits(db.search_hits(query, B62, 3, 1, "end", algo, min_score=threshold), want, 0, threshold, "end")


def test_empty_slice(db_set):
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    rows = B62.reshape(24, 24)[query]
    for mode in ("score", "end"):
        for got in (db.search_hits(query, B62, 3, 1, mode, "sw", 40, 40, 0),
                    db.search_pssm_hits(rows, 3, 1, mode, "sw", 40, 40, 0)):
            assert got["count"] == 0 and len(got["target"]) == 0 and len(got["score"]) == 0
        got = db.search_batch_hits([query, query[:5]], B62, 3, 1, mode, "sw", 40, 40, [0, 1])
        assert got["offsets"].tolist() == [0, 0, 0] and len(got["target"]) == 0


def test_pssm_form(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(21)
    query = _data.encode(_data.README_QUERY)
    # rows taken from the matrix: the plain form's answer
    rows = B62.reshape(24, 24)[query]
    for algo, mode in (("sw", "end"), ("nw", "score")):
        full = db.search(query, B62, 3, 1, mode, algo)
        for threshold in thresholds_of(full["score"])[1:]:
            want = db.search_hits(query, B62, 3, 1, mode, algo, min_score=threshold)
            got = db.search_pssm_hits(rows, 3, 1, mode, algo, min_score=threshold)
            assert got["count"] == want["count"] > 0 or threshold > full["score"].max()
            for key in want:
                assert np.array_equal(got[key], want[key]), (algo, mode, key)
    # random rows, and rows that leave the byte profile (entries up to +-300): the 32-bit kernels produce those scores
    cases = [rng.integers(-6, 12, size=(70, 24)).astype(np.int32),
             rng.choice(np.array(list(range(250, 301, 5)) * 3 + [-300, -300]), size=(170, 24)).astype(np.int32)]
    for at, rows in enumerate(cases):
        for algo, mode in (("sw", "end"), ("nw", "score"), ("hw", "end")):
            for start, end in ((0, None), (1999, 4001)):
                full = db.search_pssm(rows, None, 3, 1, mode, algo, start, end)
                routing = db.last_routing()
                if at == 1:
                    assert (routing[3] > 0 or routing[0] > 0) and full["score"].max() > 32767, (algo, mode, routing)
                for threshold in thresholds_of(full["score"]):
                    got = db.search_pssm_hits(rows, 3, 1, mode, algo, start, end, threshold)
                    assert db.last_routing() == routing
                    check_hits(got, full, start, threshold, mode)
    # no rows at all
    none = np.zeros((0, 24), dtype=np.int32)
    full = db.search_pssm(none, None, 3, 1, "score", "nw")
    check_hits(db.search_pssm_hits(none, 3, 1, "score", "nw", min_score=int(np.median(full["score"]))), full, 0,
               int(np.median(full["score"])), "score")


def batch_case(db, rng, mode, algo, start=0, end=None):
    queries = [_data.random_protein(rng, L) for L in BATCH_LENGTHS]
    singles = [db.search(q, B62, 3, 1, mode, algo, start, end) for q in queries]
    # one threshold per query, walking through the quantiles (the last one above its query's maximum)
    thresholds = [thresholds_of(s["score"])[i % 4] for i, s in enumerate(singles)]
    return queries, singles, thresholds


def check_batch(db, queries, thresholds, mode, algo, start, end, got):
    offsets = got["offsets"]
    assert offsets.dtype == np.int64 and len(offsets) == len(queries) + 1 and offsets[0] == 0
    for i, q in enumerate(queries):
        want = db.search_hits(q, B62, 3, 1, mode, algo, start, end, thresholds[i])
        assert offsets[i + 1] - offsets[i] == want["count"], i
        for key in want:
            if key != "count":
                assert np.array_equal(got[key][offsets[i]:offsets[i + 1]], want[key]), (i, key)
    assert len(got["target"]) == offsets[-1]


@pytest.mark.parametrize("algo", ["sw", "nw"])
@pytest.mark.parametrize("mode", ["score", "end"])
def test_batch_form(db_set, algo, mode):
    db, res, off = db_set
    rng = np.random.default_rng(6)
    for start, end in ((0, 5000), (7, 4093)):
        queries, singles, thresholds = batch_case(db, rng, mode, algo, start, end)
        got = db.search_batch_hits(queries, B62, 3, 1, mode, algo, start, end, thresholds)
        routing = db.last_batch_routing()
        db.search_batch(queries, B62, 3, 1, mode, algo, start, end)
        assert routing == db.last_batch_routing()
        # both the batch kernels and the single-query path (lengths 0, 65 and 150 at least) were used
        assert routing[0] > 0 and routing[2] >= 3 and routing[2] < len(queries)
        check_batch(db, queries, thresholds, mode, algo, start, end, got)
        # ... and every hit is what the plain search says
        for i, full in enumerate(singles):
            row = {key: got[key][got["offsets"][i]:got["offsets"][i + 1]] for key in got if key != "offsets"}
            row["count"] = len(row["target"])
            check_hits(row, full, start, thresholds[i], mode)
    # one threshold for all, and none
    got = db.search_batch_hits(queries, B62, 3, 1, mode, algo, 0, 5000, 30)
    check_batch(db, queries, [30] * len(queries), mode, algo, 0, 5000, got)
    got = db.search_batch_hits(queries[:3], B62, 3, 1, mode, algo, 100, 700)
    assert got["offsets"].tolist() == [0, 600, 1200, 1800]
    # no queries
    got = db.search_batch_hits([], B62, 3, 1, mode, algo, 0, 5000, 0)
    assert got["offsets"].tolist() == [0] and len(got["target"]) == 0 and len(got["score"]) == 0


def test_batch_form_below_the_small_search_bound(small_set, tuning):
    db, res, off = small_set
    tuning.delenv("MIOPAL_NO_SMALL_SEARCH", raising=False)
    rng = np.random.default_rng(16)
    for mode, algo in (("end", "sw"), ("score", "hw")):
        queries, singles, thresholds = batch_case(db, rng, mode, algo)
        got = db.search_batch_hits(queries, B62, 3, 1, mode, algo, min_score=thresholds)
        routing = db.last_batch_routing()
        db.search_batch(queries, B62, 3, 1, mode, algo)
        assert routing == db.last_batch_routing()
        assert routing[0] == 0 and routing[1] > 0 and routing[3] == 0   # everything one wavefront per pair
        check_batch(db, queries, thresholds, mode, algo, 0, None, got)


def test_max_hits_single(db_set, capi):
    db, res, off = db_set
    query = _data.encode(_data.README_QUERY)
    full = db.search(query, B62, 3, 1, "end", "sw")
    threshold = thresholds_of(full["score"])[1]
    total = int(np.count_nonzero(full["score"] >= threshold))
    assert total > 1000
    check_hits(db.search_hits(query, B62, 3, 1, "end", "sw", min_score=threshold, max_hits=total), full, 0, threshold, "end")
    with pytest.raises(capi.TooManyHits) as info:
        db.search_hits(query, B62, 3, 1, "end", "sw", min_score=threshold, max_hits=total - 1)
    assert info.value.counts == total
    # the C call itself: the count filled, the pointers as they were
    count = ctypes.c_int64(-1)
    ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
    rc = capi.lib().miopalSearchHits(db.handle, query.ctypes.data, len(query), 3, 1, B62.ctypes.data, 24, 1, 3, 0, 5000,
                                     threshold, 0, ctypes.byref(count), *[ctypes.byref(p) for p in ptrs])
    assert rc == capi.MIOPAL_ERR_TOO_MANY_HITS == 103 and count.value == total and all(p.value == 0x55 for p in ptrs)
    assert str(total) in capi.last_error()
    # the handle stays usable, for the PSSM form as well
    check_hits(db.search_hits(query, B62, 3, 1, "end", "sw", min_score=threshold), full, 0, threshold, "end")
    rows = B62.reshape(24, 24)[query]
    with pytest.raises(capi.TooManyHits) as info:
        db.search_pssm_hits(rows, 3, 1, "score", "sw", min_score=threshold, max_hits=total - 1)
    assert info.value.counts == total
    assert db.search_pssm_hits(rows, 3, 1, "score", "sw", min_score=threshold, max_hits=total)["count"] == total
    # a bound of 0 with no hits is no error
    assert db.search_hits(query, B62, 3, 1, "end", "sw", min_score=int(full["score"].max()) + 1, max_hits=0)["count"] == 0


def test_max_hits_batch(db_set, capi):
    db, res, off = db_set
    rng = np.random.default_rng(26)
    queries, singles, thresholds = batch_case(db, rng, "end", "sw")
    counts = [int(np.count_nonzero(s["score"] >= t)) for s, t in zip(singles, thresholds)]
    total = sum(counts)
    assert total > 5000
    got = db.search_batch_hits(queries, B62, 3, 1, "end", "sw", min_score=thresholds, max_hits=total)
    check_batch(db, queries, thresholds, "end", "sw", 0, None, got)
    # one too few - and a bound that the first chunk already passes: the counts of ALL queries come back
    for bound in (total - 1, 1, 0):
        with pytest.raises(capi.TooManyHits) as info:
            db.search_batch_hits(queries, B62, 3, 1, "end", "sw", min_score=thresholds, max_hits=bound)
        assert np.diff(info.value.counts).tolist() == counts, bound
    # the C call itself: hitOffsets filled, the pointers as they were
    flat = np.concatenate(queries)
    offsets = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int64)
    t = np.array(thresholds, dtype=np.int32)
    hit_offsets = np.full(len(queries) + 1, -7, dtype=np.int64)
    ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
    rc = capi.lib().miopalSearchBatchHits(db.handle, flat.ctypes.data, offsets.ctypes.data, len(queries), 3, 1,
                                          B62.ctypes.data, 24, 1, 3, 0, 5000, t.ctypes.data, total - 1,
                                          hit_offsets.ctypes.data, *[ctypes.byref(p) for p in ptrs])
    assert rc == 103 and np.diff(hit_offsets).tolist() == counts and hit_offsets[0] == 0
    assert all(p.value == 0x55 for p in ptrs)
    # the next call on the handle is right
    got = db.search_batch_hits(queries, B62, 3, 1, "end", "sw", min_score=thresholds)
    check_batch(db, queries, thresholds, "end", "sw", 0, None, got)


def test_threads_on_one_handle(db_set):
    db, res, off = db_set
    rng = np.random.default_rng(8)
    queries = [_data.random_protein(rng, int(L)) for L in (30, 53, 120, 300)]
    want = [db.search(q, B62, 3, 1, "end", "sw") for q in queries]
    thresholds = [thresholds_of(w["score"])[1 + i % 2] for i, w in enumerate(want)]
    errors = []

    def work(i):
        try:
            for _ in range(3):
                check_hits(db.search_hits(queries[i], B62, 3, 1, "end", "sw", min_score=thresholds[i]), want[i], 0,
                           thresholds[i], "end")
        except Exception as e:   # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def same(a, b):
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
    seqs = ["".join(rng.choice(list(_data.NCBI[:20]), size=int(L))) for L in rng.integers(1, 200, size=3000)]
    seqs[5] = _data.README_QUERY
    seqs[9] = _data.README_QUERY[:30]
    return pyopal_amd.Aligner(), pyopal_amd.Database(seqs), [_data.README_QUERY, _data.README_QUERY[5:40], "W", seqs[100]]


def test_aligner_hits(python_case):
    aligner, database, queries = python_case
    for mode in ("score", "end", "full"):
        for algo in ("sw", "nw"):
            for q in queries[:2]:
                everything = aligner.align(q, database, mode=mode, algorithm=algo)
                for threshold in thresholds_of(np.array([r.score for r in everything]))[1:]:
                    want = [r for r in everything if r.score >= threshold]
                    same(aligner.hits(q, database, threshold, mode=mode, algorithm=algo), want)
            part = aligner.align(queries[0], database, mode=mode, algorithm=algo, start=3, end=2500)
            threshold = thresholds_of(np.array([r.score for r in part]))[2]
            same(aligner.hits(queries[0], database, threshold, mode=mode, algorithm=algo, start=3, end=2500),
                 [r for r in part if r.score >= threshold])


def test_aligner_hits_sorted_equal_top_hits(python_case):
    aligner, database, queries = python_case
    for mode in ("score", "end", "full"):
        for q in queries:
            scores = np.array([r.score for r in aligner.align(q, database)])
            threshold = thresholds_of(scores)[2]
            count = int(np.count_nonzero(scores >= threshold))
            assert 0 < count <= 4096
            got = aligner.hits(q, database, threshold, mode=mode, sort=True)
            assert len(got) == count
            same(got, aligner.top_hits(q, database, min(count + 5, 4096), mode=mode, min_score=threshold))
    arrays = aligner.hits_arrays(queries[0], database, 10, mode="end", sort=True)
    assert np.all(np.diff(arrays["score"].astype(np.int64)) <= 0) and arrays["offsets"].tolist() == [0, len(arrays["score"])]


def test_aligner_hits_many(python_case):
    aligner, database, queries = python_case
    thresholds = []
    for q in queries:
        scores = np.array([r.score for r in aligner.align(q, database, start=3, end=2500)])
        thresholds.append(thresholds_of(scores)[2])
    for mode in ("score", "end", "full"):
        for sort in (False, True):
            many = aligner.hits_many(queries, database, thresholds, mode=mode, start=3, end=2500, sort=sort)
            assert len(many) == len(queries)
            for q, t, got in zip(queries, thresholds, many):
                assert len(got) > 0
                same(got, aligner.hits(q, database, t, mode=mode, start=3, end=2500, sort=sort))
    # one threshold for all, as a CSR of arrays
    csr = aligner.hits_many_arrays(queries, database, 12, mode="end")
    for i, q in enumerate(queries):
        want = aligner.hits(q, database, 12, mode="end")
        lo, hi = csr["offsets"][i], csr["offsets"][i + 1]
        assert csr["target"][lo:hi].tolist() == [r.target_index for r in want]
        assert csr["score"][lo:hi].tolist() == [r.score for r in want]
        assert csr["end_q"][lo:hi].tolist() == [r.query_end for r in want]
        assert csr["end_t"][lo:hi].tolist() == [r.target_end for r in want]


def test_aligner_hits_pssm(python_case, capi):
    import pyopal_amd
    aligner, database, queries = python_case
    pssm = pyopal_amd.Pssm.from_sequence(queries[0])
    for mode in ("full", "score"):
        for algo in ("sw", "hw"):
            everything = aligner.align_pssm(pssm, database, mode=mode, algorithm=algo)
            threshold = thresholds_of(np.array([r.score for r in everything]))[2]
            want = [r for r in everything if r.score >= threshold]
            assert want
            same(aligner.hits_pssm(pssm, database, threshold, mode=mode, algorithm=algo), want)
            same(aligner.hits_pssm(pssm, database, threshold, mode=mode, algorithm=algo, sort=True),
                 aligner.top_hits_pssm(pssm, database, len(want) + 1, mode=mode, algorithm=algo, min_score=threshold))
    with pytest.raises(capi.TooManyHits) as info:
        aligner.hits_pssm(pssm, database, threshold, algorithm="hw", max_hits=len(want) - 1)
    assert info.value.counts == len(want)
