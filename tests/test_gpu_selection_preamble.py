"""The corners of the selection entry points that lie between their checks and their score pass (host_top.inc,
host_hits.inc, host_stats.inc, host.hip): where the 32-bit range check of a PSSM sits relative to the empty answers,
that the plain forms have no such check, what an error leaves of the outputs, and the assembly of the batch forms'
CSR from chunks and single-path queries with the bound on the total.

Eight targets of 4 to 12 residues over 32 letters, a PSSM of 5 rows and a copy with one entry of 2**30 that leaves
the 32-bit bound of score_ranges.h (the construction of tests/test_gpu_pssm_top_pairs.py). Every comparison is exact;
the witnesses are the single-query calls on the same handle, which the families' own files hold to the checker."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 32
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
SW = 3
LENGTHS = (4, 12, 7, 5, 9, 6, 11, 8)


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def case(capi):
    rng = np.random.default_rng(909)
    targets = [rng.integers(0, A, size=L).astype(np.uint8) for L in LENGTHS]
    offsets = np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)
    db = capi.DeviceDatabase(np.concatenate(targets), offsets, A)
    rows = rng.integers(-4, 7, size=(5, A)).astype(np.int32)
    huge = rows.copy()
    huge[2, 7] = 2 ** 30
    matrix = rng.integers(-4, 7, size=(A, A)).astype(np.int32)
    matrix[np.arange(A), np.arange(A)] += 5
    # 33 symbols fit the batch kernels' table up to 32 rows only (interseqPairFits): the query of 40 residues takes the
    # single-query path, its neighbours share a chunk
    queries = [np.concatenate([targets[1][:6], targets[4][:3]]), rng.integers(0, A, size=40).astype(np.uint8),
               targets[6][2:9].copy()]
    yield db, rows, huge, np.ascontiguousarray(matrix.ravel()), queries
    db.close()


def empty_fit(capi):
    fit = capi.ScoreFit()
    fit.degenerate = 1
    for b in range(capi.MIOPAL_STAT_BINS):
        fit.ceiling[b] = fit.threshold[b] = INT_MAX
    return bytes(fit)


# ---- the k best: the range check of the rows comes before "nothing to select" only where there is a slice -----------
def test_pssm_top_range_check_and_empty_answers(capi, case):
    db, rows, huge, matrix, queries = case
    lib = capi.lib()
    count = np.full(1, 77, dtype=np.int32)
    target = np.full(4, 77, dtype=np.int64)
    score = np.full(4, 77, dtype=np.int32)

    def top(r, k, start=0, end=len(LENGTHS)):
        return lib.miopalSearchPssmTop(db.handle, r.ctypes.data, len(r), 3, 1, A, 0, SW, start, end, k, INT_MIN,
                                       count.ctypes.data, target.ctypes.data, score.ctypes.data, None, None)

    assert top(huge, 0) == capi.OPAL_ERR_OVERFLOW and "32-bit range" in capi.last_error()
    assert count[0] == 77 and np.all(target == 77) and np.all(score == 77)
    assert top(rows, 0) == 0 and count[0] == 0
    assert np.all(target == 77) and np.all(score == 77)   # (k = 0: no entries)
    count[0] = 77
    assert top(huge, 4, start=3, end=3) == 0
    assert count[0] == 0 and np.all(target == -1) and np.all(score == -1)


def test_plain_top_has_no_range_check(capi, case):
    db, rows, huge, matrix, queries = case
    big = matrix.copy()
    big[5 * A + 9] = 2 ** 30
    count = np.full(1, 77, dtype=np.int32)
    q = queries[0]
    rc = capi.lib().miopalSearchTop(db.handle, q.ctypes.data, len(q), 3, 1, big.ctypes.data, A, 0, SW, 0, len(LENGTHS), 0,
                                    INT_MIN, count.ctypes.data, None, None, None, None)
    assert rc == 0 and count[0] == 0


# ---- hits and significant hits: the error leaves the outputs alone, the empty slice is answered before the check ----
def pssm_hits(capi, db, r, start, end, count, ptrs):
    return capi.lib().miopalSearchPssmHits(db.handle, r.ctypes.data, len(r), 3, 1, A, 0, SW, start, end, INT_MIN, -1,
                                           ctypes.byref(count), *[ctypes.byref(p) for p in ptrs])


def pssm_significant(capi, db, r, start, end, fit, count, ptrs, ev):
    return capi.lib().miopalSearchPssmSignificant(db.handle, r.ctypes.data, len(r), 3, 1, A, 0, SW, start, end, 1e9, 0.0,
                                                  -1, ctypes.addressof(fit), ctypes.byref(count),
                                                  *[ctypes.byref(p) for p in ptrs], ctypes.byref(ev))


def test_pssm_hits_range_check_and_empty_slice(capi, case):
    db, rows, huge, matrix, queries = case
    count = ctypes.c_int64(-9)
    ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
    assert pssm_hits(capi, db, huge, 0, len(LENGTHS), count, ptrs) == capi.OPAL_ERR_OVERFLOW
    assert "32-bit range" in capi.last_error()
    assert count.value == -9 and all(p.value == 0x55 for p in ptrs)
    assert pssm_hits(capi, db, huge, 3, 3, count, ptrs) == 0
    assert count.value == 0 and all(not p.value for p in ptrs)
    # (the handle is as it was)
    got = db.search_pssm_hits(rows, 3, 1, "score", "sw")
    assert got["count"] == len(LENGTHS)
    assert np.array_equal(got["score"], db.search_pssm(rows, None, 3, 1, "score", "sw")["score"])


def test_pssm_significant_range_check_and_empty_slice(capi, case):
    db, rows, huge, matrix, queries = case
    count = ctypes.c_int64(-9)
    ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
    ev = ctypes.c_void_p(0x55)
    fit = capi.ScoreFit()
    ctypes.memset(ctypes.addressof(fit), 0x55, ctypes.sizeof(fit))
    before = bytes(fit)
    assert pssm_significant(capi, db, huge, 0, len(LENGTHS), fit, count, ptrs, ev) == capi.OPAL_ERR_OVERFLOW
    assert "32-bit range" in capi.last_error()
    assert count.value == -9 and all(p.value == 0x55 for p in ptrs) and ev.value == 0x55 and bytes(fit) == before
    assert pssm_significant(capi, db, huge, 3, 3, fit, count, ptrs, ev) == 0
    assert count.value == 0 and all(not p.value for p in ptrs) and not ev.value
    assert bytes(fit) == empty_fit(capi)


# ---- the batch forms: chunk rows and a single-path query assembled in query order, and the bound on the total -------
def batch_arguments(queries):
    flat = np.concatenate(queries)
    offsets = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int64)
    return flat, offsets


def test_batch_hits_csr_and_bound(capi, case):
    db, rows, huge, matrix, queries = case
    thresholds = [2, 0, -3]
    for mode in ("score", "end"):
        singles = [db.search_hits(q, matrix, 3, 1, mode, "sw", min_score=t) for q, t in zip(queries, thresholds)]
        counts = [s["count"] for s in singles]
        total = sum(counts)
        assert total > 1 and counts[1] > 0
        got = db.search_batch_hits(queries, matrix, 3, 1, mode, "sw", min_score=thresholds, max_hits=total)
        routing = db.last_batch_routing()
        assert routing[2] == 1 and routing[0] + routing[1] == 2 * len(LENGTHS), routing
        assert np.diff(got["offsets"]).tolist() == counts and got["offsets"][0] == 0
        for key in ("target", "score") + (("end_t", "end_q") if mode == "end" else ()):
            assert np.array_equal(got[key], np.concatenate([s[key] for s in singles])), (mode, key)
        # one below the total: the offsets of every query, no arrays
        flat, offsets = batch_arguments(queries)
        t = np.array(thresholds, dtype=np.int32)
        hit_offsets = np.full(len(queries) + 1, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
        rc = capi.lib().miopalSearchBatchHits(db.handle, flat.ctypes.data, offsets.ctypes.data, len(queries), 3, 1,
                                              matrix.ctypes.data, A, capi.SEARCH[mode], SW, 0, len(LENGTHS),
                                              t.ctypes.data, total - 1, hit_offsets.ctypes.data,
                                              *[ctypes.byref(p) for p in ptrs])
        assert rc == capi.MIOPAL_ERR_TOO_MANY_HITS
        assert hit_offsets[0] == 0 and np.diff(hit_offsets).tolist() == counts
        assert all(p.value == 0x55 for p in ptrs)


def test_batch_significant_csr_and_bound(capi, case):
    db, rows, huge, matrix, queries = case
    # (a cut above the number of targets: every target of a row whose fit is not degenerate is a hit)
    for mode in ("score", "end"):
        singles = [db.search_significant(q, matrix, 3, 1, mode, "sw", max_evalue=1e9, exclude_z=0.0) for q in queries]
        counts = [s["count"] for s in singles]
        total = sum(counts)
        assert total > 1 and counts[1] > 0
        got = db.search_batch_significant(queries, matrix, 3, 1, mode, "sw", max_evalue=1e9, exclude_z=0.0, max_hits=total)
        routing = db.last_batch_routing()
        assert routing[2] == 1 and routing[0] + routing[1] == 2 * len(LENGTHS), routing
        assert np.diff(got["offsets"]).tolist() == counts and got["offsets"][0] == 0
        for key in ("target", "score", "evalue") + (("end_t", "end_q") if mode == "end" else ()):
            assert np.array_equal(got[key], np.concatenate([s[key] for s in singles])), (mode, key)
        for i, s in enumerate(singles):
            assert bytes(got["fits"][i]) == bytes(s["fit"]), (mode, i)
        # one below the total: the offsets and the fits of every query, no arrays
        flat, offsets = batch_arguments(queries)
        cuts = np.full(len(queries), 1e9, dtype=np.float64)
        fits = (capi.ScoreFit * len(queries))()
        hit_offsets = np.full(len(queries) + 1, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
        ev = ctypes.c_void_p(0x55)
        rc = capi.lib().miopalSearchBatchSignificant(db.handle, flat.ctypes.data, offsets.ctypes.data, len(queries), 3, 1,
                                                     matrix.ctypes.data, A, capi.SEARCH[mode], SW, 0, len(LENGTHS),
                                                     cuts.ctypes.data, 0.0, total - 1, ctypes.addressof(fits),
                                                     hit_offsets.ctypes.data, *[ctypes.byref(p) for p in ptrs],
                                                     ctypes.byref(ev))
        assert rc == capi.MIOPAL_ERR_TOO_MANY_HITS
        assert hit_offsets[0] == 0 and np.diff(hit_offsets).tolist() == counts
        assert all(p.value == 0x55 for p in ptrs) and ev.value == 0x55
        for i, s in enumerate(singles):
            assert bytes(fits[i]) == bytes(s["fit"]), (mode, i)
