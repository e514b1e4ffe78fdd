"""Every occurrence of a query in each target, picked on the device (miopalSearchOccurrences,
miopalSearchPssmOccurrences; DeviceDatabase.search_occurrences / search_occurrences_pssm). Three witnesses: a numpy
statement of the recurrence (tests/_occurrences.column_values) that returns every column's value and row; the project's
CPU checker on prefixes and on whole targets; and tests/_occurrences.pick, the rule itself."""
import ctypes
import functools

import numpy as np
import pytest

import _data
import _oracle
import _pssm
from _occurrences import INT_MIN, column_values, pick   # noqa: F401 (column_values: other modules import it from here)
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
R32 = np.random.default_rng(32).integers(-8, 13, size=32 * 32).astype(np.int32)   # 32 letters, asymmetric
MATRICES = {"blosum62": (B62, 24), "random32": (R32, 32)}
QUERY_LENGTHS = (1, 7, 64, 65, 130)      # one strip, its edge, two strips, three strips
GAPS = ((3, 1), (11, 1), (2, 2))
TOO_MANY = 103


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def expected(V, R, lengths, min_score, window, start=0):
    """`pick` over every target's columns -> the four arrays of an answer"""
    out = [(start + k, v, j, r) for k in range(len(lengths)) for j, v, r in pick(V[k, :lengths[k]], min_score, window, R[k])]
    table = np.array(out, dtype=np.int64).reshape(-1, 4)
    return {"target": table[:, 0], "score": table[:, 1].astype(np.int32), "end_t": table[:, 2].astype(np.int32),
            "end_q": table[:, 3].astype(np.int32)}


def assert_answer(got, want, context):
    assert got["count"] == len(want["target"]), (context, got["count"], len(want["target"]))
    for key in ("target", "score", "end_t", "end_q"):
        assert got[key].dtype == want[key].dtype, (context, key)
        assert np.array_equal(got[key], want[key]), (context, key, np.flatnonzero(got[key] != want[key])[:8])


# ---- 1, 2: every column value, against the recurrence and against the checker on prefixes ---------------------------

@functools.lru_cache(maxsize=None)
def column_set(name):
    """300 targets of 0 .. 200 residues, shuffled, every length next to a query length among them"""
    matrix, alphabet = MATRICES[name]
    rng = np.random.default_rng(100 + alphabet)
    lengths = rng.integers(0, 201, size=300)
    edges = sorted({0, 1, 200} | {q + d for q in QUERY_LENGTHS for d in (-1, 0, 1)})
    lengths[:len(edges)] = edges
    rng.shuffle(lengths)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    return residues, offsets, targets, lengths


@pytest.fixture(scope="module")
def column_dbs(capi):
    dbs = {}
    for name, (matrix, alphabet) in MATRICES.items():
        residues, offsets, _, _ = column_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, alphabet)
    yield dbs
    for db in dbs.values():
        db.close()


def query_of(name, q):
    alphabet = MATRICES[name][1]
    return np.random.default_rng(1000 + q).integers(0, alphabet, size=q).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def witness(name, q, gaps, algorithm):
    matrix, alphabet = MATRICES[name]
    _, _, targets, _ = column_set(name)
    return column_values(matrix.reshape(alphabet, alphabet)[query_of(name, q)], targets, gaps[0], gaps[1], algorithm)


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("q", QUERY_LENGTHS)
def test_every_column_value(column_dbs, q, gaps, name):
    """window = 0 returns every column at or above the cut: with the cut at INT_MIN (HW) every value of the last row,
    at 1 (SW) every positive column maximum and its row - all of them equal to the recurrence's"""
    matrix, alphabet = MATRICES[name]
    _, _, _, lengths = column_set(name)
    query = query_of(name, q)
    for algorithm, cut in (("hw", INT_MIN), ("sw", 1)):
        V, R = witness(name, q, gaps, algorithm)
        got = column_dbs[name].search_occurrences(query, matrix, gaps[0], gaps[1], algorithm, min_score=cut, window=0)
        want = expected(V, R, lengths, cut, 0)
        assert_answer(got, want, (algorithm, q, gaps, name))
        if algorithm == "hw":
            assert got["count"] == lengths.sum() and np.all(got["end_q"] == q - 1)
        else:
            assert 0 < got["count"] <= lengths.sum() and got["score"].min() >= 1
        assert column_dbs[name].last_occurrence_routing()[3] == (q + 63) // 64


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("q", QUERY_LENGTHS)
def test_running_maximum_is_the_checkers_score_of_the_prefix(column_dbs, q, gaps, name):
    """held to the project's checker: the best value up to column j of a target is the checker's score of the target's
    first j + 1 residues - 20 targets and all their prefixes, as a database of their own"""
    matrix, alphabet = MATRICES[name]
    _, offsets, targets, lengths = column_set(name)
    query = query_of(name, q)
    chosen = np.argsort(-lengths, kind="stable")[::15][:20]
    prefixes = [targets[k][:j + 1] for k in chosen for j in range(lengths[k])]
    residues, prefix_offsets = _oracle.flatten(prefixes)
    for algorithm, cut in (("hw", INT_MIN), ("sw", 1)):
        got = column_dbs[name].search_occurrences(query, matrix, gaps[0], gaps[1], algorithm, min_score=cut, window=0)
        want = _oracle.search(query, residues, prefix_offsets, matrix, gaps[0], gaps[1], "score", algorithm)["score"]
        at = 0
        for k in chosen:
            values = np.zeros(lengths[k], dtype=np.int64) if algorithm == "sw" else np.full(lengths[k], INT_MIN, dtype=np.int64)
            mine = got["target"] == k
            values[got["end_t"][mine]] = got["score"][mine]   # (SW: the columns below the cut hold 0)
            running = np.maximum.accumulate(values)
            assert np.array_equal(running, want[at:at + lengths[k]]), (algorithm, q, gaps, name, k)
            at += lengths[k]
        assert at == len(want) and at > 1000


# ---- 3: the anchor property -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def anchor_set(capi):
    """400 targets of 0 .. 300 residues, a third of them with noisy copies of the query's pieces planted"""
    rng = np.random.default_rng(77)
    queries = {q: _data.random_protein(rng, q) for q in (20, 70)}
    targets = []
    for k in range(400):
        t = _data.random_protein(rng, int(rng.integers(0, 301)))
        if k % 3 == 0 and len(t) > 80:
            for q in queries.values():
                for _ in range(int(rng.integers(1, 4))):
                    piece = np.array(_data.mutate(rng, q, 0.1), dtype=np.uint8)
                    at = int(rng.integers(0, len(t) - len(piece))) if len(t) > len(piece) else 0
                    t = np.concatenate([t[:at], piece, t[at + len(piece):]])[:300]
        targets.append(np.asarray(t, dtype=np.uint8))
    residues, offsets = _oracle.flatten(targets)
    db = capi.DeviceDatabase(residues, offsets, 24)
    yield db, residues, offsets, targets, queries
    db.close()


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
@pytest.mark.parametrize("q", [20, 70])
def test_anchor_property(anchor_set, q, algorithm):
    db, residues, offsets, targets, queries = anchor_set
    query = queries[q]
    lengths = np.diff(offsets)
    want = _oracle.search(query, residues, offsets, B62, 11, 1, "end", algorithm)
    V, R = column_values(B62.reshape(24, 24)[query], targets, 11, 1, algorithm)
    scored = np.sort(want["score"][lengths > 0])
    cuts = [max(int(scored[len(scored) // 2]), 1 if algorithm == "sw" else INT_MIN), max(int(scored[(len(scored) * 9) // 10]), 1)]
    assert cuts[0] < cuts[1]
    for cut in cuts:
        above = (want["score"] >= cut) & (lengths > 0)
        assert 10 < above.sum() < len(lengths)
        for window in (0, q, 1000):
            got = db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut, window=window)
            context = (algorithm, q, cut, window)
            # a target scoring below the cut has none; the others hold the checker's best location, their maximum
            assert set(got["target"].tolist()) == set(np.flatnonzero(above).tolist()), context
            for k in np.flatnonzero(above):
                mine = np.flatnonzero(got["target"] == k)
                found = list(zip(got["score"][mine].tolist(), got["end_t"][mine].tolist(), got["end_q"][mine].tolist()))
                assert (int(want["score"][k]), int(want["end_t"][k]), int(want["end_q"][k])) in found, (context, k)
                assert got["score"][mine].max() == want["score"][k], (context, k)
                assert np.all(np.diff(got["end_t"][mine]) > window), (context, k)
            # order: targets ascending, columns ascending inside a target
            assert np.all(np.diff(got["target"]) >= 0)
            # ... and the whole answer is the rule's over the recurrence's values
            assert_answer(got, expected(V, R, lengths, cut, window), context)
            if window == 1000:
                assert got["count"] == above.sum()   # (no target is longer than the window: one each)


# ---- 4: planted copies ----------------------------------------------------------------------------------------------

def test_planted_copies(capi):
    rng = np.random.default_rng(8)
    motif = _data.random_protein(rng, 20)
    window = 40
    target = _data.random_protein(rng, 600)
    # three copies more than `window` apart, then two with 8 residues between them (their ends 28 columns apart)
    starts = [30, 150, 300, 450, 478]
    for at in starts:
        target[at:at + 20] = motif
    others = [_data.random_protein(rng, n) for n in (0, 19, 20, 600)]
    residues, offsets = _oracle.flatten([others[0], others[1], target, others[2], others[3]])
    self_score = int(B62.reshape(24, 24)[motif, motif].sum())
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        got = db.search_occurrences(motif, B62, 11, 1, "hw", min_score=self_score - 1, window=window)
        V, R = column_values(B62.reshape(24, 24)[motif], [target], 11, 1, "hw")
        want = pick(V[0], self_score - 1, window, R[0])
        assert [j for j, _, _ in want] == [at + 19 for at in starts[:4]]
        assert got["count"] == 4 and got["target"].tolist() == [2] * 4
        assert got["end_t"].tolist() == [j for j, _, _ in want] and got["score"].tolist() == [self_score] * 4
        assert got["end_q"].tolist() == [19] * 4
        # with a window shorter than their distance the last two copies are two occurrences
        got = db.search_occurrences(motif, B62, 11, 1, "hw", min_score=self_score - 1, window=27)
        assert got["end_t"].tolist() == [at + 19 for at in starts]
        # the default window is the query's length
        got = db.search_occurrences(motif, B62, 11, 1, "hw", min_score=self_score - 1)
        assert got["end_t"].tolist() == [at + 19 for at in starts]
    finally:
        db.close()


# ---- 5: the contract ------------------------------------------------------------------------------------------------

def test_contract(capi, anchor_set):
    db, residues, offsets, targets, queries = anchor_set
    query, lengths = queries[20], np.diff(offsets)
    whole = db.search_occurrences(query, B62, 11, 1, "hw", min_score=-20, window=5)
    routing = db.last_occurrence_routing()
    assert whole["count"] > 1000
    assert routing == [len(lengths), len(set(whole["target"].tolist())), 2, 1]
    assert routing[1] < routing[0]   # (empty targets and targets below the cut are not swept twice)
    # a slice returns absolute indices, and what the whole database returns for its targets
    start, end = 123, 311
    part = db.search_occurrences(query, B62, 11, 1, "hw", start, end, -20, 5)
    inside = (whole["target"] >= start) & (whole["target"] < end)
    assert part["count"] == inside.sum() > 0 and part["target"].min() >= start
    for key in ("target", "score", "end_t", "end_q"):
        assert np.array_equal(part[key], whole[key][inside]), key
    assert db.last_occurrence_routing()[0] == end - start
    # two calls return the same bytes
    again = db.search_occurrences(query, B62, 11, 1, "hw", min_score=-20, window=5)
    for key in ("target", "score", "end_t", "end_q"):
        assert again[key].tobytes() == whole[key].tobytes(), key
    # an empty slice: checked, answered, nothing launched
    got = db.search_occurrences(query, B62, 11, 1, "hw", 40, 40, -20, 5)
    assert got["count"] == 0 and all(len(got[key]) == 0 for key in ("target", "score", "end_t", "end_q"))
    assert db.last_occurrence_routing() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="bad slice"):
        db.search_occurrences(query, B62, 11, 1, "hw", 41, 40, -20, 5)
    # maxHits: the count is filled, the pointers are as they were, the handle works afterwards
    lib = capi.lib()
    matrix = np.ascontiguousarray(B62)
    count = ctypes.c_int64(-7)
    ptrs = [ctypes.c_void_p(0x77) for _ in range(4)]
    rc = lib.miopalSearchOccurrences(db.handle, query.ctypes.data, len(query), 11, 1, matrix.ctypes.data, 24, 1, 0,
                                     len(lengths), -20, 5, whole["count"] - 1, ctypes.byref(count),
                                     *[ctypes.byref(p) for p in ptrs])
    assert rc == TOO_MANY and count.value == whole["count"] and all(p.value == 0x77 for p in ptrs)
    assert "maxHits" in capi.last_error()
    with pytest.raises(capi.TooManyHits) as info:
        db.search_occurrences(query, B62, 11, 1, "hw", min_score=-20, window=5, max_hits=0)
    assert info.value.counts == whole["count"]
    bounded = db.search_occurrences(query, B62, 11, 1, "hw", min_score=-20, window=5, max_hits=whole["count"])
    assert bounded["count"] == whole["count"] and np.array_equal(bounded["end_t"], whole["end_t"])
    # other errors leave every output as it was: NW is refused, a negative window, SW without a cut
    for mode, cut, window, code in ((0, 5, 5, capi.OPAL_ERR_INVALID_MODE), (2, 5, 5, capi.OPAL_ERR_INVALID_MODE), (1, 5, -1, 101), (3, 0, 5, 101)):
        rc = lib.miopalSearchOccurrences(db.handle, query.ctypes.data, len(query), 11, 1, matrix.ctypes.data, 24, mode, 0,
                                         len(lengths), cut, window, -1, ctypes.byref(count), *[ctypes.byref(p) for p in ptrs])
        assert rc == code and count.value == whole["count"] and all(p.value == 0x77 for p in ptrs), (mode, cut, window)
    # an empty query has no occurrences
    got = db.search_occurrences(np.zeros(0, dtype=np.uint8), B62, 11, 1, "hw", min_score=INT_MIN, window=0)
    assert got["count"] == 0 and len(got["target"]) == 0


def test_range_check_is_the_plain_searchs(capi):
    """32-bit arithmetic only: what miopalSearch refuses with OPAL_ERR_OVERFLOW is refused here"""
    rng = np.random.default_rng(2)
    residues, offsets = _data.random_db(rng, [50, 60])
    huge = np.full(24 * 24, 2 ** 26, dtype=np.int32)
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        query = _data.random_protein(rng, 70)
        with pytest.raises(OverflowError):
            db.search(query, huge, 3, 1, "end", "hw")
        with pytest.raises(OverflowError):
            db.search_occurrences(query, huge, 3, 1, "hw", min_score=0, window=0)
        assert db.search_occurrences(query, B62, 3, 1, "sw", min_score=1, window=0)["count"] > 0
    finally:
        db.close()


def test_strip_workspace_limit_is_stated(capi):
    """a query of more than 64 rows against a handle whose longest target passes one wavefront's share of the strip
    workspace (2 097 152 columns under SW, twice that under HW) is refused with a message, before any launch"""
    rng = np.random.default_rng(6)
    residues, offsets = _data.random_db(rng, [2_097_153, 40])
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        tall, short = _data.random_protein(rng, 65), _data.random_protein(rng, 64)
        with pytest.raises(RuntimeError, match="2097153 residues.*2097152 residues at most"):
            db.search_occurrences(tall, B62, 11, 1, "sw", min_score=30)
        assert db.last_occurrence_routing()[:3] == [0, 0, 0]
        with pytest.raises(RuntimeError, match="at most"):
            db.search_occurrences_pssm(B62.reshape(24, 24)[tall], 11, 1, "sw", min_score=30)
        # an empty slice is answered as ever, and the handle works afterwards
        assert db.search_occurrences(tall, B62, 11, 1, "sw", 1, 1, min_score=30)["count"] == 0
        assert db.search(short, B62, 11, 1, "score", "sw", 1, 2)["score"].shape == (1,)
    finally:
        db.close()


# ---- 6: position-specific scoring matrices --------------------------------------------------------------------------

def test_pssm_rows_of_a_matrix_give_the_plain_answer(anchor_set):
    db, residues, offsets, targets, queries = anchor_set
    for q, algorithm, cut, window in ((20, "hw", 0, 20), (70, "hw", -40, 0), (70, "sw", 25, 70), (20, "sw", 1, 3)):
        query = queries[q]
        want = db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut, window=window)
        routing = db.last_occurrence_routing()
        got = db.search_occurrences_pssm(B62.reshape(24, 24)[query], 11, 1, algorithm, min_score=cut, window=window)
        assert want["count"] > 0 and got["count"] == want["count"]
        for key in ("target", "score", "end_t", "end_q"):
            assert np.array_equal(got[key], want[key]), (q, algorithm, key)
        assert db.last_occurrence_routing() == routing


def test_pssm_of_its_own_rows(capi):
    """100 rows that no matrix explains row by row (classes in random order), against the recurrence; and the limit"""
    rng = np.random.default_rng(19)
    classes, matrix, rows = _pssm.class_pssm(rng, 100)
    lengths = _pssm.db_lengths(rng, 200, 150)
    residues, offsets = _pssm.random_db(rng, lengths)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    db = capi.DeviceDatabase(residues, offsets, 32)
    try:
        for algorithm, cut, window in (("hw", INT_MIN, 0), ("hw", -60, 100), ("sw", 1, 0), ("sw", 30, 10)):
            V, R = column_values(rows, targets, 3, 1, algorithm)
            got = db.search_occurrences_pssm(rows, 3, 1, algorithm, min_score=cut, window=window)
            assert_answer(got, expected(V, R, lengths, cut, window), (algorithm, cut, window))
            assert got["count"] > 50 and db.last_occurrence_routing()[3] == 2
        # the table of the sweep holds 493 rows at 32 letters
        tall = np.ascontiguousarray(np.tile(rows, (5, 1)))
        assert tall.shape == (500, 32)
        with pytest.raises(RuntimeError, match="500 rows at 32 letters does not fit.*493 rows at most"):
            db.search_occurrences_pssm(tall, 3, 1, "hw", min_score=0, window=0)
        # ... and 493 rows run (eight strips)
        got = db.search_occurrences_pssm(tall[:493], 3, 1, "sw", 0, 40, min_score=40, window=493)
        V, R = column_values(tall[:493], targets[:40], 3, 1, "sw")
        assert_answer(got, expected(V, R, lengths[:40], 40, 493), "493 rows")
    finally:
        db.close()


# ---- 7: the Python layer --------------------------------------------------------------------------------------------

def test_python_layer(capi, anchor_set):
    """`window=None` is the query's length, for both forms; the dict's keys and dtypes"""
    db, residues, offsets, targets, queries = anchor_set
    for q, algorithm, cut in ((20, "hw", 30), (70, "sw", 40)):
        query = queries[q]
        rows = B62.reshape(24, 24)[query]
        want = db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut, window=q)
        assert want["count"] > 20 and want["count"] > len(set(want["target"].tolist()))   # (several per target)
        assert sorted(want) == ["count", "end_q", "end_t", "score", "target"]
        assert want["target"].dtype == np.int64 and all(want[key].dtype == np.int32 for key in ("score", "end_t", "end_q"))
        other = db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut, window=q - 1)
        assert other["count"] >= want["count"]
        for got in (db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut),
                    db.search_occurrences_pssm(rows, 11, 1, algorithm, min_score=cut)):
            assert got["count"] == want["count"]
            for key in ("target", "score", "end_t", "end_q"):
                assert np.array_equal(got[key], want[key]), (q, algorithm, key)
    with pytest.raises(ValueError, match="at least 1"):
        db.search_occurrences(queries[20], B62, 11, 1, "sw", min_score=0)
