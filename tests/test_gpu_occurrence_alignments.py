"""Where every occurrence starts, and its alignment (miopalSearchOccurrencesAligned, miopalSearchPssmOccurrencesAligned;
DeviceDatabase.search_occurrence_alignments / ..._pssm; pyopal_amd.find_occurrences). Witnesses: the occurrence search
itself for the first five arrays, the project's CPU checker where an occurrence is a target's best, and
tests/_occurrence_alignments.py - the start rule restated, pinned against the checker on the CPU - for every
occurrence."""
import ctypes
import functools

import numpy as np
import pytest

import _data
import _oracle
import _pssm
from _occurrence_alignments import operations, starts
from _occurrences import INT_MIN
from test_gpu_occurrences import GAPS, MATRICES, column_values, expected

import pyopal_amd
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
FIVE = ("target", "score", "end_t", "end_q")
QUERY_LENGTHS = (1, 53, 64, 65, 130)     # one row, the headline query, a strip, its edge, three strips
# per query length the suppression window of the helper test: short enough that most targets hold several occurrences,
# long enough that the helper's lanes (one per occurrence) stay a few thousand
WINDOWS = {1: 0, 53: 15, 64: 20, 65: 20, 130: 10}
TOO_MANY = 103
MATCH, DEL, INS, MISMATCH = 0, 1, 2, 3


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def occurrences_of(got):
    return list(zip(got["target"].tolist(), got["score"].tolist(), got["end_t"].tolist(), got["end_q"].tolist()))


def assert_alignments(got, rows, query, matrix, targets, gaps, algorithm, context, target_base=0):
    """starts and operations of every occurrence of `got` against the helper"""
    occ = [(t - target_base, s, j, r) for t, s, j, r in occurrences_of(got)]
    start_t, start_q = starts(rows, targets, occ, gaps[0], gaps[1], algorithm)
    assert got["start_t"].dtype == np.int32 and got["start_q"].dtype == np.int32
    assert np.array_equal(got["start_t"], start_t), (context, np.flatnonzero(got["start_t"] != start_t)[:8])
    assert np.array_equal(got["start_q"], start_q), (context, np.flatnonzero(got["start_q"] != start_q)[:8])
    want = operations(query, matrix, targets, occ, start_t, start_q, gaps[0], gaps[1])
    off = got["aln_off"]
    assert off.dtype == np.int64 and len(off) == len(occ) + 1 and off[0] == 0 and off[-1] == len(got["aln_flat"])
    assert np.array_equal(np.diff(off), [len(w) for w in want]), context
    flat = np.concatenate(want) if want else np.zeros(0, dtype=np.uint8)
    assert np.array_equal(got["aln_flat"], flat), (context, np.flatnonzero(got["aln_flat"] != flat)[:8])


# ---- the targets of the helper tests: 300 of 1 .. 300 residues per alphabet -------------------------------------------

@functools.lru_cache(maxsize=None)
def helper_set(name):
    matrix, alphabet = MATRICES[name]
    rng = np.random.default_rng(400 + alphabet)
    lengths = rng.integers(1, 301, size=300)
    edges = sorted({1, 2, 300} | {q + d for q in QUERY_LENGTHS for d in (-1, 0, 1) if q + d >= 1})
    lengths[:len(edges)] = edges
    rng.shuffle(lengths)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    return residues, offsets, targets, lengths


@pytest.fixture(scope="module")
def helper_dbs(capi):
    dbs = {}
    for name, (matrix, alphabet) in MATRICES.items():
        residues, offsets, _, _ = helper_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, alphabet)
    yield dbs
    for db in dbs.values():
        db.close()


def query_of(name, q):
    alphabet = MATRICES[name][1]
    return np.random.default_rng(2000 + q).integers(0, alphabet, size=q).astype(np.uint8)


def cut_of(algorithm):
    """the lowest cut there is: every column is a candidate under HW, every positive column maximum under SW"""
    return 1 if algorithm == "sw" else INT_MIN


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("q", QUERY_LENGTHS)
def test_every_occurrence_against_the_helper(helper_dbs, q, gaps, name):
    matrix, alphabet = MATRICES[name]
    _, _, targets, lengths = helper_set(name)
    query = query_of(name, q)
    rows = matrix.reshape(alphabet, alphabet)[query]
    for algorithm in ("hw", "sw"):
        V, R = column_values(rows, targets, gaps[0], gaps[1], algorithm)
        cut, window = cut_of(algorithm), WINDOWS[q]
        want = expected(V, R, lengths, cut, window)
        context = (algorithm, q, gaps, name)
        # not vacuous, by the recurrence alone: several occurrences in a third of the targets, occurrences that end in
        # column 0 and in the last column
        per_target = np.bincount(want["target"], minlength=len(lengths))
        assert (per_target >= 2).sum() * 3 >= len(lengths), (context, (per_target >= 2).sum())
        assert (want["end_t"] == 0).any() and (want["end_t"] == lengths[want["target"]] - 1).any(), context
        got = helper_dbs[name].search_occurrence_alignments(query, matrix, gaps[0], gaps[1], algorithm, min_score=cut,
                                                            window=window)
        assert got["count"] == len(want["target"]), context
        for key in FIVE:
            assert np.array_equal(got[key], want[key]), (context, key)
        assert_alignments(got, rows, query, matrix, targets, gaps, algorithm, context)
        routing = helper_dbs[name].last_occurrence_align_routing()
        assert routing[0] + routing[1] == got["count"] and routing[2] >= 1, (context, routing)
        assert routing[3] == (got["end_t"] - got["start_t"] + 1).max(), (context, routing)


# ---- planted copies among random residues: the anchor set -------------------------------------------------------------

@pytest.fixture(scope="module")
def anchor_set(capi):
    """300 targets of 1 .. 300 residues, a third of them with noisy copies of the queries' pieces planted"""
    rng = np.random.default_rng(78)
    queries = {q: _data.random_protein(rng, q) for q in (20, 70)}
    targets = []
    for k in range(300):
        t = _data.random_protein(rng, int(rng.integers(1, 301)))
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
def test_first_five_arrays_are_the_occurrence_searchs(anchor_set, q, algorithm):
    """byte for byte, whatever the window, with and without operations, plain and PSSM"""
    db, residues, offsets, targets, queries = anchor_set
    query = queries[q]
    rows = np.ascontiguousarray(B62.reshape(24, 24)[query])
    cut = 12 if algorithm == "sw" else -10
    for window in (0, q, 10 ** 6):
        want = db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut, window=window)
        sweeps = db.last_occurrence_routing()
        assert want["count"] > 30
        calls = [lambda ops: db.search_occurrence_alignments(query, B62, 11, 1, algorithm, min_score=cut, window=window,
                                                             operations=ops),
                 lambda ops: db.search_occurrence_alignments_pssm(rows, query, 11, 1, algorithm, min_score=cut,
                                                                  window=window, operations=ops)]
        answers = []
        for call in calls:
            for ops in (True, False):
                got = call(ops)
                assert got["count"] == want["count"] and db.last_occurrence_routing() == sweeps
                for key in FIVE:
                    assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (window, key)
                answers.append(got)
        # the PSSM of the matrix's rows with the query as its consensus gives the plain form's starts and operations
        for key in ("start_t", "start_q", "aln_off", "aln_flat"):
            assert np.array_equal(answers[0][key], answers[2][key]), (window, key)
        for got in answers[1::2]:
            assert np.array_equal(got["start_t"], answers[0]["start_t"]) and np.array_equal(got["start_q"], answers[0]["start_q"])


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
@pytest.mark.parametrize("q", [20, 70])
def test_anchor_against_the_checker(anchor_set, q, algorithm):
    """the occurrence at the checker's end cell of a target carries the checker's start and operations exactly"""
    db, residues, offsets, targets, queries = anchor_set
    query = queries[q]
    want = _oracle.search(query, residues, offsets, B62, 11, 1, "full", algorithm)
    scored = np.sort(want["score"])
    for cut in (max(int(scored[len(scored) // 2]), 1 if algorithm == "sw" else INT_MIN), max(int(scored[(len(scored) * 9) // 10]), 1)):
        above = np.flatnonzero(want["score"] >= cut)
        assert len(above) > 10
        for window in (0, q):
            got = db.search_occurrence_alignments(query, B62, 11, 1, algorithm, min_score=cut, window=window)
            where = {(t, j, r): k for k, (t, _, j, r) in enumerate(occurrences_of(got))}
            for t in above:
                k = where[(int(t), int(want["end_t"][t]), int(want["end_q"][t]))]
                context = (algorithm, q, cut, window, t)
                assert got["score"][k] == want["score"][t], context
                assert (got["start_t"][k], got["start_q"][k]) == (want["start_t"][t], want["start_q"][t]), context
                assert got["aln"][k].tolist() == want["aln"][t].tolist(), context


def test_anchor_degenerate_against_the_checker(capi):
    """every substitution -20 at 1/1, HW, a very negative cut: the checker's answer for every target is the gap over
    the query with an empty target span, and the occurrence at its end cell says the same"""
    rng = np.random.default_rng(4)
    matrix = np.full(24 * 24, -20, dtype=np.int32)
    lengths = np.concatenate([[1, 2, 63, 64, 65, 300], rng.integers(1, 301, size=294)])
    residues, offsets = _data.random_db(rng, lengths)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        for q in (7, 70):
            query = _data.random_protein(rng, q)
            want = _oracle.search(query, residues, offsets, matrix, 1, 1, "full", "hw")
            assert np.all(want["score"] == -q) and np.all(want["start_t"] == want["end_t"] + 1)
            got = db.search_occurrence_alignments(query, matrix, 1, 1, "hw", min_score=-10 ** 6, window=0)
            assert got["count"] == lengths.sum()
            where = {(t, j): k for k, (t, _, j, _) in enumerate(occurrences_of(got))}
            for t in range(len(lengths)):
                k = where[(t, int(want["end_t"][t]))]
                assert (got["score"][k], got["end_q"][k]) == (-q, q - 1)
                assert (got["start_t"][k], got["start_q"][k]) == (want["start_t"][t], 0), (q, t)
                assert got["aln"][k].tolist() == want["aln"][t].tolist() == [DEL] * q, (q, t)
            # ... and every other column is the same gap, one column further: the first 40 targets against the helper
            few = db.search_occurrence_alignments(query, matrix, 1, 1, "hw", 0, 40, min_score=-10 ** 6, window=0)
            assert few["count"] == lengths[:40].sum()
            assert_alignments(few, matrix.reshape(24, 24)[query], query, matrix, targets, (1, 1), "hw", ("degenerate", q))
    finally:
        db.close()


def test_planted_copies(capi):
    """random + exact copy + random + copy with one substitution and one deletion: the starts are the plant positions,
    the exact copy is Q matches"""
    rng = np.random.default_rng(9)
    self_score = lambda m: int(B62.reshape(24, 24)[m, m].sum())   # noqa: E731
    for q in (40, 53, 100):
        motif = _data.random_protein(rng, q)
        noisy = motif.copy()
        noisy[q // 3] = (noisy[q // 3] + 1) % 20                    # one substitution ...
        noisy = np.delete(noisy, 2 * q // 3)                        # ... and one deletion
        targets, plants = [], []
        for k in range(40):
            a, b, c = (_data.random_protein(rng, int(rng.integers(5, 90))) for _ in range(3))
            targets.append(np.concatenate([a, motif, b, noisy, c]).astype(np.uint8))
            plants.append((len(a), len(a) + q + len(b)))
        residues, offsets = _oracle.flatten(targets)
        db = capi.DeviceDatabase(residues, offsets, 24)
        try:
            cut = self_score(motif) - 40
            for algorithm in ("hw", "sw"):
                got = db.search_occurrence_alignments(motif, B62, 11, 1, algorithm, min_score=cut)
                assert got["count"] == 2 * len(targets) and got["target"].tolist() == sorted(list(range(40)) * 2)
                for k, (first, second) in enumerate(plants):
                    exact, other = 2 * k, 2 * k + 1
                    assert (got["start_t"][exact], got["end_t"][exact]) == (first, first + q - 1), (q, algorithm, k)
                    assert got["start_q"][exact] == 0 and got["end_q"][exact] == q - 1
                    assert got["score"][exact] == self_score(motif)
                    assert got["aln"][exact].tolist() == [MATCH] * q
                    assert (got["start_t"][other], got["end_t"][other]) == (second, second + q - 2), (q, algorithm, k)
                    ops = got["aln"][other].tolist()
                    assert ops.count(DEL) == 1 and ops.count(MISMATCH) == 1 and ops.count(INS) == 0 and len(ops) == q
        finally:
            db.close()


def test_starts_only(capi, anchor_set):
    """operations=False: the same starts, no operations, and the routing of a call with no direction work"""
    db, residues, offsets, targets, queries = anchor_set
    for q, algorithm, cut in ((20, "hw", -10), (70, "sw", 15)):
        query = queries[q]
        full = db.search_occurrence_alignments(query, B62, 11, 1, algorithm, min_score=cut, window=5)
        with_ops = db.last_occurrence_align_routing()
        only = db.search_occurrence_alignments(query, B62, 11, 1, algorithm, min_score=cut, window=5, operations=False)
        without = db.last_occurrence_align_routing()
        assert full["count"] > 300
        assert sorted(only) == ["count", "end_q", "end_t", "score", "start_q", "start_t", "target"]
        assert sorted(full) == sorted(list(only) + ["aln", "aln_flat", "aln_off"])
        for key in FIVE + ("start_t", "start_q"):
            assert only[key].tobytes() == full[key].tobytes(), (q, algorithm, key)
        assert with_ops[0] + with_ops[1] == full["count"] and with_ops[2] >= 1
        assert without[:2] == [0, 0] and without[2] >= 1 and without[3] == with_ops[3] > 1
        # through the C ABI: exactly one of the two operation outputs missing is refused, every output as it was
        lib = capi.lib()
        matrix = np.ascontiguousarray(B62)
        count = ctypes.c_int64(-7)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(8)]
        for missing in (6, 7):
            refs = [None if i == missing else ctypes.byref(p) for i, p in enumerate(ptrs)]
            rc = lib.miopalSearchOccurrencesAligned(db.handle, query.ctypes.data, len(query), 11, 1, matrix.ctypes.data, 24,
                                                    1, 0, len(targets), cut, 5, -1, ctypes.byref(count), *refs)
            assert rc == 101 and "both, or neither" in capi.last_error()
            assert count.value == -7 and all(p.value == 0x77 for p in ptrs)


def test_several_chunks(capi):
    """one 8000-residue repetitive target among short ones, window 0, a low cut, three strips of query: more
    occurrences than one chunk of the alignment stage holds. The chunks are invisible: the answer is that of the same
    call on single-target slices, and a handful of occurrences are the helper's."""
    rng = np.random.default_rng(12)
    query = _data.random_protein(rng, 130)
    unit = np.concatenate([query[20:70], _data.random_protein(rng, 11)])
    long_target = np.tile(unit, 8000 // len(unit) + 1)[:8000].astype(np.uint8)
    targets = [_data.random_protein(rng, int(n)) for n in rng.integers(1, 200, size=12)]
    targets.insert(5, long_target)
    residues, offsets = _oracle.flatten(targets)
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        got = db.search_occurrence_alignments(query, B62, 11, 1, "hw", min_score=-10 ** 6, window=0)
        routing = db.last_occurrence_align_routing()
        assert got["count"] == sum(len(t) for t in targets) > 8000
        assert routing[2] > 1 and routing[0] + routing[1] == got["count"]
        pieces = [db.search_occurrence_alignments(query, B62, 11, 1, "hw", k, k + 1, min_score=-10 ** 6, window=0)
                  for k in range(len(targets))]
        for key in FIVE + ("start_t", "start_q", "aln_flat"):
            assert np.array_equal(got[key], np.concatenate([p[key] for p in pieces])), key
        assert np.array_equal(np.diff(got["aln_off"]), np.concatenate([np.diff(p["aln_off"]) for p in pieces]))
        # a handful against the helper: both ends of the long target, and across it (a chunk holds 2774 occurrences)
        first = int(np.searchsorted(got["target"], 5))
        chosen = [0, first, first + 1, 2773, 2774, 5547, 5548, first + 7999, got["count"] - 1]
        few = {key: got[key][chosen] for key in FIVE + ("start_t", "start_q")}
        few["aln_flat"] = np.concatenate([got["aln"][k] for k in chosen])
        few["aln_off"] = np.concatenate([[0], np.cumsum([len(got["aln"][k]) for k in chosen])]).astype(np.int64)
        assert_alignments(few, B62.reshape(24, 24)[query], query, B62, targets, (11, 1), "hw", "several chunks")
        # starts only takes larger chunks, and gives the same starts
        only = db.search_occurrence_alignments(query, B62, 11, 1, "hw", min_score=-10 ** 6, window=0, operations=False)
        assert np.array_equal(only["start_t"], got["start_t"]) and np.array_equal(only["start_q"], got["start_q"])
        assert 1 <= db.last_occurrence_align_routing()[2] <= routing[2]
    finally:
        db.close()


def test_pssm_of_its_own_rows(capi):
    """100 rows that no matrix explains row by row (classes in random order): an ordinary search over the classes for
    the checker and the helper, a PSSM with the classes as its consensus for the library"""
    rng = np.random.default_rng(21)
    classes, matrix, rows = _pssm.class_pssm(rng, 100)
    lengths = np.maximum(_pssm.db_lengths(rng, 200, 150), 1)
    residues, offsets = _pssm.random_db(rng, lengths)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    db = capi.DeviceDatabase(residues, offsets, 32)
    try:
        for algorithm, cut, window in (("hw", -60, 10), ("sw", 20, 10)):
            got = db.search_occurrence_alignments_pssm(rows, classes, 3, 1, algorithm, min_score=cut, window=window)
            want = db.search_occurrences_pssm(rows, 3, 1, algorithm, min_score=cut, window=window)
            assert got["count"] == want["count"] > len(lengths) // 2   # (not vacuous: more than one in two targets)
            for key in FIVE:
                assert got[key].tobytes() == want[key].tobytes(), (algorithm, key)
            assert_alignments(got, rows, classes, matrix, targets, (3, 1), algorithm, ("pssm", algorithm))
            # without residues in the consensus nothing is a match, and the starts are the same
            blind = db.search_occurrence_alignments_pssm(rows, np.full(100, 255, dtype=np.uint8), 3, 1, algorithm,
                                                         min_score=cut, window=window)
            assert np.array_equal(blind["start_t"], got["start_t"]) and np.array_equal(blind["aln_off"], got["aln_off"])
            assert np.array_equal(blind["aln_flat"], np.where(got["aln_flat"] == MATCH, MISMATCH, got["aln_flat"]))
            only = db.search_occurrence_alignments_pssm(rows, None, 3, 1, algorithm, min_score=cut, window=window,
                                                        operations=False)
            assert np.array_equal(only["start_t"], got["start_t"]) and np.array_equal(only["start_q"], got["start_q"])
        with pytest.raises(RuntimeError, match="null consensus"):
            db.search_occurrence_alignments_pssm(rows, None, 3, 1, "hw", min_score=0)
    finally:
        db.close()


def test_contract(capi, anchor_set):
    db, residues, offsets, targets, queries = anchor_set
    query = queries[20]
    args = dict(algorithm="hw", min_score=-20, window=5)
    keys = FIVE + ("start_t", "start_q", "aln_off", "aln_flat")
    whole = db.search_occurrence_alignments(query, B62, 11, 1, **args)
    assert whole["count"] > 1000
    # a slice returns absolute indices, and what the whole database returns for its targets
    start, end = 123, 211
    part = db.search_occurrence_alignments(query, B62, 11, 1, start=start, end=end, **args)
    inside = (whole["target"] >= start) & (whole["target"] < end)
    assert part["count"] == inside.sum() > 0 and part["target"].min() >= start
    for key in FIVE + ("start_t", "start_q"):
        assert np.array_equal(part[key], whole[key][inside]), key
    lo, hi = whole["aln_off"][np.flatnonzero(inside)[0]], whole["aln_off"][np.flatnonzero(inside)[-1] + 1]
    assert np.array_equal(part["aln_flat"], whole["aln_flat"][lo:hi])
    # two calls return the same bytes
    again = db.search_occurrence_alignments(query, B62, 11, 1, **args)
    for key in keys:
        assert again[key].tobytes() == whole[key].tobytes(), key
    # an empty slice: checked, answered, nothing launched; the offsets hold their single 0
    got = db.search_occurrence_alignments(query, B62, 11, 1, start=40, end=40, **args)
    assert got["count"] == 0 and all(len(got[key]) == 0 for key in FIVE + ("start_t", "start_q", "aln_flat"))
    assert got["aln_off"].tolist() == [0] and len(got["aln"]) == 0
    assert db.last_occurrence_align_routing() == [0, 0, 0, 0] and db.last_occurrence_routing() == [0, 0, 0, 0]
    # ... and so does a cut nothing reaches
    got = db.search_occurrence_alignments(query, B62, 11, 1, algorithm="hw", min_score=10 ** 6)
    assert got["count"] == 0 and got["aln_off"].tolist() == [0] and db.last_occurrence_align_routing() == [0, 0, 0, 0]
    # maxHits, before any alignment: the count is filled, the pointers are as they were, no chunk has run
    lib = capi.lib()
    matrix = np.ascontiguousarray(B62)
    count = ctypes.c_int64(-7)
    ptrs = [ctypes.c_void_p(0x77) for _ in range(8)]
    rc = lib.miopalSearchOccurrencesAligned(db.handle, query.ctypes.data, len(query), 11, 1, matrix.ctypes.data, 24, 1, 0,
                                            len(targets), -20, 5, whole["count"] - 1, ctypes.byref(count),
                                            *[ctypes.byref(p) for p in ptrs])
    assert rc == TOO_MANY and count.value == whole["count"] and all(p.value == 0x77 for p in ptrs)
    assert db.last_occurrence_align_routing() == [0, 0, 0, 0]
    with pytest.raises(capi.TooManyHits) as info:
        db.search_occurrence_alignments(query, B62, 11, 1, max_hits=0, **args)
    assert info.value.counts == whole["count"]
    bounded = db.search_occurrence_alignments(query, B62, 11, 1, max_hits=whole["count"], **args)
    assert bounded["aln_flat"].tobytes() == whole["aln_flat"].tobytes()
    # the occurrence search itself is as it was
    plain = db.search_occurrences(query, B62, 11, 1, **args)
    for key in FIVE:
        assert plain[key].tobytes() == whole[key].tobytes(), key


def test_find_occurrences_objects_agree_with_the_arrays(capi, anchor_set):
    db, residues, offsets, targets, queries = anchor_set
    letters = _data.NCBI
    text = lambda codes: "".join(letters[c] for c in codes)   # noqa: E731
    aligner = pyopal_amd.Aligner("BLOSUM62", gap_open=11, gap_extend=1)
    database = pyopal_amd.Database([text(t) for t in targets])
    query = queries[20]
    for algorithm, cut in (("hw", 10), ("sw", 25)):
        want = db.search_occurrence_alignments(query, B62, 11, 1, algorithm, min_score=cut)
        arrays = pyopal_amd.find_occurrences_arrays(aligner, text(query), database, cut, algorithm=algorithm)
        assert arrays["count"] == want["count"] > 50
        for key in FIVE + ("start_t", "start_q", "aln_off", "aln_flat"):
            assert np.array_equal(arrays[key], want[key]), (algorithm, key)
        found = pyopal_amd.find_occurrences(aligner, text(query), database, cut, algorithm=algorithm)
        assert len(found) == want["count"] and all(isinstance(r, pyopal_amd.FullResult) for r in found)
        for k, r in enumerate(found):
            assert (r.target_index, r.score, r.target_end, r.query_end, r.target_start, r.query_start) == tuple(
                int(want[key][k]) for key in ("target", "score", "end_t", "end_q", "start_t", "start_q")), (algorithm, k)
            assert r.alignment == "".join("MDIX"[o] for o in want["aln"][k].tolist())
            assert r.query_length == 20 and r.target_length == len(targets[r.target_index])
        ends = pyopal_amd.find_occurrences(aligner, text(query), database, cut, algorithm=algorithm, mode="end")
        assert [type(r) for r in ends] == [pyopal_amd.EndResult] * want["count"]
        assert [(r.target_index, r.score, r.target_end, r.query_end) for r in ends] == [
            (r.target_index, r.score, r.target_end, r.query_end) for r in found]
        # the PSSM of the query gives the same objects; a slice and a window pass through; max_hits raises
        pssm = pyopal_amd.Pssm.from_sequence(text(query), "BLOSUM62")
        again = pyopal_amd.find_occurrences_pssm(aligner, pssm, database, cut, algorithm=algorithm)
        assert [(r.target_index, r.target_start, r.target_end, r.alignment) for r in again] == [
            (r.target_index, r.target_start, r.target_end, r.alignment) for r in found]
        part = pyopal_amd.find_occurrences(aligner, text(query), database, cut, algorithm=algorithm, start=50, end=90, window=3)
        ref = db.search_occurrence_alignments(query, B62, 11, 1, algorithm, 50, 90, min_score=cut, window=3)
        assert [(r.target_index, r.target_start) for r in part] == list(zip(ref["target"].tolist(), ref["start_t"].tolist()))
        with pytest.raises(capi.TooManyHits):
            pyopal_amd.find_occurrences(aligner, text(query), database, cut, algorithm=algorithm, max_hits=3)
