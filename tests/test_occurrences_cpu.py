"""CPU tier of the occurrence searches (miopalSearchOccurrences, miopalSearchPssmOccurrences,
miopalLastOccurrenceRouting, the test hook miopalTestPickOccurrences; DeviceDatabase.search_occurrences /
search_occurrences_pssm / pick_occurrences_rows): the C ABI is declared, listed and
exported; with no handle the checks that need none come in their documented order; the hook refuses bad arguments
before any device call; the Python layer refuses what the C side refuses before it is reached; and the Python
restatement of the picker, the witness of the GPU tests, is pinned on rows worked out by hand."""
import ctypes
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from pyopal_amd import _capi

import _oracle
from _occurrences import INT_MAX, INT_MIN, column_values, expected_flat, flat_columns, pick, pick_rows, row_values
from pyopal_amd.matrices import ScoringMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE
NAMES = ("miopalSearchOccurrences", "miopalSearchPssmOccurrences", "miopalLastOccurrenceRouting", "miopalTestPickOccurrences")
HW, SW = 1, 3


def prototype(name):
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^)]*)\)", text)
    assert found, f"{name} is not declared"
    return re.sub(r"\s+", " ", found.group(1)).strip()


def test_header_declares_the_entry_points():
    tail = ("int64_t start, int64_t end, int minScore, int window, int64_t maxHits, int64_t* count, "
            "int64_t** targetIndex, int** score, int** endTarget, int** endQuery")
    assert prototype("miopalSearchOccurrences") == (
        "MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt, const int* scoreMatrix, "
        "int alphabetLength, int mode, " + tail)
    assert prototype("miopalSearchPssmOccurrences") == (
        "MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt, int alphabetLength, int mode, " + tail)
    assert prototype("miopalLastOccurrenceRouting") == "int64_t counts[4]"
    assert prototype("miopalTestPickOccurrences") == (
        "const int* value, const int* valueRow, int rows, int64_t stride, const int32_t* length, int minScore, "
        "int window, int64_t* hitOffsets, int32_t** column, int** score, int** row")
    for name in NAMES:
        assert name in _capi.EXPORTS
    for name in ("search_occurrences", "search_occurrences_pssm", "pick_occurrences_rows"):
        assert hasattr(_capi.DeviceDatabase, name)


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names
    lib = _capi.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    # the routing of a thread that has searched nothing (the counters are thread_local: asked from a fresh thread,
    # whatever this one has searched before)
    seen = []
    fresh = threading.Thread(target=lambda: seen.append(_capi.last_occurrence_routing()))
    fresh.start()
    fresh.join()
    assert seen == [[0, 0, 0, 0]]
    lib.miopalLastOccurrenceRouting(None)


class Outputs:
    """A count and four array pointers, all set to a mark that no refused call may change."""
    MARK = 0x77

    def __init__(self, n=4):
        self.count = np.full(3, 77, dtype=np.int64)
        self.ptrs = [ctypes.c_void_p(self.MARK) for _ in range(n)]

    def refs(self, missing=()):
        return [None if i in missing else ctypes.byref(p) for i, p in enumerate(self.ptrs)]

    def untouched(self):
        return np.all(self.count == 77) and all(p.value == self.MARK for p in self.ptrs)


def test_pssm_form_reports_argument_errors_before_a_device():
    """miopalSearchPssmOccurrences with no handle at all: miopalSearchPssmHits' order - mode range, query length, rows,
    alphabet; where that function refuses alignments the mode, the window and the SW cut; the outputs; the PSSM's
    height - and then the missing handle."""
    lib = _capi.lib()
    rows = np.ones((4, 32), dtype=np.int32)
    tall = np.ones((500, 32), dtype=np.int32)
    out = Outputs()

    def call(r=rows, q=4, alphabet=32, mode=HW, min_score=5, window=3, count=True, missing=(), max_hits=-1):
        return lib.miopalSearchPssmOccurrences(None, None if r is None else r.ctypes.data, q, 3, 1, alphabet, mode, 0, 2,
                                               min_score, window, max_hits,
                                               out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if count else None,
                                               *out.refs(missing))

    assert call(mode=4) == INVALID and "alignment mode" in _capi.last_error()
    assert call(mode=-1, q=-1) == INVALID and "alignment mode" in _capi.last_error()
    assert call(q=-1) == BAD and "query length" in _capi.last_error()
    assert call(q=-1, mode=0) == BAD and "query length" in _capi.last_error()
    assert call(r=None) == BAD and "null row scores" in _capi.last_error()
    assert call(alphabet=0) == BAD and "alphabet length" in _capi.last_error()
    assert call(alphabet=33, mode=2, window=-1) == BAD and "alphabet length" in _capi.last_error()
    # the occurrence rule: mode, then window, then the SW cut
    for mode in (0, 2):
        assert call(mode=mode, window=-1, min_score=0, count=False) == INVALID and "OPAL_MODE_HW and OPAL_MODE_SW" in _capi.last_error()
    assert call(window=-1, count=False) == BAD and "negative window" in _capi.last_error()
    assert call(mode=SW, window=-1, min_score=0) == BAD and "negative window" in _capi.last_error()
    for cut in (0, -3, INT_MIN):
        assert call(mode=SW, min_score=cut, count=False) == BAD and "at least 1" in _capi.last_error()
    # null outputs
    assert call(count=False) == BAD and "null count" in _capi.last_error()
    assert call(missing=(0,)) == BAD and "null target / score" in _capi.last_error()
    assert call(missing=(1,)) == BAD and "null target / score" in _capi.last_error()
    assert call(missing=(2,)) == BAD and "null end-location" in _capi.last_error()
    assert call(missing=(3,), r=tall, q=500) == BAD and "null end-location" in _capi.last_error()
    # a PSSM beyond the LDS table: 493 rows at 32 letters, 651 at 24
    assert call(r=tall, q=500) == BAD and "493 rows at most" in _capi.last_error()
    assert call(r=tall, q=494, mode=SW) == BAD and "does not fit" in _capi.last_error()
    assert call(r=tall, q=493) == BAD and "null database handle" in _capi.last_error()
    wide = np.ones((652, 24), dtype=np.int32)
    assert call(r=wide, q=652, alphabet=24) == BAD and "651 rows at most" in _capi.last_error()
    assert call(r=wide, q=651, alphabet=24) == BAD and "null database handle" in _capi.last_error()
    # nothing wrong with the arguments: the handle is what is missing
    for mode, cut, window, max_hits in ((HW, INT_MIN, 0, -1), (HW, 0, INT_MAX, 0), (SW, 1, 0, 2 ** 40), (SW, INT_MAX, 7, -5)):
        assert call(mode=mode, min_score=cut, window=window, max_hits=max_hits) == BAD and "null database handle" in _capi.last_error()
    assert call(r=None, q=0) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_plain_form_looks_at_the_handle_first():
    """miopalSearchOccurrences with no handle: miopalSearchHits' order - miopalSearch's checks begin with the handle, so
    every call is told that it is missing, whatever else is wrong."""
    lib = _capi.lib()
    query = np.zeros(4, dtype=np.uint8)
    matrix = np.ones(24 * 24, dtype=np.int32)
    out = Outputs()
    for mode, q, cut, window in ((HW, 4, 5, 3), (0, 4, 5, 3), (2, 4, 5, 3), (7, 4, 5, 3), (HW, -1, 5, 3), (HW, 4, 5, -1), (SW, 4, 0, 3)):
        rc = lib.miopalSearchOccurrences(None, query.ctypes.data, q, 3, 1, matrix.ctypes.data, 24, mode, 0, 2, cut, window, -1,
                                         out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), *out.refs())
        assert rc == BAD and "null database handle" in _capi.last_error(), (mode, q, cut, window)
    assert out.untouched()


def test_hook_refuses_bad_arguments_before_a_device():
    lib = _capi.lib()
    value = np.zeros((2, 8), dtype=np.int32)
    lengths = np.array([8, 3], dtype=np.int32)
    out = Outputs(3)

    def call(v=value, vr=None, rows=2, stride=8, length=lengths, window=1, offsets=True, missing=()):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.miopalTestPickOccurrences(ptr(v), ptr(vr), rows, stride, ptr(length), 0, window,
                                             out.count.ctypes.data if offsets else None, *out.refs(missing))

    for rows, stride in ((0, 8), (-1, 8), (2, 0), (2, -3)):
        assert call(rows=rows, stride=stride) == BAD and "both at least 1" in _capi.last_error()
    assert call(v=None) == BAD and "null value rows" in _capi.last_error()
    assert call(length=None) == BAD and "lengths" in _capi.last_error()
    assert call(offsets=False) == BAD and "null hitOffsets" in _capi.last_error()
    for k in range(3):
        assert call(missing=(k,)) == BAD and "null hitOffsets" in _capi.last_error()
    for rows, stride in ((2, 2 ** 26 + 1), (2 ** 27 + 1, 1), (1, 2 ** 27 + 1), (3, 2 ** 62)):
        assert call(rows=rows, stride=stride) == BAD and "more than 2^27" in _capi.last_error(), (rows, stride)
    for bad in ([9, 3], [8, -1], [-2 ** 31, 0]):
        assert call(length=np.array(bad, dtype=np.int32)) == BAD and "outside [0, 8]" in _capi.last_error()
    assert call(window=-1) == BAD and "negative window" in _capi.last_error()
    assert call(window=INT_MIN, vr=value) == BAD and "negative window" in _capi.last_error()
    assert out.untouched()
    # the Python wrapper checks the shapes
    with pytest.raises(ValueError, match="shape"):
        _capi.pick_occurrences_rows(np.zeros((2, 2, 2), dtype=np.int32), 2, 0, 0)
    with pytest.raises(ValueError, match="value_row"):
        _capi.pick_occurrences_rows(value, 8, 0, 0, value_row=np.zeros((2, 7), dtype=np.int32))


# ---- the picker's restatement, on rows worked out by hand -----------------------------------------------------------

def columns(values, min_score, window):
    return [j for j, _, _ in pick(values, min_score, window)]


def test_pick_a_plateau_keeps_its_first_column():
    assert pick([1, 5, 5, 5, 1], 5, 10) == [(1, 5, -1)]
    assert pick([5, 5, 5, 5], 5, 3) == [(0, 5, -1)]
    # ... and with window 0 every column at or above the cut is its own occurrence
    assert columns([1, 5, 5, 5, 1], 5, 0) == [1, 2, 3]
    assert columns([1, 5, 5, 5, 1], 1, 0) == [0, 1, 2, 3, 4]
    # a plateau longer than the window: a new candidate once the first is more than `window` behind
    assert columns([5] * 7, 5, 2) == [0, 3, 6]
    # rows travel with their columns
    assert pick([1, 5, 5], 5, 10, rows=[7, 8, 9]) == [(1, 5, 8)]


def test_pick_a_strictly_rising_row_gives_its_last_column():
    assert pick([1, 2, 3, 4, 5, 6], 1, 1) == [(5, 6, -1)]
    assert pick(list(range(100)), 0, 0 + 1) == [(99, 99, -1)]
    # (each column replaces the candidate before the window can run out; with window 0 nothing is replaced)
    assert columns([1, 2, 3, 4], 1, 0) == [0, 1, 2, 3]
    # below the cut nothing is a candidate
    assert pick([1, 2, 3], 4, 5) == []
    assert pick([], 0, 5) == []


def test_pick_a_strictly_falling_row_restarts_behind_the_window():
    values = [20, 19, 18, 17, 16, 15, 14, 13, 12, 11]
    assert columns(values, 1, 2) == [0, 3, 6, 9]
    assert [v for _, v, _ in pick(values, 1, 2)] == [20, 17, 14, 11]
    # the cut ends the series
    assert columns(values, 15, 2) == [0, 3]
    assert columns(values, 14, 2) == [0, 3, 6]


def test_pick_two_peaks_at_and_behind_the_window():
    w = 4
    at = [0, 9, 0, 0, 0, 9, 0, 0]          # exactly `window` apart: one occurrence, the first (ties keep the left)
    behind = [0, 9, 0, 0, 0, 0, 9, 0]      # window + 1 apart: two
    assert columns(at, 5, w) == [1]
    assert columns(behind, 5, w) == [1, 6]
    # a higher peak inside the window replaces the candidate, and the window then counts from IT
    assert columns([0, 8, 0, 0, 0, 9, 0, 0, 0, 8], 5, w) == [5]
    assert columns([0, 8, 0, 0, 0, 9, 0, 0, 0, 0, 8], 5, w) == [5, 10]
    # a lower peak inside the window is lost, one behind it is kept
    assert columns([0, 9, 0, 0, 0, 8, 0], 5, w) == [1]
    assert columns([0, 9, 0, 0, 0, 0, 8], 5, w) == [1, 6]
    # the extremes of the arguments
    assert columns(at, INT_MIN, INT_MAX) == [1]
    assert columns([INT_MIN, INT_MAX, INT_MIN], INT_MIN, 0) == [0, 1, 2]


def test_pick_rows_is_a_csr():
    value = np.array([[5, 0, 5, 0], [0, 0, 0, 0], [1, 2, 3, 4]])
    got = pick_rows(value, [4, 4, 2], 1, 0)
    assert got["offsets"].tolist() == [0, 2, 2, 4]
    assert got["column"].tolist() == [0, 2, 0, 1] and got["score"].tolist() == [5, 5, 1, 2] and got["row"].tolist() == [-1] * 4


# ---- the recurrence row by row: the witness of the long-target tests ------------------------------------------------

@pytest.mark.parametrize("alphabet", [2, 4, 24])
@pytest.mark.parametrize("gaps", [(3, 1), (11, 1), (2, 2), (5, 0), (0, 0), (1, 1)])
def test_row_values_is_column_values(gaps, alphabet):
    """values and rows, "hw" and "sw", queries of one row to three strips, targets of 0 .. 90 residues (0, 1 and a
    two-letter one among them)"""
    rng = np.random.default_rng(alphabet * 100 + gaps[0] * 10 + gaps[1])
    matrix = rng.integers(-6, 9, size=(alphabet, alphabet))
    lengths = [0, 1, 2, 63, 64, 65, 90] + rng.integers(0, 91, size=5).tolist()
    targets = [rng.integers(0, alphabet, size=n).astype(np.uint8) for n in lengths]
    targets.append(rng.integers(0, 2, size=80).astype(np.uint8))
    for q in (1, 7, 64, 65, 130):
        rows = matrix[rng.integers(0, alphabet, size=q)]
        for algorithm in ("hw", "sw"):
            V, R = column_values(rows, targets, gaps[0], gaps[1], algorithm)
            for k, t in enumerate(targets):
                v, r = row_values(rows, t, gaps[0], gaps[1], algorithm)
                assert v.shape == r.shape == (len(t),)
                assert np.array_equal(v, V[k, :len(t)]) and np.array_equal(r, R[k, :len(t)]), (q, algorithm, k)


def test_row_values_marks_the_ties_between_strips():
    """a column's maximum reached in two strips of 64 rows: worked by hand (every score 0 under "sw": every cell is 0,
    the smallest row 0, and every later strip ties), and none where the query is one strip"""
    target = np.zeros(9, dtype=np.uint8)
    for q, want in ((64, False), (65, True), (130, True)):
        tied = np.ones(9, dtype=bool)
        v, r = row_values(np.zeros((q, 2), dtype=np.int64), target, 3, 1, "sw", tied=tied)
        assert np.all(v == 0) and np.all(r == 0) and np.all(tied == want), q
    # a maximum that a later strip passes is no tie: row 70 alone scores
    rows = np.zeros((130, 2), dtype=np.int64)
    rows[70] = 5
    tied = np.ones(9, dtype=bool)
    v, r = row_values(rows, target, 3, 1, "sw", tied=tied)
    assert np.all(v == 5) and np.all(r == 70) and not tied.any()
    with pytest.raises(AssertionError):
        row_values(rows, target, 1, 2, "sw")


def test_flat_answers_are_the_per_target_rule():
    rng = np.random.default_rng(3)
    values = [rng.integers(-5, 6, size=n) for n in (7, 0, 1, 30)]
    rows = [rng.integers(0, 9, size=len(v)) for v in values]
    V, R, offsets = flat_columns(values, rows)
    assert offsets.tolist() == [0, 7, 7, 8, 38]
    for cut, window, first, last in ((0, 0, 0, 4), (-5, 0, 1, 4), (2, 3, 0, 4), (2, 0, 3, 4), (9, 0, 0, 4)):
        got = expected_flat(V, R, offsets, cut, window, first=first, last=last)
        want = [(k, v, j, r) for k in range(first, last) for j, v, r in pick(values[k], cut, window, rows[k])]
        assert list(zip(*(got[key].tolist() for key in ("target", "score", "end_t", "end_q")))) == want, (cut, window)
        assert got["target"].dtype == np.int64 and got["score"].dtype == np.int32


@pytest.mark.parametrize("q", [7, 65, 130])
def test_row_values_against_the_checker_at_read_length(q):
    """two targets of 5000 and 20 000 residues: the largest value, the first column that reaches it and its row are the
    C checker's score, end_t and end_q"""
    B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
    rng = np.random.default_rng(50 + q)
    query = rng.integers(0, 20, size=q).astype(np.uint8)
    targets = [rng.integers(0, 20, size=n).astype(np.uint8) for n in (5000, 20000)]
    residues, offsets = _oracle.flatten(targets)
    for gaps in ((11, 1), (2, 2)):
        for algorithm in ("hw", "sw"):
            want = _oracle.search(query, residues, offsets, B62, gaps[0], gaps[1], "end", algorithm)
            for k, t in enumerate(targets):
                v, r = row_values(B62.reshape(24, 24)[query], t, gaps[0], gaps[1], algorithm)
                j = int(np.argmax(v))   # (the first column that holds the maximum)
                assert (int(v[j]), j, int(r[j])) == (int(want["score"][k]), int(want["end_t"][k]), int(want["end_q"][k])), (
                    q, gaps, algorithm, k)


# ---- the Python layer -----------------------------------------------------------------------------------------------

class _NoHandle(_capi.DeviceDatabase):
    """a DeviceDatabase that owns no handle: what its methods refuse before they call the library"""

    def __init__(self, alphabet_length=24):
        self._h, self.count, self.alphabet_length = None, 3, alphabet_length


def test_python_refusals_come_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    db = _NoHandle()
    query = np.zeros(4, dtype=np.uint8)
    matrix = np.ones(24 * 24, dtype=np.int32)
    rows = np.ones((4, 24), dtype=np.int32)
    forms = (lambda **kw: db.search_occurrences(query, matrix, 3, 1, **kw),
             lambda **kw: db.search_occurrences_pssm(rows, 3, 1, **kw))
    for call in forms:
        for algorithm in ("nw", "ov", "blast"):
            with pytest.raises(ValueError, match="'hw' and 'sw'"):
                call(algorithm=algorithm, min_score=3)
        with pytest.raises(ValueError, match="window must not be negative"):
            call(min_score=3, window=-1)
        with pytest.raises(ValueError, match="window must not be negative"):
            call(algorithm="sw", min_score=0, window=-1)
        for cut in (0, -1, INT_MIN):
            with pytest.raises(ValueError, match="at least 1"):
                call(algorithm="sw", min_score=cut)
        # nothing wrong with these: the library is what they reach
        for kw in (dict(min_score=INT_MIN, window=0), dict(algorithm="sw", min_score=1), dict(min_score=0, window=INT_MAX)):
            with pytest.raises(AssertionError, match="device reached"):
                call(**kw)
    with pytest.raises(ValueError, match="row_scores must have shape"):
        db.search_occurrences_pssm(np.ones((4, 23), dtype=np.int32), 3, 1, min_score=3)


def test_the_hook_fails_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.pick_occurrences_rows(np.zeros((2, 8), dtype=np.int32), 8, 0, 0)
