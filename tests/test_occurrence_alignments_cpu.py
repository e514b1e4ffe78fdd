"""CPU tier of the aligned occurrence search (miopalSearchOccurrencesAligned, miopalSearchPssmOccurrencesAligned,
miopalLastOccurrenceAlignRouting; DeviceDatabase.search_occurrence_alignments / ..._pssm; pyopal_amd.find_occurrences
and its forms): the C ABI is declared, listed and exported; with no handle the checks that need none come in their
documented order, the new null-output rules among them; the Python layers refuse what they must before any device call
and answer empty requests without one; and the witness of the GPU tests (tests/_occurrence_alignments.py) is pinned
against the C checker and on two cases worked out by hand."""
import ctypes
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import _capi
from pyopal_amd.matrices import ScoringMatrix

import _data
import _oracle
from _occurrence_alignments import border, operations, starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE
NAMES = ("miopalSearchOccurrencesAligned", "miopalSearchPssmOccurrencesAligned", "miopalLastOccurrenceAlignRouting")
HW, SW = 1, 3
B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)


def prototype(name):
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^)]*)\)", text)
    assert found, f"{name} is not declared"
    return re.sub(r"\s+", " ", found.group(1)).strip()


def test_header_declares_the_entry_points():
    tail = ("int64_t start, int64_t end, int minScore, int window, int64_t maxHits, int64_t* count, "
            "int64_t** targetIndex, int** score, int** endTarget, int** endQuery, int** startTarget, int** startQuery, "
            "unsigned char** alignments, int64_t** alignmentOffsets")
    assert prototype("miopalSearchOccurrencesAligned") == (
        "MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt, const int* scoreMatrix, "
        "int alphabetLength, int mode, " + tail)
    assert prototype("miopalSearchPssmOccurrencesAligned") == (
        "MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength, int gapOpen, int gapExt, "
        "int alphabetLength, int mode, " + tail)
    assert prototype("miopalLastOccurrenceAlignRouting") == "int64_t counts[4]"
    for name in NAMES:
        assert name in _capi.EXPORTS
    for name in ("search_occurrence_alignments", "search_occurrence_alignments_pssm", "last_occurrence_align_routing"):
        assert hasattr(_capi.DeviceDatabase, name)
    # the header no longer lists the other end of an occurrence as missing
    header = open(os.path.join(ROOT, "include", "miopal.h")).read()
    assert "Not part of this call: the start locations and operations" not in header


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names
    lib = _capi.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.miopalSearchOccurrencesAligned.argtypes) == 22
    assert len(lib.miopalSearchPssmOccurrencesAligned.argtypes) == 22
    # the routing of a thread that has searched nothing (the counters are thread_local: asked from a fresh thread,
    # whatever this one has searched before)
    seen = []
    fresh = threading.Thread(target=lambda: seen.append(_capi.last_occurrence_align_routing()))
    fresh.start()
    fresh.join()
    assert seen == [[0, 0, 0, 0]]
    lib.miopalLastOccurrenceAlignRouting(None)


class Outputs:
    """A count and eight array pointers (target, score, endT, endQ, startT, startQ, alignments, offsets), all set to a
    mark that no refused call may change."""
    MARK = 0x77

    def __init__(self):
        self.count = np.full(3, 77, dtype=np.int64)
        self.ptrs = [ctypes.c_void_p(self.MARK) for _ in range(8)]

    def refs(self, missing=()):
        return [None if i in missing else ctypes.byref(p) for i, p in enumerate(self.ptrs)]

    def untouched(self):
        return np.all(self.count == 77) and all(p.value == self.MARK for p in self.ptrs)


def test_pssm_form_reports_argument_errors_before_a_device():
    """miopalSearchPssmOccurrencesAligned with no handle at all: miopalSearchPssmOccurrences' order - mode range, query
    length, rows, alphabet; the occurrence rule; its outputs - then the new outputs, the consensus, the PSSM's height,
    and the missing handle last."""
    lib = _capi.lib()
    rows = np.ones((4, 32), dtype=np.int32)
    tall = np.ones((500, 32), dtype=np.int32)
    cons = np.zeros(500, dtype=np.uint8)
    out = Outputs()

    def call(r=rows, c=cons, q=4, alphabet=32, mode=HW, min_score=5, window=3, count=True, missing=()):
        return lib.miopalSearchPssmOccurrencesAligned(
            None, None if r is None else r.ctypes.data, None if c is None else c.ctypes.data, q, 3, 1, alphabet, mode, 0, 2,
            min_score, window, -1, out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if count else None,
            *out.refs(missing))

    assert call(mode=4) == INVALID and "alignment mode" in _capi.last_error()
    assert call(q=-1, missing=(6,)) == BAD and "query length" in _capi.last_error()
    assert call(r=None) == BAD and "null row scores" in _capi.last_error()
    assert call(alphabet=33, window=-1) == BAD and "alphabet length" in _capi.last_error()
    for mode in (0, 2):
        assert call(mode=mode, window=-1, count=False) == INVALID and "OPAL_MODE_HW and OPAL_MODE_SW" in _capi.last_error()
    assert call(window=-1, count=False) == BAD and "negative window" in _capi.last_error()
    assert call(mode=SW, min_score=0, missing=(4,)) == BAD and "at least 1" in _capi.last_error()
    # miopalSearchPssmOccurrences' outputs, then the new ones
    assert call(count=False, missing=(4, 6)) == BAD and "null count" in _capi.last_error()
    assert call(missing=(0, 5)) == BAD and "null target / score" in _capi.last_error()
    assert call(missing=(3, 4)) == BAD and "null end-location" in _capi.last_error()
    assert call(missing=(4,)) == BAD and "null start-location" in _capi.last_error()
    assert call(missing=(5, 6)) == BAD and "null start-location" in _capi.last_error()
    for one in (6, 7):
        assert call(missing=(one,), c=None) == BAD and "both, or neither" in _capi.last_error()
    # the consensus: required with operations, its residues in range (255: no residue) either way
    assert call(c=None, r=tall, q=500) == BAD and "null consensus" in _capi.last_error()
    wrong = cons.copy()
    wrong[2] = 32
    assert call(c=wrong) == BAD and "consensus residue 32 out of range at 2" in _capi.last_error()
    assert call(c=wrong, missing=(6, 7)) == BAD and "consensus residue" in _capi.last_error()
    wrong[2] = 255
    assert call(c=wrong) == BAD and "null database handle" in _capi.last_error()
    # the height limit of the sweep stays
    assert call(r=tall, q=500) == BAD and "493 rows at most" in _capi.last_error()
    assert call(r=tall, q=493) == BAD and "null database handle" in _capi.last_error()
    # starts only needs no consensus; an empty PSSM needs none either
    assert call(c=None, missing=(6, 7)) == BAD and "null database handle" in _capi.last_error()
    assert call(r=None, c=None, q=0) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_plain_form_looks_at_the_handle_first():
    """miopalSearchOccurrencesAligned with no handle: miopalSearchOccurrences' order begins with the handle, so every
    call is told that it is missing, whatever else is wrong - the new null outputs included."""
    lib = _capi.lib()
    query = np.zeros(4, dtype=np.uint8)
    matrix = np.ones(24 * 24, dtype=np.int32)
    out = Outputs()
    for mode, q, cut, window, missing in ((HW, 4, 5, 3, ()), (0, 4, 5, 3, ()), (7, 4, 5, 3, (4,)), (HW, -1, 5, 3, (6,)),
                                          (HW, 4, 5, -1, (7,)), (SW, 4, 0, 3, (6, 7)), (HW, 4, 5, 3, (0, 5))):
        rc = lib.miopalSearchOccurrencesAligned(None, query.ctypes.data, q, 3, 1, matrix.ctypes.data, 24, mode, 0, 2, cut,
                                                window, -1, out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                *out.refs(missing))
        assert rc == BAD and "null database handle" in _capi.last_error(), (mode, q, cut, window, missing)
    assert out.untouched()


# ---- the Python layers ----------------------------------------------------------------------------------------------

def no_device():
    """a DeviceDatabase that was never created: any C call through it fails on the handle"""
    db = _capi.DeviceDatabase.__new__(_capi.DeviceDatabase)
    db._h, db.count, db.alphabet_length = None, 3, 24
    return db


def test_capi_refuses_the_rule_before_the_c_side():
    db = no_device()
    query = np.zeros(5, dtype=np.uint8)
    plain = _capi.DeviceDatabase.search_occurrence_alignments
    pssm = _capi.DeviceDatabase.search_occurrence_alignments_pssm
    for operations_ in (True, False):
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            plain(db, query, B62, 11, 1, "nw", operations=operations_)
        with pytest.raises(ValueError, match="negative"):
            plain(db, query, B62, 11, 1, "hw", window=-1, operations=operations_)
        with pytest.raises(ValueError, match="at least 1"):
            plain(db, query, B62, 11, 1, "sw", min_score=0, operations=operations_)
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            pssm(db, B62.reshape(24, 24)[query], query, 11, 1, "ov", operations=operations_)
    with pytest.raises(ValueError, match="one entry per row"):
        pssm(db, B62.reshape(24, 24)[query], query[:3], 11, 1, "hw")
    # ... and what passes reaches the C side, which misses the handle
    with pytest.raises(RuntimeError, match="null database handle"):
        plain(db, query, B62, 11, 1, "hw", min_score=5)


def test_find_occurrences_faults_and_empty_requests():
    assert pyopal_amd.find_occurrences is pyopal_amd.occurrences.find_occurrences
    for name in ("find_occurrences", "find_occurrences_pssm", "find_occurrences_arrays"):
        assert hasattr(pyopal_amd, name) and name not in pyopal_amd.__all__
    assert not any(hasattr(pyopal_amd.Aligner, name) for name in ("find_occurrences", "occurrences"))
    aligner = pyopal_amd.Aligner(gap_open=11, gap_extend=1)
    database = pyopal_amd.Database(["MKVLA", "ETSEEES", ""])
    pssm = pyopal_amd.Pssm.from_sequence("ETSE", "BLOSUM50")
    forms = ((pyopal_amd.find_occurrences, "ETSE"), (pyopal_amd.find_occurrences_arrays, "ETSE"),
             (pyopal_amd.find_occurrences_pssm, pssm))
    for find, query in forms:
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            find(aligner, query, database, 5, algorithm="nw")
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            find(aligner, query, database, 5, algorithm="smith")
        with pytest.raises(ValueError, match="negative"):
            find(aligner, query, database, 5, window=-1)
        with pytest.raises(ValueError, match="at least 1"):
            find(aligner, query, database, 0, algorithm="sw")
        for mode in ("score", "ends", None):
            with pytest.raises(ValueError, match="'end' or 'full'"):
                find(aligner, query, database, 5, mode=mode)
        with pytest.raises(TypeError, match="min_score"):
            find(aligner, query, database, 5.0)
        with pytest.raises(ValueError, match="max_hits"):
            find(aligner, query, database, 5, max_hits=-1)
        with pytest.raises(OverflowError):
            find(aligner, query, database, 5, start=-1)
        with pytest.raises(TypeError, match="database"):
            find(aligner, query, ["MKVLA"], 5)
        with pytest.raises(IndexError):
            find(aligner, query, database, 5, start=2, end=1)
    with pytest.raises(TypeError, match="Pssm"):
        pyopal_amd.find_occurrences_pssm(aligner, "ETSE", database, 5)
    # empty requests: an empty slice, an empty database, an empty query - no device is asked for
    for mode in ("end", "full"):
        assert pyopal_amd.find_occurrences(aligner, "ETSE", database, 5, mode=mode, start=1, end=1) == []
        assert pyopal_amd.find_occurrences(aligner, "ETSE", pyopal_amd.Database([]), 5, mode=mode) == []
        assert pyopal_amd.find_occurrences(aligner, "", database, 5, mode=mode) == []
        assert pyopal_amd.find_occurrences_pssm(aligner, pssm, database, 5, mode=mode, start=3) == []
        got = pyopal_amd.find_occurrences_arrays(aligner, "ETSE", database, 5, mode=mode, start=2, end=2)
        assert got["count"] == 0 and got["target"].dtype == np.int64 and len(got["score"]) == 0
        assert ("aln_off" in got) == (mode == "full") and ("start_t" in got) == (mode == "full")
        if mode == "full":
            assert got["aln_off"].tolist() == [0] and len(got["aln_flat"]) == 0


# ---- the witness, against the C checker -----------------------------------------------------------------------------

@pytest.mark.parametrize("algorithm", ["hw", "sw"])
@pytest.mark.parametrize("gaps", [(3, 1), (11, 1), (2, 2)])
def test_starts_from_the_checkers_end_cell_are_the_checkers(gaps, algorithm):
    """a few hundred random pairs: the checker's own best (score, end cell) is an occurrence, and the rule applied to it
    must give the checker's start; the operations of the rectangle are then the checker's"""
    rng = np.random.default_rng(5 + gaps[0])
    hits = 0
    for q in (1, 7, 30, 70):
        query = _data.random_protein(rng, q)
        targets = []
        for k in range(60):
            t = _data.random_protein(rng, int(rng.integers(1, 90)))
            if k % 2 == 0 and len(t) > q:
                piece = np.array(_data.mutate(rng, query, 0.2), dtype=np.uint8)
                at = int(rng.integers(0, len(t) - len(piece) + 1)) if len(t) > len(piece) else 0
                t = np.concatenate([t[:at], piece, t[at + len(piece):]])
            targets.append(np.asarray(t, dtype=np.uint8))
        residues, offsets = _oracle.flatten(targets)
        want = _oracle.search(query, residues, offsets, B62, gaps[0], gaps[1], "full", algorithm)
        live = np.flatnonzero(want["end_t"] >= 0)
        occ = [(k, want["score"][k], want["end_t"][k], want["end_q"][k]) for k in live]
        start_t, start_q = starts(B62.reshape(24, 24)[query], targets, occ, gaps[0], gaps[1], algorithm)
        assert np.array_equal(start_t, want["start_t"][live]), (q, gaps, algorithm)
        assert np.array_equal(start_q, want["start_q"][live]), (q, gaps, algorithm)
        ops = operations(query, B62, targets, occ, start_t, start_q, gaps[0], gaps[1])
        for k, mine in zip(live, ops):
            assert mine.tolist() == want["aln"][k].tolist(), (q, gaps, algorithm, k)
        hits += len(live)
    assert hits > 200


def test_degenerate_optimum_against_the_checker():
    """a matrix of -20 throughout at 1/1: the HW optimum is the gap over the whole query, no target residue"""
    rng = np.random.default_rng(3)
    matrix = np.full(24 * 24, -20, dtype=np.int32)
    query = _data.random_protein(rng, 6)
    targets = [_data.random_protein(rng, n) for n in (1, 5, 9)]
    residues, offsets = _oracle.flatten(targets)
    want = _oracle.search(query, residues, offsets, matrix, 1, 1, "full", "hw")
    assert want["score"].tolist() == [border(5, 1, 1)] * 3 == [-6] * 3
    occ = [(k, want["score"][k], want["end_t"][k], want["end_q"][k]) for k in range(3)]
    start_t, start_q = starts(matrix.reshape(24, 24)[query], targets, occ, 1, 1, "hw")
    assert np.array_equal(start_t, want["start_t"]) and np.array_equal(start_q, want["start_q"])
    assert np.array_equal(start_t, want["end_t"] + 1) and start_q.tolist() == [0, 0, 0]
    ops = operations(query, matrix, targets, occ, start_t, start_q, 1, 1)
    for k in range(3):
        assert ops[k].tolist() == want["aln"][k].tolist() == [1] * 6


# ---- ... and worked out by hand -------------------------------------------------------------------------------------

def test_hand_worked_start():
    """match +2, mismatch -1, gaps 2/1, query ABC (0 1 2). Target C A B C A: the last row of HW over the columns is
    -1 -1 2 6 4; the occurrence (6, row 2, column 3) is A B C = columns 1 .. 3: the reversed pass meets 6 first in its
    column 2, row 2. The column after it, (4, row 2, column 4), is the same alignment with one target residue gapped
    behind it: the reversed maximum 4 = 6 - 2 lies in column 3."""
    A = 4
    matrix = np.full((A, A), -1, dtype=np.int32)
    np.fill_diagonal(matrix, 2)
    query = np.array([0, 1, 2], dtype=np.uint8)
    target = np.array([2, 0, 1, 2, 0], dtype=np.uint8)
    rows = matrix[query]
    start_t, start_q = starts(rows, [target], [(0, 6, 3, 2), (0, 4, 4, 2)], 2, 1, "hw")
    assert start_t.tolist() == [1, 1] and start_q.tolist() == [0, 0]
    ops = operations(query, matrix.ravel(), [target], [(0, 6, 3, 2), (0, 4, 4, 2)], start_t, start_q, 2, 1)
    assert ops[0].tolist() == [0, 0, 0] and ops[1].tolist() == [0, 0, 0, 2]
    # SW: the cell (row 1, column 2) holds A B = 4, begun at (row 0, column 1)
    start_t, start_q = starts(rows, [target], [(0, 4, 2, 1)], 2, 1, "sw")
    assert (start_t.tolist(), start_q.tolist()) == ([1], [0])
    # a score that the cell does not hold is no occurrence
    with pytest.raises(AssertionError):
        starts(rows, [target], [(0, 5, 3, 2)], 2, 1, "hw")


def test_hand_worked_degenerate_start():
    """every substitution -20, gaps 1/1, query of 3 rows: the last row of HW holds -3 in every column - the gap over
    the query, border(2) - and no real alignment reaches it (the best one, a substitution and two gaps, is -22). The
    target span is empty: start_t = column + 1, start_q = 0, three query-consuming gaps."""
    matrix = np.full((4, 4), -20, dtype=np.int32)
    query = np.array([0, 1, 2], dtype=np.uint8)
    target = np.array([3, 3, 0, 1], dtype=np.uint8)
    occ = [(0, -3, j, 2) for j in range(4)]
    assert border(2, 1, 1) == -3
    start_t, start_q = starts(matrix[query], [target], occ, 1, 1, "hw")
    assert start_t.tolist() == [1, 2, 3, 4] and start_q.tolist() == [0, 0, 0, 0]
    ops = operations(query, matrix.ravel(), [target], occ, start_t, start_q, 1, 1)
    assert all(o.tolist() == [1, 1, 1] for o in ops)
