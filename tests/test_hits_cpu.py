"""CPU tier of the hit searches (miopalSearchHits, miopalSearchPssmHits, miopalSearchBatchHits, the test hook
miopalTestSelectHits; DeviceDatabase.search_hits / search_pssm_hits / search_batch_hits / select_hits_rows;
Aligner.hits / hits_many / hits_pssm): the C ABI is declared, listed and exported; the new error code is defined and
mapped; with no handle the checks that need none come first, with their documented codes and in their documented
order; the test hook refuses bad arguments before any device call; the Python layer checks its arguments as `top_hits`
does and answers empty requests without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import Pssm, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE
INT_MIN = -(2 ** 31)
NAMES = ("miopalSearchHits", "miopalSearchPssmHits", "miopalSearchBatchHits", "miopalTestSelectHits")


def prototype(name):
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert found, f"{name} is not declared"
    return re.sub(r"\s+", " ", found.group(1)).strip()


def test_header_declares_the_entry_points():
    tail = "int64_t** targetIndex, int** score, int** endTarget, int** endQuery"
    args = prototype("miopalSearchHits")
    assert args.startswith("MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt, "
                           "const int* scoreMatrix, int alphabetLength, int searchType, int mode,")
    assert args.endswith("int64_t start, int64_t end, int minScore, int64_t maxHits, int64_t* count, " + tail)
    args = prototype("miopalSearchPssmHits")
    assert args.startswith("MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt, int alphabetLength,")
    assert args.endswith("int64_t start, int64_t end, int minScore, int64_t maxHits, int64_t* count, " + tail)
    args = prototype("miopalSearchBatchHits")
    assert args.startswith("MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,")
    assert args.endswith("int64_t start, int64_t end, const int* minScore, int64_t maxHits, int64_t* hitOffsets, " + tail)
    args = prototype("miopalTestSelectHits")
    assert args == ("const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride, "
                    "const int* minScore, int64_t start, int64_t* hitOffsets, int64_t** targetIndex, int** outScore, "
                    "int** outEndTarget, int** outEndQuery")
    for name in NAMES:
        assert name in _capi.EXPORTS
    for name in ("search_hits", "search_pssm_hits", "search_batch_hits", "select_hits_rows"):
        assert hasattr(_capi.DeviceDatabase, name)
    for name in ("hits", "hits_many", "hits_pssm", "hits_arrays", "hits_many_arrays", "hits_pssm_arrays"):
        assert hasattr(pyopal_amd.Aligner, name)


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names


def test_too_many_hits_is_defined_and_mapped():
    text = open(os.path.join(ROOT, "include", "opal.h")).read()
    assert re.search(r"^#define\s+MIOPAL_ERR_TOO_MANY_HITS\s+103\s*$", text, re.M)
    assert _capi.MIOPAL_ERR_TOO_MANY_HITS == 103
    assert issubclass(_capi.TooManyHits, RuntimeError)
    with pytest.raises(_capi.TooManyHits, match="max_hits"):
        _capi.raise_for(103)
    # (the other codes keep their mapping)
    with pytest.raises(OverflowError):
        _capi.raise_for(_capi.OPAL_ERR_OVERFLOW)
    with pytest.raises(RuntimeError, match="code=101") as info:
        _capi.raise_for(101)
    assert not isinstance(info.value, _capi.TooManyHits)


class Outputs:
    """A count (or three offsets) and four array pointers, all set to a mark that no call may change."""
    MARK = 0x77

    def __init__(self):
        self.count = np.full(3, 77, dtype=np.int64)
        self.ptrs = [ctypes.c_void_p(self.MARK) for _ in range(4)]

    def refs(self, missing=()):
        return [None if i in missing else ctypes.byref(p) for i, p in enumerate(self.ptrs)]

    def untouched(self):
        return np.all(self.count == 77) and all(p.value == self.MARK for p in self.ptrs)


def test_pssm_form_reports_argument_errors_before_a_device():
    """miopalSearchPssmHits with no handle at all: miopalSearchPssmTop's order - mode, search type, query length, rows,
    alphabet, the refusal of alignments, the outputs - and then the missing handle."""
    lib = _capi.lib()
    rows = np.ones((4, 32), dtype=np.int32)
    out = Outputs()

    def call(r=rows, q=4, alphabet=32, st=1, mode=3, count=True, missing=(), max_hits=-1):
        return lib.miopalSearchPssmHits(None, None if r is None else r.ctypes.data, q, 3, 1, alphabet, st, mode, 0, 2,
                                        INT_MIN, max_hits,
                                        out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if count else None,
                                        *out.refs(missing))

    assert call(mode=4) == INVALID and "alignment mode" in _capi.last_error()
    assert call(mode=-1) == INVALID
    assert call(mode=4, st=3, q=-1) == INVALID and "alignment mode" in _capi.last_error()
    assert call(st=3) == INVALID and "search type" in _capi.last_error()
    assert call(st=-1, q=-1) == INVALID and "search type" in _capi.last_error()
    assert call(q=-1) == BAD and "query length" in _capi.last_error()
    assert call(q=-1, r=None, alphabet=0) == BAD and "query length" in _capi.last_error()
    assert call(r=None) == BAD and "null row scores" in _capi.last_error()
    assert call(r=None, alphabet=33) == BAD and "null row scores" in _capi.last_error()
    assert call(alphabet=0) == BAD and "alphabet length" in _capi.last_error()
    assert call(alphabet=33) == BAD and "alphabet length" in _capi.last_error()
    # alignments are not selected on the device: refused whatever else is asked for
    assert call(st=2) == INVALID and "alignments are not selected" in _capi.last_error()
    assert call(st=2, count=False) == INVALID
    # null outputs (the end-location pointers only where the search type produces them)
    assert call(count=False) == BAD and "null count" in _capi.last_error()
    assert call(missing=(0,)) == BAD and "null target / score" in _capi.last_error()
    assert call(missing=(1,)) == BAD and "null target / score" in _capi.last_error()
    assert call(missing=(2,)) == BAD and "null end-location" in _capi.last_error()
    assert call(missing=(3,)) == BAD and "null end-location" in _capi.last_error()
    assert call(st=0, missing=(2, 3)) == BAD and "null database handle" in _capi.last_error()
    # nothing wrong with the arguments: the handle is what is missing (any maxHits is an argument, not an error)
    for st, max_hits in ((0, -1), (1, -1), (0, 0), (1, 2 ** 40), (0, -5)):
        assert call(st=st, max_hits=max_hits) == BAD and "null database handle" in _capi.last_error()
    assert call(r=None, q=0) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_plain_form_looks_at_the_handle_first():
    """miopalSearchHits with no handle: miopalSearchTop's order - miopalSearch's checks begin with the handle, so every
    call is told that it is missing, a request for alignments included."""
    lib = _capi.lib()
    query = np.zeros(4, dtype=np.uint8)
    matrix = np.ones(24 * 24, dtype=np.int32)
    out = Outputs()
    for st, mode, q in ((0, 3, 4), (2, 3, 4), (3, 3, 4), (1, 7, 4), (1, 3, -1)):
        rc = lib.miopalSearchHits(None, query.ctypes.data, q, 3, 1, matrix.ctypes.data, 24, st, mode, 0, 2, INT_MIN, -1,
                                  out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), *out.refs())
        assert rc == BAD and "null database handle" in _capi.last_error(), (st, mode, q)
    assert out.untouched()


def test_batch_form_reports_argument_errors_before_a_device():
    """miopalSearchBatchHits with no handle: miopalSearchBatchTop's order - alignments refused first, then the query
    list and its offsets, and only then the per-query checks of miopalSearch, which begin with the handle."""
    lib = _capi.lib()
    queries = np.zeros(8, dtype=np.uint8)
    offsets = np.array([0, 3, 8], dtype=np.int64)
    matrix = np.ones(24 * 24, dtype=np.int32)
    thresholds = np.zeros(2, dtype=np.int32)
    out = Outputs()

    def call(q=queries, off=offsets, n=2, st=1, mode=3):
        return lib.miopalSearchBatchHits(None, None if q is None else q.ctypes.data, None if off is None else off.ctypes.data,
                                         n, 3, 1, matrix.ctypes.data, 24, st, mode, 0, 2, thresholds.ctypes.data, -1,
                                         out.count.ctypes.data, *out.refs())

    assert call(st=2) == INVALID and "alignments are not selected" in _capi.last_error()
    assert call(st=2, n=-1) == INVALID
    assert call(n=-1) == BAD and "bad query list" in _capi.last_error()
    assert call(q=None) == BAD and "bad query list" in _capi.last_error()
    assert call(off=None) == BAD and "bad query list" in _capi.last_error()
    # (query by query: the offsets of a query, then miopalSearch's checks of it)
    assert call(off=np.array([5, 3, 8], dtype=np.int64)) == BAD and "bad query offsets at 0" in _capi.last_error()
    assert call(off=np.array([-1, 3, 8], dtype=np.int64)) == BAD and "bad query offsets at 0" in _capi.last_error()
    assert call() == BAD and "null database handle" in _capi.last_error()
    assert call(mode=9) == BAD and "null database handle" in _capi.last_error()
    assert call(n=0) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_hook_refuses_bad_arguments_before_a_device():
    lib = _capi.lib()
    score = np.zeros((2, 8), dtype=np.int32)
    ends = np.zeros((2, 8), dtype=np.int32)
    thresholds = np.zeros(2, dtype=np.int32)
    out = Outputs()

    def call(s=score, et=None, eq=None, rows=2, stride=8, t=thresholds, offsets=True, missing=()):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.miopalTestSelectHits(ptr(s), ptr(et), ptr(eq), rows, stride, ptr(t), 0,
                                        out.count.ctypes.data if offsets else None, *out.refs(missing))

    for rows, stride in ((0, 8), (-1, 8), (2, 0), (2, -3)):
        assert call(rows=rows, stride=stride) == BAD and "both at least 1" in _capi.last_error()
    assert call(s=None) == BAD and "null score rows" in _capi.last_error()
    assert call(t=None) == BAD and "minScore" in _capi.last_error()
    assert call(et=ends) == BAD and "one end array without the other" in _capi.last_error()
    assert call(eq=ends) == BAD and "one end array without the other" in _capi.last_error()
    assert call(offsets=False) == BAD and "null hitOffsets" in _capi.last_error()
    assert call(missing=(0,)) == BAD and call(missing=(1,)) == BAD
    assert call(et=ends, eq=ends, missing=(2,)) == BAD and "null end-location" in _capi.last_error()
    assert call(et=ends, eq=ends, missing=(3,)) == BAD and "null end-location" in _capi.last_error()
    for rows, stride in ((2, 2 ** 26 + 1), (2 ** 27 + 1, 1), (1, 2 ** 27 + 1), (3, 2 ** 62)):
        assert call(rows=rows, stride=stride) == BAD and "more than 2^27" in _capi.last_error(), (rows, stride)
    assert out.untouched()


@pytest.fixture
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture
def database():
    return pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])


def forms(aligner, database):
    """(name, call(min_score=..., **kw)) of the three forms and their array variants, on a well-formed query"""
    pssm = Pssm.from_sequence("MKV")
    return [
        ("hits", lambda min_score=3, db=database, **kw: aligner.hits("MKV", db, min_score, **kw)),
        ("hits_arrays", lambda min_score=3, db=database, **kw: aligner.hits_arrays("MKV", db, min_score, **kw)),
        ("hits_many", lambda min_score=3, db=database, **kw: aligner.hits_many(["MKV", "A"], db, min_score, **kw)),
        ("hits_many_arrays", lambda min_score=3, db=database, **kw: aligner.hits_many_arrays(["MKV", "A"], db, min_score, **kw)),
        ("hits_pssm", lambda min_score=3, db=database, **kw: aligner.hits_pssm(pssm, db, min_score, **kw)),
        ("hits_pssm_arrays", lambda min_score=3, db=database, **kw: aligner.hits_pssm_arrays(pssm, db, min_score, **kw)),
    ]


def test_python_validation_is_that_of_top_hits(aligner, database):
    def top(**kw):
        return aligner.top_hits("MKV", database, 3, **kw)

    for name, call in forms(aligner, database):
        for kw in (dict(mode="sorted"), dict(algorithm="blast"), dict(start=2, end=1), dict(start=10), dict(start=-1),
                   dict(end=-1)):
            with pytest.raises(Exception) as want:
                top(**kw)
            with pytest.raises(type(want.value)) as got:
                call(**kw)
            assert str(got.value) == str(want.value), (name, kw)
        # the threshold is the integer of these calls, as k is of top_hits: the same refusals
        for value in (1.0, "3", None, True):
            with pytest.raises(TypeError) as want:
                aligner.top_hits("MKV", database, value)
            with pytest.raises(TypeError, match="min_score must be an integer"):
                call(min_score=value)
        with pytest.raises(OverflowError):
            call(min_score=2 ** 31)
        with pytest.raises(TypeError, match="expected BaseDatabase"):
            call(db=["MKV"])
        with pytest.raises(ValueError, match="different alphabets"):
            call(db=pyopal_amd.Database(["ACGT"], alphabet="ACGT"))
        for value in (1.5, "3", True):
            with pytest.raises(TypeError, match="max_hits"):
                call(max_hits=value)
        with pytest.raises(ValueError, match="max_hits"):
            call(max_hits=-1)
    with pytest.raises(TypeError, match="expected Pssm"):
        aligner.hits_pssm("MKV", database, 3)
    with pytest.raises(ValueError, match="different alphabets"):
        aligner.hits_pssm(Pssm(np.eye(4, dtype=np.int32), "ACGT"), database, 3)
    with pytest.raises(TypeError, match="must not be None"):
        aligner.hits(None, database, 3)
    # one threshold per query, or one for all
    for wrong in ([1], [1, 2, 3], np.array([1, 2, 3])):
        with pytest.raises(ValueError, match="one per query"):
            aligner.hits_many(["MKV", "A"], database, wrong)
    with pytest.raises(TypeError, match="min_score must be an integer"):
        aligner.hits_many(["MKV", "A"], database, [1, 2.5])
    with pytest.raises(TypeError, match="min_score must be an integer"):
        aligner.hits("MKV", database, [1])


def test_empty_answers_need_no_device(aligner, database, monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    for mode in ("score", "end", "full"):
        for name, call in forms(aligner, database):
            for kw in (dict(start=1, end=1), dict(start=3)):
                got = call(mode=mode, **kw)
                if name.endswith("_arrays"):
                    rows = 2 if "many" in name else 1
                    assert got["offsets"].tolist() == [0] * (rows + 1) and len(got["target"]) == 0 and len(got["score"]) == 0
                    assert ("end_q" in got) == (mode != "score") and ("aln_flat" in got) == (mode == "full")
                else:
                    assert got == ([[], []] if "many" in name else []), (name, mode, kw)
        assert aligner.hits_many([], database, 3, mode=mode) == []
        assert aligner.hits_many([], database, [], mode=mode) == []
        assert aligner.hits_many_arrays([], database, 3, mode=mode)["offsets"].tolist() == [0]


def test_well_formed_calls_fail_loudly_without_a_device(aligner, database):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for name, call in forms(aligner, database):
        with pytest.raises(RuntimeError, match="no supported SIMD backend"):
            call()
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.select_hits_rows(np.zeros((2, 8), dtype=np.int32), 0)
