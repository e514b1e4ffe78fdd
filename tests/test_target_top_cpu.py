"""CPU tier of the per-target selection (miopalSearchBatchTargetTop, the test hook miopalTestSelectColumns;
DeviceDatabase.search_batch_target_top / select_columns_rows; Aligner.best_queries / best_queries_arrays): the C ABI is
declared, listed and exported; the Python prototypes have the header's arity; with no handle and no device the checks
come in the header's order with its codes; the hook refuses bad arguments before any device call; the Python layer
checks its arguments as `top_hits_many` does and answers empty requests without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE
INT_MIN = -(2 ** 31)
NAMES = ("miopalSearchBatchTargetTop", "miopalTestSelectColumns")


def prototype(name):
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert found, f"{name} is not declared"
    return re.sub(r"\s+", " ", found.group(1)).strip()


def test_header_declares_the_entry_points():
    args = prototype("miopalSearchBatchTargetTop")
    assert args == ("MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries, "
                    "int gapOpen, int gapExt, const int* scoreMatrix, int alphabetLength, int searchType, "
                    "int mode, int64_t start, int64_t end, int m, int minScore, "
                    "int* count, int32_t* queryIndex, int* score, int* endTarget, int* endQuery")
    args = prototype("miopalTestSelectColumns")
    assert args == ("const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride, "
                    "const int32_t* pieceFirst, const int32_t* pieceCount, int pieces, "
                    "const unsigned char* skip, int m, int minScore, "
                    "int* count, int32_t* queryIndex, int* outScore, int* outEndTarget, int* outEndQuery")
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    assert re.search(r"^#define\s+MIOPAL_MAX_TARGET_TOP\s+8\s*$", text, re.M)
    assert _capi.MIOPAL_MAX_TARGET_TOP == 8
    for name in NAMES:
        assert name in _capi.EXPORTS
    for name in ("search_batch_target_top", "select_columns_rows"):
        assert hasattr(_capi.DeviceDatabase, name)
    assert callable(_capi.select_columns_rows)
    for name in ("best_queries", "best_queries_arrays"):
        assert hasattr(pyopal_amd.Aligner, name)


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names


def test_python_prototypes_have_the_arity_of_the_header():
    lib = _capi.lib()
    for name in NAMES:
        declared = [a.strip() for a in prototype(name).split(",")]
        argtypes = getattr(lib, name).argtypes
        assert len(argtypes) == len(declared), name
        assert getattr(lib, name).restype is ctypes.c_int
        for arg, ctype in zip(declared, argtypes):
            if "*" in arg:
                assert ctype is ctypes.c_void_p, (name, arg)
            elif arg.startswith("int64_t"):
                assert ctype is ctypes.c_int64, (name, arg)
            else:
                assert arg.startswith("int ") and ctype is ctypes.c_int, (name, arg)


class Outputs:
    """count and the four [n][m] arrays, all set to a mark that no failing call may change"""

    def __init__(self, cells=16):
        self.arrays = [np.full(cells, 77, dtype=np.int32) for _ in range(5)]

    def ptrs(self, missing=()):
        return [None if i in missing else a.ctypes.data for i, a in enumerate(self.arrays)]

    def untouched(self):
        return all(np.all(a == 77) for a in self.arrays)


def test_search_reports_argument_errors_before_a_device():
    """miopalSearchBatchTargetTop with no handle: alignments refused first, then the query list and its offsets, then the
    per-query checks of miopalSearch - which begin with the handle, so m and the outputs, checked after them, are not
    reached."""
    lib = _capi.lib()
    queries = np.zeros(8, dtype=np.uint8)
    offsets = np.array([0, 3, 8], dtype=np.int64)
    matrix = np.ones(24 * 24, dtype=np.int32)
    out = Outputs()

    def call(q=queries, off=offsets, n=2, st=1, mode=3, m=2, missing=()):
        return lib.miopalSearchBatchTargetTop(None, None if q is None else q.ctypes.data,
                                              None if off is None else off.ctypes.data, n, 3, 1, matrix.ctypes.data, 24,
                                              st, mode, 0, 2, m, INT_MIN, *out.ptrs(missing))

    assert call(st=2) == INVALID and "alignments are not selected" in _capi.last_error()
    assert call(st=2, n=-1) == INVALID
    assert call(st=2, m=0, missing=(0, 1, 2, 3, 4)) == INVALID
    assert call(n=-1) == BAD and "bad query list" in _capi.last_error()
    assert call(n=-1, m=0) == BAD and "bad query list" in _capi.last_error()
    assert call(q=None) == BAD and "bad query list" in _capi.last_error()
    assert call(off=None, missing=(0,)) == BAD and "bad query list" in _capi.last_error()
    # (query by query: the offsets of a query, then miopalSearch's checks of it)
    assert call(off=np.array([5, 3, 8], dtype=np.int64)) == BAD and "bad query offsets at 0" in _capi.last_error()
    assert call(off=np.array([-1, 3, 8], dtype=np.int64), m=9) == BAD and "bad query offsets at 0" in _capi.last_error()
    assert call() == BAD and "null database handle" in _capi.last_error()
    assert call(mode=9) == BAD and "null database handle" in _capi.last_error()
    assert call(n=0) == BAD and "null database handle" in _capi.last_error()
    # m and the outputs come after the queries: with no handle they are never looked at
    for m in (0, -1, 9):
        assert call(m=m) == BAD and "null database handle" in _capi.last_error()
    assert call(missing=(0,)) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_hook_refuses_bad_arguments_before_a_device():
    lib = _capi.lib()
    score = np.zeros((4, 8), dtype=np.int32)
    ends = np.zeros((4, 8), dtype=np.int32)
    first = np.array([0, 2], dtype=np.int32)
    counts = np.array([2, 2], dtype=np.int32)
    out = Outputs(cells=64)

    def call(s=score, et=None, eq=None, rows=4, stride=8, pf=first, pc=counts, pieces=2, m=2, missing=()):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.miopalTestSelectColumns(ptr(s), ptr(et), ptr(eq), rows, stride, ptr(pf), ptr(pc), pieces, None, m,
                                           INT_MIN, *out.ptrs(missing))

    for rows, stride in ((0, 8), (-1, 8), (4, 0), (4, -3)):
        assert call(rows=rows, stride=stride) == BAD and "both at least 1" in _capi.last_error()
    for m in (0, -1, 9, 4096):
        assert call(m=m) == BAD and "outside [1, 8]" in _capi.last_error()
    assert call(s=None) == BAD and "null score rows" in _capi.last_error()
    assert call(pf=None) == BAD and "bad piece list" in _capi.last_error()
    assert call(pc=None) == BAD and "bad piece list" in _capi.last_error()
    assert call(pieces=-1) == BAD and "bad piece list" in _capi.last_error()
    assert call(et=ends) == BAD and "one end array without the other" in _capi.last_error()
    assert call(eq=ends) == BAD and "one end array without the other" in _capi.last_error()
    for k in (0, 1, 2):
        assert call(missing=(k,)) == BAD and "null count / query / score" in _capi.last_error()
    assert call(et=ends, eq=ends, missing=(3,)) == BAD and "null end-location" in _capi.last_error()
    assert call(et=ends, eq=ends, missing=(4,)) == BAD and "null end-location" in _capi.last_error()
    for pf, pc in (([-1, 2], [2, 2]), ([0, 4], [2, 1]), ([0, 3], [2, 2]), ([0, 2], [2, 0]), ([0, 2], [5, 1]),
                   ([0, 2 ** 31 - 1], [2, 2])):
        rc = call(pf=np.array(pf, dtype=np.int32), pc=np.array(pc, dtype=np.int32))
        assert rc == BAD and "outside [0, 4)" in _capi.last_error(), (pf, pc)
    one = np.array([1], dtype=np.int32)
    zero = np.array([0], dtype=np.int32)
    for rows, stride in ((2, 2 ** 26 + 1), (2 ** 27 + 1, 1), (1, 2 ** 27 + 1), (3, 2 ** 62)):
        rc = call(rows=rows, stride=stride, pf=zero, pc=one, pieces=1)
        assert rc == BAD and "more than 2^27" in _capi.last_error(), (rows, stride)
    assert out.untouched()


@pytest.fixture
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture
def database():
    return pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])


def forms(aligner):
    return [("best_queries", aligner.best_queries), ("best_queries_arrays", aligner.best_queries_arrays)]


def test_python_validation_is_that_of_top_hits_many(aligner, database):
    def top(**kw):
        return aligner.top_hits_many(["MKV", "A"], database, 3, **kw)

    for name, call in forms(aligner):
        for kw in (dict(mode="sorted"), dict(algorithm="blast"), dict(start=2, end=1), dict(start=10), dict(start=-1),
                   dict(end=-1)):
            with pytest.raises(Exception) as want:
                top(**kw)
            with pytest.raises(type(want.value)) as got:
                call(["MKV", "A"], database, 2, **kw)
            assert str(got.value) == str(want.value), (name, kw)
        for value in (1.0, "3", None, True):
            with pytest.raises(TypeError, match="m must be an integer, not " + type(value).__name__):
                call(["MKV", "A"], database, value)
        for value in (0, -1, 9, 4096):
            with pytest.raises(ValueError, match=r"m must be between 1 and 8 \(MIOPAL_MAX_TARGET_TOP\), got " + str(value)):
                call(["MKV", "A"], database, value)
        with pytest.raises(TypeError, match="expected BaseDatabase"):
            call(["MKV"], ["MKV"])
        with pytest.raises(ValueError, match="different alphabets"):
            call(["MKV"], pyopal_amd.Database(["ACGT"], alphabet="ACGT"))
        with pytest.raises(TypeError, match="must not be None"):
            call(["MKV", None], database)
        # the order of `_top`: the mode before m, m before the database
        with pytest.raises(ValueError, match="invalid search mode"):
            call(["MKV"], ["MKV"], 0, mode="sorted")
        with pytest.raises(ValueError, match="m must be between"):
            call(["MKV"], ["MKV"], 0)


def test_empty_answers_need_no_device(aligner, database, monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    for mode in ("score", "end", "full"):
        # an empty slice: no targets
        for kw in (dict(start=1, end=1), dict(start=3)):
            assert aligner.best_queries(["MKV", "A"], database, 2, mode=mode, **kw) == []
            got = aligner.best_queries_arrays(["MKV", "A"], database, 2, mode=mode, **kw)
            assert got["count"].shape == (0,) and got["query"].shape == (0, 2) and got["score"].shape == (0, 2)
            assert ("end_q" in got) == (mode == "end") and ("pairs" in got) == (mode == "full")
        # no queries: every target without a candidate
        assert aligner.best_queries([], database, 3, mode=mode) == [[], [], []]
        got = aligner.best_queries_arrays([], database, 3, mode=mode, start=1)
        assert got["count"].tolist() == [0, 0] and got["query"].dtype == np.int32
        assert np.all(got["query"] == -1) and np.all(got["score"] == -1) and got["score"].shape == (2, 3)
        if mode == "end":
            assert np.all(got["end_q"] == -1) and np.all(got["end_t"] == -1)
        if mode == "full":
            assert len(got["pairs"]["query"]) == 0 and got["pairs"]["aln_off"].tolist() == [0]


def test_well_formed_calls_fail_loudly_without_a_device(aligner, database):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for name, call in forms(aligner):
        with pytest.raises(RuntimeError, match="no supported SIMD backend"):
            call(["MKV", "A"], database, 2)
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.select_columns_rows(np.zeros((2, 8), dtype=np.int32), 1)
