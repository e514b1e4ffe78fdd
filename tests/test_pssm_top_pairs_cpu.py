"""CPU tier of the PSSM forms of the top-k selection and of the pair list (miopalSearchPssmTop, miopalAlignPairsPssm,
DeviceDatabase.search_pssm_top / align_pairs_pssm, Aligner.top_hits_pssm / align_pairs_pssm): the C ABI is declared,
listed and exported; every argument check that needs no handle is made before the handle is looked at, with its
documented code and in its documented order; the Python layer checks its arguments and answers empty requests
without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import Pssm, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "miopal.h")
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE


def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    top = re.search(r"\bint\s+miopalSearchPssmTop\s*\(([^)]*)\)", text)
    assert top, "miopalSearchPssmTop is not declared"
    args = re.sub(r"\s+", " ", top.group(1))
    assert args.startswith("MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt, int alphabetLength,")
    assert args.endswith("int k, int minScore, int* count, int64_t* targetIndex, int* score, int* endTarget, int* endQuery")
    pairs = re.search(r"\bint\s+miopalAlignPairsPssm\s*\(([^)]*)\)", text)
    assert pairs, "miopalAlignPairsPssm is not declared"
    args = re.sub(r"\s+", " ", pairs.group(1))
    assert args.startswith("MiopalDb* db, const int* rowScores, const unsigned char* consensus, const int64_t* rowOffsets, "
                           "int nPssms, const int32_t* pairPssm, const int64_t* pairTarget, int64_t nPairs,")
    assert args.endswith("unsigned char** operations, int64_t* operationOffsets")
    for name in ("miopalSearchPssmTop", "miopalAlignPairsPssm"):
        assert name in _capi.EXPORTS
    for name in ("search_pssm_top", "align_pairs_pssm"):
        assert hasattr(_capi.DeviceDatabase, name)
    for name in ("top_hits_pssm", "align_pairs_pssm"):
        assert hasattr(pyopal_amd.Aligner, name)


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"miopalSearchPssmTop", "miopalAlignPairsPssm"} <= names


def test_top_call_reports_argument_errors_before_a_device():
    """miopalSearchPssmTop with no handle at all: what needs no handle is refused first, in miopalSearchPssm's order,
    the two refusals of the selection (alignments, k) among it; a well-formed call is told that the handle is missing."""
    lib = _capi.lib()
    rows = np.ones((4, 32), dtype=np.int32)
    count = np.full(1, 77, dtype=np.int32)
    target = np.full(8, 77, dtype=np.int64)
    outs = np.full((3, 8), 77, dtype=np.int32)

    def call(r=rows, q=4, alphabet=32, st=1, mode=3, k=8):
        return lib.miopalSearchPssmTop(None, None if r is None else r.ctypes.data, q, 3, 1, alphabet, st, mode, 0, 2, k,
                                       -(2 ** 31), count.ctypes.data, target.ctypes.data, outs[0].ctypes.data,
                                       outs[1].ctypes.data, outs[2].ctypes.data)

    assert call(mode=4) == INVALID and "alignment mode" in _capi.last_error()
    assert call(mode=-1) == INVALID
    # (the mode comes first, then the search type, then the PSSM)
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
    assert call(st=2, k=-1) == INVALID
    for k in (-1, _capi.MIOPAL_MAX_TOP + 1):
        assert call(k=k) == BAD and f"k = {k}" in _capi.last_error() and "4096" in _capi.last_error()
    # nothing wrong with the arguments: the handle is what is missing (no consensus is asked for)
    for st, k in ((0, 8), (1, 8), (0, 0), (1, _capi.MIOPAL_MAX_TOP)):
        assert call(st=st, k=k) == BAD and "null database handle" in _capi.last_error()
    assert call(r=None, q=0) == BAD and "null database handle" in _capi.last_error()
    # nothing was written on any of these errors
    assert np.all(count == 77) and np.all(target == 77) and np.all(outs == 77)


def test_pairs_call_reports_argument_errors_before_a_device():
    """miopalAlignPairsPssm with no handle at all: mode, search type, offsets, rows, alphabet, consensus, the pair
    list's PSSM side, the outputs - in that order - and then the missing handle."""
    lib = _capi.lib()
    rows = np.ones((7, 32), dtype=np.int32)
    cons = np.array([0, 31, 255, 5, 1, 2, 3], dtype=np.uint8)
    offsets = np.array([0, 4, 4, 7], dtype=np.int64)     # three PSSMs, the second one empty
    pair_pssm = np.array([0, 2, 1, 2], dtype=np.int32)
    pair_target = np.array([0, 1, 1, 0], dtype=np.int64)
    outs = np.full((5, 4), 77, dtype=np.int32)
    aoff = np.full(5, 77, dtype=np.int64)
    ops = ctypes.c_void_p()

    def ptr(a):
        return None if a is None else a.ctypes.data

    def call(r=rows, c=cons, off=offsets, n_pssms=3, pp=pair_pssm, pt=pair_target, n_pairs=4, alphabet=32, st=2, mode=3,
             score=outs[0], ops_out=True, off_out=aoff):
        return lib.miopalAlignPairsPssm(None, ptr(r), ptr(c), ptr(off), n_pssms, ptr(pp), ptr(pt), n_pairs, 3, 1,
                                        alphabet, st, mode, ptr(score), outs[1].ctypes.data, outs[2].ctypes.data,
                                        outs[3].ctypes.data, outs[4].ctypes.data,
                                        ctypes.byref(ops) if ops_out else None, ptr(off_out))

    assert call(mode=4) == INVALID and "alignment mode" in _capi.last_error()
    assert call(mode=4, st=3, n_pssms=-1) == INVALID and "alignment mode" in _capi.last_error()
    assert call(st=3) == INVALID and "search type" in _capi.last_error()
    assert call(st=-1, n_pssms=-1) == INVALID and "search type" in _capi.last_error()
    assert call(n_pssms=-1) == BAD and "PSSM list" in _capi.last_error()
    assert call(off=None) == BAD and "PSSM list" in _capi.last_error()
    decreasing = np.array([0, 4, 3, 7], dtype=np.int64)
    assert call(off=decreasing) == BAD and "row offsets at 1" in _capi.last_error()
    assert call(off=decreasing, r=None) == BAD and "row offsets at 1" in _capi.last_error()
    negative = np.array([-1, 4, 4, 7], dtype=np.int64)
    assert call(off=negative) == BAD and "row offsets at 0" in _capi.last_error()
    too_many = np.array([0, 4, 4, 2 ** 31 - 64], dtype=np.int64)
    assert call(off=too_many) == BAD and "rows at most" in _capi.last_error()
    assert call(r=None) == BAD and "null row scores" in _capi.last_error()
    assert call(r=None, alphabet=0) == BAD and "null row scores" in _capi.last_error()
    assert call(alphabet=0) == BAD and "alphabet length" in _capi.last_error()
    assert call(alphabet=33) == BAD and "alphabet length" in _capi.last_error()
    assert call(c=None) == BAD and "null consensus" in _capi.last_error()
    bad = cons.copy()
    bad[5] = 40
    assert call(c=bad) == BAD and "consensus residue 40" in _capi.last_error() and "at 5" in _capi.last_error()
    assert call(c=bad, st=0) == BAD and "consensus residue 40" in _capi.last_error()   # (checked whenever it is given)
    # (rows before the first offset belong to no PSSM and are not looked at)
    late = np.array([6, 6, 7, 7], dtype=np.int64)
    assert call(c=bad, off=late, pp=np.array([1, 1, 0, 2], dtype=np.int32)) == BAD and "null database handle" in _capi.last_error()
    assert call(pp=None) == BAD and "pair list" in _capi.last_error()
    assert call(n_pairs=-1) == BAD and "pair list" in _capi.last_error()
    for value in (3, -1):
        wrong = pair_pssm.copy()
        wrong[2] = value
        wrong[3] = 9
        assert call(pp=wrong) == BAD, value
        assert f"pair 2: PSSM index {value} outside [0, 3)" in _capi.last_error()
    assert call(ops_out=False) == BAD and "null alignment outputs" in _capi.last_error()
    assert call(off_out=None) == BAD and "null alignment outputs" in _capi.last_error()
    assert call(score=None) == BAD and "null score output" in _capi.last_error()
    # nothing wrong with the list: the handle is what is missing (score and end lists need no consensus)
    assert call() == BAD and "null database handle" in _capi.last_error()
    for st in (0, 1):
        assert call(c=None, st=st) == BAD and "null database handle" in _capi.last_error()
    assert call(n_pairs=0, pp=None, pt=None) == BAD and "null database handle" in _capi.last_error()
    assert call(r=None, c=None, off=np.zeros(3, dtype=np.int64), n_pssms=2, pp=np.zeros(4, dtype=np.int32)) == BAD
    assert "null database handle" in _capi.last_error()
    # nothing was written on any of these errors
    assert np.all(outs == 77) and np.all(aoff == 77) and not ops.value


@pytest.fixture
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture
def database():
    return pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])


def test_top_hits_pssm_validation(aligner, database):
    pssm = Pssm.from_sequence("MKV")
    for not_a_pssm in ("MKV", None, pssm.scores):
        with pytest.raises(TypeError, match="expected Pssm"):
            aligner.top_hits_pssm(not_a_pssm, database, 3)
    for k in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            aligner.top_hits_pssm(pssm, database, k)
    for k in (-1, _capi.MIOPAL_MAX_TOP + 1):
        with pytest.raises(ValueError, match="4096"):
            aligner.top_hits_pssm(pssm, database, k)
    with pytest.raises(ValueError):
        aligner.top_hits_pssm(pssm, database, 3, mode="sorted")
    with pytest.raises(ValueError):
        aligner.top_hits_pssm(pssm, database, 3, algorithm="blast")
    with pytest.raises(IndexError):
        aligner.top_hits_pssm(pssm, database, 3, start=2, end=1)
    with pytest.raises(IndexError):
        aligner.top_hits_pssm(pssm, database, 3, start=10)
    with pytest.raises(OverflowError):
        aligner.top_hits_pssm(pssm, database, 3, start=-1)
    with pytest.raises(TypeError):
        aligner.top_hits_pssm(pssm, ["MKV"], 3)
    with pytest.raises(ValueError, match="different alphabets"):
        aligner.top_hits_pssm(pssm, pyopal_amd.Database(["ACGT"], alphabet="ACGT"), 3)
    with pytest.raises(ValueError, match="different alphabets"):
        aligner.top_hits_pssm(Pssm(np.eye(4, dtype=np.int32), "ACGT"), database, 3)


def test_align_pairs_pssm_validation(aligner, database):
    pssms = [Pssm.from_sequence("MKV"), Pssm.from_sequence("A")]
    with pytest.raises(TypeError, match="expected Pssm"):
        aligner.align_pairs_pssm([pssms[0], "MKV"], database, [(0, 0)])
    with pytest.raises(TypeError, match="expected Pssm"):
        aligner.align_pairs_pssm([None], database, [(0, 0)])
    with pytest.raises(TypeError):
        aligner.align_pairs_pssm(pssms, ["MKV"], [(0, 0)])
    with pytest.raises(ValueError, match="different alphabets"):
        aligner.align_pairs_pssm(pssms + [Pssm(np.eye(4, dtype=np.int32), "ACGT")], database, [(0, 0)])
    with pytest.raises(ValueError):
        aligner.align_pairs_pssm(pssms, database, [(0, 0)], mode="sorted")
    with pytest.raises(ValueError):
        aligner.align_pairs_pssm(pssms, database, [(0, 0)], algorithm="blast")
    for bad_pairs in ([0, 1], [(0, 1, 2)], [(0.5, 1.0)]):
        with pytest.raises(ValueError, match="pairs"):
            aligner.align_pairs_pssm(pssms, database, bad_pairs)
    for bad_pair in ((2, 0), (-1, 0)):
        with pytest.raises(IndexError, match="PSSM index"):
            aligner.align_pairs_pssm(pssms, database, [(0, 0), bad_pair])
    for bad_pair in ((0, 3), (0, -1)):
        with pytest.raises(IndexError, match="target index"):
            aligner.align_pairs_pssm(pssms, database, [(0, 0), bad_pair])


def test_empty_answers_need_no_device(aligner, database, monkeypatch):
    # (no device is reached: the library's device count is never asked for)
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    pssm = Pssm.from_sequence("MKV")
    for mode in ("score", "end", "full"):
        assert aligner.top_hits_pssm(pssm, database, 0, mode=mode) == []
        assert aligner.top_hits_pssm(pssm, database, 5, mode=mode, start=1, end=1) == []
        assert aligner.top_hits_pssm(pssm, database, 5, mode=mode, start=3) == []
        assert aligner.align_pairs_pssm([pssm], database, [], mode=mode) == []
        assert aligner.align_pairs_pssm([], database, np.zeros((0, 2), dtype=np.int64), mode=mode) == []


def test_well_formed_calls_fail_loudly_without_a_device(aligner, database):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    pssm = Pssm.from_sequence("MKVLA")
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        aligner.top_hits_pssm(pssm, database, 2)
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        aligner.align_pairs_pssm([pssm], database, [(0, 1)])
