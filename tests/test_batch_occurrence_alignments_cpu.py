"""CPU tier of the aligned occurrence search of a panel of queries (miopalSearchBatchOccurrencesAligned,
miopalLastBatchOccurrenceAlignRouting; DeviceDatabase.search_batch_occurrence_alignments;
pyopal_amd.find_occurrence_alignments_many): the symbols are declared, listed and exported; with no handle the call is
refused with every output as it was; the Python layers refuse the rule's faults before they reach the library; an
empty request is answered without a device, with the keys and dtypes of an answer."""
import subprocess
import threading

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import _capi

from test_batch_occurrences_cpu import _NoHandle
from test_occurrences_cpu import BAD, Outputs, prototype

NAMES = ("miopalSearchBatchOccurrencesAligned", "miopalLastBatchOccurrenceAlignRouting")
FORMS = ("find_occurrence_alignments_many", "find_occurrence_alignments_many_arrays")


def test_header_declares_the_entry_points():
    assert prototype("miopalSearchBatchOccurrencesAligned") == (
        prototype("miopalSearchBatchOccurrences") +
        ", int** startTarget, int** startQuery, unsigned char** alignments, int64_t** alignmentOffsets")
    assert prototype("miopalLastBatchOccurrenceAlignRouting") == "int64_t counts[4]"
    for name in NAMES:
        assert name in _capi.EXPORTS
    assert hasattr(_capi.DeviceDatabase, "search_batch_occurrence_alignments")
    assert hasattr(_capi.DeviceDatabase, "last_batch_occurrence_align_routing")


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names
    lib = _capi.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.miopalSearchBatchOccurrencesAligned.argtypes) == len(lib.miopalSearchBatchOccurrences.argtypes) + 4
    seen = []
    fresh = threading.Thread(target=lambda: seen.append(_capi.last_batch_occurrence_align_routing()))
    fresh.start()
    fresh.join()
    assert seen == [[0, 0, 0, 0]]
    lib.miopalLastBatchOccurrenceAlignRouting(None)


def test_no_handle_is_refused_with_the_outputs_as_they_were():
    """miopalSearchBatchOccurrences' order: the query list, then the handle - whatever the new outputs are"""
    lib = _capi.lib()
    out = Outputs(8)
    queries = np.zeros(6, dtype=np.uint8)
    offsets = np.array([0, 2, 6], dtype=np.int64)
    matrix = np.ones(16, dtype=np.int32)
    cuts, windows = np.array([3, 3], dtype=np.int32), np.array([2, 2], dtype=np.int32)

    def call(n=2, off=offsets, missing=()):
        return lib.miopalSearchBatchOccurrencesAligned(None, queries.ctypes.data, None if off is None else off.ctypes.data, n,
                                                       3, 1, matrix.ctypes.data, 4, 1, 0, 2, cuts.ctypes.data,
                                                       windows.ctypes.data, -1, out.count.ctypes.data, *out.refs(missing))

    assert call(n=-1) == BAD and "bad query list" in _capi.last_error()
    assert call(off=None) == BAD and "bad query list" in _capi.last_error()
    assert call() == BAD and "null database handle" in _capi.last_error()
    assert call(missing=(6,)) == BAD and "null database handle" in _capi.last_error()
    assert call(n=0, missing=(4, 5)) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_device_database_refusals_come_before_any_device_call(monkeypatch):
    """the preamble search_batch_occurrences has, shared: the same faults, before the library is reached"""
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    db = _NoHandle()
    panel = [np.zeros(n, dtype=np.uint8) for n in (4, 0, 9, 70, 2)]
    matrix = np.ones(16, dtype=np.int32)
    for operations in (True, False):
        call = lambda **kw: db.search_batch_occurrence_alignments(panel, matrix, 3, 1, operations=operations, **kw)   # noqa: E731
        for algorithm in ("nw", "ov", "blast"):
            with pytest.raises(ValueError, match="'hw' and 'sw'"):
                call(algorithm=algorithm, min_score=3)
        with pytest.raises(ValueError, match="window must not be negative"):
            call(min_score=3, window=[0, None, 5, -1, 2])
        with pytest.raises(ValueError, match="at least 1"):
            call(algorithm="sw", min_score=[5, 5, 5, 0, 5])
        with pytest.raises(ValueError, match="one value or one per query"):
            call(min_score=[1, 2, 3])
        with pytest.raises(ValueError, match="one value or one per query"):
            call(min_score=1, window=[1, 2, 3, 4, 5, 6])
        with pytest.raises(OverflowError):
            call(min_score=2 ** 31)
        for kw in (dict(min_score=-(2 ** 31), window=0), dict(algorithm="sw", min_score=1),
                   dict(min_score=[1, 2, 3, 4, 5], window=[None, 0, 5, None, 1])):
            with pytest.raises(AssertionError, match="device reached"):
                call(**kw)


def test_free_functions_faults_and_empty_requests(monkeypatch):
    for name in FORMS:
        assert getattr(pyopal_amd, name) is getattr(pyopal_amd.occurrences, name)
        assert name not in pyopal_amd.__all__ and not hasattr(pyopal_amd.Aligner, name)
    aligner = pyopal_amd.Aligner(gap_open=11, gap_extend=1)
    database = pyopal_amd.Database(["MKVLA", "ETSEEES", ""])
    panel = ["ETSE", "", "KVL"]
    # the rule's faults, before a mirror of the database is asked for
    monkeypatch.setattr(pyopal_amd.lib._Request, "mirror", lambda self: (_ for _ in ()).throw(AssertionError("device reached")))
    many, arrays = (getattr(pyopal_amd, name) for name in FORMS)
    for form in (many, arrays, lambda *a, **kw: arrays(*a, operations=False, **kw)):
        with pytest.raises(TypeError):
            form(aligner, panel, database, 5, mode="end")          # (no mode: these are the aligned forms)
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            form(aligner, panel, database, 5, algorithm="nw")
        with pytest.raises(ValueError, match="window must not be negative"):
            form(aligner, panel, database, 5, window=[3, -1, None])
        with pytest.raises(ValueError, match="window must not be negative"):
            form(aligner, panel, database, 5, window=-1)
        with pytest.raises(ValueError, match="at least 1"):
            form(aligner, panel, database, [5, 0, 5], algorithm="sw")
        with pytest.raises(TypeError, match="min_score must be an integer"):
            form(aligner, panel, database, [5, 2.5, 5])
        with pytest.raises(TypeError, match="min_score must be an integer"):
            form(aligner, panel, database, None)
        with pytest.raises(TypeError, match="window must be an integer or None"):
            form(aligner, panel, database, 5, window="3")
        with pytest.raises(ValueError, match="one value or one per query"):
            form(aligner, panel, database, [5, 5])
        with pytest.raises(ValueError, match="one value or one per query"):
            form(aligner, panel, database, 5, window=[1, 2, 3, 4])
        with pytest.raises(ValueError, match="max_hits must not be negative"):
            form(aligner, panel, database, 5, max_hits=-1)
        with pytest.raises(TypeError, match="must not be None"):
            form(aligner, ["ETSE", None], database, 5)
        with pytest.raises(IndexError):
            form(aligner, panel, database, 5, start=2, end=1)
        # a request with something to compute reaches the device
        with pytest.raises(AssertionError, match="device reached"):
            form(aligner, panel, database, 5)
    # find_occurrences_many keeps its own answer to mode="full", and says where the alignments are
    with pytest.raises(ValueError, match="find_occurrence_alignments_many"):
        pyopal_amd.find_occurrences_many(aligner, panel, database, 5, mode="full")
    # an empty panel, an empty slice, a panel of empty queries: answered without a device
    assert many(aligner, [], database, 5) == []
    assert many(aligner, panel, database, 5, start=1, end=1) == [[], [], []]
    assert many(aligner, panel, pyopal_amd.Database([]), [5, 6, 7], window=[None, 0, 1]) == [[], [], []]
    assert many(aligner, ["", ""], database, 5) == [[], []]
    small = ("score", "end_q", "end_t", "start_q", "start_t")
    for operations in (True, False):
        got = arrays(aligner, panel, database, 5, start=2, end=2, operations=operations)
        assert sorted(got) == sorted(("offsets", "target") + small + (("aln_flat", "aln_off") if operations else ()))
        assert got["offsets"].dtype == np.int64 and got["offsets"].tolist() == [0, 0, 0, 0]
        assert got["target"].dtype == np.int64 and all(got[key].dtype == np.int32 for key in small)
        assert all(len(got[key]) == 0 for key in ("target",) + small)
        if operations:
            assert got["aln_off"].dtype == np.int64 and got["aln_off"].tolist() == [0]
            assert got["aln_flat"].dtype == np.uint8 and len(got["aln_flat"]) == 0
