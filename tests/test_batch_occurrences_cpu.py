"""CPU tier of the occurrence search of a panel of queries (miopalSearchBatchOccurrences,
miopalLastBatchOccurrenceRouting; DeviceDatabase.search_batch_occurrences; pyopal_amd.find_occurrences_many): the two
symbols are declared, listed and exported; with no handle the call is refused with every output as it was; the Python
layers refuse the rule's faults before they reach the library; an empty panel is answered without a device."""
import ctypes
import subprocess
import threading

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import _capi

from test_occurrences_cpu import BAD, Outputs, prototype

NAMES = ("miopalSearchBatchOccurrences", "miopalLastBatchOccurrenceRouting", "miopalLastBatchOccurrenceGroups")


def test_header_declares_the_entry_points():
    assert prototype("miopalSearchBatchOccurrences") == (
        "MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries, int gapOpen, int gapExt, "
        "const int* scoreMatrix, int alphabetLength, int mode, int64_t start, int64_t end, const int* minScore, "
        "const int* window, int64_t maxHits, int64_t* hitOffsets, int64_t** targetIndex, int** score, int** endTarget, "
        "int** endQuery")
    assert prototype("miopalLastBatchOccurrenceRouting") == "int64_t counts[4]"
    assert prototype("miopalLastBatchOccurrenceGroups") == "int64_t counts[3]"
    for name in NAMES:
        assert name in _capi.EXPORTS
    assert hasattr(_capi.DeviceDatabase, "search_batch_occurrences")
    assert hasattr(_capi.DeviceDatabase, "last_batch_occurrence_routing")
    assert hasattr(_capi.DeviceDatabase, "last_batch_occurrence_groups")


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names
    lib = _capi.lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    seen = []
    fresh = threading.Thread(target=lambda: seen.append(_capi.last_batch_occurrence_routing()))
    fresh.start()
    fresh.join()
    assert seen == [[0, 0, 0, 0]]
    lib.miopalLastBatchOccurrenceRouting(None)
    lib.miopalLastBatchOccurrenceGroups(None)
    assert _capi.last_batch_occurrence_groups() == [0, 0, 0]


def test_no_handle_is_refused_with_the_outputs_as_they_were():
    lib = _capi.lib()
    out = Outputs()
    queries = np.zeros(6, dtype=np.uint8)
    offsets = np.array([0, 2, 6], dtype=np.int64)
    matrix = np.ones(16, dtype=np.int32)
    cuts, windows = np.array([3, 3], dtype=np.int32), np.array([2, 2], dtype=np.int32)

    def call(n=2, q=queries, off=offsets):
        return lib.miopalSearchBatchOccurrences(None, None if q is None else q.ctypes.data,
                                                None if off is None else off.ctypes.data, n, 3, 1, matrix.ctypes.data, 4,
                                                1, 0, 2, cuts.ctypes.data, windows.ctypes.data, -1, out.count.ctypes.data,
                                                *out.refs())

    assert call(n=-1) == BAD and "bad query list" in _capi.last_error()
    assert call(off=None) == BAD and "bad query list" in _capi.last_error()
    assert call() == BAD and "null database handle" in _capi.last_error()
    assert call(n=0) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


class _NoHandle(_capi.DeviceDatabase):
    """a DeviceDatabase that owns no handle: what its methods refuse before they call the library"""

    def __init__(self, alphabet_length=4):
        self._h, self.count, self.alphabet_length = None, 3, alphabet_length


def test_device_database_refusals_come_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    db = _NoHandle()
    panel = [np.zeros(n, dtype=np.uint8) for n in (4, 0, 9, 70, 2)]
    matrix = np.ones(16, dtype=np.int32)
    call = lambda **kw: db.search_batch_occurrences(panel, matrix, 3, 1, **kw)   # noqa: E731
    for algorithm in ("nw", "ov", "blast"):
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            call(algorithm=algorithm, min_score=3)
    with pytest.raises(ValueError, match="window must not be negative"):
        call(min_score=3, window=[0, None, 5, -1, 2])
    with pytest.raises(ValueError, match="window must not be negative"):
        call(min_score=3, window=-1)
    with pytest.raises(ValueError, match="at least 1"):
        call(algorithm="sw", min_score=[5, 5, 5, 0, 5])
    with pytest.raises(ValueError, match="one value or one per query"):
        call(min_score=[1, 2, 3])
    with pytest.raises(ValueError, match="one value or one per query"):
        call(min_score=1, window=[1, 2, 3, 4, 5, 6])
    with pytest.raises(OverflowError):
        call(min_score=2 ** 31)
    # nothing wrong with these: the library is what they reach
    for kw in (dict(min_score=-(2 ** 31), window=0), dict(algorithm="sw", min_score=1),
               dict(min_score=[1, 2, 3, 4, 5], window=[None, 0, 5, None, 1])):
        with pytest.raises(AssertionError, match="device reached"):
            call(**kw)


def test_find_occurrences_many_faults_and_empty_requests(monkeypatch):
    assert pyopal_amd.find_occurrences_many is pyopal_amd.occurrences.find_occurrences_many
    assert pyopal_amd.find_occurrences_many_arrays is pyopal_amd.occurrences.find_occurrences_many_arrays
    assert not any(hasattr(pyopal_amd.Aligner, name) for name in ("find_occurrences_many", "find_occurrences_many_arrays"))
    aligner = pyopal_amd.Aligner(gap_open=11, gap_extend=1)
    database = pyopal_amd.Database(["MKVLA", "ETSEEES", ""])
    panel = ["ETSE", "", "KVL"]
    # the rule's faults, before a mirror of the database is asked for
    monkeypatch.setattr(pyopal_amd.lib._Request, "mirror", lambda self: (_ for _ in ()).throw(AssertionError("device reached")))
    for form in (pyopal_amd.find_occurrences_many, pyopal_amd.find_occurrences_many_arrays):
        with pytest.raises(ValueError, match="alignments of a panel.*not available yet"):
            form(aligner, panel, database, 5, mode="full")
        with pytest.raises(ValueError, match="'end' or 'full'"):
            form(aligner, panel, database, 5, mode="score")
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            form(aligner, panel, database, 5, algorithm="nw")
        with pytest.raises(ValueError, match="window must not be negative"):
            form(aligner, panel, database, 5, window=[3, -1, None])
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
    # an empty panel, an empty slice, a panel of empty queries: answered without a device
    assert pyopal_amd.find_occurrences_many(aligner, [], database, 5) == []
    assert pyopal_amd.find_occurrences_many(aligner, panel, database, 5, start=1, end=1) == [[], [], []]
    assert pyopal_amd.find_occurrences_many(aligner, panel, pyopal_amd.Database([]), [5, 6, 7], window=[None, 0, 1]) == [[], [], []]
    assert pyopal_amd.find_occurrences_many(aligner, ["", ""], database, 5) == [[], []]
    got = pyopal_amd.find_occurrences_many_arrays(aligner, panel, database, 5, start=2, end=2)
    assert sorted(got) == ["end_q", "end_t", "offsets", "score", "target"]
    assert got["offsets"].dtype == np.int64 and got["offsets"].tolist() == [0, 0, 0, 0]
    assert got["target"].dtype == np.int64 and all(got[key].dtype == np.int32 for key in ("score", "end_q", "end_t"))
    assert all(len(got[key]) == 0 for key in ("target", "score", "end_q", "end_t"))
