"""The batched search (miopalSearchBatch, Aligner.align_many / align_many_arrays) on the CPU tier:
the C ABI declares and exports it, and the Python layer validates its arguments like `align` and
answers an empty query list or an empty slice without a device."""
import os
import re
import threading

import numpy as np
import pytest

import pyopal_amd as pyopal
from pyopal_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_entry_points_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miopal.h")).read(), flags=re.S)
    for name in ("miopalSearchBatch", "miopalLastBatchRouting"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.EXPORTS
        assert hasattr(_capi.lib(), name), name
    assert hasattr(_capi.DeviceDatabase, "search_batch")
    assert hasattr(_capi.DeviceDatabase, "last_batch_routing")


def test_last_batch_routing_starts_at_zero():
    # (a thread that never ran a batch: the thread-local counters are zero - asked from a fresh thread, whatever this
    # one has run before)
    seen = []
    fresh = threading.Thread(target=lambda: seen.append(_capi.DeviceDatabase.last_batch_routing()))
    fresh.start()
    fresh.join()
    assert seen == [(0, 0, 0, 0)]


def test_align_many_argument_validation():
    a = pyopal.Aligner()
    db = pyopal.Database(["AACCGCTG"])
    for kw in (dict(mode="fast"), dict(algorithm="xx")):
        with pytest.raises(ValueError):
            a.align_many(["ACCTCG"], db, **kw)
        with pytest.raises(ValueError):
            a.align_many_arrays(["ACCTCG"], db, **kw)
    with pytest.raises(ValueError):
        a.align_many(["ACCTCG"], pyopal.Database(["ACGT"], "ACGT"))       # alphabets differ
    with pytest.raises(ValueError):
        a.align_many_arrays(["ACCTCG", "ACC-CG"], db)                     # bad query character
    with pytest.raises(IndexError):
        a.align_many(["ACCTCG"], db, start=1, end=0)
    with pytest.raises(IndexError):
        a.align_many_arrays(["ACCTCG"], db, start=2, end=5)               # start past the end
    with pytest.raises(OverflowError):
        a.align_many(["ACCTCG"], db, start=-1)
    with pytest.raises(TypeError):
        a.align_many(["ACCTCG"], ["AACCGCTG"])
    with pytest.raises(TypeError):
        a.align_many_arrays([None], db)
    with pytest.raises(ValueError):
        a.align_many_arrays(["ACCTCG"], db, mode="full")                  # arrays: score / end only


def test_align_many_empty_inputs_need_no_device():
    a = pyopal.Aligner()
    db = pyopal.Database(["AACCGCTG", "ACGT"])
    assert a.align_many([], db) == []
    assert a.align_many([], db, mode="full") == []
    assert a.align_many(["ACCTCG", "CCC"], pyopal.Database()) == [[], []]
    assert a.align_many(["ACCTCG"], db, start=1, end=1) == [[]]
    arrays = a.align_many_arrays([], db, mode="end")
    assert len(arrays) == 0 and arrays.score.shape == (0, 2) and arrays.query_end.shape == (0, 2)
    arrays = a.align_many_arrays(["ACCTCG", "CC"], db, mode="end", start=2)
    assert arrays.score.shape == (2, 0) and arrays.score.dtype == np.int32
    assert len(arrays[1]) == 0 and arrays[1].query_end.shape == (0,)
    assert list(arrays[-1]) == []
