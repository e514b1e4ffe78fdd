"""CPU tier of the top-k selection (miopalSearchTop / miopalSearchBatchTop, Aligner.top_hits / top_hits_many): the C ABI
is declared, listed and exported, and the Python layer checks its arguments and answers empty requests without a
device."""
import os
import re
import subprocess

import pytest

import pyopal_amd
from pyopal_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "miopal.h")


def test_header_declares_the_entry_points_and_the_bound():
    text = open(HEADER).read()
    assert re.search(r"#define\s+MIOPAL_MAX_TOP\s+4096\b", text)
    for name in ("miopalSearchTop", "miopalSearchBatchTop"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _capi.EXPORTS
    assert _capi.MIOPAL_MAX_TOP == 4096


def test_library_exports_the_entry_points():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libmiopal.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"miopalSearchTop", "miopalSearchBatchTop"} <= names


@pytest.fixture
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture
def database():
    return pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])


@pytest.mark.parametrize("method", ["top_hits", "top_hits_many"])
def test_validation(aligner, database, method):
    call = getattr(aligner, method)
    q = "MKV" if method == "top_hits" else ["MKV", "A"]
    for k in (1.0, "3", None, True):
        with pytest.raises(TypeError):
            call(q, database, k)
    for k in (-1, _capi.MIOPAL_MAX_TOP + 1):
        with pytest.raises(ValueError, match="4096"):
            call(q, database, k)
    with pytest.raises(ValueError):
        call(q, database, 3, mode="sorted")
    with pytest.raises(ValueError):
        call(q, database, 3, algorithm="blast")
    with pytest.raises(IndexError):
        call(q, database, 3, start=2, end=1)
    with pytest.raises(IndexError):
        call(q, database, 3, start=10)
    with pytest.raises(OverflowError):
        call(q, database, 3, start=-1)
    with pytest.raises(TypeError):
        call(None if method == "top_hits" else ["MK", None], database, 3)
    with pytest.raises(TypeError):
        call(q, ["MKV"], 3)
    with pytest.raises(ValueError):
        call(q, pyopal_amd.Database(["ACGT"], alphabet="ACGT"), 3)


def test_empty_answers_need_no_device(aligner, database, monkeypatch):
    # (no device is reached: the library's device count is never asked for)
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    assert aligner.top_hits("MKV", database, 0) == []
    assert aligner.top_hits("MKV", database, 5, start=1, end=1) == []
    assert aligner.top_hits("MKV", database, 5, start=3) == []
    assert aligner.top_hits_many([], database, 5) == []
    assert aligner.top_hits_many(["MKV", "A"], database, 0, mode="full") == [[], []]
    assert aligner.top_hits_many(["MKV"], database, 4, start=2, end=2) == [[]]


# ---- miopalTestSelectTop: the selection on caller-supplied rows (test hook). Its arguments are refused before any
# device call, so the refusals are checked here, where there is no device. ----

def test_select_rows_hook_is_declared_listed_and_exported():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+miopalTestSelectTop\s*\(", text)
    assert "miopalTestSelectTop" in _capi.EXPORTS
    assert hasattr(_capi.lib(), "miopalTestSelectTop")


def _hook(score, end_t, end_q, rows, stride, k, outs="ctse", ends_out=True, gave_up=True):
    """The raw call with outputs of the right sizes; `outs` names the ones that are not NULL (count, target, score,
    ends)."""
    import ctypes
    import numpy as np
    rk = max(rows, 1) * max(k, 1)
    count = np.zeros(max(rows, 1), dtype=np.int32)
    target = np.zeros(rk, dtype=np.int64)
    out_score = np.zeros(rk, dtype=np.int32)
    out_et = np.zeros(rk, dtype=np.int32)
    out_eq = np.zeros(rk, dtype=np.int32)
    gave = ctypes.c_int(-7)
    p = _capi._ptr
    rc = _capi.lib().miopalTestSelectTop(
        p(score), p(end_t), p(end_q), rows, stride, k, -(2 ** 31), 0,
        p(count) if "c" in outs else None, p(target) if "t" in outs else None, p(out_score) if "s" in outs else None,
        p(out_et) if "e" in outs and ends_out else None, p(out_eq) if "e" in outs and ends_out else None,
        ctypes.byref(gave) if gave_up else None)
    return rc, gave.value


def test_select_rows_hook_refuses_bad_arguments():
    import numpy as np
    BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
    # (the refusals come before any device call: without a device, a call that got past them returns another code)
    score = np.arange(12, dtype=np.int32)
    ends = np.arange(12, dtype=np.int32)
    cases = {
        "rows 0": (score, None, None, 0, 12, 3, {}),
        "rows -1": (score, None, None, -1, 12, 3, {}),
        "stride 0": (score, None, None, 3, 0, 3, {}),
        "stride -4": (score, None, None, 3, -4, 3, {}),
        "k 0": (score, None, None, 3, 4, 0, {}),
        "k -1": (score, None, None, 3, 4, -1, {}),
        "k above the bound": (score, None, None, 3, 4, _capi.MIOPAL_MAX_TOP + 1, {}),
        "null scores": (None, None, None, 3, 4, 3, {}),
        "null count": (score, None, None, 3, 4, 3, {"outs": "tse"}),
        "null target": (score, None, None, 3, 4, 3, {"outs": "cse"}),
        "null score output": (score, None, None, 3, 4, 3, {"outs": "cte"}),
        "null gaveUp": (score, None, None, 3, 4, 3, {"gave_up": False}),
        "null end outputs with end arrays": (score, ends, ends, 3, 4, 3, {"ends_out": False}),
        "end targets only": (score, ends, None, 3, 4, 3, {}),
        "end queries only": (score, None, ends, 3, 4, 3, {}),
        # (refused on their sizes alone: the 12 entries behind the pointer are never read)
        "2^27 + 1 entries in one row": (score, None, None, 1, 2 ** 27 + 1, 1, {}),
        "2 rows of 2^26 + 1": (score, None, None, 2, 2 ** 26 + 1, 1, {}),
        "rows x stride past 2^63": (score, None, None, 2 ** 31 - 1, 2 ** 62, 1, {}),
    }
    for name, (s, et, eq, rows, stride, k, kw) in cases.items():
        rc, gave = _hook(s, et, eq, rows, stride, k, **kw)
        assert rc == BAD, (name, rc, _capi.last_error())
        assert _capi.last_error(), name
        assert gave == -7 or not kw.get("gave_up", True), name   # (nothing was written)


def test_select_top_rows_passes_the_refusal_on():
    import numpy as np
    score = np.zeros((2, 5), dtype=np.int32)
    for k in (0, _capi.MIOPAL_MAX_TOP + 1):
        with pytest.raises(RuntimeError, match="code=101"):
            _capi.select_top_rows(score, k)
    with pytest.raises(RuntimeError, match="code=101"):
        _capi.select_top_rows(score, 3, end_q=np.zeros((2, 5), dtype=np.int32))
    with pytest.raises(RuntimeError, match="code=101"):
        _capi.select_top_rows(np.zeros((3, 0), dtype=np.int32), 3)
    with pytest.raises(ValueError):
        _capi.select_top_rows(score, 3, end_q=np.zeros((2, 4), dtype=np.int32), end_t=np.zeros((2, 5), dtype=np.int32))
