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
