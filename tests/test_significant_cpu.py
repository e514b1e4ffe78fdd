"""CPU tier of the significance searches (miopalSearchSignificant, miopalSearchPssmSignificant,
miopalSearchBatchSignificant, the test hooks miopalTestRowStats and miopalTestSelectHitsBinned; DeviceDatabase.
search_significant and its forms; Aligner.significant_hits and its forms; ScoreFit): the C ABI is declared, listed and
exported and the structure has the header's layout; ScoreFit's z-score, E-value and threshold are the header's
formulas; with no handle the checks that need none come first, in their documented order; the Python layer refuses bad
arguments before any device call and answers empty requests without a device."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import Pssm, ScoreFit, SignificantHits, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
NAMES = ("miopalSearchSignificant", "miopalSearchPssmSignificant", "miopalSearchBatchSignificant", "miopalTestRowStats",
         "miopalTestSelectHitsBinned")


def header():
    return open(os.path.join(ROOT, "include", "miopal.h")).read()


def prototype(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert found, f"{name} is not declared"
    return re.sub(r"\s+", " ", found.group(1)).strip()


def test_header_declares_the_entry_points():
    tail = "int64_t** targetIndex, int** score, int** endTarget, int** endQuery, double** evalue"
    args = prototype("miopalSearchSignificant")
    assert args.startswith("MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt, "
                           "const int* scoreMatrix, int alphabetLength, int searchType, int mode,")
    assert args.endswith("int64_t start, int64_t end, double maxEvalue, double excludeZ, int64_t maxHits, "
                         "MiopalScoreFit* fit, int64_t* count, " + tail)
    args = prototype("miopalSearchPssmSignificant")
    assert args.startswith("MiopalDb* db, const int* rowScores, int queryLength, int gapOpen, int gapExt, int alphabetLength,")
    assert args.endswith("double maxEvalue, double excludeZ, int64_t maxHits, MiopalScoreFit* fit, int64_t* count, " + tail)
    args = prototype("miopalSearchBatchSignificant")
    assert args.startswith("MiopalDb* db, const unsigned char* queries, const int64_t* queryOffsets, int nQueries,")
    assert args.endswith("const double* maxEvalue, double excludeZ, int64_t maxHits, MiopalScoreFit* fits, "
                         "int64_t* hitOffsets, " + tail)
    assert prototype("miopalTestRowStats") == ("const int* score, int rows, int64_t stride, const int32_t* length, "
                                               "const int32_t* ceiling, const int* skip, int64_t* stats, unsigned char* bin")
    assert prototype("miopalTestSelectHitsBinned") == (
        "const int* score, const int* endTarget, const int* endQuery, int rows, int64_t stride, const int32_t* length, "
        "const int32_t* threshold, int64_t start, int64_t* hitOffsets, int64_t** targetIndex, int** outScore, "
        "int** outEndTarget, int** outEndQuery")
    for name in NAMES:
        assert name in _capi.EXPORTS
    for name in ("search_significant", "search_pssm_significant", "search_batch_significant", "row_stats_rows",
                 "select_hits_binned_rows"):
        assert hasattr(_capi.DeviceDatabase, name)
    for name in ("significant_hits", "significant_hits_many", "significant_hits_pssm", "significant_hits_arrays",
                 "significant_hits_many_arrays", "significant_hits_pssm_arrays"):
        assert hasattr(pyopal_amd.Aligner, name)


def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names


def test_structure_has_the_header_layout():
    text = header()
    assert re.search(r"^#define\s+MIOPAL_STAT_BINS\s+128\s*$", text, re.M) and _capi.MIOPAL_STAT_BINS == 128
    assert re.search(r"^#define\s+MIOPAL_FIT_MAX_REFITS\s+3\s*$", text, re.M) and _capi.MIOPAL_FIT_MAX_REFITS == 3
    body = re.search(r"typedef struct MiopalScoreFit \{(.*?)\} MiopalScoreFit;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for kind, names in re.findall(r"(int64_t|int32_t|double)\s+([^;]+);", body):
        declared += [(re.match(r"\w+", n.strip()).group(0), kind, n.count("[")) for n in names.split(",")]
    sizes = {"int64_t": 8, "int32_t": 4, "double": 8}
    assert [d[0] for d in declared] == [f[0] for f in _capi.ScoreFit._fields_]
    for (name, kind, dims), (_, ctype) in zip(declared, _capi.ScoreFit._fields_):
        want = sizes[kind] * (1 if dims == 0 else 128 if dims == 1 else 128 * 3)
        assert ctypes.sizeof(ctype) == want, name
    # 2 + 1 + 4 words, two arrays of 128 words, two of 128 x 3, two of 128 half words: no padding
    assert ctypes.sizeof(_capi.ScoreFit) == 8 * (2 + 1 + 4 + 2 * 128 + 2 * 384) + 4 * 2 * 128 == 9272


def bin_of(L):
    if L == 0:
        return 0
    e = L.bit_length() - 1
    return 1 + 4 * e + ((L >> (e - 2)) & 3 if e >= 2 else (L << (2 - e)) & 3)


def test_length_bins_are_the_integer_definition():
    lengths = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 299, 300, 319, 320, 2 ** 20 - 1, 2 ** 20, 2 ** 31 - 1]
    assert _capi.length_bins(lengths).tolist() == [bin_of(L) for L in lengths]
    assert _capi.length_bins([1, 2, 3, 4, 2 ** 31 - 1]).tolist() == [1, 5, 7, 9, 124]
    with pytest.raises(ValueError):
        _capi.length_bins([-1])


def a_fit():
    """two populated bins (lengths 100 and 400) with hand-made sums"""
    raw = _capi.ScoreFit()
    raw.targets, raw.used, raw.passes, raw.degenerate = 1000, 990, 2, 0
    raw.intercept, raw.slope, raw.sigma, raw.zCut = 10.0, 5.0, 4.0, 3.5
    for b in range(128):
        raw.ceiling[b] = raw.threshold[b] = INT_MAX
    for L, n in ((100, 600), (400, 400)):
        b = bin_of(L)
        raw.binTargets[b], raw.binLength[b] = n, n * L
        raw.threshold[b] = math.ceil(10.0 + 5.0 * math.log(L) + 3.5 * 4.0)
    return ScoreFit(raw)


def test_score_fit_formulas():
    fit = a_fit()
    assert (fit.targets, fit.used, fit.passes, fit.degenerate, fit.z_cut) == (1000, 990, 2, False, 3.5)
    score = np.array([40, 60, 33, 90])
    length = np.array([100, 100, 400, 447])   # (384 .. 447 share a bin: the bin's mean length is what counts)
    mean = np.array([10 + 5 * math.log(100)] * 2 + [10 + 5 * math.log(400)] * 2)
    z = (score - mean) / 4.0
    assert np.allclose(fit.zscore(score, length), z, rtol=1e-14)
    p = 1 - np.exp(-np.exp(-(math.pi / math.sqrt(6)) * z - 0.5772156649015329))
    assert np.allclose(fit.evalue(score, length), 1000 * p, rtol=1e-9)
    assert fit.evalue(1000, 100) < 1e-100 and abs(fit.evalue(-1000, 100) - 1000) < 1e-9   # both tails, no cancellation
    assert fit.threshold(length).tolist() == [fit.thresholds[bin_of(100)]] * 2 + [fit.thresholds[bin_of(400)]] * 2
    assert fit.threshold([0, 7]).tolist() == [INT_MAX, INT_MAX]          # empty targets, a bin without targets
    assert np.isnan(fit.zscore(5, 7)) and np.isnan(fit.bin_means()[0])
    # a score at the threshold has z >= z_cut and an E-value within the cut that z_cut stands for
    at = fit.threshold([100, 400])
    assert np.all(fit.zscore(at, [100, 400]) >= 3.5) and np.all(fit.zscore(at - 1, [100, 400]) < 3.5)
    empty = ScoreFit()
    assert empty.degenerate and empty.targets == 0 and np.all(empty.thresholds == INT_MAX)
    assert np.isnan(empty.zscore([1, 2], [3, 4])).all() and np.isnan(empty.evalue(1, 3))
    assert "degenerate=True" in repr(empty)


class Outputs:
    """A count (or three offsets), four array pointers and the E-value pointer, all set to a mark no call may change."""
    MARK = 0x77

    def __init__(self):
        self.count = np.full(3, 77, dtype=np.int64)
        self.ptrs = [ctypes.c_void_p(self.MARK) for _ in range(5)]
        self.fit = (_capi.ScoreFit * 2)()
        ctypes.memset(self.fit, 0x5A, ctypes.sizeof(self.fit))

    def refs(self, missing=()):
        return [None if i in missing else ctypes.byref(p) for i, p in enumerate(self.ptrs)]

    def untouched(self):
        return (np.all(self.count == 77) and all(p.value == self.MARK for p in self.ptrs) and
                bytes(self.fit) == b"\x5a" * ctypes.sizeof(self.fit))


def test_pssm_form_reports_argument_errors_before_a_device():
    """miopalSearchPssmSignificant with no handle: miopalSearchPssmHits' order, the fit and E-value outputs and the cut
    behind the null outputs, and then the missing handle."""
    lib = _capi.lib()
    rows = np.ones((4, 32), dtype=np.int32)
    out = Outputs()

    def call(q=4, alphabet=32, st=1, mode=3, count=True, missing=(), fit=True, cut=1e-3, z=5.0):
        return lib.miopalSearchPssmSignificant(
            None, rows.ctypes.data, q, 3, 1, alphabet, st, mode, 0, 2, cut, z, -1,
            ctypes.addressof(out.fit) if fit else None,
            out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if count else None, *out.refs(missing))

    assert call(mode=4) == INVALID and "alignment mode" in _capi.last_error()
    assert call(st=3) == INVALID and "search type" in _capi.last_error()
    assert call(q=-1) == BAD and "query length" in _capi.last_error()
    assert call(alphabet=33) == BAD and "alphabet length" in _capi.last_error()
    assert call(st=2) == INVALID and "alignments are not selected" in _capi.last_error()   # mode "full" at the C level
    assert call(st=2, fit=False, cut=-1.0) == INVALID
    assert call(count=False) == BAD and "null count" in _capi.last_error()
    assert call(missing=(0,), fit=False) == BAD and "null target / score" in _capi.last_error()
    assert call(missing=(2,), cut=0.0) == BAD and "null end-location" in _capi.last_error()
    assert call(fit=False) == BAD and "null fit" in _capi.last_error()
    assert call(fit=False, cut=0.0) == BAD and "null fit" in _capi.last_error()
    assert call(missing=(4,)) == BAD and "null evalue" in _capi.last_error()
    for cut in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(cut=cut) == BAD and "maxEvalue" in _capi.last_error(), cut
    assert call(z=math.nan) == BAD and "excludeZ" in _capi.last_error()
    assert call(cut=0.0, z=math.nan) == BAD and "maxEvalue" in _capi.last_error()
    # nothing wrong with the arguments: the handle is what is missing (any finite or infinite excludeZ is an argument)
    for z in (5.0, 0.0, -3.0, math.inf):
        assert call(z=z) == BAD and "null database handle" in _capi.last_error()
    assert call(st=0, missing=(2, 3)) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_plain_and_batch_forms_look_at_the_handle_first():
    lib = _capi.lib()
    query = np.zeros(8, dtype=np.uint8)
    matrix = np.ones(24 * 24, dtype=np.int32)
    offsets = np.array([0, 3, 8], dtype=np.int64)
    cuts = np.array([1e-3, math.nan])
    out = Outputs()
    for st, cut, fit in ((0, 1e-3, True), (2, 1e-3, True), (1, math.nan, True), (1, 1e-3, False)):
        rc = lib.miopalSearchSignificant(None, query.ctypes.data, 4, 3, 1, matrix.ctypes.data, 24, st, 3, 0, 2, cut, 5.0, -1,
                                         ctypes.addressof(out.fit) if fit else None,
                                         out.count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), *out.refs())
        assert rc == BAD and "null database handle" in _capi.last_error(), (st, cut, fit)

    def batch(st=1, n=2, off=offsets):
        return lib.miopalSearchBatchSignificant(None, query.ctypes.data, off.ctypes.data, n, 3, 1, matrix.ctypes.data, 24,
                                                st, 3, 0, 2, cuts.ctypes.data, 5.0, -1, ctypes.addressof(out.fit),
                                                out.count.ctypes.data, *out.refs())

    assert batch(st=2) == INVALID and "alignments are not selected" in _capi.last_error()
    assert batch(n=-1) == BAD and "bad query list" in _capi.last_error()
    assert batch(off=np.array([5, 3, 8], dtype=np.int64)) == BAD and "bad query offsets at 0" in _capi.last_error()
    assert batch() == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_hooks_refuse_bad_arguments_before_a_device():
    lib = _capi.lib()
    score = np.zeros((2, 8), dtype=np.int32)
    length = np.arange(8, dtype=np.int32)
    table = np.zeros((2, 128), dtype=np.int32)
    stats = np.full((2, 128, 3), 77, dtype=np.int64)
    bins = np.full(8, 77, dtype=np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731

    def row_stats(s=score, rows=2, stride=8, lengths=length, out=stats, b=bins):
        return lib.miopalTestRowStats(ptr(s), rows, stride, ptr(lengths), None, None, ptr(out), ptr(b))

    for rows, stride in ((0, 8), (-1, 8), (2, 0), (2, -3)):
        assert row_stats(rows=rows, stride=stride) == BAD and "both at least 1" in _capi.last_error()
    assert row_stats(s=None) == BAD and "null score rows" in _capi.last_error()
    assert row_stats(lengths=None) == BAD and "lengths" in _capi.last_error()
    assert row_stats(out=None) == BAD and row_stats(b=None) == BAD and "null stats / bin" in _capi.last_error()
    negative = length.copy()
    negative[5] = -1
    assert row_stats(lengths=negative) == BAD and "negative length at 5" in _capi.last_error()
    for rows, stride in ((2, 2 ** 26 + 1), (2 ** 27 + 1, 1), (3, 2 ** 62)):
        assert row_stats(rows=rows, stride=stride) == BAD and "more than 2^27" in _capi.last_error()
    assert np.all(stats == 77) and np.all(bins == 77)

    out = Outputs()
    ends = np.zeros((2, 8), dtype=np.int32)

    def binned(s=score, et=None, eq=None, rows=2, stride=8, lengths=length, t=table, offsets=True, missing=()):
        return lib.miopalTestSelectHitsBinned(ptr(s), ptr(et), ptr(eq), rows, stride, ptr(lengths), ptr(t), 0,
                                              out.count.ctypes.data if offsets else None, *out.refs(missing)[:4])

    for rows, stride in ((0, 8), (2, -3)):
        assert binned(rows=rows, stride=stride) == BAD and "both at least 1" in _capi.last_error()
    assert binned(s=None) == BAD and "null score rows" in _capi.last_error()
    assert binned(lengths=None) == BAD and "null lengths / threshold" in _capi.last_error()
    assert binned(t=None) == BAD and "null lengths / threshold" in _capi.last_error()
    assert binned(et=ends) == BAD and "one end array without the other" in _capi.last_error()
    assert binned(offsets=False) == BAD and "null hitOffsets" in _capi.last_error()
    assert binned(missing=(0,)) == BAD and binned(missing=(1,)) == BAD
    assert binned(et=ends, eq=ends, missing=(3,)) == BAD and "null end-location" in _capi.last_error()
    assert binned(rows=2, stride=2 ** 26 + 1) == BAD and "more than 2^27" in _capi.last_error()
    assert binned(lengths=negative) == BAD and "negative length at 5" in _capi.last_error()
    assert out.untouched()
    # the Python wrappers check shapes themselves
    with pytest.raises(ValueError, match="one entry per column"):
        _capi.row_stats_rows(score, length[:5])
    with pytest.raises(ValueError, match="128 entries"):
        _capi.row_stats_rows(score, length, np.zeros(5))
    with pytest.raises(ValueError, match="128 entries"):
        _capi.select_hits_binned_rows(score, length, np.zeros((3, 128)))


@pytest.fixture
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture
def database():
    return pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])


def forms(aligner, database):
    pssm = Pssm.from_sequence("MKV")
    a = aligner
    return [
        ("significant_hits", lambda cut=1e-3, db=database, **kw: a.significant_hits("MKV", db, cut, **kw)),
        ("significant_hits_arrays", lambda cut=1e-3, db=database, **kw: a.significant_hits_arrays("MKV", db, cut, **kw)),
        ("significant_hits_many", lambda cut=1e-3, db=database, **kw: a.significant_hits_many(["MKV", "A"], db, cut, **kw)),
        ("significant_hits_many_arrays",
         lambda cut=1e-3, db=database, **kw: a.significant_hits_many_arrays(["MKV", "A"], db, cut, **kw)),
        ("significant_hits_pssm", lambda cut=1e-3, db=database, **kw: a.significant_hits_pssm(pssm, db, cut, **kw)),
        ("significant_hits_pssm_arrays",
         lambda cut=1e-3, db=database, **kw: a.significant_hits_pssm_arrays(pssm, db, cut, **kw)),
    ]


def test_python_validation_comes_before_any_device_call(aligner, database, monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    for name, call in forms(aligner, database):
        for kw in (dict(mode="sorted"), dict(algorithm="blast"), dict(start=2, end=1), dict(start=10), dict(start=-1),
                   dict(end=-1)):
            with pytest.raises(Exception) as want:
                aligner.hits("MKV", database, 3, **kw)
            with pytest.raises(type(want.value)) as got:
                call(**kw)
            assert str(got.value) == str(want.value), (name, kw)
        for value in (0, 0.0, -1e-3, math.nan, math.inf, -math.inf):
            with pytest.raises(ValueError, match="max_evalue must be finite and positive"):
                call(cut=value)
        for value in ("1e-3", None, True, [1e-3] if "many" not in name else "x"):
            with pytest.raises(TypeError, match="max_evalue must be a number"):
                call(cut=value)
        with pytest.raises(ValueError, match="exclude_z must not be NaN"):
            call(exclude_z=math.nan)
        for value in ("5", None, True):
            with pytest.raises(TypeError, match="exclude_z must be a number"):
                call(exclude_z=value)
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
        aligner.significant_hits_pssm("MKV", database, 1e-3)
    with pytest.raises(TypeError, match="must not be None"):
        aligner.significant_hits(None, database, 1e-3)
    for wrong in ([1.0], [1.0, 2.0, 3.0], np.array([1.0, 2.0, 3.0])):
        with pytest.raises(ValueError, match="one per query"):
            aligner.significant_hits_many(["MKV", "A"], database, wrong)
    with pytest.raises(ValueError, match="finite and positive"):
        aligner.significant_hits_many(["MKV", "A"], database, [1.0, 0.0])
    # the device layer refuses the same before its C call
    handle = _capi.DeviceDatabase.__new__(_capi.DeviceDatabase)
    handle.count, handle.alphabet_length, handle._h = 3, 24, None
    query, matrix = np.zeros(3, dtype=np.uint8), np.ones((24, 24), dtype=np.int32)
    for cut, z in ((0.0, 5.0), (math.nan, 5.0), (math.inf, 5.0), (1.0, math.nan)):
        with pytest.raises(ValueError):
            handle.search_significant(query, matrix, max_evalue=cut, exclude_z=z)
        with pytest.raises(ValueError):
            handle.search_pssm_significant(np.ones((3, 24), dtype=np.int32), max_evalue=cut, exclude_z=z)
        with pytest.raises(ValueError):
            handle.search_batch_significant([query], matrix, max_evalue=[cut], exclude_z=z)


def test_empty_answers_need_no_device(aligner, database, monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    for mode in ("score", "end", "full"):
        for name, call in forms(aligner, database):
            for kw in (dict(start=1, end=1), dict(start=3)):
                got = call(mode=mode, **kw)
                rows = 2 if "many" in name else 1
                if name.endswith("_arrays"):
                    assert got["offsets"].tolist() == [0] * (rows + 1) and len(got["target"]) == 0
                    assert got["evalue"].dtype == np.float64 and len(got["evalue"]) == 0 and len(got["zscore"]) == 0
                    assert ("end_q" in got) == (mode != "score") and ("aln_flat" in got) == (mode == "full")
                    fits = got["fits"] if "many" in name else [got["fit"]]
                    assert len(fits) == rows and all(isinstance(f, ScoreFit) and f.degenerate for f in fits)
                else:
                    answers = got if "many" in name else [got]
                    assert len(answers) == rows
                    for answer in answers:
                        assert isinstance(answer, SignificantHits) and len(answer) == 0 and list(answer) == []
                        assert answer.results == [] and answer.fit.degenerate and answer.fit.targets == 0
        assert aligner.significant_hits_many([], database, 1e-3, mode=mode) == []
        assert aligner.significant_hits_many([], database, [], mode=mode) == []
        assert aligner.significant_hits_many_arrays([], database, 1.0, mode=mode)["offsets"].tolist() == [0]


def test_well_formed_calls_fail_loudly_without_a_device(aligner, database):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for name, call in forms(aligner, database):
        with pytest.raises(RuntimeError, match="no supported SIMD backend"):
            call()
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.row_stats_rows(np.zeros((2, 8), dtype=np.int32), np.arange(8))
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.select_hits_binned_rows(np.zeros((2, 8), dtype=np.int32), np.arange(8), np.zeros(128))
