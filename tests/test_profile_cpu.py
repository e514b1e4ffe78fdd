"""CPU tier of the profile columns (miopalProfileColumns / miopalProfileColumnsPssm, the test hook
miopalTestProfileColumns; DeviceDatabase.profile_columns / profile_columns_pssm, _capi.profile_columns_rows;
Aligner.profile_columns / iterated_search, ProfileColumns, Pssm.from_columns, matrix_lambda): the C ABI is declared,
listed and exported; the Python prototypes have the header's arity; with no handle and no device the checks come in the
header's order with its codes; the hook refuses bad arguments before any device call; the Python layer checks its
arguments as `align_pairs` does and answers an empty target list without a device; the host arithmetic of the next
round's PSSM is the formula of the docstring."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _profile
import pyopal_amd
from pyopal_amd import _capi
from pyopal_amd.matrices import ScoringMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 101   # MIOPAL_ERR_BAD_ARGUMENT (include/opal.h)
INVALID = _capi.OPAL_ERR_INVALID_MODE
NAMES = ("miopalProfileColumns", "miopalProfileColumnsPssm", "miopalTestProfileColumns")
TAIL = ("const int64_t* targets, int64_t nTargets, "
        "int64_t* counts, int64_t* weighted, int64_t* memberWeight, unsigned char* msa")


def prototype(name):
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert found, f"{name} is not declared"
    return re.sub(r"\s+", " ", found.group(1)).strip()


def test_header_declares_the_entry_points():
    assert prototype("miopalProfileColumns") == (
        "MiopalDb* db, const unsigned char* query, int queryLength, int gapOpen, int gapExt, "
        "const int* scoreMatrix, int alphabetLength, int mode, " + TAIL)
    assert prototype("miopalProfileColumnsPssm") == (
        "MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength, "
        "int gapOpen, int gapExt, int alphabetLength, int mode, " + TAIL)
    assert prototype("miopalTestProfileColumns") == (
        "const unsigned char* msa, int64_t members, int queryLength, int alphabetLength, "
        "int64_t* counts, int64_t* weighted, int64_t* memberWeight")
    text = open(os.path.join(ROOT, "include", "miopal.h")).read()
    assert re.search(r"^#define\s+MIOPAL_PROFILE_WEIGHT_ONE\s+\(1ll << 32\)\s*$", text, re.M)
    assert _capi.MIOPAL_PROFILE_WEIGHT_ONE == 2 ** 32 == _profile.ONE
    for name in NAMES:
        assert name in _capi.EXPORTS
    for name in ("profile_columns", "profile_columns_pssm"):
        assert hasattr(_capi.DeviceDatabase, name)
    assert callable(_capi.profile_columns_rows)
    for name in ("profile_columns", "iterated_search"):
        assert hasattr(pyopal_amd.Aligner, name)
    assert hasattr(pyopal_amd.Pssm, "from_columns") and callable(pyopal_amd.matrix_lambda)
    assert pyopal_amd.ProfileColumns.WEIGHT_ONE == 2 ** 32


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
    """counts, weighted, memberWeight and msa, all set to a mark that no failing call may change"""

    def __init__(self, cells=512):
        self.arrays = [np.full(cells, 77, dtype=np.int64) for _ in range(3)] + [np.full(cells, 77, dtype=np.uint8)]

    def ptrs(self, missing=()):
        return [None if i in missing else a.ctypes.data for i, a in enumerate(self.arrays)]

    def untouched(self):
        return all(np.all(a == 77) for a in self.arrays)


def ptr(a):
    return None if a is None else a.ctypes.data


def test_plain_entry_reports_argument_errors_before_a_device():
    """miopalProfileColumns with no handle: miopalAlignPairs' checks of the list (query, targets[p]) in its order - the
    mode, the query and its residues, the target list - end with the handle; the outputs and the size of the multiple
    alignment, checked after them, are not reached."""
    lib = _capi.lib()
    query = np.array([0, 5, 7, 2], dtype=np.uint8)
    matrix = np.ones(24 * 24, dtype=np.int32)
    targets = np.array([0, 1, 1], dtype=np.int64)
    out = Outputs()

    def call(q=query, n_q=4, s=matrix, a=24, mode=3, t=targets, n=3, missing=()):
        return lib.miopalProfileColumns(None, ptr(q), n_q, 3, 1, ptr(s), a, mode, ptr(t), n, *out.ptrs(missing))

    for mode in (-1, 4, 9):
        assert call(mode=mode) == INVALID and "invalid alignment mode" in _capi.last_error()
    assert call(mode=9, q=None, n=-1, missing=(0, 1, 2)) == INVALID
    assert call(q=None) == BAD and "bad query list" in _capi.last_error()
    assert call(s=None) == BAD and "bad score matrix" in _capi.last_error()
    for a in (0, -1, 33):
        assert call(a=a) == BAD and "alphabet length" in _capi.last_error()
    assert call(n_q=-1) == BAD and "bad query offsets at 0" in _capi.last_error()
    assert call(q=np.array([0, 5, 24, 2], dtype=np.uint8)) == BAD and "query residue 24 out of range at 2" in _capi.last_error()
    assert call(n=-1) == BAD and "bad pair list" in _capi.last_error()
    assert call(t=None) == BAD and "bad pair list" in _capi.last_error()
    # the handle ends the checks that can be made without one: what comes after it is never looked at
    assert call() == BAD and "null database handle" in _capi.last_error()
    assert call(n=0, t=None) == BAD and "null database handle" in _capi.last_error()
    assert call(n_q=0, q=None) == BAD and "null database handle" in _capi.last_error()
    for k in (0, 1, 2, 3):
        assert call(missing=(k,)) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_pssm_entry_reports_argument_errors_before_a_device():
    """miopalProfileColumnsPssm with no handle: what miopalAlignPairsPssm checks without one, in its order - the mode,
    the rows, the alphabet length, the consensus - then the target list and the handle."""
    lib = _capi.lib()
    rows = np.ones((4, 24), dtype=np.int32)
    consensus = np.array([0, 255, 7, 2], dtype=np.uint8)
    targets = np.array([0, 1, 1], dtype=np.int64)
    out = Outputs()

    def call(r=rows, c=consensus, n_q=4, a=24, mode=3, t=targets, n=3, missing=()):
        return lib.miopalProfileColumnsPssm(None, ptr(r), ptr(c), n_q, 3, 1, a, mode, ptr(t), n, *out.ptrs(missing))

    assert call(mode=4, r=None, a=0) == INVALID and "invalid alignment mode" in _capi.last_error()
    assert call(n_q=-1, r=None) == BAD and "bad query length -1" in _capi.last_error()
    assert call(r=None, a=0) == BAD and "null row scores" in _capi.last_error()
    for a in (0, -1, 33):
        assert call(a=a, c=None) == BAD and "bad alphabet length" in _capi.last_error()
    assert call(c=None, n=-1) == BAD and "null consensus" in _capi.last_error()
    bad = np.array([0, 255, 24, 2], dtype=np.uint8)
    assert call(c=bad, n=-1) == BAD and "consensus residue 24 out of range at 2" in _capi.last_error()
    assert call(n=-1) == BAD and "bad pair list" in _capi.last_error()
    assert call(t=None) == BAD and "bad pair list" in _capi.last_error()
    assert call() == BAD and "null database handle" in _capi.last_error()
    assert call(n_q=0, r=None, c=None) == BAD and "null database handle" in _capi.last_error()
    for k in (0, 1, 2, 3):
        assert call(missing=(k,)) == BAD and "null database handle" in _capi.last_error()
    assert out.untouched()


def test_hook_refuses_bad_arguments_before_a_device():
    lib = _capi.lib()
    msa = np.array([[0, 24, 255, 3], [23, 1, 1, 255]], dtype=np.uint8)
    out = Outputs()

    def call(m=msa, members=2, q=4, a=24, missing=()):
        return lib.miopalTestProfileColumns(ptr(m), members, q, a, *out.ptrs(missing)[:3])

    for members, q in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        assert call(members=members, q=q) == BAD and "both at least 1" in _capi.last_error()
    for a in (0, -1, 33):
        assert call(a=a) == BAD and "bad alphabet length" in _capi.last_error()
    assert call(m=None) == BAD and "null multiple alignment" in _capi.last_error()
    for k in (0, 1, 2):
        assert call(missing=(k,)) == BAD and "null multiple alignment" in _capi.last_error()
    for members, q in ((2 ** 27 + 1, 1), (2 ** 26 + 1, 2), (1, 2 ** 27 + 1), (2 ** 20, 129), (2 ** 62, 3)):
        assert call(members=members, q=q) == BAD and "more than 2^27" in _capi.last_error(), (members, q)
    for entry in (25, 31, 100, 254):
        wrong = msa.copy()
        wrong[1, 2] = entry
        assert call(m=wrong) == BAD and f"entry {entry} at 6 is neither a letter" in _capi.last_error()
    # (the gap letter follows the alphabet: 24 is no entry of a 20-letter one)
    assert call(a=20) == BAD and "entry 24 at 1" in _capi.last_error()
    assert out.untouched()


@pytest.fixture
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture
def database():
    return pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])


def test_python_validation_is_that_of_align_pairs(aligner, database):
    call = aligner.profile_columns
    with pytest.raises(Exception) as want:
        aligner.align_pairs(["MKV"], database, [(0, 1)], algorithm="blast")
    with pytest.raises(type(want.value)) as got:
        call("MKV", database, [1], algorithm="blast")
    assert str(got.value) == str(want.value)
    with pytest.raises(TypeError, match="expected BaseDatabase"):
        call("MKV", ["MKV"], [0])
    with pytest.raises(ValueError, match="different alphabets"):
        call("MKV", pyopal_amd.Database(["ACGT"], alphabet="ACGT"), [0])
    with pytest.raises(ValueError, match="database and PSSM have different alphabets"):
        call(pyopal_amd.Pssm.from_sequence("MKV"), pyopal_amd.Database(["ACGT"], alphabet="ACGT"), [0])
    with pytest.raises(TypeError, match="must not be None"):
        call(None, database, [0])
    for targets in ([[0, 1]], [0.5], ["1"]):
        with pytest.raises(ValueError, match="targets must be a sequence of integer target indices"):
            call("MKV", database, targets)
    for targets in ([3], [-1], [0, 1, 7]):
        with pytest.raises(IndexError, match="target index outside the database"):
            call("MKV", database, targets)
    # the order of `align_pairs`: the algorithm before the database
    with pytest.raises(ValueError, match="invalid algorithm"):
        call("MKV", ["MKV"], [0], algorithm="blast")
    for rounds, error in ((0, ValueError), (-1, ValueError), (1.5, TypeError), (True, TypeError)):
        with pytest.raises(error, match="rounds must be"):
            aligner.iterated_search("MKV", database, 1e-3, rounds=rounds)


def test_empty_targets_need_no_device(aligner, database, monkeypatch):
    pssm = pyopal_amd.Pssm(np.ones((5, 24), dtype=np.int32), consensus=[10, 255, 19, 10, 0])
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    for query, codes in (("MKVLA", np.frombuffer(database.alphabet.encode("MKVLA"), dtype=np.uint8)), (pssm, pssm.consensus),
                         ("", np.zeros(0, dtype=np.uint8))):
        for targets in ([], np.zeros(0, dtype=np.int64)):
            for return_msa in (False, True):
                got = aligner.profile_columns(query, database, targets, return_msa=return_msa)
                msa = np.where(codes < 24, codes, 255).astype(np.uint8)[None, :]
                counts, k, terms, weights, weighted = _profile.columns(msa, 24)
                assert got.counts.dtype == np.int64 and got.counts.shape == (len(codes), 25)
                assert np.array_equal(got.counts, counts) and np.array_equal(got.weighted, weighted)
                assert got.member_weights.tolist() == weights.tolist() == [int((codes < 24).sum()) * 2 ** 32]
                assert np.array_equal(got.distinct, k) and np.array_equal(got.consensus, codes)
                assert got.alphabet == database.alphabet
                assert (got.msa is None) if not return_msa else np.array_equal(got.msa, msa)


def test_reference_agrees_with_its_plain_witness():
    rng = np.random.default_rng(5)
    for members, Q, A in ((1, 1, 24), (7, 9, 4), (40, 13, 32), (3, 5, 1)):
        msa = rng.choice(np.concatenate([np.arange(A + 1), [255, 255]]), size=(members, Q)).astype(np.uint8)
        for fast, plain in zip(_profile.columns(msa, A), _profile.columns_plain(msa, A)):
            assert fast.dtype == plain.dtype and np.array_equal(fast, plain), (members, Q, A)
    ops = [2, 0, 3, 1, 1, 2, 0]
    row = _profile.project(ops, 2, 5, np.arange(100, 120), 9, 24)
    assert row.tolist() == [255, 255, 106, 107, 24, 24, 109, 255, 255]
    assert _profile.project([], -1, -1, np.zeros(0, np.uint8), 3, 24).tolist() == [255] * 3


UNIFORM20 = np.array([1.0 / 20] * 20 + [0.0] * 4)   # the 20 standard letters of the matrices' 24 (ARNDCQEGHILKMFPSTWYV BZX*)


def test_matrix_lambda_solves_its_equation():
    S = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.float64).reshape(24, 24)
    lam = pyopal_amd.matrix_lambda("BLOSUM62", UNIFORM20)
    assert 0.2 < lam < 0.5
    total = sum(UNIFORM20[a] * UNIFORM20[b] * np.exp(lam * S[a, b]) for a in range(24) for b in range(24))
    assert abs(total - 1.0) <= 1e-12
    assert pyopal_amd.matrix_lambda(ScoringMatrix.from_name("BLOSUM62"), UNIFORM20 * 7) == lam   # (normalised here)
    identity = ScoringMatrix.from_match_mismatch(1.0, -1.0)
    n = len(identity.alphabet)
    with pytest.raises(ValueError, match="not negative"):
        pyopal_amd.matrix_lambda(identity, np.eye(n)[0])   # one letter: every pair a match
    negative = ScoringMatrix([[-1.0] * 4] * 4, "ACGT")
    with pytest.raises(ValueError, match="no positive score"):
        pyopal_amd.matrix_lambda(negative, [0.25] * 4)
    with pytest.raises(ValueError, match="background must hold 24"):
        pyopal_amd.matrix_lambda("BLOSUM62", [0.25] * 4)


def hand_columns(msa, codes):
    counts, k, terms, weights, weighted = _profile.columns(np.asarray(msa, dtype=np.uint8), 24)
    return pyopal_amd.ProfileColumns(counts, weighted, weights, pyopal_amd.Alphabet(), codes, msa)


def test_from_columns_is_the_formula():
    """Pssm.from_columns against the formula written out again, entry by entry in Python floats, on hand-made columns: a
    column with only the query, one with all members on one letter, one with an empty weighted row (no residue in the
    consensus, nobody else covers it), mixed columns, and four letters of frequency 0. Exact, except that an entry
    whose unrounded value lies within 1e-9 of a half-integer may differ by 1."""
    import math
    codes = np.array([10, 3, 255, 7, 0, 19], dtype=np.uint8)
    msa = np.array([[10, 3, 255, 7, 0, 19],
                    [255, 3, 255, 8, 24, 1],
                    [255, 3, 255, 7, 2, 22],     # 22: a letter of frequency 0 in a column
                    [255, 3, 255, 24, 2, 255],
                    [255, 3, 255, 9, 255, 5]], dtype=np.uint8)
    columns = hand_columns(msa, codes)
    assert columns.distinct.tolist() == [1, 1, 0, 3, 2, 4]
    assert columns.weighted[2].sum() == 0 and columns.frequencies()[2].tolist() == [0.0] * 24
    assert np.allclose(columns.frequencies()[[0, 1, 3, 4, 5]].sum(axis=1), 1.0)
    prior_scores = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32).reshape(24, 24)[[10, 3, 4, 7, 0, 19]]
    prior = pyopal_amd.Pssm(prior_scores, consensus=codes)
    p = UNIFORM20 * np.linspace(0.5, 1.5, 24)
    p = p / p.sum()
    lam = pyopal_amd.matrix_lambda("BLOSUM62", p)
    for beta in (10.0, 0.25):
        got = pyopal_amd.Pssm.from_columns(columns, prior, p, lam, pseudocount=beta)
        assert got.scores.dtype == np.int32 and got.scores.shape == (6, 24)
        assert np.array_equal(got.consensus, codes) and got.alphabet == prior.alphabet
        f = columns.frequencies()
        for i in range(6):
            alpha = max(int(columns.distinct[i]) - 1, 0)
            g = [p[a] * math.exp(lam * int(prior_scores[i, a])) if p[a] > 0 else 0.0 for a in range(24)]
            total = math.fsum(g)
            for a in range(24):
                if p[a] == 0 or columns.weighted[i, :24].sum() == 0:
                    assert got.scores[i, a] == prior_scores[i, a], (i, a)
                    continue
                q = (alpha * f[i, a] + beta * g[a] / total) / (alpha + beta)
                raw = math.log(q / p[a]) / lam
                want = min(max(round(raw), -(2 ** 15)), 2 ** 15 - 1)
                near_half = abs(abs(raw - math.floor(raw)) - 0.5) <= 1e-9
                assert abs(int(got.scores[i, a]) - want) <= (1 if near_half else 0), (beta, i, a, raw)
    # a column only the query covers keeps its prior row up to the normalisation of g: one shift for the whole row
    shift = got.scores[0, :20].astype(int) - prior_scores[0, :20]
    assert shift.max() - shift.min() <= 1
    with pytest.raises(ValueError, match="differ in length or alphabet"):
        pyopal_amd.Pssm.from_columns(columns, pyopal_amd.Pssm(prior_scores[:5]), p, lam)
    with pytest.raises(ValueError, match="pseudocount must be finite and positive"):
        pyopal_amd.Pssm.from_columns(columns, prior, p, lam, pseudocount=0.0)
    with pytest.raises(TypeError, match="expected ProfileColumns"):
        pyopal_amd.Pssm.from_columns(None, prior, p, lam)


def test_well_formed_calls_fail_loudly_without_a_device(aligner, database):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        aligner.profile_columns("MKV", database, [0, 2])
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        aligner.profile_columns(pyopal_amd.Pssm.from_sequence("MKV", "BLOSUM50"), database, [1])
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        aligner.iterated_search("MKV", database, 1e-3)
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.profile_columns_rows(np.zeros((2, 8), dtype=np.uint8), 24)
