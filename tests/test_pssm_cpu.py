"""CPU tier of the PSSM search (miopalSearchPssm, DeviceDatabase.search_pssm, pyopal_amd.Pssm, Aligner.align_pssm):
the C ABI is declared, listed and exported; argument errors are reported before a device is needed; the Python
types validate, compare and pickle; an empty slice is answered without a device; and the two things the GPU tier
leans on - the class identity of tests/_pssm.py and its numpy DP - are pinned against the CPU checker here."""
import ctypes
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import _data
import _oracle
import _pssm
import pyopal_amd
from pyopal_amd import Pssm, _capi
from pyopal_amd.matrices import ScoringMatrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "miopal.h")
BLOSUM62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)


def test_header_declares_the_entry_point():
    text = open(HEADER).read()
    m = re.search(r"\bint\s+miopalSearchPssm\s*\(([^)]*)\)", text)
    assert m, "miopalSearchPssm is not declared"
    args = re.sub(r"\s+", " ", m.group(1))
    assert args.startswith("MiopalDb* db, const int* rowScores, const unsigned char* consensus, int queryLength,")
    assert args.endswith("unsigned char** operations, int64_t* operationOffsets")
    assert "miopalSearchPssm" in _capi.EXPORTS
    assert hasattr(_capi.DeviceDatabase, "search_pssm")


def test_library_exports_the_entry_point():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libmiopal.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "miopalSearchPssm" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_c_call_reports_argument_errors_before_a_device():
    """Every check of miopalSearchPssm that needs no handle comes before the handle is looked at (here: no handle at
    all), let alone a device; the handle's own checks (alphabet, slice, 32-bit range) are in the GPU tier."""
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libmiopal.so not built")
    lib = _capi.lib()
    rows = np.ones((4, 32), dtype=np.int32)
    cons = np.array([0, 31, 255, 5], dtype=np.uint8)
    score = np.full(2, 77, dtype=np.int32)
    ends = np.full((4, 2), 77, dtype=np.int32)
    aoff = np.full(3, 77, dtype=np.int64)
    ops = ctypes.c_void_p()

    def call(r=rows, c=cons, q=4, alphabet=32, st=2, mode=3):
        return lib.miopalSearchPssm(None, None if r is None else r.ctypes.data, None if c is None else c.ctypes.data, q,
                                    3, 1, alphabet, st, mode, 0, 2, score.ctypes.data, ends[0].ctypes.data,
                                    ends[1].ctypes.data, ends[2].ctypes.data, ends[3].ctypes.data, ctypes.byref(ops),
                                    aoff.ctypes.data)

    assert call(mode=4) == _capi.OPAL_ERR_INVALID_MODE and "alignment mode" in _capi.last_error()
    assert call(mode=-1) == _capi.OPAL_ERR_INVALID_MODE
    assert call(st=3) == _capi.OPAL_ERR_INVALID_MODE and "search type" in _capi.last_error()
    assert call(q=-1) == 101 and "query length" in _capi.last_error()             # MIOPAL_ERR_BAD_ARGUMENT
    assert call(r=None) == 101 and "null row scores" in _capi.last_error()
    assert call(alphabet=0) == 101 and "alphabet length" in _capi.last_error()
    assert call(alphabet=33) == 101 and "alphabet length" in _capi.last_error()
    assert call(c=None) == 101 and "null consensus" in _capi.last_error()
    bad = cons.copy()
    bad[1] = 32
    assert call(c=bad) == 101 and "consensus residue 32" in _capi.last_error() and "at 1" in _capi.last_error()
    bad[1] = 254
    assert call(c=bad) == 101 and "consensus residue 254" in _capi.last_error()
    # nothing wrong with the PSSM: the handle is what is missing (score and end searches need no consensus)
    assert call() == 101 and "null database handle" in _capi.last_error()
    assert call(c=None, st=0) == 101 and "null database handle" in _capi.last_error()
    assert call(c=None, st=1) == 101 and "null database handle" in _capi.last_error()
    assert call(r=None, c=None, q=0, st=0) == 101 and "null database handle" in _capi.last_error()
    # nothing was written on any of these errors
    assert np.all(score == 77) and np.all(ends == 77) and np.all(aoff == 77) and not ops.value


def test_a_well_formed_search_fails_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    pssm = Pssm.from_sequence("MKVLA")
    db = pyopal_amd.Database(["MKVLA", "AAAA"])
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        pyopal_amd.Aligner().align_pssm(pssm, db)
    with pytest.raises(RuntimeError, match="no supported SIMD backend"):
        _capi.DeviceDatabase(np.zeros(4, dtype=np.uint8), np.array([0, 4], dtype=np.int64), 24).search_pssm(pssm.scores)


def test_pssm_construction():
    scores = np.arange(3 * 24).reshape(3, 24) % 7
    p = Pssm(scores)
    assert len(p) == 3 and p.alphabet == pyopal_amd.Alphabet() and p.scores.dtype == np.int32
    assert p.scores.flags.c_contiguous and not p.scores.flags.writeable and np.array_equal(p.scores, scores)
    assert p.scores is not scores and p.consensus.dtype == np.uint8
    # the default consensus: each row's best-scoring letter, the lowest index on ties
    assert p.consensus.tolist() == [int(np.argmax(r)) for r in scores] == [6, 3, 0]
    tied = np.zeros((2, 24), dtype=np.int64)
    tied[1, [5, 9]] = 4
    assert Pssm(tied).consensus.tolist() == [0, 5]
    # a transposed view is made contiguous; floats that are whole numbers are accepted, others are not
    assert np.array_equal(Pssm(np.asfortranarray(scores)).scores, scores) and Pssm(scores.astype(float)) == p
    with pytest.raises(ValueError):
        Pssm(scores + 0.5)
    # explicit consensus: text over the alphabet, or codes with 255 for "no residue"
    assert Pssm(scores, consensus="ARN").consensus.tolist() == [0, 1, 2]
    q = Pssm(scores, consensus=[0, 255, 23])
    assert q.consensus.tolist() == [0, 255, 23] and q.consensus_sequence == "A-*" and q != p
    assert Pssm(np.zeros((0, 24), dtype=np.int32)).consensus.tolist() == [] and len(Pssm(np.zeros((0, 24)))) == 0
    dna = Pssm(np.eye(4, dtype=np.int32), "ACGT")
    assert dna.alphabet == pyopal_amd.Alphabet("ACGT") and dna.consensus_sequence == "ACGT"
    assert Pssm(np.eye(4, dtype=np.int32), pyopal_amd.Alphabet("ACGT")) == dna
    for bad in (lambda: Pssm(np.zeros((3, 23))),                       # a row is not the alphabet's length
                lambda: Pssm(np.zeros(24)),                            # not two-dimensional
                lambda: Pssm(np.zeros((3, 4)), "ACGT", consensus="AC"),      # consensus of the wrong length
                lambda: Pssm(np.zeros((2, 4)), "ACGT", consensus=[0, 4]),    # ... with a residue outside the alphabet
                lambda: Pssm(np.zeros((2, 4)), "ACGT", consensus=[0, -1]),
                lambda: Pssm(np.zeros((2, 4)), "ACGT", consensus="A1"),
                lambda: Pssm(np.zeros((2, 4)), "ACGT", consensus=[0.5, 1.0]),
                lambda: Pssm([["a"] * 4], "ACGT")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(OverflowError):
        Pssm(np.full((1, 4), 2 ** 31, dtype=np.int64), "ACGT")
    with pytest.raises(TypeError):
        Pssm(np.zeros((1, 4)), alphabet=4)
    assert "Pssm" not in pyopal_amd.__all__ and pyopal_amd.lib.Pssm is Pssm


def test_pssm_from_sequence_and_pickling():
    p = Pssm.from_sequence(_data.README_QUERY)
    codes = _data.encode(_data.README_QUERY)
    assert len(p) == 53 and p.consensus.tolist() == codes.tolist() and p.consensus_sequence == _data.README_QUERY
    assert np.array_equal(p.scores, BLOSUM62.reshape(24, 24)[codes])
    assert Pssm.from_sequence("MKV", "BLOSUM50") != Pssm.from_sequence("MKV") == Pssm.from_sequence("MKV", ScoringMatrix.from_name("BLOSUM62"))
    assert Pssm.from_sequence("ACGT", ScoringMatrix.from_match_mismatch(5, -4)).scores.tolist()[0] == [5, -4, -4, -4]
    with pytest.raises(ValueError):
        Pssm.from_sequence("MK1")
    with pytest.raises(TypeError):
        Pssm.from_sequence("MKV", 62)
    again = pickle.loads(pickle.dumps(p))
    assert again == p and again.scores.dtype == np.int32 and not again.scores.flags.writeable
    odd = Pssm(np.arange(8).reshape(2, 4), "ACGT", consensus=[255, 2])
    assert pickle.loads(pickle.dumps(odd)) == odd and pickle.loads(pickle.dumps(odd)).consensus.tolist() == [255, 2]
    with pytest.raises(TypeError):
        hash(p)


def test_align_pssm_validates_and_answers_an_empty_slice_without_a_device(monkeypatch):
    aligner = pyopal_amd.Aligner()
    database = pyopal_amd.Database(["MKVLA", "AAAA", "WWW"])
    pssm = Pssm.from_sequence("MKV")
    with pytest.raises(TypeError):
        aligner.align_pssm("MKV", database)
    with pytest.raises(TypeError):
        aligner.align_pssm(pssm, ["MKVLA"])
    with pytest.raises(ValueError):
        aligner.align_pssm(pssm, database, mode="sorted")
    with pytest.raises(ValueError):
        aligner.align_pssm(pssm, database, algorithm="blast")
    with pytest.raises(ValueError, match="different alphabets"):
        aligner.align_pssm(pssm, pyopal_amd.Database(["ACGT"], alphabet="ACGT"))
    with pytest.raises(OverflowError):
        aligner.align_pssm(pssm, database, start=-1)
    with pytest.raises(IndexError):
        aligner.align_pssm(pssm, database, start=2, end=1)
    with pytest.raises(IndexError):
        aligner.align_pssm(pssm, database, start=4)
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    for mode in ("score", "end", "full"):
        assert aligner.align_pssm(pssm, database, mode=mode, start=1, end=1) == []
        assert aligner.align_pssm(pssm, pyopal_amd.Database([]), mode=mode) == []
        arrays = aligner.align_pssm_arrays(pssm, database, mode=mode, start=3)
        assert len(arrays) == 0 and arrays.query_length == 3 and arrays.start == 3 and arrays.score.dtype == np.int32
        assert (arrays.operation_offsets.tolist() == [0]) if mode == "full" else arrays.operation_offsets is None


def _merged(ops):
    """match and mismatch as one operation: what a relabelled query cannot change"""
    return [np.where(a == 3, 0, a).tolist() for a in ops]


@pytest.mark.parametrize("algorithm", ["nw", "hw", "ov", "sw"])
def test_class_identity_between_two_checker_runs(algorithm):
    """A plain query under BLOSUM62 against its class-expanded form: 32 classes, each standing for one of the 24
    residues (several for some), query[i] a class of the residue, matrix[c] that residue's row. The checker gives the
    same scores, locations and gaps for both; only match / mismatch follow the labels (position i "matches" residue t
    iff query[i] == t)."""
    rng = np.random.default_rng(5)
    residue_of = np.concatenate([rng.permutation(24), rng.integers(0, 24, size=8)]).astype(np.uint8)
    rng.shuffle(residue_of)
    table = np.zeros((32, 32), dtype=np.int32)
    table[:, :24] = BLOSUM62.reshape(24, 24)[residue_of]
    table[:, 24:] = rng.integers(-9, 9, size=(32, 8))     # (letters no target holds)
    query = _data.random_protein(rng, 70)
    classes = np.array([rng.choice(np.flatnonzero(residue_of == r)) for r in query], dtype=np.uint8)
    residues, offsets = _data.random_db(rng, rng.integers(0, 90, size=60))
    plain = _oracle.search(query, residues, offsets, BLOSUM62, 3, 1, "full", algorithm)
    expanded = _oracle.search(classes, residues, offsets, table.ravel(), 3, 1, "full", algorithm)
    for key in ("score", "end_t", "end_q", "start_t", "start_q"):
        assert np.array_equal(plain[key], expanded[key]), key
    assert _merged(plain["aln"]) == _merged(expanded["aln"])
    assert any(0 in a for a in plain["aln"])


@pytest.mark.parametrize("algorithm,gaps", [("sw", (3, 1)), ("nw", (3, 1)), ("sw", (11, 1)), ("nw", (2, 5))])
def test_numpy_dp_agrees_with_the_checker_on_a_derived_pssm(algorithm, gaps):
    rng = np.random.default_rng(9)
    query = _data.random_protein(rng, 45)
    lengths = rng.integers(1, 70, size=40)
    lengths[[0, 7]] = 0
    residues, offsets = _data.random_db(rng, lengths)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    rows = BLOSUM62.reshape(24, 24)[query]
    want = _oracle.search(query, residues, offsets, BLOSUM62, gaps[0], gaps[1], "score", algorithm)["score"]
    assert np.array_equal(_pssm.dp_scores(rows, targets, gaps[0], gaps[1], algorithm), want)
