"""CPU tier of the occurrence search of a panel of position-specific scoring matrices
(miopalSearchPssmBatchOccurrences, miopalSearchPssmBatchOccurrencesAligned;
DeviceDatabase.search_batch_occurrences_pssm / search_batch_occurrence_alignments_pssm;
pyopal_amd.find_occurrences_pssm_many and its three siblings; Pssm.reverse_complement): the two symbols are declared,
listed and exported; with no handle the calls report what is wrong with their arguments, in the order the header
states, with every output as it was; the Python layers refuse the rule's faults before they reach the library; an
empty panel is answered without a device; the reverse complement of a PSSM."""
import subprocess

import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import Pssm, _capi

from test_occurrences_cpu import BAD, INVALID, Outputs, prototype

NAMES = ("miopalSearchPssmBatchOccurrences", "miopalSearchPssmBatchOccurrencesAligned")
FORMS = ("find_occurrences_pssm_many", "find_occurrences_pssm_many_arrays", "find_occurrence_alignments_pssm_many",
         "find_occurrence_alignments_pssm_many_arrays")
HW, SW = 1, 3


def test_header_declares_and_the_library_exports_the_entry_points():
    head = "MiopalDb* db, const int* rowScores, "
    middle = ("const int64_t* rowOffsets, int nPssms, int gapOpen, int gapExt, int alphabetLength, int mode, int64_t start, "
              "int64_t end, const int* minScore, const int* window, int64_t maxHits, int64_t* hitOffsets, "
              "int64_t** targetIndex, int** score, int** endTarget, int** endQuery")
    assert prototype(NAMES[0]) == head + middle
    assert prototype(NAMES[1]) == (head + "const unsigned char* consensus, " + middle + ", int** startTarget, int** startQuery, "
                                   "unsigned char** alignments, int64_t** alignmentOffsets")
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= names
    for name in NAMES:
        assert name in _capi.EXPORTS
        assert getattr(_capi.lib(), name).argtypes is not None, name
    assert len(_capi.lib().miopalSearchPssmBatchOccurrences.argtypes) == 18
    assert len(_capi.lib().miopalSearchPssmBatchOccurrencesAligned.argtypes) == 23
    assert hasattr(_capi.DeviceDatabase, "search_batch_occurrences_pssm")
    assert hasattr(_capi.DeviceDatabase, "search_batch_occurrence_alignments_pssm")


@pytest.mark.parametrize("aligned", (False, True))
def test_no_handle_reports_the_arguments_in_order_with_the_outputs_as_they_were(aligned):
    lib = _capi.lib()
    A = 32
    rows = np.ones((12, A), dtype=np.int32)
    tall = np.ones((500, A), dtype=np.int32)
    offsets = np.array([0, 4, 4, 12], dtype=np.int64)
    consensus = np.zeros(500, dtype=np.uint8)
    cuts, windows = np.array([3, 3, 3], dtype=np.int32), np.array([2, 0, 2], dtype=np.int32)
    out = Outputs(8 if aligned else 4)

    def call(n=3, r=rows, off=offsets, A=A, mode=HW, cut=cuts, window=windows, cons=consensus, missing=(), hit=out.count):
        p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        common = (p(off), n, 3, 1, A, mode, 0, 2, p(cut), p(window), -1, p(hit))
        if aligned:
            return lib.miopalSearchPssmBatchOccurrencesAligned(None, p(r), p(cons), *common, *out.refs(missing))
        return lib.miopalSearchPssmBatchOccurrences(None, p(r), *common, *out.refs(missing))

    def refused(code, text, **kw):
        rc = call(**kw)
        assert rc == code and text in _capi.last_error(), (kw, rc, _capi.last_error())
        assert out.untouched(), kw

    # each call below has everything wrong that the calls after it have, and one thing more
    bad_offsets = np.array([0, 4, 2, 12], dtype=np.int64)
    negative, zero = np.array([2, -1, 2], dtype=np.int32), np.array([3, 0, 3], dtype=np.int32)
    big = np.array([0, 4, 4, 498], dtype=np.int64)   # PSSM 2: 494 rows, one more than 32 letters allow
    last = dict(r=tall, off=big)
    refused(INVALID, "invalid alignment mode 7", mode=7, n=-1)
    refused(INVALID, "OPAL_MODE_HW and OPAL_MODE_SW", mode=0, n=-1)
    refused(INVALID, "OPAL_MODE_HW and OPAL_MODE_SW", mode=2, n=-1)
    refused(BAD, "bad PSSM list", n=-1, A=0)
    refused(BAD, "bad PSSM list", off=None, A=0)
    refused(BAD, "bad row offsets at 1", off=bad_offsets, r=None, A=0)
    refused(BAD, "null row scores", r=None, A=0)
    refused(BAD, "bad alphabet length 0", A=0, window=negative)
    refused(BAD, "bad alphabet length 33", A=33, window=negative)
    refused(BAD, "negative window -1 at PSSM 1", window=negative, mode=SW, cut=zero)
    refused(BAD, "minScore = 0 at PSSM 1", mode=SW, cut=zero, missing=(0,))
    refused(BAD, "null minScore / window list", cut=None, missing=(0,))
    refused(BAD, "null minScore / window list", window=None, missing=(0,))
    refused(BAD, "null", missing=(2,), **last)
    refused(BAD, "null", hit=None, **last)
    if aligned:
        refused(BAD, "null start-location outputs", missing=(4,), cons=None, **last)
        refused(BAD, "both, or neither", missing=(6,), cons=None, **last)
        refused(BAD, "null consensus for an alignment search", cons=None, **last)
        wrong = consensus.copy()
        wrong[7] = 40
        refused(BAD, "consensus residue 40 out of range at 7", cons=wrong, **last)
        wrong[7] = 255
        refused(BAD, "PSSM 2 of the panel", cons=wrong, **last)
    refused(BAD, "PSSM 2 of the panel: a PSSM of 494 rows at 32 letters does not fit the occurrence sweep's LDS table", **last)
    assert "493 rows at most" in _capi.last_error()
    # 493 rows fit; at 24 letters 651 do and 652 do not: then the handle is what is missing
    refused(BAD, "null database handle", r=tall, off=np.array([0, 4, 4, 497], dtype=np.int64))
    wide = np.ones((660, 24), dtype=np.int32)
    wide_cons = np.zeros(660, dtype=np.uint8)
    refused(BAD, "PSSM 0 of the panel: a PSSM of 652 rows at 24 letters", r=wide, A=24, cons=wide_cons,
            off=np.array([0, 652, 652, 656], dtype=np.int64))
    refused(BAD, "null database handle", r=wide, A=24, cons=wide_cons, off=np.array([0, 651, 651, 655], dtype=np.int64))
    refused(BAD, "null database handle")
    refused(BAD, "null database handle", n=0)
    if aligned:   # starts only: no consensus is needed
        refused(BAD, "null database handle", cons=None, missing=(6, 7))


class _NoHandle(_capi.DeviceDatabase):
    """a DeviceDatabase that owns no handle: what its methods refuse before they call the library"""

    def __init__(self, alphabet_length=4):
        self._h, self.count, self.alphabet_length = None, 3, alphabet_length


@pytest.mark.parametrize("aligned", (False, True))
def test_device_database_refusals_come_before_any_device_call(monkeypatch, aligned):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))
    db = _NoHandle()
    panel = [np.ones((n, 4), dtype=np.int32) for n in (4, 0, 9, 70, 2)]
    consensus = [np.zeros(len(p), dtype=np.uint8) for p in panel]
    if aligned:
        call = lambda rows=panel, cons=consensus, **kw: db.search_batch_occurrence_alignments_pssm(rows, cons, 3, 1, **kw)   # noqa: E731
    else:
        call = lambda rows=panel, cons=None, **kw: db.search_batch_occurrences_pssm(rows, 3, 1, **kw)   # noqa: E731
    with pytest.raises(ValueError, match=r"every PSSM must have shape \(rows, 4\)"):
        call(rows=panel[:2] + [np.ones((3, 5), dtype=np.int32)], min_score=3)
    if aligned:
        with pytest.raises(ValueError, match="one entry per row of every PSSM"):
            call(cons=consensus[:4] + [np.zeros(3, dtype=np.uint8)], min_score=3)
    for algorithm in ("nw", "ov", "blast"):
        with pytest.raises(ValueError, match="'hw' and 'sw'"):
            call(algorithm=algorithm, min_score=3)
    with pytest.raises(ValueError, match="window must not be negative"):
        call(min_score=3, window=[0, None, 5, -1, 2])
    with pytest.raises(ValueError, match="at least 1"):
        call(algorithm="sw", min_score=[5, 5, 5, 0, 5])
    with pytest.raises(ValueError, match="one value or one per query"):
        call(min_score=[1, 2, 3])
    with pytest.raises(OverflowError):
        call(min_score=2 ** 31)
    # nothing wrong with these: the library is what they reach
    for kw in (dict(min_score=-(2 ** 31), window=0), dict(algorithm="sw", min_score=1),
               dict(min_score=[1, 2, 3, 4, 5], window=[None, 0, 5, None, 1])):
        with pytest.raises(AssertionError, match="device reached"):
            call(**kw)
    if aligned:
        with pytest.raises(AssertionError, match="device reached"):
            call(cons=None, operations=False, min_score=1)


DNA_LETTERS = "ACGT"


def dna_pssms(heights, seed=5):
    rng = np.random.default_rng(seed)
    return [Pssm(rng.integers(-5, 6, size=(q, 4)), DNA_LETTERS) for q in heights]


def test_find_pssm_many_faults_and_empty_requests(monkeypatch):
    for name in FORMS:
        assert getattr(pyopal_amd, name) is getattr(pyopal_amd.occurrences, name)
        assert name not in pyopal_amd.__all__ and not hasattr(pyopal_amd.Aligner, name)
    aligner = pyopal_amd.Aligner(pyopal_amd.ScoringMatrix.from_match_mismatch(5, -4), gap_open=3, gap_extend=1)
    database = pyopal_amd.Database(["ACGTACGT", "TTGACA", ""], pyopal_amd.Alphabet(DNA_LETTERS))
    panel = dna_pssms((4, 0, 3))
    monkeypatch.setattr(pyopal_amd.lib._Request, "mirror", lambda self: (_ for _ in ()).throw(AssertionError("device reached")))
    for name in FORMS:
        form = getattr(pyopal_amd, name)
        ends = "alignments" not in name
        if ends:
            with pytest.raises(ValueError, match="not available yet from find_occurrences_pssm_many.*find_occurrence_alignments_pssm_many"):
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
        with pytest.raises(TypeError, match="window must be an integer or None"):
            form(aligner, panel, database, 5, window="3")
        with pytest.raises(TypeError, match="expected Pssm, got str"):
            form(aligner, [panel[0], "ACGT"], database, 5)
        with pytest.raises(ValueError, match="one value or one per query"):
            form(aligner, panel, database, [5, 5])
        with pytest.raises(ValueError, match="max_hits must not be negative"):
            form(aligner, panel, database, 5, max_hits=-1)
        with pytest.raises(ValueError, match="different alphabets"):
            form(aligner, [Pssm(np.zeros((3, 24), dtype=np.int32))], database, 5)
        with pytest.raises(IndexError):
            form(aligner, panel, database, 5, start=2, end=1)
        with pytest.raises(AssertionError, match="device reached"):
            form(aligner, panel, database, 5)
    # an empty panel, an empty slice, a panel of empty PSSMs: answered without a device
    for name in (FORMS[0], FORMS[2]):
        form = getattr(pyopal_amd, name)
        assert form(aligner, [], database, 5) == []
        assert form(aligner, panel, database, 5, start=1, end=1) == [[], [], []]
        assert form(aligner, dna_pssms((0, 0)), database, 5) == [[], []]
    got = pyopal_amd.find_occurrences_pssm_many_arrays(aligner, panel, database, 5, start=2, end=2)
    assert sorted(got) == ["end_q", "end_t", "offsets", "score", "target"]
    assert got["offsets"].dtype == np.int64 and got["offsets"].tolist() == [0, 0, 0, 0]
    got = pyopal_amd.find_occurrence_alignments_pssm_many_arrays(aligner, panel, database, 5, start=2, end=2)
    assert sorted(got) == ["aln_flat", "aln_off", "end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]
    got = pyopal_amd.find_occurrence_alignments_pssm_many_arrays(aligner, panel, database, 5, start=2, end=2, operations=False)
    assert sorted(got) == ["end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]


# ---- Pssm.reverse_complement ----------------------------------------------------------------------------------------

def revcomp(text, pairs="ACGT", to="TGCA"):
    return text.translate(str.maketrans(pairs, to))[::-1]


def test_reverse_complement_is_an_involution_and_commutes_with_from_sequence():
    dna = pyopal_amd.ScoringMatrix.from_match_mismatch(5, -4)
    rng = np.random.default_rng(9)
    for q in (0, 1, 7, 20):
        scores = rng.integers(-9, 10, size=(q, 4))
        consensus = rng.choice([0, 1, 2, 3, 255], size=q)
        pssm = Pssm(scores, DNA_LETTERS, consensus)
        other = pssm.reverse_complement()
        assert other.alphabet == pssm.alphabet and len(other) == q
        assert other.scores.dtype == np.int32 and other.consensus.dtype == np.uint8
        # row i of the other strand is row Q - 1 - i, its column of a letter the column of the letter's complement
        for t, u in enumerate((3, 2, 1, 0)):
            assert np.array_equal(other.scores[:, u], pssm.scores[::-1, t])
        assert np.array_equal(other.consensus == 255, pssm.consensus[::-1] == 255)
        back = other.reverse_complement()
        assert np.array_equal(back.scores, pssm.scores) and np.array_equal(back.consensus, pssm.consensus)
    for text in ("A", "ACGTTGCAAC", "GATTACA", "TTTTCCCCAG"):
        a, b = Pssm.from_sequence(text, dna).reverse_complement(), Pssm.from_sequence(revcomp(text), dna)
        assert np.array_equal(a.scores, b.scores) and np.array_equal(a.consensus, b.consensus), text
        assert a.consensus_sequence == revcomp(text)


def test_reverse_complement_mappings():
    rng = np.random.default_rng(10)
    # U is mapped like T; every other letter stays where it is
    letters = "ACGTUN"
    pssm = Pssm(rng.integers(-9, 10, size=(6, 6)), letters, "ACGTUN")
    other = pssm.reverse_complement()
    assert other.consensus_sequence == "NAACGT"
    for letter, opposite in zip("ACGTUN", "TGCAAN"):
        assert np.array_equal(other.scores[:, letters.index(letter)], pssm.scores[::-1, letters.index(opposite)]), letter
    spelled = pssm.reverse_complement({"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "N": "N"})
    assert np.array_equal(spelled.scores, other.scores) and np.array_equal(spelled.consensus, other.consensus)
    rna = Pssm(rng.integers(-9, 10, size=(5, 4)), "ACGU", "ACGUU")
    assert rna.reverse_complement().consensus_sequence == "AACGU"
    assert np.array_equal(rna.reverse_complement().scores[:, 3], rna.scores[::-1, 0])
    # a mapping of one's own: letters it leaves out stay
    custom = Pssm(rng.integers(-9, 10, size=(4, 4)), "WXYZ", "WXYZ")
    swapped = custom.reverse_complement({"W": "X", "X": "W"})
    assert swapped.consensus_sequence == "ZYWX"
    assert np.array_equal(swapped.scores[:, 0], custom.scores[::-1, 1]) and np.array_equal(swapped.scores[:, 2], custom.scores[::-1, 2])
    with pytest.raises(ValueError, match="letters of the alphabet"):
        custom.reverse_complement({"W": "Q"})
    with pytest.raises(TypeError, match="mapping"):
        custom.reverse_complement("WX")
    with pytest.raises(ValueError, match="none of the pairs"):
        custom.reverse_complement()
    # the protein alphabet holds A, C, G and T beside its other letters: no default exchanges amino acids
    protein = Pssm(rng.integers(-9, 10, size=(3, 24)))
    with pytest.raises(ValueError, match="no nucleotide codes"):
        protein.reverse_complement()
    assert protein.reverse_complement({"A": "T", "T": "A"}).alphabet == protein.alphabet
