"""Where every occurrence of a whole panel of position-specific scoring matrices starts, and its alignment, in one
call (miopalSearchPssmBatchOccurrencesAligned; DeviceDatabase.search_batch_occurrence_alignments_pssm;
pyopal_amd.find_occurrence_alignments_pssm_many). Witnesses, none of them the code under test: the plain aligned panel
where the rows are a matrix's and the consensus the query; the unchanged search_occurrence_alignments_pssm of one PSSM
at a time; and, because that witness shares the later passes with the new path, `starts` of
tests/_occurrence_alignments.py directly."""
import ctypes
import functools

import numpy as np
import pytest

import _occurrence_alignments
import _pssm
import pyopal_amd
from test_gpu_batch_occurrence_alignments import (ALL, BAD, FIVE, ON_PANEL, STARTS, TOO_MANY, assert_csr, panel_set, rule_of)
from test_gpu_batch_occurrences import NOWHERE, PANEL
from test_gpu_occurrences import GAPS, MATRICES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def panel_dbs(capi):
    dbs = {}
    for name, (matrix, alphabet) in MATRICES.items():
        residues, offsets, _, _, _ = panel_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, alphabet)
    yield dbs
    for db in dbs.values():
        db.close()


def singles(db, panel, consensus, gaps, algorithm, cuts, windows, start=0, end=None, operations=True, routing=None):
    """search_occurrence_alignments_pssm PSSM by PSSM, laid end to end as the CSR; ``routing``: a list that receives
    what miopalLastOccurrenceAlignRouting reports behind every call"""
    parts = []
    for rows, cons, c, w in zip(panel, consensus, cuts, windows):
        parts.append(db.search_occurrence_alignments_pssm(rows, cons, gaps[0], gaps[1], algorithm, start, end, min_score=int(c),
                                                          window=w, operations=operations))
        if routing is not None:
            routing.append(db.last_occurrence_align_routing())
    out = {"offsets": np.concatenate([[0], np.cumsum([p["count"] for p in parts])]).astype(np.int64)}
    for key in FIVE + STARTS + (("aln_flat",) if operations else ()):
        dtype = np.int64 if key == "target" else np.uint8 if key == "aln_flat" else np.int32
        out[key] = np.concatenate([p[key] for p in parts]) if parts else np.zeros(0, dtype=dtype)
    if operations:
        lengths = np.concatenate([np.diff(p["aln_off"]) for p in parts]) if parts else np.zeros(0, dtype=np.int64)
        out["aln_off"] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return out


# ---- 1: rows of the matrix, the query as consensus: the plain aligned panel -----------------------------------------

@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gaps", GAPS)
def test_rows_of_the_matrix_equal_the_plain_aligned_panel(panel_dbs, gaps, name):
    matrix, alphabet = MATRICES[name]
    _, _, _, _, panel = panel_set(name)
    rows = [np.ascontiguousarray(matrix.reshape(alphabet, alphabet)[q]) for q in panel]
    db = panel_dbs[name]
    rng = np.random.default_rng(gaps[0] * 10 + gaps[1])
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(panel, algorithm, rng)
        context = (name, gaps, algorithm)
        want = db.search_batch_occurrence_alignments(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        plain = db.last_batch_occurrence_routing(), db.last_batch_occurrence_align_routing()
        got = db.search_batch_occurrence_alignments_pssm(rows, panel, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        assert_csr(got, want, context)
        assert want["offsets"][-1] > 100 and len(want["aln_flat"]) > 1000
        sweeps, stage = db.last_batch_occurrence_routing(), db.last_batch_occurrence_align_routing()
        assert sweeps == plain[0] and sweeps[:3] == [8, 2, 1], (context, sweeps, plain)
        # every occurrence aligned, the same longest window; how many lanes and wavefronts is the stage's own affair
        assert stage[0] + stage[1] == plain[1][0] + plain[1][1] == want["offsets"][-1] and stage[3] == plain[1][3], (context, stage, plain)


# ---- 2: rows of their own, a consensus that is not their argmax ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def own_panel(name):
    """PANEL's heights with `class_pssm` rows, and per PSSM a consensus drawn at random - not the rows' best letter -
    with 255 (no residue: never a match) at some positions"""
    alphabet = MATRICES[name][1]
    rng = np.random.default_rng(900 + alphabet)
    rows = [_pssm.class_pssm(rng, q, alphabet)[2] for q in PANEL]
    consensus = []
    for r in rows:
        c = rng.integers(0, alphabet, size=len(r)).astype(np.uint8)
        c[rng.random(len(r)) < 0.2] = 255
        consensus.append(c)
    assert any(np.any((c != r.argmax(axis=1)) & (c != 255)) for r, c in zip(rows, consensus) if len(r))
    assert sum(int(np.count_nonzero(c == 255)) for c in consensus) > 10
    return rows, consensus


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gaps", GAPS[:2])
def test_rows_of_their_own_equal_the_singles_and_the_helper(panel_dbs, gaps, name):
    _, _, targets, _, _ = panel_set(name)
    rows, consensus = own_panel(name)
    db = panel_dbs[name]
    rng = np.random.default_rng(gaps[0] * 10 + gaps[1] + 2)
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(rows, algorithm, rng)
        if algorithm == "sw":
            cuts = [c + 8 for c in cuts]
            cuts[NOWHERE] = 10 ** 6
        context = (name, gaps, algorithm)
        got = db.search_batch_occurrence_alignments_pssm(rows, consensus, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        sweeps, stage = db.last_batch_occurrence_routing(), db.last_batch_occurrence_align_routing()
        want = singles(db, rows, consensus, gaps, algorithm, cuts, windows)
        assert_csr(got, want, context)
        counts = np.diff(got["offsets"])
        assert counts[NOWHERE] == 0 and counts[NOWHERE - 1] > 0 and counts[NOWHERE + 1] > 0, (context, counts)
        assert counts[PANEL.index(130)] > 0 and counts[PANEL.index(65)] > 0 and counts[PANEL.index(0)] == 0, (context, counts)
        assert sweeps[:3] == [8, 2, 1] and stage[0] + stage[1] == got["offsets"][-1], (context, sweeps, stage)
        # the ends are the plain PSSM panel's, byte for byte
        ends = db.search_batch_occurrences_pssm(rows, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        for key in ("offsets",) + FIVE:
            assert got[key].tobytes() == ends[key].tobytes(), (context, key)
        # the starts against the helper, PSSM by PSSM (one numpy lane per occurrence: those that end in similar columns together)
        for i in ON_PANEL + [PANEL.index(65)]:
            lo, hi = int(got["offsets"][i]), int(got["offsets"][i + 1])
            bucket = got["end_t"][lo:hi] // 32
            for b in np.unique(bucket).tolist():
                at = lo + np.flatnonzero(bucket == b)
                occurrences = np.stack([got[key][at] for key in FIVE], axis=1)
                start_t, start_q = _occurrence_alignments.starts(rows[i], targets, occurrences, gaps[0], gaps[1], algorithm)
                assert np.array_equal(got["start_t"][at], start_t) and np.array_equal(got["start_q"][at], start_q), (context, i, b)
        # starts only: the same starts, no operation arrays
        only = db.search_batch_occurrence_alignments_pssm(rows, None, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows,
                                                          operations=False)
        assert_csr(only, want, (context, "starts only"), operations=False)
        assert db.last_batch_occurrence_align_routing()[:2] == [0, 0]


# ---- 3: the runs of the stage ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("free", ((), (3,), (7,), (6, 7), (0, 11)))
def test_runs_of_the_stage(capi, tuning, free):
    """12 PSSMs of 64 rows at 32 letters: 768 rows, above the 493 the table of the lane-per-pair later passes holds -
    two runs, PSSMs 0 .. 6 (448 rows) and 7 .. 11. ``free``: PSSMs whose cut nothing reaches - one in the middle of a
    run (3), one where the second run would begin (7: the run begins at 8), the last of a run and the first of the next
    (6, 7), both ends of the chunk (0, 11).
    The routing: on this few occurrences the cost estimates hand every chunk to the wavefront-per-pair kernels, in the
    singles as in the panel, so the claim - no occurrence leaves the lane-per-pair kernels because the chunk is large -
    is checked with MIOPAL_FORCE_LANE_PER_PAIR, which takes the estimates out and leaves what the table allows. The
    premise is checked here: every single call then reports no wavefront-per-pair occurrence."""
    alphabet = 32
    rng = np.random.default_rng(77)
    lengths = rng.integers(1, 61, size=130)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    rows = [_pssm.class_pssm(rng, 64, alphabet)[2] for _ in range(12)]
    consensus = [rng.integers(0, alphabet, size=64).astype(np.uint8) for _ in rows]
    assert sum(len(r) for r in rows) == 768 and (768 + 1) * (alphabet + 1) * 4 + 256 > 64 * 1024 >= (448 + 1) * (alphabet + 1) * 4 + 256
    db = capi.DeviceDatabase(residues, offsets, alphabet)
    try:
        for algorithm, cut in (("hw", -60), ("sw", 30)):
            cuts = [10 ** 6 if i in free else cut for i in range(12)]
            windows = [None] * 12
            for forced in (False, True):
                if forced:
                    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")
                context = (algorithm, free, forced)
                routing = []
                want = singles(db, rows, consensus, (3, 1), algorithm, cuts, windows, routing=routing)
                counts = np.diff(want["offsets"])
                assert all((counts[i] == 0) == (i in free) for i in range(12)), (context, counts)
                got = db.search_batch_occurrence_alignments_pssm(rows, consensus, 3, 1, algorithm, min_score=cuts, window=windows)
                stage = db.last_batch_occurrence_align_routing()
                assert_csr(got, want, context)
                assert db.last_batch_occurrence_routing()[:3] == [12, 0, 1], context
                assert stage[0] + stage[1] == want["offsets"][-1], (context, stage)
                # one sub-chunk per run that has occurrences (a run is far below a sub-chunk's capacity here)
                assert stage[2] == 2, (context, stage)
                if forced:
                    assert all(r[1] == 0 for r in routing), (context, routing)      # the premise
                    assert stage[1] == 0 and stage[0] == want["offsets"][-1], (context, stage)
                    tuning.delenv("MIOPAL_FORCE_LANE_PER_PAIR")
    finally:
        db.close()


# ---- 4: the contract of the aligned form ----------------------------------------------------------------------------

def test_contract(capi, tuning, panel_dbs):
    name = "random32"
    alphabet = MATRICES[name][1]
    _, _, _, lengths, _ = panel_set(name)
    rows, consensus = own_panel(name)
    db = panel_dbs[name]
    gaps = (3, 1)
    cuts, windows = rule_of(rows, "hw", np.random.default_rng(6))
    rule = dict(min_score=cuts, window=windows)
    whole = db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", **rule)
    counts = np.diff(whole["offsets"])
    total = int(whole["offsets"][-1])
    again = db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", **rule)
    for key in ("offsets",) + ALL:
        assert again[key].tobytes() == whole[key].tobytes(), key
    start, end = 37, 101
    part = db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", start, end, **rule)
    assert_csr(part, singles(db, rows, consensus, gaps, "hw", cuts, windows, start, end), "slice")
    assert part["offsets"][-1] > 0 and part["target"].min() >= start and part["target"].max() < end
    nothing = np.zeros((0, alphabet), dtype=np.int32)
    none = np.zeros(0, dtype=np.uint8)
    for got, n in ((db.search_batch_occurrence_alignments_pssm([], [], *gaps, "hw"), 0),
                   (db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", 40, 40, **rule), len(rows)),
                   (db.search_batch_occurrence_alignments_pssm([nothing, nothing], [none, none], *gaps, "hw", min_score=0), 2)):
        assert got["offsets"].tolist() == [0] * (n + 1) and got["aln_off"].tolist() == [0]
        assert all(len(got[key]) == 0 for key in FIVE + STARTS + ("aln_flat",))
        assert db.last_batch_occurrence_align_routing() == [0, 0, 0, 0]

    lib = capi.lib()
    flat = np.ascontiguousarray(np.concatenate(rows))
    cons = np.ascontiguousarray(np.concatenate(consensus))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    w = np.ascontiguousarray([(len(r) if x is None else x) for r, x in zip(rows, windows)], dtype=np.int32)
    s = np.ascontiguousarray(cuts, dtype=np.int32)

    def call(max_hits=-1, missing=(), mode=1, consensus=cons):
        hit_offsets = np.full(len(rows) + 1, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(8)]
        refs = [None if i in missing else ctypes.byref(p) for i, p in enumerate(ptrs)]
        rc = lib.miopalSearchPssmBatchOccurrencesAligned(db.handle, flat.ctypes.data, None if consensus is None else consensus.ctypes.data,
                                                         off.ctypes.data, len(rows), *gaps, alphabet, mode, 0, len(lengths),
                                                         s.ctypes.data, w.ctypes.data, max_hits, hit_offsets.ctypes.data, *refs)
        return rc, hit_offsets, all(p.value == 0x77 for p in ptrs)

    for kw, text in ((dict(missing=(6,)), "both, or neither"), (dict(missing=(4,)), "null start-location"),
                     (dict(consensus=None), "null consensus for an alignment search")):
        rc, hit_offsets, untouched = call(**kw)
        assert rc == BAD and text in capi.last_error(), (kw, rc, capi.last_error())
        assert np.all(hit_offsets == -7) and untouched, kw
    # maxHits below the total: in one chunk, and in three where the bound is passed in the last one - what the chunks
    # before it aligned is discarded, hitOffsets is filled, every pointer is as it was
    on_panel = [int(counts[i]) for i in ON_PANEL]
    for entries, chunks in ((None, 1), (3 * len(lengths), 3)):
        if entries:
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", str(entries))
        bound = total - 1
        if chunks == 3:
            assert sum(on_panel[6:]) > 0 and bound - (total - sum(on_panel)) >= sum(on_panel[:6])
        rc, hit_offsets, untouched = call(max_hits=bound)
        assert rc == TOO_MANY and "maxHits" in capi.last_error(), (chunks, rc)
        assert np.array_equal(hit_offsets, whole["offsets"]) and untouched, chunks
        assert db.last_batch_occurrence_routing()[2] == chunks
        with pytest.raises(capi.TooManyHits) as info:
            db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", max_hits=bound, **rule)
        assert np.array_equal(info.value.counts, whole["offsets"])
        bounded = db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", max_hits=total, **rule)
        assert_csr(bounded, whole, ("max_hits = total", chunks))
        if entries:
            tuning.delenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES")
    assert_csr(db.search_batch_occurrence_alignments_pssm(rows, consensus, *gaps, "hw", **rule), whole, "afterwards")


# ---- 5: the free functions -------------------------------------------------------------------------------------------

def test_find_occurrence_alignments_pssm_many_equals_find_occurrences_pssm(capi):
    rng = np.random.default_rng(95)
    letters = "ACGT"
    text = lambda codes: "".join(letters[c] for c in codes)   # noqa: E731
    reads = [rng.integers(0, 4, size=int(n)) for n in rng.integers(0, 201, size=130)]
    aligner = pyopal_amd.Aligner(pyopal_amd.ScoringMatrix.from_match_mismatch(5, -4), gap_open=3, gap_extend=1)
    database = pyopal_amd.Database([text(r) for r in reads], pyopal_amd.Alphabet(letters))
    forward = [pyopal_amd.Pssm(rng.integers(-6, 7, size=(q, 4)), letters) for q in (6, 20, 11, 0, 64, 70)]
    pssms = [p for f in forward for p in (f, f.reverse_complement())]
    fields = lambda r: (type(r), r.target_index, r.score, r.target_end, r.query_end, r.target_start, r.query_start,   # noqa: E731
                        r.query_length, r.target_length, r.alignment, r.cigar())
    for algorithm, cut in (("hw", 8), ("sw", 14)):
        cuts = [cut + k for k in range(len(pssms))]
        windows = [None if k % 2 else k for k in range(len(pssms))]
        found = pyopal_amd.find_occurrence_alignments_pssm_many(aligner, pssms, database, cuts, algorithm=algorithm, window=windows)
        assert len(found) == len(pssms) and sum(len(f) for f in found) > 100
        for i, (pssm, mine) in enumerate(zip(pssms, found)):
            alone = pyopal_amd.find_occurrences_pssm(aligner, pssm, database, cuts[i], algorithm=algorithm, window=windows[i], mode="full")
            assert [fields(r) for r in mine] == [fields(r) for r in alone], (algorithm, i)
            assert all(isinstance(r, pyopal_amd.FullResult) for r in mine)
        arrays = pyopal_amd.find_occurrence_alignments_pssm_many_arrays(aligner, pssms, database, cuts, algorithm=algorithm, window=windows)
        assert sorted(arrays) == ["aln_flat", "aln_off", "end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]
        flat = [r for mine in found for r in mine]
        for key, name in (("target", "target_index"), ("score", "score"), ("end_t", "target_end"), ("end_q", "query_end"),
                          ("start_t", "target_start"), ("start_q", "query_start")):
            assert arrays[key].tolist() == [getattr(r, name) for r in flat], (algorithm, key)
        assert "".join("MDIX"[o] for o in arrays["aln_flat"].tolist()) == "".join(r.alignment for r in flat)
        part = pyopal_amd.find_occurrence_alignments_pssm_many_arrays(aligner, pssms, database, cuts, algorithm=algorithm,
                                                                      window=windows, start=20, end=90, operations=False)
        assert sorted(part) == ["end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]
        assert part["offsets"][-1] > 0 and part["target"].min() >= 20 and part["target"].max() < 90
