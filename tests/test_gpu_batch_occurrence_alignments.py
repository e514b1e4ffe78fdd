"""Where every occurrence of a whole panel of queries starts, and its alignment, in one call
(miopalSearchBatchOccurrencesAligned; DeviceDatabase.search_batch_occurrence_alignments;
pyopal_amd.find_occurrence_alignments_many). Two witnesses, neither of them the code under test: the unchanged
search_occurrence_alignments of one query at a time, which its own tests hold to the helper - and, because that
witness shares the later passes of the pair list with the new path, tests/_occurrence_alignments.py (`starts`,
`operations`) directly."""
import ctypes
import functools

import numpy as np
import pytest

import _cases
import _data
import _oracle
import _pssm
import pyopal_amd
from _case_witnesses import cut_of
from _occurrences import INT_MIN
from pyopal_amd.matrices import ScoringMatrix
from test_gpu_batch_occurrences import DNA, NOWHERE, PANEL, _flatten
from test_gpu_occurrence_alignments import assert_alignments
from test_gpu_occurrences import GAPS, MATRICES

pytestmark = pytest.mark.gpu

FIVE = ("target", "score", "end_t", "end_q")
STARTS = ("start_t", "start_q")
ALL = FIVE + STARTS + ("aln_off", "aln_flat")
TOO_MANY, BAD, OVERFLOW = 103, 101, 1
MATCH = 0
ON_PANEL = [i for i, q in enumerate(PANEL) if 1 <= q <= 64]      # the queries the panel kernels take: eight of eleven
CASES = _cases.cases()


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def singles(db, panel, matrix, gaps, algorithm, cuts, windows, start=0, end=None, operations=True):
    """the first witness: search_occurrence_alignments query by query, laid end to end as the CSR"""
    parts = [db.search_occurrence_alignments(q, matrix, gaps[0], gaps[1], algorithm, start, end, min_score=int(c), window=w,
                                             operations=operations)
             for q, c, w in zip(panel, cuts, windows)]
    out = {"offsets": np.concatenate([[0], np.cumsum([p["count"] for p in parts])]).astype(np.int64)}
    for key in FIVE + STARTS + (("aln_flat",) if operations else ()):
        dtype = np.int64 if key == "target" else np.uint8 if key == "aln_flat" else np.int32
        out[key] = np.concatenate([p[key] for p in parts]) if parts else np.zeros(0, dtype=dtype)
    if operations:
        lengths = np.concatenate([np.diff(p["aln_off"]) for p in parts]) if parts else np.zeros(0, dtype=np.int64)
        out["aln_off"] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return out


def assert_csr(got, want, context, operations=True):
    """every array of the CSR: the five of the search, the starts, the operations and their lengths"""
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], want["offsets"]), (context, got["offsets"], want["offsets"])
    for key in FIVE + STARTS + (("aln_off", "aln_flat") if operations else ()):
        assert got[key].dtype == want[key].dtype, (context, key, got[key].dtype)
        assert len(got[key]) == len(want[key]), (context, key, len(got[key]), len(want[key]))
        assert np.array_equal(got[key], want[key]), (context, key, np.flatnonzero(got[key] != want[key])[:8])
    if operations:
        assert got["aln_off"][0] == 0 and got["aln_off"][-1] == len(got["aln_flat"]), context
    else:
        assert not [key for key in got if key.startswith("aln")], (context, sorted(got))


def some(got, chosen):
    """the occurrences `chosen` of an answer as an answer of their own"""
    chosen = np.asarray(chosen, dtype=np.int64)
    off = got["aln_off"]
    out = {key: got[key][chosen] for key in FIVE + STARTS}
    out["aln_off"] = np.concatenate([[0], np.cumsum(np.diff(off)[chosen])]).astype(np.int64)
    pieces = [got["aln_flat"][off[k]:off[k + 1]] for k in chosen.tolist()]
    out["aln_flat"] = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    return out


def assert_helper(got, chosen, query, matrix, alphabet, targets, gaps, algorithm, context, target_base=0):
    """the second witness on the occurrences `chosen`. The helper runs one numpy lane per occurrence over as many
    columns as the longest prefix among them: occurrences that end in similar columns go together."""
    chosen = np.asarray(chosen, dtype=np.int64)
    rows = matrix.reshape(alphabet, alphabet)[query]
    bucket = got["end_t"][chosen] // 32
    for b in np.unique(bucket).tolist():
        assert_alignments(some(got, chosen[bucket == b]), rows, query, matrix, targets, gaps, algorithm, (context, b), target_base)


# ---- 1: the panel equals the singles, and the helper ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def panel_set(name):
    """130 targets (two full wavefronts and a ragged third) of 1 .. 300 residues - most of them short, so that the
    helper's lanes at window 0 stay a few thousand per query; the strip's edges and the longest among them - and the
    panel of tests/test_gpu_batch_occurrences.py, in this alphabet"""
    matrix, alphabet = MATRICES[name]
    rng = np.random.default_rng(500 + alphabet)
    lengths = rng.integers(1, 61, size=130)
    lengths[:8] = (1, 2, 63, 64, 65, 130, 299, 300)
    rng.shuffle(lengths)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    panel = [rng.integers(0, alphabet, size=q).astype(np.uint8) for q in PANEL]
    return residues, offsets, targets, lengths, panel


@pytest.fixture(scope="module")
def panel_dbs(capi):
    dbs = {}
    for name, (matrix, alphabet) in MATRICES.items():
        residues, offsets, _, _, _ = panel_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, alphabet)
    yield dbs
    for db in dbs.values():
        db.close()


def rule_of(panel, algorithm, rng):
    """test_gpu_batch_occurrences.py's: one cut and one window per query, one query whose cut nothing reaches"""
    windows = [(0, None, 5)[k] for k in rng.integers(0, 3, size=len(panel))]
    if algorithm == "hw":
        cuts = [int(-2 * len(q) - rng.integers(0, 6)) for q in panel]
    else:
        cuts = [int(1 + rng.integers(0, 8)) for q in panel]
    cuts[NOWHERE] = 10 ** 6
    return cuts, windows


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("gaps", GAPS)
def test_panel_equals_singles_and_the_helper(panel_dbs, gaps, name):
    """64, 1, 9, 8, 7, 0, 63, 24, 65, 130 and 2 rows: a short query right behind a tall one and the reverse - a wrong
    query origin reads another query's residues - and a long and an empty query spliced in between"""
    matrix, alphabet = MATRICES[name]
    _, _, targets, lengths, panel = panel_set(name)
    db = panel_dbs[name]
    rng = np.random.default_rng(gaps[0] * 10 + gaps[1])
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(panel, algorithm, rng)
        context = (name, gaps, algorithm)
        got = db.search_batch_occurrence_alignments(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        sweeps, stage = db.last_batch_occurrence_routing(), db.last_batch_occurrence_align_routing()
        want = singles(db, panel, matrix, gaps, algorithm, cuts, windows)
        assert_csr(got, want, context)
        counts = np.diff(got["offsets"])
        assert counts[NOWHERE] == 0 and counts[NOWHERE - 1] > 0 and counts[NOWHERE + 1] > 0, (context, counts)
        assert counts[PANEL.index(0)] == 0 and counts[PANEL.index(130)] > 0 and counts[PANEL.index(65)] > 0, (context, counts)
        # eight queries on the panel kernels in one chunk, two on the single-query path; one stage behind each of the three
        assert sweeps[:3] == [8, 2, 1], (context, sweeps)
        assert stage[0] + stage[1] == got["offsets"][-1] and stage[2] >= 3, (context, stage)
        assert stage[3] == (got["end_t"] - got["start_t"] + 1).max(), (context, stage)
        # ... and the ends are search_batch_occurrences', byte for byte
        ends = db.search_batch_occurrences(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        for key in ("offsets",) + FIVE:
            assert got[key].tobytes() == ends[key].tobytes(), (context, key)
        if gaps != GAPS[0]:
            continue
        # window 0 at the lowest cut (the degenerate all-gap optimum of HW among them): every occurrence against the helper
        cut = INT_MIN if algorithm == "hw" else 1
        every = db.search_batch_occurrence_alignments(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cut, window=0)
        assert len(every["offsets"]) == len(panel) + 1 and every["offsets"][0] == 0
        for i, query in enumerate(panel):
            lo, hi = int(every["offsets"][i]), int(every["offsets"][i + 1])
            if len(query) == 0:
                assert lo == hi
                continue
            assert algorithm != "hw" or hi - lo == lengths.sum(), (context, i)
            assert_helper(every, np.arange(lo, hi), query, matrix, alphabet, targets, gaps, algorithm, (context, i))


# ---- 2: queries without occurrences in every position -----------------------------------------------------------------

def test_queries_without_occurrences_in_every_position(capi):
    """Ten queries of 20 letters, cuts at the exact-match score, sites planted for six of them: the first query, the
    last, and two neighbours in the middle have none - equal neighbours in the per-query offsets the gather searches.
    Every planted site comes back with its planted start and an all-match alignment; nothing else comes back."""
    rng = np.random.default_rng(57)
    lengths = rng.integers(80, 151, size=300)
    reads = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lengths]
    panel = [rng.integers(0, 4, size=20).astype(np.uint8) for _ in range(10)]
    empty = (0, 4, 5, 9)
    planted = set()       # (query, read, start column)
    for i in range(10):
        if i in empty:
            continue
        for read in rng.choice(300, size=3 + i, replace=False).tolist():
            sites = (5, 50) if read % 7 == 0 else (int(rng.integers(0, lengths[read] - 20)),)
            for at in sites:
                reads[read][at:at + 20] = panel[i]
    # (a later plant may have overwritten an earlier one: the sites are what the reads hold in the end)
    for i in range(10):
        for read in range(300):
            here = np.all(np.lib.stride_tricks.sliding_window_view(reads[read], 20) == panel[i], axis=1)
            planted.update((i, read, int(at)) for at in np.flatnonzero(here))
    assert {i for i, _, _ in planted} == set(range(10)) - set(empty) and len(planted) > 40
    residues, offsets = _flatten(reads)
    db = capi.DeviceDatabase(residues, offsets, 4)
    try:
        for algorithm in ("hw", "sw"):
            got = db.search_batch_occurrence_alignments(panel, DNA, 3, 1, algorithm, min_score=100)
            counts = np.diff(got["offsets"])
            assert all(counts[i] == 0 for i in empty) and all(counts[i] > 0 for i in range(10) if i not in empty), counts
            owner = np.repeat(np.arange(10), counts)
            seen = set(zip(owner.tolist(), got["target"].tolist(), got["start_t"].tolist()))
            assert seen == planted and len(got["target"]) == len(planted), (algorithm, seen ^ planted)
            assert np.all(got["score"] == 100) and np.all(got["start_q"] == 0) and np.all(got["end_q"] == 19)
            assert np.all(got["end_t"] - got["start_t"] == 19)
            assert np.array_equal(got["aln_off"], 20 * np.arange(len(planted) + 1)) and np.all(got["aln_flat"] == MATCH)
            assert db.last_batch_occurrence_align_routing()[0] + db.last_batch_occurrence_align_routing()[1] == len(planted)
            assert_csr(got, singles(db, panel, DNA, (3, 1), algorithm, [100] * 10, [None] * 10), algorithm)
    finally:
        db.close()


# ---- 3: panel chunks --------------------------------------------------------------------------------------------------

def test_panel_chunks(panel_dbs, tuning):
    """the eight panel queries in three chunks (3 + 3 + 2) and one a chunk: the bytes of the one-chunk answer. Every
    chunk but the first counts behind a stage that took the slots of the slice's sorted jobs: its ends are still
    search_batch_occurrences'."""
    name, gaps = "blosum62", (11, 1)
    matrix, alphabet = MATRICES[name]
    _, _, targets, lengths, panel = panel_set(name)
    db = panel_dbs[name]
    rng = np.random.default_rng(3)
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(panel, algorithm, rng)
        call = lambda: db.search_batch_occurrence_alignments(panel, matrix, *gaps, algorithm, min_score=cuts, window=windows)   # noqa: E731
        whole = call()
        assert db.last_batch_occurrence_routing()[:3] == [8, 2, 1]
        one = db.last_batch_occurrence_align_routing()
        assert np.all(np.diff(whole["offsets"])[[i for i in ON_PANEL if i != NOWHERE]] > 0)
        for entries, chunks in ((3 * len(lengths), 3), (100, 8)):
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", str(entries))
            got = call()
            assert db.last_batch_occurrence_routing()[:3] == [8, 2, chunks], (algorithm, entries)
            stage = db.last_batch_occurrence_align_routing()
            for key in ("offsets",) + ALL:
                assert got[key].dtype == whole[key].dtype and got[key].tobytes() == whole[key].tobytes(), (algorithm, entries, key)
            # a stage per chunk that has occurrences (the query whose cut nothing reaches is a chunk of its own at 8)
            assert stage[2] >= one[2] + chunks - 1 - (chunks == 8), (algorithm, entries, stage, one)
            assert stage[0] + stage[1] == one[0] + one[1] == whole["offsets"][-1] and stage[3] == one[3]
            ends = db.search_batch_occurrences(panel, matrix, *gaps, algorithm, min_score=cuts, window=windows)
            assert db.last_batch_occurrence_routing()[:3] == [8, 2, chunks]
            for key in ("offsets",) + FIVE:
                assert got[key].tobytes() == ends[key].tobytes(), (algorithm, entries, key)
            tuning.delenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES")


# ---- 4: sub-chunks of the stage ---------------------------------------------------------------------------------------

def test_stage_sub_chunks(capi):
    """One repetitive target of 8000 residues among a dozen short ones, window 0, the lowest HW cut, four queries of 40
    to 64 rows: every column of every target is an occurrence of every query - more than 32 000, and more than one
    sub-chunk of the stage holds (sized by the longest target that has an occurrence). More sub-chunks than queries:
    whatever their size, one of their boundaries falls inside a query's stretch."""
    rng = np.random.default_rng(14)
    panel = [_data.random_protein(rng, q) for q in (64, 40, 57, 48)]
    unit = np.concatenate([q[5:25] for q in panel] + [_data.random_protein(rng, 11)])
    long_target = np.tile(unit, 8000 // len(unit) + 1)[:8000].astype(np.uint8)
    targets = [_data.random_protein(rng, int(n)) for n in rng.integers(1, 200, size=12)]
    targets.insert(5, long_target)
    residues, offsets = _oracle.flatten(targets)
    B62, alphabet = MATRICES["blosum62"]
    gaps = (11, 1)
    db = capi.DeviceDatabase(residues, offsets, alphabet)
    try:
        rule = dict(min_score=INT_MIN, window=0)
        got = db.search_batch_occurrence_alignments(panel, B62, *gaps, "hw", **rule)
        sweeps, stage = db.last_batch_occurrence_routing(), db.last_batch_occurrence_align_routing()
        total = int(got["offsets"][-1])
        per_query = sum(len(t) for t in targets)
        assert got["offsets"].tolist() == [per_query * i for i in range(5)] and total > 32000
        assert sweeps[:3] == [4, 0, 1]
        assert stage[2] > sweeps[2] and stage[2] > len(panel), (stage, sweeps)
        assert stage[0] + stage[1] == total, stage
        want = singles(db, panel, B62, gaps, "hw", [INT_MIN] * 4, [0] * 4)
        assert_csr(got, want, "sub-chunks")
        # a handful against the helper: both ends, both sides of every query boundary, both ends of the long target
        first = int(np.searchsorted(got["target"][:per_query], 5))
        for i, query in enumerate(panel):
            lo = per_query * i
            chosen = [lo, lo + 1, lo + first, lo + first + 1, lo + first + 7999, lo + per_query - 2, lo + per_query - 1]
            assert_helper(got, chosen, query, B62, alphabet, targets, gaps, "hw", ("sub-chunks", i))
        # starts only: the same starts, no direction work, and no more sub-chunks than the full form
        only = db.search_batch_occurrence_alignments(panel, B62, *gaps, "hw", operations=False, **rule)
        without = db.last_batch_occurrence_align_routing()
        assert_csr(only, want, "sub-chunks, starts only", operations=False)
        assert without[:2] == [0, 0] and 1 <= without[2] <= stage[2] and without[3] == stage[3], (without, stage)
    finally:
        db.close()


# ---- 5: starts only ---------------------------------------------------------------------------------------------------

def test_starts_only(panel_dbs):
    name, gaps = "random32", (3, 1)
    matrix, alphabet = MATRICES[name]
    _, _, _, _, panel = panel_set(name)
    db = panel_dbs[name]
    rng = np.random.default_rng(8)
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(panel, algorithm, rng)
        full = db.search_batch_occurrence_alignments(panel, matrix, *gaps, algorithm, min_score=cuts, window=windows)
        with_ops = db.last_batch_occurrence_align_routing()
        only = db.search_batch_occurrence_alignments(panel, matrix, *gaps, algorithm, min_score=cuts, window=windows,
                                                     operations=False)
        without = db.last_batch_occurrence_align_routing()
        assert full["offsets"][-1] > 300
        assert sorted(only) == ["end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]
        assert sorted(full) == sorted(list(only) + ["aln", "aln_flat", "aln_off"])
        for key in ("offsets",) + FIVE + STARTS:
            assert only[key].dtype == full[key].dtype and only[key].tobytes() == full[key].tobytes(), (algorithm, key)
        assert with_ops[0] + with_ops[1] == full["offsets"][-1]
        assert without[:2] == [0, 0] and 1 <= without[2] <= with_ops[2] and without[3] == with_ops[3] > 1, (without, with_ops)
        assert_csr(only, singles(db, panel, matrix, gaps, algorithm, cuts, windows, operations=False), algorithm, operations=False)


# ---- 6: the contract, through ctypes ------------------------------------------------------------------------------------

def test_contract(capi, panel_dbs, tuning):
    name, gaps = "blosum62", (11, 1)
    matrix, alphabet = MATRICES[name]
    _, _, targets, lengths, panel = panel_set(name)
    db = panel_dbs[name]
    cuts, windows = [-100, -5, -12, -12, -10, 0, -90, -30, -100, -200, -5], [None, 0, 5, None, 0, 3, None, 5, 20, None, 0]
    rule = dict(min_score=cuts, window=windows)
    whole = db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", **rule)
    total = int(whole["offsets"][-1])
    counts = np.diff(whole["offsets"])
    assert total > 300 and all(counts[i] > 0 for i in range(len(panel)) if len(panel[i]))
    # two calls return the same bytes
    again = db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", **rule)
    for key in ("offsets",) + ALL:
        assert again[key].tobytes() == whole[key].tobytes(), key
    # a slice in the middle of the handle: absolute target indices, and what the singles return for it
    start, end = 37, 101
    part = db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", start, end, **rule)
    assert_csr(part, singles(db, panel, matrix, gaps, "hw", cuts, windows, start, end), "slice")
    assert part["offsets"][-1] > 0 and part["target"].min() >= start and part["target"].max() < end
    lo = int(part["offsets"][0])
    assert_helper(part, np.arange(lo, lo + min(40, int(part["offsets"][1]))), panel[0], matrix, alphabet, targets, gaps, "hw", "slice")
    # an empty panel, an empty slice, a panel of only empty queries: no occurrences, the offsets hold their single 0
    nothing = np.zeros(0, dtype=np.uint8)
    for got, queries in ((db.search_batch_occurrence_alignments([], matrix, *gaps, "hw"), 0),
                         (db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", 40, 40, **rule), len(panel)),
                         (db.search_batch_occurrence_alignments([nothing, nothing], matrix, *gaps, "hw", min_score=0), 2)):
        assert got["offsets"].tolist() == [0] * (queries + 1) and all(len(got[key]) == 0 for key in FIVE + STARTS + ("aln_flat",))
        assert got["aln_off"].dtype == np.int64 and got["aln_off"].tolist() == [0] and len(got["aln"]) == 0
        assert db.last_batch_occurrence_align_routing() == [0, 0, 0, 0]
    got = db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", min_score=10 ** 6)
    assert got["offsets"][-1] == 0 and got["aln_off"].tolist() == [0] and db.last_batch_occurrence_align_routing() == [0, 0, 0, 0]

    # the C ABI: what a refused call leaves of its outputs
    lib = capi.lib()
    flat = np.concatenate(panel)
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in panel])]).astype(np.int64)
    m = np.ascontiguousarray(matrix)
    w = np.ascontiguousarray([(len(q) if x is None else x) for q, x in zip(panel, windows)], dtype=np.int32)
    s = np.ascontiguousarray(cuts, dtype=np.int32)

    def call(max_hits=-1, missing=(), mode=1):
        hit_offsets = np.full(len(panel) + 1, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(8)]
        refs = [None if i in missing else ctypes.byref(p) for i, p in enumerate(ptrs)]
        rc = lib.miopalSearchBatchOccurrencesAligned(db.handle, flat.ctypes.data, qoff.ctypes.data, len(panel), *gaps,
                                                     m.ctypes.data, alphabet, mode, 0, len(lengths), s.ctypes.data,
                                                     w.ctypes.data, max_hits, hit_offsets.ctypes.data, *refs)
        return rc, hit_offsets, all(p.value == 0x77 for p in ptrs)

    # exactly one of alignments / alignmentOffsets missing, a missing start output: 101, every output as it was
    for missing, text in (((6,), "both, or neither"), ((7,), "both, or neither"), ((4,), "null start-location"), ((5, 6, 7), "null start-location")):
        rc, hit_offsets, untouched = call(missing=missing)
        assert rc == BAD and text in capi.last_error(), (missing, rc, capi.last_error())
        assert np.all(hit_offsets == -7) and untouched, missing
    # ... behind miopalSearchBatchOccurrences' own checks
    rc, hit_offsets, untouched = call(missing=(6,), mode=0)
    assert rc == capi.OPAL_ERR_INVALID_MODE and np.all(hit_offsets == -7) and untouched
    # maxHits below the total: TooManyHits, hitOffsets filled, every pointer as it was - in one chunk, and in three
    # where the bound is passed in the last one (the chunks before it have been aligned by then, and are discarded)
    on_panel = [int(counts[i]) for i in ON_PANEL]
    for entries, chunks in ((None, 1), (3 * len(lengths), 3)):
        if entries:
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", str(entries))
        bound = total - 1
        if chunks == 3:
            assert sum(on_panel[6:]) > 0
            long_ones = total - sum(on_panel)
            assert bound - long_ones >= sum(on_panel[:6]), "the bound is passed in the last chunk, not before"
        rc, hit_offsets, untouched = call(max_hits=bound)
        assert rc == TOO_MANY and "maxHits" in capi.last_error(), (chunks, rc)
        assert np.array_equal(hit_offsets, whole["offsets"]) and untouched, chunks
        assert db.last_batch_occurrence_routing()[2] == chunks
        with pytest.raises(capi.TooManyHits) as info:
            db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", max_hits=bound, **rule)
        assert np.array_equal(info.value.counts, whole["offsets"])
        bounded = db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", max_hits=total, **rule)
        assert_csr(bounded, whole, ("max_hits = total", chunks))
        if entries:
            tuning.delenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES")
    # ... and the handle works afterwards
    assert_csr(db.search_batch_occurrence_alignments(panel, matrix, *gaps, "hw", **rule), whole, "afterwards")


def test_range_check_of_one_query_refuses_the_call(capi):
    """tests/test_gpu_batch_occurrences.py's: a matrix of 2^26 and a query of 70 rows fail miopalSearch's 32-bit range
    check, a query of 5 rows beside it passes - the whole call is refused before any device work, every output as it was"""
    rng = np.random.default_rng(2)
    residues, offsets = _data.random_db(rng, [50, 60])
    huge = np.full(24 * 24, 2 ** 26, dtype=np.int32)
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        short, tall = _data.random_protein(rng, 5), _data.random_protein(rng, 70)
        with pytest.raises(OverflowError):
            db.search_batch_occurrence_alignments([short, tall], huge, 3, 1, "hw", min_score=0, window=0)
        flat = np.concatenate([short, tall]).astype(np.uint8)
        qoff = np.array([0, 5, 75], dtype=np.int64)
        cuts, windows = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        hit_offsets = np.full(3, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(8)]
        rc = capi.lib().miopalSearchBatchOccurrencesAligned(db.handle, flat.ctypes.data, qoff.ctypes.data, 2, 3, 1,
                                                            huge.ctypes.data, 24, 1, 0, 2, cuts.ctypes.data, windows.ctypes.data,
                                                            -1, hit_offsets.ctypes.data, *[ctypes.byref(p) for p in ptrs])
        assert rc == OVERFLOW == capi.OPAL_ERR_OVERFLOW
        assert np.all(hit_offsets == -7) and all(p.value == 0x77 for p in ptrs)
        assert db.last_batch_occurrence_align_routing() == [0, 0, 0, 0]     # (no stage has run)
        B62 = MATRICES["blosum62"][0]
        got = db.search_batch_occurrence_alignments([short, tall], B62, 3, 1, "sw", min_score=1, window=0)
        assert np.all(np.diff(got["offsets"]) > 0)
    finally:
        db.close()


# ---- 7: the free functions ----------------------------------------------------------------------------------------------

def test_find_occurrence_alignments_many_equals_find_occurrences(capi):
    rng = np.random.default_rng(93)
    targets = [_data.random_protein(rng, int(n)) for n in rng.integers(0, 201, size=130)]
    panel = [_data.random_protein(rng, q) for q in PANEL]
    text = lambda codes: "".join(_data.NCBI[c] for c in codes)   # noqa: E731
    aligner = pyopal_amd.Aligner("BLOSUM62", gap_open=11, gap_extend=1)
    database = pyopal_amd.Database([text(t) for t in targets])
    queries = [text(q) for q in panel]
    fields = lambda r: (type(r), r.target_index, r.score, r.target_end, r.query_end, r.target_start, r.query_start,   # noqa: E731
                        r.query_length, r.target_length, r.alignment, r.cigar())
    for algorithm, cut in (("hw", -10), ("sw", 12)):
        cuts = [cut + k for k in range(len(queries))]
        windows = [None if k % 2 else k for k in range(len(queries))]
        found = pyopal_amd.find_occurrence_alignments_many(aligner, queries, database, cuts, algorithm=algorithm, window=windows)
        assert len(found) == len(queries) and sum(len(f) for f in found) > 100
        for i, (query, mine) in enumerate(zip(queries, found)):
            alone = pyopal_amd.find_occurrences(aligner, query, database, cuts[i], algorithm=algorithm, window=windows[i], mode="full")
            assert [fields(r) for r in mine] == [fields(r) for r in alone], (algorithm, i)
            assert all(isinstance(r, pyopal_amd.FullResult) for r in mine)
        # the arrays form against the objects; a slice; starts only
        arrays = pyopal_amd.find_occurrence_alignments_many_arrays(aligner, queries, database, cuts, algorithm=algorithm, window=windows)
        assert sorted(arrays) == ["aln_flat", "aln_off", "end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]
        flat = [r for mine in found for r in mine]
        assert arrays["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(f) for f in found])]).tolist()
        for key, name in (("target", "target_index"), ("score", "score"), ("end_t", "target_end"), ("end_q", "query_end"),
                          ("start_t", "target_start"), ("start_q", "query_start")):
            assert arrays[key].tolist() == [getattr(r, name) for r in flat], (algorithm, key)
        assert np.diff(arrays["aln_off"]).tolist() == [len(r.alignment) for r in flat]
        assert "".join("MDIX"[o] for o in arrays["aln_flat"].tolist()) == "".join(r.alignment for r in flat)
        part = pyopal_amd.find_occurrence_alignments_many_arrays(aligner, queries, database, cuts, algorithm=algorithm,
                                                                 window=windows, start=20, end=90, operations=False)
        assert sorted(part) == ["end_q", "end_t", "offsets", "score", "start_q", "start_t", "target"]
        for i, query in enumerate(queries):
            alone = pyopal_amd.find_occurrences_arrays(aligner, query, database, cuts[i], algorithm=algorithm, window=windows[i],
                                                       start=20, end=90)
            lo, hi = part["offsets"][i], part["offsets"][i + 1]
            assert hi - lo == alone["count"]
            for key in FIVE + STARTS:
                assert np.array_equal(part[key][lo:hi], alone[key]), (algorithm, i, key)
    with pytest.raises(capi.TooManyHits) as info:
        pyopal_amd.find_occurrence_alignments_many(aligner, queries, database, -10, max_hits=3)
    assert len(info.value.counts) == len(queries) + 1 and info.value.counts[-1] > 3


# ---- 8: the case list of tests/_cases.py ----------------------------------------------------------------------------------

LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_panel_of_the_case_equals_singles(capi, case):
    """the case's queries of 1, 7, 64, 65 and 130 rows as one panel against the case's targets, at the lowest cut, held to
    the unchanged search_occurrence_alignments of one query at a time. Through find_occurrence_alignments_many_arrays
    where the case's alphabet can be spelt (an `Alphabet` holds 26 letters and the wildcard: not the cases of 32
    letters, which go through DeviceDatabase.search_batch_occurrence_alignments alone)."""
    s, panel = case.search_set(), case.pair_set().queries
    assert sorted(len(q) for q in panel) == sorted(_cases.QUERY_LENGTHS)
    on_panel = sum(1 <= len(q) <= 64 for q in panel)
    A = case.alphabet
    db = capi.DeviceDatabase(s.residues, s.offsets, A)
    try:
        for algorithm in ("hw", "sw"):
            cut = cut_of(algorithm)
            cuts, windows = [cut] * len(panel), [None] * len(panel)
            want = singles(db, panel, s.matrix, case.gaps, algorithm, cuts, windows)
            got = db.search_batch_occurrence_alignments(panel, s.matrix, *case.gaps, algorithm, min_score=cut, window=None)
            assert db.last_batch_occurrence_routing()[:3] == [on_panel, len(panel) - on_panel, 1], (case.id, algorithm)
            assert_csr(got, want, (case.id, algorithm))
            if algorithm == "hw":
                assert np.all(np.diff(got["offsets"]) >= np.count_nonzero(s.lengths)), (case.id, got["offsets"])
            if A > len(LETTERS):
                continue
            text = lambda codes: "".join(LETTERS[c] for c in codes)   # noqa: E731
            aligner = pyopal_amd.Aligner(ScoringMatrix(s.matrix.reshape(A, A).tolist(), LETTERS[:A]), gap_open=case.gaps[0],
                                         gap_extend=case.gaps[1])
            database = pyopal_amd.Database([text(t) for t in s.targets], alphabet=pyopal_amd.Alphabet(LETTERS[:A]))
            arrays = pyopal_amd.find_occurrence_alignments_many_arrays(aligner, [text(q) for q in panel], database, cut,
                                                                       algorithm=algorithm)
            assert_csr(arrays, want, (case.id, algorithm, "free function"))
    finally:
        db.close()
