"""Every occurrence of a whole panel of queries in one call (miopalSearchBatchOccurrences;
DeviceDatabase.search_batch_occurrences; pyopal_amd.find_occurrences_many). Two witnesses, neither of them the code
under test: the unchanged search_occurrences of one query at a time, and the numpy recurrence with the rule
(column_values / expected of tests/test_gpu_occurrences.py, tests/_occurrences.py)."""
import ctypes
import functools

import numpy as np
import pytest

import _data
import _pssm
import pyopal_amd
from _occurrences import INT_MIN
from test_gpu_occurrences import GAPS, MATRICES, column_values, expected

pytestmark = pytest.mark.gpu

KEYS = ("target", "score", "end_t", "end_q")
DNA = np.where(np.eye(4, dtype=bool), 5, -4).astype(np.int32).ravel()       # 4 letters: match 5, mismatch -4
SETS = dict(MATRICES, dna4=(DNA, 4))
# a short query right behind a tall one and the reverse (stale rows of the query before would show), an empty one,
# and two of more than 64 rows
PANEL = (64, 1, 9, 8, 7, 0, 63, 24, 65, 130, 2)
NOWHERE = 3          # the query whose cut no target reaches: an empty stretch in the middle of the CSR
TOO_MANY, BAD, OVERFLOW = 103, 101, 1
# How the host groups a chunk's queries for the count sweep. "spread": the library's own rule - with the few targets of
# these tests, one query a group. "filled": MIOPAL_BATCH_OCCURRENCE_WORKGROUPS_PER_CU = 0 - a group is as many queries as
# fit the 160 KB of LDS, the form a large read set runs: a lane walks its target once per query of the group.
GROUPINGS = ("spread", "filled")
LDS = 160 * 1024


def lds_bytes(rows, alphabet):
    """a group's table: its queries' rows, each query padded to a multiple of eight, alphabet + 1 ints a row"""
    return sum((q + 7) // 8 * 8 for q in rows) * (alphabet + 1) * 4


def filled_groups(rows, alphabet):
    """the groups of "filled", restated: consecutive queries while their tables fit the LDS -> [[rows of a query, ...], ...]"""
    groups = [[]]
    for q in rows:
        if groups[-1] and lds_bytes(groups[-1] + [q], alphabet) > LDS:
            groups.append([])
        groups[-1].append(q)
    return groups


def group(tuning, grouping):
    if grouping == "filled":
        tuning.setenv("MIOPAL_BATCH_OCCURRENCE_WORKGROUPS_PER_CU", "0")
    else:
        tuning.delenv("MIOPAL_BATCH_OCCURRENCE_WORKGROUPS_PER_CU")


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def singles(db, panel, matrix, gaps, algorithm, cuts, windows, start=0, end=None):
    """the first witness: search_occurrences query by query, laid end to end as the CSR"""
    parts = [db.search_occurrences(q, matrix, gaps[0], gaps[1], algorithm, start, end, min_score=int(c), window=w)
             for q, c, w in zip(panel, cuts, windows)]
    out = {"offsets": np.concatenate([[0], np.cumsum([p["count"] for p in parts])]).astype(np.int64)}
    for key in KEYS:
        out[key] = np.concatenate([p[key] for p in parts]) if parts else np.zeros(0, dtype=np.int64 if key == "target" else np.int32)
    return out


def assert_csr(got, want, context):
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], want["offsets"]), (context, got["offsets"], want["offsets"])
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, (context, key)
        assert np.array_equal(got[key], want[key]), (context, key, np.flatnonzero(got[key] != want[key])[:8])


# ---- 1: the panel equals the singles and the recurrence -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def panel_set(name):
    """130 targets (two full wavefronts and a ragged third) of 0 .. 200 residues, lengths 0 and 1 among them; the panel"""
    matrix, alphabet = SETS[name]
    rng = np.random.default_rng(300 + alphabet)
    lengths = rng.integers(0, 201, size=130)
    lengths[:5] = (0, 1, 200, 64, 65)
    rng.shuffle(lengths)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    panel = [rng.integers(0, alphabet, size=q).astype(np.uint8) for q in PANEL]
    return residues, offsets, targets, lengths, panel


@pytest.fixture(scope="module")
def panel_dbs(capi):
    dbs = {}
    for name, (matrix, alphabet) in SETS.items():
        residues, offsets, _, _, _ = panel_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, alphabet)
    yield dbs
    for db in dbs.values():
        db.close()


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("gaps", GAPS)
def test_panel_equals_singles_and_the_recurrence(panel_dbs, tuning, gaps, name, grouping):
    """"filled": the eight panel queries 64, 1, 9, 8, 7, 63, 24, 2 are ONE group - every lane walks its target eight times,
    a short query right behind a tall one and the reverse, each against its own rows of the shared table"""
    group(tuning, grouping)
    on_panel = [q for q in PANEL if 1 <= q <= 64]
    matrix, alphabet = SETS[name]
    _, _, targets, lengths, panel = panel_set(name)
    db = panel_dbs[name]
    rng = np.random.default_rng(gaps[0] * 10 + gaps[1])
    for algorithm in ("hw", "sw"):
        windows = [(0, None, 5)[k] for k in rng.integers(0, 3, size=len(panel))]
        if algorithm == "hw":
            cuts = [int(-2 * len(q) - rng.integers(0, 6)) for q in panel]
        else:
            cuts = [int(1 + rng.integers(0, 8)) for q in panel]
        cuts[NOWHERE] = 10 ** 6
        context = (name, gaps, algorithm)
        got = db.search_batch_occurrences(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        routing = db.last_batch_occurrence_routing()
        want = singles(db, panel, matrix, gaps, algorithm, cuts, windows)
        assert_csr(got, want, context)
        counts = np.diff(got["offsets"])
        assert counts[NOWHERE] == 0 and counts[NOWHERE - 1] > 0 and counts[NOWHERE + 1] > 0, (context, counts)
        assert counts[PANEL.index(0)] == 0 and counts[PANEL.index(130)] > 0 and counts[PANEL.index(65)] > 0, (context, counts)
        # eight queries on the panel kernels, two on the single-query path, the empty one in neither; one chunk
        assert routing[:3] == [8, 2, 1], (context, routing)
        want_groups = [1, 8, lds_bytes(on_panel, alphabet)] if grouping == "filled" else [8, 1, lds_bytes([64], alphabet)]
        assert db.last_batch_occurrence_groups() == want_groups, (context, db.last_batch_occurrence_groups())
        pairs = sum(len(set(got["target"][got["offsets"][i]:got["offsets"][i + 1]].tolist()))
                    for i, q in enumerate(PANEL) if 1 <= q <= 64)
        assert routing[3] == pairs, (context, routing, pairs)
        # window 0 at the lowest cut: every column value (every positive column maximum under SW) of the recurrence
        cut = INT_MIN if algorithm == "hw" else 1
        every = db.search_batch_occurrences(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cut, window=0)
        assert len(every["offsets"]) == len(panel) + 1 and every["offsets"][0] == 0
        assert db.last_batch_occurrence_groups() == want_groups, context
        for i, query in enumerate(panel):
            lo, hi = every["offsets"][i], every["offsets"][i + 1]
            if len(query) == 0:
                assert lo == hi
                continue
            V, R = column_values(matrix.reshape(alphabet, alphabet)[query], targets, gaps[0], gaps[1], algorithm)
            rule = expected(V, R, lengths, cut, 0)
            for key in KEYS:
                assert np.array_equal(every[key][lo:hi], rule[key]), (context, i, key)
            if algorithm == "hw":
                assert hi - lo == lengths.sum()


# ---- 2: groups and chunks -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grouping", GROUPINGS)
def test_groups_and_chunks(capi, tuning, grouping):
    """40 queries of 64 rows at 32 letters: 40 x 64 x 33 x 4 bytes = 338 KB of rows. "filled": three groups - 19 queries
    fill the 160 KB, twice, and two are left - in one chunk; 14 + 14 + 12 queries in three chunks, a group each; one
    query a chunk. "spread": one query a group throughout."""
    group(tuning, grouping)
    filled = grouping == "filled"
    matrix, alphabet = MATRICES["random32"]
    rng = np.random.default_rng(41)
    lengths = rng.integers(0, 61, size=130)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    panel = [rng.integers(0, alphabet, size=64).astype(np.uint8) for _ in range(40)]
    db = capi.DeviceDatabase(residues, offsets, alphabet)
    try:
        for algorithm, cut in (("hw", -20), ("sw", 25)):
            cuts, windows = [cut] * len(panel), [None] * len(panel)
            want = singles(db, panel, matrix, (3, 1), algorithm, cuts, windows)
            assert want["offsets"][-1] > 500 and np.all(np.diff(want["offsets"]) > 0)
            got = db.search_batch_occurrences(panel, matrix, 3, 1, algorithm, min_score=cut)
            assert_csr(got, want, (algorithm, "one chunk"))
            assert db.last_batch_occurrence_routing()[:3] == [40, 0, 1]
            assert [len(g) for g in filled_groups([64] * 40, 32)] == [19, 19, 2] and lds_bytes([64] * 19, 32) > 64 * 1024
            assert db.last_batch_occurrence_groups() == ([3, 19, lds_bytes([64] * 19, 32)] if filled else [40, 1, lds_bytes([64], 32)])
            # 14 queries x 130 targets a chunk: 14 + 14 + 12
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", str(14 * 130))
            got = db.search_batch_occurrences(panel, matrix, 3, 1, algorithm, min_score=cut)
            assert_csr(got, want, (algorithm, "three chunks"))
            assert db.last_batch_occurrence_routing()[:3] == [40, 0, 3]
            assert db.last_batch_occurrence_groups() == ([3, 14, lds_bytes([64] * 14, 32)] if filled else [40, 1, lds_bytes([64], 32)])
            # ... and one query a chunk when the slice alone passes the bound
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", "100")
            got = db.search_batch_occurrences(panel[:5], matrix, 3, 1, algorithm, min_score=cut)
            assert_csr(got, singles(db, panel[:5], matrix, (3, 1), algorithm, cuts[:5], windows[:5]), (algorithm, "five chunks"))
            assert db.last_batch_occurrence_routing()[:3] == [5, 0, 5]
            tuning.delenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES")
    finally:
        db.close()


def test_several_queries_share_a_group(capi, tuning):
    """Nothing but this: groups of many queries of unequal heights that fill the LDS. 80 queries of 40 .. 64 rows at 32
    letters with "filled" grouping are at least three groups of more than 150 KB (beyond the 64 KB of a plain launch)
    and a rest, cut where the next query's rows no longer fit; every query behind a group's first reads its rows at an
    offset into the shared table, behind a query of another height. Equal to the singles, all 80; and, for the queries
    on both sides of every cut and at both ends, to the numpy recurrence's every column value."""
    group(tuning, "filled")
    matrix, alphabet = MATRICES["random32"]
    rng = np.random.default_rng(67)
    lengths = rng.integers(0, 61, size=130)
    lengths[:3] = (0, 1, 60)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    rows = [64, 40] + rng.integers(40, 65, size=78).tolist()
    panel = [rng.integers(0, alphabet, size=q).astype(np.uint8) for q in rows]
    groups = filled_groups(rows, alphabet)
    sizes = [len(g) for g in groups]
    full = [g for g in groups if lds_bytes(g, alphabet) > 150 * 1024]
    assert len(full) >= 3 and len(groups) == len(full) + 1 and min(sizes[:-1]) >= 19, sizes
    edges = sorted({0, 1, len(rows) - 1} | {c + d for c in np.cumsum(sizes)[:-1].tolist() for d in (-1, 0, 1)})
    db = capi.DeviceDatabase(residues, offsets, alphabet)
    try:
        for algorithm, low in (("hw", INT_MIN), ("sw", 1)):
            cuts = [int(c) for c in (rng.integers(-30, -10, size=80) if algorithm == "hw" else rng.integers(20, 40, size=80))]
            windows = [(0, None, 5)[k] for k in rng.integers(0, 3, size=80)]
            got = db.search_batch_occurrences(panel, matrix, 3, 1, algorithm, min_score=cuts, window=windows)
            assert db.last_batch_occurrence_routing()[:3] == [80, 0, 1]
            assert db.last_batch_occurrence_groups() == [len(groups), max(sizes), max(lds_bytes(g, alphabet) for g in groups)]
            want = singles(db, panel, matrix, (3, 1), algorithm, cuts, windows)
            assert_csr(got, want, algorithm)
            assert np.all(np.diff(want["offsets"]) > 0)
            every = db.search_batch_occurrences(panel, matrix, 3, 1, algorithm, min_score=low, window=0)
            for i in edges:
                V, R = column_values(matrix.reshape(alphabet, alphabet)[panel[i]], targets, 3, 1, algorithm)
                rule = expected(V, R, lengths, low, 0)
                lo, hi = every["offsets"][i], every["offsets"][i + 1]
                for key in KEYS:
                    assert np.array_equal(every[key][lo:hi], rule[key]), (algorithm, i, key)
    finally:
        db.close()


# ---- 3: the write pass sweeps the pairs that have occurrences, and no others ------------------------------------------

def test_sparse_write(capi):
    rng = np.random.default_rng(53)
    lengths = rng.integers(80, 151, size=300)
    reads = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lengths]
    panel = [rng.integers(0, 4, size=20).astype(np.uint8) for _ in range(5)]
    planted = set()       # (query, read, end column)
    for k, read in enumerate(range(10, 101, 10)):       # the first query: ten reads, two of them twice
        for at in ((5, 50) if k < 2 else (int(rng.integers(0, lengths[read] - 20)),)):
            reads[read][at:at + 20] = panel[0]
            planted.add((0, read, at + 19))
    for read in (0, 299):                               # the second: the first and the last read only
        reads[read][30:50] = panel[1]
        planted.add((1, read, 49))
    residues, offsets = _flatten(reads)
    cut = 100       # twenty matches: only an exact copy reaches it
    db = capi.DeviceDatabase(residues, offsets, 4)
    try:
        cuts, windows = [cut] * 5, [None] * 5
        want = singles(db, panel, DNA, (3, 1), "hw", cuts, windows)
        # the witness alone answers every planted site and nothing else
        seen = {(i, int(t), int(j)) for i in range(5)
                for t, j in zip(want["target"][want["offsets"][i]:want["offsets"][i + 1]],
                                want["end_t"][want["offsets"][i]:want["offsets"][i + 1]])}
        assert seen == planted and len(planted) == 14 and np.all(want["score"] == cut)
        got = db.search_batch_occurrences(panel, DNA, 3, 1, "hw", min_score=cut)
        assert_csr(got, want, "sparse")
        assert got["offsets"].tolist() == [0, 12, 14, 14, 14, 14]
        pairs = len({(i, t) for i, t, _ in planted})
        assert pairs == 12
        assert db.last_batch_occurrence_routing() == [5, 0, 1, pairs]
    finally:
        db.close()


def _flatten(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return np.ascontiguousarray(np.concatenate(seqs), dtype=np.uint8), offsets


# ---- 4: the contract ------------------------------------------------------------------------------------------------

def test_contract(capi, panel_dbs):
    name = "dna4"
    matrix, alphabet = SETS[name]
    _, _, targets, lengths, panel = panel_set(name)
    db = panel_dbs[name]
    panel = panel[:8]          # 64, 1, 9, 8, 7, 0, 63, 24
    cuts, windows = [0, 5, 10, 10, 10, 0, 0, 20], [None, 0, 5, None, 0, 3, None, 5]
    whole = db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts, window=windows)
    total = int(whole["offsets"][-1])
    assert total > 100
    # two calls return the same bytes
    again = db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts, window=windows)
    for key in ("offsets",) + KEYS:
        assert again[key].tobytes() == whole[key].tobytes(), key
    # targets absolute and ascending, columns ascending inside a target, stretch by stretch
    for i in range(len(panel)):
        lo, hi = whole["offsets"][i], whole["offsets"][i + 1]
        t, j = whole["target"][lo:hi], whole["end_t"][lo:hi]
        assert np.all(np.diff(t) >= 0) and np.all((np.diff(t) > 0) | (np.diff(j) > 0)), i
    # a slice returns absolute indices, and what the singles return for it
    start, end = 37, 101
    part = db.search_batch_occurrences(panel, matrix, 3, 1, "hw", start, end, min_score=cuts, window=windows)
    assert_csr(part, singles(db, panel, matrix, (3, 1), "hw", cuts, windows, start, end), "slice")
    assert part["offsets"][-1] > 0 and part["target"].min() >= start and part["target"].max() < end
    # max_hits one below the total: TooManyHits with the offsets; at the total: the answer
    with pytest.raises(capi.TooManyHits) as info:
        db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts, window=windows, max_hits=total - 1)
    assert np.array_equal(info.value.counts, whole["offsets"])
    bounded = db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts, window=windows, max_hits=total)
    assert_csr(bounded, whole, "max_hits = total")
    # no queries, an empty slice: answered, nothing launched
    got = db.search_batch_occurrences([], matrix, 3, 1, "hw")
    assert got["offsets"].tolist() == [0] and all(len(got[key]) == 0 for key in KEYS)
    assert db.last_batch_occurrence_routing() == [0, 0, 0, 0]
    got = db.search_batch_occurrences(panel, matrix, 3, 1, "hw", 40, 40, min_score=cuts, window=windows)
    assert got["offsets"].tolist() == [0] * (len(panel) + 1) and all(len(got[key]) == 0 for key in KEYS)
    assert db.last_batch_occurrence_routing() == [0, 0, 0, 0]

    # the C ABI: what a refused call leaves of its outputs
    lib = capi.lib()
    flat = np.concatenate(panel)
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in panel])]).astype(np.int64)
    m = np.ascontiguousarray(matrix)

    def call(mode=1, cut=cuts, window=windows, max_hits=-1, n=len(panel), matrix=m, queries=flat, offsets=qoff, count=len(lengths)):
        c = np.ascontiguousarray([(len(q) if w is None else w) for q, w in zip(panel, window)], dtype=np.int32)
        s = np.ascontiguousarray(cut, dtype=np.int32)
        hit_offsets = np.full(n + 1, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(4)]
        rc = lib.miopalSearchBatchOccurrences(db.handle, queries.ctypes.data, offsets.ctypes.data, n, 3, 1, matrix.ctypes.data,
                                              alphabet, mode, 0, count, s.ctypes.data, c.ctypes.data, max_hits,
                                              hit_offsets.ctypes.data, *[ctypes.byref(p) for p in ptrs])
        return rc, hit_offsets, all(p.value == 0x77 for p in ptrs)

    rc, hit_offsets, untouched = call(max_hits=total - 1)
    assert rc == TOO_MANY and np.array_equal(hit_offsets, whole["offsets"]) and untouched
    assert "maxHits" in capi.last_error()
    # NW and OV, a negative window at query 3 of 5, SW with a cut of 0 at one query: every output as it was
    for kw, code, text in ((dict(mode=0), capi.OPAL_ERR_INVALID_MODE, "OPAL_MODE_HW and OPAL_MODE_SW"),
                           (dict(mode=2), capi.OPAL_ERR_INVALID_MODE, "OPAL_MODE_HW and OPAL_MODE_SW"),
                           (dict(n=5, window=[0, 1, 2, -1, 4], cut=[1] * 5), BAD, "negative window -1 at query 3"),
                           (dict(mode=3, cut=[5, 5, 0, 5, 5, 5, 5, 5]), BAD, "at least 1")):
        rc, hit_offsets, untouched = call(**kw)
        assert rc == code and text in capi.last_error(), (kw, rc, capi.last_error())
        assert np.all(hit_offsets == -7) and untouched, kw
    # ... and the handle works afterwards
    assert_csr(db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts, window=windows), whole, "afterwards")


def test_range_check_of_one_query_refuses_the_call(capi):
    """test_range_check_is_the_plain_searchs' model (tests/test_gpu_occurrences.py): a matrix of 2^26 and a query of 70
    rows fail miopalSearch's 32-bit range check; a query of 5 rows beside it passes (6 x 2^26 < 2^29), and the whole call is refused"""
    rng = np.random.default_rng(2)
    residues, offsets = _data.random_db(rng, [50, 60])
    huge = np.full(24 * 24, 2 ** 26, dtype=np.int32)
    B62 = MATRICES["blosum62"][0]
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        short, tall = _data.random_protein(rng, 5), _data.random_protein(rng, 70)
        assert db.search_occurrences(short, huge, 3, 1, "hw", min_score=0, window=0)["count"] > 0
        with pytest.raises(OverflowError):
            db.search_occurrences(tall, huge, 3, 1, "hw", min_score=0, window=0)
        with pytest.raises(OverflowError):
            db.search_batch_occurrences([short, tall], huge, 3, 1, "hw", min_score=0, window=0)
        # the outputs of the refused call are as they were
        flat = np.concatenate([short, tall]).astype(np.uint8)
        qoff = np.array([0, 5, 75], dtype=np.int64)
        cuts, windows = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        hit_offsets = np.full(3, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(4)]
        rc = capi.lib().miopalSearchBatchOccurrences(db.handle, flat.ctypes.data, qoff.ctypes.data, 2, 3, 1, huge.ctypes.data, 24, 1,
                                                     0, 2, cuts.ctypes.data, windows.ctypes.data, -1, hit_offsets.ctypes.data,
                                                     *[ctypes.byref(p) for p in ptrs])
        assert rc == OVERFLOW == capi.OPAL_ERR_OVERFLOW
        assert np.all(hit_offsets == -7) and all(p.value == 0x77 for p in ptrs)
        got = db.search_batch_occurrences([short, tall], B62, 3, 1, "sw", min_score=1, window=0)
        assert np.all(np.diff(got["offsets"]) > 0)
    finally:
        db.close()


# ---- 5: the Python layer --------------------------------------------------------------------------------------------

def test_find_occurrences_many_equals_find_occurrences(capi):
    rng = np.random.default_rng(91)
    targets = [_data.random_protein(rng, int(n)) for n in rng.integers(0, 201, size=130)]
    panel = [_data.random_protein(rng, q) for q in PANEL]
    letters = _data.NCBI
    text = lambda codes: "".join(letters[c] for c in codes)   # noqa: E731
    aligner = pyopal_amd.Aligner("BLOSUM62", gap_open=11, gap_extend=1)
    database = pyopal_amd.Database([text(t) for t in targets])
    queries = [text(q) for q in panel]
    fields = lambda r: (type(r), r.target_index, r.score, r.target_end, r.query_end)   # noqa: E731
    for algorithm, cut in (("hw", -10), ("sw", 12)):
        for window in (None, 3):
            found = pyopal_amd.find_occurrences_many(aligner, queries, database, cut, algorithm=algorithm, window=window)
            assert len(found) == len(queries) and sum(len(f) for f in found) > 100
            for query, mine in zip(queries, found):
                alone = pyopal_amd.find_occurrences(aligner, query, database, cut, algorithm=algorithm, window=window, mode="end")
                assert [fields(r) for r in mine] == [fields(r) for r in alone], (algorithm, window, len(query))
                assert all(isinstance(r, pyopal_amd.EndResult) for r in mine)
        # one cut and one window per query, a slice, the arrays form
        cuts = [cut + k for k in range(len(queries))]
        windows = [None if k % 2 else k for k in range(len(queries))]
        arrays = pyopal_amd.find_occurrences_many_arrays(aligner, queries, database, cuts, algorithm=algorithm, window=windows,
                                                         start=20, end=90)
        assert sorted(arrays) == ["end_q", "end_t", "offsets", "score", "target"]
        for i, query in enumerate(queries):
            alone = pyopal_amd.find_occurrences_arrays(aligner, query, database, cuts[i], algorithm=algorithm, window=windows[i],
                                                       mode="end", start=20, end=90)
            lo, hi = arrays["offsets"][i], arrays["offsets"][i + 1]
            assert hi - lo == alone["count"]
            for key in KEYS:
                assert np.array_equal(arrays[key][lo:hi], alone[key]), (algorithm, i, key)
    with pytest.raises(ValueError, match="alignments of a panel.*not available yet"):
        pyopal_amd.find_occurrences_many(aligner, queries, database, 5, mode="full")
    with pytest.raises(capi.TooManyHits) as info:
        pyopal_amd.find_occurrences_many(aligner, queries, database, -10, max_hits=3)
    assert len(info.value.counts) == len(queries) + 1 and info.value.counts[-1] > 3
