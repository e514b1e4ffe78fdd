"""Every occurrence of a whole panel of position-specific scoring matrices in one call
(miopalSearchPssmBatchOccurrences; DeviceDatabase.search_batch_occurrences_pssm; pyopal_amd.find_occurrences_pssm_many).
Three witnesses, none of them the code under test: the plain panel search where the rows are a matrix's
(tests/test_gpu_batch_occurrences.py, whose shapes these are), the unchanged search_occurrences_pssm of one PSSM at a
time, and the numpy recurrence with the rule (column_values / expected_flat of tests/_occurrences.py)."""
import ctypes
import functools

import numpy as np
import pytest

import _pssm
import pyopal_amd
from _occurrences import INT_MIN, column_values, expected_flat, flat_columns
from test_gpu_batch_occurrences import (BAD, DNA, GROUPINGS, KEYS, NOWHERE, OVERFLOW, PANEL, SETS, TOO_MANY, _flatten,
                                        assert_csr, filled_groups, group, lds_bytes, panel_set)
from test_gpu_occurrences import GAPS

pytestmark = pytest.mark.gpu

NAMES = ("dna4", "random32")      # the 4-letter and the 32-letter set


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def panel_dbs(capi):
    dbs = {}
    for name in NAMES:
        residues, offsets, _, _, _ = panel_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, SETS[name][1])
    yield dbs
    for db in dbs.values():
        db.close()


def singles(db, panel, gaps, algorithm, cuts, windows, start=0, end=None):
    """the second witness: search_occurrences_pssm PSSM by PSSM, laid end to end as the CSR"""
    parts = [db.search_occurrences_pssm(rows, gaps[0], gaps[1], algorithm, start, end, min_score=int(c), window=w)
             for rows, c, w in zip(panel, cuts, windows)]
    out = {"offsets": np.concatenate([[0], np.cumsum([p["count"] for p in parts])]).astype(np.int64)}
    for key in KEYS:
        out[key] = np.concatenate([p[key] for p in parts]) if parts else np.zeros(0, dtype=np.int64 if key == "target" else np.int32)
    return out


def want_groups(grouping, alphabet):
    """what miopalLastBatchOccurrenceGroups reports for PANEL: the figures of the plain panel"""
    on_panel = [q for q in PANEL if 1 <= q <= 64]
    return [1, 8, lds_bytes(on_panel, alphabet)] if grouping == "filled" else [8, 1, lds_bytes([64], alphabet)]


def rule_of(rng, panel, algorithm):
    windows = [(0, None, 5)[k] for k in rng.integers(0, 3, size=len(panel))]
    if algorithm == "hw":
        cuts = [int(-2 * len(q) - rng.integers(0, 6)) for q in panel]
    else:
        cuts = [int(1 + rng.integers(0, 8)) for q in panel]
    cuts[NOWHERE] = 10 ** 6
    return cuts, windows


# ---- 1: rows taken from the matrix: the plain panel, byte for byte --------------------------------------------------

@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("gaps", GAPS)
def test_rows_of_the_matrix_equal_the_plain_panel(panel_dbs, tuning, gaps, name, grouping):
    group(tuning, grouping)
    matrix, alphabet = SETS[name]
    _, _, _, _, panel = panel_set(name)
    rows = [np.ascontiguousarray(matrix.reshape(alphabet, alphabet)[q]) for q in panel]
    db = panel_dbs[name]
    rng = np.random.default_rng(gaps[0] * 10 + gaps[1])
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(rng, panel, algorithm)
        context = (name, gaps, algorithm, grouping)
        want = db.search_batch_occurrences(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        plain = db.last_batch_occurrence_routing(), db.last_batch_occurrence_groups()
        got = db.search_batch_occurrences_pssm(rows, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        assert_csr(got, want, context)
        for key in ("offsets",) + KEYS:
            assert got[key].tobytes() == want[key].tobytes(), (context, key)
        assert want["offsets"][-1] > 100
        # the reporters say of this call what they say of the plain one: 8 on the panel kernels, 65 and 130 rows on
        # the single path, one chunk, the same pairs, the same groups
        assert (db.last_batch_occurrence_routing(), db.last_batch_occurrence_groups()) == plain, context
        assert plain[0][:3] == [8, 2, 1] and plain[1] == want_groups(grouping, alphabet), (context, plain)


# ---- 2: rows of their own: the singles and the recurrence ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def own_rows(name):
    """PANEL's heights with rows of their own, different from position to position and not symmetric: `class_pssm`
    over the whole alphabet where it is large (classes in random order: a row addressed by the wrong position gives a
    wrong score), independent rows at 4 letters, where four classes would repeat every few rows"""
    alphabet = SETS[name][1]
    rng = np.random.default_rng(700 + alphabet)
    if alphabet >= 24:
        return tuple(_pssm.class_pssm(rng, q, alphabet)[2] for q in PANEL)
    return tuple(np.ascontiguousarray(rng.integers(-8, 13, size=(q, alphabet)).astype(np.int32)) for q in PANEL)


@functools.lru_cache(maxsize=None)
def every_column(name, gaps, algorithm):
    """the recurrence's answer at window 0 and the lowest cut, one per PSSM of own_rows (None: the empty one); shared
    by the groupings"""
    _, _, targets, lengths, _ = panel_set(name)
    cut = INT_MIN if algorithm == "hw" else 1
    out = []
    for rows in own_rows(name):
        if len(rows) == 0:
            out.append(None)
            continue
        V, R = column_values(rows, targets, gaps[0], gaps[1], algorithm)
        flat = flat_columns([V[k, :n] for k, n in enumerate(lengths)], [R[k, :n] for k, n in enumerate(lengths)])
        out.append(expected_flat(*flat, cut, 0))
    return out


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("gaps", GAPS[:2])
def test_rows_of_their_own_equal_the_singles_and_the_recurrence(panel_dbs, tuning, gaps, name, grouping):
    """a short PSSM right behind a tall one and the reverse (64, 1, 9 .. 7, 0, 63): a wrong row origin or a pad row left
    from the PSSM before would show in the rows that follow"""
    group(tuning, grouping)
    alphabet = SETS[name][1]
    _, _, _, lengths, _ = panel_set(name)
    panel = list(own_rows(name))
    db = panel_dbs[name]
    rng = np.random.default_rng(gaps[0] * 10 + gaps[1] + 1)
    for algorithm in ("hw", "sw"):
        cuts, windows = rule_of(rng, panel, algorithm)
        if algorithm == "sw":
            cuts = [c + 6 for c in cuts]
        context = (name, gaps, algorithm, grouping)
        got = db.search_batch_occurrences_pssm(panel, gaps[0], gaps[1], algorithm, min_score=cuts, window=windows)
        routing = db.last_batch_occurrence_routing()
        assert db.last_batch_occurrence_groups() == want_groups(grouping, alphabet), context
        want = singles(db, panel, gaps, algorithm, cuts, windows)
        assert_csr(got, want, context)
        counts = np.diff(got["offsets"])
        assert counts[NOWHERE] == 0 and counts[NOWHERE - 1] > 0 and counts[NOWHERE + 1] > 0, (context, counts)
        assert counts[PANEL.index(0)] == 0 and counts[PANEL.index(130)] > 0 and counts[PANEL.index(65)] > 0, (context, counts)
        # PSSMs of 65 and 130 rows go through the single path: counts[1]
        assert routing[:3] == [8, 2, 1], (context, routing)
        pairs = sum(len(set(got["target"][got["offsets"][i]:got["offsets"][i + 1]].tolist()))
                    for i, q in enumerate(PANEL) if 1 <= q <= 64)
        assert routing[3] == pairs, (context, routing, pairs)
        # window 0 at the lowest cut: every column value (every positive column maximum under SW) of the recurrence
        cut = INT_MIN if algorithm == "hw" else 1
        every = db.search_batch_occurrences_pssm(panel, gaps[0], gaps[1], algorithm, min_score=cut, window=0)
        for i, rule in enumerate(every_column(name, gaps, algorithm)):
            lo, hi = every["offsets"][i], every["offsets"][i + 1]
            if rule is None:
                assert lo == hi
                continue
            for key in KEYS:
                assert np.array_equal(every[key][lo:hi], rule[key]), (context, i, key)
            if algorithm == "hw":
                assert hi - lo == lengths.sum()


# ---- 3: the LDS fill: groups and chunks -----------------------------------------------------------------------------

@pytest.mark.parametrize("grouping", GROUPINGS)
def test_groups_fill_the_lds_and_chunks(capi, tuning, grouping):
    """40 PSSMs of 64 rows at 32 letters, test_groups_and_chunks' shape: "filled" gives groups of 19, 19 and 2 and 160 512
    bytes, the figures the plain panel reports; then three chunks and one PSSM a chunk"""
    group(tuning, grouping)
    filled = grouping == "filled"
    alphabet = 32
    rng = np.random.default_rng(41)
    lengths = rng.integers(0, 61, size=130)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    panel = [_pssm.class_pssm(rng, 64, alphabet)[2] for _ in range(40)]
    db = capi.DeviceDatabase(residues, offsets, alphabet)
    try:
        for algorithm, cut in (("hw", -20), ("sw", 25)):
            cuts, windows = [cut] * len(panel), [None] * len(panel)
            want = singles(db, panel, (3, 1), algorithm, cuts, windows)
            assert want["offsets"][-1] > 500 and np.all(np.diff(want["offsets"]) > 0)
            got = db.search_batch_occurrences_pssm(panel, 3, 1, algorithm, min_score=cut)
            assert_csr(got, want, (algorithm, "one chunk"))
            assert db.last_batch_occurrence_routing()[:3] == [40, 0, 1]
            assert [len(g) for g in filled_groups([64] * 40, 32)] == [19, 19, 2] and lds_bytes([64] * 19, 32) == 160512
            assert db.last_batch_occurrence_groups() == ([3, 19, 160512] if filled else [40, 1, lds_bytes([64], 32)])
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", str(14 * 130))
            got = db.search_batch_occurrences_pssm(panel, 3, 1, algorithm, min_score=cut)
            assert_csr(got, want, (algorithm, "three chunks"))
            assert db.last_batch_occurrence_routing()[:3] == [40, 0, 3]
            assert db.last_batch_occurrence_groups() == ([3, 14, lds_bytes([64] * 14, 32)] if filled else [40, 1, lds_bytes([64], 32)])
            tuning.setenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES", "100")
            got = db.search_batch_occurrences_pssm(panel[:5], 3, 1, algorithm, min_score=cut)
            assert_csr(got, singles(db, panel[:5], (3, 1), algorithm, cuts[:5], windows[:5]), (algorithm, "five chunks"))
            assert db.last_batch_occurrence_routing()[:3] == [5, 0, 5]
            tuning.delenv("MIOPAL_BATCH_OCCURRENCE_ENTRIES")
    finally:
        db.close()


# ---- 4: the write pass sweeps the pairs that have occurrences, and no others ------------------------------------------

def test_sparse_write(capi):
    """test_sparse_write of the plain panel with each query as its PSSM: 14 planted sites in 12 (PSSM, read) pairs"""
    rng = np.random.default_rng(53)
    lengths = rng.integers(80, 151, size=300)
    reads = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lengths]
    motifs = [rng.integers(0, 4, size=20).astype(np.uint8) for _ in range(5)]
    planted = set()       # (PSSM, read, end column)
    for k, read in enumerate(range(10, 101, 10)):
        for at in ((5, 50) if k < 2 else (int(rng.integers(0, lengths[read] - 20)),)):
            reads[read][at:at + 20] = motifs[0]
            planted.add((0, read, at + 19))
    for read in (0, 299):
        reads[read][30:50] = motifs[1]
        planted.add((1, read, 49))
    residues, offsets = _flatten(reads)
    panel = [np.ascontiguousarray(DNA.reshape(4, 4)[m]) for m in motifs]
    cut = 100       # twenty matches: only an exact copy reaches it
    db = capi.DeviceDatabase(residues, offsets, 4)
    try:
        want = singles(db, panel, (3, 1), "hw", [cut] * 5, [None] * 5)
        seen = {(i, int(t), int(j)) for i in range(5)
                for t, j in zip(want["target"][want["offsets"][i]:want["offsets"][i + 1]],
                                want["end_t"][want["offsets"][i]:want["offsets"][i + 1]])}
        assert seen == planted and len(planted) == 14 and np.all(want["score"] == cut)
        got = db.search_batch_occurrences_pssm(panel, 3, 1, "hw", min_score=cut)
        assert_csr(got, want, "sparse")
        assert got["offsets"].tolist() == [0, 12, 14, 14, 14, 14]
        assert len({(i, t) for i, t, _ in planted}) == 12
        assert db.last_batch_occurrence_routing() == [5, 0, 1, 12]
    finally:
        db.close()


# ---- 5: the contract ------------------------------------------------------------------------------------------------

def test_contract(capi, panel_dbs):
    name = "random32"
    alphabet = SETS[name][1]
    _, _, _, lengths, _ = panel_set(name)
    db = panel_dbs[name]
    panel = list(own_rows(name))[:8]          # 64, 1, 9, 8, 7, 0, 63, 24
    cuts, windows = [0, 5, 10, 10, 10, 0, 0, 20], [None, 0, 5, None, 0, 3, None, 5]
    rule = dict(min_score=cuts, window=windows)
    whole = db.search_batch_occurrences_pssm(panel, 3, 1, "hw", **rule)
    total = int(whole["offsets"][-1])
    assert total > 100
    again = db.search_batch_occurrences_pssm(panel, 3, 1, "hw", **rule)
    for key in ("offsets",) + KEYS:
        assert again[key].tobytes() == whole[key].tobytes(), key
    # a slice returns absolute indices, and what the singles return for it
    start, end = 37, 101
    part = db.search_batch_occurrences_pssm(panel, 3, 1, "hw", start, end, **rule)
    assert_csr(part, singles(db, panel, (3, 1), "hw", cuts, windows, start, end), "slice")
    assert part["offsets"][-1] > 0 and part["target"].min() >= start and part["target"].max() < end
    # max_hits below the total: TooManyHits with the offsets; at the total and above it: the answer
    with pytest.raises(capi.TooManyHits) as info:
        db.search_batch_occurrences_pssm(panel, 3, 1, "hw", max_hits=total - 1, **rule)
    assert np.array_equal(info.value.counts, whole["offsets"])
    for bound in (total, total + 1):
        assert_csr(db.search_batch_occurrences_pssm(panel, 3, 1, "hw", max_hits=bound, **rule), whole, bound)
    # no PSSMs, an empty slice, nothing but empty PSSMs: answered, nothing launched
    got = db.search_batch_occurrences_pssm([], 3, 1, "hw")
    assert got["offsets"].tolist() == [0] and all(len(got[key]) == 0 for key in KEYS)
    assert db.last_batch_occurrence_routing() == [0, 0, 0, 0]
    got = db.search_batch_occurrences_pssm(panel, 3, 1, "hw", 40, 40, **rule)
    assert got["offsets"].tolist() == [0] * (len(panel) + 1) and all(len(got[key]) == 0 for key in KEYS)
    assert db.last_batch_occurrence_routing() == [0, 0, 0, 0]
    nothing = np.zeros((0, alphabet), dtype=np.int32)
    got = db.search_batch_occurrences_pssm([nothing, nothing], 3, 1, "hw", min_score=0)
    assert got["offsets"].tolist() == [0, 0, 0] and db.last_batch_occurrence_routing()[2:] == [0, 0]

    # the C ABI: what a refused call leaves of its outputs
    lib = capi.lib()
    rng = np.random.default_rng(8)
    too_tall = rng.integers(-3, 4, size=(494, alphabet)).astype(np.int32)

    def call(rows, cut, window, mode=1, max_hits=-1):
        flat = np.ascontiguousarray(np.concatenate(rows))
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        w = np.ascontiguousarray([(len(r) if x is None else x) for r, x in zip(rows, window)], dtype=np.int32)
        s = np.ascontiguousarray(cut, dtype=np.int32)
        hit_offsets = np.full(len(rows) + 1, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(4)]
        rc = lib.miopalSearchPssmBatchOccurrences(db.handle, flat.ctypes.data, off.ctypes.data, len(rows), 3, 1, alphabet, mode, 0,
                                                  len(lengths), s.ctypes.data, w.ctypes.data, max_hits, hit_offsets.ctypes.data,
                                                  *[ctypes.byref(p) for p in ptrs])
        return rc, hit_offsets, all(p.value == 0x77 for p in ptrs)

    rc, hit_offsets, untouched = call(panel, cuts, windows, max_hits=total - 1)
    assert rc == TOO_MANY and np.array_equal(hit_offsets, whole["offsets"]) and untouched
    assert "maxHits" in capi.last_error()
    # one PSSM of 494 rows at 32 letters among the others: the whole call, nothing launched
    rc, hit_offsets, untouched = call(panel[:3] + [too_tall] + panel[3:], cuts[:3] + [0] + cuts[3:], windows[:3] + [0] + windows[3:])
    assert rc == BAD and "PSSM 3 of the panel: a PSSM of 494 rows at 32 letters" in capi.last_error(), capi.last_error()
    assert np.all(hit_offsets == -7) and untouched
    assert db.last_batch_occurrence_routing() == [0, 0, 0, 0] and db.last_batch_occurrence_groups() == [0, 0, 0]
    with pytest.raises(RuntimeError, match="494 rows"):
        db.search_batch_occurrences_pssm(panel[:3] + [too_tall], 3, 1, "hw", min_score=0)
    for kw, code, text in ((dict(mode=0), capi.OPAL_ERR_INVALID_MODE, "OPAL_MODE_HW and OPAL_MODE_SW"),
                           (dict(mode=3, cut=[5, 5, 0, 5, 5, 5, 5, 5]), BAD, "at least 1")):
        rc, hit_offsets, untouched = call(panel, kw.get("cut", cuts), windows, mode=kw["mode"])
        assert rc == code and text in capi.last_error(), (kw, rc, capi.last_error())
        assert np.all(hit_offsets == -7) and untouched, kw
    # 493 rows are served, through the single path; and the handle works afterwards
    fits = db.search_batch_occurrences_pssm(panel[:2] + [too_tall[:493]], 3, 1, "sw", min_score=1, window=0)
    assert db.last_batch_occurrence_routing()[:2] == [2, 1] and np.all(np.diff(fits["offsets"]) > 0)
    assert_csr(db.search_batch_occurrences_pssm(panel, 3, 1, "hw", **rule), whole, "afterwards")


def test_range_check_of_one_pssm_refuses_the_call(capi):
    """rows of 2^26 and 70 of them fail miopalSearch's 32-bit range check; 5 rows pass (6 x 2^26 < 2^29). Each PSSM is
    checked with the extreme entries of its own rows: modest rows beside the huge ones do not rescue the call, and the
    huge entries of a short PSSM do not condemn a tall one"""
    rng = np.random.default_rng(2)
    residues, offsets = _pssm.random_db(rng, [50, 60], 24)
    db = capi.DeviceDatabase(residues, offsets, 24)
    try:
        short, tall = np.full((5, 24), 2 ** 26, dtype=np.int32), np.full((70, 24), 2 ** 26, dtype=np.int32)
        modest = rng.integers(-4, 9, size=(70, 24)).astype(np.int32)
        assert db.search_occurrences_pssm(short, 3, 1, "hw", min_score=0, window=0)["count"] > 0
        with pytest.raises(OverflowError):
            db.search_occurrences_pssm(tall, 3, 1, "hw", min_score=0, window=0)
        with pytest.raises(OverflowError):
            db.search_batch_occurrences_pssm([short, modest, tall], 3, 1, "hw", min_score=0, window=0)
        flat = np.ascontiguousarray(np.concatenate([short, tall]))
        off = np.array([0, 5, 75], dtype=np.int64)
        cuts, windows = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
        hit_offsets = np.full(3, -7, dtype=np.int64)
        ptrs = [ctypes.c_void_p(0x77) for _ in range(4)]
        rc = capi.lib().miopalSearchPssmBatchOccurrences(db.handle, flat.ctypes.data, off.ctypes.data, 2, 3, 1, 24, 1, 0, 2,
                                                         cuts.ctypes.data, windows.ctypes.data, -1, hit_offsets.ctypes.data,
                                                         *[ctypes.byref(p) for p in ptrs])
        assert rc == OVERFLOW == capi.OPAL_ERR_OVERFLOW
        assert np.all(hit_offsets == -7) and all(p.value == 0x77 for p in ptrs)
        got = db.search_batch_occurrences_pssm([short, modest], 3, 1, "hw", min_score=0, window=0)
        assert_csr(got, singles(db, [short, modest], (3, 1), "hw", [0, 0], [0, 0]), "own extremes")
        assert np.all(np.diff(got["offsets"]) > 0)
    finally:
        db.close()


# ---- 6: the Python layer --------------------------------------------------------------------------------------------

def test_find_occurrences_pssm_many_equals_find_occurrences_pssm(capi):
    """a motif library on both strands: each PSSM beside its reverse complement"""
    rng = np.random.default_rng(91)
    letters = "ACGT"
    text = lambda codes: "".join(letters[c] for c in codes)   # noqa: E731
    reads = [rng.integers(0, 4, size=int(n)) for n in rng.integers(0, 201, size=130)]
    aligner = pyopal_amd.Aligner(pyopal_amd.ScoringMatrix.from_match_mismatch(5, -4), gap_open=3, gap_extend=1)
    database = pyopal_amd.Database([text(r) for r in reads], pyopal_amd.Alphabet(letters))
    forward = [pyopal_amd.Pssm(rng.integers(-6, 7, size=(q, 4)), letters) for q in (6, 20, 11, 0, 64, 70)]
    pssms = [p for f in forward for p in (f, f.reverse_complement())]
    fields = lambda r: (type(r), r.target_index, r.score, r.target_end, r.query_end)   # noqa: E731
    for algorithm, cut in (("hw", 8), ("sw", 14)):
        found = pyopal_amd.find_occurrences_pssm_many(aligner, pssms, database, cut, algorithm=algorithm)
        assert len(found) == len(pssms) and sum(len(f) for f in found) > 100
        for pssm, mine in zip(pssms, found):
            alone = pyopal_amd.find_occurrences_pssm(aligner, pssm, database, cut, algorithm=algorithm, mode="end")
            assert [fields(r) for r in mine] == [fields(r) for r in alone], (algorithm, len(pssm))
            assert all(isinstance(r, pyopal_amd.EndResult) for r in mine)
        cuts = [cut + k for k in range(len(pssms))]
        windows = [None if k % 2 else k for k in range(len(pssms))]
        arrays = pyopal_amd.find_occurrences_pssm_many_arrays(aligner, pssms, database, cuts, algorithm=algorithm,
                                                              window=windows, start=20, end=90)
        assert sorted(arrays) == ["end_q", "end_t", "offsets", "score", "target"]
        for i, pssm in enumerate(pssms):
            db = database._device_mirror(0)
            alone = db.search_occurrences_pssm(pssm.scores, 3, 1, algorithm, 20, 90, min_score=cuts[i], window=windows[i])
            lo, hi = arrays["offsets"][i], arrays["offsets"][i + 1]
            assert hi - lo == alone["count"]
            for key in KEYS:
                assert np.array_equal(arrays[key][lo:hi], alone[key]), (algorithm, i, key)
    with pytest.raises(capi.TooManyHits) as info:
        pyopal_amd.find_occurrences_pssm_many(aligner, pssms, database, 8, max_hits=3)
    assert len(info.value.counts) == len(pssms) + 1 and info.value.counts[-1] > 3
