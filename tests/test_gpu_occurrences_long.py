"""The occurrence searches at read length and across the seams of their chunks: one query (miopalSearchOccurrences,
plain and PSSM), a panel (miopalSearchBatchOccurrences) and the aligned form (miopalSearchOccurrencesAligned) on targets
of 3000 to 352 000 residues, where the other occurrence tests stop at 300.

What runs here and nowhere else in the suite: the sweep kernel's walk to a wavefront's longest length with strip
boundaries, running maxima and their rows handed through memory over thousands of columns; the second and third chunk of
occurrenceSweep (host_occurrences.inc), counting and writing; and the alignment stage with fewer than 64 occurrences a
chunk, which takes a wavefront per occurrence whatever the switches say.

Witnesses, none of them device code: tests/_occurrences.row_values - the recurrence row by row, held to column_values
and to the C checker in tests/test_occurrences_cpu.py - for every column of a long target, column_values for the short
ones, `pick` for the rule, the C checker for the alignment of a target's best occurrence and
tests/_occurrence_alignments.py for a handful of others. Every comparison is exact and covers every element. Gap models
have open >= extend throughout, where row_values is valid.

Durations on an MI355X: profiles/occurrences_long_reads.txt."""
import functools

import numpy as np
import pytest

import _oracle
import _pssm
from _occurrence_alignments import operations, starts
from _occurrences import column_values, expected_flat, flat_columns, row_values
from test_gpu_batch_occurrences import GROUPINGS, assert_csr, group, singles
from test_gpu_cases import every_routing, routed   # noqa: F401 (routed: the fixture every_routing parametrises)
from test_gpu_occurrences import B62, GAPS, MATRICES, assert_answer

pytestmark = pytest.mark.gpu

KEYS = ("target", "score", "end_t", "end_q")
LOWEST = -10 ** 6                        # below every HW value of these tests: window 0 returns every column
QUERY_LENGTHS = (7, 64, 65, 130)         # one strip, its edge, two strips, three strips
PANEL = (1, 9, 24, 63, 64, 130)          # five queries of the panel kernels; 130 rows take the single-query path
SETTINGS = [(name, gaps) for name in MATRICES for gaps in GAPS]
by_setting = pytest.mark.parametrize("name,gaps", SETTINGS, ids=[f"{n}-{g[0]}-{g[1]}" for n, g in SETTINGS])
LANES = 64
MATCH = 0


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def lowest_cut(algorithm):
    return LOWEST if algorithm == "hw" else 1


def query_of(name, q):
    return np.random.default_rng(3000 + q).integers(0, MATRICES[name][1], size=q).astype(np.uint8)


def rows_of(name, q):
    matrix, alphabet = MATRICES[name]
    return np.ascontiguousarray(matrix.reshape(alphabet, alphabet)[query_of(name, q)])


def forms_of(db, name, q, gaps):
    """the plain and the PSSM form of one search, as callables of the rule"""
    matrix = MATRICES[name][0]
    query, rows = query_of(name, q), rows_of(name, q)
    return {"plain": lambda **rule: db.search_occurrences(query, matrix, gaps[0], gaps[1], **rule),
            "pssm": lambda **rule: db.search_occurrences_pssm(rows, gaps[0], gaps[1], **rule)}


# ---- a: the long-read database ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_set(name):
    """141 targets, shuffled: 70 of 3000 .. 6000 residues (a full wavefront of long lanes with ragged ends and a part
    of a second), one of 20 000, and 70 of 0 .. 200 with 0 and 1 among them. Three of the long ones are written in two
    letters: there a column's maximum is reached in several strips. -> residues, offsets, targets, lengths, low"""
    alphabet = MATRICES[name][1]
    rng = np.random.default_rng(500 + alphabet)
    long_lengths = rng.integers(3000, 6001, size=70)
    long_lengths[:2] = (3000, 6000)
    short_lengths = rng.integers(0, 201, size=70)
    short_lengths[:4] = (0, 1, 200, 0)
    lengths = np.concatenate([long_lengths, [20000], short_lengths])
    rng.shuffle(lengths)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    mid = np.flatnonzero((lengths >= 3000) & (lengths < 20000))
    low = [int(mid[0]), int(mid[31]), int(mid[69])]
    for k, letters in zip(low, ((0, 1), (5, 11), (2, 3))):
        residues[offsets[k]:offsets[k + 1]] = np.array(letters, dtype=np.uint8)[rng.integers(0, 2, size=lengths[k])]
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    return residues, offsets, targets, lengths, low


def long_ids(name):
    return np.flatnonzero(long_set(name)[3] >= 3000)


def columns_of(name, q, gaps, algorithm):
    """every column of every target of `long_set`: row_values per long target, column_values on the short ones ->
    (V, R, offsets, ties): flat_columns' row, and how many columns of the two-letter targets hold their maximum in
    several strips"""
    _, _, targets, lengths, low = long_set(name)
    rows = rows_of(name, q)
    short = np.flatnonzero(lengths <= 200)
    Vs, Rs = column_values(rows, [targets[k] for k in short], gaps[0], gaps[1], algorithm)
    values, at_row = [None] * len(lengths), [None] * len(lengths)
    for i, k in enumerate(short):
        values[k], at_row[k] = Vs[i, :lengths[k]], Rs[i, :lengths[k]]
    ties = 0
    for k in long_ids(name):
        tied = np.zeros(lengths[k], dtype=bool)
        values[k], at_row[k] = row_values(rows, targets[k], gaps[0], gaps[1], algorithm, tied=tied)
        ties += int(tied.sum()) if k in low else 0
    V, R, offsets = flat_columns(values, at_row)
    return V.astype(np.int32), R.astype(np.int32), offsets, ties


witness = functools.lru_cache(maxsize=None)(columns_of)   # (the queries that several tests share; computed once, never written to)


def median_cut(V, algorithm):
    """the cut of the windowed picks: the median of the positive values - of all values where none is positive, as
    under "hw" with a query of more than a few rows against random residues"""
    pool = V[V > 0] if (V > 0).any() else V
    return max(int(np.median(pool)), lowest_cut(algorithm))


@pytest.fixture(scope="module")
def long_dbs(capi):
    dbs = {}
    for name, (matrix, alphabet) in MATRICES.items():
        residues, offsets, _, _, _ = long_set(name)
        dbs[name] = capi.DeviceDatabase(residues, offsets, alphabet)
    yield dbs
    for db in dbs.values():
        db.close()


@by_setting
@pytest.mark.parametrize("q", QUERY_LENGTHS)
def test_every_column_of_long_targets(long_dbs, q, name, gaps):
    """window 0 at the lowest cut: all 357 000-odd columns ("sw": every positive column maximum and its smallest row)
    equal the recurrence's, plain and PSSM; then the picker with window = Q over the same columns, on the whole
    database and on a slice that leaves part of the long targets out"""
    _, _, _, lengths, _ = long_set(name)
    db = long_dbs[name]
    first, last = 41, 118
    inside = np.count_nonzero(lengths[first:last] >= 3000)
    assert 0 < inside < LANES < len(long_ids(name))   # (the slice's long lanes share their wavefront with short ones)
    for algorithm in ("hw", "sw"):
        V, R, offsets, ties = witness(name, q, gaps, algorithm)
        if algorithm == "sw" and q > LANES:
            assert ties > 0, (name, q, gaps)   # the upper strip has ties to win
        cut = lowest_cut(algorithm)
        every = expected_flat(V, R, offsets, cut, 0)
        picked_cut = median_cut(V, algorithm)
        picked = expected_flat(V, R, offsets, picked_cut, q)
        part = expected_flat(V, R, offsets, picked_cut, q, first, last)
        assert 0 < len(part["target"]) < len(picked["target"]) < len(every["target"])
        for form, call in forms_of(db, name, q, gaps).items():
            context = (form, algorithm, q, gaps, name)
            got = call(algorithm=algorithm, min_score=cut, window=0)
            assert_answer(got, every, context)
            if algorithm == "hw":
                assert got["count"] == lengths.sum() and np.all(got["end_q"] == q - 1)
            assert db.last_occurrence_routing() == [len(lengths), len(set(every["target"].tolist())), 2, (q + 63) // 64], context
            assert_answer(call(algorithm=algorithm, min_score=picked_cut, window=q), picked, context + ("window",))
            assert_answer(call(algorithm=algorithm, start=first, end=last, min_score=picked_cut, window=q), part, context + ("slice",))
            assert db.last_occurrence_routing()[0] == last - first


# ---- b: the chunk seams of the sweeps ---------------------------------------------------------------------------------

STRIP_BYTES = 2 << 30                    # the strip workspace of a query of more than 64 rows (kOccurrenceStripBytes)
COLUMN_BYTES = {"hw": 8, "sw": 16}       # per column and lane: the boundary row; under SW the running maximum beside it
SEAM_Q, SEAM_TARGETS, SEAM_LONGEST, SEAM_LONG_AT = 65, 13500, 20000, 13400


def chunk_capacity(algorithm, longest):
    """targets a chunk of occurrenceSweep holds when the query has more than 64 rows (occurrenceChunkCapacity): whole
    wavefronts whose boundary rows, `longest` columns each, fit the strip workspace"""
    return STRIP_BYTES // (COLUMN_BYTES[algorithm] * longest) // LANES * LANES


@functools.lru_cache(maxsize=None)
def seam_set(name):
    """13 500 targets: one of 20 000 residues at index 13 400, the others 150 distinct sequences of 0 .. 60 residues
    repeated in shuffled order - the empty one at some 40 places, the two sides of every seam among them
    -> residues, offsets, distinct, which (the distinct sequence of each target; -1: the long one), long"""
    alphabet = MATRICES[name][1]
    rng = np.random.default_rng(700 + alphabet)
    distinct = [rng.integers(0, alphabet, size=n).astype(np.uint8) for n in [0, 1, 60] + rng.integers(1, 61, size=147).tolist()]
    which = rng.integers(1, len(distinct), size=SEAM_TARGETS)
    which[rng.choice(SEAM_TARGETS, size=34, replace=False)] = 0
    which[[6655, 6657, 13311, 13312, 13375, 13377]] = 0
    long = rng.integers(0, alphabet, size=SEAM_LONGEST).astype(np.uint8)
    which[SEAM_LONG_AT] = -1
    residues, offsets = _oracle.flatten([long if w < 0 else distinct[w] for w in which])
    return residues, offsets, distinct, which, long


@functools.lru_cache(maxsize=None)
def seam_witness(name, gaps, algorithm):
    """the recurrence on the 150 distinct sequences and the long one, gathered into the 13 500 targets"""
    _, _, distinct, which, long = seam_set(name)
    rows = rows_of(name, SEAM_Q)
    Vs, Rs = column_values(rows, distinct, gaps[0], gaps[1], algorithm)
    v, r = row_values(rows, long, gaps[0], gaps[1], algorithm)
    values = [v if w < 0 else Vs[w, :len(distinct[w])] for w in which]
    at_row = [r if w < 0 else Rs[w, :len(distinct[w])] for w in which]
    best = np.array([Vs[w, :len(d)].max() for w, d in enumerate(distinct) if len(d)])
    return flat_columns(values, at_row) + (best,)


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
@pytest.mark.parametrize("name,gaps", [("blosum62", (11, 1)), ("random32", (3, 1)), ("blosum62", (2, 2))])
def test_chunk_seams_of_the_sweeps(capi, name, gaps, algorithm):
    """Q = 65, the shortest query with strip workspace, and a longest target of 20 000 residues: a chunk holds 13 376
    targets under HW and 6656 under SW, so 13 500 targets are two count chunks under HW and three under SW, with the
    long target in the last. At the lowest cut (nearly) every target is listed and the write sweep is chunked too; at
    a high cut one write chunk takes a list that spans the count chunks."""
    n = SEAM_TARGETS
    cap = chunk_capacity(algorithm, SEAM_LONGEST)
    assert cap == {"hw": 13376, "sw": 6656}[algorithm] and (n - 1) // cap == SEAM_LONG_AT // cap == {"hw": 1, "sw": 2}[algorithm]
    residues, offsets, _, which, _ = seam_set(name)
    V, R, flat_offsets, best = seam_witness(name, gaps, algorithm)
    assert np.array_equal(flat_offsets, offsets)
    high = max(int(np.percentile(best, 60)), lowest_cut(algorithm))
    maxima = np.array([V[offsets[k]:offsets[k + 1]].max(initial=LOWEST - 1) for k in range(n)])
    db = capi.DeviceDatabase(residues, offsets, MATRICES[name][1])
    try:
        for cut, window in ((lowest_cut(algorithm), 0), (high, 10)):
            want = expected_flat(V, R, flat_offsets, cut, window)
            has = maxima >= cut
            listed = int(has.sum())
            assert listed == len(set(want["target"].tolist())) and has[SEAM_LONG_AT]
            for seam in range(cap, n, cap):
                # targets with occurrences and targets without, on both sides of every seam of the count sweep
                for side in (has[seam - 32:seam], has[seam:seam + 32]):
                    assert side.any() and not side.all(), (algorithm, cut, seam)
            if window == 0:
                assert listed > cap                  # the write sweep has a second chunk
            else:
                assert listed <= cap and has[:cap].any() and has[cap:].any()   # one write chunk, its list from every count chunk
            for form, call in forms_of(db, name, SEAM_Q, gaps).items():
                context = (form, algorithm, name, gaps, cut, window)
                got = call(algorithm=algorithm, min_score=cut, window=window)
                assert_answer(got, want, context)
                assert db.last_occurrence_routing() == [n, listed, -(-n // cap) + -(-listed // cap), 2], context
    finally:
        db.close()


# ---- c: the panel on long targets -------------------------------------------------------------------------------------

@by_setting
def test_panel_on_long_targets(long_dbs, tuning, name, gaps):
    """queries of 1, 9, 24, 63, 64 and 130 rows against the long-read database in one call, under both groupings of
    the count sweep: the CSR is the recurrence's with the rule, query by query - every column at window 0, and the
    picker with each query's own window and cut; the singles agree (a second check: they are the code of the test above).
    Measured: 3.9 to 4.2 s a case on an MI355X, four panel calls and six singles per algorithm, witnesses included."""
    matrix = MATRICES[name][0]
    db = long_dbs[name]
    panel = [query_of(name, q) for q in PANEL]
    for algorithm in ("hw", "sw"):
        columns = [witness(name, q, gaps, algorithm) if q in QUERY_LENGTHS else columns_of(name, q, gaps, algorithm) for q in PANEL]
        cuts = [median_cut(V, algorithm) for V, _, _, _ in columns]
        for cut, window in ((lowest_cut(algorithm), 0), (cuts, None)):
            per_query = [expected_flat(V, R, offsets, cut if window == 0 else cuts[i], 0 if window == 0 else PANEL[i])
                         for i, (V, R, offsets, _) in enumerate(columns)]
            want = {key: np.concatenate([p[key] for p in per_query]) for key in KEYS}
            want["offsets"] = np.concatenate([[0], np.cumsum([len(p["target"]) for p in per_query])]).astype(np.int64)
            assert np.all(np.diff(want["offsets"]) > 0)
            for grouping in GROUPINGS:
                group(tuning, grouping)
                got = db.search_batch_occurrences(panel, matrix, gaps[0], gaps[1], algorithm, min_score=cut, window=window)
                assert_csr(got, want, (name, gaps, algorithm, window, grouping))
                assert db.last_batch_occurrence_routing()[:3] == [5, 1, 1], (grouping, db.last_batch_occurrence_routing())
        group(tuning, GROUPINGS[0])
        windows = [None] * len(PANEL)
        assert_csr(singles(db, panel, matrix, gaps, algorithm, cuts, windows), want, (name, gaps, algorithm, "singles"))


# ---- d: aligned occurrences in long targets ---------------------------------------------------------------------------

ALIGN_WINDOW = 2000      # a handful of occurrences per long target, ten at most in the longest
ALIGN_SETTINGS = [("blosum62", (11, 1)), ("random32", (3, 1)), ("blosum62", (2, 2))]


@functools.lru_cache(maxsize=None)
def aligned_witness(name, q, gaps, algorithm):
    """The cut is the lowest of the long targets' best values, so that each of them holds its best occurrence.
    -> (cut, the first five arrays, the checker's `full` answer for the long targets, {occurrence: (start_t, start_q,
    operations)} for a handful of the others)"""
    matrix = MATRICES[name][0]
    _, _, targets, lengths, _ = long_set(name)
    V, R, offsets, _ = witness(name, q, gaps, algorithm)
    ids = long_ids(name)
    cut = max(min(int(V[offsets[k]:offsets[k + 1]].max()) for k in ids), lowest_cut(algorithm))
    want = expected_flat(V, R, offsets, cut, ALIGN_WINDOW)
    residues, long_offsets = _oracle.flatten([targets[k] for k in ids])
    full = _oracle.search(query_of(name, q), residues, long_offsets, matrix, gaps[0], gaps[1], "full", algorithm)
    occ = list(zip(*(want[key].tolist() for key in KEYS)))
    best = {int(k): (int(full["end_t"][i]), int(full["end_q"][i])) for i, k in enumerate(ids)}
    others = [i for i, (t, _, j, r) in enumerate(occ) if best.get(t, (j, r)) != (j, r)]
    others.sort(key=lambda i: -occ[i][2])
    chosen = sorted(others[:1] + others[1::max(1, len(others) // 7)][:7])   # the one that ends last, and seven across the rest
    few = [occ[i] for i in chosen]
    start_t, start_q = starts(rows_of(name, q), targets, few, gaps[0], gaps[1], algorithm)
    ops = operations(query_of(name, q), matrix, targets, few, start_t, start_q, gaps[0], gaps[1])
    helper = {i: (int(start_t[k]), int(start_q[k]), ops[k]) for k, i in enumerate(chosen)}
    return cut, want, full, helper


@every_routing
@pytest.mark.parametrize("algorithm", ["hw", "sw"])
@pytest.mark.parametrize("q", [65, 130])
@pytest.mark.parametrize("name,gaps", ALIGN_SETTINGS)
def test_aligned_occurrences_in_long_targets(long_dbs, routed, name, gaps, q, algorithm):
    """window 2000 at the lowest of the long targets' best values: one to ten occurrences in each long target, some
    of them ending beyond column 15 000. The first five arrays are the recurrence's; the best occurrence of every long
    target carries the C checker's start and operations (the anchor property of include/miopal.h); eight others the
    helper's; plain and PSSM, under the three routings of the alignment stage"""
    matrix = MATRICES[name][0]
    db = long_dbs[name]
    query, rows = query_of(name, q), rows_of(name, q)
    cut, want, full, helper = aligned_witness(name, q, gaps, algorithm)
    ids = long_ids(name)
    in_long = np.isin(want["target"], ids)
    assert len(ids) <= in_long.sum() < 400 and (want["end_t"] > 15000).any() and len(helper) == 8
    assert max(want["end_t"][i] for i in helper) > 15000
    where = {(int(t), int(j), int(r)): i for i, (t, j, r) in enumerate(zip(want["target"], want["end_t"], want["end_q"]))}
    forms = {"plain": lambda: db.search_occurrence_alignments(query, matrix, gaps[0], gaps[1], algorithm, min_score=cut, window=ALIGN_WINDOW),
             "pssm": lambda: db.search_occurrence_alignments_pssm(rows, query, gaps[0], gaps[1], algorithm, min_score=cut, window=ALIGN_WINDOW)}
    for form, call in forms.items():
        context = (form, routed, algorithm, q, name, gaps)
        got = call()
        assert_answer(got, want, context)
        for i, k in enumerate(ids):
            at = where[(int(k), int(full["end_t"][i]), int(full["end_q"][i]))]
            assert got["score"][at] == full["score"][i], (context, k)
            assert (got["start_t"][at], got["start_q"][at]) == (full["start_t"][i], full["start_q"][i]), (context, k)
            assert np.array_equal(got["aln"][at], full["aln"][i]), (context, k)
        for at, (start_t, start_q, ops) in helper.items():
            assert (got["start_t"][at], got["start_q"][at]) == (start_t, start_q), (context, at)
            assert np.array_equal(got["aln"][at], ops), (context, at)
        off = got["aln_off"]
        assert off.dtype == np.int64 and len(off) == got["count"] + 1 and off[0] == 0 and off[-1] == len(got["aln_flat"])
        routing = db.last_occurrence_align_routing()
        assert routing[0] + routing[1] == got["count"] and routing[2] >= 1, (context, routing)
        assert routing[3] == (got["end_t"] - got["start_t"] + 1).max(), (context, routing)
        if routed == "lanes":
            assert routing[0] > 0, (context, routing)
        elif routed == "waves":
            assert routing[0] == 0, (context, routing)


# ---- e: the wave-only alignment stage ---------------------------------------------------------------------------------

DIR_BUDGET = 2 << 30     # direction workspace of the later passes (full_plan.h, kDirBudget); a chunk may take twice that
DEEP_Q, DEEP_LONGEST = 130, 352000
DEEP_PLANTS = (101_000, 203_517, 299_870)
DEEP_AT = 31             # the long target's index


def align_capacity(q, longest):
    """occurrences a chunk of the alignment stage holds with operations (pairChunkCapacity): the direction slots,
    strips x (longest + 63) x 64 bytes each, within 2 x DIR_BUDGET (its other two bounds are far above that here)"""
    strips = (q + LANES - 1) // LANES
    return 2 * DIR_BUDGET // (strips * (longest + LANES - 1) * LANES)


@functools.lru_cache(maxsize=None)
def deep_set():
    """one random target of 352 000 residues with three exact copies of a 130-residue query planted deep inside, and 60
    targets of at most 300 residues, four of which hold a copy too -> query, residues, offsets, targets, ends [(target, column)]"""
    rng = np.random.default_rng(900)
    query = rng.integers(0, 20, size=DEEP_Q).astype(np.uint8)
    long = rng.integers(0, 20, size=DEEP_LONGEST).astype(np.uint8)
    for at in DEEP_PLANTS:
        long[at:at + DEEP_Q] = query
    targets = [rng.integers(0, 20, size=int(n)).astype(np.uint8) for n in rng.integers(0, 201, size=60)]
    copies = ((7, 0, 40), (19, 33, 0), (20, 90, 80), (55, 71, 1))   # (target, residues in front of the copy, behind it)
    for k, front, behind in copies:
        targets[k] = np.concatenate([rng.integers(0, 20, size=front), query, rng.integers(0, 20, size=behind)]).astype(np.uint8)
    targets.insert(DEEP_AT, long)   # (the targets behind it move up by one)
    ends = [(k + (k >= DEEP_AT), front + DEEP_Q - 1) for k, front, _ in copies] + [(DEEP_AT, at + DEEP_Q - 1) for at in DEEP_PLANTS]
    ends.sort()
    residues, offsets = _oracle.flatten(targets)
    return query, residues, offsets, targets, ends


@functools.lru_cache(maxsize=None)
def deep_witness(algorithm):
    query, _, _, targets, _ = deep_set()
    rows = B62.reshape(24, 24)[query]
    short = [k for k in range(len(targets)) if k != DEEP_AT]
    Vs, Rs = column_values(rows, [targets[k] for k in short], 11, 1, algorithm)
    values, at_row = [None] * len(targets), [None] * len(targets)
    for i, k in enumerate(short):
        values[k], at_row[k] = Vs[i, :len(targets[k])], Rs[i, :len(targets[k])]
    values[DEEP_AT], at_row[DEEP_AT] = row_values(rows, targets[DEEP_AT], 11, 1, algorithm)
    return flat_columns(values, at_row)


@pytest.fixture(scope="module")
def deep_db(capi):
    _, residues, offsets, _, _ = deep_set()
    db = capi.DeviceDatabase(residues, offsets, 24)
    yield db
    db.close()


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_wave_only_alignment_stage(deep_db, tuning, algorithm):
    """A chunk of the alignment stage holds 2^32 / (strips x (L + 63) x 64) occurrences; below 64 the stage takes a
    wavefront per occurrence whatever else would decide. For three strips that is (L + 63) x 192 > 2^26: a target of
    349 463 residues or more. BLOSUM62 at 11/1 with the cut at the query's score against itself: every diagonal entry
    exceeds the rest of its row, so only the identity alignment reaches the cut and the answer is the planted copies.
    Measured: 3.1 s (HW) and 4.1 s (SW) on an MI355X with the witness; 352 000 is 0.7 % above the threshold."""
    assert align_capacity(DEEP_Q, 349462) == 64 and align_capacity(DEEP_Q, 349463) == 63 and align_capacity(DEEP_Q, DEEP_LONGEST) == 63
    query, _, _, targets, ends = deep_set()
    table = B62.reshape(24, 24)
    assert all(table[a, a] > np.delete(table[a], a).max() for a in set(query.tolist()))
    self_score = int(table[query, query].sum())
    V, R, offsets = deep_witness(algorithm)
    want = expected_flat(V, R, offsets, self_score, DEEP_Q)
    # the witness agrees: these columns and no others reach the cut
    assert list(zip(want["target"].tolist(), want["end_t"].tolist())) == ends and np.count_nonzero(V >= self_score) == len(ends)
    assert np.all(want["score"] == self_score) and np.all(want["end_q"] == DEEP_Q - 1)
    assert all(100_000 < j < DEEP_LONGEST - 50_000 for t, j in ends if t == DEEP_AT)
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")   # (a stage that could take lanes would: routing[0] says it did not)
    got = deep_db.search_occurrence_alignments(query, B62, 11, 1, algorithm, min_score=self_score, window=DEEP_Q)
    assert_answer(got, want, algorithm)
    assert np.array_equal(got["start_t"], want["end_t"] - DEEP_Q + 1) and np.all(got["start_q"] == 0)
    assert np.array_equal(np.diff(got["aln_off"]), [DEEP_Q] * len(ends)) and np.all(got["aln_flat"] == MATCH)
    assert deep_db.last_occurrence_align_routing() == [0, len(ends), 1, DEEP_Q]
    assert deep_db.last_occurrence_routing() == [len(targets), len({t for t, _ in ends}), 2, 3]


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_every_column_of_a_very_long_target(deep_db, algorithm):
    """the sweep alone over the same database, window 0 at the lowest cut: all 352 000 columns of the long target and
    those of the short ones against the recurrence. Measured: 2.6 s (HW) and 3.5 s (SW) on an MI355X."""
    query, _, offsets, targets, _ = deep_set()
    V, R, flat_offsets = deep_witness(algorithm)
    cut = lowest_cut(algorithm)
    want = expected_flat(V, R, flat_offsets, cut, 0)
    got = deep_db.search_occurrences(query, B62, 11, 1, algorithm, min_score=cut, window=0)
    assert_answer(got, want, algorithm)
    assert got["count"] > DEEP_LONGEST // 2 and (algorithm == "sw" or got["count"] == offsets[-1])
    assert deep_db.last_occurrence_routing() == [len(targets), len(set(want["target"].tolist())), 2, 3]
