"""The entry points that have a 32-bit lane kernel of their own - pair lists, PSSMs, occurrences, aligned occurrences, the
batch search, profile columns - over the case list of tests/_cases.py: alphabets of 2, 4, 20 and 32 letters, gap models
with open < extend and with a zero among them, matrices that are asymmetric, never positive, never negative or +-1, and
queries of one row to three strips. Every comparison is exact and covers every element; the witnesses are those of
tests/_case_witnesses.py, which tests/test_cases_cpu.py holds to the C checker on the same cases."""
import numpy as np
import pytest

import _cases
import _profile
import _pssm
from _case_witnesses import (ALGORITHMS, align_window_of, alignments, checker, checker_batch, checker_pairs, cut_of,
                             occurrences, window_of)
from test_gpu_occurrences import assert_answer
from test_gpu_pairs import KEYS, check_routing, same

pytestmark = pytest.mark.gpu

CASES = _cases.cases()
by_case = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
MODES = ("score", "end", "full")
FLAT = {"score": ("score",), "end": ("score", "end_t", "end_q"),
        "full": ("score", "end_t", "end_q", "start_t", "start_q", "aln")}     # the keys of a tests/_oracle.search dict
SWITCHES = {"lanes": "MIOPAL_FORCE_LANE_PER_PAIR", "waves": "MIOPAL_NO_PERPAIR"}
PACKED = 64 | 128     # miopalLastFullRouting: directions / start cells of two pairs per lane on 16-bit halves


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def database_of(capi):
    """case -> its targets on the device, uploaded on first use"""
    dbs = {}

    def get(case):
        if case not in dbs:
            s = case.search_set()
            dbs[case] = capi.DeviceDatabase(s.residues, s.offsets, case.alphabet)
        return dbs[case]
    yield get
    for db in dbs.values():
        db.close()


@pytest.fixture
def routed(request, tuning):
    """"default": the suite's own (no small-search routing); "production": the routing of small searches as shipped
    (the small_search_routing fixture); "lanes" / "waves": one kind of pair kernel forced"""
    kind = request.param
    if kind == "production":
        request.getfixturevalue("small_search_routing")
    elif kind != "default":
        tuning.setenv(SWITCHES[kind], "1")
    return kind


every_routing = pytest.mark.parametrize("routed", ["production", "lanes", "waves"], indirect=True)


# ---- pair lists -----------------------------------------------------------------------------------------------------

@by_case
@every_routing
def test_align_pairs(database_of, routed, case):
    db, s, p = database_of(case), case.search_set(), case.pair_set()
    n = len(p.pair_query)
    for algorithm in ALGORITHMS:
        want = checker_pairs(case, algorithm)
        for mode in MODES:
            got = db.align_pairs(p.queries, p.pair_query, p.pair_target, s.matrix, *case.gaps, mode, algorithm)
            routing = db.last_pair_routing()
            check_routing(routing, n, routed)
            assert routing[2] == np.count_nonzero(s.lengths[p.pair_target] == 0), (case.id, routing)
            same(got, want, mode, f"{case.id} {routed} {mode} {algorithm}")


@by_case
@every_routing
def test_align_pairs_pssm(database_of, routed, case):
    """the class identity of tests/_pssm.py: each PSSM is the matrix rows of its query, the query its consensus. On a
    list this short the cost estimates prefer a wavefront per pair: only "lanes" reaches the row-indexed lane kernel
    of pairlist_pssm.hip, and check_routing asserts that it did."""
    db, s, p = database_of(case), case.search_set(), case.pair_set()
    table = s.matrix.reshape(case.alphabet, case.alphabet)
    pssms = [np.ascontiguousarray(table[q]) for q in p.queries]
    for algorithm in ALGORITHMS:
        want = checker_pairs(case, algorithm)
        for mode in MODES:
            got = db.align_pairs_pssm(pssms, p.queries, p.pair_query, p.pair_target, *case.gaps, mode, algorithm)
            routing = db.last_pair_routing()
            check_routing(routing, len(p.pair_query), routed)
            assert routing[2] == np.count_nonzero(s.lengths[p.pair_target] == 0), (case.id, routing)
            _pssm.assert_same(got, {key: want[key] for key in KEYS[mode]}, (case.id, routed, mode, algorithm))


@by_case
@pytest.mark.parametrize("routed", ["default", "production", "lanes"], indirect=True)
def test_search_pssm(database_of, routed, case):
    """the lane-per-target kernels (the suite's default for small databases), the routing as shipped, and the later
    passes one lane per pair - where the packed 16-bit kernels are the router's choice whenever they apply"""
    db, s = database_of(case), case.search_set()
    for algorithm in ALGORITHMS:
        want = checker(case, algorithm)
        for mode in MODES:
            got = db.search_pssm(s.rows, s.query, *case.gaps, mode, algorithm)
            _pssm.assert_same(got, {key: want[key] for key in FLAT[mode]}, (case.id, routed, mode, algorithm))
            if mode == "full" and case.gaps[0] < case.gaps[1]:
                # what the router promises: no packed 16-bit later pass where opening is cheaper than extending
                assert db.last_full_routing() & PACKED == 0, (case.id, routed, algorithm, db.last_full_routing())


def test_packed_later_passes_are_taken_where_opening_costs_at_least_extending(database_of, tuning):
    """the other side of the promise above, so that it is not kept by a router that never packs: at 3/1, with entries
    in [-6, 15] and the later passes forced onto one lane per pair, the scores fit the byte profile and the half floats
    of perpair_packed.hip (packedTraceFits, packedScanFits) - some case takes the packed directions, some the packed
    start cells"""
    tuning.setenv(SWITCHES["lanes"], "1")
    seen = 0
    for case in CASES:
        if case.gaps == (3, 1):
            db, s = database_of(case), case.search_set()
            for algorithm in ("sw", "hw"):
                got = db.search_pssm(s.rows, s.query, *case.gaps, "full", algorithm)
                _pssm.assert_same(got, {key: checker(case, algorithm)[key] for key in FLAT["full"]}, (case.id, algorithm))
                seen |= db.last_full_routing()
    assert seen & 64 and seen & 128, seen


# ---- occurrences ----------------------------------------------------------------------------------------------------

@by_case
def test_search_occurrences(database_of, case):
    """window 0 at the lowest cut: every column value (every positive column maximum under SW) is compared; and a
    window of a quarter of the query: the picker's choices among them"""
    db, s = database_of(case), case.search_set()
    forms = {"plain": lambda **rule: db.search_occurrences(s.query, s.matrix, *case.gaps, **rule),
             "pssm": lambda **rule: db.search_occurrences_pssm(s.rows, *case.gaps, **rule)}
    for algorithm in ("hw", "sw"):
        for window in (0, window_of(case)):
            want = occurrences(case, algorithm, window)
            for form, call in forms.items():
                got = call(algorithm=algorithm, min_score=cut_of(algorithm), window=window)
                assert_answer(got, want, (case.id, form, algorithm, window))
                assert db.last_occurrence_routing()[3] == (case.q + 63) // 64
        if algorithm == "hw":
            assert len(occurrences(case, "hw", 0)["target"]) == s.lengths.sum()


@by_case
@every_routing
def test_search_occurrence_alignments(database_of, routed, case):
    """starts and operations of every occurrence against tests/_occurrence_alignments.py's, plain and PSSM"""
    db, s = database_of(case), case.search_set()
    forms = {"plain": lambda **rule: db.search_occurrence_alignments(s.query, s.matrix, *case.gaps, **rule),
             "pssm": lambda **rule: db.search_occurrence_alignments_pssm(s.rows, s.query, *case.gaps, **rule)}
    for algorithm in ("hw", "sw"):
        found, start_t, start_q, ops = alignments(case, algorithm)
        lengths = np.array([len(o) for o in ops], dtype=np.int64)
        flat = np.concatenate(ops) if ops else np.zeros(0, dtype=np.uint8)
        for form, call in forms.items():
            context = (case.id, routed, form, algorithm)
            got = call(algorithm=algorithm, min_score=cut_of(algorithm), window=align_window_of(case))
            assert_answer(got, found, context)
            assert got["start_t"].dtype == np.int32 and got["start_q"].dtype == np.int32
            assert np.array_equal(got["start_t"], start_t), (context, np.flatnonzero(got["start_t"] != start_t)[:8])
            assert np.array_equal(got["start_q"], start_q), (context, np.flatnonzero(got["start_q"] != start_q)[:8])
            off = got["aln_off"]
            assert off.dtype == np.int64 and len(off) == len(ops) + 1 and off[0] == 0 and off[-1] == len(got["aln_flat"])
            assert np.array_equal(np.diff(off), lengths), context
            assert np.array_equal(got["aln_flat"], flat), (context, np.flatnonzero(got["aln_flat"] != flat)[:8])
            routing = db.last_occurrence_align_routing()
            if len(ops) == 0:
                assert routing == [0, 0, 0, 0], context
                continue
            assert routing[0] + routing[1] == len(ops) and routing[2] >= 1, (context, routing)
            assert routing[3] == (found["end_t"] - start_t + 1).max(), (context, routing)
            if routed == "lanes":
                assert routing[0] > 0, (context, routing)
            elif routed == "waves":
                assert routing[0] == 0, (context, routing)


# ---- the batch search -----------------------------------------------------------------------------------------------

@by_case
def test_search_batch(database_of, case):
    """the five queries at once, each row against the checker's answer for that query"""
    db, s, p = database_of(case), case.search_set(), case.pair_set()
    for algorithm in ALGORITHMS:
        want = checker_batch(case, algorithm)
        for mode in ("score", "end"):
            got = db.search_batch(p.queries, s.matrix, *case.gaps, mode, algorithm)
            assert sorted(got) == sorted(FLAT[mode])
            for key in FLAT[mode]:
                assert got[key].shape == (5, len(s.targets)) and got[key].dtype == np.int32
                assert np.array_equal(got[key], want[key]), (case.id, mode, algorithm, key, np.argwhere(got[key] != want[key])[:8])
            # every pair is accounted for: settled by a batch kernel, by the wavefront-per-pair kernel, or its query
            # went the single-query path
            routing = db.last_batch_routing()
            assert routing[0] + routing[1] + routing[2] * len(s.targets) == 5 * len(s.targets), (case.id, routing)


# ---- profile columns ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if c.q >= 7], ids=lambda c: c.id)
def test_profile_columns(database_of, case):
    """the ten best targets under each algorithm, in the checker's order of scores with two repeats: the checker's
    alignments projected (tests/_profile.project) and counted (tests/_profile.columns)"""
    db, s = database_of(case), case.search_set()
    A, Q = case.alphabet, case.q
    for algorithm in ALGORITHMS:
        want = checker(case, algorithm)
        best = np.argsort(-want["score"].astype(np.int64), kind="stable")[:10]
        targets = np.concatenate([best, best[:2]]).astype(np.int64)
        rows = [_profile.project(want["aln"][t], want["start_q"][t], want["start_t"][t], s.targets[t], Q, A) for t in targets]
        msa = np.vstack([s.query[None, :], np.stack(rows)])
        counts, _, _, weights, weighted = _profile.columns(msa, A)
        for form in ("plain", "pssm"):
            if form == "plain":
                got = db.profile_columns(s.query, s.matrix, targets, *case.gaps, algorithm, return_msa=True)
            else:
                got = db.profile_columns_pssm(s.rows, s.query, targets, *case.gaps, algorithm, return_msa=True)
            context = (case.id, form, algorithm)
            routing = db.last_pair_routing()
            assert routing[0] + routing[1] + routing[2] == len(targets), (context, routing)
            assert np.array_equal(got["msa"], msa), (context, np.argwhere(got["msa"] != msa)[:8])
            assert np.array_equal(got["counts"], counts), context
            assert np.array_equal(got["member_weights"], weights), context
            assert np.array_equal(got["weighted"], weighted), context
