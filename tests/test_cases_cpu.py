"""CPU tier of the case list (tests/_cases.py): the list covers what it claims to cover; the numpy witnesses that
tests/test_gpu_cases.py holds the kernels to - the generalised start rule of tests/_occurrence_alignments.py,
test_gpu_occurrences.column_values, _pssm.dp_scores - agree with the C checker on every case, before any kernel is
asked; and the list is not vacuous, by the witnesses alone."""
import itertools

import numpy as np
import pytest

import _cases
import _oracle
import _pssm
from _case_witnesses import (ALGORITHMS, DEL, INS, MATCH, MISMATCH, align_window_of, alignments, checker, checker_pairs,
                             columns, occurrences, window_of)
from _occurrence_alignments import border, operations, starts

CASES = _cases.cases()
by_case = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])


# ---- census ---------------------------------------------------------------------------------------------------------

def test_every_pair_of_values_of_two_axes_occurs():
    assert len(CASES) == 40 == len(_cases.GAPS) * len(_cases.KINDS)   # (the floor: the two widest axes)
    assert [c.index for c in CASES] == list(range(40)) and len({c.id for c in CASES}) == 40
    for c in CASES:
        for axis, values in _cases.AXES.items():
            assert getattr(c, axis) in values, (c.id, axis)
    for (a, values_a), (b, values_b) in itertools.combinations(_cases.AXES.items(), 2):
        seen = {(getattr(c, a), getattr(c, b)) for c in CASES}
        assert seen == set(itertools.product(values_a, values_b)), (a, b)


@by_case
def test_fill(case):
    s, p = case.search_set(), case.pair_set()
    A, Q = case.alphabet, case.q
    m = s.matrix.reshape(A, A)
    used = m[np.ix_(s.letters, s.letters)]
    assert len(s.letters) == (2 if case.span == "two" else A) and s.letters.max() == A - 1
    assert set(np.unique(s.residues).tolist()) <= set(s.letters.tolist()) and set(s.query.tolist()) <= set(s.letters.tolist())
    if case.kind == "asymmetric":
        assert m.min() >= -4 and m.max() <= 11 and not np.array_equal(m, m.T)
    elif case.kind == "symmetric":
        assert m.min() >= -4 and m.max() <= 11 and np.array_equal(m, m.T)
    elif case.kind == "nonpositive":
        assert m.max() == 0 and (used == 0).any() and (used < 0).any()
    elif case.kind == "nonnegative":
        assert m.min() == 0 and (used == 0).any() and (used > 0).any()
    else:
        assert set(np.unique(m).tolist()) == {-1, 1} == set(np.unique(used).tolist())
    # three wavefronts of lane-per-target, the last one ragged; the lengths next to the query's among them
    assert len(s.targets) == 130 and 130 % 64 not in (0, 63) and np.array_equal(np.diff(s.offsets), s.lengths)
    assert {0, 1, Q - 1, Q, Q + 1} <= set(s.lengths.tolist()) and s.lengths.max() <= max(_cases.LONGEST, 2 * Q)
    assert np.array_equal(s.targets[s.twice], np.concatenate([s.query, s.query]))
    assert abs(len(s.targets[s.copy]) - Q) <= 60 and np.array_equal(s.rows, m[s.query])
    # the pair list: every query length, repeats, the empty targets under every query, lanes that differ in strips
    assert [len(q) for q in p.queries] == list(_cases.QUERY_LENGTHS) and p.queries[_cases.QUERY_LENGTHS.index(Q)] is s.query
    pairs = list(zip(p.pair_query.tolist(), p.pair_target.tolist()))
    assert 280 <= len(pairs) <= 320 and len(set(pairs)) < len(pairs)
    assert {(i, int(t)) for i in range(5) for t in np.flatnonzero(s.lengths == 0)} <= set(pairs)
    assert all(len(set(p.pair_query[k:k + 64].tolist())) == 5 for k in range(0, len(pairs) - 63, 64))


# ---- the generalised start rule, against the C checker --------------------------------------------------------------

@by_case
@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_starts_from_the_checkers_end_cell_are_the_checkers(case, algorithm):
    """the checker's own best (score, end cell) of every target is an occurrence, and the rule applied to it must give
    the checker's start, under all eight gap models; the operations of the rectangle are then the checker's. Where both
    forms of F apply, they agree."""
    s = case.search_set()
    want = checker(case, algorithm)
    live = np.flatnonzero(want["end_t"] >= 0)
    assert np.array_equal(live, np.flatnonzero(want["score"] > 0 if algorithm == "sw" else s.lengths > 0))
    assert len(live) > 100 or (algorithm == "sw" and case.kind == "nonpositive" and len(live) == 0)
    occ = [(k, want["score"][k], want["end_t"][k], want["end_q"][k]) for k in live]
    start_t, start_q = starts(s.rows, s.targets, occ, *case.gaps, algorithm)
    assert np.array_equal(start_t, want["start_t"][live]), case.id
    assert np.array_equal(start_q, want["start_q"][live]), case.id
    if case.gaps[0] >= case.gaps[1]:
        other = starts(s.rows, s.targets, occ, *case.gaps, algorithm, by_rows=True)
        assert np.array_equal(other[0], start_t) and np.array_equal(other[1], start_q)
    else:
        with pytest.raises(AssertionError):
            starts(s.rows, s.targets, occ, *case.gaps, algorithm, by_rows=False)
    ops = operations(s.query, s.matrix, s.targets, occ, start_t, start_q, *case.gaps)
    for k, mine in zip(live, ops):
        assert mine.tolist() == want["aln"][k].tolist(), (case.id, k)


def test_both_forms_on_a_hand_worked_column():
    """match +2, mismatch -1, query ABC, target C A B C A (test_occurrence_alignments_cpu.py's): at 2/1 both forms, at
    1/3 the rows only - every gap residue then costs an opening, and the column after the exact occurrence is that
    occurrence and one residue gapped: 6 - 1"""
    matrix = np.full((4, 4), -1, dtype=np.int32)
    np.fill_diagonal(matrix, 2)
    query, target = np.array([0, 1, 2], dtype=np.uint8), np.array([2, 0, 1, 2, 0], dtype=np.uint8)
    for by_rows in (False, True):
        start_t, start_q = starts(matrix[query], [target], [(0, 6, 3, 2), (0, 4, 4, 2)], 2, 1, "hw", by_rows=by_rows)
        assert start_t.tolist() == [1, 1] and start_q.tolist() == [0, 0]
    start_t, start_q = starts(matrix[query], [target], [(0, 6, 3, 2), (0, 5, 4, 2)], 1, 3, "hw")
    assert start_t.tolist() == [1, 1] and start_q.tolist() == [0, 0]
    # the left border of the reversed pass is k + 1 openings: against the target A, C and B gapped at -2 and A on A
    assert border(1, 1, 3) == -2
    start_t, start_q = starts(matrix[query], [np.array([0], dtype=np.uint8)], [(0, 0, 0, 2)], 1, 3, "hw")
    assert (start_t.tolist(), start_q.tolist()) == ([0], [0])


# ---- the second witness: every column, and the scores ---------------------------------------------------------------

@by_case
@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_running_maximum_of_the_columns_is_the_checkers_score_of_the_prefix(case, algorithm):
    """column_values against the checker: the best value up to column j of a target is the checker's score of the
    target's first j + 1 residues - twelve targets, the two planted ones among them, and all their prefixes; and the
    first column that holds a target's best value, with its row, is the checker's end cell"""
    s = case.search_set()
    V, R = columns(case, algorithm)
    chosen = sorted({s.copy, s.twice, *np.argsort(-s.lengths, kind="stable")[::13][:10].tolist()})
    prefixes = [s.targets[k][:j + 1] for k in chosen for j in range(s.lengths[k])]
    residues, offsets = _oracle.flatten(prefixes)
    want = _oracle.search(s.query, residues, offsets, s.matrix, *case.gaps, "score", algorithm)["score"]
    at = 0
    for k in chosen:
        values = V[k, :s.lengths[k]]
        running = np.maximum.accumulate(np.maximum(values, 0) if algorithm == "sw" else values)
        assert np.array_equal(running, want[at:at + s.lengths[k]]), (case.id, k)
        at += s.lengths[k]
    assert at == len(want) > 500
    whole = checker(case, algorithm)
    for k in np.flatnonzero(whole["end_t"] >= 0):
        j = int(np.argmax(V[k, :s.lengths[k]]))
        assert (V[k, j], j, R[k, j]) == (whole["score"][k], whole["end_t"][k], whole["end_q"][k]), (case.id, k)


@by_case
@pytest.mark.parametrize("algorithm", ["sw", "nw"])
def test_dp_scores_are_the_checkers(case, algorithm):
    s = case.search_set()
    assert np.array_equal(_pssm.dp_scores(s.rows, s.targets, *case.gaps, algorithm), checker(case, algorithm)["score"]), case.id


# ---- not vacuous, by the witnesses alone ----------------------------------------------------------------------------

def operations_seen(case, algorithms=ALGORITHMS):
    flat = [a for algorithm in algorithms for a in checker(case, algorithm)["aln"] if len(a)]
    return set(np.unique(np.concatenate(flat)).tolist()) if flat else set()


def test_every_operation_code_occurs():
    assert set().union(*(operations_seen(c) for c in CASES)) == {MATCH, DEL, INS, MISMATCH}
    # ... and in the pair lists, whose queries differ in strip count inside a wavefront
    seen = set()
    for c in CASES[::7]:
        for algorithm in ALGORITHMS:
            seen |= set(np.unique(checker_pairs(c, algorithm)["aln_flat"]).tolist())
    assert seen == {MATCH, DEL, INS, MISMATCH}


@pytest.mark.parametrize("gaps", [g for g in _cases.GAPS if g != (40, 12)], ids=lambda g: f"{g[0]}.{g[1]}")
def test_gap_models_with_a_deletion_and_an_insertion(gaps):
    """in the alignments that are free to do without: local, and semi-global with a target longer than the query"""
    def both(c):
        s = c.search_set()
        for algorithm in ("sw", "hw", "ov"):
            want = checker(c, algorithm)
            for k, a in enumerate(want["aln"]):
                if (algorithm == "sw" or s.lengths[k] > c.q) and DEL in a and INS in a:
                    return True
        return False
    assert any(both(c) for c in CASES if c.gaps == gaps)


@pytest.mark.parametrize("kind", [k for k in _cases.KINDS if k != "nonpositive"])
def test_kinds_with_two_occurrences_in_one_target(kind):
    """at the cut and the window of the GPU tests, and at the wider window of the aligned ones"""
    def several(c):
        return all(np.bincount(occurrences(c, algorithm, window(c))["target"]).max() >= 2
                   for algorithm in ("hw", "sw") for window in (window_of, align_window_of))
    assert any(several(c) for c in CASES if c.kind == kind)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "nonpositive"], ids=lambda c: c.id)
def test_nothing_to_find_below_zero(case):
    s = case.search_set()
    for window in (0, window_of(case), align_window_of(case)):
        assert len(occurrences(case, "sw", window)["target"]) == 0
    assert np.all(columns(case, "sw")[0] == 0)
    want = checker(case, "sw")
    assert np.all(want["score"] == 0) and np.all(want["end_t"] == -1) and all(len(a) == 0 for a in want["aln"])
    # ... while HW has one occurrence per column at the lowest cut
    assert len(occurrences(case, "hw", 0)["target"]) == s.lengths.sum()


def test_degenerate_optimum_where_opening_is_cheaper_than_extending():
    """start target = end + 1: the gap over the whole query piece is the HW optimum, in the checker's answers and among
    the aligned occurrences"""
    in_checker = in_occurrences = 0
    for c in CASES:
        if c.gaps[0] < c.gaps[1]:
            want = checker(c, "hw")
            live = want["end_t"] >= 0
            in_checker += np.count_nonzero(want["start_t"][live] == want["end_t"][live] + 1)
            found, start_t, start_q, ops = alignments(c, "hw")
            empty = np.flatnonzero(start_t == found["end_t"] + 1)
            in_occurrences += len(empty)
            for k in empty:
                assert found["score"][k] == border(c.q - 1, *c.gaps) and ops[k].tolist() == [DEL] * c.q and start_q[k] == 0
    assert in_checker > 0 and in_occurrences > 0


def test_aligned_occurrences_stay_in_the_low_thousands():
    for c in CASES:
        for algorithm in ("hw", "sw"):
            n = len(alignments(c, algorithm)[0]["target"])
            assert n <= 4000 and (n > 0 or (c.kind == "nonpositive" and algorithm == "sw")), (c.id, algorithm, n)
