"""The inputs of tests/test_gpu_windows.py held to their purpose, with the CPU checker alone (no GPU): the model
of the windows (tests/_windows.py) merges the checker's per-window results into the checker's whole-target result,
the tie databases do contain targets that only the merge's order decides, and every planted alignment of the seam
databases covers the column it was aimed at."""
import numpy as np
import pytest

import _data
import _oracle
import _windows as W

GEOMETRIES = [(256, 256), (256, 1024), (384, 512), (128, 8192)]   # (overlap, stride): the seam builders take any


def test_windows_of_a_target_at_its_transitions():
    """windowsOf and the last window's length at L = window, window + 1, k stride + overlap (+ 1)"""
    O, S = 128, 256
    assert W.windows(0, O, S) == [(0, 0)] and W.windows(384, O, S) == [(0, 384)]
    assert W.windows(385, O, S) == [(0, 384), (256, 129)]
    assert W.windows(2 * S + O, O, S) == [(0, 384), (256, 384)]
    assert W.windows(2 * S + O + 1, O, S) == [(0, 384), (256, 384), (512, 129)]
    for L in range(0, 2000):
        cut = W.windows(L, O, S)
        # every column is in a window, every window but the last is full, the last one's tail is beyond the
        # overlap of the one before
        assert cut[-1][0] + cut[-1][1] == L and all(n == S + O for _, n in cut[:-1])
        assert len(cut) == 1 or cut[-1][1] > O
    assert W.entries([0, 384, 385, 641], O, S) == 1 + 1 + 2 + 3
    assert W.segment_stride(128) == 256 and W.segment_stride(640) == 384


def test_merged_prefers_the_score_then_the_column_then_the_row():
    assert W.merged([(0, 7, 10, 3), (256, 7, 2, 1)]) == (7, 10, 3)        # the earlier column, whatever the window
    assert W.merged([(256, 7, 2, 1), (0, 7, 258, 0)]) == (7, 258, 0)      # one column: the smaller row
    assert W.merged([(0, 7, 10, 3), (256, 8, 300, 5)]) == (8, 556, 5)
    assert W.merged([(0, 0, -1, -1), (256, 0, -1, -1)]) == (0, -1, -1)
    assert W.merged([(0, -9, -1, -1), (256, -5, 0, 3)]) == (-5, 256, 3)


@pytest.fixture(scope="module", params=list(W.TIE_KINDS))
def tie_case(request):
    q, seqs, matrix, alphabet, built = W.tie_db(request.param)
    res, off = _oracle.flatten(seqs)
    out = {}
    for algo in ("sw", "hw"):
        out[algo] = (W.window_results(q, seqs, matrix, W.TIE_GAPS, algo, *W.TIE_PLAN),
                     _oracle.search(q, res, off, matrix, W.TIE_GAPS[0], W.TIE_GAPS[1], "end", algo))
    return q, seqs, built, out


@pytest.mark.parametrize("algo", ["sw", "hw"])
def test_model_of_the_merge_equals_the_checker_on_whole_targets(tie_case, algo):
    q, seqs, built, out = tie_case
    per, ref = out[algo]
    for k in range(len(seqs)):
        assert W.merged(per[k]) == (ref["score"][k], ref["end_t"][k], ref["end_q"][k]), (k, per[k])


@pytest.mark.parametrize("algo", ["sw", "hw"])
def test_tie_databases_hold_cross_window_ties(tie_case, algo):
    """a condition on the inputs: at least 20 of the 200 random targets have two windows whose first maxima tie at
    the optimum in different cells, and every constructed target has one (its copies of the query)"""
    q, seqs, built, out = tie_case
    per, ref = out[algo]
    ties = W.cross_window_ties(per)
    assert len([k for k in ties if k < 200]) >= 20, len(ties)
    assert set(built) <= set(ties)
    for k, end in built.items():   # the checker reports the first copy
        assert ref["end_t"][k] == end and ref["end_q"][k] == len(q) - 1
        held = [_holding(len(seqs[k]), c, len(q)) for c in _copies(seqs[k], q)]
        assert len(held) in (2, 3) and all(h for h in held)
        assert all(not (a & b) for x, a in enumerate(held) for b in held[x + 1:]), "a window holds two copies"


def _holding(L, c, qlen):
    """the windows of a target of L residues that hold the whole copy ending on column c"""
    return {x for x, (a, n) in enumerate(W.windows(L, *W.TIE_PLAN)) if a <= c - qlen + 1 and c < a + n}


def _copies(t, q):
    """last columns of the exact copies of q in t"""
    return [at + len(q) - 1 for at in range(len(t) - len(q) + 1) if np.array_equal(t[at:at + len(q)], q)]


@pytest.fixture(scope="module")
def seam_query():
    q = _data.random_protein(np.random.default_rng(5), 24)
    return q, W.widest_join(7, q, W.B62, (1, 1))


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_seam_databases_cover_their_aims(seam_query, geometry):
    """every planted offset yields an alignment whose [start_t, end_t] covers the column it was aimed at (the last
    column of a window, the first column of the next), and the long-gap ones span len(q) + g columns: with g = 40 and
    with the widest g the checker joins. (The span of an optimal alignment of the two halves stays below
    len(q) + the weaker half's score / the gap cost per column, about a third of the overlap: `reach` bounds EVERY
    positive alignment, joined or not, and no input spans it.)"""
    q, widest = seam_query
    O, S = geometry
    assert 40 < widest < O
    long_spans = 0
    for g, gaps in ((0, (3, 1)), (40, (1, 1)), (widest, (1, 1))):
        seqs, aims = W.seam_db(7, q[:12], q[12:], g, O, S)
        assert len(seqs) == len(aims) == 36 and all(len(t) == 3 * S + O // 2 for t in seqs)
        wanted = {k * S + O - 1 for k in (1, 2)} | {k * S for k in (1, 2)}   # last / first columns of windows
        assert wanted <= {c for _, c in aims}
        res, off = _oracle.flatten(seqs)
        for algo in ("sw", "hw"):
            ref = _oracle.search(q, res, off, W.B62, gaps[0], gaps[1], "full", algo)
            assert W.covers(ref, aims).all(), (g, algo, np.flatnonzero(~W.covers(ref, aims)))
            spans = ref["end_t"] - ref["start_t"] + 1
            assert (spans == len(q) + g).all(), (g, algo, spans)
            np.testing.assert_array_equal(ref["start_t"], [at for at, _ in aims])
            long_spans += int((spans > len(q) + 20).sum()) if algo == "sw" else 0
    assert long_spans >= 5


def test_transition_database_has_every_listed_length():
    q = _data.random_protein(np.random.default_rng(5), 24)
    for O, S in GEOMETRIES:
        seqs, listed = W.transition_db(3, q, O, S)
        lengths = [len(t) for t in seqs]
        assert lengths[:listed] == 2 * W.transition_lengths(O, S) and max(lengths[listed:]) < 400
        assert W.entries(lengths, O, S) == len(seqs) + 2 * (0 + 0 + 1 + 1 + 1 + 2 + 2 + 3)
