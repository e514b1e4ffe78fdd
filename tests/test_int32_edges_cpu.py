"""The CPU checker at the edge of the 32-bit rule (score_ranges.h, int32Bound < 2^29), where test_gpu_int32_edges.py
holds every 32-bit kernel to it. The checker's traceback keeps `int` tables with NEG_INF = INT_MIN / 4, the very
sentinel the kernels use, so it is checked here first:

  * its scores in all four modes against the affine-gap recurrence in numpy int64 (test_range_edges_cpu.gotoh_scores)
    at the far end of every axis of _edges.INT32_AXES - the largest v with the formula's bound below 2^29; the CPU
    tier has no router to ask, the GPU tier takes its thresholds from the router,
  * every alignment of `full` re-scored in Python integers from its operations, the matrix and the gap costs: equal
    to the score, and running from the start cell to the end cell - independent of the 32-bit traceback tables,
  * the family does its job: at Q = 64 some target's NW or SW score has a magnitude of at least 2^27 on the axes that
    can reach one, so the GPU tier cannot pass on values that never leave the middle of the range,
  * miopalSelfTest(4) (score_ranges_selftest.h) holds one row per term of int32Bound, one unit inside and one outside.
"""
import functools

import numpy as np
import pytest

import _edges
import _oracle
from _edges import ALPHABET as A
from test_range_edges_cpu import ALGOS, gotoh_scores

AXES = list(_edges.INT32_AXES)
MATCH, DEL, INS, MISMATCH = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def far_end(axis, form, Q):
    """(model, query, targets, residues, offsets) at the largest v the formula admits for this family"""
    q, seqs = _edges.int32_family(form, Q)
    longest = max(len(s) for s in seqs)
    assert longest == max(_edges.INT32_LONG + Q, 4 * Q)
    v = _edges.int32_formula_last(axis, Q, longest)
    model = _edges.int32_model(axis, v)
    assert _edges.int32_formula(model, Q, longest) < 1 << 29 <= _edges.int32_formula(_edges.int32_model(axis, v + 1), Q, longest)
    res, off = _oracle.flatten(seqs)
    return model, q, seqs, res, off


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", [1, 33, 65, 130])
def test_checker_scores_against_the_int64_recurrence(Q, axis):
    for form in _edges.int32_forms(axis):
        m, q, seqs, res, off = far_end(axis, form, Q)
        matrix = _edges.model_matrix(m)
        for algo in ALGOS:
            want = gotoh_scores(np.repeat(q[None, :], len(seqs), axis=0), seqs, matrix, A, m["open"], m["ext"], algo)
            assert np.abs(want).max() < 1 << 29, (axis, form, algo)   # (what the rule promises of every final value)
            got = _oracle.search(q, res, off, matrix, m["open"], m["ext"], "score", algo)["score"]
            np.testing.assert_array_equal(got, want, err_msg=f"{axis} Q={Q} {form} {algo} {m}")


def rescore(ops, q, t, sq, st, S, go, ge):
    """(score, query residues consumed, target residues consumed) of the operations in Python integers: a run of k gap
    operations of one kind costs open + (k - 1) ext (open >= ext in every model here)"""
    score, i, j, run = 0, sq, st, None
    for op in ops:
        if op in (MATCH, MISMATCH):
            assert (q[i] == t[j]) == (op == MATCH)
            score += int(S[q[i], t[j]])
            i, j, run = i + 1, j + 1, None
        else:
            score -= ge if run == op else go
            run = op
            if op == DEL:
                i += 1
            else:
                j += 1
    return score, i - sq, j - st


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", [1, 33, 65, 130])
def test_full_alignments_rescored_from_their_operations(Q, axis):
    for form in _edges.int32_forms(axis):
        m, q, seqs, res, off = far_end(axis, form, Q)
        assert m["open"] >= m["ext"]
        matrix = _edges.model_matrix(m)
        S = matrix.reshape(A, A).astype(np.int64)
        for algo in ALGOS:
            got = _oracle.search(q, res, off, matrix, m["open"], m["ext"], "full", algo)
            want = _oracle.search(q, res, off, matrix, m["open"], m["ext"], "score", algo)["score"]
            np.testing.assert_array_equal(got["score"], want)
            for k, t in enumerate(seqs):
                where = (axis, Q, form, algo, k)
                eq, et, sq, st = (int(got[key][k]) for key in ("end_q", "end_t", "start_q", "start_t"))
                ops = got["aln"][k].tolist()
                if eq < 0 or et < 0:   # no cell at all: an empty target (a closed form of the border), or SW's empty best
                    assert ops == [] and (len(t) == 0 or (algo == "sw" and got["score"][k] == 0)), where
                    continue
                score, rows, columns = rescore(ops, q, t, sq, st, S, m["open"], m["ext"])
                assert score == got["score"][k], where
                assert (rows, columns) == (eq - sq + 1, et - st + 1), where
                if algo == "nw":
                    assert (sq, st, eq, et) == (0, 0, Q - 1, len(t) - 1), where
                elif algo == "hw":
                    assert (sq, eq) == (0, Q - 1), where
                elif algo == "ov":
                    assert (sq == 0 or st == 0) and (eq == Q - 1 or et == len(t) - 1), where


@pytest.mark.parametrize("axis", ["match", "open", "open=ext", "mixed"])
def test_family_reaches_the_ends_of_the_range(axis):
    # a condition on the INPUTS: some NW or SW score of the family at Q = 64 is within a factor of four of 2^29
    m, q, seqs, res, off = far_end(axis, "random", 64)
    matrix = _edges.model_matrix(m)
    extreme = 0
    for algo in ("nw", "sw"):
        score = _oracle.search(q, res, off, matrix, m["open"], m["ext"], "score", algo)["score"].astype(np.int64)
        extreme = max(extreme, int(np.abs(score).max()))
    print(f"INT32 family axis={axis} Q=64 model={m} largest |NW or SW score|={extreme}")
    assert extreme >= 1 << 27, (axis, m, extreme)


def test_self_test_rows_of_the_int32_bound():
    # score_ranges_selftest.h, rows 54 .. 59: every term of int32Bound one unit inside and one outside
    from pyopal_amd import _capi
    assert _capi.lib().miopalSelfTest(4) == 0
