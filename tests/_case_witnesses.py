"""What the witnesses say about each case of tests/_cases.py, computed once per process and shared by
tests/test_cases_cpu.py (which holds them to the C checker) and tests/test_gpu_cases.py (which holds the kernels to
them). The witnesses themselves are imported from where they are defined; nothing here restates one."""
import functools

import numpy as np

import _oracle
from _occurrence_alignments import operations, starts
from _occurrences import INT_MIN
from test_gpu_occurrences import column_values, expected
from test_gpu_pairs import expected as pairs_expected

ALGORITHMS = ("sw", "nw", "hw", "ov")
MATCH, DEL, INS, MISMATCH = 0, 1, 2, 3


def cut_of(algorithm):
    """the lowest cut there is: every column under HW, every positive column maximum under SW"""
    return 1 if algorithm == "sw" else INT_MIN


def window_of(case):
    """the suppression window of the occurrence tests: about a quarter of the query"""
    return case.q // 4


def align_window_of(case):
    """... and of the aligned ones: wide enough that the helper's lanes, one per occurrence, stay in the low thousands"""
    return max(case.q // 4, 3)


@functools.lru_cache(maxsize=None)
def checker(case, algorithm):
    """the C checker's `full` answer for the case's query against its targets"""
    s = case.search_set()
    return _oracle.search(s.query, s.residues, s.offsets, s.matrix, *case.gaps, "full", algorithm)


@functools.lru_cache(maxsize=None)
def checker_pairs(case, algorithm):
    """the C checker's `full` answer for every pair of the case's pair list"""
    s, p = case.search_set(), case.pair_set()
    return pairs_expected(p.queries, s.residues, s.offsets, p.pair_query, p.pair_target, s.matrix, *case.gaps, "full",
                          algorithm, threads=4)


@functools.lru_cache(maxsize=None)
def columns(case, algorithm):
    """every column's value and row (test_gpu_occurrences.column_values)"""
    s = case.search_set()
    return column_values(s.rows, s.targets, *case.gaps, algorithm)


@functools.lru_cache(maxsize=None)
def occurrences(case, algorithm, window):
    """the occurrences at the lowest cut: the rule (tests/_occurrences.pick) over `columns`"""
    V, R = columns(case, algorithm)
    return expected(V, R, case.search_set().lengths, cut_of(algorithm), window)


def as_tuples(found):
    return list(zip(found["target"].tolist(), found["score"].tolist(), found["end_t"].tolist(), found["end_q"].tolist()))


@functools.lru_cache(maxsize=None)
def alignments(case, algorithm):
    """-> (occurrences at align_window_of(case), start_t, start_q, operations): tests/_occurrence_alignments.py"""
    s = case.search_set()
    found = occurrences(case, algorithm, align_window_of(case))
    occ = as_tuples(found)
    start_t, start_q = starts(s.rows, s.targets, occ, *case.gaps, algorithm)
    return found, start_t, start_q, operations(s.query, s.matrix, s.targets, occ, start_t, start_q, *case.gaps)


@functools.lru_cache(maxsize=None)
def checker_batch(case, algorithm):
    """the C checker's `end` answer for each query of the case's pair set against every target, stacked by query"""
    s, p = case.search_set(), case.pair_set()
    parts = [_oracle.search(q, s.residues, s.offsets, s.matrix, *case.gaps, "end", algorithm) for q in p.queries]
    return {key: np.stack([part[key] for part in parts]) for key in ("score", "end_t", "end_q")}
