"""The PSSM forms of the top-k selection and of the pair list (miopalSearchPssmTop, miopalAlignPairsPssm,
DeviceDatabase.search_pssm_top / align_pairs_pssm, Aligner.top_hits_pssm / align_pairs_pssm).

The witnesses are those of tests/_pssm.py: a PSSM drawn from 32 row classes is an ordinary search over 32 letters for
the CPU checker; a numpy DP for rows that are all distinct; and miopalSearchPssm on the same handle, which is the
definition of both calls. Every comparison is exact and covers every pair / every slot. The database is test_gpu_pssm's:
~700 targets of 0-180 residues, zero-length ones and a repeated one among them; tests/conftest.py keeps lists of this
size eligible for the lane-per-pair kernels."""
import os
import re
import threading

import numpy as np
import pytest

import _data
import _oracle
import _pssm
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pyopal_amd", "csrc")
B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
ALGORITHMS = ("nw", "hw", "ov", "sw")
MODES = ("score", "end", "full")
KEYS = {"score": ("score",), "end": ("score", "end_q", "end_t"),
        "full": ("score", "end_q", "end_t", "start_q", "start_t", "aln")}
PLAIN_KEYS = {"score": ("score",), "end": ("score", "end_q", "end_t"),
              "full": ("score", "end_q", "end_t", "start_q", "start_t", "aln_off", "aln_flat")}
HEIGHTS = (1, 63, 64, 65, 130, 100)   # 423 rows: the table of the whole list fits LDS at 32 letters (493)
TALL = 200                            # ... and with this one, 623 rows, it does not


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def class_db(capi):
    """32 letters, for the class identity: (handle, residues, offsets)"""
    rng = np.random.default_rng(202)
    residues, offsets = _pssm.with_repeat(*_pssm.random_db(rng, _pssm.db_lengths(rng)))
    db = capi.DeviceDatabase(residues, offsets, 32)
    yield db, residues, offsets
    db.close()


@pytest.fixture(scope="module")
def protein_db(capi):
    """24 letters, for the PSSMs derived from a sequence"""
    rng = np.random.default_rng(101)
    residues, offsets = _pssm.with_repeat(*_data.random_db(rng, _pssm.db_lengths(rng)))
    db = capi.DeviceDatabase(residues, offsets, 24)
    yield db
    db.close()


@pytest.fixture(scope="module")
def pair_case(class_db):
    """Six class PSSMs (and a seventh, tall one for the list that does not fit) and ~1500 random pairs in random
    order: several workgroups, PSSMs of different heights in one wavefront, repeated pairs, and every PSSM against
    the empty targets and the targets of 1 / 63 / 64 / 65 residues."""
    db, residues, offsets = class_db
    rng = np.random.default_rng(404)
    pssms = [_pssm.class_pssm(rng, h) for h in HEIGHTS + (TALL,)]
    n = db.count
    pp = rng.integers(0, len(HEIGHTS), size=1400)
    pt = rng.integers(0, n, size=1400)
    pp[:100], pt[:100] = pp[100:200], pt[100:200]   # repeats
    special = np.array([(m, t) for m in range(len(HEIGHTS)) for t in (3, 5, 6, 7, 8, 11, 77, 20, n - 1)])
    pp = np.concatenate([pp, special[:, 0]])
    pt = np.concatenate([pt, special[:, 1]])
    order = rng.permutation(len(pp))
    return pssms, pp[order].astype(np.int32), pt[order].astype(np.int64)


_CHECKER = {}


def checker_full(tag, m, pssm, residues, offsets, gaps, algorithm):
    """the CPU checker's `full` answer of one class PSSM over the whole database, once per module (the score and the
    end cells of a `full` search are those of the score and end searches)"""
    key = (tag, m, gaps, algorithm)
    if key not in _CHECKER:
        _CHECKER[key] = _oracle.search(pssm[0], residues, offsets, pssm[1], gaps[0], gaps[1], "full", algorithm)
    return _CHECKER[key]


def gather(per_pssm, pp, pt, mode):
    """per-PSSM results over the whole database -> one entry per pair, in pair order (alignments as a list)"""
    out = {}
    for key in KEYS[mode]:
        if key == "aln":
            out[key] = [per_pssm[int(m)]["aln"][int(t)] for m, t in zip(pp, pt)]
        else:
            out[key] = np.array([per_pssm[int(m)][key][int(t)] for m, t in zip(pp, pt)], dtype=np.int32)
    return out


def by_search(db, pssms, pp, pt, gaps, mode, algorithm, consensus=None):
    """miopalSearchPssm's answer for every pair: one search per PSSM over the whole database, gathered"""
    per = {}
    for m in np.unique(pp):
        cons = pssms[m][0] if consensus is None else consensus[m]
        per[int(m)] = db.search_pssm(pssms[m][2], cons, gaps[0], gaps[1], mode, algorithm)
    return gather(per, pp, pt, mode)


def rows_of(pssms):
    return [p[2] for p in pssms]


def consensus_of(pssms):
    return [p[0] for p in pssms]


def check_sum(routing, n):
    assert routing[0] + routing[1] + routing[2] == n and routing[3] >= 1, routing


# ---- 1. pairs against the checker -------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("mode", MODES)
def test_pairs_against_the_checker(class_db, pair_case, tuning, mode, algorithm):
    """production routing, the lane-per-pair kernels forced (the row-indexed pairlist_forward_kernel, and for `full`
    perpair_kernel's row-indexed scan and direction pass), and the wavefront-per-pair kernels forced"""
    db, residues, offsets = class_db
    pssms, pp, pt = pair_case
    fits = pssms[:len(HEIGHTS)]
    per = {m: checker_full("pairs", m, fits[m], residues, offsets, (3, 1), algorithm) for m in range(len(fits))}
    want = gather(per, pp, pt, mode)
    empty = int(np.count_nonzero(np.diff(offsets)[pt] == 0))
    for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR", "MIOPAL_NO_PERPAIR"):
        if switch:
            tuning.setenv(switch, "1")
        got = db.align_pairs_pssm(rows_of(fits), consensus_of(fits), pp, pt, 3, 1, mode, algorithm)
        routing = db.last_pair_routing()
        # (score and end lists never read the consensus)
        bare = db.align_pairs_pssm(rows_of(fits), None, pp, pt, 3, 1, mode, algorithm) if mode != "full" else None
        if switch:
            tuning.delenv(switch)
        check_sum(routing, len(pp))
        assert routing[2] == empty, routing
        if switch == "MIOPAL_FORCE_LANE_PER_PAIR":
            assert routing[0] > 0, routing
        if switch == "MIOPAL_NO_PERPAIR":
            assert routing[0] == 0, routing
        _pssm.assert_same(got, want, (mode, algorithm, switch))
        if bare is not None:
            _pssm.assert_same(bare, want, (mode, algorithm, switch, "no consensus"))


# ---- 2. more rows than the table holds --------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_table_too_large_runs_one_wavefront_per_pair(class_db, pair_case, tuning, algorithm):
    """623 rows do not fit LDS: no error, no lane-per-pair kernel even when it is asked for, and every output is
    miopalSearchPssm's - for the pairs of the six PSSMs that alone would fit as well as for the tall one's"""
    db, residues, offsets = class_db
    pssms, pp, pt = pair_case
    rng = np.random.default_rng(6)
    extra = rng.integers(0, db.count, size=120)
    pp = np.concatenate([pp, np.full(len(extra), len(HEIGHTS), dtype=np.int32)])
    pt = np.concatenate([pt, extra])
    assert sum(len(p[2]) for p in pssms) == 623
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")
    for mode in ("end", "full"):
        got = db.align_pairs_pssm(rows_of(pssms), consensus_of(pssms), pp, pt, 3, 1, mode, algorithm)
        routing = db.last_pair_routing()
        check_sum(routing, len(pp))
        assert routing[0] == 0, routing
        _pssm.assert_same(got, by_search(db, pssms, pp, pt, (3, 1), mode, algorithm), (mode, algorithm))
    # ... and the tall PSSM's pairs against the checker
    tall = checker_full("tall", len(HEIGHTS), pssms[-1], residues, offsets, (3, 1), algorithm)
    mine = pp == len(HEIGHTS)
    want = gather({len(HEIGHTS): tall}, pp[mine], pt[mine], "full")
    _pssm.assert_same({k: ([got["aln"][int(i)] for i in np.flatnonzero(mine)] if k == "aln" else got[k][mine])
                       for k in KEYS["full"]}, want, ("tall", algorithm))


# ---- 3. derived == plain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_derived_pssms_equal_the_plain_pair_list(protein_db, tuning, algorithm):
    """rows = matrix[query], consensus = query: every output equals align_pairs of the same queries and pairs, and the
    list is routed like the plain one"""
    rng = np.random.default_rng(33)
    queries = [_data.random_protein(rng, n) for n in (1, 53, 64, 65, 130)]
    rows = [B62.reshape(24, 24)[q] for q in queries]
    pp = rng.integers(0, len(queries), size=900).astype(np.int32)
    pt = rng.integers(0, protein_db.count, size=900).astype(np.int64)
    for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR"):
        if switch:
            tuning.setenv(switch, "1")
        for mode in MODES:
            for gaps in ((3, 1), (11, 1)):
                plain = protein_db.align_pairs(queries, pp, pt, B62, gaps[0], gaps[1], mode, algorithm)
                plain_routing = protein_db.last_pair_routing()
                got = protein_db.align_pairs_pssm(rows, queries, pp, pt, gaps[0], gaps[1], mode, algorithm)
                assert protein_db.last_pair_routing() == plain_routing, (switch, mode, gaps)
                for key in PLAIN_KEYS[mode]:
                    assert np.array_equal(got[key], plain[key]), (switch, mode, gaps, key)
        assert not switch or plain_routing[0] > 0, plain_routing


# ---- 4. edges ---------------------------------------------------------------------------------------------------
def test_no_pairs(class_db, pair_case):
    db = class_db[0]
    pssms = pair_case[0][:2]
    for mode in MODES:
        got = db.align_pairs_pssm(rows_of(pssms), consensus_of(pssms), [], [], 3, 1, mode, "sw")
        assert len(got["score"]) == 0 and db.last_pair_routing() == (0, 0, 0, 0)
        if mode == "full":
            assert got["aln_off"].tolist() == [0] and len(got["aln_flat"]) == 0
    got = db.align_pairs_pssm([], None, [], [], 3, 1, "full", "nw")
    assert len(got["score"]) == 0 and got["aln_off"].tolist() == [0]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_empty_pssms_and_empty_targets(class_db, pair_case, tuning, algorithm):
    """the closed forms of the border: an empty PSSM against empty and other targets, PSSMs against empty targets"""
    db, residues, offsets = class_db
    none = (np.zeros(0, dtype=np.uint8), None, np.zeros((0, 32), dtype=np.int32))
    pssms = [pair_case[0][3], none, pair_case[0][0], none]
    pp = np.array([1, 1, 0, 0, 3, 2, 2, 1, 0], dtype=np.int32)
    pt = np.array([3, 11, 3, 77, 5, 3, 11, 8, 12], dtype=np.int64)
    assert np.diff(offsets)[[3, 77]].tolist() == [0, 0]
    without_dp = int(np.count_nonzero((np.diff(offsets)[pt] == 0) | (np.array([len(p[2]) for p in pssms])[pp] == 0)))
    assert without_dp >= 7
    for mode in MODES:
        want = by_search(db, pssms, pp, pt, (4, 2), mode, algorithm)
        for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR"):
            if switch:
                tuning.setenv(switch, "1")
            got = db.align_pairs_pssm(rows_of(pssms), consensus_of(pssms), pp, pt, 4, 2, mode, algorithm)
            assert db.last_pair_routing()[2] == without_dp
            _pssm.assert_same(got, want, (mode, algorithm, switch))
            if switch:
                tuning.delenv(switch)
        if mode != "score":
            assert got["end_q"][[0, 1, 2, 3, 4, 5]].tolist() == [-1] * 6 and got["end_t"][0] == -1
    # a list of empty PSSMs only: nothing for a device to do
    got = db.align_pairs_pssm([none[2]], [none[0]], [0, 0], [3, 11], 4, 2, "full", algorithm)
    assert db.last_pair_routing() == (0, 0, 2, 0) and got["aln_off"].tolist() == [0, 0, 0]
    assert got["score"].tolist() == by_search(db, [none], [0, 0], [3, 11], (4, 2), "score", algorithm)["score"].tolist()


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_few_pairs(class_db, pair_case, tuning, count):
    """one pair, and lists around one wavefront: as routed and on the lane-per-pair kernels"""
    db, residues, offsets = class_db
    pssms, pp, pt = pair_case
    fits = pssms[:len(HEIGHTS)]
    live = np.flatnonzero(np.diff(offsets)[pt] > 0)[:count]
    for algorithm in ("sw", "nw"):
        per = {m: checker_full("pairs", m, fits[m], residues, offsets, (3, 1), algorithm) for m in range(len(fits))}
        want = gather(per, pp[live], pt[live], "full")
        for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR"):
            if switch:
                tuning.setenv(switch, "1")
            got = db.align_pairs_pssm(rows_of(fits), consensus_of(fits), pp[live], pt[live], 3, 1, "full", algorithm)
            routing = db.last_pair_routing()
            check_sum(routing, count)
            assert not switch or routing[0] + routing[1] == count
            _pssm.assert_same(got, want, (count, algorithm, switch))
            if switch:
                tuning.delenv(switch)


def test_consensus_of_no_residues(class_db, pair_case, tuning):
    """a consensus of 255 throughout: no match operations, everything else unchanged"""
    db = class_db[0]
    pssms, pp, pt = pair_case
    fits = pssms[:len(HEIGHTS)]
    nothing = [np.full(len(p[2]), 255, dtype=np.uint8) for p in fits]
    for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR"):
        if switch:
            tuning.setenv(switch, "1")
        base = db.align_pairs_pssm(rows_of(fits), consensus_of(fits), pp, pt, 3, 1, "full", "sw")
        got = db.align_pairs_pssm(rows_of(fits), nothing, pp, pt, 3, 1, "full", "sw")
        assert 0 in base["aln_flat"] and 0 not in got["aln_flat"] and 3 in got["aln_flat"]
        for key in ("score", "end_q", "end_t", "start_q", "start_t", "aln_off"):
            assert np.array_equal(got[key], base[key]), (switch, key)
        differs = got["aln_flat"] != base["aln_flat"]
        assert np.all(base["aln_flat"][differs] == 0) and np.all(got["aln_flat"][differs] == 3)
    want = by_search(db, fits, pp[:300], pt[:300], (3, 1), "full", "sw", consensus=nothing)
    first = {k: (got[k][:300] if k != "aln" else got["aln"][:300]) for k in KEYS["full"]}
    _pssm.assert_same(first, want, "no residues")


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_rows_rich_in_ties(class_db, tuning, algorithm):
    """entries from {-2, 0, 3}: the tie-breaks of end cells and traceback, against the checker"""
    db, residues, offsets = class_db
    rng = np.random.default_rng(55)
    pssms = [_pssm.class_pssm(rng, h, values=[-2, 0, 3]) for h in (40, 64, 65, 170)]
    pp = rng.integers(0, len(pssms), size=500).astype(np.int32)
    pt = rng.integers(0, db.count, size=500).astype(np.int64)
    pt[:2] = (20, db.count - 1)   # the repeated target
    pp[:2] = 3
    per = {m: checker_full("ties", m, pssms[m], residues, offsets, (3, 1), algorithm) for m in range(len(pssms))}
    want = gather(per, pp, pt, "full")
    for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR"):
        if switch:
            tuning.setenv(switch, "1")
        got = db.align_pairs_pssm(rows_of(pssms), consensus_of(pssms), pp, pt, 3, 1, "full", algorithm)
        _pssm.assert_same(got, want, (algorithm, switch))
        assert got["score"][0] == got["score"][1] and got["aln"][0].tolist() == got["aln"][1].tolist()


# ---- 5. the second witness --------------------------------------------------------------------------------------
def test_distinct_rows_against_the_numpy_dp(class_db, tuning):
    """two PSSMs of 40 rows, all 80 different (no class identity to lean on), 50 pairs: scores against
    tests/_pssm.dp_scores, as routed and on the lane-per-pair kernel"""
    db, residues, offsets = class_db
    rng = np.random.default_rng(88)
    both = rng.integers(-9, 13, size=(80, 32)).astype(np.int32)
    assert len({r.tobytes() for r in both}) == 80
    rows = [both[:40], both[40:]]
    pp = rng.integers(0, 2, size=50).astype(np.int32)
    pt = rng.integers(0, db.count, size=50).astype(np.int64)
    pt[:3] = (3, 5, 11)
    targets = [residues[offsets[t]:offsets[t + 1]] for t in pt]
    for algorithm in ("sw", "nw"):
        for gaps in ((3, 1), (7, 2)):
            want = np.empty(50, dtype=np.int32)
            for m in (0, 1):
                mine = np.flatnonzero(pp == m)
                want[mine] = _pssm.dp_scores(rows[m], [targets[i] for i in mine], gaps[0], gaps[1], algorithm)
            for switch in (None, "MIOPAL_FORCE_LANE_PER_PAIR"):
                if switch:
                    tuning.setenv(switch, "1")
                got = db.align_pairs_pssm(rows, None, pp, pt, gaps[0], gaps[1], "score", algorithm)["score"]
                if switch:
                    assert db.last_pair_routing()[0] > 0
                    tuning.delenv(switch)
                assert np.array_equal(got, want), (algorithm, gaps, switch)


# ---- 6. the k best hits -----------------------------------------------------------------------------------------
def expected_top(full, k, min_score, start=0):
    """numpy's stable sort of miopalSearchPssm's arrays: score descending, index ascending; -1 past the count"""
    score = full["score"]
    order = np.argsort(-score.astype(np.int64), kind="stable")
    if min_score is not None:
        order = order[score[order] >= min_score]
    order = order[:k]
    out = {"count": len(order), "target": np.full(k, -1, dtype=np.int64)}
    out["target"][:len(order)] = order + start
    for key in full:
        out[key] = np.full(k, -1, dtype=np.int32)
        out[key][:len(order)] = full[key][order]
    return out


def check_top(got, want, context):
    assert got["count"] == want["count"], context
    for key in want:
        if key != "count":
            assert np.array_equal(got[key], want[key]), (context, key)


@pytest.mark.parametrize("length,values", [(40, None), (170, None), (40, (-2, 0, 3)), (170, (-2, 0, 3))])
def test_top_equals_the_sorted_search(class_db, length, values):
    db, residues, offsets = class_db
    rng = np.random.default_rng(7000 + length + (1 if values else 0))
    classes, matrix, rows = _pssm.class_pssm(rng, length, values=values)
    n = db.count
    for algorithm in ("sw", "nw"):
        for mode in ("score", "end"):
            full = db.search_pssm(rows, None, 3, 1, mode, algorithm)
            routing = db.last_routing()
            if mode == "score":
                want = checker_full(("top", length, values), 0, (classes, matrix), residues, offsets, (3, 1), algorithm)
                assert np.array_equal(full["score"], want["score"]), (algorithm, "the search itself")
            bound = int(np.sort(full["score"])[-25])   # a bound that cuts inside the list of the ten best ... or not
            for k in (1, 10, n + 5):
                for min_score in (None, bound, int(full["score"].max()) + 1):
                    got = db.search_pssm_top(rows, 3, 1, mode, algorithm, 0, None, k, min_score)
                    assert db.last_routing() == routing, (algorithm, mode, k)
                    check_top(got, expected_top(full, k, min_score), (length, values, algorithm, mode, k, min_score))
            # the repeated target: equal results, the smaller index first
            got = db.search_pssm_top(rows, 3, 1, mode, algorithm, 0, None, n)
            at = {int(t): i for i, t in enumerate(got["target"])}
            assert got["score"][at[20]] == got["score"][at[n - 1]] and at[20] < at[n - 1]


def test_top_of_a_slice_of_large_entries_and_of_nothing(class_db, capi):
    db, residues, offsets = class_db
    rng = np.random.default_rng(7100)
    classes, matrix, rows = _pssm.class_pssm(rng, 100)
    # a sub-slice: absolute indices
    for mode in ("score", "end"):
        part = db.search_pssm(rows, None, 3, 1, mode, "sw", 100, 230)
        got = db.search_pssm_top(rows, 3, 1, mode, "sw", 100, 230, 10)
        check_top(got, expected_top(part, 10, None, 100), ("slice", mode))
        assert got["target"].min() >= 100 and got["target"].max() < 230
    # entries up to +-300 (most of them +250 .. +300, one in seventeen -300): 170 rows against the longer targets score
    # beyond 32767, so those lanes leave the profile-driven kernels (test_large_entries_leave_the_16_bit_lanes)
    classes, matrix, rows = _pssm.class_pssm(rng, 170, values=list(range(250, 301, 5)) * 3 + [-300, -300])
    assert rows.max() == 300 and rows.min() == -300
    for algorithm in ("sw", "nw"):
        for mode in ("score", "end"):
            full = db.search_pssm(rows, None, 3, 1, mode, algorithm)
            routing = db.last_routing()
            assert routing[3] > 0 or routing[0] > 0, (algorithm, mode, routing)
            if mode == "score":
                want = _oracle.search(classes, residues, offsets, matrix, 3, 1, "score", algorithm)
                assert np.array_equal(full["score"], want["score"]) and want["score"].max() > 32767, algorithm
            got = db.search_pssm_top(rows, 3, 1, mode, algorithm, 0, None, 10)
            assert db.last_routing() == routing
            check_top(got, expected_top(full, 10, None), ("large", algorithm, mode))
    # nothing to select: checked, answered, nothing launched
    for k, start, end in ((0, 0, None), (5, 40, 40)):
        got = db.search_pssm_top(rows, 3, 1, "end", "sw", start, end, k)
        assert got["count"] == 0 and np.all(got["target"] == -1) and np.all(got["score"] == -1) and len(got["score"]) == k
    empty = db.search_pssm_top(np.zeros((0, 32), dtype=np.int32), 3, 1, "score", "nw", 0, None, 4)
    check_top(empty, expected_top(db.search_pssm(np.zeros((0, 32), dtype=np.int32), None, 3, 1, "score", "nw"), 4, None), "no rows")


def test_handle_checks_come_before_any_launch(capi, class_db, pair_case):
    """the checks that need the handle: its alphabet, the slice / the pair list's targets, the outputs of the
    selection, and the 32-bit range check with the rows' extreme entries"""
    db = class_db[0]
    lib = capi.lib()
    rows = np.ones((5, 32), dtype=np.int32)
    count = np.full(1, 77, dtype=np.int32)
    target = np.full(4, 77, dtype=np.int64)
    score = np.full(4, 77, dtype=np.int32)

    def top(r, alphabet=32, start=0, end=9, st=0, score_out=score):
        return lib.miopalSearchPssmTop(db.handle, r.ctypes.data, len(r), 3, 1, alphabet, st, 3, start, end, 4, -(2 ** 31),
                                       count.ctypes.data, target.ctypes.data,
                                       None if score_out is None else score_out.ctypes.data, None, None)

    assert top(np.ones((5, 24), dtype=np.int32), alphabet=24) == 101 and "differs from the database's" in capi.last_error()
    assert top(rows, start=3, end=2) == 101 and "bad slice" in capi.last_error()
    assert top(rows, end=db.count + 1) == 101 and "bad slice" in capi.last_error()
    assert top(rows, score_out=None) == 101 and "null target / score outputs" in capi.last_error()
    assert top(rows, st=1) == 101 and "null end-location outputs" in capi.last_error()
    huge = rows.copy()
    huge[2, 7] = 2 ** 30
    assert top(huge) == capi.OPAL_ERR_OVERFLOW and "32-bit range" in capi.last_error()
    assert np.all(count == 77) and np.all(target == 77) and np.all(score == 77)
    assert top(rows) == 0 and count[0] == 4 and not np.any(score == 77)

    offsets = np.array([0, 2, 5], dtype=np.int64)
    pair_pssm = np.array([0, 1, 1], dtype=np.int32)
    out = np.full(3, 77, dtype=np.int32)

    def pairs(r, pt, alphabet=32):
        pt = np.asarray(pt, dtype=np.int64)
        return lib.miopalAlignPairsPssm(db.handle, r.ctypes.data, None, offsets.ctypes.data, 2, pair_pssm.ctypes.data,
                                        pt.ctypes.data, 3, 3, 1, alphabet, 0, 3, out.ctypes.data, None, None, None, None,
                                        None, None)

    assert pairs(np.ones((5, 24), dtype=np.int32), [0, 1, 2], alphabet=24) == 101 and "differs from the database's" in capi.last_error()
    assert pairs(rows, [0, db.count, -1]) == 101 and f"pair 1: target index {db.count}" in capi.last_error()
    assert pairs(rows, [0, 1, -1]) == 101 and "pair 2: target index -1" in capi.last_error()
    assert pairs(huge, [0, 1, 2]) == capi.OPAL_ERR_OVERFLOW and "32-bit range" in capi.last_error()
    assert np.all(out == 77)
    assert pairs(rows, [0, 1, 2]) == 0 and not np.any(out == 77)
    with pytest.raises(ValueError):
        db.align_pairs_pssm([np.ones((5, 24), dtype=np.int32)], None, [0], [0])
    with pytest.raises(ValueError):
        db.align_pairs_pssm([rows], [np.zeros(4, dtype=np.uint8)], [0], [0], mode="full")
    with pytest.raises(ValueError):
        db.search_pssm_top(np.ones((5, 24), dtype=np.int32))


# ---- 7. Python --------------------------------------------------------------------------------------------------
FIELDS = {"score": ("target_index", "score"), "end": ("target_index", "score", "query_end", "target_end"),
          "full": ("target_index", "score", "query_end", "target_end", "query_start", "target_start",
                   "query_length", "target_length", "alignment")}


def _fields(result, names):
    """the named properties of a result object; None where the object refuses (a location of an empty alignment)"""
    out = []
    for name in names:
        try:
            out.append(getattr(result, name))
        except AssertionError:
            out.append(None)
    return out


@pytest.fixture(scope="module")
def python_case():
    import pyopal_amd
    rng = np.random.default_rng(77)
    residues, offsets = _data.random_db(rng, _pssm.db_lengths(rng, 300, 150))
    letters = np.frombuffer(_data.NCBI.encode(), dtype=np.uint8)
    targets = [bytes(letters[residues[offsets[k]:offsets[k + 1]]]).decode() for k in range(300)]
    targets.append(targets[20])
    database = pyopal_amd.Database(targets)
    pssms = []
    for length in (90, 1, 70, 0):
        classes, matrix, rows = _pssm.class_pssm(rng, length, alphabet=24)
        pssms.append(pyopal_amd.Pssm(rows.reshape(length, 24), consensus=classes))
    return pyopal_amd.Aligner(gap_open=4, gap_extend=2), database, pssms


def test_top_hits_pssm_equals_the_sorted_align_pssm(python_case):
    aligner, database, pssms = python_case
    for algorithm in ("sw", "nw"):
        for mode in MODES:
            everything = aligner.align_pssm(pssms[0], database, mode=mode, algorithm=algorithm)
            ranked = sorted(everything, key=lambda r: r.score, reverse=True)
            for k, min_score in ((10, None), (10, ranked[4].score), (len(database) + 3, None)):
                want = [r for r in ranked if min_score is None or r.score >= min_score][:k]
                got = aligner.top_hits_pssm(pssms[0], database, k, mode=mode, algorithm=algorithm, min_score=min_score)
                assert len(got) == len(want) and all(type(a) is type(b) for a, b in zip(got, want))
                for a, b in zip(got, want):
                    assert _fields(a, FIELDS[mode]) == _fields(b, FIELDS[mode]), (algorithm, mode, k, b.target_index)
    sliced = aligner.top_hits_pssm(pssms[0], database, 5, mode="end", start=50, end=120)
    want = sorted(aligner.align_pssm(pssms[0], database, mode="end", start=50, end=120), key=lambda r: r.score, reverse=True)[:5]
    assert [_fields(a, FIELDS["end"]) for a in sliced] == [_fields(b, FIELDS["end"]) for b in want]
    assert aligner.top_hits_pssm(pssms[0], database, 3, min_score=10 ** 6) == []


def test_align_pairs_pssm_equals_align_pssm_on_slices(python_case):
    aligner, database, pssms = python_case
    pairs = [(0, 5), (1, 5), (2, 299), (0, 3), (3, 9), (3, 3), (2, 20), (2, 300), (0, 5), (1, 77), (2, 11), (0, 150)]
    for algorithm in ("sw", "hw"):
        for mode in MODES:
            got = aligner.align_pairs_pssm(pssms, database, pairs, mode=mode, algorithm=algorithm)
            assert len(got) == len(pairs)
            for (i, j), a in zip(pairs, got):
                b = aligner.align_pssm(pssms[i], database, mode=mode, algorithm=algorithm, start=j, end=j + 1)[0]
                assert type(a) is type(b) and _fields(a, FIELDS[mode]) == _fields(b, FIELDS[mode]), (algorithm, mode, i, j)
                assert mode != "full" or a.query_length == len(pssms[i])
    as_array = aligner.align_pairs_pssm(pssms, database, np.array(pairs), mode="end")
    assert [_fields(a, FIELDS["end"]) for a in as_array] == \
           [_fields(b, FIELDS["end"]) for b in aligner.align_pairs_pssm(pssms, database, pairs, mode="end")]


# ---- 8. threads -------------------------------------------------------------------------------------------------
def test_two_threads_on_one_handle(class_db, pair_case):
    """each thread runs both calls five times on the shared handle and gets the single-threaded answers"""
    db, residues, offsets = class_db
    pssms, pp, pt = pair_case
    fits = pssms[:len(HEIGHTS)]
    cases = []
    for k, (mode, algorithm) in enumerate((("full", "sw"), ("end", "nw"))):
        cases.append((mode, algorithm, pssms[4 + k][2],
                      db.align_pairs_pssm(rows_of(fits), consensus_of(fits), pp, pt, 3, 1, mode, algorithm),
                      db.search_pssm_top(pssms[4 + k][2], 3, 1, "end", algorithm, 0, None, 25)))
    errors = []
    barrier = threading.Barrier(2)

    def work(k):
        mode, algorithm, rows, want_pairs, want_top = cases[k]
        try:
            barrier.wait(timeout=30)
            for _ in range(5):
                got = db.align_pairs_pssm(rows_of(fits), consensus_of(fits), pp, pt, 3, 1, mode, algorithm)
                for key in PLAIN_KEYS[mode]:
                    assert np.array_equal(got[key], want_pairs[key]), (k, key)
                check_top(db.search_pssm_top(rows, 3, 1, "end", algorithm, 0, None, 25), want_top, ("thread", k))
        except BaseException as e:   # noqa: BLE001 (reported on the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- 9. resources -----------------------------------------------------------------------------------------------
def test_forward_kernels_do_not_spill():
    """The build's resource remarks: sixteen pairlist_forward_kernel entries - the eight plain ones in pairlist.rpt, the
    eight row-indexed ones in pairlist_pssm.rpt (a translation unit of their own) - none with a spilled vector register
    or scratch memory, all at two wavefronts per SIMD."""
    reports = [os.path.join(CSRC, "pairlist.rpt"), os.path.join(CSRC, "pairlist_pssm.rpt")]
    if not all(os.path.exists(r) and os.path.getsize(r) for r in reports):
        pytest.skip("the build left no resource remarks")
    entries = {}
    for report in reports:
        name = None
        for line in open(report):
            m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
            if m:
                name = m.group(1) if "pairlist_forward_kernel" in m.group(1) else None
                if name:
                    entries[name] = {}
                continue
            m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
            if m and name:
                entries[name][m.group(1)] = int(m.group(2))
    assert len(entries) == 16, sorted(entries)
    assert sum(1 for n in entries if re.search(r"ILi\dELb[01]ELb1EEE", n)) == 8, sorted(entries)   # PSSM = true
    for name, k in entries.items():
        assert k["VGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0, (name, k)
        assert k["VGPRs"] <= 256 and k["Occupancy [waves/SIMD]"] >= 2, (name, k)
