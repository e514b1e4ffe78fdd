"""The 32-bit kernels at the edge of the rule that admits a scoring model (score_ranges.h: int32Bound < 2^29), bit for
bit against the CPU checker - for column values against the int64 witness - through every entry point whose only
arithmetic, or last rung, they are.

The kernels share sentinels sized against exactly that bound: kNegInf = INT32_MIN / 4 = -2^29 (intraseq.hip,
perpair.hip, pairlist.hip, occurrences.hip), kPadScore = -2^28, table entries with `open` folded in, columns stored
scaled by j * ext. Every axis of _edges.INT32_AXES takes one term of the bound (`mixed`: all of them) to the LAST VALUE
THE ROUTER ADMITS - asked of the entry point under test by bisection on OverflowError, a refused search launches
nothing - and the edge family runs there:

  a. the score pass of DeviceDatabase.search, three search types x four modes, and once under the production routing
     of small searches,
  b. the later passes of `full` (start cells, directions, walk) in their lane-per-pair forms,
  c. search_pssm, over the class identity of tests/_pssm.py and with a PSSM whose extremes sit in different rows,
  d. align_pairs / align_pairs_pssm, two queries of 33 and 130 rows in one list, lane per pair and wavefront per pair,
  e. search_occurrences / search_occurrences_pssm: every column value, then a windowed pick,
  f. search_occurrence_alignments behind them.

Each test prints what it probed and reached (lines that start with INT32EDGE; profiles/int32_edges.txt holds those of
one run). test_int32_edges_cpu.py holds the
checker itself to the int64 recurrence on the same family at the same far ends.
"""
import functools

import numpy as np
import pytest

import _edges
import _oracle
from _edges import ALPHABET as A
from _occurrence_alignments import operations, starts
from _occurrences import INT_MAX, INT_MIN
from test_gpu_occurrences import assert_answer, column_values, expected
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

AXES = list(_edges.INT32_AXES)
QS = _edges.INT32_Q
ALGOS = ["nw", "hw", "ov", "sw"]
MODES = ["score", "end", "full"]
PACKED_TRACE, PACKED_SCAN, PACKED_GROUPS = 64, 128, 256     # miopalLastFullRouting: the 16-bit forms of the later passes
LANE_START_CELLS, LANE_DIRECTIONS = 1, 4                    # ... and their 32-bit forms, one lane per pair
WITNESS_NEG = -(1 << 60)
# Where a 16-bit rung of the score pass may keep results although the model is at the edge of the 32-bit rule:
# Smith-Waterman when only the gap costs are extreme. The lanes take min(cost, 32767) (host_search.inc,
# prepareLaunch); a positive value of SW's that pays such a gap is below zero either way, and the floor at 0 makes
# both the same cell. Lanes that leave the 16-bit range are flagged and redone at 32 bit as ever. The comparison
# with the checker stands; if it fails there, it is that argument that is wrong.
SW_KEEPS_16_BIT = {("sw", "open"), ("sw", "open=ext")}


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@functools.lru_cache(maxsize=None)
def inputs(form, Q):
    """(query, targets, residues, offsets) of the edge family; shared, nobody writes to it"""
    q, seqs = _edges.int32_family(form, Q)
    res, off = _oracle.flatten(seqs)
    for a in (q, res, off):
        a.setflags(write=False)
    return q, seqs, res, off


@pytest.fixture(scope="module")
def dbs(capi):
    """one handle per (query form, Q), for the whole module"""
    handles = {}

    def get(form, Q):
        if (form, Q) not in handles:
            _, _, res, off = inputs(form, Q)
            handles[(form, Q)] = capi.DeviceDatabase(res, off, A)
        return handles[(form, Q)]
    yield get
    for db in handles.values():
        db.close()


@pytest.fixture
def lane_per_pair(tuning):
    tuning.setenv("MIOPAL_NO_HYBRID_TRACE", "1")
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")


def gaps(m):
    return m["open"], m["ext"]


_PROBES = {}


def probe(entry, axis, Q, call, model_of=None):
    """The last v of `axis` that `call(model)` does not refuse with OverflowError, once per (entry point, axis, Q)."""
    key = (entry, axis, Q)
    if key not in _PROBES:
        model_of = model_of or (lambda v: _edges.int32_model(axis, v))

        def admitted(v):
            m = model_of(v)
            if max(abs(x) for x in m.values()) >= 1 << 31:   # (not an `int` any more: nothing to hand over)
                return False
            try:
                call(m)
            except OverflowError:
                return False
            return True
        _PROBES[key] = _edges.last_admitted(admitted, _edges.INT32_AXES[axis][1] if axis in _edges.INT32_AXES else 11,
                                            _edges.INT32_HIGH)
        print(f"INT32EDGE probe entry={entry} axis={axis} Q={Q} last_admitted={_PROBES[key]} model={model_of(_PROBES[key])}")
    return _PROBES[key]


@functools.lru_cache(maxsize=None)
def checker(form, Q, axis, v, mode, algo):
    q, _, res, off = inputs(form, Q)
    m = _edges.int32_model(axis, v)
    return _oracle.search(q, res, off, _edges.model_matrix(m), m["open"], m["ext"], mode, algo)


def extreme_of(want):
    score = want["score"].astype(np.int64)
    return int(score[np.argmax(np.abs(score))])


def search_probe(dbs, axis, Q):
    db = dbs("random", Q)
    q = inputs("random", Q)[0]
    return probe("search", axis, Q, lambda m: db.search(q, _edges.model_matrix(m), *gaps(m), "score", "sw"))


# ---- a. the score pass -------------------------------------------------------------------------------------------------
def run_score_pass(capi, dbs, Q, axis, small):
    v = search_probe(dbs, axis, Q)
    m = _edges.int32_model(axis, v)
    matrix = _edges.model_matrix(m)
    reached = {}
    for form in _edges.int32_forms(axis):
        q, seqs, res, off = inputs(form, Q)
        db = dbs(form, Q)
        nonempty = sum(1 for s in seqs if len(s))
        for mode in MODES:
            for algo in ALGOS:
                got = db.search(q, matrix, *gaps(m), mode, algo)
                routed = capi.DeviceDatabase.last_routing()
                where = f"{axis}={v} Q={Q} {form} {mode} {algo} routing {routed}"
                want = checker(form, Q, axis, v, mode, algo)
                compare(got, want, mode, where)
                if small:
                    assert routed == (len(seqs), 0, 0, 0), where
                elif routed[0] < nonempty:
                    # a 16-bit rung kept some results: only where the argument at SW_KEEPS_16_BIT holds
                    assert (algo, axis) in SW_KEEPS_16_BIT, where
                    print(f"INT32EDGE 16-bit rung admitted: {where}")
                reached[algo] = max(reached.get(algo, 0), abs(extreme_of(want)))
    print(f"INT32EDGE search Q={Q} axis={axis} last_admitted={v} largest |score| per mode={reached}")


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", QS)
def test_score_pass(capi, dbs, Q, axis):
    """intraseq_wide_kernel at Q <= 64, the strip-after-strip and strip-unit kernels above, the traced forms under
    `full`: every target with residues is computed at 32 bit, or a 16-bit rung is entitled to it"""
    run_score_pass(capi, dbs, Q, axis, small=False)


@pytest.mark.parametrize("axis", AXES)
def test_score_pass_production_small_search_routing(capi, dbs, small_search_routing, axis):
    """a search of so few targets goes to the 32-bit kernels whole: that routing, once"""
    for Q in (64, 130):
        run_score_pass(capi, dbs, Q, axis, small=True)


# ---- b. the later passes of `full` ------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", QS)
def test_full_later_passes_one_lane_per_pair(capi, dbs, lane_per_pair, Q, axis):
    """start-cell scan with its stop rule, direction pass and walk, one lane per pair at 32 bit: the packed 16-bit forms
    refuse every model here by their own rules"""
    v = search_probe(dbs, axis, Q)
    m = _edges.int32_model(axis, v)
    seen = set()
    for form in _edges.int32_forms(axis):
        q = inputs(form, Q)[0]
        for algo in ALGOS:
            got = dbs(form, Q).search(q, _edges.model_matrix(m), *gaps(m), "full", algo)
            bits = capi.DeviceDatabase.last_full_routing()
            where = f"{axis}={v} Q={Q} {form} full {algo} full routing {bits}"
            assert bits & (PACKED_TRACE | PACKED_SCAN | PACKED_GROUPS) == 0, where
            # (directions one lane per pair; start cells too, which NW does not need)
            assert bits & LANE_DIRECTIONS and (algo == "nw" or bits & LANE_START_CELLS), where
            seen.add(bits)
            compare(got, checker(form, Q, axis, v, "full", algo), "full", where)
    print(f"INT32EDGE full later passes Q={Q} axis={axis} v={v} routing words seen={sorted(seen)}")


# ---- c. position-specific scoring matrices ------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", QS)
def test_pssm_form(capi, dbs, Q, axis):
    """the rows of the matrix under the query's residues: the checker on (query, matrix) is the truth"""
    rows_of = lambda q, m: np.ascontiguousarray(_edges.model_matrix(m).reshape(A, A)[q])   # noqa: E731
    q0 = inputs("random", Q)[0]
    v = probe("search_pssm", axis, Q, lambda m: dbs("random", Q).search_pssm(rows_of(q0, m), None, *gaps(m), "score", "sw"))
    assert v == search_probe(dbs, axis, Q)   # (the extremes of these rows are the matrix's: one rule, one threshold)
    m = _edges.int32_model(axis, v)
    for form in _edges.int32_forms(axis):
        q = inputs(form, Q)[0]
        for mode in MODES:
            for algo in ALGOS:
                got = dbs(form, Q).search_pssm(rows_of(q, m), q, *gaps(m), mode, algo)
                compare(got, checker(form, Q, axis, v, mode, algo), mode, f"pssm {axis}={v} Q={Q} {form} {mode} {algo}")


@pytest.mark.parametrize("Q", [33, 130])
def test_pssm_extremes_in_different_rows(capi, dbs, Q):
    """the range check reads the extremes of the ROWS: the maximum stands in row 0 alone, the minimum in the last row
    alone, both at the last magnitude the router admits. Classes 0 and 1 are those two rows, the rest of the query is
    the family's: an ordinary search over (classes, matrix) for the checker."""
    q, seqs, res, off = inputs("random", Q)
    classes = q.copy()
    classes[0], classes[-1] = 0, 1
    assert 0 not in q and 1 not in q

    def matrix_of(v):
        S = _edges.model_matrix(_edges.BASE).reshape(A, A).copy()
        S[0, :] = S[1, :] = _edges.BASE["mild"]
        S[0, _edges.LETTER_A], S[1, _edges.LETTER_C] = v, -v
        return np.ascontiguousarray(S.ravel())
    db = dbs("random", Q)
    model_of = lambda v: dict(_edges.BASE, match=v, low=-v)   # noqa: E731
    v = probe("search_pssm split rows", "split", Q,
              lambda m: db.search_pssm(matrix_of(m["match"]).reshape(A, A)[classes], None, *gaps(m), "score", "sw"), model_of)
    matrix = matrix_of(v)
    rows = np.ascontiguousarray(matrix.reshape(A, A)[classes])
    assert (rows[0].max(), rows[-1].min()) == (v, -v) and np.abs(rows[1:-1]).max() < v
    for mode in MODES:
        for algo in ALGOS:
            got = db.search_pssm(rows, classes, 3, 1, mode, algo)
            want = _oracle.search(classes, res, off, matrix, 3, 1, mode, algo)
            compare(got, want, mode, f"pssm split rows v={v} Q={Q} {mode} {algo}")
    with pytest.raises(OverflowError):
        db.search_pssm(np.ascontiguousarray(matrix_of(v + 1).reshape(A, A)[classes]), classes, 3, 1, "score", "sw")


# ---- d. pair lists ------------------------------------------------------------------------------------------------------
PAIR_Q = (33, 130)


@functools.lru_cache(maxsize=None)
def pair_inputs(axis):
    """two queries of different lengths, the family of the longer and the made members of the shorter's, every target
    against both"""
    forms = _edges.int32_forms(axis)
    queries = [_edges.edge_query(forms[0], PAIR_Q[0]), _edges.edge_query(forms[-1], PAIR_Q[1])]
    seqs = _edges.int32_family(forms[-1], PAIR_Q[1])[1] + _edges.int32_family(forms[0], PAIR_Q[0])[1][:15]
    res, off = _oracle.flatten(seqs)
    pq = np.repeat(np.arange(2, dtype=np.int32), len(seqs))
    pt = np.tile(np.arange(len(seqs), dtype=np.int64), 2)
    order = np.random.default_rng(3).permutation(len(pq))
    return queries, seqs, res, off, pq[order], pt[order]


@pytest.fixture(scope="module")
def pair_dbs(capi):
    handles = {}

    def get(axis):
        key = _edges.int32_forms(axis)
        if key not in handles:
            _, _, res, off, _, _ = pair_inputs(axis)
            handles[key] = capi.DeviceDatabase(res, off, A)
        return handles[key]
    yield get
    for db in handles.values():
        db.close()


@functools.lru_cache(maxsize=None)
def pair_checker(axis, v, mode, algo):
    queries, seqs, res, off, pq, pt = pair_inputs(axis)
    m = _edges.int32_model(axis, v)
    per = [_oracle.search(q, res, off, _edges.model_matrix(m), m["open"], m["ext"], mode, algo) for q in queries]
    out = {key: np.where(pq == 0, per[0][key][pt], per[1][key][pt]) for key in per[0] if key != "aln"}
    if mode == "full":
        out["aln"] = [per[i]["aln"][t] for i, t in zip(pq.tolist(), pt.tolist())]
    return out


@pytest.mark.parametrize("switch,kind", [("MIOPAL_FORCE_LANE_PER_PAIR", "lanes"), ("MIOPAL_NO_PERPAIR", "waves")])
@pytest.mark.parametrize("axis", AXES)
def test_pair_lists(capi, pair_dbs, tuning, axis, switch, kind):
    """align_pairs and align_pairs_pssm (the rows of all the list's PSSMs in one LDS table, or one wavefront per pair):
    the rule is probed through the pair-list entry, which reads the list's own longest query and target"""
    queries, seqs, res, off, pq, pt = pair_inputs(axis)
    db = pair_dbs(axis)
    v = probe("align_pairs", axis, PAIR_Q, lambda m: db.align_pairs(queries, pq, pt, _edges.model_matrix(m), *gaps(m), "score", "sw"))
    m = _edges.int32_model(axis, v)
    matrix = _edges.model_matrix(m)
    rows = [np.ascontiguousarray(matrix.reshape(A, A)[q]) for q in queries]
    vp = probe("align_pairs_pssm", axis, PAIR_Q,
               lambda mm: db.align_pairs_pssm([np.ascontiguousarray(_edges.model_matrix(mm).reshape(A, A)[q]) for q in queries],
                                              None, pq, pt, *gaps(mm), "score", "sw"))
    assert vp == v
    tuning.setenv(switch, "1")
    without_dp = int(np.count_nonzero(np.diff(off)[pt] == 0))
    for mode in MODES:
        for algo in ALGOS:
            want = pair_checker(axis, v, mode, algo)
            for name, call in (("align_pairs", lambda: db.align_pairs(queries, pq, pt, matrix, *gaps(m), mode, algo)),
                               ("align_pairs_pssm", lambda: db.align_pairs_pssm(rows, queries, pq, pt, *gaps(m), mode, algo))):
                got = call()
                routing = db.last_pair_routing()
                where = f"{name} {axis}={v} {mode} {algo} {switch} routing {routing}"
                assert routing[0] + routing[1] + routing[2] == len(pq) and routing[2] == without_dp, where
                assert (routing[0] > 0) if kind == "lanes" else (routing[0] == 0 and routing[1] > 0), where
                compare(got, want, mode, where)
    print(f"INT32EDGE pair lists axis={axis} {kind} last_admitted={v} "
          f"extreme NW score={extreme_of(pair_checker(axis, v, 'score', 'nw'))} SW={extreme_of(pair_checker(axis, v, 'score', 'sw'))}")


# ---- e. the occurrence sweeps ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def witness(form, Q, axis, v, algo):
    """every column's value and row by the int64 recurrence, minus infinity at -2^60"""
    q, seqs, _, _ = inputs(form, Q)
    m = _edges.int32_model(axis, v)
    rows = _edges.model_matrix(m).reshape(A, A)[q]
    V, R = column_values(rows, seqs, m["open"], m["ext"], algo, neg=WITNESS_NEG)
    lengths = np.array([len(s) for s in seqs], dtype=np.int64)
    inside = np.arange(V.shape[1])[None, :] < lengths[:, None]
    assert V[inside].min() > -(1 << 29) and V[inside].max() < 1 << 29   # (what the rule promises of every value)
    return V, R, lengths, inside


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", QS)
def test_occurrence_sweeps(capi, dbs, Q, axis):
    """HW with the cut at INT_MIN and SW with the cut at 1, window 0: every value of the last row, every positive column
    maximum and its row; then one windowed pick, window = Q, the cut at the median. Q = 65 and 130 carry the boundary
    row and SW's running maximum from strip to strip through memory on the column scale j * ext."""
    q0 = inputs("random", Q)[0]
    db0 = dbs("random", Q)
    nothing = dict(min_score=INT_MAX, window=0)
    v = probe("search_occurrences", axis, Q, lambda m: db0.search_occurrences(q0, _edges.model_matrix(m), *gaps(m), "hw", **nothing))
    vp = probe("search_occurrences_pssm", axis, Q,
               lambda m: db0.search_occurrences_pssm(np.ascontiguousarray(_edges.model_matrix(m).reshape(A, A)[q0]), *gaps(m), "hw", **nothing))
    assert v == vp == search_probe(dbs, axis, Q)
    m = _edges.int32_model(axis, v)
    matrix = _edges.model_matrix(m)
    reached = {}
    for form in _edges.int32_forms(axis):
        q = inputs(form, Q)[0]
        db = dbs(form, Q)
        rows = np.ascontiguousarray(matrix.reshape(A, A)[q])
        for algo, lowest in (("hw", INT_MIN), ("sw", 1)):
            V, R, lengths, inside = witness(form, Q, axis, v, algo)
            values = V[inside] if algo == "hw" else V[inside & (V >= 1)]
            median = max(int(np.sort(values)[len(values) // 2]), lowest) if len(values) else lowest
            reached[algo] = (int(V[inside].min()), int(V[inside].max()))
            for cut, window in ((lowest, 0), (median, Q)):
                want = expected(V, R, lengths, cut, window)
                where = f"{axis}={v} Q={Q} {form} {algo} cut {cut} window {window}"
                got = db.search_occurrences(q, matrix, *gaps(m), algo, min_score=cut, window=window)
                assert db.last_occurrence_routing()[3] == (Q + 63) // 64, where
                assert_answer(got, want, where)
                assert_answer(db.search_occurrences_pssm(rows, *gaps(m), algo, min_score=cut, window=window), want, "pssm " + where)
                if window == 0 and algo == "hw":
                    assert got["count"] == lengths.sum(), where
                assert got["count"] > 0, where
    print(f"INT32EDGE occurrences Q={Q} axis={axis} last_admitted={v} (lowest, highest) column value={reached}")


# ---- f. the stage behind the sweeps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["hw", "sw"])
@pytest.mark.parametrize("axis", ["match", "open=ext"])
@pytest.mark.parametrize("Q", [33, 130])
def test_occurrence_alignments(capi, dbs, Q, axis, algo):
    """where every occurrence starts, and its operations, against the witness of tests/_occurrence_alignments.py; the
    cut leaves the few hundred highest columns, window 0"""
    q, seqs, res, off = inputs("random", Q)
    db = dbs("random", Q)
    v = probe("search_occurrence_alignments", axis, Q,
              lambda m: db.search_occurrence_alignments(q, _edges.model_matrix(m), *gaps(m), "hw", min_score=INT_MAX, window=0))
    assert v == search_probe(dbs, axis, Q)
    m = _edges.int32_model(axis, v)
    matrix = _edges.model_matrix(m)
    rows = matrix.reshape(A, A)[q]
    V, R, lengths, inside = witness("random", Q, axis, v, algo)
    values = np.sort(V[inside] if algo == "hw" else V[inside & (V >= 1)])[::-1]
    cut = int(values[min(300, len(values) - 1)])
    want = expected(V, R, lengths, cut, 0)
    assert 200 <= len(want["target"]) <= 3000, (axis, Q, algo, cut, len(want["target"]))
    got = db.search_occurrence_alignments(q, matrix, *gaps(m), algo, min_score=cut, window=0)
    where = f"aligned {axis}={v} Q={Q} {algo} cut {cut}"
    assert got["count"] == len(want["target"]), where
    for key in ("target", "score", "end_t", "end_q"):
        assert np.array_equal(got[key], want[key]), (where, key)
    occ = list(zip(got["target"].tolist(), got["score"].tolist(), got["end_t"].tolist(), got["end_q"].tolist()))
    start_t, start_q = starts(rows, seqs, occ, *gaps(m), algo)
    assert np.array_equal(got["start_t"], start_t), (where, np.flatnonzero(got["start_t"] != start_t)[:8])
    assert np.array_equal(got["start_q"], start_q), (where, np.flatnonzero(got["start_q"] != start_q)[:8])
    ops = operations(q, matrix, seqs, occ, start_t, start_q, *gaps(m))
    assert np.array_equal(np.diff(got["aln_off"]), [len(o) for o in ops]), where
    assert np.array_equal(got["aln_flat"], np.concatenate(ops)), where
    routing = db.last_occurrence_align_routing()
    assert routing[0] + routing[1] == got["count"] and routing[2] >= 1, (where, routing)
    print(f"INT32EDGE occurrence alignments Q={Q} axis={axis} algo={algo} last_admitted={v} cut={cut} occurrences={got['count']} "
          f"longest span={routing[3]} routing={routing}")
