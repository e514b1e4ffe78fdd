"""The windowed views of long targets against the checker at every seam (planWindows in host_search.inc, buildView
in host_view.inc, the pack / scatter / decode kernels of pack.hip).

Every test reads what its searches ran under from last_window_plan() - (overlap, stride of the view, entries of the
view, merged by key) - asserts it, and derives its lengths and offsets from that overlap O and stride S. The plan of a
query depends on the query, the scores and the gap model (O) and on the size of the slice (S), not on the residues:
`probe` reads it off a small database first, the test builds its database for it and asserts that its own searches
report the same. Every comparison is bit for bit, against the scalar checker or, for whole large databases, the
AVX2 baseline. tests/test_windows_cpu.py holds the inputs (tests/_windows.py) to their purpose."""
import numpy as np
import pytest

import _cpu_baseline
import _data
import _oracle
import _pssm
import _windows as W
import pyopal_amd

pytestmark = pytest.mark.gpu

B62 = W.B62
ALGOS = ["sw", "hw"]
SWITCH = "MIOPAL_TEST_WINDOW_STRIDE"
QUERY = _data.random_protein(np.random.default_rng(5), 24)   # (the query of test_windows_cpu.py)


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def widest():
    return W.widest_join(7, QUERY, B62, (1, 1))


def plain(q, matrix, gaps, algo):
    """a search of (q, matrix) as a function of (handle, mode, start, end)"""
    return lambda db, mode, start=0, end=None: db.search(q, matrix, gaps[0], gaps[1], mode, algo, start, end)


def probe(capi, run, alphabet=24):
    """(overlap, stride) of the windows `run` is searched in, read off a small database with one long target"""
    rng = np.random.default_rng(0)
    seqs = [rng.integers(0, min(alphabet, 20), size=n).astype(np.uint8) for n in [30_000] + [50] * 40]
    res, off = _oracle.flatten(seqs)
    db = capi.DeviceDatabase(res, off, alphabet)
    try:
        run(db, "score")
        O, S = capi.DeviceDatabase.last_window_plan()[:2]
    finally:
        db.close()
    assert O > 0 and S >= W.segment_stride(O) and S % 256 == 0, f"no windows: plan {(O, S)}"
    print(f"plan of the probe: overlap {O}, stride {S}")
    return O, S


def check(capi, db, run, ref, seqs, O, S, modes=("score", "end", "full"), start=0, end=None, tag=""):
    """`run` in each mode against the rows [start, end) of the checker's `full` result `ref`, and the plan of each"""
    end = len(seqs) if end is None else end
    lengths = [len(t) for t in seqs[start:end]]
    for mode in modes:
        got = run(db, mode, start, end)
        plan = capi.DeviceDatabase.last_window_plan()
        assert plan == (O, S, W.entries(lengths, O, S), int(mode != "score")), (tag, mode, plan, (O, S))
        keys = {"score": ["score"], "end": ["score", "end_t", "end_q"], "full": list(ref)}[mode]
        want = {k: ref[k][start:end] for k in keys}
        _pssm.assert_same(got, want, (tag, mode, plan))


def reference(q, seqs, matrix, gaps, algo, mode="full"):
    res, off = _oracle.flatten(seqs)
    return res, off, _oracle.search(q, res, off, matrix, gaps[0], gaps[1], mode, algo)


# ---- a. length transitions ------------------------------------------------------------------------------------
def run_transitions(capi, algo, O, S, tag):
    seqs, listed = W.transition_db(3, QUERY, O, S)
    res, off, ref = reference(QUERY, seqs, B62, (3, 1), algo)
    assert (ref["score"][:listed] > 0).sum() >= listed - 8, "the planted copies score"
    db = capi.DeviceDatabase(res, off, 24)
    try:
        check(capi, db, plain(QUERY, B62, (3, 1), algo), ref, seqs, O, S, tag=tag)
    finally:
        db.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_length_transitions(capi, algo):
    """one target of each length at which the number of windows or the last window's length changes - W - 1, W,
    W + 1, S + O + S / 2, k S + O, k S + O + 1 - and of 0, 1, 2 and O + 1 residues, a hit ending on the last column
    (first set) and starting on the first (second set), among 150 short targets: score, end, full and the number of
    view entries"""
    O, S = probe(capi, plain(QUERY, B62, (3, 1), algo))
    run_transitions(capi, algo, O, S, f"transitions {algo}")


# ---- b. seam sweep -------------------------------------------------------------------------------------------------
def run_seams(capi, algo, g, gaps, O, S, tag, full_every=1):
    seqs, aims = W.seam_db(7, QUERY[:12], QUERY[12:], g, O, S)
    res, off, ref = reference(QUERY, seqs, B62, gaps, algo)
    assert W.covers(ref, aims).all() and (ref["end_t"] - ref["start_t"] + 1 == len(QUERY) + g).all(), tag
    db = capi.DeviceDatabase(res, off, 24)
    try:
        run = plain(QUERY, B62, gaps, algo)
        check(capi, db, run, ref, seqs, O, S, modes=("score", "end") if full_every > 1 else ("score", "end", "full"), tag=tag)
        if full_every > 1:
            for k in range(0, len(seqs), full_every):
                check(capi, db, run, ref, seqs, O, S, modes=("full",), start=k, end=k + 1, tag=f"{tag} target {k}")
    finally:
        db.close()


@pytest.mark.parametrize("gap", ["none", "forty", "widest"])
@pytest.mark.parametrize("algo", ALGOS)
def test_seam_sweep(capi, widest, algo, gap):
    """the two halves of the query with g unrelated residues between them, at every offset that puts the alignment's
    last column on k S + O - 3 .. k S + O + 2 (the last column of window k - 1 is k S + O - 1), its first column on
    k S - 3 .. k S + 2 (window k starts at k S), and its last column there, k = 1, 2; g = 0, 40 and the widest gap
    the checker joins under gaps (1, 1)"""
    g, gaps = {"none": (0, (3, 1)), "forty": (40, (1, 1)), "widest": (widest, (1, 1))}[gap]
    O, S = probe(capi, plain(QUERY, B62, gaps, algo))
    run_seams(capi, algo, g, gaps, O, S, f"seams {algo} g={g}")


# ---- c. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(W.TIE_KINDS))
@pytest.mark.parametrize("algo", ALGOS)
def test_ties_across_windows(capi, algo, kind):
    """targets whose optimum is reached in two windows, in different cells: the merge reports the smallest column,
    then the smallest row, whichever window it is in - the checker's first maximum. 200 random targets of few letters
    and a short query (at least 20 of them hold such a tie under the reported windows), and targets with the exact
    query two and three times, no window holding two copies: the first copy is the answer. Scores alone
    (the TAKE_MAX scatter) equal the same scores."""
    k = W.TIE_KINDS[kind]
    q = W.tie_db(kind)[0]
    O, S = probe(capi, plain(q, k["matrix"], W.TIE_GAPS, algo), k["alphabet"])
    q, seqs, matrix, alphabet, built = W.tie_db(kind, window=O + S)
    per = W.window_results(q, seqs, matrix, W.TIE_GAPS, algo, O, S)
    ties = W.cross_window_ties(per)
    assert len([t for t in ties if t < 200]) >= 20 and set(built) <= set(ties), (len(ties), (O, S))
    res, off, ref = reference(q, seqs, matrix, W.TIE_GAPS, algo)
    for t, first in built.items():
        assert ref["end_t"][t] == first and ref["end_q"][t] == len(q) - 1
    db = capi.DeviceDatabase(res, off, alphabet)
    try:
        run = plain(q, matrix, W.TIE_GAPS, algo)
        check(capi, db, run, ref, seqs, O, S, tag=f"ties {kind} {algo}")
        end = run(db, "end")
        wrong = [t for t in ties if (end["end_t"][t], end["end_q"][t]) != W.merged(per[t])[1:]]
        assert not wrong, f"targets {wrong[:8]}: not the first of the tied cells"
        for t, first in built.items():
            assert end["end_t"][t] == first, f"target {t}: copy ending at {end['end_t'][t]}, the first ends at {first}"
    finally:
        db.close()


# ---- d. strides -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [512, 1024, 4096, 8192])
@pytest.mark.parametrize("algo", ALGOS)
def test_strides(capi, tuning, algo, stride):
    """the strides the planner only chooses for databases of 1e8 .. 2e9 residues, set through the test switch: the
    length transitions and the seam aims over again, relative to the stride the plan reports (targets of up to
    3 S + O + 1 residues: at 8192 a dozen of them are cut)"""
    tuning.setenv(SWITCH, str(stride))
    O, S = probe(capi, plain(QUERY, B62, (3, 1), algo))
    assert S == stride
    run_transitions(capi, algo, O, S, f"transitions {algo} stride {stride}")
    run_seams(capi, algo, 0, (3, 1), O, S, f"seams {algo} stride {stride}", full_every=4)
    O1, S1 = probe(capi, plain(QUERY, B62, (1, 1), algo))
    assert S1 == stride
    run_seams(capi, algo, 40, (1, 1), O1, S1, f"seams {algo} stride {stride} g=40", full_every=4)


@pytest.mark.parametrize("algo", ALGOS)
def test_views_of_two_strides_on_one_handle(capi, tuning, algo):
    """the view cache is keyed by (start, end, overlap, stride): two strides and a sub-slice in turn on one handle,
    each search on a view of the stride it asked for"""
    O, S0 = probe(capi, plain(QUERY, B62, (3, 1), algo))
    seqs, listed = W.transition_db(3, QUERY, O, 1024)
    seqs = seqs[:40] + W.transition_db(4, QUERY, O, 512, fillers=0)[0]
    res, off, ref = reference(QUERY, seqs, B62, (3, 1), algo)
    db = capi.DeviceDatabase(res, off, 24)
    run = plain(QUERY, B62, (3, 1), algo)
    try:
        for stride, (start, end) in [(512, (0, None)), (1024, (0, None)), (512, (3, 30)), (1024, (3, 30)),
                                     (None, (3, 30)), (512, (0, None)), (1024, (3, 30)), (None, (0, None))]:
            if stride is None:
                tuning.delenv(SWITCH)
            else:
                tuning.setenv(SWITCH, str(stride))
            check(capi, db, run, ref, seqs, O, stride or S0, modes=("end", "score"), start=start, end=end,
                  tag=f"stride {stride} slice {(start, end)}")
    finally:
        db.close()


@pytest.mark.parametrize("value", ["300", "16384", "128", "0", "-512", "512k"])
def test_an_invalid_stride_is_ignored(capi, tuning, value):
    """not a multiple of 256, above 8192, below the overlap's shortest stride, not a number: the planner's own"""
    run = plain(QUERY, B62, (3, 1), "sw")
    O, S0 = probe(capi, run)
    tuning.setenv(SWITCH, value)
    assert probe(capi, run) == (O, S0)


def test_the_switch_never_turns_windows_on(capi, tuning):
    """a search that is not cut (no target beyond the window) stays whole under the switch"""
    tuning.setenv(SWITCH, "512")
    seqs = W.transition_db(3, QUERY, 256, 256)[0][-150:]   # (the short fillers)
    res, off, ref = reference(QUERY, seqs, B62, (3, 1), "sw", "end")
    db = capi.DeviceDatabase(res, off, 24)
    try:
        got = db.search(QUERY, B62, 3, 1, "end", "sw")
        assert capi.DeviceDatabase.last_window_plan() == (0, 0, 0, 0)
        _pssm.assert_same(got, ref, "whole targets")
    finally:
        db.close()


# ---- e. the planner's own enlarged stride ---------------------------------------------------------------------------
def test_the_planners_enlarged_stride(capi):
    """16 000 targets of 7000 residues, 1.1e8 in all: planWindows enlarges the stride itself (no switch). Every
    score against the AVX2 baseline; end locations of 64 targets with the query planted on the reported seams
    against the scalar checker."""
    n, L = 16_000, 7000
    rng = np.random.default_rng(8)
    q = _data.random_protein(rng, 8)
    res = _data.AA20_CODES[rng.integers(0, 20, size=n * L, dtype=np.uint8)]
    off = np.arange(n + 1, dtype=np.int64) * L
    db = capi.DeviceDatabase(res, off, 24)
    try:
        db.search(q, B62, 3, 1, "score", "sw")
        plan = capi.DeviceDatabase.last_window_plan()
    finally:
        db.close()
    O, S = plan[:2]
    print(f"plan of {n * L} residues: {plan}")
    assert O > 0 and S > W.segment_stride(O) and S % 256 == 0, \
        f"the stride of {n * L} residues was not enlarged: plan {plan}, shortest stride {W.segment_stride(O)}"
    # the query on the seams the plan reports: ending on the last column of a window (and one to each side),
    # starting on the first column of the next
    picked = np.arange(64) * (n // 64) + 7
    for x, t in enumerate(picked):
        k = 1 + x % ((L - O) // S - 1)
        at = [k * S + O - 1 - len(q), k * S + O - len(q), k * S + O + 1 - len(q), k * S - 1, k * S, k * S + 1][x % 6]
        res[off[t] + at:off[t] + at + len(q)] = q
    db = capi.DeviceDatabase(res, off, 24)
    try:
        sres, soff = _oracle.flatten([res[off[t]:off[t + 1]] for t in picked])
        cpu = _cpu_baseline.CpuDatabase(res, off)
        for algo in ALGOS:
            want = cpu.search(q, B62, 3, 1, algo, 8)
            ref = _oracle.search(q, sres, soff, B62, 3, 1, "end", algo)
            assert (ref["score"] == ref["score"].max()).all(), "the planted copies are the optima"
            got = db.search(q, B62, 3, 1, "score", algo)["score"]
            plan = capi.DeviceDatabase.last_window_plan()
            # (HW has an overlap of its own, and with it a stride of its own)
            assert plan[0] > 0 and plan[1] > W.segment_stride(plan[0]) and plan[1] % 256 == 0, (algo, plan)
            assert plan[2:] == (n * len(W.windows(L, *plan[:2])), 0) and (algo == "hw" or plan[:2] == (O, S)), (algo, plan)
            np.testing.assert_array_equal(got, want, err_msg=f"{algo} scores, plan {plan}")
            end = db.search(q, B62, 3, 1, "end", algo)
            assert capi.DeviceDatabase.last_window_plan() == plan[:3] + (1,)
            np.testing.assert_array_equal(end["score"], want)
            for key in ("score", "end_t", "end_q"):
                np.testing.assert_array_equal(end[key][picked], ref[key], err_msg=f"{algo} {key}, plan {plan}")
        cpu.close()
    finally:
        db.close()


# ---- f. the fields of the merge key -----------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", ["last", "first and last"])
@pytest.mark.parametrize("algo", ALGOS)
def test_the_column_field_at_its_limit(capi, algo, copies):
    """one target of 2^24 - 1 residues - the longest that is cut - with the query on its last columns: the key's
    24-bit column field holds 2^24 - 1 - (2^24 - 2) = 1. With a second copy at column 0 the first one is reported."""
    L = 2 ** 24 - 1
    rng = np.random.default_rng(1)
    q = _data.random_protein(rng, 8)
    t = _data.AA20_CODES[rng.integers(0, 20, size=L, dtype=np.uint8)]
    t[L - len(q):] = q
    if copies != "last":
        t[:len(q)] = q
    off = np.array([0, L], dtype=np.int64)
    ref = _oracle.search(q, t, off, B62, 3, 1, "end", algo)
    assert ref["end_t"][0] == (L - 1 if copies == "last" else len(q) - 1) and ref["end_q"][0] == len(q) - 1
    db = capi.DeviceDatabase(t, off, 24)
    try:
        for mode in ("end", "score"):
            got = db.search(q, B62, 3, 1, mode, algo)
            plan = capi.DeviceDatabase.last_window_plan()
            assert plan[0] > 0 and plan == plan[:2] + (W.entries([L], *plan[:2]), int(mode == "end")), plan
            _pssm.assert_same(got, ref if mode == "end" else {"score": ref["score"]}, (algo, copies, mode, plan))
    finally:
        db.close()


def test_hw_when_every_score_is_negative(capi):
    """HW keys carry a bias of 2^22 on the score: a database that shares no letter with the query, every score below
    zero, an empty and a one-residue target among the windows"""
    rng = np.random.default_rng(12)
    q = _data.encode("WCGPDN")[rng.integers(0, 6, size=24)]
    O, S = probe(capi, plain(q, B62, (3, 1), "hw"))
    lengths = [0, 1, S + O - 1, S + O, S + O + 1, 2 * S + O + 1, 3 * S + O, 5000] + list(rng.integers(2, 3000, size=150))
    seqs = [_data.encode("ILVMAKERST")[rng.integers(0, 10, size=int(n))] for n in lengths]
    res, off, ref = reference(q, seqs, B62, (3, 1), "hw")
    assert ref["score"].max() < 0
    db = capi.DeviceDatabase(res, off, 24)
    try:
        check(capi, db, plain(q, B62, (3, 1), "hw"), ref, seqs, O, S, tag="hw, negative scores")
    finally:
        db.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_scores_beyond_the_16_bit_lanes(capi, algo):
    """mismatches of -30 000 under a query of 32: where the search is cut into windows, lanes leave the 16-bit
    range and their targets are redone whole; either way the answers are the checker's"""
    rng = np.random.default_rng(13)
    matrix = np.where(np.eye(24, dtype=bool), 5, -30_000).astype(np.int32).ravel()
    q = _data.random_protein(rng, 32)
    seqs = [_data.random_protein(rng, int(n)) for n in list(rng.integers(700, 3000, size=24)) + list(rng.integers(1, 400, size=150))]
    for t in seqs[:24:2]:
        at = int(rng.integers(0, len(t) - 40))
        copy = _data.mutate(rng, q, 0.1)
        t[at:at + len(copy)] = copy
    res, off, ref = reference(q, seqs, matrix, (3, 1), algo)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for mode in ("score", "end", "full"):
            got = db.search(q, matrix, 3, 1, mode, algo)
            plan, routing = capi.DeviceDatabase.last_window_plan(), capi.DeviceDatabase.last_routing()
            what = f"{algo} {mode}: plan {plan}, routing {routing}"
            if plan[0] > 0:
                assert plan[2] == W.entries([len(t) for t in seqs], *plan[:2]), what
                assert algo == "sw" or routing[3] > 0 or routing[0] > 0, "windows, and no lane redone: " + what
            keys = {"score": ["score"], "end": ["score", "end_t", "end_q"], "full": list(ref)}[mode]
            _pssm.assert_same(got, {k: ref[k] for k in keys}, what)
    finally:
        db.close()


# ---- g. the entry points that share the score pass ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_set(capi):
    """the seam database of (b), g = 40 under gaps (1, 1), among 400 short targets (the selections have something
    to leave out), with the checker's rows"""
    run = plain(QUERY, B62, (1, 1), "sw")
    O, S = probe(capi, run)
    seqs, aims = W.seam_db(7, QUERY[:12], QUERY[12:], 40, O, S)
    rng = np.random.default_rng(21)
    seqs = seqs + [_data.random_protein(rng, int(n)) for n in rng.integers(30, 600, size=400)]
    res, off = _oracle.flatten(seqs)
    refs = {algo: _oracle.search(QUERY, res, off, B62, 1, 1, "end", algo) for algo in ALGOS}
    db = capi.DeviceDatabase(res, off, 24)
    yield db, seqs, refs, (O, S)
    db.close()


def windowed(capi, seqs, mode="end"):
    plan = capi.DeviceDatabase.last_window_plan()
    assert plan[0] > 0 and plan[2] == W.entries([len(t) for t in seqs], *plan[:2]) and plan[3] == int(mode != "score"), plan
    return plan


@pytest.mark.parametrize("algo", ALGOS)
def test_top_hits_over_windows(capi, seam_set, algo):
    db, seqs, refs, _ = seam_set
    ref = refs[algo]
    got = db.search_top(QUERY, B62, 1, 1, "end", algo, k=10)
    windowed(capi, seqs)
    order = np.lexsort((np.arange(len(seqs)), -ref["score"].astype(np.int64)))[:10]
    assert got["count"] == 10 and np.array_equal(got["target"], order)
    for key in ("score", "end_t", "end_q"):
        np.testing.assert_array_equal(got[key], ref[key][order], err_msg=key)


@pytest.mark.parametrize("algo", ALGOS)
def test_hits_over_windows(capi, seam_set, algo):
    db, seqs, refs, _ = seam_set
    ref = refs[algo]
    cut = int(np.sort(ref["score"])[-len(seqs) // 10])   # keeps about a tenth
    keep = np.flatnonzero(ref["score"] >= cut)
    assert 36 <= len(keep) <= len(seqs) // 5
    got = db.search_hits(QUERY, B62, 1, 1, "end", algo, min_score=cut)
    windowed(capi, seqs)
    assert got["count"] == len(keep) and np.array_equal(got["target"], keep)
    for key in ("score", "end_t", "end_q"):
        np.testing.assert_array_equal(got[key], ref[key][keep], err_msg=key)


@pytest.mark.parametrize("algo", ALGOS)
def test_significant_hits_over_windows(capi, seam_set, algo):
    """the planted alignments are the significant ones: the table of thresholds the call reports, applied to the
    checker's rows, and the statistics of every score"""
    db, seqs, refs, _ = seam_set
    ref = refs[algo]
    got = db.search_significant(QUERY, B62, 1, 1, "end", algo, max_evalue=1e-3)
    windowed(capi, seqs)
    fit = pyopal_amd.ScoreFit(got["fit"])
    lengths = np.array([len(t) for t in seqs], dtype=np.int64)
    bins = np.asarray(capi.length_bins(lengths), dtype=np.int64)
    score = ref["score"].astype(np.int64)
    for b in np.unique(bins):
        s = score[bins == b]
        assert tuple(fit.all[b]) == (len(s), s.sum(), (s * s).sum()), b
    keep = np.flatnonzero(score >= fit.thresholds[bins].astype(np.int64))
    assert got["count"] == len(keep) and np.array_equal(got["target"], keep)
    for key in ("score", "end_t", "end_q"):
        np.testing.assert_array_equal(got[key], ref[key][keep], err_msg=key)


@pytest.mark.parametrize("algo", ALGOS)
def test_pssm_over_windows(capi, algo):
    """a PSSM of 24 positions drawn from 32 row classes is a search over a 32-letter alphabet (tests/_pssm.py): the
    seam database over those letters, each position's best residue planted (g = 0 under gaps (3, 1): at a gap
    cost of 1 a column the random rows of a class PSSM align the unrelated residues as well as the planted ones)"""
    rng = np.random.default_rng(31)
    classes, table, rows = _pssm.class_pssm(rng, 24)
    best = rows.argmax(axis=1).astype(np.uint8)

    def run(db, mode, start=0, end=None):
        return db.search_pssm(rows, classes, 3, 1, mode, algo, start, end)

    O, S = probe(capi, run, _pssm.A32)
    seqs, aims = W.seam_db(7, best[:12], best[12:], 0, O, S, letters=lambda r, n: r.integers(0, _pssm.A32, size=n).astype(np.uint8))
    res, off, ref = reference(classes, seqs, table, (3, 1), algo)
    assert W.covers(ref, aims).all() and (ref["end_t"] - ref["start_t"] + 1 == len(classes)).all()
    db = capi.DeviceDatabase(res, off, _pssm.A32)
    try:
        check(capi, db, run, ref, seqs, O, S, tag=f"pssm {algo}")
    finally:
        db.close()
