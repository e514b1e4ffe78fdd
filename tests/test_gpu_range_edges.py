"""NW / HW / OV at the edges of the static range rules, bit for bit against the CPU checker through the C ABI.

Whether a scoring model (and, in the general kernel, a target length) may run on 16-bit patterns is decided before the
launch by inequalities (score_ranges.h: globalOneStripFits, globalStripsFit, fitsPlain, fitsDiag, fitsUnsigned,
unsignedDiagUsable; perpair_packed.hip: packedScanFits, packedTraceFits). Nothing is flagged afterwards and nothing is
redone: a rule a few units too generous returns wrong scores in silence. Every test here

  * asks the ROUTER for the last value it admits (tests/_edges.py, last_admitted: a bisection over one parameter on
    the routing word) - a rule that has stopped deciding anything fails the probe,
  * runs the edge family (tests/_edges.py: copies of the query for the top of the range, runs of the lowest-scoring
    letter for the bottom) at that value, one beyond it and one before it, and asserts the routing word each time.

A small search sends leading groups of 128 targets whose longest has more than 512 columns to the wavefront-per-pair
kernel (planSideCut): the family's `long` members are checked there, and the same members at 512 columns
(_edges.lanes_members) meet the kernel under test. Each test prints its thresholds (lines that start with EDGE);
profiles/range_edges.txt holds those of one run.
"""
import functools

import numpy as np
import pytest

import _edges
import _oracle
from _edges import ALPHABET as A
from pyopal_amd.matrices import ScoringMatrix
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
ONE_STRIP, STRIPS = 2 + 3, 2 + 5           # miopalLastRouting counts[1] & 31: the pair-table kernels of NW / HW / OV
FLAVOUR = {"plain": 2, "diag": 4, "unsigned": 5}   # counts[1] = 1 + 32 * flavour: the general kernel's lane arithmetic
PACKED_TRACE, PACKED_SCAN = 64, 128        # miopalLastFullRouting
ALGOS = ["nw", "hw", "ov"]
AXES = list(_edges.AXES)


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture
def strips(tuning):
    tuning.setenv("MIOPAL_PAIR_STRIPS", "1")


@pytest.fixture
def lane_per_pair(tuning):
    tuning.setenv("MIOPAL_NO_SMALL_SEARCH", "1")
    tuning.setenv("MIOPAL_NO_HYBRID_TRACE", "1")
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")


def word(capi):
    return capi.DeviceDatabase.last_routing()[1] & 31


@functools.lru_cache(maxsize=None)
def edge_db(form, Q, long=_edges.LONG, lanes=True):
    """(query, residues, offsets) of the edge family, with its long members once more at 512 columns and the targets
    beyond 512 columns as whole groups (module docstring). Shared by the tests; nobody writes to it."""
    q = _edges.edge_query(form, Q)
    seqs = _edges.family(q, long=long)
    if lanes:
        seqs = _edges.whole_groups(seqs + _edges.lanes_members(q))
    res, off = _oracle.flatten(seqs)
    for a in (q, res, off):
        a.setflags(write=False)
    return q, res, off


def checker(q, res, off, matrix, go, ge, mode, algo):
    return _oracle.search_parallel(q, res, off, matrix, go, ge, mode, algo, threads=8, chunk=24)


def exact(got, want, mode, tag):
    for key in ("score",) + (("end_q", "end_t") if mode == "end" else ()):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {tag}")


def probe_axis(capi, Q, axis, algo, mode, kernel):
    """The last value of `axis` for which a tiny search of this query length runs `kernel`."""
    q = _edges.edge_query("random", Q)
    res, off = _oracle.flatten([q, _edges.pc(5)])
    db = capi.DeviceDatabase(res, off, A)

    def search(v):
        m = _edges.axis_model(axis, v)
        db.search(q, _edges.model_matrix(m), m["open"], m["ext"], mode, algo)
        return word(capi) == kernel
    try:
        _, lo, hi = _edges.AXES[axis]
        return _edges.last_admitted(search, lo, hi)
    finally:
        db.close()


def run_models(capi, Q, algo, mode, kernel, runs, tag):
    """runs: (model, whether the kernel under test must run). Every form of the query against its family."""
    stayed = []
    for form in _edges.QUERY_FORMS:
        q, res, off = edge_db(form, Q)
        db = capi.DeviceDatabase(res, off, A)
        try:
            for m, admitted in runs:
                matrix = _edges.model_matrix(m)
                got = db.search(q, matrix, m["open"], m["ext"], mode, algo)
                routed = capi.DeviceDatabase.last_routing()
                where = f"{tag} {algo} {mode} {form} {m}"
                assert ((routed[1] & 31) == kernel) == admitted, f"{where}: routing {routed}"
                exact(got, checker(q, res, off, matrix, m["open"], m["ext"], mode, algo), mode, where)
                if admitted:
                    assert routed[2] >= 1, f"{where}: no group stayed in the lanes {routed}"
                    stayed.append((routed[0], routed[2]))
        finally:
            db.close()
    return stayed


def edge_cell(capi, Q, axis, algo, mode, kernel, name):
    v = probe_axis(capi, Q, axis, algo, mode, kernel)
    runs = [(_edges.axis_model(axis, v), True), (_edges.axis_model(axis, v + 1), False),
            (_edges.axis_model(axis, v - 1), True)]
    if axis == "open" and algo == "nw":
        # the topGap clause: NW's top border is no constant on the kernel's scale when opening is cheaper than extending
        runs += [(dict(_edges.BASE, open=1, ext=1), True), (dict(_edges.BASE, open=0, ext=1), False)]
    stayed = run_models(capi, Q, algo, mode, kernel, runs, f"{name} Q={Q} {axis}={v}")
    print(f"EDGE {name} Q={Q} axis={axis} algo={algo} mode={mode} last_admitted={v} (side targets, groups in lanes)={stayed[0]}")


# ---- a. the one-strip pair-table kernel (globalOneStripFits) -----------------------------------------------------
@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", _edges.ONE_STRIP_Q)
def test_one_strip_pair_table(capi, Q, axis, algo, mode):
    edge_cell(capi, Q, axis, algo, mode, ONE_STRIP, "one-strip")


# ---- b. the multi-strip pair-table kernel (globalStripsFit) ------------------------------------------------------
@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("Q", _edges.STRIPS_Q)
def test_strips_pair_table(capi, strips, Q, axis, algo, mode):
    edge_cell(capi, Q, axis, algo, mode, STRIPS, "strips")


W, C, D = 17, 4, 3   # BLOSUM62: W-W 11 (its maximum), C-C 9, W-D -4 (its minimum)


COPIES = 128   # of every target: the groups of 128 targets of the length-sorted view then hold one length each


@pytest.mark.parametrize("algo", ALGOS)
def test_strips_longest_query(capi, strips, algo):
    # The last query length the strips kernel takes under BLOSUM62 11 / 1, and one beyond it, against 60 targets of the
    # family (long = 600; the query and the query with 2 % of its residues changed among them). At that length the
    # quantity at the limit is Q * max S, so the copy of the query has to meet the strips kernel - and a search of 60
    # targets would send every target of more than 512 columns to the wavefront-per-pair kernel (planSideCut). Each
    # target is therefore in the database 128 times: the cut's estimate then keeps all but the longest groups, the side
    # kernel takes a prefix of the length-sorted view, and counts[0] bounds it: nothing as short as the query leaves.
    # (The checker runs the 60 once.)
    assert (B62.reshape(A, A)[W, W], B62.reshape(A, A)[W, D]) == (B62.max(), B62.min())
    rng = np.random.default_rng(41)
    tiny = _oracle.flatten([_edges.edge_query("random", 100, letters=(W, C)), _edges.pc(5, D)])
    db = capi.DeviceDatabase(*tiny, A)

    def search(v):
        db.search(_edges.edge_query("one", v, letters=(W, C)), B62, 11, 1, "score", algo)
        return word(capi) == STRIPS
    try:
        longest = _edges.last_admitted(search, 65, 4000)
    finally:
        db.close()
    print(f"EDGE strips axis=Q algo={algo} mode=score BLOSUM62 11/1 last_admitted={longest}")
    for form in ("one", "random"):
        for Q, admitted in ((longest, True), (longest + 1, False)):
            q = _edges.edge_query(form, Q, letters=(W, C))
            changed = q.copy()
            changed[rng.choice(Q, size=Q // 50, replace=False)] = D
            seqs = _edges.family(q, c=D, long=600, n_random=44, max_random=_edges.STAYS, letters=(W, C)) + [changed]
            assert len(seqs) == 60
            want = checker(q, *_oracle.flatten(seqs), B62, 11, 1, "score", algo)["score"]
            if admitted:
                top = Q * int(B62.max()) if form == "one" else None
                assert want[0] == want.max() and (top is None or want[0] == top), (form, Q, want[0])
            res, off = _oracle.flatten(seqs * COPIES)
            db = capi.DeviceDatabase(res, off, A)
            try:
                got = db.search(q, B62, 11, 1, "score", algo)
                routed = capi.DeviceDatabase.last_routing()
            finally:
                db.close()
            assert ((routed[1] & 31) == STRIPS) == admitted, (form, Q, routed)
            if admitted:
                # the query, its changed copy and the run of Q low letters are in the lanes of the strips kernel
                longer = sum(1 for t in seqs if len(t) > Q)
                print(f"EDGE strips axis=Q algo={algo} form={form} Q={Q} side targets={routed[0]} of {len(seqs) * COPIES}, "
                      f"longer than the query={longer * COPIES}, groups in lanes={routed[2]}")
                assert routed[0] <= longer * COPIES, (form, Q, routed, longer)
            np.testing.assert_array_equal(got["score"], np.tile(want, COPIES), err_msg=f"{algo} {form} Q={Q} {routed}")


# ---- c. the general kernel's three int16 flavours (fitsPlain, fitsDiag, fitsUnsigned) ---------------------------
@pytest.fixture
def general(tuning):
    tuning.setenv("MIOPAL_NO_PAIR_TABLE", "1")
    tuning.setenv("MIOPAL_NO_GLOBAL_STRIPS", "1")
    # (HW would take its long targets as windows of a few hundred columns, none beyond a flavour's range: whole here)
    tuning.setenv("MIOPAL_NO_SEGMENTS", "1")


def general_db(q, lengths=()):
    """The family with every target within 512 columns (no group leaves for its length: counts[0] then counts the
    targets beyond the flavour's range alone), and two targets of each of `lengths`: a run of the low letter, and one
    that holds the query (or its first residues)."""
    Q = len(q)
    seqs = _edges.family(q, long=_edges.STAYS - Q)
    for L in lengths:
        seqs += [_edges.pc(L), np.concatenate([_edges.pc(L - Q), q]).astype(np.uint8) if L >= Q else q[:L].copy()]
    assert max(len(s) for s in seqs) <= _edges.STAYS
    return seqs


def flavour_cases():
    return [pytest.param(flavour, Q, m, id=f"{flavour}-{tag}") for flavour, models in _edges.GENERAL_MODELS.items()
            for tag, Q, m in models]


@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("flavour,Q,m", flavour_cases())
def test_general_kernel_longest_packed_target(capi, general, tuning, flavour, Q, m, algo, mode):
    if flavour == "plain":
        tuning.setenv("MIOPAL_NO_DIAG_SHIFT", "1")
    matrix = _edges.model_matrix(m)
    q = _edges.edge_query("random", Q)
    three = np.array([_edges.LETTER_A, _edges.LETTER_B, _edges.LETTER_C], dtype=np.uint8)
    rng = np.random.default_rng(43)
    # lengths 1 .. 512, one target each: counts[0] = the targets beyond the longest that stays packed
    steps = [three[rng.integers(0, 3, size=L)] for L in range(1, _edges.STAYS + 1)]
    res, off = _oracle.flatten(steps)
    db = capi.DeviceDatabase(res, off, A)
    try:
        got = db.search(q, matrix, m["open"], m["ext"], mode, algo)
        routed = capi.DeviceDatabase.last_routing()
    finally:
        db.close()
    assert routed[1] == 1 + 32 * FLAVOUR[flavour], routed
    exact(got, checker(q, res, off, matrix, m["open"], m["ext"], mode, algo), mode, f"{flavour} steps {routed}")
    assert 0 < routed[0] < _edges.STAYS, f"the flavour's rule decides nothing within 512 columns: {routed}"
    longest = _edges.STAYS - routed[0]
    print(f"EDGE general flavour={flavour} Q={Q} algo={algo} mode={mode} model={m} longest_packed={longest}")
    for form in _edges.QUERY_FORMS:
        q = _edges.edge_query(form, Q)
        seqs = general_db(q, [L for L in range(longest - 2, longest + 3) if 0 < L <= _edges.STAYS])
        res, off = _oracle.flatten(seqs)
        beyond = sum(1 for s in seqs if len(s) > longest)
        db = capi.DeviceDatabase(res, off, A)
        try:
            got = db.search(q, matrix, m["open"], m["ext"], mode, algo)
            routed = capi.DeviceDatabase.last_routing()
            assert routed[1] == 1 + 32 * FLAVOUR[flavour] and routed[0] == beyond, (form, mode, routed, beyond)
            exact(got, checker(q, res, off, matrix, m["open"], m["ext"], mode, algo), mode, f"{flavour} {form} L*={longest}")
        finally:
            db.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_general_kernel_stays_packed_where_the_rule_admits_everything(capi, general, tuning, algo):
    # match 500: min(Q, L) * match is 31500 at Q = 63 for every target (64 rows: 32000 from L = 64 on, above)
    tuning.setenv("MIOPAL_NO_DIAG_SHIFT", "1")
    m = dict(match=500, mild=-1, low=-4, open=3, ext=1)
    matrix = _edges.model_matrix(m)
    for form in _edges.QUERY_FORMS:
        q = _edges.edge_query(form, 63)
        res, off = _oracle.flatten(general_db(q, [62, 63, 64, 65]))
        db = capi.DeviceDatabase(res, off, A)
        try:
            for mode in ("score", "end"):
                got = db.search(q, matrix, 3, 1, mode, algo)
                routed = capi.DeviceDatabase.last_routing()
                assert routed[1] == 1 + 32 * FLAVOUR["plain"] and routed[0] == 0, routed
                exact(got, checker(q, res, off, matrix, 3, 1, mode, algo), mode, f"Q=63 match 500 {form}")
        finally:
            db.close()


@pytest.mark.parametrize("ext,low", [(60, -180), (200, -600), (820, -2460), (200, -4), (600, -4)])
@pytest.mark.parametrize("Q", [2, 33])
def test_hw_windows_beside_targets_beyond_the_shifted_flavours(capi, tuning, Q, ext, low):
    # HW cuts long targets into windows, and every window stays in the launch: a short target shares its group with
    # windows that a shifted flavour cannot hold, and its lane sweeps their columns. The signed flavour (low = -3 ext
    # keeps the unsigned one out: min + ext + open < 0) takes its last-row maximum over every swept column, its shift
    # (i + j) ext left 16 bits there, and short targets came back as 32767: such a view takes the plain lanes. The
    # unsigned flavour (low = -4) masks the columns beyond a lane's own target and keeps such views.
    tuning.setenv("MIOPAL_NO_PAIR_TABLE", "1")
    tuning.setenv("MIOPAL_NO_GLOBAL_STRIPS", "1")
    m = dict(match=11, mild=-1, low=low, open=ext, ext=ext)
    assert m in [model for _, _, _, model in _edges.shared_models()]
    matrix = _edges.model_matrix(m)
    flavours = ("unsigned",) if low == -4 else ("plain", "diag")
    for form in _edges.QUERY_FORMS:
        q, res, off = edge_db(form, Q)
        db = capi.DeviceDatabase(res, off, A)
        try:
            for mode in ("score", "end"):
                got = db.search(q, matrix, ext, ext, mode, "hw")
                routed = capi.DeviceDatabase.last_routing()
                assert routed[1] in [1 + 32 * FLAVOUR[f] for f in flavours], routed
                exact(got, checker(q, res, off, matrix, ext, ext, mode, "hw"), mode, f"HW windows Q={Q} ext {ext} {form} {routed}")
        finally:
            db.close()


def flavour_run(capi, algo, Q, runs, tag):
    for form in _edges.QUERY_FORMS:
        q = _edges.edge_query(form, Q)
        res, off = _oracle.flatten(general_db(q))
        db = capi.DeviceDatabase(res, off, A)
        try:
            for m, flavour in runs:
                matrix = _edges.model_matrix(m)
                for mode in ("score", "end"):
                    got = db.search(q, matrix, m["open"], m["ext"], mode, algo)
                    routed = capi.DeviceDatabase.last_routing()
                    assert routed[1] == 1 + 32 * FLAVOUR[flavour], (tag, form, m, routed)
                    exact(got, checker(q, res, off, matrix, m["open"], m["ext"], mode, algo), mode, f"{tag} {form} {m}")
        finally:
            db.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_unsigned_flavour_usable_clauses(capi, general, algo):
    # unsignedDiagUsable: open >= ext; min + ext + open >= 0; the room below the zero (probed along `open`)
    base = dict(match=11, mild=-1, low=-4)
    flavour_run(capi, algo, 33, [(dict(base, open=5, ext=5), "unsigned"), (dict(base, open=4, ext=5), "diag")], "open == ext")
    flavour_run(capi, algo, 33, [(dict(base, open=3, ext=1), "unsigned"), (dict(base, low=-5, open=3, ext=1), "diag"),
                                 (dict(base, low=-9, open=5, ext=4), "unsigned"), (dict(base, low=-10, open=5, ext=4), "diag")],
                "min + ext + open == 0")
    q = _edges.edge_query("random", 33)
    db = capi.DeviceDatabase(*_oracle.flatten([q, _edges.pc(5)]), A)

    def search(v):
        db.search(q, _edges.model_matrix(dict(base)), v, 1, "score", algo)
        return capi.DeviceDatabase.last_routing()[1] == 1 + 32 * FLAVOUR["unsigned"]
    try:
        v = _edges.last_admitted(search, 3, 4000)
    finally:
        db.close()
    print(f"EDGE general unsignedDiagUsable room below zero: algo={algo} low=-4 ext=1 last_admitted open={v}")
    flavour_run(capi, algo, 33, [(dict(base, open=v, ext=1), "unsigned"), (dict(base, open=v + 1, ext=1), "diag"),
                                 (dict(base, open=v - 1, ext=1), "unsigned")], "room below zero")


# ---- d. the packed kernels of `full` searches (packedScanFits, packedTraceFits) ---------------------------------
PACKED_AXES = {"match": (11, 300), "open": (3, 300), "low": (4, 1024)}   # as in _edges.AXES, their far ends nearer


def full_search(capi, db, q, m, algo):
    got = db.search(q, _edges.model_matrix(m), m["open"], m["ext"], "full", algo)
    return got, capi.DeviceDatabase.last_full_routing()


def test_nw_has_no_start_cell_scan(capi, lane_per_pair):
    q, res, off = edge_db("random", 64, 400, False)
    db = capi.DeviceDatabase(res, off, A)
    try:
        assert full_search(capi, db, q, _edges.BASE, "nw")[1] & PACKED_SCAN == 0
    finally:
        db.close()


def packed_cases():
    return [pytest.param(algo, bit, id=f"{algo}-{name}") for algo in ("sw", "nw", "hw", "ov")
            for bit, name in ((PACKED_SCAN, "scan"), (PACKED_TRACE, "trace")) if (algo, name) != ("nw", "scan")]


@pytest.mark.parametrize("axis", list(PACKED_AXES))
@pytest.mark.parametrize("algo,bit", packed_cases())
@pytest.mark.parametrize("Q", _edges.PACKED_Q)
def test_packed_full_kernels(capi, lane_per_pair, Q, algo, axis, bit):
    # Which gate decides: the scan's thresholds are packedScanFits' own (score + open + bias within 31, and its range
    # at Q = 130). The trace's, along these three axes, are NOT packedTraceFits': the direction pass needs the byte
    # profile first (host_full.inc: max S + open <= 127, min S + open > -128), which gives match 124, open 116 and low
    # -130 whatever the query and the mode, and under which packedTraceFits' own byte clauses (> 255) cannot fire. Its
    # range clause is probed along ext below (test_packed_trace_range_clause).
    lo, hi = PACKED_AXES[axis]
    for form in _edges.QUERY_FORMS:
        # (the rules read the database's longest target and the batch's windows: probed on the family itself)
        q, res, off = edge_db(form, Q, 400, False)
        db = capi.DeviceDatabase(res, off, A)
        try:
            v = _edges.last_admitted(lambda x: bool(full_search(capi, db, q, _edges.axis_model(axis, x), algo)[1] & bit), lo, hi)
            print(f"EDGE packed {'scan' if bit == PACKED_SCAN else 'trace'} Q={Q} algo={algo} axis={axis} form={form} last_admitted={v}")
            for x, admitted in ((v, True), (v + 1, False), (v - 1, None)):
                m = _edges.axis_model(axis, x)
                got, routing = full_search(capi, db, q, m, algo)
                if admitted is not None:
                    assert bool(routing & bit) == admitted, (form, m, routing)
                ref = _oracle.search(q, res, off, _edges.model_matrix(m), m["open"], m["ext"], "full", algo)
                compare(got, ref, "full", f"{algo} Q={Q} {form} {m} routing {routing}")
        finally:
            db.close()


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
def test_packed_trace_window_times_ext(capi, lane_per_pair, algo):
    # best + (rows + columns) * ext on both sides of the half floats' end: windows of up to 700 columns
    seen = set()
    for Q in _edges.PACKED_Q:
        for form in _edges.QUERY_FORMS:
            q, res, off = edge_db(form, Q, 700 - Q, False)
            db = capi.DeviceDatabase(res, off, A)
            try:
                for ext in (1, 10, 40):
                    m = dict(_edges.BASE, open=ext + 2, ext=ext)
                    got, routing = full_search(capi, db, q, m, algo)
                    seen.add(bool(routing & PACKED_TRACE))
                    if ext == 1:
                        assert routing & PACKED_TRACE, (Q, form, routing)
                    print(f"EDGE packed trace windows Q={Q} algo={algo} form={form} ext={ext} packed={bool(routing & PACKED_TRACE)}")
                    ref = _oracle.search(q, res, off, _edges.model_matrix(m), m["open"], m["ext"], "full", algo)
                    compare(got, ref, "full", f"{algo} Q={Q} {form} ext {ext} routing {routing}")
            finally:
                db.close()
    if algo == "nw":   # (its windows are the whole targets; the other modes: test_packed_trace_range_clause)
        assert seen == {True, False}, seen


TRACE_RANGE_Q = (130, 260)


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("Q", TRACE_RANGE_Q)
def test_packed_trace_range_clause(capi, lane_per_pair, Q, algo):
    # packedTraceFits' range clause, zero + best + (rows + columns) ext + slack <= 0x7BFF, is the one whose error would
    # steer the walk: probed along ext (open = ext + 2) on the family with windows of up to 700 columns, and run at the
    # last admitted ext and one beyond. The byte profile ends at open = 116 (ext 114): a threshold below that is the
    # range clause's, which is asserted where the windows make it certain (NW: the whole targets; 260 rows: any mode).
    for form in _edges.QUERY_FORMS:
        q, res, off = edge_db(form, Q, 700 - min(Q, 130), False)
        db = capi.DeviceDatabase(res, off, A)
        model = lambda ext: dict(_edges.BASE, open=ext + 2, ext=ext)
        try:
            v = _edges.last_admitted(lambda x: bool(full_search(capi, db, q, model(x), algo)[1] & PACKED_TRACE), 1, 120)
            print(f"EDGE packed trace range clause Q={Q} algo={algo} form={form} last_admitted ext={v}")
            if algo == "nw" or Q >= 260:
                assert v < 114, (form, v)
            for x, admitted in ((v, True), (v + 1, False)):
                m = model(x)
                got, routing = full_search(capi, db, q, m, algo)
                assert bool(routing & PACKED_TRACE) == admitted, (form, m, routing)
                ref = _oracle.search(q, res, off, _edges.model_matrix(m), m["open"], m["ext"], "full", algo)
                compare(got, ref, "full", f"{algo} Q={Q} {form} {m} routing {routing}")
        finally:
            db.close()


# ---- e. the same threshold through the PSSM entry point and through a batch -------------------------------------
@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ALGOS)
def test_one_strip_threshold_through_a_pssm(capi, algo, mode):
    Q, axis = 33, "match"
    rows = lambda q, m: _edges.model_matrix(m).reshape(A, A)[q]
    q = _edges.edge_query("random", Q)
    db = capi.DeviceDatabase(*_oracle.flatten([q, _edges.pc(5)]), A)

    def search(v):
        m = _edges.axis_model(axis, v)
        db.search_pssm(rows(q, m), None, m["open"], m["ext"], mode, algo)
        return word(capi) == ONE_STRIP
    try:
        v = _edges.last_admitted(search, *_edges.AXES[axis][1:])
    finally:
        db.close()
    print(f"EDGE one-strip pssm Q={Q} axis={axis} algo={algo} mode={mode} last_admitted={v}")
    for form in _edges.QUERY_FORMS:
        q, res, off = edge_db(form, Q)
        db = capi.DeviceDatabase(res, off, A)
        try:
            for x, admitted in ((v, True), (v + 1, False), (v - 1, True)):
                m = _edges.axis_model(axis, x)
                got = db.search_pssm(rows(q, m), None, m["open"], m["ext"], mode, algo)
                assert (word(capi) == ONE_STRIP) == admitted, (form, m, capi.DeviceDatabase.last_routing())
                exact(got, checker(q, res, off, _edges.model_matrix(m), m["open"], m["ext"], mode, algo), mode, f"pssm {form} {m}")
        finally:
            db.close()


@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ALGOS)
def test_one_strip_threshold_through_a_batch(capi, algo, mode):
    # three queries of the row class of 60 rows; the batch rule reads the class and the padding rows' floor
    axis = "match"
    queries = [_edges.edge_query(form, Q) for form, Q in zip(_edges.QUERY_FORMS, (57, 59, 60))]
    db = capi.DeviceDatabase(*_oracle.flatten([queries[2], _edges.pc(5)]), A)

    def search(v):
        m = _edges.axis_model(axis, v)
        db.search_batch(queries, _edges.model_matrix(m), m["open"], m["ext"], mode, algo)
        routing = db.last_batch_routing()
        return routing[0] > 0 and routing[2] == 0
    try:
        v = _edges.last_admitted(search, *_edges.AXES[axis][1:])
    finally:
        db.close()
    print(f"EDGE one-strip batch rows=60 axis={axis} algo={algo} mode={mode} last_admitted={v}")
    _, res, off = edge_db("random", 60)
    db = capi.DeviceDatabase(res, off, A)
    try:
        for x, admitted in ((v, True), (v + 1, False), (v - 1, True)):
            m = _edges.axis_model(axis, x)
            matrix = _edges.model_matrix(m)
            got = db.search_batch(queries, matrix, m["open"], m["ext"], mode, algo)
            routing = db.last_batch_routing()
            assert (routing[0] > 0 and routing[2] == 0) == admitted and (admitted or routing[2] == 3), (m, routing)
            for i, q in enumerate(queries):
                want = checker(q, res, off, matrix, m["open"], m["ext"], mode, algo)
                exact({k: a[i] for k, a in got.items()}, want, mode, f"batch query {i} {m}")
    finally:
        db.close()
