"""Search with a position-specific scoring matrix (miopalSearchPssm, DeviceDatabase.search_pssm, Aligner.align_pssm).

Two yardsticks, both exact. A PSSM derived from a sequence and a matrix must give what the plain search gives, array
for array, on the same kernels (the routing counters agree). A true PSSM is checked against the CPU checker through
the class identity of tests/_pssm.py: rows drawn from 32 row vectors are an ordinary search over 32 letters, which the
checker can run; the library gets the Q x 32 rows. A numpy DP in tests/_pssm.py is the second witness for rows that
are all distinct. Databases: ~700 targets of 0-180 residues (zero-length ones and a repeated one among them), which
tests/conftest.py keeps on the lane-per-target kernels."""
import threading

import numpy as np
import pytest

import _data
import _oracle
import _pssm
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
ALGORITHMS = ("nw", "hw", "ov", "sw")
MODES = ("score", "end", "full")
KEYS = {"score": ("score",), "end": ("score", "end_q", "end_t"),
        "full": ("score", "end_q", "end_t", "start_q", "start_t", "aln_off", "aln_flat")}


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def protein_db(capi):
    """24 letters, for the PSSMs derived from a sequence"""
    rng = np.random.default_rng(101)
    residues, offsets = _pssm.with_repeat(*_data.random_db(rng, _pssm.db_lengths(rng)))
    db = capi.DeviceDatabase(residues, offsets, 24)
    yield db
    db.close()


@pytest.fixture(scope="module")
def class_db(capi):
    """32 letters, for the class identity: (handle, residues, offsets)"""
    rng = np.random.default_rng(202)
    residues, offsets = _pssm.with_repeat(*_pssm.random_db(rng, _pssm.db_lengths(rng)))
    db = capi.DeviceDatabase(residues, offsets, 32)
    yield db, residues, offsets
    db.close()


_WANT = {}


def checker(key, classes, residues, offsets, matrix, gaps, mode, algorithm):
    """the CPU checker's answer for a class query, computed once per case of the module"""
    key = (key, gaps, mode, algorithm)
    if key not in _WANT:
        _WANT[key] = _oracle.search(classes, residues, offsets, matrix, gaps[0], gaps[1], mode, algorithm)
    return _WANT[key]


# ---- 1. derived == plain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 53, 64, 65, 130, 300])
def test_derived_pssm_equals_the_plain_search(protein_db, tuning, length):
    """rows = matrix[query], consensus = query: every output of every mode and search type equals DeviceDatabase.search,
    and the search takes the same kernels - it is not parked on a slow one. `full` twice: as routed (few pairs: a
    wavefront per pair) and with the lane-per-pair passes a large database takes."""
    rng = np.random.default_rng(length)
    query = _data.random_protein(rng, length)
    rows = B62.reshape(24, 24)[query]
    for gaps in ((3, 1), (11, 1)):
        for algorithm in ALGORITHMS:
            for mode, lanes in (("score", False), ("end", False), ("full", False), ("full", True)):
                if lanes:
                    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")
                else:
                    tuning.delenv("MIOPAL_FORCE_LANE_PER_PAIR", raising=False)
                plain = protein_db.search(query, B62, gaps[0], gaps[1], mode, algorithm)
                plain_routing = (protein_db.last_routing(), protein_db.last_full_routing() if mode == "full" else 0)
                got = protein_db.search_pssm(rows, query, gaps[0], gaps[1], mode, algorithm)
                routing = (protein_db.last_routing(), protein_db.last_full_routing() if mode == "full" else 0)
                for key in KEYS[mode]:
                    assert np.array_equal(got[key], plain[key]), (gaps, algorithm, mode, lanes, key)
                assert routing == plain_routing, (gaps, algorithm, mode, lanes)
                assert not lanes or routing[1] & 4, routing
                if mode != "full":
                    # (score and end searches never read the consensus)
                    bare = protein_db.search_pssm(rows, None, gaps[0], gaps[1], mode, algorithm)
                    assert all(np.array_equal(bare[key], plain[key]) for key in KEYS[mode]), (gaps, algorithm, mode)
    assert plain_routing[0][2] > 0   # the lane-per-target kernels


def test_derived_pssm_at_the_edges(protein_db):
    """no rows at all, a slice, an empty slice: as miopalSearchFlat answers them"""
    empty = np.zeros((0, 24), dtype=np.int32)
    for algorithm in ALGORITHMS:
        for mode in MODES:
            plain = protein_db.search(np.zeros(0, dtype=np.uint8), B62, 3, 1, mode, algorithm)
            got = protein_db.search_pssm(empty, None, 3, 1, mode, algorithm)
            for key in KEYS[mode]:
                assert np.array_equal(got[key], plain[key]), (algorithm, mode, key)
    query = _data.random_protein(np.random.default_rng(3), 40)
    rows = B62.reshape(24, 24)[query]
    plain = protein_db.search(query, B62, 3, 1, "full", "sw", 100, 230)
    got = protein_db.search_pssm(rows, query, 3, 1, "full", "sw", 100, 230)
    for key in KEYS["full"]:
        assert np.array_equal(got[key], plain[key]), key
    nothing = protein_db.search_pssm(rows, query, 3, 1, "full", "sw", 50, 50)
    assert len(nothing["score"]) == 0 and nothing["aln_off"].tolist() == [0] and len(nothing["aln_flat"]) == 0


def test_handle_checks_come_before_any_launch(capi, class_db):
    """the checks that need the handle: its alphabet, the slice, and miopalSearch's 32-bit range check with the rows'
    extreme entries where the matrix's stand"""
    db = class_db[0]
    rows = np.ones((5, 32), dtype=np.int32)
    with pytest.raises(ValueError):
        db.search_pssm(np.ones((5, 24), dtype=np.int32))
    lib = capi.lib()
    score = np.full(4, 77, dtype=np.int32)

    def call(r, alphabet=32, start=0, end=4):
        return lib.miopalSearchPssm(db.handle, r.ctypes.data, None, len(r), 3, 1, alphabet, 0, 3, start, end,
                                    score.ctypes.data, None, None, None, None, None, None)

    assert call(np.ones((5, 24), dtype=np.int32), alphabet=24) == 101 and "differs from the database's" in capi.last_error()
    assert call(rows, start=3, end=2) == 101 and "bad slice" in capi.last_error()
    assert call(rows, end=db.count + 1) == 101 and "bad slice" in capi.last_error()
    huge = rows.copy()
    huge[2, 7] = 2 ** 30
    assert call(huge) == capi.OPAL_ERR_OVERFLOW and "32-bit range" in capi.last_error()
    huge[2, 7] = -(2 ** 30)
    assert call(huge) == capi.OPAL_ERR_OVERFLOW
    assert np.all(score == 77)
    assert call(rows, start=2, end=2) == 0 and np.all(score == 77)     # an empty slice: nothing launched, nothing written
    assert call(rows) == 0 and not np.any(score == 77)


# ---- 2. true PSSMs against the checker --------------------------------------------------------------------------
@pytest.mark.parametrize("length,values", [(31, None), (64, None), (65, None), (200, None),
                                           (64, (-1, 0, 0, 1, 1, 2)), (65, (-1, 0, 0, 1, 1, 2))])
def test_true_pssm_against_the_checker(class_db, tuning, length, values):
    """entries in [-8, 12], and once rows rich in ties (many equal entries: the tie-breaks of end cells and traceback);
    `full` as routed and with the lane-per-pair passes"""
    db, residues, offsets = class_db
    rng = np.random.default_rng(1000 + length + (7 if values else 0))
    classes, matrix, rows = _pssm.class_pssm(rng, length, values=values)
    for algorithm in ALGORITHMS:
        for mode, lanes in (("score", False), ("end", False), ("full", False), ("full", True)):
            if lanes:
                tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")
            else:
                tuning.delenv("MIOPAL_FORCE_LANE_PER_PAIR", raising=False)
            want = checker(("true", length, values), classes, residues, offsets, matrix, (3, 1), mode, algorithm)
            got = db.search_pssm(rows, classes, 3, 1, mode, algorithm)
            _pssm.assert_same(got, want, (length, values, algorithm, mode, lanes))
            if mode == "score":
                assert db.last_routing()[2] > 0
    k = len(offsets) - 2   # the repeated target: the same answer at both indices
    assert got["score"][20] == got["score"][k] and got["aln"][20].tolist() == got["aln"][k].tolist()


# ---- 3. the int32 rung ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [100, 170])
def test_large_entries_leave_the_16_bit_lanes(class_db, length):
    """Entries of +300 .. +400: against the longer targets a query of 100 rows scores beyond 32767, so their lanes
    leave every 16-bit rung (Smith-Waterman) or are kept out of them by their length (NW / HW / OV), and the int32
    kernels' row-indexed forms redo them - two and three strips of rows. (No one-strip query reaches a 16-bit limit
    with entries up to 400; the long target and the small searches below run the one-strip forms.)"""
    db, residues, offsets = class_db
    rng = np.random.default_rng(3000 + length)
    classes, matrix, rows = _pssm.class_pssm(rng, length, low=300, high=400)
    for algorithm in ALGORITHMS:
        for mode in ("score", "end"):
            want = checker(("large", length), classes, residues, offsets, matrix, (3, 1), mode, algorithm)
            got = db.search_pssm(rows, None, 3, 1, mode, algorithm)
            routing = db.last_routing()
            _pssm.assert_same(got, want, (length, algorithm, mode))
            assert routing[3] > 0 or routing[0] > 0, (length, algorithm, mode, routing)


LONG_TARGET_QUERIES = (40, 100, 170)


@pytest.fixture(scope="module")
def long_target_db(capi):
    """~700 short targets and one long enough that the PLAIN search hands it to the wavefront-per-pair kernel beside
    the packed launch: (handle, residues, offsets, index of the long target). The length is found, not assumed."""
    rng = np.random.default_rng(303)
    lengths = _pssm.db_lengths(rng)
    probes = [_pssm.class_pssm(rng, length) for length in LONG_TARGET_QUERIES]
    for longest in (3000, 6000, 12000, 24000, 48000):
        lengths[13] = longest
        residues, offsets = _pssm.random_db(rng, lengths)
        db = capi.DeviceDatabase(residues, offsets, 32)
        on_the_side = []
        for classes, matrix, _ in probes:   # (NW: a global alignment cannot be cut into windows)
            db.search(classes, matrix, 3, 1, "score", "nw")
            on_the_side.append(db.last_routing()[0] > 0 and db.last_routing()[2] > 0)
        if all(on_the_side):
            yield db, residues, offsets, 13
            db.close()
            return
        db.close()
    pytest.fail("no target length up to 48000 reached the wavefront-per-pair kernel in the plain search")


@pytest.mark.parametrize("length,one_by_one", [(40, False), (100, False), (100, True), (170, False)])
def test_long_target_beside_the_packed_launch(long_target_db, tuning, length, one_by_one):
    """the side kernel's row-indexed forms: a one-strip query (intraseq_wide_kernel), two and three strips as units of
    (pair, strip) (intraseq_strips_kernel), and two strips one after the other (intraseq_kernel)"""
    db, residues, offsets, at = long_target_db
    if one_by_one:
        tuning.setenv("MIOPAL_NO_PAIR_STRIP_UNITS", "1")
    rng = np.random.default_rng(3300 + length)
    classes, matrix, rows = _pssm.class_pssm(rng, length)
    assert length in LONG_TARGET_QUERIES
    for algorithm in ALGORITHMS:
        for mode in ("score", "end"):
            want = checker(("long", length), classes, residues, offsets, matrix, (3, 1), mode, algorithm)
            plain = db.search(classes, matrix, 3, 1, mode, algorithm)
            plain_routing = db.last_routing()
            got = db.search_pssm(rows, None, 3, 1, mode, algorithm)
            assert db.last_routing() == plain_routing, (length, algorithm, mode)
            _pssm.assert_same(got, want, (length, algorithm, mode))
            _pssm.assert_same(plain, want, (length, algorithm, mode, "plain"))
            # (Smith-Waterman and HW may cut the long target into windows instead; NW cannot)
            assert algorithm != "nw" or (plain_routing[0] > 0 and plain_routing[2] > 0), (length, mode, plain_routing)


# ---- 4. small searches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [40, 150])
def test_small_search_routing(capi, small_search_routing, length):
    """five targets under the production routing: every pass on the wavefront-per-pair kernels, traceback included"""
    rng = np.random.default_rng(4000 + length)
    residues, offsets = _pssm.random_db(rng, [90, 0, 181, 37, 64])
    classes, matrix, rows = _pssm.class_pssm(rng, length)
    db = capi.DeviceDatabase(residues, offsets, 32)
    try:
        for algorithm in ALGORITHMS:
            for mode in MODES:
                want = _oracle.search(classes, residues, offsets, matrix, 3, 1, mode, algorithm)
                got = db.search_pssm(rows, classes, 3, 1, mode, algorithm)
                assert db.last_routing()[0] == 5 and db.last_routing()[2] == 0
                _pssm.assert_same(got, want, (length, algorithm, mode))
    finally:
        db.close()


# ---- 5. `full`: the packed passes and what stands behind them -----------------------------------------------------
@pytest.mark.parametrize("length", [40, 65])
def test_full_packed_and_fallback(class_db, tuning, length):
    """One scheme the two-pairs-per-lane passes take (packedTraceFits holds), and two they do not: an opening cheaper
    than an extension, which the byte-profile kernels take, and entries too large for a byte profile, which
    perpair_kernel's row-indexed form takes. All against the checker."""
    db, residues, offsets = class_db
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")   # (the cost estimates prefer a wavefront per pair on few pairs)
    rng = np.random.default_rng(5000 + length)
    seen = {}
    for name, gaps, high in (("packed", (3, 1), 12), ("open < extend", (2, 5), 12), ("large", (5, 2), 150)):
        classes, matrix, rows = _pssm.class_pssm(rng, length, high=high)
        routes = []
        for algorithm in ALGORITHMS:
            want = checker(("full", name, length), classes, residues, offsets, matrix, gaps, "full", algorithm)
            got = db.search_pssm(rows, classes, gaps[0], gaps[1], "full", algorithm)
            routes.append(db.last_full_routing())
            _pssm.assert_same(got, want, (name, length, algorithm))
        seen[name] = routes
    assert all(r & 64 for r in seen["packed"]), seen                 # packed direction pass
    assert not any(r & 64 for r in seen["large"]), seen
    assert not any(r & 64 for r in seen["open < extend"]) and all(r & 8 for r in seen["open < extend"]), seen   # byte profile
    assert not any(r & 8 for r in seen["large"]) and all(r & 4 for r in seen["large"]), seen   # lane per pair, no profile
    assert seen["packed"] != seen["open < extend"] != seen["large"] != seen["packed"], seen


def test_full_with_more_rows_than_the_lane_kernel_stages(class_db, tuning):
    """Large entries (no byte profile) and more rows than perpair_kernel's row-indexed form holds in LDS - 493 at 32
    letters: the start-cell scan and the direction pass run one wavefront per pair (the documented difference to the
    plain search, which keeps its lanes), and the answers are the checker's. At 493 rows the lane kernel still runs."""
    db, residues, offsets = class_db
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")
    n = 120
    for length, lanes in ((493, True), (494, False)):
        rng = np.random.default_rng(5500 + length)
        classes, matrix, rows = _pssm.class_pssm(rng, length, high=150)
        for algorithm in ("sw", "ov"):
            want = _oracle.search(classes, residues[:offsets[n]], offsets[:n + 1], matrix, 5, 2, "full", algorithm)
            got = db.search_pssm(rows, classes, 5, 2, "full", algorithm, 0, n)
            routing = db.last_full_routing()
            _pssm.assert_same(got, want, (length, algorithm))
            assert bool(routing & 4) == lanes and bool(routing & 1) == lanes and not routing & (8 | 64), (length, routing)
            db.search(classes, matrix, 5, 2, "full", algorithm, 0, n)
            assert db.last_full_routing() & 5 == 5, length


# ---- 6. the consensus -------------------------------------------------------------------------------------------
def test_consensus_only_tells_match_from_mismatch(class_db):
    db, residues, offsets = class_db
    rng = np.random.default_rng(6)
    classes, matrix, rows = _pssm.class_pssm(rng, 80)
    best = rows.argmax(axis=1).astype(np.uint8)
    for algorithm in ALGORITHMS:
        base = db.search_pssm(rows, best, 3, 1, "full", algorithm)
        none = db.search_pssm(rows, np.full(80, 255, dtype=np.uint8), 3, 1, "full", algorithm)
        other = db.search_pssm(rows, classes, 3, 1, "full", algorithm)
        assert 0 in base["aln_flat"] and 3 in base["aln_flat"]
        assert 0 not in none["aln_flat"]              # "no residue" is never a match
        for alt in (none, other):
            for key in ("score", "end_q", "end_t", "start_q", "start_t", "aln_off"):
                assert np.array_equal(alt[key], base[key]), (algorithm, key)
            differs = alt["aln_flat"] != base["aln_flat"]
            assert np.all(np.isin(alt["aln_flat"][differs], (0, 3))) and np.all(np.isin(base["aln_flat"][differs], (0, 3)))
        assert np.any(other["aln_flat"] != base["aln_flat"])
        # match exactly where the target's residue is the consensus'
        k = int(np.argmax(np.diff(base["aln_off"])))
        i, j = int(base["start_q"][k]), int(base["start_t"][k])
        for op in base["aln"][k]:
            if op in (0, 3):
                assert (op == 0) == (best[i] == residues[offsets[k] + j]), (algorithm, k, i, j)
            i += op != 2
            j += op != 1


# ---- 7. Python --------------------------------------------------------------------------------------------------
def _fields(result, names):
    """the named properties of a result object; None where the object refuses (a location of an empty alignment)"""
    out = []
    for name in names:
        try:
            out.append(getattr(result, name))
        except AssertionError:
            out.append(None)
    return out


def test_align_pssm_equals_align():
    import pyopal_amd
    rng = np.random.default_rng(7)
    letters = np.array(list(_data.AA20))
    targets = ["".join(letters[rng.integers(0, 20, size=n)]) for n in _pssm.db_lengths(rng, 300, 120)]
    targets[9] = _data.README_QUERY[3:40]
    database = pyopal_amd.Database(targets)
    aligner = pyopal_amd.Aligner("BLOSUM62", 3, 1)
    pssm = pyopal_amd.Pssm.from_sequence(_data.README_QUERY)
    for algorithm in ("sw", "nw"):
        for mode in MODES:
            want = aligner.align(_data.README_QUERY, database, mode=mode, algorithm=algorithm)
            got = aligner.align_pssm(pssm, database, mode=mode, algorithm=algorithm)
            assert len(got) == len(want) == 300 and type(got[0]) is type(want[0])
            names = {"score": ("target_index", "score"), "end": ("target_index", "score", "query_end", "target_end"),
                     "full": ("target_index", "score", "query_end", "target_end", "query_start", "target_start",
                              "query_length", "target_length", "alignment")}[mode]
            for a, b in zip(got, want):
                assert _fields(a, names) == _fields(b, names), (algorithm, mode, b.target_index)
    # another aligner's matrix does not matter, its gap penalties do
    assert [r.score for r in pyopal_amd.Aligner("BLOSUM50", 3, 1).align_pssm(pssm, database)] == \
           [r.score for r in aligner.align(_data.README_QUERY, database)]
    assert [r.score for r in pyopal_amd.Aligner("BLOSUM62", 11, 1).align_pssm(pssm, database)] == \
           [r.score for r in pyopal_amd.Aligner("BLOSUM62", 11, 1).align(_data.README_QUERY, database)]
    sliced = aligner.align_pssm(pssm, database, mode="end", start=5, end=40)
    assert [r.target_index for r in sliced] == list(range(5, 40))
    assert [r.score for r in sliced] == [r.score for r in aligner.align(_data.README_QUERY, database, start=5, end=40)]


def test_align_pssm_arrays_against_the_checker():
    """a true PSSM through the Python layer: 24 row classes over the default alphabet"""
    import pyopal_amd
    rng = np.random.default_rng(77)
    residues, offsets = _data.random_db(rng, _pssm.db_lengths(rng, 300, 150))
    targets = [bytes(np.frombuffer(_data.NCBI.encode(), dtype=np.uint8)[residues[offsets[k]:offsets[k + 1]]]).decode()
               for k in range(300)]
    database = pyopal_amd.Database(targets)
    classes, matrix, rows = _pssm.class_pssm(rng, 90, alphabet=24)
    pssm = pyopal_amd.Pssm(rows, consensus=classes)
    for algorithm in ("sw", "hw"):
        want = _oracle.search(classes, residues, offsets, matrix, 4, 2, "full", algorithm)
        arrays = pyopal_amd.Aligner(gap_open=4, gap_extend=2).align_pssm_arrays(pssm, database, mode="full", algorithm=algorithm)
        assert arrays.query_length == 90 and len(arrays) == 300
        for name, key in (("score", "score"), ("query_end", "end_q"), ("target_end", "end_t"),
                          ("query_start", "start_q"), ("target_start", "start_t")):
            assert np.array_equal(getattr(arrays, name), want[key]), (algorithm, name)
        for k in range(300):
            assert arrays.operations[arrays.operation_offsets[k]:arrays.operation_offsets[k + 1]].tolist() == want["aln"][k].tolist()
        assert arrays[9].query_length == 90 and arrays[9].score == want["score"][9]


def test_two_threads_search_one_database(class_db):
    db, residues, offsets = class_db
    rng = np.random.default_rng(8)
    cases = [_pssm.class_pssm(rng, 70), _pssm.class_pssm(rng, 150)]
    wants = [checker(("threads", k), c[0], residues, offsets, c[1], (3, 1), "full", "sw") for k, c in enumerate(cases)]
    errors = []
    barrier = threading.Barrier(2)

    def work(k):
        try:
            barrier.wait(timeout=30)
            for _ in range(4):
                got = db.search_pssm(cases[k][2], cases[k][0], 3, 1, "full", "sw")
                _pssm.assert_same(got, wants[k], ("thread", k))
        except BaseException as e:   # noqa: BLE001 (reported on the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---- 8. the second witness --------------------------------------------------------------------------------------
def test_distinct_rows_against_the_numpy_dp(capi):
    """100 rows, all different (no class identity to lean on), 50 targets: scores against tests/_pssm.dp_scores,
    which tests/test_pssm_cpu.py pins against the checker"""
    rng = np.random.default_rng(88)
    rows = rng.integers(-9, 13, size=(100, 32)).astype(np.int32)
    assert len({r.tobytes() for r in rows}) == 100
    lengths = rng.integers(1, 181, size=50)
    lengths[[4, 30]] = 0
    residues, offsets = _pssm.random_db(rng, lengths)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(50)]
    db = capi.DeviceDatabase(residues, offsets, 32)
    try:
        for algorithm in ("sw", "nw"):
            for gaps in ((3, 1), (7, 2)):
                got = db.search_pssm(rows, None, gaps[0], gaps[1], "score", algorithm)["score"]
                assert np.array_equal(got, _pssm.dp_scores(rows, targets, gaps[0], gaps[1], algorithm)), (algorithm, gaps)
    finally:
        db.close()
