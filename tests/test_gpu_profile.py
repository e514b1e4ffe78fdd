"""Profile columns from hits (miopalProfileColumns / miopalProfileColumnsPssm, DeviceDatabase.profile_columns /
profile_columns_pssm, Aligner.profile_columns / iterated_search) against the CPU checker: the alignments of
tests/_oracle.search(mode="full"), target by target, projected and counted by the integer reference of
tests/_profile.py. The multiple alignment, the counts, the weighted counts and the member weights are equal bit for bit,
and the rows are also the projection of what align_pairs returns for the same pairs."""
import numpy as np
import pytest

import _data
import _oracle
import _profile
import _pssm
import pyopal_amd

pytestmark = pytest.mark.gpu

A = 32
QUERY_LENGTHS = [1, 63, 64, 65, 130]
LIST_LENGTHS = [1, 64, 65, 700]
ALGOS = ["sw", "nw", "hw", "ov"]


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def target_list(rng, n, count, always=()):
    """n target indices in random order, a quarter of them repeats of another quarter, `always` among them"""
    t = rng.integers(0, count, size=n)
    q = n // 4
    t[:q] = t[q:2 * q]
    if n >= len(always):
        t[:len(always)] = always
    return rng.permutation(t).astype(np.int64)


class World:
    """a database over 32 letters, queries as (classes, matrix, rows) of tests/_pssm.py - an ordinary query over its own
    32 x 32 matrix and the same search as a PSSM - and the checker's rows of every target, computed once per case"""

    def __init__(self, capi, rng, lengths):
        self.res, self.off = _pssm.random_db(rng, lengths, A)
        self.db = capi.DeviceDatabase(self.res, self.off, A)
        self.count = len(lengths)
        self.queries = {}
        self._rows = {}
        self.rng = rng

    def query(self, L):
        if L not in self.queries:
            # (scores of mean -1: local alignments stay local, global ones need their gaps)
            self.queries[L] = _pssm.class_pssm(self.rng, L, A, low=-9, high=7)
        return self.queries[L]

    def target(self, t):
        return self.res[self.off[t]:self.off[t + 1]]

    def rows(self, L, algo, go=3, ge=1):
        """uint8[targets][L]: the projection of the checker's alignment of every target of the database"""
        key = (L, algo, go, ge)
        if key not in self._rows:
            classes, matrix, _ = self.query(L)
            res = self.res if len(self.res) else np.zeros(1, np.uint8)
            want = _oracle.search(classes, res, self.off, matrix, go, ge, "full", algo)
            self._rows[key] = np.stack([
                _profile.project(want["aln"][t], want["start_q"][t], want["start_t"][t], self.target(t), L, A)
                for t in range(self.count)])
            self._rows[key].setflags(write=False)
        return self._rows[key]

    def close(self):
        self.db.close()


@pytest.fixture(scope="module")
def world(capi):
    rng = np.random.default_rng(31)
    w = World(capi, rng, _pssm.db_lengths(rng))
    w.lists = {n: target_list(rng, n, w.count, always=(3, 77, w.count - 1, 11)) for n in LIST_LENGTHS}
    yield w
    w.close()


def same(got, first, rows, targets, tag, msa=True):
    """got (a profile_columns dict) against the reference of the rows: `first` for the query, rows[targets]"""
    want = np.vstack([first[None, :], rows[targets]])
    if msa:
        np.testing.assert_array_equal(got["msa"], want, err_msg=f"msa {tag}")
    else:
        assert got["msa"] is None
    counts, k, terms, weights, weighted = _profile.columns(want, A)
    np.testing.assert_array_equal(got["counts"], counts, err_msg=f"counts {tag}")
    np.testing.assert_array_equal(got["member_weights"], weights, err_msg=f"member weights {tag}")
    np.testing.assert_array_equal(got["weighted"], weighted, err_msg=f"weighted {tag}")


def rows_of_pairs(world, pairs, targets, L):
    """the projection of an align_pairs(mode="full") dict"""
    return np.stack([_profile.project(pairs["aln"][p], pairs["start_q"][p], pairs["start_t"][p], world.target(t), L, A)
                     for p, t in enumerate(np.asarray(targets).tolist())])


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("L", QUERY_LENGTHS)
def test_against_the_checker(world, L, algo):
    classes, matrix, _ = world.query(L)
    rows = world.rows(L, algo)
    for n, targets in world.lists.items():
        got = world.db.profile_columns(classes, matrix, targets, 3, 1, algo, return_msa=True)
        routing = world.db.last_pair_routing()
        assert routing[0] + routing[1] + routing[2] == n, routing   # (reported like a plain pair list)
        same(got, classes, rows, targets, (L, algo, n))
        pairs = world.db.align_pairs([classes], np.zeros(n, dtype=np.int32), targets, matrix, 3, 1, "full", algo)
        np.testing.assert_array_equal(got["msa"][1:], rows_of_pairs(world, pairs, targets, L), err_msg=f"pairs {(L, algo, n)}")
    # the multiple alignment stays on the device: the same tables
    quiet = world.db.profile_columns(classes, matrix, world.lists[65], 3, 1, algo)
    same(quiet, classes, rows, world.lists[65], (L, algo, "no msa"), msa=False)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("switch,kind", [("MIOPAL_FORCE_LANE_PER_PAIR", "lanes"), ("MIOPAL_NO_PERPAIR", "waves")])
def test_both_kinds_of_kernel(world, tuning, switch, kind, algo):
    """one lane per pair and one wavefront per pair leave their operations in differently addressed slots"""
    tuning.setenv(switch, "1")
    for L in (64, 130):
        classes, matrix, _ = world.query(L)
        targets = world.lists[700]
        got = world.db.profile_columns(classes, matrix, targets, 3, 1, algo, return_msa=True)
        routing = world.db.last_pair_routing()
        assert routing[0] + routing[1] + routing[2] == len(targets), routing
        assert (routing[0] > 0) if kind == "lanes" else (routing[0] == 0 and routing[1] > 0), routing
        same(got, classes, world.rows(L, algo), targets, (L, algo, kind))


@pytest.mark.parametrize("algo", ALGOS)
def test_cheap_gaps(world, algo):
    """gap_open = gap_extend = 1: deletions and insertions in most alignments"""
    classes, matrix, _ = world.query(65)
    rows = world.rows(65, algo, 1, 1)
    targets = world.lists[700]
    assert np.count_nonzero(rows[targets] == A) > len(targets)   # (the gap letter is frequent)
    got = world.db.profile_columns(classes, matrix, targets, 1, 1, algo, return_msa=True)
    same(got, classes, rows, targets, (algo, "gaps"))


@pytest.mark.parametrize("algo", ["sw", "hw"])
def test_long_target_among_short_ones(capi, algo):
    """a 5000-residue target among short ones, in a list longer than a chunk sized for it holds: the pairs are taken
    largest first, in chunks, and a member's row is the caller's position, not the processing order"""
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 150, size=300)
    lengths[123] = 5000
    w = World(capi, rng, lengths)
    try:
        classes, matrix, _ = w.query(130)
        targets = target_list(rng, 4600, w.count, always=(123, 0, 123))
        got = w.db.profile_columns(classes, matrix, targets, 3, 1, algo, return_msa=True)
        routing = w.db.last_pair_routing()
        assert routing[3] > 1 and routing[0] + routing[1] + routing[2] == len(targets), routing
        same(got, classes, w.rows(130, algo), targets, (algo, "long target"))
    finally:
        w.close()


@pytest.mark.parametrize("algo", ["sw", "nw"])
def test_tall_query_on_the_wavefront_kernels(capi, algo):
    """a query of 4100 rows: taller than the lane-per-pair kernels take, sorted and chunked on its own path"""
    rng = np.random.default_rng(43)
    w = World(capi, rng, np.array([90, 20, 0, 150, 64, 33, 120, 75]))
    try:
        classes, matrix, _ = w.query(4100)
        targets = np.array([5, 0, 2, 7, 3, 3, 1, 6, 4], dtype=np.int64)
        got = w.db.profile_columns(classes, matrix, targets, 3, 1, algo, return_msa=True)
        routing = w.db.last_pair_routing()
        assert routing[0] == 0 and routing[1] == 8 and routing[2] == 1, routing
        same(got, classes, w.rows(4100, algo), targets, (algo, "tall"))
    finally:
        w.close()


def test_empty_alignments_and_empty_targets_only(world):
    """targets that are all empty: no pair has a DP, nothing is launched, the rows stay uncovered"""
    classes, matrix, _ = world.query(64)
    targets = np.array([3, 77, 3, world.count - 1], dtype=np.int64)
    got = world.db.profile_columns(classes, matrix, targets, 3, 1, "sw", return_msa=True)
    assert world.db.last_pair_routing()[2] == 4
    same(got, classes, world.rows(64, "sw"), targets, "empty targets")
    assert np.all(got["msa"][1:] == 255) and got["member_weights"].tolist() == [64 * 2 ** 32, 0, 0, 0, 0]
    # no target at all, and no query
    got = world.db.profile_columns(classes, matrix, [], 3, 1, "sw", return_msa=True)
    same(got, classes, world.rows(64, "sw"), np.zeros(0, dtype=np.int64), "no targets")
    got = world.db.profile_columns(np.zeros(0, np.uint8), matrix, [5, 6], 3, 1, "nw", return_msa=True)
    assert got["counts"].shape == (0, A + 1) and got["msa"].shape == (3, 0) and got["member_weights"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("L", [65, 130])
def test_pssm_form(world, L, algo):
    """the class identity of tests/_pssm.py: the rows of the PSSM are the matrix rows of its classes, so the checker on
    (classes, matrix) says what the alignments are. Positions without a consensus residue (255) are never a match -
    which the projection does not see - and do not count for the query's own row."""
    classes, matrix, pssm_rows = world.query(L)
    rows = world.rows(L, algo)
    targets = world.lists[700]
    plain = world.db.profile_columns(classes, matrix, targets, 3, 1, algo, return_msa=True)
    got = world.db.profile_columns_pssm(pssm_rows, classes, targets, 3, 1, algo, return_msa=True)
    for key in plain:
        np.testing.assert_array_equal(got[key], plain[key], err_msg=f"{key} {(L, algo)}")
    consensus = classes.copy()
    consensus[::7] = 255
    got = world.db.profile_columns_pssm(pssm_rows, consensus, targets, 3, 1, algo, return_msa=True)
    same(got, consensus, rows, targets, (L, algo, "no residue"))
    assert np.all(got["msa"][0, ::7] == 255) and got["member_weights"][0] < plain["member_weights"][0]
    pairs = world.db.align_pairs_pssm([pssm_rows], [consensus], np.zeros(len(targets), dtype=np.int32), targets, 3, 1,
                                      "full", algo)
    np.testing.assert_array_equal(got["msa"][1:], rows_of_pairs(world, pairs, targets, L))
    quiet = world.db.profile_columns_pssm(pssm_rows, consensus, world.lists[64], 3, 1, algo)
    same(quiet, consensus, rows, world.lists[64], (L, algo, "no msa"), msa=False)


def test_errors_leave_the_outputs_alone(world, capi):
    """a bad target index, a null output and a database of another alphabet: reported with the handle in place, before
    any device call, the message naming the target"""
    lib = capi.lib()
    classes, matrix, _ = world.query(64)
    q = np.ascontiguousarray(classes)
    s = np.ascontiguousarray(matrix, dtype=np.int32)
    outs = [np.full(64 * (A + 1), 77, dtype=np.int64), np.full(64 * (A + 1), 77, dtype=np.int64),
            np.full(4, 77, dtype=np.int64)]

    def call(targets, missing=(), alphabet=A):
        t = np.asarray(targets, dtype=np.int64)
        ptrs = [None if i in missing else o.ctypes.data for i, o in enumerate(outs)]
        return lib.miopalProfileColumns(world.db.handle, q.ctypes.data, 64, 3, 1, s.ctypes.data, alphabet, 3,
                                        t.ctypes.data, len(t), *ptrs, None)

    assert call([5, world.count, 6]) == 101 and f"target 1: target index {world.count} outside" in capi.last_error()
    assert call([5, -1, 6]) == 101 and "target 1: target index -1" in capi.last_error()
    for k in (0, 1, 2):
        assert call([5, 6, 7], missing=(k,)) == 101 and "null counts / weighted / member weight" in capi.last_error()
    assert call([5, 6, 7], alphabet=24) == 101   # (residues of the 32-letter query beyond 24, or the handle's alphabet)
    assert all(np.all(o == 77) for o in outs)
    assert call([5, 6, 7]) == 0 and not any(np.any(o == 77) for o in outs[:2])


def letters(codes):
    return "".join(_data.NCBI[c] for c in codes)


def test_iterated_search_is_the_composition_of_its_steps():
    """Aligner.iterated_search on a small planted family - 300 random targets and 12 mutated copies of the query: the
    returned hits, PSSM and per-round index lists are those of significant_hits, profile_columns, Pssm.from_columns and
    significant_hits_pssm composed by hand, and the loop ends by repetition or at `rounds`. No statistical claim."""
    rng = np.random.default_rng(53)
    query = _data.random_protein(rng, 120)
    seqs = [_data.random_protein(rng, int(n)) for n in rng.integers(60, 400, size=312)]
    where = np.sort(rng.choice(312, size=12, replace=False))
    for k in where:
        seqs[k] = np.concatenate([_data.random_protein(rng, int(rng.integers(0, 60))), _data.mutate(rng, query, rate=0.3),
                                  _data.random_protein(rng, int(rng.integers(0, 60)))]).astype(np.uint8)
    database = pyopal_amd.Database([letters(s) for s in seqs])
    aligner = pyopal_amd.Aligner("BLOSUM62", gap_open=11, gap_extend=1)
    q = letters(query)
    cut, rounds = 1.0, 4

    indices = lambda hits: np.array(sorted(r.target_index for r in hits.results), dtype=np.int64)   # noqa: E731
    background = np.bincount(np.concatenate(seqs), minlength=24).astype(np.float64)
    background /= background.sum()
    lam = pyopal_amd.matrix_lambda(aligner.scoring_matrix, background)
    hits = aligner.significant_hits(q, database, cut)
    found, pssm = [indices(hits)], None
    current, prior = q, pyopal_amd.Pssm.from_sequence(q, "BLOSUM62")
    while len(found) < rounds:
        columns = aligner.profile_columns(current, database, found[-1])
        assert columns.counts.shape == (120, 25) and len(columns.member_weights) == len(found[-1]) + 1
        pssm = pyopal_amd.Pssm.from_columns(columns, prior, background, lam, pseudocount=10.0)
        hits = aligner.significant_hits_pssm(pssm, database, cut)
        found.append(indices(hits))
        if any(np.array_equal(found[-1], f) for f in found[:-1]):
            break
        current = prior = pssm

    got_hits, got_pssm, got_found = aligner.iterated_search(q, database, cut, rounds=rounds)
    assert len(got_found) == len(found) <= rounds
    for a, b in zip(got_found, found):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    assert len(found) == rounds or any(np.array_equal(found[-1], f) for f in found[:-1])
    assert got_pssm == pssm and pssm is not None
    assert [(r.target_index, r.score) for r in got_hits.results] == [(r.target_index, r.score) for r in hits.results]
    assert np.array_equal(got_hits.evalues, hits.evalues)
    assert len(found[0]) > 0   # (round 2 had members to build on)
    # one round: the plain search, no PSSM
    one_hits, one_pssm, one_found = aligner.iterated_search(q, database, cut, rounds=1)
    assert one_pssm is None and len(one_found) == 1 and np.array_equal(one_found[0], found[0])
    # a given background in the place of the database's composition
    flat = aligner.iterated_search(q, database, cut, rounds=2, background=np.bincount(np.concatenate(seqs), minlength=24))
    again = aligner.iterated_search(q, database, cut, rounds=2)
    assert flat[1] == again[1] and np.array_equal(flat[2][-1], again[2][-1])
