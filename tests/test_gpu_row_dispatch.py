"""Every row count of the pair-table kernels reaches its own instantiation (launch_layer.h, dispatchRows; the unit of
a row count: interseq.hip). A count that the launch layer sends to a translation unit that does not hold it comes
back as hipErrorInvalidValue: the search fails, or the host falls back to another kernel and the routing word says
so. Small databases, every result bit for bit against the CPU checker, BLOSUM62 with gaps 3 / 1.

  * one strip, SW and NW / HW / OV: every query length from 1 to 64, scores and end locations;
  * the column split of the one-strip SW kernel: every query length from 1 to 64;
  * several strips, SW and NW: every strip height the host can choose (host_search.inc), SW end locations from row
    keys and from the second sweep that looks for the known optimum.

The pair table of 61 .. 64 rows holds 21 symbols, not the 25 of the 24-letter alphabet (interseqPairFits): those four
lengths run on the 20 amino acids the data is made of, as in test_gpu_column_split.py.
The batch kernels' row classes (8, 16, ..., 56, 60, 64; SW, SW with end locations, NW / HW / OV) are all visited by
test_gpu_batch_edges.py (LONG_QUERY_LENGTHS: every class that holds 25 symbols; the flag thresholds and the other
alphabets: class 64): nothing to add here."""
import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
B62_20 = np.ascontiguousarray(B62.reshape(24, 24)[:20, :20]).ravel()
PAIR_BIASED = 2 + 2     # miopalLastRouting counts[1]: 2 + kPairSwBiased
PAIR_GLOBAL = 2 + 3     # ... kPairGlobalBiased
PAIR_STRIPS = 2 + 4     # ... kPairSwStrips
GLOBAL_STRIPS = 2 + 5   # ... kPairGlobalStrips
SPLIT = 64              # ... + 64: the column split
ROWS = range(1, 65)


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def routed(capi):
    return capi.DeviceDatabase.last_routing()[1]


def related_query(rng, res, off, qlen):
    """A noisy copy of the first residues of the database: some targets score high, wherever they are."""
    query = _data.mutate(rng, res[:qlen + 24], 0.1)[:qlen].copy() if qlen >= 8 else _data.random_protein(rng, qlen)
    assert len(query) == qlen
    return query


def assert_same(got, want, tag):
    for key in ("score", "end_t", "end_q"):
        if key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"{tag} {key}")


# ---- one strip ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_strip(capi):
    # three groups of 128 lanes, the last one ragged: 256 + 77 targets of 24 residues (with MIOPAL_NO_SMALL_SEARCH,
    # which tests/conftest.py sets, the host sends a database of any size to the lane-per-target kernels)
    rng = np.random.default_rng(64)
    res, off = _data.random_db(rng, np.full(256 + 77, 24))
    dbs = {24: capi.DeviceDatabase(res, off, 24), 20: capi.DeviceDatabase(res, off, 20)}
    yield dbs, res, off
    for db in dbs.values():
        db.close()


@pytest.mark.parametrize("qlen", ROWS)
@pytest.mark.parametrize("algo,kernel", [("sw", PAIR_BIASED), ("nw", PAIR_GLOBAL), ("hw", PAIR_GLOBAL), ("ov", PAIR_GLOBAL)])
def test_one_strip_every_row_count(capi, one_strip, algo, kernel, qlen):
    dbs, res, off = one_strip
    alphabet, matrix = (24, B62) if qlen <= 60 else (20, B62_20)
    query = related_query(np.random.default_rng(100 + qlen), res, off, qlen)
    for mode in ("score", "end"):
        got = dbs[alphabet].search(query, matrix, 3, 1, mode, algo)
        assert routed(capi) & 31 == kernel, f"{algo} {mode} Q={qlen}: {capi.DeviceDatabase.last_routing()}"
        assert_same(got, _oracle.search(query, res, off, matrix, 3, 1, mode, algo), f"{algo} {mode} Q={qlen}")


# ---- the column split -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split_set(capi):
    # the smallest shape of test_gpu_column_split.py: 40 groups of 75 chunks
    rng = np.random.default_rng(65)
    res, off = _data.random_db(rng, np.full(5120, 300))
    dbs = {24: capi.DeviceDatabase(res, off, 24), 20: capi.DeviceDatabase(res, off, 20)}
    yield dbs, res, off
    for db in dbs.values():
        db.close()


@pytest.mark.parametrize("qlen", ROWS)
def test_column_split_every_row_count(capi, split_set, qlen):
    dbs, res, off = split_set
    alphabet, matrix = (24, B62) if qlen <= 60 else (20, B62_20)
    query = related_query(np.random.default_rng(200 + qlen), res, off, qlen)
    with capi.tuning(COLUMN_SPLIT="2"):
        got = dbs[alphabet].search(query, matrix, 3, 1, "score", "sw")
        assert routed(capi) == PAIR_BIASED + SPLIT, f"Q={qlen}: {capi.DeviceDatabase.last_routing()}"
    assert_same(got, _oracle.search_parallel(query, res, off, matrix, 3, 1, "score", "sw", chunk=640), f"split Q={qlen}")


# ---- several strips -------------------------------------------------------------------------------------------------
# The host's strip height for a query of Q rows (host_search.inc), h_max = 52 for scores, 48 with end locations, 40 for
# the two sweeps of an `end` search that looks for the known optimum:
#   SW:            ns = max(2, ceil(Q / h_max)) strips of the even height >= Q / ns
#   NW / HW / OV:  the even height in 32 .. h_max of least ns * (height + 4) (+ height / 8 when more than one row is padded)
# Both give two strips of Q / 2 rows for Q = 64, 68, ..., 2 h_max:
#   Q       64  68  72  76  80  84  88  92  96  100  104
#   height  32  34  36  38  40  42  44  46  48   50   52
# (64 rows are one strip for at most 21 symbols: with 25 they are two strips of 32.)
def strip_lengths(h_max):
    return range(64, 2 * h_max + 1, 4)


@pytest.fixture(scope="module")
def strips_set(capi):
    # the small database of test_gpu_global_strips.py (the strips kernels are forced: MIOPAL_PAIR_STRIPS): mixed lengths,
    # relatives of the longest query - its prefixes are the other queries - halves of it, an empty and a one-residue target
    rng = np.random.default_rng(66)
    base = _data.random_protein(rng, 104)
    seqs = [_data.random_protein(rng, int(k)) for k in rng.integers(1, 500, size=300)]
    seqs += [np.concatenate([_data.random_protein(rng, int(rng.integers(0, 40))), _data.mutate(rng, base, 0.15),
                             _data.random_protein(rng, int(rng.integers(0, 40)))]) for _ in range(20)]
    seqs += [base[:52], base[35:], base.copy(), np.zeros(0, dtype=np.uint8), _data.random_protein(rng, 1)]
    res, off = _oracle.flatten(seqs)
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off, base
    db.close()


def strips_case(capi, strips_set, algo, mode, qlen, kernel, **switches):
    db, res, off, base = strips_set
    query = base[:qlen].copy()
    with capi.tuning(PAIR_STRIPS="1", **switches):
        got = db.search(query, B62, 3, 1, mode, algo)
        assert routed(capi) & 31 == kernel, f"{algo} {mode} Q={qlen}: {capi.DeviceDatabase.last_routing()}"
    assert_same(got, _oracle.search(query, res, off, B62, 3, 1, mode, algo), f"{algo} {mode} Q={qlen}")


@pytest.mark.parametrize("algo,kernel", [("sw", PAIR_STRIPS), ("nw", GLOBAL_STRIPS)])
@pytest.mark.parametrize("qlen", strip_lengths(52))
def test_strips_scores_every_height(capi, strips_set, algo, kernel, qlen):
    strips_case(capi, strips_set, algo, "score", qlen, kernel)


@pytest.mark.parametrize("algo,kernel", [("sw", PAIR_STRIPS), ("nw", GLOBAL_STRIPS)])
@pytest.mark.parametrize("qlen", strip_lengths(48))
def test_strips_end_locations_every_height(capi, strips_set, algo, kernel, qlen):
    strips_case(capi, strips_set, algo, "end", qlen, kernel)


@pytest.mark.parametrize("qlen", strip_lengths(40))
def test_strips_known_optimum_every_height(capi, strips_set, qlen):
    # (MIOPAL_TWO_PASS_ENDS as in test_gpu_biased.py: a scores-only sweep, then the sweep of the KNOWN kernel)
    strips_case(capi, strips_set, "sw", "end", qlen, PAIR_STRIPS, TWO_PASS_ENDS="1")
