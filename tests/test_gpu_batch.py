"""The batched search (miopalSearchBatch / DeviceDatabase.search_batch / Aligner.align_many_arrays) against the
single-query search of each query and against the CPU checker: every mode, both search types, the row-class
boundaries of the batch kernels, and the pairs they hand to the wavefront-per-pair kernel or the single-query path.
tests/test_gpu_batch_edges.py compares every pair with the CPU checker where the batch path can go wrong: long targets,
several chunks of queries, the planner's range bounds and flag threshold, other alphabets and tied end locations."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B50 = np.array(ScoringMatrix.from_name("BLOSUM50").int_array(), dtype=np.int32)
B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
# (the gap models of the parity tests: the usual ones, opening cheaper than extending, free extension)
MODELS = [(B62, 3, 1), (B50, 10, 1), (B62, 1, 3), (B50, 5, 0)]
# every row-class boundary of the batch kernels (8, 16, ..., 56, 60, 64) and both sides of it
BOUNDARY_LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 47, 48, 49, 55, 56, 57, 59, 60, 61,
                    63, 64]


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def db_set(capi):
    rng = np.random.default_rng(7)
    # above the small-search bound; a few empty targets and a 35 000-residue tail target
    lengths = rng.integers(20, 400, size=5000)
    lengths[[3, 1000]] = 0
    lengths[-1] = 35000
    res, off = _data.random_db(rng, lengths)
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off
    db.close()


def queries_for(rng, count, res, off):
    lengths = (BOUNDARY_LENGTHS * (count // len(BOUNDARY_LENGTHS) + 1))[:count]
    lengths = list(rng.permutation(lengths)) if count > 2 else [60, 1][:count]
    out = []
    for k, L in enumerate(lengths):
        if k % 3 == 0:   # a piece of a target: high scores, end cells inside the target
            t = rng.integers(0, len(off) - 2)
            seg = res[off[t]:off[t + 1]][:L]
            if len(seg) == L:
                out.append(np.array(seg, dtype=np.uint8))
                continue
        out.append(_data.random_protein(rng, int(L)))
    return out


def check_rows(db, queries, got, matrix, go, ge, mode, algo, start=0, end=None):
    for i, q in enumerate(queries):
        want = db.search(q, matrix, go, ge, mode, algo, start=start, end=end)
        np.testing.assert_array_equal(got["score"][i], want["score"], err_msg=f"score of query {i} (Q={len(q)})")
        if mode == "end":
            np.testing.assert_array_equal(got["end_q"][i], want["end_q"], err_msg=f"end_q of query {i} (Q={len(q)})")
            np.testing.assert_array_equal(got["end_t"][i], want["end_t"], err_msg=f"end_t of query {i} (Q={len(q)})")


def check_oracle(queries, got, rows, res, off, matrix, go, ge, mode, algo, start, end):
    sub_off = off[start:end + 1] - off[start]
    sub_res = res[off[start]:off[end]]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        wants = pool.map(lambda i: _oracle.search(queries[i], sub_res, sub_off, matrix, go, ge, mode, algo), rows)
    for i, want in zip(rows, wants):
        np.testing.assert_array_equal(got["score"][i], want["score"], err_msg=f"oracle score {i}")
        if mode == "end":
            np.testing.assert_array_equal(got["end_q"][i], want["end_q"], err_msg=f"oracle end_q {i}")
            np.testing.assert_array_equal(got["end_t"][i], want["end_t"], err_msg=f"oracle end_t {i}")


@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
def test_batch_equals_single_searches(capi, db_set, algo, mode):
    db, res, off = db_set
    rng = np.random.default_rng(["sw", "nw", "hw", "ov"].index(algo) * 2 + (mode == "end"))
    # (the oracle's share: a slice without the 35 000-residue target, a few rows per batch)
    for k, m in enumerate([1, 2, 7, 64, 300]):
        matrix, go, ge = MODELS[k % len(MODELS)]
        queries = queries_for(rng, m, res, off)
        got = db.search_batch(queries, matrix, go, ge, mode, algo)
        routing = db.last_batch_routing()
        assert got["score"].shape == (m, db.count)
        check_rows(db, queries, got, matrix, go, ge, mode, algo)
        sub = db.search_batch(queries, matrix, go, ge, mode, algo, start=0, end=1500)
        # (every row of the batches of at most 64 queries)
        rows = range(m) if m <= 64 else sorted({0, m // 2, m - 1})
        check_oracle(queries, sub, rows, res, off, matrix, go, ge, mode, algo, 0, 1500)
        if (go, ge) == (3, 1):
            # the batch kernels settled the bulk of the pairs, in few launches
            # (61 .. 64 rows: a pair table of 25 symbols does not fit LDS, those queries take the single-query path)
            batched = sum(len(q) <= 60 for q in queries)
            assert routing[0] >= 0.95 * batched * db.count, routing
            assert routing[2] == m - batched and 1 <= routing[3] <= 9, routing


def test_padding_rows_change_nothing_and_zero_optima(capi):
    # Smith-Waterman queries whose best score is 0 against every target (ties everywhere: end cell -1 / -1), in
    # every row class, beside queries whose last rows score exactly like padding would not
    rng = np.random.default_rng(3)
    res, off = _data.random_db(rng, rng.integers(30, 200, size=5000))
    w = _oracle.encode("W")[0]
    d = _oracle.encode("D")[0]
    targets = [np.full(int(L), d, dtype=np.uint8) for L in rng.integers(5, 90, size=4500)]
    zres, zoff = _oracle.flatten(targets + [res[off[k]:off[k + 1]] for k in range(500)])
    db = capi.DeviceDatabase(zres, zoff, 24)
    try:
        queries = [np.full(L, w, dtype=np.uint8) for L in BOUNDARY_LENGTHS]
        queries += [_data.random_protein(rng, L) for L in BOUNDARY_LENGTHS]
        for mode in ("score", "end"):
            for algo in ("sw", "nw", "hw", "ov"):
                for matrix, go, ge in MODELS:
                    got = db.search_batch(queries, matrix, go, ge, mode, algo)
                    check_rows(db, queries, got, matrix, go, ge, mode, algo)
        got = db.search_batch(queries[:len(BOUNDARY_LENGTHS)], B62, 3, 1, "end", "sw", end=4500)
        assert (got["score"] == 0).all() and (got["end_q"] == -1).all() and (got["end_t"] == -1).all()
    finally:
        db.close()


def test_long_queries_take_the_single_query_path(capi, db_set):
    db, res, off = db_set
    rng = np.random.default_rng(11)
    queries = [_data.random_protein(rng, L) for L in (30, 65, 12, 130, 60, 300, 5)]
    for mode, algo in (("end", "sw"), ("score", "hw"), ("end", "ov")):
        got = db.search_batch(queries, B62, 3, 1, mode, algo)
        assert db.last_batch_routing()[2] == 3
        check_rows(db, queries, got, B62, 3, 1, mode, algo)


def test_flagged_lanes_are_recomputed(capi):
    # end locations of 33 .. 64 rows carry 6 row bits: scores above 384 leave the biased lanes' range and go to the
    # int32 kernel; near-copies of the queries among the targets reach that
    rng = np.random.default_rng(5)
    queries = [_data.random_protein(rng, L) for L in (40, 56, 64, 60, 20)]
    queries[0] = np.full(40, _oracle.encode("W")[0], dtype=np.uint8)
    targets = [_data.random_protein(rng, int(L)) for L in rng.integers(50, 300, size=5000)]
    for k in range(0, 5000, 97):
        q = queries[k % len(queries)]
        targets[k] = np.concatenate([targets[k][:20], q, q, targets[k][20:]]).astype(np.uint8)
    res, off = _oracle.flatten(targets)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for mode in ("end", "score"):
            got = db.search_batch(queries, B62, 3, 1, mode, "sw")
            routing = db.last_batch_routing()
            check_rows(db, queries, got, B62, 3, 1, mode, "sw")
            if mode == "end":
                assert routing[1] > 0, routing
        check_oracle(queries, got, [0, 1], res, off, B62, 3, 1, "score", "sw", 0, len(off) - 1)
    finally:
        db.close()


def test_small_slice_and_sub_slices(capi, db_set, tuning):
    db, res, off = db_set
    rng = np.random.default_rng(13)
    queries = queries_for(rng, 40, res, off)
    tuning.delenv("MIOPAL_NO_SMALL_SEARCH")
    for start, end in ((100, 1100), (4000, 5000), (17, 18)):
        for mode, algo in (("end", "sw"), ("score", "nw"), ("end", "hw")):
            got = db.search_batch(queries, B50, 3, 1, mode, algo, start=start, end=end)
            # (61 .. 64 rows: the single-query path, see test_batch_equals_single_searches)
            assert db.last_batch_routing()[1] == sum(len(q) <= 60 for q in queries) * (end - start)
            check_rows(db, queries, got, B50, 3, 1, mode, algo, start, end)
    tuning.setenv("MIOPAL_NO_SMALL_SEARCH", "1")
    for mode, algo in (("end", "sw"), ("end", "ov")):
        got = db.search_batch(queries, B50, 3, 1, mode, algo, start=300, end=4900)
        check_rows(db, queries, got, B50, 3, 1, mode, algo, 300, 4900)


def test_threads_share_a_handle(capi, db_set):
    db, res, off = db_set
    rng = np.random.default_rng(17)
    queries = queries_for(rng, 48, res, off)
    want = {algo: db.search_batch(queries, B62, 3, 1, "end", algo) for algo in ("sw", "hw")}
    errors = []

    def work(t):
        try:
            for rep in range(3):
                algo = ("sw", "hw")[(t + rep) % 2]
                if t % 2 == 0:
                    got = db.search_batch(queries, B62, 3, 1, "end", algo)
                    for key in ("score", "end_q", "end_t"):
                        assert np.array_equal(got[key], want[algo][key]), (t, algo, key)
                else:
                    for i in range(0, len(queries), 7):
                        got = db.search(queries[i], B62, 3, 1, "end", algo)
                        for key in ("score", "end_q", "end_t"):
                            assert np.array_equal(got[key], want[algo][key][i]), (t, algo, key, i)
        except Exception as e:   # noqa: BLE001 - reported below
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_align_many_equals_align(capi):
    import pyopal_amd as pyopal
    rng = np.random.default_rng(23)
    letters = "ARNDCQEGHILKMFPSTWYV"
    targets = ["".join(rng.choice(list(letters), size=int(L))) for L in rng.integers(20, 300, size=4500)]
    database = pyopal.Database(targets)
    queries = ["".join(rng.choice(list(letters), size=int(L))) for L in (5, 64, 33, 80)]
    aligner = pyopal.Aligner()
    for mode in ("score", "end"):
        many = aligner.align_many(queries, database, mode=mode, algorithm="sw", start=10, end=4000)
        assert many == [aligner.align(q, database, mode=mode, algorithm="sw", start=10, end=4000) for q in queries]
        arrays = aligner.align_many_arrays(queries, database, mode=mode, algorithm="hw")
        assert arrays.score.shape == (4, 4500) and arrays.score.dtype == np.int32
        for i, q in enumerate(queries):
            one = aligner.align_arrays(q, database, mode=mode, algorithm="hw")
            assert np.array_equal(arrays[i].score, one.score)
            if mode == "end":
                assert np.array_equal(arrays[i].query_end, one.query_end)
                assert np.array_equal(arrays[i].target_end, one.target_end)
    full = aligner.align_many(queries[:2], database, mode="full", start=0, end=50)
    assert full == [aligner.align(q, database, mode="full", start=0, end=50) for q in queries[:2]]
