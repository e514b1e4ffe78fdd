"""A list of (query, target) pairs in one call (miopalAlignPairs, DeviceDatabase.align_pairs, Aligner.align_pairs,
Aligner.top_hits_many(mode="full")): against the CPU checker, against miopalSearch on the one-target slice (the
definition of every output), under the production routing, with the lane-per-pair kernels forced and with the
wavefront-per-pair kernels forced. Every comparison is exact and covers every pair of the list."""
import json
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
QUERY_LENGTHS = [0, 1, 7, 8, 33, 63, 64, 65, 128, 129, 300, 700]
KEYS = {"score": ("score",), "end": ("score", "end_q", "end_t"),
        "full": ("score", "end_q", "end_t", "start_q", "start_t", "aln_off", "aln_flat")}


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def expected(queries, res, off, pq, pt, matrix, go, ge, mode, algo, threads=16):
    """What the CPU checker says about every pair: _oracle.search once per query over the targets that query is
    paired with (in pieces, on a thread pool), gathered back into pair order."""
    pq = np.asarray(pq)
    pt = np.asarray(pt)
    tasks, per_query = [], {}
    for i in np.unique(pq):
        u = np.unique(pt[pq == i])
        per_query[int(i)] = u
        lens = off[u + 1] - off[u]
        # pieces of about 2M cells (a long target alone)
        start, cells = 0, 0
        for k in range(len(u)):
            cells += int(lens[k]) * max(len(queries[i]), 1)
            if cells >= 2_000_000 or k == len(u) - 1:
                tasks.append((int(i), start, k + 1))
                start, cells = k + 1, 0

    def run(task):
        i, lo, hi = task
        u = per_query[i][lo:hi]
        sub_off = np.zeros(len(u) + 1, dtype=np.int64)
        np.cumsum(off[u + 1] - off[u], out=sub_off[1:])
        sub_res = np.concatenate([res[off[t]:off[t + 1]] for t in u]) if len(u) else np.zeros(0, np.uint8)
        if len(sub_res) == 0:
            sub_res = np.zeros(1, np.uint8)
        return _oracle.search(queries[i], sub_res, sub_off, matrix, go, ge, mode, algo)

    with ThreadPoolExecutor(max_workers=threads) as pool:
        parts = list(pool.map(run, tasks))
    n = len(pq)
    out = {key: np.zeros(n, dtype=np.int32) for key in KEYS[mode] if not key.startswith("aln")}
    aln = [None] * n
    for (i, lo, hi), part in zip(tasks, parts):
        u = per_query[i][lo:hi]
        mine = np.nonzero((pq == i) & (pt >= u[0]) & (pt <= u[-1]))[0]
        at = np.searchsorted(u, pt[mine])
        for key in out:
            out[key][mine] = part[key][at]
        if mode == "full":
            for p, k in zip(mine.tolist(), at.tolist()):
                aln[p] = part["aln"][k]
    if mode == "full":
        lens = np.array([len(a) for a in aln], dtype=np.int64)
        out["aln_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        out["aln_flat"] = np.concatenate(aln).astype(np.uint8) if n else np.zeros(0, np.uint8)
    return out


def same(got, want, mode, tag=""):
    for key in KEYS[mode]:
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]), err_msg=f"{key} {tag}")


@pytest.fixture(scope="module")
def pair_set(capi):
    """The database of test_gpu_top.py's db_set (5000 targets of 20-400 residues, two empty ones, one of 35 000),
    queries of every strip boundary, and about 20 000 random pairs with repeats, in random order; the long target
    and the empty ones paired with every query."""
    rng = np.random.default_rng(11)
    lengths = rng.integers(20, 400, size=5000)
    lengths[[3, 1000]] = 0
    lengths[-1] = 35000
    res, off = _data.random_db(rng, lengths)
    db = capi.DeviceDatabase(res, off, 24)
    queries = [_data.random_protein(rng, L) for L in QUERY_LENGTHS]
    nq = len(queries)
    pq = rng.integers(0, nq, size=19_000)
    pt = rng.integers(0, 4999, size=19_000)
    pq[:600], pt[:600] = pq[600:1200], pt[600:1200]   # repeats
    special = np.array([(i, t) for i in range(nq) for t in (3, 1000, 4999)])
    pq = np.concatenate([pq, special[:, 0]])
    pt = np.concatenate([pt, special[:, 1]])
    order = rng.permutation(len(pq))
    yield db, res, off, queries, pq[order].astype(np.int32), pt[order].astype(np.int64)
    db.close()


_expected_cache = {}


def expected_of(pair_set, mode, algo):
    if (mode, algo) not in _expected_cache:
        db, res, off, queries, pq, pt = pair_set
        _expected_cache[(mode, algo)] = expected(queries, res, off, pq, pt, B62, 3, 1, mode, algo)
    return _expected_cache[(mode, algo)]


def check_routing(routing, n, kind):
    assert routing[0] + routing[1] + routing[2] == n, routing
    assert routing[3] >= 1
    if kind == "lanes":
        assert routing[0] > 0, routing
    if kind == "waves":
        assert routing[0] == 0, routing


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("mode", ["score", "end", "full"])
def test_against_the_checker_production_routing(pair_set, small_search_routing, mode, algo):
    db, res, off, queries, pq, pt = pair_set
    got = db.align_pairs(queries, pq, pt, B62, 3, 1, mode, algo)
    routing = db.last_pair_routing()
    check_routing(routing, len(pq), "production")
    assert routing[2] == int(np.count_nonzero((np.diff(off)[pt] == 0) | (np.array(QUERY_LENGTHS)[pq] == 0)))
    same(got, expected_of(pair_set, mode, algo), mode, f"{mode} {algo}")


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("mode", ["score", "end", "full"])
@pytest.mark.parametrize("switch,kind", [("MIOPAL_FORCE_LANE_PER_PAIR", "lanes"), ("MIOPAL_NO_PERPAIR", "waves")])
def test_against_the_checker_forced_routing(pair_set, tuning, switch, kind, mode, algo):
    db, res, off, queries, pq, pt = pair_set
    tuning.setenv(switch, "1")
    got = db.align_pairs(queries, pq, pt, B62, 3, 1, mode, algo)
    check_routing(db.last_pair_routing(), len(pq), kind)
    same(got, expected_of(pair_set, mode, algo), mode, f"{mode} {algo} {switch}")


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("mode", ["score", "end", "full"])
def test_against_the_one_target_search(pair_set, tuning, mode, algo):
    """The definition: entry p equals search(query, start=j, end=j + 1), key by key."""
    db, res, off, queries, pq, pt = pair_set
    rng = np.random.default_rng(5)
    special = np.nonzero((pt == 3) | (pt == 4999))[0]
    pick = np.concatenate([rng.choice(len(pq), size=200, replace=False), special])
    tuning.setenv("MIOPAL_FORCE_LANE_PER_PAIR", "1")
    got = db.align_pairs(queries, pq[pick], pt[pick], B62, 3, 1, mode, algo)
    tuning.delenv("MIOPAL_FORCE_LANE_PER_PAIR")
    assert len(got["score"]) == len(pick)
    for x, p in enumerate(pick.tolist()):
        j = int(pt[p])
        one = db.search(queries[pq[p]], B62, 3, 1, mode, algo, j, j + 1)
        for key in KEYS[mode]:
            if key == "aln_off":
                assert int(one[key][1]) == int(got[key][x + 1] - got[key][x]), (x, key)
            elif key == "aln_flat":
                assert one[key].tolist() == got["aln"][x].tolist(), (x, key)
            else:
                assert int(one[key][0]) == int(got[key][x]), (x, key, mode, algo)


def related(rng, q, n, edits=12, flank=30):
    seqs = []
    for _ in range(n):
        t = q.copy()
        for _ in range(rng.integers(0, edits)):
            k = rng.integers(0, len(t))
            op = rng.integers(0, 3)
            if op == 0:
                t[k] = rng.integers(0, 20)
            elif op == 1 and len(t) > 2:
                t = np.delete(t, k)
            else:
                t = np.insert(t, k, rng.integers(0, 20))
        f = _data.random_protein(rng, int(rng.integers(0, flank)))
        seqs.append(np.concatenate([f, t, f[::-1]]).astype(np.uint8))
    return seqs


def flat_db(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.uint8), off


def all_routes(capi, tuning, queries, res, off, pq, pt, matrix, go, ge, mode, algo, tag):
    want = expected(queries, res, off, pq, pt, matrix, go, ge, mode, algo)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for switch in ("MIOPAL_FORCE_LANE_PER_PAIR", "MIOPAL_NO_PERPAIR"):
            tuning.setenv(switch, "1")
            got = db.align_pairs(queries, pq, pt, matrix, go, ge, mode, algo)
            tuning.delenv(switch)
            check_routing(db.last_pair_routing(), len(pq), "lanes" if "LANE" in switch else "waves")
            same(got, want, mode, f"{tag} {switch}")
    finally:
        db.close()


@pytest.mark.parametrize("algo", ["sw", "nw", "hw", "ov"])
@pytest.mark.parametrize("matrix,go,ge", [(B50, 3, 1), (B50, 4, 0), (B62, 3, 1), (B62, 11, 1), (B62, 2, 2), (B62, 0, 0)],
                         ids=["b50-3-1", "b50-4-0", "b62-3-1", "b62-11-1", "b62-2-2", "b62-0-0"])
def test_gap_models(capi, tuning, algo, matrix, go, ge):
    rng = np.random.default_rng(7 + go)
    res, off = _data.random_db(rng, rng.integers(1, 350, size=300))
    queries = [_data.random_protein(rng, L) for L in (1, 7, 53, 64, 65, 129, 260)]
    pq = rng.integers(0, len(queries), size=1500).astype(np.int32)
    pt = rng.integers(0, 300, size=1500).astype(np.int64)
    all_routes(capi, tuning, queries, res, off, pq, pt, matrix, go, ge, "full", algo, f"{algo} gaps {go}/{ge}")


def test_ties_low_complexity_and_other_matrices(capi, tuning):
    rng = np.random.default_rng(13)
    # related sequences under cheap gaps: the first-maximum rule and the flags' tie-breaks decide
    queries = [_data.random_protein(rng, L) for L in (40, 64, 100, 300)]
    seqs = [t for q in queries for t in related(rng, q, 100)]
    res, off = flat_db(seqs)
    pq = np.repeat(np.arange(4), 100).astype(np.int32)
    pt = np.arange(400, dtype=np.int64)
    cross = rng.integers(0, 400, size=400)
    pq, pt = np.concatenate([pq, rng.integers(0, 4, size=400).astype(np.int32)]), np.concatenate([pt, cross])
    for go, ge in ((3, 1), (1, 1), (6, 2)):
        for algo in ("sw", "ov"):
            all_routes(capi, tuning, queries, res, off, pq, pt, B62, go, ge, "full", algo, f"related {algo} {go}/{ge}")
    # runs of one residue: every cell of a run ties with its neighbours
    seqs = []
    for _ in range(300):
        parts = [np.full(int(rng.integers(1, 25)), rng.integers(0, 4), dtype=np.uint8) for _ in range(int(rng.integers(1, 8)))]
        seqs.append(np.concatenate(parts))
    res, off = flat_db(seqs)
    queries = [np.concatenate([np.full(L // 3, 0), np.full(L // 3, 1), np.full(L - 2 * (L // 3), 0)]).astype(np.uint8)
               for L in (30, 90)]
    pq = rng.integers(0, 2, size=600).astype(np.int32)
    pt = rng.integers(0, 300, size=600).astype(np.int64)
    for go, ge in ((3, 1), (0, 0)):
        for algo in ("sw", "hw", "ov", "nw"):
            all_routes(capi, tuning, queries, res, off, pq, pt, B62, go, ge, "full", algo, f"runs {algo} {go}/{ge}")
    # an asymmetric matrix (the query indexes the rows), and scores that leave int16 on a long NW pair
    asym = B62.reshape(24, 24).copy()
    asym[np.triu_indices(24, 1)] -= 2
    asym = np.ascontiguousarray(asym.ravel(), dtype=np.int32)
    res, off = _data.random_db(rng, rng.integers(1, 200, size=200))
    queries = [_data.random_protein(rng, L) for L in (20, 70, 150)]
    pq = rng.integers(0, 3, size=500).astype(np.int32)
    pt = rng.integers(0, 200, size=500).astype(np.int64)
    for algo in ("sw", "nw", "hw", "ov"):
        all_routes(capi, tuning, queries, res, off, pq, pt, asym, 3, 1, "full", algo, f"asymmetric {algo}")
    q = _data.random_protein(rng, 2100)
    seqs = related(rng, q, 6, edits=40, flank=5) + [_data.random_protein(rng, 2000)]
    res, off = flat_db(seqs)
    pq = np.zeros(7, dtype=np.int32)
    pt = np.arange(7, dtype=np.int64)
    want = expected([q], res, off, pq, pt, B62 * 9, 20, 3, "full", "nw")
    assert want["score"].max() > 32767
    all_routes(capi, tuning, [q], res, off, pq, pt, B62 * 9, 20, 3, "full", "nw", "beyond int16")


def test_large_list_takes_the_lane_kernels(capi, small_search_routing):
    """Enough pairs of short queries for the production routing to choose the lane kernels; uniform target lengths, so
    that the sort reports no outlier head (nothing is twice as long as the 90th percentile)."""
    rng = np.random.default_rng(21)
    res, off = _data.random_db(rng, rng.integers(20, 400, size=5000))
    db = capi.DeviceDatabase(res, off, 24)
    queries = [_data.random_protein(rng, int(L)) for L in rng.integers(20, 65, size=200)]
    n = 120_000
    pq = rng.integers(0, len(queries), size=n).astype(np.int32)
    pt = rng.integers(0, 5000, size=n).astype(np.int64)
    try:
        for algo in ("sw", "nw", "hw", "ov"):
            batch = db.search_batch(queries, B62, 3, 1, "end", algo)
            for mode in ("score", "end", "full"):
                got = db.align_pairs(queries, pq, pt, B62, 3, 1, mode, algo)
                routing = db.last_pair_routing()
                assert routing[1] == 0 and routing[0] + routing[2] == n, routing
                np.testing.assert_array_equal(got["score"], batch["score"][pq, pt], err_msg=f"{mode} {algo}")
                if mode != "score":
                    np.testing.assert_array_equal(got["end_q"], batch["end_q"][pq, pt], err_msg=f"{mode} {algo}")
                    np.testing.assert_array_equal(got["end_t"], batch["end_t"][pq, pt], err_msg=f"{mode} {algo}")
                if mode == "full":
                    # the checker on every pair of a subset of whole queries
                    mine = np.nonzero(pq < 12)[0]
                    want = expected(queries, res, off, pq[mine], pt[mine], B62, 3, 1, "full", algo)
                    for key in ("score", "end_q", "end_t", "start_q", "start_t"):
                        np.testing.assert_array_equal(got[key][mine], want[key], err_msg=f"{key} full {algo}")
                    lens = np.diff(got["aln_off"])
                    np.testing.assert_array_equal(lens[mine], np.diff(want["aln_off"]))
                    flat = np.concatenate([got["aln"][int(p)] for p in mine])
                    np.testing.assert_array_equal(flat, want["aln_flat"])
    finally:
        db.close()


def test_several_chunks(capi, tuning):
    """One very long target paired many times: the direction budget splits the list into several chunks; the answers
    are those of the same pairs one call at a time (device against device), the checker on a handful."""
    rng = np.random.default_rng(23)
    lengths = rng.integers(20, 300, size=400)
    lengths[77] = 8000
    res, off = _data.random_db(rng, lengths)
    db = capi.DeviceDatabase(res, off, 24)
    queries = [_data.random_protein(rng, L) for L in (30, 64, 100, 130)]
    pq = np.concatenate([rng.integers(0, 4, size=6500), rng.integers(0, 4, size=1500)]).astype(np.int32)
    pt = np.concatenate([np.full(6500, 77), rng.integers(0, 400, size=1500)]).astype(np.int64)
    order = rng.permutation(len(pq))
    pq, pt = pq[order], pt[order]
    try:
        for algo in ("nw", "sw"):
            got = db.align_pairs(queries, pq, pt, B62, 3, 1, "full", algo)
            routing = db.last_pair_routing()
            assert routing[3] > 1, routing
            assert routing[0] + routing[1] + routing[2] == len(pq)
            # every distinct pair in a call of its own
            singles = {}
            for p in range(len(pq)):
                key = (int(pq[p]), int(pt[p]))
                if key not in singles:
                    singles[key] = db.align_pairs(queries, [key[0]], [key[1]], B62, 3, 1, "full", algo)
                one = singles[key]
                for name in ("score", "end_q", "end_t", "start_q", "start_t"):
                    assert int(got[name][p]) == int(one[name][0]), (p, name, algo)
                assert got["aln"][p].tolist() == one["aln"][0].tolist(), (p, algo)
            few = np.concatenate([np.nonzero(pt == 77)[0][:4], np.nonzero(pt != 77)[0][:40]])
            want = expected(queries, res, off, pq[few], pt[few], B62, 3, 1, "full", algo)
            for name in ("score", "end_q", "end_t", "start_q", "start_t"):
                np.testing.assert_array_equal(got[name][few], want[name])
            np.testing.assert_array_equal(np.concatenate([got["aln"][int(p)] for p in few]), want["aln_flat"])
    finally:
        db.close()


FIELDS = ("target_index", "score", "query_end", "target_end", "query_start", "target_start", "query_length",
          "target_length", "alignment")


def field(result, name):
    """A field of a result object; None where the reference's property refuses to answer (the -1 locations of an
    empty alignment: src/pyopal/lib.pyx asserts on them)."""
    try:
        return getattr(result, name)
    except AssertionError:
        return None


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y), (x, y)
        for name in FIELDS:
            if hasattr(type(x), name):
                assert field(x, name) == field(y, name), (name, field(x, name), field(y, name))


def test_aligner_align_pairs(capi):
    import pyopal_amd
    aligner = pyopal_amd.Aligner()
    database = pyopal_amd.Database(_data.README_TARGETS)
    queries = [_data.README_QUERY, _data.README_QUERY[10:40], "W"]
    pairs = [(i, j) for i in range(len(queries)) for j in range(len(_data.README_TARGETS))]
    pairs = pairs[::-1] + pairs[:3]
    for mode in ("score", "end", "full"):
        for algo in ("sw", "nw", "hw", "ov"):
            got = aligner.align_pairs(queries, database, pairs, mode=mode, algorithm=algo)
            want = [aligner.align(queries[i], database, mode=mode, algorithm=algo, start=j, end=j + 1)[0] for i, j in pairs]
            same_results(got, want)
            assert [r.target_index for r in got] == [j for _, j in pairs]
            same_results(aligner.align_pairs(queries, database, np.array(pairs), mode=mode, algorithm=algo), want)
    vectors = json.load(open(os.path.join(HERE, "golden", "reference_vectors.json")))["vectors"]
    for vid in ("G3", "G4"):
        v = next(x for x in vectors if x["id"] == vid)
        database = pyopal_amd.Database(v["targets"])
        aligner = pyopal_amd.Aligner(v["matrix"], gap_open=v["gap_open"], gap_extend=v["gap_extend"])
        pairs = [(0, j) for j in range(len(v["targets"]))]
        for mode in ("score", "end", "full"):
            got = aligner.align_pairs([v["query"]], database, pairs, mode=mode, algorithm=v["algorithm"])
            same_results(got, aligner.align(v["query"], database, mode=mode, algorithm=v["algorithm"]))
            for r, s in zip(got, v["score"]):
                assert s is None or r.score == s


def test_top_hits_many_full_is_one_pair_list_call(capi):
    import pyopal_amd
    rng = np.random.default_rng(12)
    seqs = ["".join(rng.choice(list(_data.NCBI[:20]), size=int(L))) for L in rng.integers(1, 200, size=3000)]
    database = pyopal_amd.Database(seqs)
    aligner = pyopal_amd.Aligner()
    queries = [seqs[int(i)][: int(rng.integers(5, 64))] for i in rng.integers(0, 3000, size=200)]
    queries[7] = "W"
    for algo in ("sw", "nw"):
        many = aligner.top_hits_many(queries, database, 7, mode="full", algorithm=algo, start=3, end=2500)
        routing = capi.DeviceDatabase.last_pair_routing()
        assert routing[0] + routing[1] + routing[2] == sum(len(m) for m in many) == 7 * len(queries), routing
        for q, got in zip(queries, many):
            results = sorted(aligner.align(q, database, mode="full", algorithm=algo, start=3, end=2500),
                             key=lambda r: r.score, reverse=True)[:7]
            same_results(got, results)


def test_threads_on_one_handle(pair_set):
    db, res, off, queries, pq, pt = pair_set
    rng = np.random.default_rng(8)
    lists = [rng.choice(len(pq), size=3000, replace=False) for _ in range(4)]
    modes = [("full", "sw"), ("end", "nw"), ("full", "hw"), ("score", "ov")]
    want = [expected_of(pair_set, m, a) for m, a in modes]
    errors = []

    def work(i):
        try:
            mode, algo = modes[i]
            for _ in range(3):
                got = db.align_pairs(queries, pq[lists[i]], pt[lists[i]], B62, 3, 1, mode, algo)
                for key in KEYS[mode]:
                    if key == "aln_off":
                        np.testing.assert_array_equal(np.diff(got[key]), np.diff(want[i][key])[lists[i]])
                    elif key == "aln_flat":
                        w = want[i]
                        flat = np.concatenate([w["aln_flat"][w["aln_off"][p]:w["aln_off"][p + 1]] for p in lists[i]])
                        np.testing.assert_array_equal(got[key], flat)
                    else:
                        np.testing.assert_array_equal(got[key], want[i][key][lists[i]])
        except Exception as e:   # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
