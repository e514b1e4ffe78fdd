"""The batched search (miopalSearchBatch) against the CPU checker, pair by pair, where its kernels and its host
planner (interseq_batch_impl.h, host_batch.inc) can go wrong: targets long enough for the lanes to rebase, batches
of several chunks of queries, every acceptance bound of planBatchQuery from both sides, the Smith-Waterman flag
threshold of every row class, other alphabets, and end locations with many ties.

Every test compares every (query, target) pair with the checker (scores and, in end mode, both end coordinates)
and asserts through last_batch_routing() that the pairs went where the planner's rules (mirrored below) send them,
so that no test passes on the fallback path alone. tests/test_gpu_batch.py compares the batch with the
single-query search."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
ALGOS = ("sw", "nw", "hw", "ov")
THREADS = min(16, os.cpu_count() or 1)

# ---- host_batch.inc / common.h mirrored -------------------------------------------------------------------
ROW_CLASSES = (8, 16, 24, 32, 40, 48, 56, 60, 64)      # kBatchRowClasses
CHUNK_PAIRS = 1 << 23                                   # kBatchChunkPairs (a small search: an eighth of it)


def row_class(Q):
    return next((r for r in ROW_CLASSES if Q <= r), 0)


def loc_bits(R):
    return 4 if R <= 16 else 5 if R <= 32 else 6        # locRowBitsHost


def pair_fits(R, n_symbols):
    return n_symbols * n_symbols * (((R + 3) // 4) | 1) * 16 <= 158 * 1024   # interseqPairFits


def sw_limit(R, locate, max_score, go, ge):
    """planBatchQuery's p.biasedLimit: a Smith-Waterman lane at or above it is flagged and redone."""
    bits = loc_bits(R) if locate else 0
    up = max(max_score + ge, ge - go)
    return ((0x7C00 - 0x0C00 - 4096 if locate else 25600) - max(0, (up << bits) - 0x0400)) >> bits


def batch_rows(Q, matrix, go, ge, algo, mode, max_len):
    """planBatchQuery: the row class the batch kernels run a query of Q residues in, 0 for the single-query path."""
    A = int(round(len(matrix) ** 0.5))
    mx, mn = int(np.max(matrix)), int(np.min(matrix))
    if Q < 1 or Q > 64 or go < 0 or ge < 0 or mx > 16383 or mn < -16383:
        return 0
    mag = max(abs(mx), abs(mn))
    if 2 * go + (Q + max_len) * ge + min(Q, max_len) * mag + mag >= 1 << 29:
        return 0
    R = row_class(Q)
    if not pair_fits(R, A + 1) or mn <= -1024:
        return 0
    if algo == "sw":
        bits = loc_bits(R) if mode != "score" else 0
        up = max(mx + ge, ge - go)
        down = max(-(mn + ge), go - ge)
        if (up << bits) > 0x1000 or (down << bits) > (0x800 if mode != "score" else 1024) or 5 * (ge << bits) > 4096:
            return 0
    else:
        if (algo == "nw" and go < ge) or 5 * ge > 4096:
            return 0
        pos = max(mx, 0)
        zero = 0x0400 + 3 * go + (R + 4) * ge + max(0, -mn, 2 * ge)
        if zero + R * (pos + ge) + 4096 + 5 * ge + pos + (R + 4) * ge + go >= 0x7C00:
            return 0
    return R


def query_best(q, matrix):
    """planBatchQuery's queryBest: every residue with its most favourable partner."""
    A = int(round(len(matrix) ** 0.5))
    return int(np.asarray(matrix).reshape(A, A)[np.asarray(q, dtype=np.int64)].max(axis=1, initial=0).sum())


# ---- checker and comparisons ------------------------------------------------------------------------------
def checker(queries, res, off, matrix, go, ge, algo, mode="end", rows=None):
    """The checker's answers, {row: dict}, for the queries `rows` (all by default) against every target; pieces of
    about 2^18 residues of the database run in parallel. End mode holds the scores too."""
    rows = range(len(queries)) if rows is None else rows
    lens = np.diff(off)
    bounds, acc = [0], 0
    for k, L in enumerate(lens):
        acc += int(L)
        if acc >= 1 << 18:
            bounds.append(k + 1)
            acc = 0
    if bounds[-1] != len(lens):
        bounds.append(len(lens))

    def run(task):
        i, lo, hi = task
        return _oracle.search(queries[i], res[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], matrix, go, ge, mode, algo)

    tasks = [(i, bounds[k], bounds[k + 1]) for i in rows for k in range(len(bounds) - 1)]
    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        parts = list(pool.map(run, tasks))
    out, at = {}, 0
    for i in rows:
        p = parts[at:at + len(bounds) - 1]
        at += len(bounds) - 1
        out[i] = {key: np.concatenate([x[key] for x in p]) for key in p[0]}
    return out


def assert_pairs(got, want, mode, what, rows=None):
    """Every pair of the rows `rows` (all of `want` by default) equals the checker's."""
    for i in (want if rows is None else rows):
        keys = ("score", "end_q", "end_t") if mode == "end" else ("score",)
        for key in keys:
            np.testing.assert_array_equal(got[key][i], want[i][key], err_msg=f"{what}: {key} of query {i}")


def pair_jobs(plan, want, off, matrix, go, ge, algo, mode):
    """The pairs of batched queries the lanes hand to the wavefront-per-pair kernel: targets longer than
    kLongTarget (8192, host.hip), empty targets of NW / HW / OV, and Smith-Waterman pairs whose true score is at or
    above the flag threshold (every one of them: below it a lane is exact, and its best never falls back)."""
    lens = np.diff(off)
    rows = [i for i, R in enumerate(plan) if R]
    jobs = len(rows) * int((lens > 8192).sum())
    if algo != "sw":
        return jobs + len(rows) * int((lens == 0).sum())
    mx = int(np.max(matrix))
    return jobs + sum(int(((want[i]["score"] >= sw_limit(plan[i], mode != "score", mx, go, ge)) & (lens <= 8192)).sum())
                      for i in rows)


def assert_routing(routing, plan, n, *, small=False, jobs=None):
    """Queries the planner refuses take the single-query path; every pair of the others is settled exactly once,
    by the batch lanes or the wavefront-per-pair kernel (all of them on the latter in a small search); `jobs`:
    the number of pairs on the latter (pair_jobs)."""
    batched = sum(1 for R in plan if R)
    assert routing[2] == len(plan) - batched, (routing, plan)
    assert routing[0] + routing[1] == batched * n, (routing, batched, n)
    if jobs is not None:
        assert routing[1] == jobs, (routing, jobs)
    if small:
        assert routing[0] == 0 and routing[3] == 0, routing
    elif batched:
        assert routing[0] > 0 and routing[3] >= 1, routing


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def _segment_into(target, piece, at):
    """target with `piece` written over it from `at` on (the length stays)."""
    t = target.copy()
    piece = piece[:len(t) - at]
    t[at:at + len(piece)] = piece
    return t


# ---- 1. long targets in the lanes: the rebase of both kernels, NW over 8192 columns, far end columns -------------
LONG_MODELS = [(3, 1), (11, 1), (1, 3), (5, 0), (0, 0), (14, 12), (40, 12)]
# one query in every row class that holds 25 symbols (61 .. 64 do not: test_other_alphabets) and both sides of
# every boundary
LONG_QUERY_LENGTHS = [1, 8, 9, 15, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 59, 60]


@pytest.fixture(scope="module")
def long_set(capi):
    rng = np.random.default_rng(101)
    lengths = np.exp(rng.uniform(np.log(400), np.log(8192), size=300)).astype(np.int64)
    lengths = np.concatenate([[0], lengths, np.arange(4093, 4101), [8192, 8192, 8193, 0]])
    targets = [_data.random_protein(rng, int(L)) for L in lengths]
    queries = [_data.random_protein(rng, L) for L in LONG_QUERY_LENGTHS]
    # related sequences: near-copies of the queries far into long targets (high Smith-Waterman scores, end columns
    # past the rebase and at the very end), and queries cut from far into long targets (high HW / OV scores)
    long_ids = [k for k, L in enumerate(lengths) if L >= 4093]
    for k, q in enumerate(queries):
        for t in rng.choice(long_ids, size=3, replace=False):
            L = len(targets[t])
            copy = _data.mutate(rng, q, 0.1) if k % 2 else q
            at = L - len(copy) if L < 4300 or rng.random() < 0.5 else int(rng.integers(4096, L - len(copy)))
            targets[t] = _segment_into(targets[t], copy, at)
    for k in range(1, len(queries), 3):
        t = targets[long_ids[k % len(long_ids)]]
        at = int(rng.integers(4100, len(t) - len(queries[k])))
        queries[k] = t[at:at + len(queries[k])].copy()
    res, off = _oracle.flatten(targets)
    assert list(np.diff(off)[-4:]) == [8192, 8192, 8193, 0]
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off, queries
    db.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_long_targets(capi, long_set, algo):
    db, res, off, queries = long_set
    max_len = int(np.diff(off).max())
    for go, ge in LONG_MODELS:
        if algo == "nw" and go < ge:
            continue
        want = checker(queries, res, off, B62, go, ge, algo)
        for mode in ("score", "end"):
            plan = [batch_rows(len(q), B62, go, ge, algo, mode, max_len) for q in queries]
            assert all(plan), (go, ge, algo, mode)
            got = db.search_batch(queries, B62, go, ge, mode, algo)
            routing = db.last_batch_routing()
            assert routing[0] > 0 and routing[2] == 0, routing
            assert_routing(routing, plan, db.count, jobs=pair_jobs(plan, want, off, B62, go, ge, algo, mode))
            assert_pairs(got, want, mode, f"{algo} {mode} {go}/{ge}")
        if algo == "sw" and (go, ge) == (3, 1):
            # (the near-copies did what they are for: high scores with best cells far past the first rebase)
            assert sum(((w["end_t"] > 4096) & (w["score"] >= 100)).sum() for w in want.values()) >= 20


# ---- 2. the Smith-Waterman flag threshold of every row class -----------------------------------------------------
# Alphabet of 4 (every row class holds it). The query is X^Q; X scores M, M - 1, M - 2, M - 3 against X, Y, Z, W, so
# a target of i residues (i <= Q) scores any i M - d, 0 <= d <= 3 i, aligned whole. Every other entry is -2.
def flag_matrix(M):
    S = np.full((4, 4), -2, dtype=np.int32)
    S[0] = [M, M - 1, M - 2, M - 3]
    S[1, 1] = S[2, 2] = S[3, 3] = 1
    return S.ravel()


def flag_db(capi):
    # target (i, d): i residues, deficit d against X^Q: d // 3 W, then a Z (2) or Y (1), the rest X
    targets = []
    for i in range(1, 65):
        for d in range(0, 3 * i + 1):
            w, rest = divmod(d, 3)
            t = [3] * w + ([rest] if rest else []) + [0] * (i - w - (1 if rest else 0))
            targets.append(np.array(t, dtype=np.uint8))
    rng = np.random.default_rng(202)
    targets += [rng.integers(0, 4, size=int(L)).astype(np.uint8) for L in rng.integers(1, 300, size=200)]
    res, off = _oracle.flatten(targets)
    return capi.DeviceDatabase(res, off, 4), res, off


def flag_scheme(R, Q, locate, go, ge, shrink):
    """A match score M whose reachable scores cover limit - 3 .. limit + 3 with room above; with `shrink`, one whose
    step up (M + ext) << bits is far above 0x0400, where the limit shrinks by the excess."""
    bits = loc_bits(R) if locate else 0
    top = (0x1000 >> bits) - ge
    cands = range(top, 3, -1) if shrink else range(4, min(top, (0x0400 >> bits) - ge) + 1)
    for M in cands:
        lim = sw_limit(R, locate, M, go, ge)
        if shrink and ((M + ge) << bits) < 0x0400 + 0x0200:
            break
        reach = [(i * (M - 3), i * M) for i in range(1, Q + 1)]
        covered = all(any(lo <= v <= hi for lo, hi in reach) for v in range(lim - 3, lim + 4))
        if covered and Q * M >= lim + 64:
            return M, lim
    return None


@pytest.mark.parametrize("locate", [False, True], ids=["score", "end"])
def test_sw_flag_threshold(capi, locate):
    db, res, off = flag_db(capi)
    mode = "end" if locate else "score"
    go, ge = 5, 1
    try:
        cases = []
        for R in ROW_CLASSES:
            for shrink in (False, True):
                s = flag_scheme(R, R, locate, go, ge, shrink)
                if s is not None:
                    cases.append((R, shrink) + s)
            assert any(c[0] == R for c in cases), R
        # the limit shrinks in some class of every search type, and every class flags at 4, 5 and 6 row bits
        assert any(c[1] for c in cases)
        flagged_far = False
        for R, shrink, M, lim in cases:
            S = flag_matrix(M)
            queries = [np.zeros(R, dtype=np.uint8), np.zeros(max(R - 3, 1), dtype=np.uint8)]
            queries.append(np.array(([0, 1, 2, 3] * 16)[:R], dtype=np.uint8))
            plan = [batch_rows(len(q), S, go, ge, "sw", mode, int(np.diff(off).max())) for q in queries]
            assert plan[0] == R and row_class(len(queries[1])) == R, (R, plan)
            assert sw_limit(R, locate, int(S.max()), go, ge) == lim
            got = db.search_batch(queries, S, go, ge, mode, "sw")
            routing = db.last_batch_routing()
            want = checker(queries, res, off, S, go, ge, "sw", mode)
            scores = want[0]["score"]
            # (the checker's own scores show that the threshold is hit on both sides, densely)
            for v in range(lim - 2, lim + 3):
                assert (scores == v).any(), (R, M, lim, v)
            # every pair at or above the limit was redone, and no other
            jobs = pair_jobs(plan, want, off, S, go, ge, "sw", mode)
            assert jobs >= (scores >= lim).sum() > 0
            assert_routing(routing, plan, db.count, jobs=jobs)
            flagged_far = flagged_far or scores.max() >= 0x7C00
            assert_pairs(got, want, mode, f"R={R} M={M} limit={lim}")
        if not locate:
            assert flagged_far   # (a true score above the 16-bit lane's whole range)
        # queryBest below the limit: the flags are never read back, and nothing may need them
        M = 5
        S = flag_matrix(M)
        queries = [np.zeros(Q, dtype=np.uint8) for Q in (8, 40, 64)]
        assert all(query_best(q, S) < sw_limit(row_class(len(q)), locate, M, go, ge) for q in queries)
        got = db.search_batch(queries, S, go, ge, mode, "sw")
        routing = db.last_batch_routing()
        assert routing[0] == len(queries) * db.count and routing[1] == 0 and routing[2] == 0, routing
        assert_pairs(got, checker(queries, res, off, S, go, ge, "sw", mode), mode, "queryBest < limit")
    finally:
        db.close()


# ---- 3. the acceptance bounds of planBatchQuery, one unit inside and one outside ---------------------------------
def edge_matrix(max_score, min_score):
    """Alphabet of 4: X scores max_score against itself; W scores min_score against every other letter (and they
    against it), the rest is small."""
    S = np.array([[2, -1, -1, 0], [-1, 3, -2, 0], [-1, -2, 1, 0], [0, 0, 0, 1]], dtype=np.int32)
    S[0, 0] = max_score
    S[:3, 3] = min_score
    S[3, :3] = min_score
    return S.ravel()


def edge_cases():
    """(label, algo, mode, Q, max_score, min_score, go, ge, inside)"""
    out = []

    def both(label, algo, mode, Q, inner, outer):
        out.append((label + "/in", algo, mode, Q) + inner + (True,))
        out.append((label + "/out", algo, mode, Q) + outer + (False,))

    # Smith-Waterman, scores (0 row bits): the step up, the step down (open - ext), the pad bound, ext
    for Q in (8, 64):
        both(f"sw-up-{Q}", "sw", "score", Q, (4095, -4, 3, 1), (4096, -4, 3, 1))
        both(f"sw-open-ext-{Q}", "sw", "score", Q, (11, -4, 1025, 1), (11, -4, 1026, 1))
        both(f"sw-pad-{Q}", "sw", "score", Q, (11, -1023, 3, 0), (11, -1024, 3, 0))
        both(f"sw-ext-{Q}", "sw", "score", Q, (11, -4, 900, 819), (11, -4, 900, 820))
    # Smith-Waterman, end locations at 4, 5 and 6 row bits
    for Q, bits in ((8, 4), (32, 5), (40, 6), (64, 6)):
        k = 0x1000 >> bits
        both(f"swl-up-{Q}", "sw", "end", Q, (k - 1, -4, 3, 1), (k, -4, 3, 1))
        g = 0x800 >> bits
        both(f"swl-down-{Q}", "sw", "end", Q, (11, -(g + 1), 3, 1), (11, -(g + 2), 3, 1))
        both(f"swl-open-ext-{Q}", "sw", "end", Q, (11, -4, g + 1, 1), (11, -4, g + 2, 1))
        e = 4096 // (5 << bits)
        both(f"swl-ext-{Q}", "sw", "end", Q, (11, -4, e + 2, e), (11, -4, e + 2, e + 1))
    # NW / HW / OV: the zero bound (largest match score inside), the pad bound, NW's open >= ext
    for algo in ("nw", "hw", "ov"):
        for Q in (8, 64):
            R = row_class(Q)
            go, ge, mn = 3, 1, -4
            zero = 0x0400 + 3 * go + (R + 4) * ge + max(0, -mn, 2 * ge)
            pos = (0x7C00 - 1 - zero - R * ge - 4096 - 5 * ge - (R + 4) * ge - go) // (R + 1)
            for mode in ("score", "end"):
                both(f"{algo}-zero-{Q}-{mode}", algo, mode, Q, (pos, mn, go, ge), (pos + 1, mn, go, ge))
            both(f"{algo}-pad-{Q}", algo, "end", Q, (4, -1023, go, ge), (4, -1024, go, ge))
    both("nw-open-ext", "nw", "end", 40, (6, -4, 3, 3), (6, -4, 2, 3))
    return out


@pytest.fixture(scope="module")
def edge_set(capi):
    rng = np.random.default_rng(303)
    targets = [np.zeros(0, dtype=np.uint8)]
    targets += [np.zeros(L, dtype=np.uint8) for L in range(1, 72)]                  # all-match (X runs)
    targets += [np.full(L, 3, dtype=np.uint8) for L in (1, 5, 40, 64, 200)]          # all-mismatch (W runs)
    targets += [rng.integers(0, 3, size=int(L)).astype(np.uint8) for L in rng.integers(1, 400, size=300)]
    # near-copies of the queries below (X runs with a few changes) and long targets for the global modes
    for L in (8, 40, 64):
        for _ in range(4):
            t = np.zeros(L + 20, dtype=np.uint8)
            t[rng.integers(0, L + 20, size=2)] = rng.integers(1, 3, size=2)
            targets.append(t)
    targets += [np.zeros(L, dtype=np.uint8) for L in (4096, 8192)]
    targets += [rng.integers(0, 4, size=L).astype(np.uint8) for L in (5000, 8192)]
    targets += [_segment_into(rng.integers(0, 3, size=8192).astype(np.uint8), np.zeros(64, np.uint8), 8100)]
    res, off = _oracle.flatten(targets)
    db = capi.DeviceDatabase(res, off, 4)
    yield db, res, off
    db.close()


@pytest.mark.parametrize("k", range(len(edge_cases())), ids=[c[0] for c in edge_cases()])
def test_scheme_edges(capi, edge_set, k):
    label, algo, mode, Q, mx, mn, go, ge, inside = edge_cases()[k]
    db, res, off = edge_set
    rng = np.random.default_rng(k)
    S = edge_matrix(mx, mn)
    R = row_class(Q)
    # (and the shortest query of the class)
    queries = [np.zeros(Q, dtype=np.uint8), rng.integers(0, 3, size=Q).astype(np.uint8),
               np.zeros(max([r for r in ROW_CLASSES if r < R], default=0) + 1, dtype=np.uint8)]
    max_len = int(np.diff(off).max())
    plan = [batch_rows(len(q), S, go, ge, algo, mode, max_len) for q in queries]
    # (the scheme sits where its label says: one unit inside the bound, or one outside)
    assert plan == [R if inside else 0] * len(queries), (label, plan)
    got = db.search_batch(queries, S, go, ge, mode, algo)
    routing = db.last_batch_routing()
    want = checker(queries, res, off, S, go, ge, algo, mode)
    assert_routing(routing, plan, db.count, jobs=pair_jobs(plan, want, off, S, go, ge, algo, mode))
    if inside:
        assert routing[2] == 0 and routing[0] > 0, routing
    else:
        assert routing[2] == len(queries), routing
    assert_pairs(got, want, mode, label)


# ---- 4. batches of several chunks ------------------------------------------------------------------------------
def chunk_queries(rng, count, rows_per_chunk, single_chunk, flag_rows, w):
    """Queries of 1 .. 64 residues, with longer ones and empty ones on every chunk boundary, one chunk of the
    single-query path only, and W runs (flagged Smith-Waterman lanes at end locations) at `flag_rows`."""
    queries = [_data.random_protein(rng, int(L)) for L in rng.integers(1, 65, size=count)]
    for i0 in range(rows_per_chunk, count, rows_per_chunk):
        queries[i0 - 1] = _data.random_protein(rng, 70)
        queries[i0] = np.zeros(0, dtype=np.uint8)
        if i0 + 1 < count:
            queries[i0 + 1] = _data.random_protein(rng, int(rng.integers(33, 61)))
    lo = single_chunk * rows_per_chunk
    for i in range(lo, min(count, lo + rows_per_chunk)):
        queries[i] = _data.random_protein(rng, int(rng.integers(65, 90))) if i % 5 else np.zeros(0, np.uint8)
    for i in flag_rows:
        queries[i] = np.full(int(rng.integers(36, 61)), w, dtype=np.uint8)
    return queries


def boundary_rows(count, rows_per_chunk):
    rows = {0, count - 1}
    for i0 in range(rows_per_chunk, count, rows_per_chunk):
        rows |= {i0 - 1, i0, min(i0 + 1, count - 1)}
    return sorted(rows)


def run_chunks(db, res, off, queries, rows_per_chunk, runs, small):
    max_len = int(np.diff(off).max())
    check = boundary_rows(len(queries), rows_per_chunk)
    for algo, mode in runs:
        got = db.search_batch(queries, B62, 3, 1, mode, algo)
        routing = db.last_batch_routing()
        plan = [batch_rows(len(q), B62, 3, 1, algo, mode, max_len) for q in queries]
        assert_routing(routing, plan, db.count, small=small)
        if algo == "sw" and mode == "end":
            assert routing[1] > 0, routing
        for i, q in enumerate(queries):
            one = db.search(q, B62, 3, 1, mode, algo)
            for key in ("score", "end_q", "end_t") if mode == "end" else ("score",):
                np.testing.assert_array_equal(got[key][i], one[key], err_msg=f"{algo} {mode}: {key} of row {i}")
        assert_pairs(got, checker(queries, res, off, B62, 3, 1, algo, mode, rows=check), mode, f"{algo} {mode}")
    return check


def test_several_chunks(capi):
    rng = np.random.default_rng(404)
    n = 70000
    lengths = rng.integers(10, 41, size=n)
    lengths[[5, n - 1]] = 0
    res, off = _data.random_db(rng, lengths)
    w = _oracle.encode("W")[0]
    # W runs among the targets: scores of 11 a residue, above the 6-row-bit limit (384) against the W queries
    for k in range(100, n, 997):
        res[off[k]:off[k + 1]] = w
    rows_per_chunk = CHUNK_PAIRS // n
    assert rows_per_chunk == 119
    count = 4 * rows_per_chunk + 24                       # five chunks, the fourth of single-query rows only
    flag_rows = [rows_per_chunk + 1, rows_per_chunk + 50, 2 * rows_per_chunk + 1, 2 * rows_per_chunk + 3]
    queries = chunk_queries(rng, count, rows_per_chunk, 3, flag_rows, w)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        check = run_chunks(db, res, off, queries, rows_per_chunk,
                           [("sw", "end"), ("nw", "score"), ("hw", "end"), ("ov", "score")], small=False)
        assert {118, 119, 120, 356, 357, 475, 476} <= set(check)
    finally:
        db.close()


def test_several_chunks_small_search(capi, tuning):
    tuning.delenv("MIOPAL_NO_SMALL_SEARCH")
    rng = np.random.default_rng(405)
    n = 4000
    lengths = rng.integers(10, 120, size=n)
    lengths[[0, 17]] = 0
    res, off = _data.random_db(rng, lengths)
    w = _oracle.encode("W")[0]
    for k in range(3, n, 211):
        res[off[k]:off[k + 1]] = w
    rows_per_chunk = CHUNK_PAIRS // 8 // n
    assert rows_per_chunk == 262
    count = 2 * rows_per_chunk + 90
    queries = chunk_queries(rng, count, rows_per_chunk, 1, [5, 2 * rows_per_chunk + 2], w)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        run_chunks(db, res, off, queries, rows_per_chunk, [("sw", "end"), ("hw", "score"), ("ov", "end")], small=True)
    finally:
        db.close()


# ---- 5. other alphabets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A, go, ge", [(4, 5, 2), (20, 3, 1), (32, 10, 1)])
def test_other_alphabets(capi, A, go, ge):
    rng = np.random.default_rng(500 + A)
    S = rng.integers(-5, 7, size=(A, A)).astype(np.int32)
    S[np.arange(A), np.arange(A)] += 5                   # (asymmetric: S[a][b] != S[b][a] in general)
    S = S.ravel()
    lengths = rng.integers(20, 400, size=1000)
    lengths[[2, 999]] = 0
    targets = [rng.integers(0, A, size=int(L)).astype(np.uint8) for L in lengths]
    qlens = [1, 2, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 56, 57, 59, 60, 61, 62, 63, 64]
    queries = [rng.integers(0, A, size=L).astype(np.uint8) for L in qlens]
    for k in range(0, len(targets), 40):   # near-copies: high scores, end cells inside the targets
        q = queries[(k // 40) % len(queries)]
        t = targets[k]
        targets[k] = np.concatenate([t[:len(t) // 2], q, t[len(t) // 2:]]).astype(np.uint8)
    res, off = _oracle.flatten(targets)
    max_len = int(np.diff(off).max())
    db = capi.DeviceDatabase(res, off, A)
    try:
        for algo in ALGOS:
            want = checker(queries, res, off, S, go, ge, algo)
            for mode in ("score", "end"):
                plan = [batch_rows(len(q), S, go, ge, algo, mode, max_len) for q in queries]
                # (what interseqPairFits implies: every class holds 5 and 21 symbols, 33 only up to 32 rows)
                assert plan == [row_class(len(q)) if (A < 32 or len(q) <= 32) else 0 for q in queries], plan
                got = db.search_batch(queries, S, go, ge, mode, algo)
                routing = db.last_batch_routing()
                assert_routing(routing, plan, db.count, jobs=pair_jobs(plan, want, off, S, go, ge, algo, mode))
                assert routing[2] == (sum(len(q) > 32 for q in queries) if A == 32 else 0), routing
                assert_pairs(got, want, mode, f"A={A} {algo} {mode}")
    finally:
        db.close()


# ---- 6. end locations with many ties ----------------------------------------------------------------------------
def test_tie_rich_end_locations(capi):
    rng = np.random.default_rng(606)
    S = np.where(np.eye(4, dtype=bool), 2, -1).astype(np.int32).ravel()
    queries = []
    for L in (1, 7, 8, 9, 16, 17, 23, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 60, 61, 64):
        kind = len(queries) % 3
        unit = [[0], [0, 1], [0, 1, 2]][kind]
        queries.append(np.array((unit * 64)[:L], dtype=np.uint8))
    targets = [np.zeros(0, dtype=np.uint8)]
    targets += [np.full(L, c, dtype=np.uint8) for L in range(1, 90, 4) for c in (0, 1)]
    for unit in ([0, 1], [1, 0], [0, 1, 2], [2, 0, 1], [0, 0, 1]):
        targets += [np.array((unit * 100)[:L], dtype=np.uint8) for L in range(2, 160, 7)]
    for q in queries:   # two copies of the query, apart and back to back
        gap = rng.integers(0, 4, size=int(rng.integers(1, 20))).astype(np.uint8)
        targets += [np.concatenate([q, gap, q]), np.concatenate([q, q]), np.concatenate([gap, q, gap, q, gap])]
    targets += [rng.integers(0, 4, size=int(L)).astype(np.uint8) for L in rng.integers(1, 300, size=150)]
    res, off = _oracle.flatten(targets)
    max_len = int(np.diff(off).max())
    db = capi.DeviceDatabase(res, off, 4)
    try:
        for go, ge in ((3, 1), (1, 1)):
            for algo in ("sw", "hw", "ov"):
                plan = [batch_rows(len(q), S, go, ge, algo, "end", max_len) for q in queries]
                assert all(plan), plan
                got = db.search_batch(queries, S, go, ge, "end", algo)
                routing = db.last_batch_routing()
                want = checker(queries, res, off, S, go, ge, algo)
                assert_routing(routing, plan, db.count, jobs=pair_jobs(plan, want, off, S, go, ge, algo, "end"))
                assert_pairs(got, want, "end", f"{algo} {go}/{ge}")
    finally:
        db.close()
