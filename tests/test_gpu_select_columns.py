"""The per-target selection alone (miopalTestSelectColumns: the fold and finish kernels of select_columns.hip on rows the
test supplies) against numpy. The reference per column: keep the entries with score >= minScore, sort by (-score, row),
take m. The order is total, so every cut of the rows into pieces, folded in any order, must give the same arrays."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
SENTINEL = 0x5EED5EED   # end-array entries that must never come back
STRIDES = [1, 3, 63, 64, 65, 255, 256, 257, 4097]   # around the 64 columns of a workgroup, and many workgroups
KEYS = ("count", "query", "score", "end_q", "end_t")


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def reference(score, m, min_score, rows_in=None, end_q=None, end_t=None):
    rows, n = score.shape
    rows_in = np.arange(rows) if rows_in is None else np.asarray(sorted(rows_in), dtype=np.int64)
    out = {"count": np.zeros(n, dtype=np.int32), "query": np.full((n, m), -1, dtype=np.int32),
           "score": np.full((n, m), -1, dtype=np.int32)}
    if end_q is not None:
        out.update(end_q=np.full((n, m), -1, dtype=np.int32), end_t=np.full((n, m), -1, dtype=np.int32))
    if len(rows_in) == 0:
        return out
    S = score[rows_in].astype(np.int64)
    keep = S >= min_score
    index = np.broadcast_to(rows_in[:, None], S.shape)
    order = np.lexsort((index, np.where(keep, -S, 2 ** 40)), axis=0)[:m]
    out["count"][:] = np.minimum(m, keep.sum(axis=0))
    cols = np.arange(n)
    for j in range(order.shape[0]):
        has = j < out["count"]
        r = rows_in[order[j]]
        out["query"][has, j] = r[has]
        out["score"][has, j] = score[r, cols][has]
        if end_q is not None:
            out["end_q"][has, j] = end_q[r, cols][has]
            out["end_t"][has, j] = end_t[r, cols][has]
    return out


def end_arrays(rows, n):
    """distinct, recognisable end locations per cell"""
    cell = np.arange(rows, dtype=np.int64)[:, None] * 100003 + np.arange(n, dtype=np.int64)[None, :]
    return cell.astype(np.int32), (-cell - 2).astype(np.int32)


def poisoned(want, end_q, end_t):
    """the end arrays with every cell the answer does not name replaced by the sentinel"""
    named = np.zeros(end_q.shape, dtype=bool)
    t, j = np.nonzero(want["query"] >= 0)
    named[want["query"][t, j], t] = True
    return np.where(named, end_q, SENTINEL).astype(np.int32), np.where(named, end_t, SENTINEL).astype(np.int32)


def same(got, want, what):
    for key in KEYS:
        assert (key in got) == (key in want), (what, key)
        if key in want:
            assert got[key].dtype == np.int32 and got[key].shape == want[key].shape, (what, key)
            assert np.array_equal(got[key], want[key]), (what, key)
    if "end_q" in got:
        assert not np.any(got["end_q"] == SENTINEL) and not np.any(got["end_t"] == SENTINEL), what


def layouts(rng, rows):
    """one piece; one row per piece, last row first; runs of rows in a shuffled order"""
    cuts = np.unique(np.concatenate(([0, rows], rng.integers(0, rows + 1, size=min(rows, 6)))))
    runs = [(int(a), int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])]
    rng.shuffle(runs)
    return {"one piece": [(0, rows)], "rows reversed": [(r, 1) for r in reversed(range(rows))], "runs shuffled": runs}


@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_every_shape_and_every_cut_into_pieces(capi, m):
    rng = np.random.default_rng(100 + m)
    for n in STRIDES:
        for rows in sorted({1, max(m - 1, 1), m, m + 1, 65}):
            # few distinct values: ties inside most columns
            score = rng.integers(-3, 4, size=(rows, n)).astype(np.int32)
            end_q, end_t = end_arrays(rows, n)
            threshold = int(rng.integers(-3, 3))
            want = reference(score, m, threshold, None, end_q, end_t)
            bad_q, bad_t = poisoned(want, end_q, end_t)
            for name, pieces in layouts(rng, rows).items():
                got = capi.select_columns_rows(score, m, threshold, bad_q, bad_t, pieces=pieces)
                same(got, want, (n, rows, name))
            plain = {k: v for k, v in want.items() if not k.startswith("end")}
            same(capi.select_columns_rows(score, m, threshold, pieces=layouts(rng, rows)["runs shuffled"]), plain,
                 (n, rows, "no end arrays"))


@pytest.mark.parametrize("m", [1, 3, 8])
def test_ties(capi, m):
    rng = np.random.default_rng(7)
    rows, n = 65, 257
    end_q, end_t = end_arrays(rows, n)
    # all-equal columns: rows 0 .. m - 1, whatever the order of the pieces
    score = np.broadcast_to(rng.integers(-50, 50, size=n).astype(np.int32), (rows, n)).copy()
    for name, pieces in layouts(rng, rows).items():
        got = capi.select_columns_rows(score, m, None, end_q, end_t, pieces=pieces)
        assert np.all(got["count"] == m) and np.array_equal(got["query"], np.broadcast_to(np.arange(m), (n, m))), name
        same(got, reference(score, m, INT_MIN, None, end_q, end_t), name)
    # values drawn from {0, 1}
    score = rng.integers(0, 2, size=(rows, n)).astype(np.int32)
    for threshold in (0, 1):
        want = reference(score, m, threshold, None, end_q, end_t)
        for name, pieces in layouts(rng, rows).items():
            same(capi.select_columns_rows(score, m, threshold, *poisoned(want, end_q, end_t), pieces=pieces), want,
                 (threshold, name))


@pytest.mark.parametrize("m", [2, 8])
def test_extreme_values_and_thresholds(capi, m):
    rng = np.random.default_rng(8)
    rows, n = 12, 300
    score = rng.choice(np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX], dtype=np.int64),
                       size=(rows, n)).astype(np.int32)
    score[:, 0] = INT_MIN   # a column of nothing but INT_MIN still counts without a bound
    score[:, 1] = INT_MAX
    end_q, end_t = end_arrays(rows, n)
    counts = []
    for threshold in (INT_MIN, INT_MIN + 1, 0, INT_MAX):
        want = reference(score, m, threshold, None, end_q, end_t)
        counts.append(want["count"])
        for name, pieces in layouts(rng, rows).items():
            same(capi.select_columns_rows(score, m, threshold, *poisoned(want, end_q, end_t), pieces=pieces), want,
                 (threshold, name))
    assert counts[0][0] == m and counts[1][0] == 0 and counts[3][1] == m
    assert np.all(counts[0] == m) and (counts[3] < m).any()
    # min_score = None is INT_MIN
    same(capi.select_columns_rows(score, m, None), {k: v for k, v in reference(score, m, INT_MIN).items()}, "no bound")
    # a threshold above every value: nothing anywhere
    score = rng.integers(-100, 100, size=(rows, n)).astype(np.int32)
    got = capi.select_columns_rows(score, m, 100, end_q, end_t, pieces=layouts(rng, rows)["runs shuffled"])
    assert np.all(got["count"] == 0)
    for key in KEYS[1:]:
        assert np.all(got[key] == -1), key


@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_skipped_rows_are_never_read(capi, m):
    rng = np.random.default_rng(30 + m)
    for rows, n in ((1, 65), (m + 1, 64), (9, 257), (65, 4097)):
        score = rng.integers(-20, 20, size=(rows, n)).astype(np.int32)
        end_q, end_t = end_arrays(rows, n)
        skip = rng.random(rows) < 0.4
        skip[0] = True
        kept = np.nonzero(~skip)[0]
        want = reference(score, m, -5, kept, end_q, end_t)
        # a skipped row would win everywhere if it were read
        score[skip] = INT_MAX
        bad_q, bad_t = poisoned(want, end_q, end_t)
        for name, pieces in layouts(rng, rows).items():
            got = capi.select_columns_rows(score, m, -5, bad_q, bad_t, pieces=pieces, skip=skip)
            same(got, want, (rows, n, name))
            assert not np.isin(got["query"], np.nonzero(skip)[0]).any()
        got = capi.select_columns_rows(score, m, -5, pieces=layouts(rng, rows)["rows reversed"], skip=skip)
        same(got, {k: v for k, v in want.items() if not k.startswith("end")}, (rows, n, "no end arrays"))
    # every row skipped, and no piece at all: nothing
    for kw in (dict(skip=np.ones(rows, dtype=bool)), dict(pieces=np.zeros((0, 2), dtype=np.int32))):
        got = capi.select_columns_rows(score, m, None, end_q, end_t, **kw)
        assert np.all(got["count"] == 0) and np.all(got["query"] == -1) and np.all(got["end_t"] == -1)
    # rows in no piece are not part of the answer
    if rows > 2:
        got = capi.select_columns_rows(score[:, :65], m, None, pieces=[(2, rows - 2)], skip=skip)
        same(got, reference(score[:, :65], m, INT_MIN, kept[kept >= 2]), "tail only")
