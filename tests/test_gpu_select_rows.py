"""The device top-k selection (select_top.hip: range, histogram rounds, scan, look-back gather, bitonic sort) on rows
built for each of its arms, through the test hook miopalTestSelectTop (_capi.select_top_rows): no DP in front of it.
The reference is numpy.lexsort on (index, -score), filtered by min_score and cut at k; every comparison is exact.

Sizes (select_top.h): a 16-byte slot holds 4 scores, a block 256 threads x 4 slots = 4096 scores (16 384 bytes), a
histogram round 4096 bins, a group of rows 1024. The cases sit at those edges - and at 16 384 scores as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
BLOCK = 4096        # scores per block (kTopBlockSlots x 4)
BINS = 4096         # kTopBins
MAX_K = 4096        # MIOPAL_MAX_TOP


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def reference(row, k, min_score=None):
    order = np.lexsort((np.arange(len(row)), -row.astype(np.int64)))
    if min_score is not None:
        order = order[row[order] >= min_score]
    return order[:k]


def end_arrays(rows, stride):
    """Injective in (row, index): a gather from another row or position shows."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    i = np.arange(stride, dtype=np.int64)[None, :]
    end_q = (r * 7 + 3 * i).astype(np.int32)
    return end_q, ~end_q


def check(capi, score, k, min_score=None, ends=False, start=0, rows_to_check=None):
    score = np.ascontiguousarray(score, dtype=np.int32)
    if score.ndim == 1:
        score = score[None, :]
    rows, stride = score.shape
    end_q = end_t = None
    if ends:
        end_q, end_t = end_arrays(rows, stride)
    got = capi.select_top_rows(score, k, min_score=min_score, end_q=end_q, end_t=end_t, start=start)
    where = (rows, stride, k, min_score, start)
    assert got["gave_up"] == 0, where
    assert got["count"].shape == (rows,) and got["target"].shape == (rows, k) and got["score"].shape == (rows, k)
    assert ("end_q" in got) == ends and ("end_t" in got) == ends
    for r in (range(rows) if rows_to_check is None else rows_to_check):
        order = reference(score[r], k, min_score)
        c = len(order)
        at = where + (r,)
        assert int(got["count"][r]) == c, at + (int(got["count"][r]), c)
        assert np.array_equal(got["target"][r, :c], start + order), at
        assert np.array_equal(got["score"][r, :c], score[r, order]), at
        assert np.all(got["target"][r, c:] == -1) and np.all(got["score"][r, c:] == -1), at
        if ends:
            assert np.array_equal(got["end_q"][r, :c], end_q[r, order]), at
            assert np.array_equal(got["end_t"][r, :c], end_t[r, order]), at
            assert np.all(got["end_q"][r, c:] == -1) and np.all(got["end_t"][r, c:] == -1), at
    return got


def wide(rng, shape):
    return rng.integers(INT_MIN, INT_MAX + 1, size=shape, dtype=np.int64).astype(np.int32)


def shift_for(span):
    sh = 0
    while (span >> sh) >= BINS:
        sh += 1
    return sh


def spread(rng, n, lo, hi):
    """n int64 values of [lo, hi] with both ends present (n >= 2 unless lo == hi)."""
    v = rng.integers(lo, hi + 1, size=n, dtype=np.int64)
    if n >= 2:
        a, b = rng.choice(n, size=2, replace=False)
        v[a], v[b] = lo, hi
    return v


# ---- slot and block geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3, 4, 5, 4093, 4095, 4096, 4097, 8191, 8193, 16383, 16384, 16385, 32768, 32769])
def test_slot_and_block_geometry(capi, stride):
    """Rows of odd strides start at all four phases inside a 16-byte slot; strides one below, at and above a block (4096
    scores) and 16 384; k up to and above the stride."""
    rng = np.random.default_rng(1000 + stride)
    for rows in (1, 2, 3, 5):
        narrow = rng.integers(0, 51, size=(rows, stride)).astype(np.int32)
        full = wide(rng, (rows, stride))
        for k in sorted({1, 4, min(stride, MAX_K), min(stride + 5, MAX_K)}):
            check(capi, narrow, k, ends=True)
            check(capi, full, k, ends=rows == 3)


# ---- histogram rounds -------------------------------------------------------------------------------------------------
SPANS = [0, 1, 4095, 4096, 4097, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 + 12345, 2 ** 32 - 1]


def span_base(span):
    if span == 2 ** 32 - 1:
        return INT_MIN                      # a row that holds INT_MIN and INT_MAX
    if span > 2 ** 31:
        return -(2 ** 30) - 12345           # negative and positive values
    return -span // 3 - 7                   # across the sign for every other span as well


@pytest.mark.parametrize("span", SPANS)
def test_histogram_rounds(capi, span):
    """max - min around the 4096 bins of one round, around the 2^24 of two, and beyond: k below, at and above the
    number of entries, in rows of 20 001 and of 3000 entries."""
    rng = np.random.default_rng(span % 99991)
    lo = span_base(span)
    for stride, ks in ((20001, (1, 100, MAX_K)), (3000, (1, 2999, 3000, 3005))):
        rows = np.stack([spread(rng, stride, lo, lo + span), spread(rng, stride, lo, lo + span)]).astype(np.int32)
        assert int(rows[0].max()) - int(rows[0].min()) == span
        for k in ks:
            check(capi, rows, k)
    # the same range with a handful of distinct values: ties inside every round
    few = rng.choice(spread(rng, 7, lo, lo + span), size=(2, 20001)).astype(np.int32)
    for k in (1, 100, MAX_K):
        check(capi, few, k)


def row_across_an_edge(rng, stride, lo, hi, edge, k):
    """k entries >= edge, edge among them; the others < edge, edge - 1 among them; lo and hi present."""
    assert lo < edge <= hi and 2 <= k <= stride - 2
    v = np.empty(stride, dtype=np.int64)
    v[:k] = rng.integers(edge, hi + 1, size=k)
    v[0], v[1] = edge, hi
    v[k:] = rng.integers(lo, edge, size=stride - k)
    v[k], v[k + 1] = edge - 1, lo
    return v[rng.permutation(stride)].astype(np.int32)


@pytest.mark.parametrize("span", [s for s in SPANS if s >= 4096])
def test_kth_and_next_across_a_bin_edge(capi, span):
    """The k-th and the (k+1)-th entry one apart, on the two sides of a bin edge of round 0 and of round 1."""
    rng = np.random.default_rng(span % 99989)
    lo = span_base(span)
    hi = lo + span
    stride = 20001
    sh0 = shift_for(span)
    assert sh0 >= 1
    for k in (2, 37, MAX_K):
        for m in (1, (span >> sh0) // 2, span >> sh0):          # first, a middle and the last edge of round 0
            edge = lo + (m << sh0)
            check(capi, row_across_an_edge(rng, stride, lo, hi, edge, k), k)
        # round 1 counts the round-0 bin [nlo, nlo + 2^sh0 - 1] (cut at hi) again, in bins of 2^sh1
        for m in (0, (span >> sh0) // 2):
            nlo = lo + (m << sh0)
            nhi = min(nlo + (1 << sh0) - 1, hi)
            sh1 = shift_for(nhi - nlo)
            for j in sorted({1, max(1, ((nhi - nlo) >> sh1) // 2), max(1, (nhi - nlo) >> sh1)}):
                edge = nlo + (j << sh1)
                assert nlo < edge <= nhi
                check(capi, row_across_an_edge(rng, stride, lo, hi, edge, k), k)
                if sh1 >= 1:
                    # ... and an edge of round 2 (bins of one score) that is no edge of round 1
                    check(capi, row_across_an_edge(rng, stride, lo, hi, edge + 1, k), k)


# ---- INT_MIN ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_score", [None, INT_MIN])
@pytest.mark.parametrize("top", [INT_MIN, INT_MIN + 50, INT_MIN + 2 ** 20, 0, INT_MAX])
def test_rows_that_hold_int_min(capi, min_score, top):
    """With no bound and INT_MIN in the row, "every entry is chosen" has no threshold below the row's minimum:
    hits <= k (every entry chosen), hits > k, and rows that are INT_MIN throughout (top = INT_MIN)."""
    rng = np.random.default_rng(7 + (top & 0xFFFF))
    for stride in (1, 5, 3000):
        rows = rng.integers(INT_MIN, top + 1, size=(3, stride), dtype=np.int64)
        rows[:, rng.integers(0, stride)] = INT_MIN
        rows[1, : stride // 2] = INT_MIN                      # many entries at INT_MIN
        rows[2] = rng.integers(max(top - 5, INT_MIN + 1), top + 1, size=stride) if top > INT_MIN else INT_MIN   # (none)
        for k in sorted({1, max(1, stride - 1), stride, min(stride + 5, MAX_K), MAX_K}):
            check(capi, rows.astype(np.int32), k, min_score=min_score, ends=True)
    # hits > k at a size of several blocks, INT_MIN among the chosen ties
    big = np.full(20001, INT_MIN, dtype=np.int64)
    big[rng.choice(20001, size=90, replace=False)] = rng.integers(INT_MIN + 1, top + 1, size=90) if top > INT_MIN else INT_MIN
    for k in (1, 90, 91, 200, MAX_K):
        check(capi, big.astype(np.int32), k, min_score=min_score)


# ---- ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [7, INT_MAX, INT_MIN])
def test_all_equal_row(capi, value):
    row = np.full(5 * 16384 + 7, value, dtype=np.int32)
    for k in (1, 3, 4, 5, MAX_K):
        check(capi, row, k, ends=True)


@pytest.mark.parametrize("block", [BLOCK, 16384])
@pytest.mark.parametrize("row", [0, 1, 2, 3])
def test_ties_that_straddle_a_block_boundary(capi, block, row):
    """Exactly the last entry of block b and the first two of block b + 1 equal T, and 1, 2 or 3 of them are taken.
    (Row r of an odd stride starts `phase` entries into a slot, so its blocks start at 4096 b - phase.)"""
    rng = np.random.default_rng(block + row)
    stride = 3 * block + 11
    phase = (row * stride) % 4
    for b in (0, 1):
        edge = (b + 1) * block - phase           # first entry of the next block
        above = 9
        for take in (1, 2, 3):
            rows = rng.integers(0, 100, size=(row + 1, stride)).astype(np.int32)
            v = rows[row]
            v[:] = rng.integers(-50, 100, size=stride)
            v[edge - 1:edge + 2] = 100                       # the three ties at T = 100
            v[rng.choice(np.setdiff1d(np.arange(stride), [edge - 1, edge, edge + 1]), size=above, replace=False)] = \
                rng.integers(101, 200, size=above)
            check(capi, rows, above + take, ends=True, rows_to_check=[row])


def test_many_ties_and_a_few_above(capi):
    rng = np.random.default_rng(70)
    row = rng.integers(-1000, 41, size=80_000).astype(np.int32)
    pos = rng.permutation(80_000)
    row[pos[:70_000]] = 41
    row[pos[70_000:70_010]] = rng.integers(42, 1000, size=10)
    check(capi, row, MAX_K, ends=True)
    check(capi, row, 10)
    check(capi, row, 11)


# ---- dense blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 2])
def test_dense_runs(capi, shift):
    """4096 consecutive entries - one whole aligned block, or two blocks straddled - all above T, then all ties: every
    wavefront's 256 entries of a load counted in one half of the packed prefix."""
    rng = np.random.default_rng(40 + shift)
    stride = 3 * BLOCK + 5
    run = slice(BLOCK + shift, 2 * BLOCK + shift)
    # all chosen and all above T: min_score cuts everything else away ("every entry is chosen": T below the run)
    row = rng.integers(0, 100, size=stride).astype(np.int32)
    row[run] = rng.integers(1000, 2000, size=BLOCK)
    check(capi, row, MAX_K, min_score=1000, ends=True)
    # 4095 of the run above T and its lowest entries at T (no bound)
    check(capi, row, MAX_K, ends=True)
    distinct = row.copy()
    distinct[run] = 1000 + rng.permutation(BLOCK)
    check(capi, distinct, MAX_K, ends=True)
    # a run of ties, everything else below
    ties = rng.integers(0, 100, size=stride).astype(np.int32)
    ties[run] = 500
    check(capi, ties, MAX_K, ends=True)
    check(capi, ties, MAX_K - 1)
    check(capi, ties, 255)
    check(capi, ties, 257)
    # ... and in the second of two rows of an odd stride
    check(capi, np.stack([row, ties]), MAX_K, ends=True)


# ---- more than 64 blocks ----------------------------------------------------------------------------------------------------
def test_more_than_64_blocks(capi):
    """Rows of 66 x 16 384 + 1 entries (265 blocks of 4096): the look-back of the gather continues past the 64
    predecessors of one step. One row random with many ties at the threshold, the other all-equal."""
    rng = np.random.default_rng(66)
    stride = 66 * 16384 + 1
    rows = np.empty((2, stride), dtype=np.int32)
    rows[0] = rng.integers(0, 30, size=stride)                 # ~36 000 entries at each value
    rows[0, rng.choice(stride, size=1000, replace=False)] = rng.integers(30, 5000, size=1000)
    rows[1] = 12
    for k in (1, MAX_K):
        check(capi, rows, k, ends=True)
    # the chosen entries in the last blocks only: their offsets come from the look-back over all the blocks before
    tail = np.zeros(stride, dtype=np.int32)
    tail[-3000:] = rng.integers(0, 3, size=3000)
    tail[:5] = 2
    check(capi, tail, MAX_K)
    check(capi, tail, 2000, min_score=1)


# ---- more than one group of rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1024, 1025, 2049])
def test_more_than_one_group_of_rows(capi, rows):
    """launchSelectTop takes 1024 rows per sequence of launches: the later groups read their own rows and write their
    own outputs. Every row has a range of its own, so an answer taken from row r - 1024 differs."""
    rng = np.random.default_rng(rows)
    stride = 37
    base = rng.integers(-10 ** 6, 10 ** 6, size=(rows, 1))
    width = rng.integers(1, 1000, size=(rows, 1))
    score = (base + rng.integers(0, 2 ** 31, size=(rows, stride)) % width).astype(np.int32)
    for k in (10, 40):
        got = check(capi, score, k, ends=True)
        end_q, end_t = end_arrays(rows, stride)
        for r in (1023, 1024, 2047, 2048):
            if r < rows:
                order = reference(score[r], k)
                c = len(order)
                assert got["count"][r] == c == min(k, stride)
                assert got["target"][r, :c].tolist() == order.tolist()
                assert got["score"][r, :c].tolist() == score[r, order].tolist()
                assert got["end_q"][r, :c].tolist() == end_q[r, order].tolist()
                assert got["end_t"][r, :c].tolist() == end_t[r, order].tolist()
                if r >= 1024:
                    assert got["score"][r].tolist() != got["score"][r - 1024].tolist()
    ms = int(np.median(score))
    check(capi, score, 10, min_score=ms, ends=True)            # rows without a hit among rows with hits


# ---- min_score ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [50, 2 ** 24 + 1000, 2 ** 32 - 1])
def test_min_score(capi, span):
    """Below the minimum, equal to the k-th score, equal to the maximum and above it (count 0, every slot -1)."""
    rng = np.random.default_rng(span % 9973)
    lo = INT_MIN if span == 2 ** 32 - 1 else -span // 2
    rows = np.stack([spread(rng, 5000, lo, lo + span) for _ in range(3)]).astype(np.int32)
    s = np.sort(rows[0].astype(np.int64))[::-1]
    for k in (1, 100, MAX_K):
        bounds = {int(s[-1]), int(s[k - 1]), int(s[k - 1]) + 1, int(s[0])}
        if s[-1] > INT_MIN:
            bounds.add(int(s[-1]) - 1)
        if s[0] < INT_MAX:
            bounds.add(int(s[0]) + 1)
        for ms in sorted(b for b in bounds if b <= INT_MAX):
            got = check(capi, rows, k, min_score=ms, ends=True)
            assert got["count"][0] == min(k, int(np.count_nonzero(rows[0] >= ms)))
            if ms > s[0]:
                assert got["count"].tolist() == [0, 0, 0] and np.all(got["target"] == -1) and np.all(got["end_t"] == -1)


# ---- start ----------------------------------------------------------------------------------------------------------------------
def test_start_above_32_bits(capi):
    rng = np.random.default_rng(33)
    score = rng.integers(0, 51, size=(3, 5001)).astype(np.int32)
    for k in (1, 77, MAX_K):
        got = check(capi, score, k, ends=True, start=2 ** 33 + 5)
        assert got["target"].dtype == np.int64 and got["target"][0, 0] >= 2 ** 33 + 5


# ---- a fixed-seed sweep -----------------------------------------------------------------------------------------------------------
def sweep_case(rng):
    rows = int(rng.integers(1, 9))
    pick = rng.integers(0, 3)
    if pick == 0:
        stride = int(rng.integers(1, 65))
    elif pick == 1:
        stride = int(BLOCK * rng.integers(1, 10) + rng.integers(-3, 4))
    else:
        stride = int(rng.integers(1, 40001))
    family = int(rng.integers(0, 4))
    shape = (rows, stride)
    if family == 0:      # uniform, narrow
        lo = int(rng.integers(-10 ** 6, 10 ** 6))
        score = rng.integers(lo, lo + int(rng.integers(1, 300)), size=shape)
    elif family == 1:    # uniform over the whole of int32
        score = wide(rng, shape)
    elif family == 2:    # geometric: a few large values over many small ones, either sign
        score = rng.geometric(10.0 ** -rng.uniform(1, 8), size=shape).clip(0, INT_MAX) * (1 if rng.integers(0, 2) else -1)
    else:                # a handful of distinct values
        score = rng.choice(wide(rng, int(rng.integers(1, 8))), size=shape)
    score = np.asarray(score, dtype=np.int64).astype(np.int32)
    k = int(rng.choice([1, 2, int(rng.integers(1, MAX_K + 1)), int(rng.integers(1, 65)), MAX_K, min(stride, MAX_K)]))
    min_score = None if rng.integers(0, 2) else int(score[rng.integers(0, rows), rng.integers(0, stride)])
    return score, k, min_score, bool(rng.integers(0, 2))


@pytest.mark.parametrize("part", range(4))
def test_sweep(capi, part):
    rng = np.random.default_rng(20240 + part)
    for _ in range(50):
        score, k, min_score, ends = sweep_case(rng)
        check(capi, score, k, min_score=min_score, ends=ends)
