"""The statistics and binned-compaction kernels of the significance searches alone (select_stats.hip through the test
hooks miopalTestRowStats and miopalTestSelectHitsBinned; _capi.row_stats_rows / select_hits_binned_rows): rows of int32
values and columns of lengths made for every arm of the kernels - rows that start at every misalignment of a 16-byte
slot, strides around one wavefront and one block of 4096, a second group of 1024 rows, whole wavefronts inside one
length bin, two bins alternating lane by lane, every bin edge, ceilings, skipped rows, sums that wrap - checked exactly
against numpy: np.add.at on int64 for the sums, fancy indexing for the thresholds. Bins in this file come from
int.bit_length, never from a floating logarithm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
BINS = 128
POISON = -123456789   # in the end rows wherever there is no hit: must never come back
STRIDES = [1, 3, 5, 63, 64, 65, 257, 4095, 4096, 4097, 8193]


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def bin_of(length):
    """the definition of include/miopal.h, in Python integers"""
    L = int(length)
    if L == 0:
        return 0
    e = L.bit_length() - 1
    m = (L >> (e - 2)) & 3 if e >= 2 else (L << (2 - e)) & 3
    return 1 + 4 * e + m


def bins_of(lengths):
    return np.array([bin_of(L) for L in lengths], dtype=np.int64)


def edge_lengths():
    """every bin edge up to 2^31 - 1: 2^e - 1, 2^e, 2^e + k 2^(e-2) - 1 / + 0 / + 1"""
    out = [0]
    for e in range(31):
        out += [2 ** e - 1, 2 ** e, 2 ** e + 1]
        if e >= 2:
            for k in (1, 2, 3):
                q = 2 ** e + k * 2 ** (e - 2)
                out += [q - 1, q, q + 1]
    out += [INT_MAX - 1, INT_MAX]
    return np.array([L for L in out if 0 <= L <= INT_MAX], dtype=np.int32)


EDGES = edge_lengths()


def lengths_of(pattern, stride):
    i = np.arange(stride, dtype=np.int64)
    if pattern == "one bin":        # whole wavefronts (the whole block) inside one bin
        return np.full(stride, 300, dtype=np.int32)
    if pattern == "two bins":       # alternating lane by lane, and entry by entry inside a slot
        return np.where(i % 2 == 0, 300, 41).astype(np.int32)
    if pattern == "index":          # length[i] = i: 0 among them, neighbours in the same and in different bins
        return i.astype(np.int32)
    if pattern == "edges":
        return EDGES[i % len(EDGES)]
    raise AssertionError(pattern)


PATTERNS = ("one bin", "two bins", "index", "edges")


def want_stats(score, bins, ceiling=None, skip=None):
    rows = score.shape[0]
    out = np.zeros((rows, BINS, 3), dtype=np.int64)
    for r in range(rows):
        if skip is not None and skip[r]:
            continue
        s = score[r].astype(np.int64)
        keep = np.ones(len(s), dtype=bool) if ceiling is None else s <= np.broadcast_to(ceiling, (rows, BINS))[r][bins]
        with np.errstate(over="ignore"):
            np.add.at(out[r, :, 0], bins[keep], 1)
            np.add.at(out[r, :, 1], bins[keep], s[keep])
            np.add.at(out[r, :, 2], bins[keep], s[keep] * s[keep])   # (int64: wraps like the device's sums)
    return out


def check_stats(capi, score, length, ceiling=None, skip=None):
    score = np.ascontiguousarray(score, dtype=np.int32)
    bins = bins_of(length)
    got = capi.row_stats_rows(score, length, ceiling, skip)
    assert got["bin"].dtype == np.uint8 and np.array_equal(got["bin"], bins)
    want = want_stats(score, bins, ceiling, skip)
    assert got["stats"].dtype == np.int64 and got["stats"].shape == want.shape
    assert np.array_equal(got["stats"], want), np.argwhere(got["stats"] != want)[:5]
    return got["stats"]


def test_bins_equal_the_integer_definition(capi):
    got = capi.row_stats_rows(np.zeros((1, len(EDGES)), dtype=np.int32), EDGES)
    assert np.array_equal(got["bin"], bins_of(EDGES))
    assert got["bin"].max() == 124 and bin_of(INT_MAX) == 124 and bin_of(1) == 1 and bin_of(2) == 5 and bin_of(3) == 7
    # quarter octaves: 2^e + k 2^(e-2) opens a bin, the length before it closes the one below
    for e in range(2, 31):
        for k in range(4):
            q = 2 ** e + k * 2 ** (e - 2)
            assert bin_of(q) == 1 + 4 * e + k
            # (below 4 a length has fewer than two bits under its leading one: 3 sits in bin 7, bin 8 stays empty)
            assert bin_of(q - 1) == (4 * e + k if q > 4 else 7)
    assert np.array_equal(capi.length_bins(EDGES), bins_of(EDGES))   # (the Python layer's copy)
    # n counts every column once, whatever its bin
    assert got["stats"][0, :, 0].sum() == len(EDGES) and np.all(got["stats"][0, :, 1:] == 0)


@pytest.mark.parametrize("rows", [1, 3, 7])
@pytest.mark.parametrize("stride", STRIDES)
def test_stats_strides_rows_patterns_ceilings(capi, stride, rows):
    rng = np.random.default_rng(1000 * stride + rows)
    score = rng.integers(-50, 51, size=(rows, stride), dtype=np.int32)
    per_row = rng.integers(-50, 51, size=(rows, BINS)).astype(np.int32)
    for pattern in PATTERNS:
        length = lengths_of(pattern, stride)
        all_of_them = check_stats(capi, score, length)
        assert all_of_them[:, :, 0].sum() == rows * stride
        kept = check_stats(capi, score, length, per_row)
        assert kept[:, :, 0].sum() <= rows * stride
        assert np.array_equal(check_stats(capi, score, length, np.full(BINS, INT_MAX, dtype=np.int32)), all_of_them)
        assert not check_stats(capi, score, length, np.full(BINS, INT_MIN, dtype=np.int32)).any()


def test_stats_more_than_one_launch_group(capi):
    rng = np.random.default_rng(1025)
    score = rng.integers(-50, 51, size=(1025, 5), dtype=np.int32)
    length = np.array([300, 41, 0, 300, 7], dtype=np.int32)
    stats = check_stats(capi, score, length)
    assert stats[1024, :, 0].sum() == 5
    check_stats(capi, score, length, rng.integers(-50, 51, size=(1025, BINS)).astype(np.int32))


def test_stats_skipped_rows_are_not_read(capi):
    rng = np.random.default_rng(9)
    rows, stride = 7, 4097
    score = rng.integers(-50, 51, size=(rows, stride), dtype=np.int32)
    skip = np.array([0, 1, 0, 0, 1, 1, 0])
    score[skip != 0] = 1_000_003   # would change every sum
    for pattern in PATTERNS:
        stats = check_stats(capi, score, lengths_of(pattern, stride), None, skip)
        assert not stats[skip != 0].any() and stats[skip == 0, :, 0].sum() == 4 * stride
    check_stats(capi, score, lengths_of("index", stride), rng.integers(-50, 51, size=(rows, BINS)).astype(np.int32), skip)
    assert not check_stats(capi, score, lengths_of("one bin", stride), None, np.ones(rows, dtype=np.int32)).any()


def test_stats_extreme_values_wrap_like_int64(capi):
    rng = np.random.default_rng(31)
    values = np.array([INT_MIN, INT_MIN, INT_MAX, INT_MIN + 1, -1, 0, INT_MAX - 1], dtype=np.int64)
    score = values[rng.integers(0, len(values), size=(3, 8193))].astype(np.int32)
    for pattern in ("one bin", "two bins", "index"):
        check_stats(capi, score, lengths_of(pattern, 8193))
        check_stats(capi, score, lengths_of(pattern, 8193), np.full(BINS, INT_MAX - 1, dtype=np.int32))
    # a row of INT_MIN alone: 8192 squares of 2^62 sum to 0 modulo 2^64
    row = np.full((1, 8192), INT_MIN, dtype=np.int32)
    stats = check_stats(capi, row, lengths_of("one bin", 8192))
    b = bin_of(300)
    assert stats[0, b].tolist() == [8192, 8192 * INT_MIN, 0]
    row = np.full((1, 8193), INT_MAX, dtype=np.int32)
    stats = check_stats(capi, row, lengths_of("one bin", 8193), np.full(BINS, INT_MIN, dtype=np.int32))
    assert not stats.any()
    stats = check_stats(capi, row, lengths_of("one bin", 8193))
    assert stats[0, b, 2] != 8193 * INT_MAX * INT_MAX   # (the exact sum does not fit: it wrapped)


# ---- the compaction with a threshold per bin -----------------------------------------------------------------------
def check_binned(capi, score, length, table, ends=True, start=0):
    score = np.ascontiguousarray(score, dtype=np.int32)
    rows, stride = score.shape
    bins = bins_of(length)
    table = np.ascontiguousarray(np.broadcast_to(np.asarray(table, dtype=np.int32), (rows, BINS)))
    hit = score >= table[:, bins]
    end_q = end_t = None
    if ends:
        flat = np.arange(rows * stride, dtype=np.int64).reshape(rows, stride)
        end_q = np.where(hit, (2 * flat + 1) % 1_000_003, POISON).astype(np.int32)
        end_t = np.where(hit, -(flat % 1_000_033) - 2, POISON).astype(np.int32)
    got = capi.select_hits_binned_rows(score, length, table, end_q, end_t, start)
    want_offsets = np.concatenate(([0], np.cumsum(hit.sum(axis=1)))).astype(np.int64)
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], want_offsets)
    r, i = np.nonzero(hit)
    assert got["target"].dtype == np.int64 and np.array_equal(got["target"], start + i.astype(np.int64))
    assert got["score"].dtype == np.int32 and np.array_equal(got["score"], score[r, i])
    if ends:
        assert np.array_equal(got["end_q"], end_q[r, i]) and np.array_equal(got["end_t"], end_t[r, i])
        assert not np.any(got["end_q"] == POISON) and not np.any(got["end_t"] == POISON)
    else:
        assert "end_q" not in got and "end_t" not in got
    return got


@pytest.mark.parametrize("rows", [1, 3, 7])
@pytest.mark.parametrize("stride", STRIDES)
def test_binned_strides_rows_patterns(capi, stride, rows):
    rng = np.random.default_rng(2000 * stride + rows)
    score = rng.integers(-50, 51, size=(rows, stride), dtype=np.int32)
    per_row = rng.integers(-50, 51, size=(rows, BINS)).astype(np.int32)
    for pattern in PATTERNS:
        length = lengths_of(pattern, stride)
        check_binned(capi, score, length, per_row)
        check_binned(capi, score, length, per_row[0], ends=False)
        # INT_MIN / INT_MAX bin by bin: every entry of the even bins, none of the odd ones
        extreme = np.where(np.arange(BINS) % 2 == 0, INT_MIN, INT_MAX).astype(np.int32)
        got = check_binned(capi, score, length, extreme)
        assert got["offsets"][-1] == rows * int(np.count_nonzero(bins_of(length) % 2 == 0))


def test_binned_more_than_one_launch_group(capi):
    rng = np.random.default_rng(1026)
    score = rng.integers(-50, 51, size=(1025, 5), dtype=np.int32)
    length = np.array([300, 41, 0, 300, 7], dtype=np.int32)
    table = rng.integers(-50, 51, size=(1025, BINS)).astype(np.int32)
    table[1024] = -50
    got = check_binned(capi, score, length, table)
    assert got["offsets"][1025] - got["offsets"][1024] == 5
    assert check_binned(capi, score, length, np.full(BINS, INT_MAX, dtype=np.int32))["offsets"][-1] == 0


def test_binned_only_one_bin_hits(capi):
    rng = np.random.default_rng(12)
    stride = 8193
    score = rng.integers(-50, 51, size=(3, stride), dtype=np.int32)
    length = lengths_of("index", stride)
    table = np.full(BINS, INT_MAX, dtype=np.int32)
    table[bin_of(4096)] = INT_MIN   # lengths 4096 .. 5119
    got = check_binned(capi, score, length, table)
    assert got["offsets"].tolist() == [0, 1024, 2048, 3072] and got["target"][:2].tolist() == [4096, 4097]
    table[:] = INT_MAX
    table[0] = -50                  # the only target of length 0
    assert check_binned(capi, score, length, table)["target"].tolist() == [0, 0, 0]


def test_binned_extreme_values(capi):
    rng = np.random.default_rng(32)
    values = np.array([INT_MIN, INT_MAX, INT_MIN + 1, -1, 0, INT_MAX - 1], dtype=np.int64)
    score = values[rng.integers(0, len(values), size=(3, 4099))].astype(np.int32)
    length = lengths_of("two bins", 4099)
    for low, high in ((INT_MIN, INT_MAX), (INT_MIN + 1, INT_MAX - 1), (INT_MAX, INT_MIN)):
        table = np.full(BINS, INT_MAX, dtype=np.int32)
        table[bin_of(300)], table[bin_of(41)] = low, high
        check_binned(capi, score, length, table)


def test_binned_start_above_two_to_the_32(capi):
    rng = np.random.default_rng(5)
    score = rng.integers(-50, 51, size=(2, 4100), dtype=np.int32)
    start = 2 ** 32 + 12345
    got = check_binned(capi, score, lengths_of("edges", 4100), rng.integers(-50, 51, size=(2, BINS)), start=start)
    assert got["target"].min() >= start and got["target"].max() < start + 4100
    check_binned(capi, score, lengths_of("index", 4100), np.full(BINS, 10), ends=False, start=2 ** 40)
