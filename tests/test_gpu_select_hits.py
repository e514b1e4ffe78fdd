"""The device compaction of the hit searches alone (select_hits.hip through the test hook miopalTestSelectHits,
_capi.select_hits_rows): rows of int32 values made for every arm of the three kernels - rows that start at every
misalignment of a 16-byte slot, strides around one block of 4096, a second group of 1024 rows, full and empty blocks
and wavefronts, the extreme values and thresholds, thresholds per row, end rows read at the hit positions only, indices
above 2^32 - checked exactly against numpy.nonzero(row >= threshold)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
POISON = -123456789   # in the end rows wherever there is no hit: must never come back


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def check(capi, score, thresholds, ends=True, start=0):
    """select_hits_rows of `score` against numpy, row by row; with `ends`, end rows that hold 2 i + 1 / -(i + 2) at the
    hit positions i (flat index) and POISON everywhere else"""
    score = np.ascontiguousarray(score, dtype=np.int32)
    if score.ndim == 1:
        score = score[None, :]
    rows, stride = score.shape
    t = np.broadcast_to(np.asarray(thresholds, dtype=np.int64), (rows,))
    hit = score >= t[:, None]
    end_q = end_t = None
    if ends:
        flat = np.arange(rows * stride, dtype=np.int64).reshape(rows, stride)
        end_q = np.where(hit, (2 * flat + 1) % 1_000_003, POISON).astype(np.int32)
        end_t = np.where(hit, -(flat % 1_000_033) - 2, POISON).astype(np.int32)
    got = capi.select_hits_rows(score, np.asarray(thresholds, dtype=np.int32), end_q, end_t, start)
    counts = hit.sum(axis=1)
    want_offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], want_offsets)
    r, i = np.nonzero(hit)   # (row-major: row after row, index ascending)
    assert got["target"].dtype == np.int64 and np.array_equal(got["target"], start + i.astype(np.int64))
    assert got["score"].dtype == np.int32 and np.array_equal(got["score"], score[r, i])
    if ends:
        assert np.array_equal(got["end_q"], end_q[r, i]) and np.array_equal(got["end_t"], end_t[r, i])
        assert not np.any(got["end_q"] == POISON) and not np.any(got["end_t"] == POISON)
    else:
        assert "end_q" not in got and "end_t" not in got
    return got


@pytest.mark.parametrize("rows", [1, 3, 7])
@pytest.mark.parametrize("stride", [1, 3, 5, 4095, 4096, 4097, 8193])
def test_strides_and_rows_around_one_block(capi, stride, rows):
    # (odd strides: rows >= 1 start at every misalignment of a 16-byte slot; 4096: every row aligned, a second block
    # that holds the row's last slot only; 4095 / 4097 / 8193: last slots of 3, 1 and 1 entries)
    rng = np.random.default_rng(1000 * stride + rows)
    score = rng.integers(-50, 50, size=(rows, stride), dtype=np.int32)
    for threshold in (0, 45, -50):
        check(capi, score, threshold, ends=True)
    check(capi, score, 10, ends=False)
    check(capi, score, rng.integers(-50, 50, size=rows), ends=True)


def test_more_than_one_launch_group(capi):
    rng = np.random.default_rng(1025)
    score = rng.integers(0, 100, size=(1025, 37), dtype=np.int32)
    thresholds = rng.integers(0, 100, size=1025)
    thresholds[[0, 1023, 1024]] = (50, 0, 97)
    got = check(capi, score, thresholds)
    assert got["offsets"][1024] < got["offsets"][1025]   # the second group's row holds hits behind the first group's
    check(capi, score, 0, ends=False)                    # every entry of every row: 37 925 hits
    check(capi, score, 100)                              # none in either group


def raw_call(capi, score, thresholds):
    """the hook itself: return code, offsets and the four pointers as the C side left them"""
    score = np.ascontiguousarray(score, dtype=np.int32)
    rows, stride = score.shape
    t = np.ascontiguousarray(thresholds, dtype=np.int32)
    offsets = np.full(rows + 1, -7, dtype=np.int64)
    ptrs = [ctypes.c_void_p(0x55) for _ in range(4)]
    rc = capi.lib().miopalTestSelectHits(score.ctypes.data, None, None, rows, stride, t.ctypes.data, 0, offsets.ctypes.data,
                                         *[ctypes.byref(p) for p in ptrs])
    return rc, offsets, ptrs


def test_hit_patterns(capi):
    rows, stride = 3, 4096 * 2 + 5
    base = np.zeros((rows, stride), dtype=np.int32)
    # every entry a hit
    got = check(capi, base, 0)
    assert got["offsets"][-1] == rows * stride
    # no entry a hit: total 0 and NULL arrays (the two end pointers are NULL without end rows as well)
    rc, offsets, ptrs = raw_call(capi, base, np.ones(rows, dtype=np.int32))
    assert rc == 0 and np.all(offsets == 0) and all(p.value is None for p in ptrs)
    got = check(capi, base, 1)
    assert len(got["target"]) == 0 and len(got["score"]) == 0 and len(got["end_q"]) == 0
    # the only hit in the last entry of the last block of the last row
    last = base.copy()
    last[-1, -1] = 9
    got = check(capi, last, 9)
    assert got["target"].tolist() == [stride - 1] and got["offsets"].tolist() == [0, 0, 0, 1]
    # the only hit in entry 0
    first = base.copy()
    first[0, 0] = 9
    got = check(capi, first, 9)
    assert got["target"].tolist() == [0] and got["offsets"].tolist() == [0, 1, 1, 1]
    # ... and both, with a hit on either side of every row boundary
    edges = base.copy()
    edges[:, 0] = 9
    edges[:, -1] = 9
    assert check(capi, edges, 9)["target"].tolist() == [0, stride - 1] * rows


@pytest.mark.parametrize("stride", [3 * 4096, 3 * 4096 + 1, 3 * 4096 + 3])
def test_full_and_empty_blocks_and_wavefronts(capi, stride):
    # (row 1 starts 0, 1 or 3 entries into a slot: its blocks are shifted against the pattern by as much)
    score = np.zeros((2, stride), dtype=np.int32)
    score[:, :4096] = 5                  # a block with all 4096 entries hits next to a block with none
    score[:, 2 * 4096 + 1536:2 * 4096 + 1792] = 5   # round 1, wavefront 2 of the third block: all 256 entries hits
    got = check(capi, score, 5)
    assert got["offsets"].tolist() == [0, 4352, 8704]
    # the complement: the empty block in front, 256 misses inside the third
    check(capi, 5 - score, 5)


def test_extreme_values_and_thresholds(capi):
    rng = np.random.default_rng(31)
    values = np.array([INT_MIN, INT_MIN, INT_MAX, INT_MIN + 1, -1, 0, INT_MAX - 1], dtype=np.int64)
    score = values[rng.integers(0, len(values), size=(3, 4099))].astype(np.int32)
    for threshold, hits in ((INT_MIN, score.size), (INT_MIN + 1, int(np.count_nonzero(score > INT_MIN))),
                            (INT_MAX, int(np.count_nonzero(score == INT_MAX)))):
        got = check(capi, score, threshold)
        assert got["offsets"][-1] == hits and 0 < hits
    check(capi, score, [INT_MIN, INT_MIN + 1, INT_MAX])
    # rows of one extreme value each
    for value in (INT_MIN, INT_MAX):
        row = np.full((2, 4097), value, dtype=np.int32)
        for threshold in (INT_MIN, INT_MIN + 1, INT_MAX):
            got = check(capi, row, threshold)
            assert got["offsets"][-1] == (row.size if value >= threshold else 0)


def test_thresholds_per_row(capi):
    rng = np.random.default_rng(77)
    score = rng.integers(-1000, 1000, size=(7, 5000), dtype=np.int32)
    thresholds = [-1000, 1000, 0, 999, -999, 500, INT_MIN]   # all, none, half, a few, nearly all, a quarter, all
    got = check(capi, score, thresholds)
    counts = np.diff(got["offsets"])
    assert counts[0] == 5000 and counts[1] == 0 and counts[6] == 5000 and 0 < counts[3] < 20
    check(capi, score, thresholds[::-1], ends=False)


def test_start_above_two_to_the_32(capi):
    rng = np.random.default_rng(5)
    score = rng.integers(0, 10, size=(2, 4100), dtype=np.int32)
    start = 2 ** 32 + 12345
    got = check(capi, score, 7, start=start)
    assert got["target"].min() >= start and got["target"].max() < start + 4100
    check(capi, score, 7, ends=False, start=2 ** 40)
