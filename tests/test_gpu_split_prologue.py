"""The prologue of the column-split form of the one-strip Smith-Waterman kernel (interseq_impl.h,
interseq_pair_biased_kernel<R, false, true>) and what the host no longer does per launch for it:

* the pair table is built from a copy of the profile in LDS, wavefront by pair row and lane by query row - every row
  count 1 .. 64, the padding symbol, and an alphabet smaller than a workgroup's twelve wavefronts;
* the flags of the cuts carry the launch's epoch and are not zeroed per launch - one handle, many launches of
  different plans over the same flag slots, and the counter's wrap;
* on the fast path the kernel reads the profile from the host's staging buffer - two searches in flight on one stream,
  and 800 of them, which fill the staging buffer twice while kernels still read from it.

Small databases, the split forced with MIOPAL_COLUMN_SPLIT; every score against the CPU checker."""
import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
DNA = np.where(np.eye(4, dtype=bool), 5, -4).astype(np.int32).ravel()
PAIR_BIASED = 4   # miopalLastRouting counts[1]: 2 + kPairSwBiased
SPLIT = 64        # ... + 64: the column split


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def routed(capi):
    return capi.DeviceDatabase.last_routing()[1]


def test_every_row_count(capi, tuning):
    # 512 targets of 24 - 40 residues: 4 groups of 6 - 10 chunks on 24 wavefronts, cuts inside every group. R < 4, R
    # not a multiple of 4, odd and even R; the targets' padding columns read the padding symbol's table rows.
    rng = np.random.default_rng(6400)
    res, off = _data.random_db(rng, rng.integers(24, 41, size=512))
    whole = _data.random_protein(rng, 64)
    res = res.copy()
    for k in range(0, 512, 37):                       # (some high scores: pieces of the query)
        res[off[k]:off[k] + 20] = whole[k % 40:k % 40 + 20]
    tuning.setenv("MIOPAL_COLUMN_SPLIT", "2")
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for qlen in range(1, 65):
            query = whole[:qlen]
            want = _oracle.search(query, res, off, B62, 3, 1, "score", "sw")["score"]
            got = db.search(query, B62, 3, 1, "score", "sw")["score"]
            # (the table of 61 - 64 rows does not fit the CU's LDS with 25 symbols: those take the general kernel)
            if qlen <= 60:
                assert routed(capi) == PAIR_BIASED + SPLIT, (qlen, routed(capi))
            np.testing.assert_array_equal(got, want, err_msg=f"Q={qlen}")
    finally:
        db.close()


def test_every_row_count_of_a_small_alphabet(capi, tuning):
    # nSym = 5, fewer symbols than wavefronts: a wavefront's next pair row is more than one tA further on; every row
    # count has its table here, 61 - 64 too
    rng = np.random.default_rng(5)
    lengths = rng.integers(24, 41, size=512)
    off = np.zeros(513, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    res = rng.integers(0, 4, size=int(off[-1])).astype(np.uint8)
    whole = rng.integers(0, 4, size=64).astype(np.uint8)
    tuning.setenv("MIOPAL_COLUMN_SPLIT", "2")
    db = capi.DeviceDatabase(res, off, 4)
    try:
        for qlen in range(1, 65):
            query = whole[:qlen]
            want = _oracle.search(query, res, off, DNA, 3, 1, "score", "sw")["score"]
            got = db.search(query, DNA, 3, 1, "score", "sw")["score"]
            assert routed(capi) == PAIR_BIASED + SPLIT, (qlen, routed(capi))
            np.testing.assert_array_equal(got, want, err_msg=f"Q={qlen}")
    finally:
        db.close()


@pytest.fixture(scope="module")
def two_slices():
    """One database searched whole (40 groups) and up to a third of it (14 groups): two views, two plans."""
    rng = np.random.default_rng(40)
    query = _oracle.encode(_data.README_QUERY)
    n = 5120
    res, off = _data.random_db(rng, rng.integers(200, 301, size=n))
    res = res.copy()
    for k in range(0, n, 61):
        t = _data.mutate(rng, query, 0.1)[:150]
        res[off[k] + 20:off[k] + 20 + len(t)] = t
    want = _oracle.search(query, res, off, B62, 3, 1, "score", "sw")["score"]
    return query, res, off, want, (n, 1700)


@pytest.mark.parametrize("recompute", [False, True])
def test_epochs_over_many_plans(capi, tuning, two_slices, recompute):
    # 40 launches of one workspace: the flag slots hold the epochs of other plans (more or fewer wavefronts, cuts
    # elsewhere) when a launch starts, and none of them is the launch's own
    query, res, off, want, ends = two_slices
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for k in range(40):
            end = ends[k % 2]
            blocks = (1, 2, 5)[k % 3]
            tuning.setenv("MIOPAL_COLUMN_SPLIT", "recompute" if recompute and k % 4 == 3 else str(blocks))
            got = db.search(query, B62, 3, 1, "score", "sw", 0, end)["score"]
            assert routed(capi) == PAIR_BIASED + SPLIT, (k, routed(capi))
            np.testing.assert_array_equal(got, want[:end], err_msg=f"launch {k}: {blocks} workgroups, {end} targets")
    finally:
        db.close()


def test_epoch_wraps(capi, tuning, two_slices):
    # the counter set to 2^32 - 2 (test hook), then four launches across the wrap: 2^32 - 1, flags zeroed and 1, 2, 3
    query, res, off, want, ends = two_slices
    db = capi.DeviceDatabase(res, off, 24)
    try:
        tuning.setenv("MIOPAL_COLUMN_SPLIT", "5")
        for k in range(3):                                 # (small epochs in the slots first)
            np.testing.assert_array_equal(db.search(query, B62, 3, 1, "score", "sw")["score"], want)
        tuning.setenv("MIOPAL_TEST_SPLIT_EPOCH", str(2 ** 32 - 2))
        np.testing.assert_array_equal(db.search(query, B62, 3, 1, "score", "sw")["score"], want, err_msg="epoch 2^32 - 2")
        tuning.delenv("MIOPAL_TEST_SPLIT_EPOCH")
        for k in range(4):
            end = ends[k % 2]
            got = db.search(query, B62, 3, 1, "score", "sw", 0, end)["score"]
            assert routed(capi) == PAIR_BIASED + SPLIT, (k, routed(capi))
            np.testing.assert_array_equal(got, want[:end], err_msg=f"launch {k} after 2^32 - 2")
    finally:
        db.close()


def test_two_searches_in_flight_read_their_own_profiles(capi, tuning, two_slices):
    # the asynchronous entry: two queries on one stream into two device buffers with nothing waited for in between -
    # the second call stages its profile while the first kernel may not have read its own yet
    import torch
    query, res, off, want, _ = two_slices
    other = _data.random_protein(np.random.default_rng(41), 37)
    res = res.copy()
    res[off[7]:off[7] + 37] = other
    want_a = _oracle.search(query, res, off, B62, 3, 1, "score", "sw")["score"]
    want_b = _oracle.search(other, res, off, B62, 3, 1, "score", "sw")["score"]
    n = len(off) - 1
    tuning.setenv("MIOPAL_COLUMN_SPLIT", "5")
    db = capi.DeviceDatabase(res, off, 24)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        out_a = torch.empty(n, dtype=torch.int32, device="cuda:0")
        out_b = torch.empty(n, dtype=torch.int32, device="cuda:0")
        for rep in range(20):
            out_a.fill_(-7)
            out_b.fill_(-7)
            db.search_device_scores(query, B62, out_a.data_ptr(), stream, 3, 1, "sw")
            assert routed(capi) == PAIR_BIASED + SPLIT, routed(capi)
            db.search_device_scores(other, B62, out_b.data_ptr(), stream, 3, 1, "sw")
            assert routed(capi) == PAIR_BIASED + SPLIT, routed(capi)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out_a.cpu().numpy(), want_a, err_msg=f"first query, repetition {rep}")
            np.testing.assert_array_equal(out_b.cpu().numpy(), want_b, err_msg=f"second query, repetition {rep}")
    finally:
        db.close()


def test_staging_buffer_drains_under_searches_in_flight(capi, tuning, two_slices):
    # 800 asynchronous searches of alternating queries on one stream, every one into a row of its own, nothing waited
    # for: at 3 KB of profile a call the workspace's staging buffer (1 MB and a little) fills twice, with kernels
    # still in flight that read their profiles from it - the call that finds it full waits for the stream before the
    # buffer starts over, so every row is its own query's scores
    import torch
    query, res, off, want_a, _ = two_slices
    other = _data.random_protein(np.random.default_rng(43), 53)
    want_b = _oracle.search(other, res, off, B62, 3, 1, "score", "sw")["score"]
    n = len(off) - 1
    calls = 800
    tuning.setenv("MIOPAL_COLUMN_SPLIT", "8")
    db = capi.DeviceDatabase(res, off, 24)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        out = torch.full((calls, n), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for k in range(calls):
            db.search_device_scores(other if k % 2 else query, B62, out[k].data_ptr(), stream, 3, 1, "sw")
        assert routed(capi) == PAIR_BIASED + SPLIT, routed(capi)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = [k for k in range(calls) if not np.array_equal(got[k], want_b if k % 2 else want_a)]
        assert not bad, f"{len(bad)} of {calls} searches read another profile, first {bad[:5]}"
    finally:
        db.close()
