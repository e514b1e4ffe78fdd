"""The column split of the one-strip Smith-Waterman kernel (interseq_impl.h, interseq_pair_biased_kernel<R, false, true>):
every resident wavefront sweeps an equal interval of the launch's chunks, and a group cut by an interval's end is
begun by one wavefront and finished by the next from the state the first one left. Small databases, the mode forced
on 1, 2, 3, 5 and 8 workgroups (MIOPAL_COLUMN_SPLIT): with 40 - 80 groups of 60 - 76 chunks the cuts fall on first
chunks, last chunks and the middle of groups, and at 5 and 8 workgroups an interval is shorter than a group, so that
groups are handed on more than once. Every score against the CPU checker and against the same search with the split
off; miopalLastRouting counts[1] carries bit 64 when the split kernel ran."""
import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
PAIR_BIASED = 4   # miopalLastRouting counts[1]: 2 + kPairSwBiased
SPLIT = 64        # ... + 64: the column split
WORKGROUPS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def database(rng, query, lengths):
    """Random targets of these lengths, every 61st a noisy copy of the query (high scores, wherever the cuts fall)."""
    res, off = _data.random_db(rng, lengths)
    res = res.copy()
    for k in range(0, len(lengths), 61):
        t = _data.mutate(rng, query, 0.1)[:lengths[k]]
        at = off[k] + (lengths[k] - len(t)) // 2
        res[at:at + len(t)] = t
    return res, off


def routed(capi):
    return capi.DeviceDatabase.last_routing()


def check(capi, query, res, off, matrix=B62, gap_open=3, gap_extend=1, settings=tuple(str(w) for w in WORKGROUPS),
          option=None, tag="", alphabet=24, workgroups=None):
    """The search with the split off and under every setting of MIOPAL_COLUMN_SPLIT: the checker's scores each time,
    the same number of lanes redone for their range, and the split kernel where it was asked for. The launch shape
    (miopalLastLaunchShape) each time: a workgroup per compute unit the launch may use or per group with the split off,
    the forced number - at most the units - with it. `workgroups`: all other units are reserved, and the launch with
    the split off has a dynamic round."""
    want = _oracle.search(query, res, off, matrix, gap_open, gap_extend, "score", "sw")["score"]
    db = capi.DeviceDatabase(res, off, alphabet)
    try:
        if option:
            db.set_option(*option)
        with capi.tuning(COLUMN_SPLIT="0"):
            plain = db.search(query, matrix, gap_open, gap_extend, "score", "sw")["score"]
            if workgroups:
                db.set_option("reserve_cus", capi.DeviceDatabase.last_launch_shape()[0] - workgroups)
                plain = db.search(query, matrix, gap_open, gap_extend, "score", "sw")["score"]
            assert routed(capi)[1] == PAIR_BIASED, f"{tag}: {routed(capi)}"
            redone, groups = routed(capi)[3], routed(capi)[2]
            shape = capi.DeviceDatabase.last_launch_shape()
            units = workgroups or (shape[0] - option[1] if option else shape[0])
            assert shape[1:3] == (min(units, groups), 12), f"{tag}: launch shape {shape}, {groups} groups on {units} units"
            assert not workgroups or groups > 12 * shape[1], f"{tag}: {groups} groups on {shape}: no dynamic round"
        np.testing.assert_array_equal(plain, want, err_msg=f"{tag} split off")
        for setting in settings:
            with capi.tuning(COLUMN_SPLIT=setting):
                got = db.search(query, matrix, gap_open, gap_extend, "score", "sw")["score"]
                assert routed(capi)[1] == PAIR_BIASED + SPLIT, f"{tag} {setting}: {routed(capi)}"
                assert routed(capi)[3] == redone, f"{tag} {setting}: lanes flagged {routed(capi)[3]} != {redone}"
                shape = capi.DeviceDatabase.last_launch_shape()
                forced = min(int(setting), units) if setting.isdigit() else min(units, groups)
                assert shape[1:] == (forced, 12, 0), f"{tag} {setting}: launch shape {shape} on {units} units"
            np.testing.assert_array_equal(got, want, err_msg=f"{tag} split {setting} against the checker")
            np.testing.assert_array_equal(got, plain, err_msg=f"{tag} split {setting} against the split off")
        return redone
    finally:
        db.close()


@pytest.mark.parametrize("length", [300, 299, 301, "240-300"])
def test_target_lengths(capi, length):
    # whole chunks, a padded last chunk, one chunk more; the mix: groups of 60 - 75 chunks, longest first, a ragged
    # last group
    rng = np.random.default_rng(300 if length == "240-300" else length)
    query = _oracle.encode(_data.README_QUERY)
    lengths = rng.integers(240, 301, size=6000) if length == "240-300" else np.full(5120, length)
    res, off = database(rng, query, lengths)
    check(capi, query, res, off, tag=f"L={length}")


@pytest.mark.parametrize("qlen", [1, 2, 33, 53, 64])
def test_query_rows(capi, qlen):
    # every translation unit of the kernel (a: 1, 2; c: 33; d: 53, 64), odd and even row counts
    rng = np.random.default_rng(9100 + qlen)
    query = _data.random_protein(rng, qlen)
    res, off = database(rng, query, np.full(5120, 300))
    if qlen > 60:
        # (the pair table of 61 - 64 rows fits a CU's LDS up to 21 symbols: the 20 amino acids the data is made of)
        check(capi, query, res, off, matrix=B62.reshape(24, 24)[:20, :20].ravel(), alphabet=20, tag=f"Q={qlen}")
    else:
        check(capi, query, res, off, tag=f"Q={qlen}")


def test_state_is_rebased_inside_a_piece(capi):
    # extension 16: the column shift reaches kBiasedMaxShift = 4096 at chunk 64 of 75, inside the pieces that end a
    # group; the producers' pieces leave at other shifts than the unsplit sweep has at that chunk
    rng = np.random.default_rng(2016)
    query = _data.random_protein(rng, 53)
    res, off = database(rng, query, np.full(5120, 300))
    check(capi, query, res, off, gap_open=20, gap_extend=16, tag="gaps 20/16")


def test_best_is_carried_across_a_cut(capi):
    # a block of targets that are the query over and over: the maximum is reached in the first columns and again and
    # again after every cut - a consumer that started from best = 0, or from another group's, would report less
    rng = np.random.default_rng(77)
    query = _data.random_protein(rng, 53)
    res, off = _data.random_db(rng, np.full(7680, 300))
    res = res.copy()
    repeated = np.tile(query, 6)[:300]
    for k in range(2000, 2400):
        res[off[k]:off[k + 1]] = repeated
    for k in range(5000, 5100):
        res[off[k]:off[k] + 53] = query          # the optimum in the first piece only
    check(capi, query, res, off, tag="repeats")


def test_lanes_that_reach_the_limit_are_flagged_alike(capi):
    # match 500: copies of 52 and 53 query residues score 26000 and 26500, beyond the flavour's 25600 - the lanes
    # flagged (and redone) are the same with the split, whichever piece the copy lies in; the rest is exact
    rng = np.random.default_rng(500)
    m = np.full((24, 24), -300, dtype=np.int32)
    np.fill_diagonal(m, 500)
    query = _data.random_protein(rng, 53)
    n = 5120
    res, off = _data.random_db(rng, np.full(n, 300))
    res = res.copy()
    for j, (k, at) in enumerate(((53, 0), (52, 247), (53, 120), (51, 30), (50, 200), (52, 100), (40, 260), (53, 246))):
        t = off[(j * 613 + 7) % n] + at
        res[t:t + k] = query[:k]
    redone = check(capi, query, res, off, matrix=m.ravel(), gap_open=700, gap_extend=100, tag="limit")
    assert redone >= 5   # the copies of 52 and 53 residues


def test_consumers_that_recompute(capi):
    # MIOPAL_COLUMN_SPLIT=recompute: nothing is handed on, every wavefront that finishes a group sweeps it from
    # column 0 - the path a consumer takes when its producer's flag does not arrive
    rng = np.random.default_rng(4)
    query = _oracle.encode(_data.README_QUERY)
    res, off = database(rng, query, rng.integers(240, 301, size=5120))
    check(capi, query, res, off, settings=("recompute",), tag="recompute")


def test_plan_follows_the_reserved_compute_units(capi):
    # 80 groups with eight units reserved: 80 workgroups with the split off (a group each, no second round), the forced
    # plans on 3 and 8, and "recompute" on 80 again - the launch shape says so. Once more with all units but two
    # reserved: the split off has its dynamic round (80 groups, 24 in the static one), the plans are held to 2 workgroups
    rng = np.random.default_rng(8)
    query = _oracle.encode(_data.README_QUERY)
    res, off = database(rng, query, np.full(10240, 300))
    check(capi, query, res, off, option=("reserve_cus", 8), settings=("3", "8", "recompute"), tag="reserve_cus 8")
    check(capi, query, res, off, settings=("3", "8", "recompute"), tag="all but 2 reserved", workgroups=2)


def test_all_result_forms(capi):
    # the kernel writes database order itself: into the library's pinned staging buffer (pageable results), into the
    # caller's pinned array, into a device buffer
    import torch
    rng = np.random.default_rng(3)
    query = _oracle.encode(_data.README_QUERY)
    n = 5120 + 77
    res, off = database(rng, query, np.full(n, 300))
    want = _oracle.search(query, res, off, B62, 3, 1, "score", "sw")["score"]
    db = capi.DeviceDatabase(res, off, 24)
    try:
        pinned = torch.empty(n, dtype=torch.int32).pin_memory().numpy()
        pageable = np.empty(n, dtype=np.int32)
        for setting in ("0", "2", "5", "8"):
            code = PAIR_BIASED + (SPLIT if setting != "0" else 0)
            with capi.tuning(COLUMN_SPLIT=setting):
                for name, buf in (("pageable", pageable), ("pinned", pinned)):
                    buf[:] = -7
                    db.search(query, B62, 3, 1, "score", "sw", score_out=buf)
                    assert routed(capi)[1] == code, (setting, name, routed(capi))
                    np.testing.assert_array_equal(buf, want, err_msg=f"split {setting} {name}")
                out = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
                db.search_device_scores(query, B62, out.data_ptr(), torch.cuda.current_stream().cuda_stream, 3, 1, "sw")
                torch.cuda.synchronize()
                assert routed(capi)[1] == code, (setting, "device", routed(capi))
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"split {setting} device")
    finally:
        db.close()


def test_end_locations_keep_the_dynamic_hand_out(capi):
    # the split carries no end locations: an `end` search under the switch takes the kernel it took before
    rng = np.random.default_rng(12)
    query = _oracle.encode(_data.README_QUERY)
    res, off = database(rng, query, np.full(5120, 120))
    want = _oracle.search(query, res, off, B62, 3, 1, "end", "sw")
    db = capi.DeviceDatabase(res, off, 24)
    try:
        with capi.tuning(COLUMN_SPLIT="3"):
            got = db.search(query, B62, 3, 1, "end", "sw")
            assert routed(capi)[1] == PAIR_BIASED
        for key in ("score", "end_t", "end_q"):
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    finally:
        db.close()


def test_default_plan_on_a_whole_device(capi):
    # no switch: short targets in enough groups that every resident wavefront's interval is at least a group long
    # (one group per wavefront of 256 compute units, and 700 more) - the split is the launch's own choice, and it
    # is not on a database half that size
    rng = np.random.default_rng(1)
    query = _oracle.encode(_data.README_QUERY)
    n = 128 * (12 * 256 + 700) + 5
    res, off = database(rng, query, rng.integers(9, 13, size=n))
    want = _oracle.search_parallel(query, res, off, B62, 3, 1, "score", "sw")["score"]
    db = capi.DeviceDatabase(res, off, 24)
    try:
        got = db.search(query, B62, 3, 1, "score", "sw")["score"]
        assert routed(capi)[1] == PAIR_BIASED + SPLIT, routed(capi)
        np.testing.assert_array_equal(got, want)
        half = db.search(query, B62, 3, 1, "score", "sw", 0, n // 2)["score"]
        assert routed(capi)[1] == PAIR_BIASED, routed(capi)
        np.testing.assert_array_equal(half, want[:n // 2])
    finally:
        db.close()
