"""The one-strip Smith-Waterman kernel at the query's own row count (interseq_impl.h, the odd counts in
interseq_swb16_*_odd.hip) on databases shaped like the headline's: targets of one length in 313 to 1670 groups
of 128. At full width that is less than one group per wavefront (miopalLastLaunchShape: one workgroup per compute
unit, twelve wavefronts each - the static first round hands out 3072 groups on 256 units), so the per-SIMD shares
of the end game (host_search.inc, tailThrottle) are set but no group is ever taken dynamically. Every case
therefore runs once more with compute units reserved ("reserve_cus") so that the launch has a third of a
wavefront per group: the dynamic rounds and their shares run, and the launch shape is asserted to say so. (Should
the device have so few compute units that the full width has a dynamic round itself, the repeat is not needed and
not made.) Bit-exact against the CPU checker, scores and end locations, through the C ABI and the device-scores
entry. tests/test_gpu_few_workgroups.py holds the hand-out's own tests."""
import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
PAIR_BIASED = 4  # miopalLastRouting counts[1]: 2 + kPairSwBiased


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def uniform_db(rng, query, n, length):
    """n targets of one length, every 97th a noisy copy of the query cut or padded to it (high scores)."""
    res, off = _data.random_db(rng, np.full(n, length))
    res = res.copy()
    for k in range(0, n, 97):
        t = _data.mutate(rng, query, 0.1)[:length]
        res[off[k]:off[k] + len(t)] = t
    return res, off


def launch_checked(capi, tag, workgroups=None, throttle=None):
    """The launch shape of the search just made: one workgroup per compute unit or per group (or `workgroups`, when
    units were reserved), twelve wavefronts, the share ceil(groups / 4 workgroups) where it is on (`throttle`: "1" / "0",
    None: not asserted). -> (compute units, groups, whether a dynamic round ran)"""
    routing, shape = capi.DeviceDatabase.last_routing(), capi.DeviceDatabase.last_launch_shape()
    groups = routing[2]
    assert shape[1] == (workgroups or min(shape[0], groups)) and shape[2] == 12, f"{tag}: launch shape {shape}, {routing}"
    if throttle is not None:
        assert shape[3] == (-(-groups // (4 * shape[1])) if throttle == "1" else 0), f"{tag}: share {shape}, {routing}"
    dynamic = groups > shape[1] * shape[2]
    assert dynamic or workgroups is None, f"{tag}: {groups} groups on {shape}: no dynamic round"
    return shape[0], groups, dynamic


class reserved:
    """After a search at full width that had no dynamic round: the handle narrowed to a third of a wavefront per group
    (`.workgroups`; None: the full width had its dynamic round, nothing is reserved). The column split stays off
    (MIOPAL_COLUMN_SPLIT=0): with so many groups per wavefront it would be the choice of a score search of targets of
    one length, and it hands out nothing dynamically."""

    def __init__(self, capi, db, tag, throttle=None):
        cus, groups, dynamic = launch_checked(capi, tag, throttle=throttle)
        self.db = db
        self.workgroups = None if dynamic else max(1, groups // 36)
        self.keep = None if dynamic else (4096 if self.workgroups == 1 else cus - self.workgroups)
        self.split_off = capi.tuning(COLUMN_SPLIT="0")

    def __enter__(self):
        if self.keep is not None:
            self.split_off.__enter__()
            self.db.set_option("reserve_cus", self.keep)
        return self.workgroups

    def __exit__(self, *exc):
        self.db.set_option("reserve_cus", -1)
        if self.keep is not None:
            self.split_off.__exit__(*exc)


def check(capi, db, query, res, off, modes=("score", "end"), tag=""):
    for mode in modes:
        got = db.search(query, B62, 3, 1, mode, "sw")
        assert capi.DeviceDatabase.last_routing()[1] & 31 == PAIR_BIASED, f"{tag} {mode}"
        want = _oracle.search_parallel(query, res, off, B62, 3, 1, mode, "sw")
        for key in ("score", "end_t", "end_q"):
            if key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=f"{tag} {mode} {key}")
        # (targets of one length: the shares are on by default)
        with reserved(capi, db, f"{tag} {mode}", throttle="1") as workgroups:
            if workgroups:
                again = db.search(query, B62, 3, 1, mode, "sw")
                assert capi.DeviceDatabase.last_routing()[1] & 31 == PAIR_BIASED, f"{tag} {mode}"
                launch_checked(capi, f"{tag} {mode} reserved", workgroups, "1")
                for key in ("score", "end_t", "end_q"):
                    if key in want:
                        np.testing.assert_array_equal(again[key], want[key], err_msg=f"{tag} {mode} {key} reserved")


# odd and even row counts on both sides of every boundary between translation units (16 / 32 / 48 rows)
@pytest.mark.parametrize("qlen", [1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 50, 53, 54, 59, 60])
def test_row_counts_around_the_instantiation_boundaries(capi, qlen):
    rng = np.random.default_rng(7000 + qlen)
    query = _data.random_protein(rng, qlen)
    # 80 000 targets: 625 groups - at full width one round, with units reserved (check) 17 workgroups: 204 groups in
    # the static round, several per SIMD after it, and a remainder that is not a whole round
    res, off = uniform_db(rng, query, 80_000, 40)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        check(capi, db, query, res, off, tag=f"Q={qlen}")
    finally:
        db.close()


@pytest.mark.parametrize("n", [128 * 1024 + 128, 128 * 1024 + 256, 128 * 1024 + 128 * 645 + 77])
def test_headline_query_device_scores_with_remainders(capi, n):
    # the README query (53 rows, odd) on the headline's direct path: database order written by the kernel;
    # 1025, 1026 and 1670 groups (a ragged last one): one static round at full width; with units reserved, on 28 and 46
    # workgroups, three rounds and a remainder that is no whole round of the SIMDs
    import torch
    rng = np.random.default_rng(n)
    query = _oracle.encode(_data.README_QUERY)
    res, off = uniform_db(rng, query, n, 24)
    want = _oracle.search_parallel(query, res, off, B62, 3, 1, "score", "sw")["score"]
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for throttle in ("1", "0"):
            with capi.tuning(TAIL_THROTTLE=throttle):
                out = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
                stream = torch.cuda.current_stream().cuda_stream
                db.search_device_scores(query, B62, out.data_ptr(), stream, 3, 1, "sw")
                torch.cuda.synchronize()
                assert capi.DeviceDatabase.last_routing()[1] & 31 == PAIR_BIASED
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"n={n} throttle {throttle}")
                with reserved(capi, db, f"n={n} throttle {throttle}", throttle) as workgroups:
                    if workgroups:
                        out = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
                        db.search_device_scores(query, B62, out.data_ptr(), stream, 3, 1, "sw")
                        torch.cuda.synchronize()
                        assert capi.DeviceDatabase.last_routing()[1] & 31 == PAIR_BIASED
                        launch_checked(capi, f"n={n} throttle {throttle} reserved", workgroups, throttle)
                        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"n={n} throttle {throttle} reserved")
    finally:
        db.close()


def test_end_game_on_and_off_agree(capi):
    # scores and end locations with the per-SIMD shares forced on and off: identical, and the checker's
    rng = np.random.default_rng(11)
    query = _data.random_protein(rng, 53)
    res, off = uniform_db(rng, query, 150_000, 30)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        got, narrow = {}, {}
        for throttle in ("1", "0"):
            with capi.tuning(TAIL_THROTTLE=throttle):
                got[throttle] = db.search(query, B62, 3, 1, "end", "sw")
                assert capi.DeviceDatabase.last_routing()[1] & 31 == PAIR_BIASED
                # (1172 groups: one round at full width; on 32 workgroups the shares decide who takes the last groups)
                with reserved(capi, db, f"throttle {throttle}", throttle) as workgroups:
                    if workgroups:
                        narrow[throttle] = db.search(query, B62, 3, 1, "end", "sw")
                        assert capi.DeviceDatabase.last_routing()[1] & 31 == PAIR_BIASED
                        launch_checked(capi, f"throttle {throttle} reserved", workgroups, throttle)
        want = _oracle.search_parallel(query, res, off, B62, 3, 1, "end", "sw")
        for key in ("score", "end_t", "end_q"):
            np.testing.assert_array_equal(got["1"][key], got["0"][key], err_msg=key)
            np.testing.assert_array_equal(got["1"][key], want[key], err_msg=key)
            for throttle, again in narrow.items():
                np.testing.assert_array_equal(again[key], want[key], err_msg=f"{key} reserved, throttle {throttle}")
    finally:
        db.close()


def test_odd_rows_lanes_leave_the_range_and_are_redone(capi):
    # match 500 at 53 rows (odd): copies of k query residues score 500 k, the scores-only flavour is exact
    # below 25600 (k = 51); uniform lengths. 313 groups are one round at full width; with units reserved (8 workgroups)
    # the lanes that leave sit in groups of the static round and of the end game, and as many are redone
    rng = np.random.default_rng(53)
    m = np.full((24, 24), -300, dtype=np.int32)
    np.fill_diagonal(m, 500)
    m = m.ravel()
    query = _data.random_protein(rng, 53)
    n, length = 40_000, 64
    res, off = _data.random_db(rng, np.full(n, length))
    res = res.copy()
    for j, k in enumerate((53, 52, 51, 50, 49, 40)):
        at = off[(j * 6151) % n]
        res[at + 5:at + 5 + k] = query[:k]
    db = capi.DeviceDatabase(res, off, 24)
    try:
        got = db.search(query, m, 700, 100, "score", "sw")
        redone = capi.DeviceDatabase.last_routing()[3]
        want = _oracle.search_parallel(query, res, off, m, 700, 100, "score", "sw")
        np.testing.assert_array_equal(got["score"], want["score"])
        assert redone >= 2   # the copies of 52 and 53 residues
        with reserved(capi, db, "range", throttle="1") as workgroups:
            if workgroups:
                again = db.search(query, m, 700, 100, "score", "sw")
                launch_checked(capi, "range reserved", workgroups, "1")
                assert capi.DeviceDatabase.last_routing()[3] == redone
                np.testing.assert_array_equal(again["score"], want["score"])
    finally:
        db.close()
