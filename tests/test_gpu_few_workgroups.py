"""The persistent lane-per-target kernels on launches of 1, 2, 3 and 5 workgroups ("reserve_cus", miopalDbSetOption):
every round of their hand-out, at database sizes of a megabyte.

A launch has at most one workgroup per compute unit. The one-strip pair-table kernels (interseq_impl.h) give the first
`wavefronts x workgroups` groups of 128 targets out statically and every later group from a counter, with a per-SIMD
share where the groups are of similar length; the strips kernels take (batch, strip) units and the batch kernels
(query, part) units from a counter. At full width a dynamic round needs more than 3072 groups (2048 for NW / HW / OV of
more than 54 rows); on W workgroups it needs `wavefronts x W + 1`. Every case here

  * narrows the launch of its own handle to W workgroups and reads W back from miopalLastLaunchShape (an option that
    was ignored does not pass), with the compute units taken from the same diagnostic;
  * shows from miopalLastRouting that more groups (units) than the static round holds were given out, and which
    kernel took them;
  * compares every array with the CPU checker, and byte for byte - the count of lanes redone for their range
    included - with the same search at full width;
  * fails, not skips, when it does not get its dynamic round.

The databases are sorted by length into the view (longest first), so the targets of the static round are known: noisy
copies of the query are planted only there, or only behind it, in every second target, at the first or at the last
columns. A wavefront that begins its second group with the first group's maximum, columns, rows or range flags
reports a copy's values for an unrelated target (or loses a copy's). Group counts per W and wavefront count:
one dynamic take into a ragged last group, `50 W + 3` groups (three rounds and more, no multiple of 4 W, ragged),
`16 W` (a multiple of 4 W, whole groups). Lengths of 24 - 28 residues (the view's last group holds 4/5 of the longest
group's chunks: the per-SIMD shares are on by default; also forced off) and of 4 - 120 (off by default; also forced
on). The Smith-Waterman one-strip cases keep the column split off (MIOPAL_COLUMN_SPLIT=0): on so few workgroups the
split would be the launch's own choice for score searches of uniform lengths, and its plan is tested on 1 - 8
workgroups in test_gpu_column_split.py."""
import zlib

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
B62_20 = np.ascontiguousarray(B62.reshape(24, 24)[:20, :20]).ravel()
PAIR_INT16, PAIR_HALF, PAIR_BIASED, PAIR_GLOBAL, PAIR_STRIPS, GLOBAL_STRIPS = 2, 3, 4, 5, 6, 7   # miopalLastRouting counts[1]
WORKGROUPS = (1, 2, 3, 5)
KINDS = ("one-take", "rounds", "multiple")
LENGTHS = ("uniform", "ragged")
PLANTINGS = ("static", "dynamic")
KEYS = ("score", "end_t", "end_q")
BASE = _data.random_protein(np.random.default_rng(20), 120)   # every query is a prefix of it
DECOY = _data.random_protein(np.random.default_rng(21), 120)  # ... and every decoy query (narrowed) of this


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def global_waves(qlen):
    """interseq_impl.h, globalWaves: the NW / HW / OV kernel sweeps rows in pairs, twelve wavefronts up to 54 rows"""
    return 12 if qlen + (qlen & 1) <= 54 else 8


def group_count(kind, W, waves):
    return {"one-take": waves * W + 1, "rounds": 50 * W + 3, "multiple": 16 * W}[kind]


class Dataset:
    """`groups` groups of 128 targets (the last one of 77 when `ragged_last`), the first `static_groups` of the
    length-sorted view strictly longer than the rest, shuffled into database order; copies of BASE's prefix in every
    second target of the static round's groups, or of the later ones."""

    RANGES = {"uniform": ((26, 29), (24, 26)), "ragged": ((40, 121), (4, 40)), "flags": ((64, 67), (60, 63)),
              "long head": ((1500, 1601), (24, 29))}

    def __init__(self, capi, groups, static_groups, lengths, planting, ragged_last, seed, alphabet=24, every=2, exact=()):
        rng = np.random.default_rng(seed)
        n = groups * 128 - (51 if ragged_last else 0)
        n_static = static_groups * 128
        assert 0 < n_static < n
        hi, lo = self.RANGES[lengths]
        by_rank = np.concatenate([rng.integers(*hi, size=n_static), rng.integers(*lo, size=n - n_static)])
        rank_of = rng.permutation(n)          # database index -> rank in the view's order by length (static: < n_static)
        self.lens = by_rank[rank_of].astype(np.int64)
        res, self.off = _data.random_db(rng, self.lens)
        res = res.copy()
        self.static = rank_of < n_static
        planted = np.flatnonzero(self.static if planting == "static" else ~self.static)[::every] if planting else []
        for j, k in enumerate(planted):
            L = int(self.lens[k])
            seg = _data.mutate(rng, BASE[:L], 0.1)[:L]
            at = self.off[k] + (0 if j & 1 else L - len(seg))   # the first columns of some, the last columns of others
            res[at:at + len(seg)] = seg
        # `exact`: the first k residues of BASE, for every k, in targets of the static round (the range-flag cases)
        static_ids = np.flatnonzero(self.static)
        for j, k in enumerate(exact):
            at = self.off[static_ids[(j * 613 + 7) % len(static_ids)]] + (j % 3) * 5
            res[at:at + k] = BASE[:k]
        self.res, self.n, self.groups, self.alphabet = res, n, groups, alphabet
        self.db = capi.DeviceDatabase(res, self.off, alphabet)
        self._want = {}

    def want(self, query, matrix, gaps, algo, tag):
        """the CPU checker's scores and end locations, once per (query, scoring, mode of alignment)"""
        key = (len(query), tag, gaps, algo)
        if key not in self._want:
            self._want[key] = _oracle.search_parallel(query, self.res, self.off, matrix, gaps[0], gaps[1], "end", algo, chunk=2048)
        return self._want[key]


_DATASETS = {}


@pytest.fixture(scope="module")
def datasets(capi):
    def get(groups, static_groups, lengths, planting, ragged_last, **more):
        key = (groups, static_groups, lengths, planting, ragged_last, tuple(sorted(more.items())))
        if key not in _DATASETS:
            _DATASETS[key] = Dataset(capi, groups, static_groups, lengths, planting, ragged_last, zlib.crc32(repr(key).encode()), **more)
        return _DATASETS[key]
    yield get
    for ds in _DATASETS.values():
        ds.db.close()
    _DATASETS.clear()


def hand_out_set(datasets, W, waves, kind, lengths, planting, **more):
    return datasets(group_count(kind, W, waves), waves * W, lengths, planting, kind != "multiple", **more)


def decoy(query):
    return [decoy(q) for q in query] if isinstance(query, list) else DECOY[:len(query)]


def narrowed(capi, db, W, run, query, tag):
    """`run(query)` at full width and on W workgroups -> (full, narrow, routing of the narrow run, its launch shape).
    The two runs took the same kernel for the same groups and redid the same number of lanes. Between them the same
    search runs for another query of that length: the buffers of the handle's workspace - view-order scores, the
    staging buffer the kernel scatters into - then hold other values than the full width's answers, so a group that
    the narrowed launch never takes does not pass on what was left there."""
    db.set_option("reserve_cus", -1)
    try:
        full = run(query)
        full_routing, full_shape = capi.DeviceDatabase.last_routing(), capi.DeviceDatabase.last_launch_shape()
        cus = full_shape[0]
        assert cus > max(WORKGROUPS), f"{tag}: {full_shape}"
        assert 0 < full_shape[1] <= cus, f"{tag}: no persistent launch {full_shape}"
        run(decoy(query))
        db.set_option("reserve_cus", 4096 if W == 1 else cus - W)
        narrow = run(query)
        routing, shape = capi.DeviceDatabase.last_routing(), capi.DeviceDatabase.last_launch_shape()
    finally:
        db.set_option("reserve_cus", -1)
    assert shape[0] == cus and shape[1] == W, f"{tag}: launch shape {shape}, wanted {W} workgroups"
    assert routing == full_routing, f"{tag}: routing {routing} on {W} workgroups, {full_routing} at full width"
    return full, narrow, routing, shape


def same(got, want, keys, tag):
    for key in keys:
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{tag} {key}")


def one_strip_case(capi, ds, W, query, matrix, gaps, mode, algo, kernel, waves, share, tag, matrix_tag="b62", **switches):
    """One search of a one-strip kernel: its dynamic round ran, on W workgroups of `waves` wavefronts with the per-SIMD
    share `share` (True: ceil(groups / 4 W), False: off), and the results are the checker's and the full width's."""
    keys = KEYS if mode == "end" else KEYS[:1]
    with capi.tuning(**switches):
        full, got, routing, shape = narrowed(
            capi, ds.db, W, lambda q: ds.db.search(q, matrix, gaps[0], gaps[1], mode, algo), query, tag)
    assert routing[1] == kernel, f"{tag}: kernel word {routing}"
    assert shape[2] == waves, f"{tag}: {shape}"
    assert routing[2] == ds.groups and routing[2] > shape[2] * W, f"{tag}: {routing[2]} groups, no dynamic round on {shape}"
    assert shape[3] == (-(-ds.groups // (4 * W)) if share else 0), f"{tag}: share {shape}"
    same(got, ds.want(query, matrix, gaps, algo, matrix_tag), keys, f"{tag} against the checker")
    same(got, full, keys, f"{tag} against the full width")
    return routing, shape


def report(family, W, routing, shape, units=None):
    """one line per case for profiles/few_workgroups_tests.txt (pytest -s): what the last search of the case ran on"""
    taken = f"{units} units, {units - W} after each workgroup's first" if units else \
        f"{routing[2]} groups, {routing[2] - shape[2] * W} dynamic takes"
    print(f"\nSHAPE {family} W={W}: launch shape {shape}, kernel word {routing[1]}, {taken}")


def throttles(lengths):
    """(MIOPAL_TAIL_THROTTLE, share expected): the default of these lengths and the other setting forced"""
    return ((None, True), ("0", False)) if lengths == "uniform" else ((None, False), ("1", True))


# ---- the one-strip Smith-Waterman kernel on biased halves -----------------------------------------------------------
@pytest.mark.parametrize("planting", PLANTINGS)
@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WORKGROUPS)
def test_one_strip_sw(capi, datasets, W, kind, lengths, planting):
    # rows of every translation unit of the kernel, odd and even; the kernel's own scatter to database order and the
    # scatter kernel that reads view order
    ds = hand_out_set(datasets, W, 12, kind, lengths, planting)
    for qlen in (2, 17, 33, 53, 60):
        for mode in ("score", "end"):
            for scatter in (None, "1"):
                for throttle, share in throttles(lengths):
                    tag = f"sw W={W} {kind} {lengths} {planting} Q={qlen} {mode} scatter={scatter} throttle={throttle}"
                    seen = one_strip_case(capi, ds, W, BASE[:qlen], B62, (3, 1), mode, "sw", PAIR_BIASED, 12, share, tag,
                                          COLUMN_SPLIT="0", NO_DIRECT_SCATTER=scatter, TAIL_THROTTLE=throttle)
    report(f"one-strip sw {kind} {lengths} {planting}", W, *seen)


# ---- the general Smith-Waterman flavours of the pair table (launchPairFlavour) ----------------------------------------
@pytest.mark.parametrize("planting", PLANTINGS)
@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WORKGROUPS)
def test_general_sw_flavours(capi, datasets, W, kind, lengths, planting):
    # MIOPAL_NO_BIASED: half floats for matrices within +-1024 (score_ranges.h, halfFloatFits: BLOSUM62), saturating
    # int16 beyond (BLOSUM62 times a hundred with gaps 300 / 100: the same alignments); scores only - end locations
    # need the biased flavour - and this hand-out has no shares
    ds = hand_out_set(datasets, W, 12, kind, lengths, planting)
    for qlen in (17, 53):
        for matrix, gaps, kernel, name in ((B62, (3, 1), PAIR_HALF, "b62"), (B62 * 100, (300, 100), PAIR_INT16, "b62x100")):
            tag = f"general W={W} {kind} {lengths} {planting} Q={qlen} {name}"
            seen = one_strip_case(capi, ds, W, BASE[:qlen], matrix, gaps, "score", "sw", kernel, 12, False, tag,
                                  matrix_tag=name, NO_BIASED="1")
    report(f"general sw {kind} {lengths} {planting}", W, *seen)


# ---- the one-strip NW / HW / OV kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("planting", PLANTINGS)
@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qlen", [53, 60])
@pytest.mark.parametrize("W", WORKGROUPS)
def test_one_strip_global(capi, datasets, W, qlen, kind, lengths, planting):
    # 53 rows: twelve wavefronts per workgroup, 60 rows: eight - the static round, and with it the database, differ
    waves = global_waves(qlen)
    assert (global_waves(53), global_waves(54), global_waves(55), global_waves(60)) == (12, 12, 8, 8)
    ds = hand_out_set(datasets, W, waves, kind, lengths, planting)
    for algo in ("nw", "hw", "ov"):
        for mode in ("score", "end"):
            for throttle, share in throttles(lengths):
                tag = f"{algo} W={W} {kind} {lengths} {planting} Q={qlen} {mode} throttle={throttle}"
                seen = one_strip_case(capi, ds, W, BASE[:qlen], B62, (3, 1), mode, algo, PAIR_GLOBAL, waves, share, tag,
                                      TAIL_THROTTLE=throttle)
    report(f"one-strip nw/hw/ov Q={qlen} {kind} {lengths} {planting}", W, *seen)
    # (OV: targets whose optimum lies in their last column are among them)
    assert np.any(ds.want(BASE[:qlen], B62, (3, 1), "ov", "b62")["end_t"] == ds.lens - 1)


# ---- lanes that leave the range, in the static round only ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WORKGROUPS)
def test_range_flags_are_not_inherited(capi, datasets, W, kind):
    # match 500 / mismatch -300 at 53 rows: copies of 52 and 53 query residues score 26000 and 26500, beyond the
    # flavour's 25600; they lie in groups of the static round only, so a wavefront that kept its flags (or its maximum)
    # for the next group would have lanes of a dynamic group redone, or wrong
    ds = hand_out_set(datasets, W, 12, kind, "flags", None, exact=(53, 52, 53, 51, 52, 50, 53, 40))
    m = np.full((24, 24), -300, dtype=np.int32)
    np.fill_diagonal(m, 500)
    m = m.ravel()
    for throttle, share in throttles("uniform"):
        tag = f"flags W={W} {kind} throttle={throttle}"
        routing, shape = one_strip_case(capi, ds, W, BASE[:53], m, (700, 100), "score", "sw", PAIR_BIASED, 12, share, tag,
                                        matrix_tag="500", COLUMN_SPLIT="0", TAIL_THROTTLE=throttle)
        assert routing[3] >= 5, f"{tag}: {routing}"   # the copies of 52 and 53 residues; as many as at full width (narrowed())
    report(f"range flags {kind}, {routing[3]} lanes redone", W, routing, shape)


# ---- the strips kernels ---------------------------------------------------------------------------------------------------
STRIPS_GROUPS = 150


@pytest.mark.parametrize("planting", PLANTINGS)
@pytest.mark.parametrize("W", WORKGROUPS)
def test_strips_kernels(capi, datasets, W, planting):
    # forced (MIOPAL_PAIR_STRIPS) as in test_gpu_row_dispatch.py; queries of 2 and 3 strips (80 and 120 rows: two strips
    # of 40, three of 40). The units are (batch of at most 12 groups, strip), strip-major: 13 batches x 2 or 3 strips on
    # W workgroups - each takes several, rebuilds its table when the strip changes and reads boundary rows that it or
    # a neighbour wrote
    ds = datasets(STRIPS_GROUPS, STRIPS_GROUPS // 2, "ragged", planting, True, every=8)
    variants = (("sw", "score", PAIR_STRIPS, {}), ("sw", "end", PAIR_STRIPS, {}),
                ("sw", "end", PAIR_STRIPS, {"TWO_PASS_ENDS": "1"}), ("nw", "score", GLOBAL_STRIPS, {}),
                ("nw", "end", GLOBAL_STRIPS, {}))
    for qlen, strips in ((80, 2), (120, 3)):
        query = BASE[:qlen]
        for algo, mode, kernel, switches in variants:
            tag = f"strips W={W} {planting} Q={qlen} {algo} {mode} {switches}"
            keys = KEYS if mode == "end" else KEYS[:1]
            with capi.tuning(PAIR_STRIPS="1", **switches):
                full, got, routing, shape = narrowed(capi, ds.db, W, lambda q: ds.db.search(q, B62, 3, 1, mode, algo), query, tag)
            assert routing[1] & 31 == kernel, f"{tag}: kernel word {routing}"
            assert shape[2:] == (12, 0), f"{tag}: {shape}"
            # (a batch holds at most twelve groups, a query of `strips` strips is not swept in fewer)
            units = -(-routing[2] // 12) * strips
            assert routing[2] == ds.groups and units > 3 * W, f"{tag}: {units} units for {W} workgroups"
            same(got, ds.want(query, B62, (3, 1), algo, "b62"), keys, f"{tag} against the checker")
            same(got, full, keys, f"{tag} against the full width")
        report(f"strips Q={qlen} {planting}", W, routing, shape, units)


# ---- the score pass behind other entry points -------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["pssm", "device_scores", "top"])
@pytest.mark.parametrize("W", [1, 3])
def test_other_entry_points(capi, datasets, W, entry):
    ds = hand_out_set(datasets, W, 12, "rounds", "uniform", "static")
    query = BASE[:53]
    want = ds.want(query, B62, (3, 1), "sw", "b62")
    tag = f"{entry} W={W}"
    if entry == "pssm":
        # (the matrix's rows of the query's residues: the plain search's answers)
        call = lambda q: ds.db.search_pssm(B62.reshape(24, 24)[q], q, 3, 1, "end", "sw")
    elif entry == "device_scores":
        import torch

        def call(q):
            out = torch.full((ds.n,), -7, dtype=torch.int32, device="cuda:0")
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())   # (the fill above)
            with torch.cuda.stream(stream):
                ds.db.search_device_scores(q, B62, out.data_ptr(), stream.cuda_stream, 3, 1, "sw")
            stream.synchronize()
            return {"score": out.cpu().numpy()}
    else:
        call = lambda q: ds.db.search_top(q, B62, 3, 1, "end", "sw", k=25)
    with capi.tuning(COLUMN_SPLIT="0"):
        full, got, routing, shape = narrowed(capi, ds.db, W, call, query, tag)
    assert routing[1] == PAIR_BIASED and shape[2] == 12, f"{tag}: {routing} {shape}"
    assert routing[2] == ds.groups and routing[2] > 12 * W, f"{tag}: {routing}"
    assert shape[3] == -(-ds.groups // (4 * W)), f"{tag}: {shape}"
    if entry == "top":
        order = np.lexsort((np.arange(ds.n), -want["score"].astype(np.int64)))[:25]
        assert got["count"] == 25 and full["count"] == 25
        np.testing.assert_array_equal(got["target"], order, err_msg=tag)
        for key in KEYS:
            np.testing.assert_array_equal(got[key], want[key][order], err_msg=f"{tag} {key}")
        same(got, full, ("target",) + KEYS, f"{tag} against the full width")
    else:
        keys = KEYS if entry == "pssm" else KEYS[:1]
        same(got, want, keys, f"{tag} against the checker")
        same(got, full, keys, f"{tag} against the full width")
    report(entry, W, routing, shape)


# ---- a launch that begins behind the first groups of the view -----------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3])
def test_group_base_of_the_dynamic_round(capi, datasets, W):
    # NW (no windows): 256 targets of 1500 - 1600 residues at the head of the view are worth the wavefront-per-pair
    # kernel's while (planSideCut), so the persistent launch starts at the view's third group - a.groupBase = 2 - and its
    # dynamic round must add that base to what the counter hands out
    groups = 2 + group_count("rounds", W, 12)
    ds = datasets(groups, 2, "long head", "dynamic", True)
    query = BASE[:53]
    for mode in ("score", "end"):
        tag = f"group base W={W} {mode}"
        keys = KEYS if mode == "end" else KEYS[:1]
        full, got, routing, shape = narrowed(capi, ds.db, W, lambda q: ds.db.search(q, B62, 3, 1, mode, "nw"), query, tag)
        assert routing[1] == PAIR_GLOBAL and shape[2] == 12, f"{tag}: {routing} {shape}"
        assert routing[0] == 256 and routing[2] == groups - 2, f"{tag}: the first groups did not leave the launch: {routing}"
        assert routing[2] > 12 * W, f"{tag}: {routing}"
        same(got, ds.want(query, B62, (3, 1), "nw", "b62"), keys, f"{tag} against the checker")
        same(got, full, keys, f"{tag} against the full width")
    report("group base (nw)", W, routing, shape)


# ---- a Smith-Waterman view with windows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2])
def test_view_with_windows(capi, W):
    # six targets of 3000 residues (three hold a copy of the query: at their first columns, in the middle, at their very
    # last columns) among 50 W + 3 groups of short ones: the long ones are cut into windows that are merged on the
    # device, by maximum for scores and by key for end locations
    rng = np.random.default_rng(3000 + W)
    query = BASE[:53]
    n = (50 * W + 3) * 128 - 51
    lens = rng.integers(24, 29, size=n)
    long_ids = rng.choice(n, size=6, replace=False)
    lens[long_ids] = 3000
    res, off = _data.random_db(rng, lens)
    res = res.copy()
    for k, at in ((long_ids[0], 40), (long_ids[1], 1260), (long_ids[2], 2947)):
        seg = _data.mutate(rng, query, 0.05)[:53]
        res[off[k] + at:off[k] + at + len(seg)] = seg
    for k in range(0, n, 7):
        if lens[k] < 100:
            seg = _data.mutate(rng, BASE[:28], 0.1)[:lens[k]]
            res[off[k]:off[k] + len(seg)] = seg
    want = _oracle.search_parallel(query, res, off, B62, 3, 1, "end", "sw", chunk=2048)
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for mode in ("score", "end"):
            tag = f"windows W={W} {mode}"
            keys = KEYS if mode == "end" else KEYS[:1]
            with capi.tuning(COLUMN_SPLIT="0"):
                full, got, routing, shape = narrowed(capi, db, W, lambda q: db.search(q, B62, 3, 1, mode, "sw"), query, tag)
                plan = capi.DeviceDatabase.last_window_plan()
            assert plan[0] > 0 and plan[2] > n, f"{tag}: no windows {plan}"
            assert plan[3] == (1 if mode == "end" else 0), f"{tag}: {plan}"
            assert routing[1] == PAIR_BIASED and shape[2] == 12, f"{tag}: {routing} {shape}"
            assert routing[2] > 12 * W, f"{tag}: {routing}"
            same(got, want, keys, f"{tag} against the checker")
            same(got, full, keys, f"{tag} against the full width")
        report(f"windows {plan}", W, routing, shape)
    finally:
        db.close()


# ---- the batch kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,mode", [("sw", "score"), ("sw", "end"), ("nw", "end")])
@pytest.mark.parametrize("W", [1, 3])
def test_batch_kernels(capi, datasets, W, algo, mode):
    # four queries in each of the row classes 8, 32 and 64 (the 20-letter alphabet: 64 rows of 21 symbols fit a
    # CU's LDS): a launch per class, each of 4 x (units per query) units on W workgroups - more queries than
    # workgroups, so some workgroup takes more units than one query has, moves on to another query and rebuilds
    # its table
    ds = datasets(50, 25, "ragged", "static", True, alphabet=20)
    queries = [BASE[:q] for q in (5, 6, 7, 8, 25, 27, 30, 32, 61, 62, 63, 64)]
    keys = KEYS if mode == "end" else KEYS[:1]
    tag = f"batch W={W} {algo} {mode}"
    batch_routing = []

    def call(qs):
        out = ds.db.search_batch(qs, B62_20, 3, 1, mode, algo)
        batch_routing.append(capi.DeviceDatabase.last_batch_routing())
        return out

    ds.db.set_option("reserve_cus", -1)
    try:
        full = call(queries)
        full_shape = capi.DeviceDatabase.last_launch_shape()
        cus = full_shape[0]
        assert cus > max(WORKGROUPS) and full_shape[1] > W, f"{tag}: {full_shape}"
        call(decoy(queries))   # (other values into the workspace's rows, as in narrowed())
        ds.db.set_option("reserve_cus", 4096 if W == 1 else cus - W)
        got = call(queries)
        shape = capi.DeviceDatabase.last_launch_shape()
        single = [ds.db.search(q, B62_20, 3, 1, mode, algo) for q in queries]
    finally:
        ds.db.set_option("reserve_cus", -1)
    # (the last launch is the class of 64 rows: eight wavefronts per workgroup)
    assert shape == (cus, W, 8, 0), f"{tag}: launch shape {shape}"
    assert batch_routing[0] == batch_routing[2], f"{tag}: {batch_routing}"
    settled, on_the_side, single_path, launches = batch_routing[2]
    assert (single_path, launches) == (0, 3) and settled > 0, f"{tag}: {batch_routing[2]}"
    assert 4 > W   # (a launch's units are 4 queries x at least one part each: more than its workgroups)
    for i, query in enumerate(queries):
        want = ds.want(query, B62_20, (3, 1), algo, "b62_20")
        for key in keys:
            np.testing.assert_array_equal(got[key][i], want[key], err_msg=f"{tag} query {i} {key} against the checker")
            np.testing.assert_array_equal(got[key][i], single[i][key], err_msg=f"{tag} query {i} {key} against the search")
    for key in keys:
        assert got[key].tobytes() == full[key].tobytes(), f"{tag} {key} against the full width"
    print(f"\nSHAPE batch {algo} {mode} W={W}: launch shape {shape} (class 64), full width {full_shape}, routing {batch_routing[2]}")
