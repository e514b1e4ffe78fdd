"""Significant hits: E-values from score statistics gathered on the device (miopalSearchSignificant /
miopalSearchPssmSignificant / miopalSearchBatchSignificant; DeviceDatabase.search_significant and its forms;
Aligner.significant_hits). Every integer the device returns - the per-bin sums of all targets and of those under the
ceilings, the per-bin targets and lengths, the hits - is compared exactly with numpy on the PLAIN search's scores; the
fit and the E-values with a restatement of include/miopal.h's formulas from the same integers (1e-9 relative: sums of
at most 127 doubles in the same order, the margin is for libm). One end-to-end case: 12 mutated copies of the query
planted among 3000 random targets are exactly the hits at E <= 1e-3."""
import math
import threading

import numpy as np
import pytest

import _data
import pyopal_amd
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
BINS = 128
GUMBEL = math.pi / math.sqrt(6.0)
GAMMA = 0.5772156649015329
PLANTED = 12


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def bins_of(lengths):
    out = np.zeros(len(lengths), dtype=np.int64)
    for k, L in enumerate(np.asarray(lengths).tolist()):
        if L:
            e = L.bit_length() - 1
            out[k] = 1 + 4 * e + ((L >> (e - 2)) & 3 if e >= 2 else (L << (2 - e)) & 3)
    return out


def planted_database(rng, query, targets, low, high, planted, empties=()):
    """`targets` random proteins, lengths log-uniform in [low, high], `planted` of them replaced by mutated copies of
    the query inside 0-200 random residues on each side -> (sequences, indices of the planted ones)"""
    lengths = np.exp(rng.uniform(math.log(low), math.log(high), size=targets)).astype(np.int64)
    seqs = [_data.random_protein(rng, int(L)) for L in lengths]
    where = np.sort(rng.choice(targets, size=planted, replace=False))
    for k in where:
        seqs[k] = np.concatenate([_data.random_protein(rng, int(rng.integers(0, 201))),
                                  _data.mutate(rng, query, rate=0.3),
                                  _data.random_protein(rng, int(rng.integers(0, 201)))]).astype(np.uint8)
    for k in empties:
        assert k not in where
        seqs[k] = np.zeros(0, dtype=np.uint8)
    return seqs, where


def flatten(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.ascontiguousarray(np.concatenate(seqs), dtype=np.uint8), off


@pytest.fixture(scope="module")
def planted_set(capi):
    """the end-to-end case of the design: 3000 targets of 40-1200 residues, a 150-residue query, 12 planted copies"""
    rng = np.random.default_rng(2024)
    query = _data.random_protein(rng, 150)
    seqs, where = planted_database(rng, query, 3000, 40, 1200, PLANTED)
    res, off = flatten(seqs)
    db = capi.DeviceDatabase(res, off, 24)
    yield db, off, query, where
    db.close()


@pytest.fixture(scope="module")
def mixed_set(capi):
    """4000 targets of 20-2000 residues, two empty ones, 6 planted copies of a 60-residue query"""
    rng = np.random.default_rng(77)
    query = _data.random_protein(rng, 60)
    seqs, where = planted_database(rng, query, 4000, 20, 2000, 6, empties=(3, 1000))
    res, off = flatten(seqs)
    db = capi.DeviceDatabase(res, off, 24)
    yield db, off, query, where
    db.close()


def want_stats(score, bins, ceiling=None):
    out = np.zeros((BINS, 3), dtype=np.int64)
    s = score.astype(np.int64)
    keep = np.ones(len(s), dtype=bool) if ceiling is None else s <= np.asarray(ceiling, dtype=np.int64)[bins]
    np.add.at(out[:, 0], bins[keep], 1)
    np.add.at(out[:, 1], bins[keep], s[keep])
    np.add.at(out[:, 2], bins[keep], s[keep] * s[keep])
    return out


def restate(fit, max_evalue):
    """include/miopal.h's fit and table from the integers of `fit` (a pyopal_amd.ScoreFit), in Python floats"""
    x, mean = [0.0] * BINS, [math.nan] * BINS
    Sn = Snx = Snxx = Ss = Sxs = 0.0
    used = bins = 0
    held = [b for b in range(1, BINS) if fit.bin_targets[b] > 0]
    for b in held:
        x[b] = math.log(float(fit.bin_length[b]) / float(fit.bin_targets[b]))
        n, s = float(fit.kept[b, 0]), float(fit.kept[b, 1])
        if n <= 0:
            continue
        bins += 1
        used += int(fit.kept[b, 0])
        Sn += n
        Snx += n * x[b]
        Snxx += n * x[b] * x[b]
        Ss += s
        Sxs += x[b] * s
    out = {"used": used, "degenerate": True, "targets": int(fit.bin_targets[1:].sum())}
    if used < 3:
        return out
    denom = Sn * Snxx - Snx * Snx
    slope, intercept = 0.0, Ss / Sn
    if bins > 1 and denom > 0:
        slope = (Sn * Sxs - Snx * Ss) / denom
        intercept = (Ss - slope * Snx) / Sn
    resid = 0.0
    for b in held:
        if fit.kept[b, 0] <= 0:
            continue
        m = intercept + slope * x[b]
        resid += float(fit.kept[b, 2]) - 2 * m * float(fit.kept[b, 1]) + float(fit.kept[b, 0]) * m * m
    if not resid > 0:
        return out
    sigma = math.sqrt(resid / (used - 2))
    for b in held:
        mean[b] = intercept + slope * x[b]
    p = max_evalue / out["targets"]
    z_cut = -math.inf if p >= 1 else -(math.log(-math.log1p(-p)) + GAMMA) / GUMBEL
    out.update(degenerate=False, intercept=intercept, slope=slope, sigma=sigma, z_cut=z_cut, mean=mean, held=held)
    return out


def close(a, b):
    return a == b or abs(a - b) <= 1e-9 * max(abs(a), abs(b))


def check_against_plain(got, plain, lengths, start, max_evalue, mode, exclude_z=5.0):
    """everything `got` (search_significant's dict) holds against the plain search `plain` of the same slice"""
    raw = got["fit"]
    fit = pyopal_amd.ScoreFit(raw)
    bins = bins_of(lengths)
    score = plain["score"]
    # the integers: exact
    want_targets = np.bincount(bins, minlength=BINS)
    assert np.array_equal(fit.bin_targets, want_targets)
    assert np.array_equal(fit.bin_length, np.array([lengths[bins == b].sum() for b in range(BINS)], dtype=np.int64))
    assert fit.targets == int(np.count_nonzero(lengths > 0))
    assert np.array_equal(fit.all, want_stats(score, bins))
    if fit.passes == 1:
        assert np.all(fit.ceilings == INT_MAX) and np.array_equal(fit.kept, fit.all)
    else:
        assert np.array_equal(fit.kept, want_stats(score, bins, fit.ceilings))
    assert 1 <= fit.passes <= 1 + 3 and (exclude_z > 0 or fit.passes == 1)
    assert np.all(fit.ceilings[fit.bin_targets == 0] == INT_MAX) and fit.ceilings[0] == INT_MAX
    # the hits: the plain search filtered with the table
    keep = np.nonzero(score >= fit.thresholds[bins].astype(np.int64))[0]
    assert got["count"] == len(keep)
    assert got["target"].dtype == np.int64 and np.array_equal(got["target"], start + keep)
    assert got["score"].dtype == np.int32 and np.array_equal(got["score"], score[keep])
    if mode == "end":
        assert np.array_equal(got["end_q"], plain["end_q"][keep]) and np.array_equal(got["end_t"], plain["end_t"][keep])
    else:
        assert "end_q" not in got and "end_t" not in got
    assert fit.thresholds[0] == INT_MAX and np.all(fit.thresholds[fit.bin_targets == 0] == INT_MAX)
    # the fit and the E-values: the formulas restated
    want = restate(fit, max_evalue)
    assert fit.used == want["used"] and fit.degenerate == want["degenerate"]
    if fit.degenerate:
        assert got["count"] == 0 and np.all(fit.thresholds == INT_MAX)
        return fit, keep
    for name in ("intercept", "slope", "sigma", "z_cut"):
        assert close(getattr(fit, name), want[name]), (name, getattr(fit, name), want[name])
    for b in want["held"]:
        if want["z_cut"] == -math.inf:
            assert fit.thresholds[b] == INT_MIN
            continue
        cut = want["mean"][b] + want["z_cut"] * want["sigma"]
        if abs(cut - round(cut)) > 1e-6:
            assert fit.thresholds[b] == math.ceil(cut), (b, fit.thresholds[b], cut)
    assert got["evalue"].dtype == np.float64 and len(got["evalue"]) == len(keep)
    for k, e in zip(keep.tolist(), got["evalue"].tolist()):
        z = (float(score[k]) - want["mean"][bins[k]]) / want["sigma"]
        assert close(e, want["targets"] * -math.expm1(-math.exp(-GUMBEL * z - GAMMA))), (k, e)
        assert e <= max_evalue * (1 + 1e-9)
    # (the Python layer's copies of the formulas)
    if len(keep):
        assert np.allclose(fit.evalue(score[keep], lengths[keep]), got["evalue"], rtol=1e-9, atol=0)
        assert np.array_equal(fit.threshold(lengths[keep]), fit.thresholds[bins[keep]])
    return fit, keep


def test_planted_copies_are_exactly_the_hits(planted_set):
    db, off, query, where = planted_set
    got = db.search_significant(query, B62, 11, 1, "score", "sw", max_evalue=1e-3)
    assert np.array_equal(got["target"], where), (got["target"], where)
    fit, _ = check_against_plain(got, db.search(query, B62, 11, 1, "score", "sw"), np.diff(off), 0, 1e-3, "score")
    assert not fit.degenerate and fit.targets == 3000 and fit.passes >= 2
    assert fit.slope > 0 and fit.z_cut > 8                    # longer random targets score higher; 1e-3 / 3000 is far out
    assert np.all(got["evalue"] <= 1e-3)
    # the scale is calibrated: the random targets with E <= 10 are about ten (8 - 13 in the design's CPU runs)
    loose = db.search_significant(query, B62, 11, 1, "score", "sw", max_evalue=10.0)
    assert 2 <= loose["count"] - PLANTED <= 25 and set(where) <= set(loose["target"].tolist())


@pytest.mark.parametrize("algo", ["sw", "hw"])
@pytest.mark.parametrize("mode", ["score", "end"])
def test_statistics_fit_and_hits_against_the_plain_search(mixed_set, algo, mode):
    db, off, query, where = mixed_set
    lengths = np.diff(off)
    for start, end, max_evalue in ((0, 4000, 1e-3), (0, 4000, 50.0), (999, 3500, 1.0)):
        plain = db.search(query, B62, 11, 1, mode, algo, start, end)
        routing = db.last_routing()
        got = db.search_significant(query, B62, 11, 1, mode, algo, start, end, max_evalue)
        assert db.last_routing() == routing
        fit, keep = check_against_plain(got, plain, lengths[start:end], start, max_evalue, mode)
        assert not fit.degenerate
        assert not np.any(lengths[start:end][keep] == 0)      # empty targets are never hits
        if algo == "sw":
            assert set(where[(where >= start) & (where < end)]) <= set(got["target"].tolist())
        if algo == "sw" and max_evalue == 50.0:
            assert got["count"] > len(where)                  # (about fifty random targets among them: no case is vacuous)


def test_exclude_z_zero_is_one_pass(mixed_set):
    db, off, query, where = mixed_set
    plain = db.search(query, B62, 11, 1, "score", "sw")
    got = db.search_significant(query, B62, 11, 1, "score", "sw", max_evalue=1e-3, exclude_z=0.0)
    fit, _ = check_against_plain(got, plain, np.diff(off), 0, 1e-3, "score", exclude_z=0.0)
    assert fit.passes == 1 and fit.used == fit.targets
    refit = pyopal_amd.ScoreFit(db.search_significant(query, B62, 11, 1, "score", "sw", max_evalue=1e-3)["fit"])
    assert refit.passes >= 2 and refit.used < refit.targets and refit.sigma < fit.sigma   # the planted ones inflate it
    got = db.search_significant(query, B62, 11, 1, "score", "sw", max_evalue=1e-3, exclude_z=-2.0)
    assert pyopal_amd.ScoreFit(got["fit"]).passes == 1


def test_a_cut_at_the_number_of_targets_keeps_every_non_empty_target(mixed_set):
    db, off, query, where = mixed_set
    lengths = np.diff(off)
    for max_evalue in (3998.0, 1e6):
        got = db.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=max_evalue)
        assert np.array_equal(got["target"], np.nonzero(lengths > 0)[0]) and got["count"] == 3998
        check_against_plain(got, db.search(query, B62, 11, 1, "end", "sw"), lengths, 0, max_evalue, "end")


def test_two_targets_are_degenerate(capi):
    rng = np.random.default_rng(5)
    res, off = _data.random_db(rng, [120, 300])
    db = capi.DeviceDatabase(res, off, 24)
    try:
        for max_evalue in (1e-3, 100.0):
            got = db.search_significant(res[:50], B62, 11, 1, "end", "sw", max_evalue=max_evalue)
            fit = pyopal_amd.ScoreFit(got["fit"])
            assert got["count"] == 0 and len(got["target"]) == 0 and len(got["evalue"]) == 0
            assert fit.degenerate and fit.targets == 2 and fit.used == 2 and np.all(fit.thresholds == INT_MAX)
            assert fit.all[:, 0].sum() == 2
        # an empty slice: nothing launched, a zeroed fit
        got = db.search_significant(res[:50], B62, 11, 1, "end", "sw", 1, 1, 1e-3)
        fit = pyopal_amd.ScoreFit(got["fit"])
        assert got["count"] == 0 and fit.degenerate and fit.targets == 0 and fit.passes == 0 and not fit.all.any()
        got = db.search_batch_significant([res[:50], res[:9]], B62, 11, 1, "score", "sw", 2, 2, 1e-3)
        assert got["offsets"].tolist() == [0, 0, 0] and all(f.degenerate == 1 for f in got["fits"])
    finally:
        db.close()


def test_max_hits_overflow_fills_the_fit(capi, mixed_set):
    db, off, query, where = mixed_set
    want = db.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=50.0)
    assert want["count"] > 6
    got = db.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=50.0, max_hits=want["count"])
    assert np.array_equal(got["target"], want["target"])
    for bound in (want["count"] - 1, 0):
        with pytest.raises(capi.TooManyHits) as info:
            db.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=50.0, max_hits=bound)
        assert info.value.counts == want["count"]
        assert bytes(info.value.fit) == bytes(want["fit"])
    # the handle stays usable
    again = db.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=50.0)
    assert np.array_equal(again["target"], want["target"]) and np.array_equal(again["evalue"], want["evalue"])


def test_subset_handle_builds_its_own_bins(mixed_set):
    db, off, query, where = mixed_set
    rng = np.random.default_rng(8)
    picked = np.sort(np.concatenate([rng.choice(4000, size=1500, replace=False), where]))
    picked = np.unique(picked)[::-1].copy()        # another order: the bins are the subset's, not the parent's
    db.search_significant(query, B62, 11, 1, "score", "sw")   # (the parent's bins exist)
    sub = db.subset(picked)
    try:
        lengths = np.diff(off)[picked]
        got = sub.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=1e-2)
        check_against_plain(got, sub.search(query, B62, 11, 1, "end", "sw"), lengths, 0, 1e-2, "end")
        assert set(np.nonzero(np.isin(picked, where))[0].tolist()) <= set(got["target"].tolist())
    finally:
        sub.close()


def same_answer(a, b):
    assert a["count"] == b["count"]
    for key in ("target", "score", "end_q", "end_t", "evalue"):
        assert (key in a) == (key in b)
        if key in a:
            assert np.array_equal(a[key], b[key]), key
    assert bytes(a["fit"]) == bytes(b["fit"])


def test_pssm_form_equals_the_plain_form(mixed_set):
    db, off, query, where = mixed_set
    pssm = pyopal_amd.Pssm.from_sequence("".join(_data.NCBI[c] for c in query))
    assert np.array_equal(pssm.scores, B62.reshape(24, 24)[query])
    for algo, mode, start, end in (("sw", "end", 0, 4000), ("hw", "score", 500, 4000)):
        want = db.search_significant(query, B62, 11, 1, mode, algo, start, end, 1.0)
        got = db.search_pssm_significant(pssm.scores, 11, 1, mode, algo, start, end, 1.0)
        same_answer(got, want)
        assert want["count"] > 0


def test_two_threads_on_one_fresh_handle(capi, mixed_set):
    db, off, query, where = mixed_set
    want = db.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=1.0)
    # a handle that has not built its bins: both threads arrive at the first significance search at once
    fresh = db.subset(np.arange(4000))
    try:
        results, errors = [None, None], []
        barrier = threading.Barrier(2)

        def work(k):
            try:
                barrier.wait()
                for _ in range(3):
                    results[k] = fresh.search_significant(query, B62, 11, 1, "end", "sw", max_evalue=1.0)
            except Exception as err:   # noqa: BLE001
                errors.append(err)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for got in results:
            same_answer(got, want)
    finally:
        fresh.close()


def check_batch_rows(db, queries, cuts, mode, algo, got, rows, start=0, end=None):
    for i in rows:
        want = db.search_significant(queries[i], B62, 11, 1, mode, algo, start, end, float(cuts[i]))
        lo, hi = int(got["offsets"][i]), int(got["offsets"][i + 1])
        assert hi - lo == want["count"], (i, hi - lo, want["count"])
        for key in ("target", "score", "end_q", "end_t", "evalue"):
            assert (key in got) == (key in want)
            if key in want:
                assert np.array_equal(got[key][lo:hi], want[key]), (i, key)
        assert bytes(got["fits"][i]) == bytes(want["fit"]), i


@pytest.mark.parametrize("algo,mode", [("sw", "end"), ("hw", "score")])
def test_batch_equals_the_single_query_calls(mixed_set, algo, mode):
    db, off, query, where = mixed_set
    rng = np.random.default_rng(13)
    # lengths on both sides of the batch kernels' 64 rows: 0, 65 and 150 take the single-query path inside the call
    queries = [np.zeros(0, dtype=np.uint8), query[:9], _data.random_protein(rng, 64), _data.random_protein(rng, 65),
               np.concatenate([query, _data.random_protein(rng, 90)]), query]
    cuts = [1.0, 50.0, 1e-3, 10.0, 1e-3, 4000.0]
    got = db.search_batch_significant(queries, B62, 11, 1, mode, algo, max_evalue=cuts)
    assert got["offsets"][0] == 0 and len(got["target"]) == got["offsets"][-1] == len(got["evalue"])
    check_batch_rows(db, queries, cuts, mode, algo, got, range(len(queries)))
    assert got["fits"][0].degenerate == 1 or algo != "sw"     # an empty query scores 0 everywhere: no spread
    assert got["offsets"][-1] - got["offsets"][-2] == 3998    # the last cut is above the number of targets
    sliced = db.search_batch_significant(queries, B62, 11, 1, mode, algo, 100, 3000, cuts, exclude_z=0.0)
    for i in range(len(queries)):
        want = db.search_significant(queries[i], B62, 11, 1, mode, algo, 100, 3000, cuts[i], exclude_z=0.0)
        assert bytes(sliced["fits"][i]) == bytes(want["fit"])
        assert np.array_equal(sliced["target"][sliced["offsets"][i]:sliced["offsets"][i + 1]], want["target"])


def test_batch_of_two_chunks(capi, mixed_set):
    db, off, query, where = mixed_set
    rng = np.random.default_rng(14)
    # 4000 targets: 2097 rows fill a chunk of 2^23 pairs; three launch groups of 1024 rows inside the first chunk
    count = 2110
    queries = [_data.random_protein(rng, 9) for _ in range(count)]
    queries[5], queries[2097], queries[-1] = query[:40], query[10:60], query[:30]
    cuts = np.where(np.arange(count) % 2 == 0, 1.0, 1e-2)
    got = db.search_batch_significant(queries, B62, 11, 1, "score", "sw", max_evalue=cuts)
    check_batch_rows(db, queries, cuts, "score", "sw", got, [0, 5, 1023, 1024, 2096, 2097, 2098, count - 1])
    # every row: the plain batch filtered with the row's table
    plain = db.search_batch(queries, B62, 11, 1, "score", "sw")["score"]
    bins = bins_of(np.diff(off))
    for i in range(count):
        table = np.array(got["fits"][i].threshold, dtype=np.int64)
        keep = np.nonzero(plain[i] >= table[bins])[0]
        assert np.array_equal(got["target"][got["offsets"][i]:got["offsets"][i + 1]], keep), i
    total = int(got["offsets"][-1])
    assert total > 0
    with pytest.raises(capi.TooManyHits) as info:
        db.search_batch_significant(queries, B62, 11, 1, "score", "sw", max_evalue=cuts, max_hits=total - 1)
    assert np.array_equal(info.value.counts, got["offsets"])
    assert bytes(info.value.fits[2097]) == bytes(got["fits"][2097])


def test_python_layer(planted_set):
    db_handle, off, query, where = planted_set
    letters = lambda codes: "".join(_data.NCBI[c] for c in codes)   # noqa: E731
    aligner = pyopal_amd.Aligner("BLOSUM62", gap_open=11, gap_extend=1)   # (the matrix of Pssm.from_sequence)
    # a smaller copy of the planted database: the Python layer keeps its own device mirror
    rng = np.random.default_rng(2025)
    planted, where = planted_database(rng, query, 1200, 40, 1200, 8)
    database = pyopal_amd.Database([letters(s) for s in planted])
    q = letters(query)
    hits = aligner.significant_hits(q, database, 1e-3)
    assert isinstance(hits, pyopal_amd.SignificantHits) and len(hits) == len(hits.results) == len(hits.evalues)
    assert [r.target_index for r in hits.results] == where.tolist()
    assert [(r.target_index, e) for r, e in hits] == list(zip(where.tolist(), hits.evalues.tolist()))
    assert np.all(hits.evalues <= 1e-3) and np.all(hits.zscores >= hits.fit.z_cut) and not hits.fit.degenerate
    lengths = np.array([len(planted[k]) for k in where])
    assert np.allclose(hits.zscores, hits.fit.zscore([r.score for r in hits.results], lengths), rtol=1e-12)
    assert np.allclose(hits.evalues, hits.fit.evalue([r.score for r in hits.results], lengths), rtol=1e-9)
    # full: the selection in score mode, then the pair list - `hits` at the same pairs
    # (E <= 20 among 1200 targets: about twenty random ones beside the planted - none at all has probability e^-20)
    loose = aligner.significant_hits(q, database, 20.0, mode="full", sort=True)
    order = np.lexsort(([r.target_index for r in loose.results], loose.evalues))
    assert order.tolist() == list(range(len(loose))) and len(loose) > len(where)
    assert np.all(np.diff(loose.evalues) >= 0)
    everything = {r.target_index: r for r in aligner.hits(q, database, INT_MIN, mode="full")}
    for r in loose.results:
        w = everything[r.target_index]
        assert (r.score, r.query_end, r.target_end, r.query_start, r.target_start, r.alignment) == \
               (w.score, w.query_end, w.target_end, w.query_start, w.target_start, w.alignment)
    unsorted = aligner.significant_hits_arrays(q, database, 20.0, mode="end")
    assert np.all(np.diff(unsorted["target"]) > 0) and sorted(unsorted["target"].tolist()) == sorted(
        r.target_index for r in loose.results)
    assert {"evalue", "zscore", "fit", "end_q", "end_t", "offsets"} <= set(unsorted)
    # the batch and PSSM forms
    many = aligner.significant_hits_many([q, q[:40]], database, [1e-3, 1.0])
    assert [r.target_index for r in many[0].results] == where.tolist() and len(many) == 2
    single = aligner.significant_hits(q[:40], database, 1.0)
    assert [r.target_index for r in many[1].results] == [r.target_index for r in single.results]
    assert np.array_equal(many[1].evalues, single.evalues)
    pssm = pyopal_amd.Pssm.from_sequence(q)
    by_pssm = aligner.significant_hits_pssm(pssm, database, 1e-3)
    assert [r.target_index for r in by_pssm.results] == where.tolist() and np.array_equal(by_pssm.evalues, hits.evalues)
