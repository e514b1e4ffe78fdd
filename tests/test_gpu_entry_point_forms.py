"""The three forms of every selecting entry point of `Aligner` - one query, a list of queries (`_many`), a `Pssm`
(`_pssm`) - give the same answer, and that answer is the selection made in Python from `align` / `align_pssm` of the
query: `top_hits`, `hits`, `significant_hits` (unsorted and sorted), `best_queries`, and `align_pairs` /
`align_pairs_pssm` on the chosen pairs. Every field of every result object is compared, and the order.

About 70 random protein targets of 0-130 residues (an empty one, several of more than 64), queries of 1, 53 and 65
residues (the 65-residue one leaves the shared batch launches for the single-query path inside the same call),
BLOSUM62 with gaps 3/1 and, for two cases, 11/1; modes score / end / full, algorithms sw and nw.

The cuts come from the `align` scores of this database, so that no list is empty and none holds every target: the
threshold is the middle one of the distinct scores, k half the number of targets at or above it. ``max_evalue`` is
chosen in Python from the E-values of a first fit (`ScoreFit.evalue`), in the widest gap between two neighbouring
E-values; the expected hits of a significance search are then the targets at or above the integer per-bin thresholds
of the fit that very call returned (`ScoreFit.threshold`) - a cut taken from the fit's own thresholds, because the
E-value fit of a 70-target sample puts targets close enough to the cut that restating it in floating point could
differ by a rounding. The E-values themselves are compared with `ScoreFit.evalue` to 1e-9 relative (the same formula
on the same integers; the margin is for libm)."""
import numpy as np
import pytest

import _data
import pyopal_amd
from pyopal_amd import Pssm

pytestmark = pytest.mark.gpu

TARGETS = 70
QUERY_LENGTHS = (1, 53, 65)
FIELDS = ("target_index", "score", "query_end", "target_end", "query_start", "target_start", "query_length",
          "target_length", "alignment")
CASES = [(3, 1, mode, algo) for mode in ("score", "end", "full") for algo in ("sw", "nw")] + [(11, 1, "full", "sw"),
                                                                                               (11, 1, "end", "nw")]


def letters(codes):
    return "".join(_data.NCBI[c] for c in codes)


def field(result, name):
    """A field of a result object; None where the property refuses to answer (the -1 locations of an empty alignment)."""
    try:
        return getattr(result, name)
    except AssertionError:
        return None


def fields(result):
    return (type(result).__name__,) + tuple(field(result, name) for name in FIELDS if hasattr(type(result), name))


def same(got, want, what):
    assert [fields(r) for r in got] == [fields(r) for r in want], what


@pytest.fixture(scope="module")
def case():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    rng = np.random.default_rng(70)
    lengths = np.concatenate(([0, 130, 64, 65, 1], rng.integers(2, 131, size=TARGETS - 5)))
    rng.shuffle(lengths)
    queries = [letters(_data.random_protein(rng, L)) for L in QUERY_LENGTHS]
    sequences = [letters(_data.random_protein(rng, int(L))) for L in lengths]
    # a few targets that hold a noisy copy of a query, so that the best scores stand out
    for k, q in ((7, 1), (23, 2), (41, 1), (58, 2)):
        if lengths[k] > 0:
            copy = letters(_data.mutate(rng, _data.encode(queries[q])))[:int(lengths[k])]
            sequences[k] = copy + sequences[k][len(copy):]
    assert [len(s) for s in sequences] == lengths.tolist()
    database = pyopal_amd.Database(sequences)
    pssms = [Pssm.from_sequence(q, "BLOSUM62") for q in queries]
    return database, queries, pssms, lengths.astype(np.int64), {}


def everything(case, gap_open, gap_extend, mode, algo):
    """(aligner, [align(q) for q], [align_pssm(p) for p]) - computed once per case and never changed"""
    database, queries, pssms, _, cache = case
    key = (gap_open, gap_extend, mode, algo)
    if key not in cache:
        aligner = pyopal_amd.Aligner("BLOSUM62", gap_open, gap_extend)
        plain = [aligner.align(q, database, mode=mode, algorithm=algo) for q in queries]
        profile = [aligner.align_pssm(p, database, mode=mode, algorithm=algo) for p in pssms]
        for a, b in zip(plain, profile):
            same(b, a, "align_pssm of the query's own PSSM against align")
        cache[key] = (aligner, plain, profile)
    return cache[key]


def cut_of(scores):
    """the middle one of the distinct scores: some target is at or above it, and not every one"""
    distinct = sorted(set(scores))
    assert len(distinct) >= 2
    cut = distinct[len(distinct) // 2]
    assert 0 < sum(s >= cut for s in scores) < len(scores)
    return cut


def best_first(results):
    return sorted(results, key=lambda r: (-r.score, r.target_index))


@pytest.mark.parametrize("gap_open, gap_extend, mode, algo", CASES)
def test_top_hits_forms(case, gap_open, gap_extend, mode, algo):
    database, queries, pssms, _, _ = case
    aligner, plain, profile = everything(case, gap_open, gap_extend, mode, algo)
    kw = dict(mode=mode, algorithm=algo)
    cuts = [cut_of([r.score for r in rows]) for rows in plain]
    ks = [max(1, sum(r.score >= c for r in rows) // 2) for rows, c in zip(plain, cuts)]
    for k in sorted(set(ks)):
        many = aligner.top_hits_many(queries, database, k, **kw)
        for i, (q, p) in enumerate(zip(queries, pssms)):
            want = best_first(plain[i])[:k]
            assert 0 < len(want) < TARGETS
            same(aligner.top_hits(q, database, k, **kw), want, ("top_hits", i, k))
            same(many[i], want, ("top_hits_many", i, k))
            same(aligner.top_hits_pssm(p, database, k, **kw), best_first(profile[i])[:k], ("top_hits_pssm", i, k))
    # with a bound on the score: fewer than k
    for i, (q, p) in enumerate(zip(queries, pssms)):
        want = [r for r in best_first(plain[i]) if r.score >= cuts[i]]
        assert 0 < len(want) < TARGETS
        same(aligner.top_hits(q, database, TARGETS, min_score=cuts[i], **kw), want, ("top_hits, min_score", i))
        same(aligner.top_hits_many(queries, database, TARGETS, min_score=cuts[i], **kw)[i], want, ("top_hits_many, min_score", i))
        same(aligner.top_hits_pssm(p, database, TARGETS, min_score=cuts[i], **kw), want, ("top_hits_pssm, min_score", i))
    # the chosen pairs through the pair lists
    pairs = [(i, r.target_index) for i in range(len(queries)) for r in best_first(plain[i])[:ks[i]]]
    want = [plain[i][t] for i, t in pairs]
    same(aligner.align_pairs(queries, database, pairs, **kw), want, "align_pairs")
    same(aligner.align_pairs_pssm(pssms, database, pairs, **kw), want, "align_pairs_pssm")
    same(aligner.align_pairs(queries, database, pairs[::-1], **kw), want[::-1], "align_pairs, reversed")


@pytest.mark.parametrize("gap_open, gap_extend, mode, algo", CASES)
def test_hits_forms(case, gap_open, gap_extend, mode, algo):
    database, queries, pssms, _, _ = case
    aligner, plain, profile = everything(case, gap_open, gap_extend, mode, algo)
    kw = dict(mode=mode, algorithm=algo)
    cuts = [cut_of([r.score for r in rows]) for rows in plain]
    for sort in (False, True):
        many = aligner.hits_many(queries, database, cuts, sort=sort, **kw)
        assert len(many) == len(queries)
        for i, (q, p) in enumerate(zip(queries, pssms)):
            want = [r for r in plain[i] if r.score >= cuts[i]]
            assert 0 < len(want) < TARGETS
            want = best_first(want) if sort else want
            same(aligner.hits(q, database, cuts[i], sort=sort, **kw), want, ("hits", i, sort))
            same(many[i], want, ("hits_many", i, sort))
            want = [r for r in profile[i] if r.score >= cuts[i]]
            same(aligner.hits_pssm(p, database, cuts[i], sort=sort, **kw), best_first(want) if sort else want,
                 ("hits_pssm", i, sort))


def evalue_cut(aligner, query, database, algo, scores, lengths):
    """a max_evalue in the widest gap between neighbouring E-values of a first fit, past the 5 lowest at least"""
    fit = aligner.significant_hits_arrays(query, database, 1.0, algorithm=algo)["fit"]
    assert not fit.degenerate
    ev = np.sort(fit.evalue(scores, lengths))
    ev = ev[np.isfinite(ev) & (ev > 0)]
    assert len(ev) >= 40
    at = 5 + int(np.argmax(ev[6:40] / ev[5:39]))
    assert ev[at + 1] > ev[at]
    return float(np.sqrt(ev[at] * ev[at + 1]))


@pytest.mark.parametrize("gap_open, gap_extend, mode, algo", CASES)
def test_significant_hits_forms(case, gap_open, gap_extend, mode, algo):
    database, queries, pssms, lengths, _ = case
    aligner, plain, profile = everything(case, gap_open, gap_extend, mode, algo)
    kw = dict(mode=mode, algorithm=algo)
    scores = [np.array([r.score for r in rows], dtype=np.int64) for rows in plain]
    cuts = [evalue_cut(aligner, q, database, algo, s, lengths) for q, s in zip(queries, scores)]

    def check(got, i, rows, sort, what):
        fit = got.fit
        assert not fit.degenerate
        chosen = np.flatnonzero(scores[i] >= fit.threshold(lengths).astype(np.int64))
        assert 0 < len(chosen) < TARGETS, what
        evalue = fit.evalue(scores[i][chosen], lengths[chosen])
        assert np.all(evalue <= cuts[i] * (1 + 1e-9)), what
        rest = np.setdiff1d(np.arange(TARGETS), chosen)
        assert not np.any(fit.evalue(scores[i][rest], lengths[rest]) <= cuts[i] * (1 - 1e-9)), what
        if sort:
            order = np.lexsort((chosen, evalue))
            chosen, evalue = chosen[order], evalue[order]
        same(got.results, [rows[t] for t in chosen], what)
        np.testing.assert_allclose(got.evalues, evalue, rtol=1e-9, atol=0, err_msg=str(what))
        np.testing.assert_allclose(got.zscores, fit.zscore(scores[i][chosen], lengths[chosen]), rtol=1e-9, atol=0,
                                   err_msg=str(what))
        assert [e for _, e in got] == got.evalues.tolist()

    for sort in (False, True):
        many = aligner.significant_hits_many(queries, database, cuts, sort=sort, **kw)
        assert len(many) == len(queries)
        for i, (q, p) in enumerate(zip(queries, pssms)):
            check(aligner.significant_hits(q, database, cuts[i], sort=sort, **kw), i, plain[i], sort, ("single", i, sort))
            check(many[i], i, plain[i], sort, ("many", i, sort))
            check(aligner.significant_hits_pssm(p, database, cuts[i], sort=sort, **kw), i, profile[i], sort,
                  ("pssm", i, sort))


@pytest.mark.parametrize("gap_open, gap_extend, mode, algo", CASES)
def test_best_queries_against_align(case, gap_open, gap_extend, mode, algo):
    database, queries, _, _, _ = case
    aligner, plain, _ = everything(case, gap_open, gap_extend, mode, algo)
    kw = dict(mode=mode, algorithm=algo)
    floor = cut_of([r.score for rows in plain for r in rows])
    for m, min_score in ((1, None), (2, None), (2, floor), (3, floor)):
        got = aligner.best_queries(queries, database, m, min_score=min_score, **kw)
        assert len(got) == TARGETS
        kept = 0
        for t in range(TARGETS):
            ranked = sorted((i for i in range(len(queries)) if min_score is None or plain[i][t].score >= min_score),
                            key=lambda i: (-plain[i][t].score, i))[:m]
            assert [i for i, _ in got[t]] == ranked, (t, m, min_score)
            same([r for _, r in got[t]], [plain[i][t] for i in ranked], ("best_queries", t, m, min_score))
            kept += len(ranked)
        assert 0 < kept and ((m, min_score) != (3, floor) or kept < TARGETS * 3)
