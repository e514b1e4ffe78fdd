"""The inputs of the range-edge tests (tests/_edges.py) and the CPU checker they are compared with, on the CPU:

  * the checker (oracle/opal_oracle.c) against the affine-gap recurrence written out in numpy int64, all four modes,
    on the edge family under a model far beyond anything a 16-bit kernel takes,
  * the family does what it is for: a best score of exactly Q * match in every mode, and the NW score of an
    all-one-letter query against a run of the low letter in closed form,
  * the checker's 32-bit sums stay below 2^29 for every model test_gpu_range_edges.py can reach.
"""
import numpy as np
import pytest

import _edges
import _oracle

ALGOS = ["nw", "hw", "ov", "sw"]
RULES = {"nw": (1, 1, 0), "hw": (0, 1, 0), "ov": (0, 0, 0), "sw": (0, 0, 1)}   # top gap, left gap, floor at 0


def gotoh_scores(queries, targets, matrix, A, go, ge, algo):
    """Scores only, one numpy lane per (query, target) pair (queries of one length), int64 throughout:
    H = max(diagonal + s, E, F), E / F = max(H - open, E / F - ext); borders of k + 1 residues cost open + k ext (or
    k + 1 openings where that is cheaper); NW reads the last cell, HW the last row, OV the last row and the last
    column, SW every cell with a floor at 0."""
    S = np.asarray(matrix, dtype=np.int64).reshape(A, A)
    top, left, floor0 = RULES[algo]
    Qs = np.asarray(queries, dtype=np.int64)
    n, Q = Qs.shape
    lens = np.array([len(t) for t in targets], dtype=np.int64)
    T = np.zeros((n, max(int(lens.max()), 1)), dtype=np.int64)
    for k, t in enumerate(targets):
        T[k, :len(t)] = t
    NEG = -(1 << 60)
    border = lambda gap, k: -min(go + k * ge, (k + 1) * go) if gap and k >= 0 else 0
    Hprev = np.repeat(np.array([border(left, i) for i in range(Q)], dtype=np.int64)[:, None], n, axis=1)
    Eprev = np.full((Q, n), NEG, dtype=np.int64)
    best = np.where(lens == 0, 0 if floor0 else border(left, Q - 1), 0 if floor0 else NEG).astype(np.int64)
    for j in range(int(lens.max())):
        s = S[Qs.T, T[:, j][None, :]]
        E = np.maximum(Hprev - go, Eprev - ge)
        H = np.empty((Q, n), dtype=np.int64)
        up_h, up_f, diag = np.full(n, border(top, j)), np.full(n, NEG), np.full(n, border(top, j - 1))
        for i in range(Q):
            f = np.maximum(up_h - go, up_f - ge)
            h = np.maximum(np.maximum(diag + s[i], E[i]), f)
            if floor0:
                h = np.maximum(h, 0)
            diag, H[i], up_h, up_f = Hprev[i], h, h, f
        last = lens - 1 == j
        if algo == "nw":
            best = np.where(last, H[Q - 1], best)
        elif algo == "sw":
            best = np.where(j < lens, np.maximum(best, H.max(axis=0)), best)
        else:
            best = np.where(j < lens, np.maximum(best, H[Q - 1]), best)
            if algo == "ov":
                best = np.where(last, np.maximum(best, H.max(axis=0)), best)
        Hprev, Eprev = H, E
    return best


def families(Q, long, forms=_edges.QUERY_FORMS, n_random=200):
    out = []
    for form in forms:
        q = _edges.edge_query(form, Q)
        out.append((form, q, _edges.family(q, long=long, n_random=n_random)))
    return out


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("Q", [2, 12])
def test_checker_agrees_with_the_numpy_recurrence_under_extreme_models(Q, algo):
    m = _edges.EXTREME
    matrix = _edges.model_matrix(m)
    fams = families(Q, _edges.LONG)
    queries = np.concatenate([np.repeat(q[None, :], len(seqs), axis=0) for _, q, seqs in fams])
    targets = [t for _, _, seqs in fams for t in seqs]
    ref = gotoh_scores(queries, targets, matrix, _edges.ALPHABET, m["open"], m["ext"], algo)
    at = 0
    for form, q, seqs in fams:
        res, off = _oracle.flatten(seqs)
        got = _oracle.search(q, res, off, matrix, m["open"], m["ext"], "score", algo)["score"]
        np.testing.assert_array_equal(got, ref[at:at + len(seqs)], err_msg=f"{algo} Q={Q} {form}")
        at += len(seqs)
    if algo == "nw":
        assert ref.min() < -(3000 * m["ext"])   # (the family reaches the bottom it is built for)


@pytest.mark.parametrize("tag,Q,model", [(f"{flavour} {tag}", Q, m) for flavour, models in _edges.GENERAL_MODELS.items()
                                         for tag, Q, m in models] + [("base", 7, _edges.BASE)])
def test_checker_agrees_with_the_numpy_recurrence_on_shared_models(tag, Q, model):
    # (the CPU tier's word on "the numpy reference and the C checker agree on every model in the shared list" is the
    # test below; here the general kernel's models at a longer family)
    matrix = _edges.model_matrix(model)
    for algo in ALGOS:
        for form, q, seqs in families(min(Q, 12), 200, n_random=40):
            res, off = _oracle.flatten(seqs)
            got = _oracle.search(q, res, off, matrix, model["open"], model["ext"], "score", algo)["score"]
            ref = gotoh_scores(np.repeat(q[None, :], len(seqs), axis=0), seqs, matrix, _edges.ALPHABET,
                               model["open"], model["ext"], algo)
            np.testing.assert_array_equal(got, ref, err_msg=f"{tag} {algo} {form}")


def test_checker_agrees_with_the_numpy_recurrence_on_every_shared_model():
    # every far end the GPU tier can reach, at a size the numpy recurrence takes in a blink
    for tag, _, _, model in _edges.shared_models():
        matrix = _edges.model_matrix(model)
        q = _edges.edge_query("random", 5)
        seqs = _edges.family(q, long=40, n_random=12)
        res, off = _oracle.flatten(seqs)
        for algo in ALGOS:
            got = _oracle.search(q, res, off, matrix, model["open"], model["ext"], "score", algo)["score"]
            ref = gotoh_scores(np.repeat(q[None, :], len(seqs), axis=0), seqs, matrix, _edges.ALPHABET,
                               model["open"], model["ext"], algo)
            np.testing.assert_array_equal(got, ref, err_msg=f"{tag} {algo}")


@pytest.mark.parametrize("Q,match,go,ge,low", [(60, 433, 3, 1, -4), (147, 205, 3, 1, -4), (60, 11, 8000, 1, -4),
                                                (12, 4000, 9000, 819, -1023)])
def test_family_reaches_the_top_of_the_range(Q, match, go, ge, low):
    matrix = _edges.edge_matrix(_edges.ALPHABET, match, -1, low, _edges.LETTER_C)
    for form, q, seqs in families(Q, _edges.LONG):
        res, off = _oracle.flatten(seqs)
        for algo in ALGOS:
            score = _oracle.search(q, res, off, matrix, go, ge, "score", algo)["score"]
            assert score.max() == Q * match, (form, algo)
            assert score[0] == Q * match, (form, algo)   # (the copy of the query)
    if (Q, go) == (60, 8000):
        assert _oracle.search(q, res, off, matrix, go, ge, "score", "nw")["score"].min() <= -11179


@pytest.mark.parametrize("Q", [1, 2, 12, 60])
@pytest.mark.parametrize("model", [_edges.BASE, _edges.EXTREME, dict(_edges.BASE, open=8000), dict(_edges.BASE, low=-1023)],
                         ids=["base", "extreme", "open8000", "low-1023"])
def test_nw_of_one_letter_against_a_low_run_in_closed_form(Q, model):
    # min(Q, L) pairings at `low` and one gap of |L - Q| residues, or the query and the target each in a gap of its own
    go, ge, low = model["open"], model["ext"], model["low"]
    gap = lambda k: go + (k - 1) * ge if k > 0 else 0
    q = _edges.edge_query("one", Q)
    lengths = [1, 2, Q - 1, Q, Q + 1, 4 * Q, _edges.LONG]
    lengths = [L for L in lengths if L > 0]
    res, off = _oracle.flatten([_edges.pc(L) for L in lengths])
    got = _oracle.search(q, res, off, _edges.model_matrix(model), go, ge, "score", "nw")["score"]
    want = [max(min(Q, L) * low - gap(abs(L - Q)), -(gap(Q) + gap(L))) for L in lengths]
    assert got.tolist() == want


def test_checker_sums_stay_below_2_29_for_every_shared_model():
    # every H, E, F of the checker is within 2 open + (Q + L) ext + (min(Q, L) + 1) max |S| of zero
    for tag, Q, L, m in _edges.shared_models() + [("extreme", 12, _edges.LONG + 12, _edges.EXTREME)]:
        mag = max(abs(m["match"]), abs(m["low"]), abs(m["mild"]))
        bound = 2 * m["open"] + (Q + L) * m["ext"] + (min(Q, L) + 1) * mag
        assert bound < 1 << 29, (tag, bound)
