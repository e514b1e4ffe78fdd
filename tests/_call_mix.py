"""The nodes of the call-order tests (tests/test_call_mix_cpu.py, tests/test_gpu_call_order.py): one small database, a
fixed list of named calls on it - every entry point of `_capi.DeviceDatabase`, most of them in a large and a small form -
and the answer each call must give whatever ran on the handle before it. A node is a closure ``(db) -> dict of numpy
arrays`` with every argument fixed; its expected answer comes from the CPU witnesses of the suite (the C checker
`_oracle.search`, numpy selections from its rows, the class identity of `_pssm`, `_occurrences`,
`_occurrence_alignments`, `_profile`) and involves no device code. The one exception is the significance search: its
fit is what the same call returns on a fresh handle (`Node.expected` takes that answer), its hits the targets at or
above the fit's thresholds on the checker's scores.

The small form of a family has a strictly shorter query and a slice inside the large form's, so that the small call
runs in the prefix of every buffer the large one filled. Cuts and k come from the checker's scores (`cut_of`): no
answer is empty and none holds every target.

`circuit(n)` is an Eulerian circuit of the complete directed graph with loops on n nodes: every ordered pair (A, then
B), (A, A) included, is consecutive exactly once. `segments` cuts it into runs that begin with the last node of the run
before, so no pair is lost at a cut."""
import functools
import threading
import typing

import numpy as np

import _data
import _occurrence_alignments
import _occurrences
import _oracle
import _profile
import _pssm
from pyopal_amd import _capi
from pyopal_amd.matrices import ScoringMatrix

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
ALPHABET = 24
GAPS = (3, 1)
TARGETS = 203
LONGEST = 3000
LONG_AT = 190            # the 3000-residue target
EMPTY = (7, 45)          # the two empty targets (45: inside SMALL)
NOISY_AT = 50            # holds a noisy copy of the longest query (inside SMALL)
TWICE_AT = 120           # holds the 53-residue query twice
SMALL = (40, 60)         # the slice of the small forms
SHORT = (0, 170)         # the slice of the aligned occurrence searches: every target but the long one's neighbourhood
TAIL = (170, TARGETS)    # a slice that holds the 3000-residue target
MAX_EVALUE = 1e-2
BAD_ARGUMENT = 101       # include/miopal.h, MIOPAL_ERR_BAD_ARGUMENT


class Side(typing.NamedTuple):
    """What a call searches with, in every form the entry points and the witnesses take: the query (or the classes of a
    PSSM's rows) with its matrix for the checker, the rows for the PSSM entry points and the numpy witnesses."""
    query: np.ndarray      # uint8[Q]; of a PSSM: the class of every row, which is also its consensus
    matrix: np.ndarray     # int32[A * A]
    rows: np.ndarray       # int32[Q][A]: matrix[query]
    alphabet: int


class World(typing.NamedTuple):
    residues: np.ndarray
    offsets: np.ndarray
    targets: list
    lengths: np.ndarray
    alphabet: int
    sides: dict            # name -> Side


def plain_side(query, matrix=B62, alphabet=ALPHABET):
    query = np.ascontiguousarray(query, dtype=np.uint8)
    return Side(query, matrix, np.ascontiguousarray(matrix.reshape(alphabet, alphabet)[query]), alphabet)


def pssm_side(rng, length, alphabet=ALPHABET):
    classes, matrix, rows = _pssm.class_pssm(rng, length, alphabet)
    return Side(classes, matrix, rows, alphabet)


@functools.lru_cache(maxsize=None)
def world():
    """About 200 protein targets of 0-300 residues over 24 letters and one of 3000; two empty ones, a noisy copy of the
    longest query in one target, the 53-residue query twice in another."""
    rng = np.random.default_rng(20260)
    sides = {f"q{n}": plain_side(_data.random_protein(rng, n)) for n in (130, 65, 64, 53, 9, 7, 1)}
    sides["q30"] = plain_side(sides["q53"].query[:30])      # (found twice in TWICE_AT as well)
    for n in (65, 53, 9, 7):
        sides[f"p{n}"] = pssm_side(rng, n)
    lengths = rng.integers(1, 301, size=TARGETS)
    lengths[[0, 1, 2, 3, 41, 42, 43]] = [300, 1, 64, 65, 63, 9, 130]
    targets = [_data.random_protein(rng, int(n)) for n in lengths]
    for k in EMPTY:
        targets[k] = np.zeros(0, dtype=np.uint8)
    targets[LONG_AT] = _data.random_protein(rng, LONGEST)
    targets[NOISY_AT] = np.concatenate([_data.random_protein(rng, 60), _data.mutate(rng, sides["q130"].query),
                                        _data.random_protein(rng, 40)]).astype(np.uint8)
    q53 = sides["q53"].query
    targets[TWICE_AT] = np.concatenate([_data.random_protein(rng, 20), q53, _data.random_protein(rng, 15), q53,
                                        _data.random_protein(rng, 10)]).astype(np.uint8)
    residues, offsets = _oracle.flatten(targets)
    residues.setflags(write=False)
    offsets.setflags(write=False)
    return World(residues, offsets, targets, np.diff(offsets), ALPHABET, sides)


@functools.lru_cache(maxsize=None)
def world32():
    """The 32-letter database of the PSSM aligned panel: 130 targets of 1-60 residues, and 12 PSSMs of 64 rows whose
    rows are rows of one matrix - 768 rows, more than the table of the alignment stage holds, so the stage runs in two
    runs - which makes the panel of their classes under that matrix the same search."""
    rng = np.random.default_rng(320)
    alphabet = 32
    lengths = rng.integers(1, 61, size=130)
    residues, offsets = _pssm.random_db(rng, lengths, alphabet)
    targets = [residues[offsets[k]:offsets[k + 1]] for k in range(len(lengths))]
    matrix = np.ascontiguousarray(rng.integers(-8, 13, size=alphabet * alphabet).astype(np.int32))
    sides = {f"m{i}": plain_side(rng.integers(0, alphabet, size=64).astype(np.uint8), matrix, alphabet) for i in range(12)}
    return World(residues, offsets, targets, np.diff(offsets), alphabet, sides)


def side(name, w=None):
    return (w or world()).sides[name]


def bounds(span, w=None):
    w = w or world()
    return (0, len(w.lengths)) if span is None else span


# ---- the witnesses, each computed once ---------------------------------------------------------------------------------

def frozen(arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _which(w):
    return world32() if w == 32 else world()


@functools.lru_cache(maxsize=None)
def checker(name, mode, algorithm, span=None, w=24):
    """`_oracle.search` of the side ``name`` on the slice ``span``; the alignments of "full" as "aln_flat" / "aln_off"
    beside the list "aln" """
    W = _which(w)
    lo, hi = bounds(span, W)
    s = side(name, W)
    residues = W.residues[W.offsets[lo]:W.offsets[hi]]
    want = _oracle.search(s.query, residues if len(residues) else np.zeros(1, dtype=np.uint8), W.offsets[lo:hi + 1] - W.offsets[lo],
                          s.matrix, GAPS[0], GAPS[1], mode, algorithm)
    if mode == "full":
        want["aln_off"] = np.concatenate([[0], np.cumsum([len(a) for a in want["aln"]])]).astype(np.int64)
        want["aln_flat"] = np.concatenate(want["aln"]).astype(np.uint8) if want["aln_off"][-1] else np.zeros(0, dtype=np.uint8)
    return frozen(want)


def flat_answer(want):
    return {key: value for key, value in want.items() if key != "aln"}


def cut_of(scores):
    """the middle one of the distinct scores: some entry is at or above it, and not every one"""
    scores = np.asarray(scores).ravel()
    distinct = np.unique(scores)
    assert len(distinct) >= 2
    cut = int(distinct[len(distinct) // 2])
    assert 0 < np.count_nonzero(scores >= cut) < len(scores)
    return cut


def best_first(scores):
    """indices ordered by score descending, index ascending"""
    scores = np.asarray(scores, dtype=np.int64)
    return np.lexsort((np.arange(len(scores)), -scores))


def pairs_answer(names, pair_query, pair_target, algorithm):
    """what a `full` pair list answers, from the checker's `full` search of every query on the whole database"""
    full = [checker(name, "full", algorithm) for name in names]
    out = {key: np.array([full[q][key][t] for q, t in zip(pair_query, pair_target)], dtype=np.int32)
           for key in ("score", "end_t", "end_q", "start_t", "start_q")}
    ops = [full[q]["aln"][t] for q, t in zip(pair_query, pair_target)]
    out["aln_off"] = np.concatenate([[0], np.cumsum([len(a) for a in ops])]).astype(np.int64)
    out["aln_flat"] = np.concatenate(ops).astype(np.uint8) if out["aln_off"][-1] else np.zeros(0, dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def column_witness(name, algorithm, w=24):
    """`_occurrences.flat_columns` of every target of the database: `column_values` for the targets of up to 300
    residues, `row_values` for the long one"""
    W = _which(w)
    s = side(name, W)
    short = [t if len(t) <= 300 else t[:0] for t in W.targets]
    V, R = _occurrences.column_values(s.rows, short, GAPS[0], GAPS[1], algorithm)
    values = [V[k, :len(t)] for k, t in enumerate(short)]
    rows = [R[k, :len(t)] for k, t in enumerate(short)]
    for k, t in enumerate(W.targets):
        if len(t) > 300:
            values[k], rows[k] = _occurrences.row_values(s.rows, t, GAPS[0], GAPS[1], algorithm)
    return _occurrences.flat_columns(values, rows)


def occurrence_cut(name, algorithm, span, w=24):
    """a cut from the checker's scores of the slice: about half of its targets hold an occurrence"""
    cut = cut_of(checker(name, "score", algorithm, span, w)["score"])
    return max(cut, 1) if algorithm == "sw" else cut


def occurrences_answer(name, algorithm, span, cut, aligned=False, w=24):
    """the arrays of an occurrence search of one query (window: its length), with ``aligned`` the starts and operations"""
    W = _which(w)
    lo, hi = bounds(span, W)
    s = side(name, W)
    V, R, offsets = column_witness(name, algorithm, w)
    out = _occurrences.expected_flat(V, R, offsets, cut, len(s.query), lo, hi)
    if aligned:
        occ = np.stack([out[key].astype(np.int64) for key in ("target", "score", "end_t", "end_q")], axis=1)
        start_t, start_q = _occurrence_alignments.starts(s.rows, W.targets, occ, GAPS[0], GAPS[1], algorithm)
        ops = _occurrence_alignments.operations(s.query, s.matrix, W.targets, occ, start_t, start_q, GAPS[0], GAPS[1])
        out.update(start_t=start_t, start_q=start_q,
                   aln_off=np.concatenate([[0], np.cumsum([len(a) for a in ops])]).astype(np.int64),
                   aln_flat=np.concatenate(ops).astype(np.uint8) if len(ops) else np.zeros(0, dtype=np.uint8))
    return out


def single_occurrences(name, algorithm, span, aligned=False, w=24):
    out = occurrences_answer(name, algorithm, span, occurrence_cut(name, algorithm, span, w), aligned, w)
    return dict(count=np.array([len(out["target"])], dtype=np.int64), **out)


def panel_occurrences(names, algorithm, span, aligned=False, w=24):
    """the CSR of a panel: the single answers laid end to end, the operation offsets rebased"""
    parts = [occurrences_answer(n, algorithm, span, occurrence_cut(n, algorithm, span, w), aligned, w) for n in names]
    out = {"offsets": np.concatenate([[0], np.cumsum([len(p["target"]) for p in parts])]).astype(np.int64)}
    for key in parts[0]:
        if key != "aln_off":
            out[key] = np.concatenate([p[key] for p in parts])
    if aligned:
        out["aln_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p["aln_off"]) for p in parts]))]).astype(np.int64)
    return out


# ---- answers as arrays ------------------------------------------------------------------------------------------------

def arrays_of(out):
    """the arrays of an entry point's dict: integers as int64[1], a fit as its bytes; the list view of the alignments
    ("aln"), owners of buffers and None are left out"""
    arrays = {}
    for key, value in out.items():
        if key == "aln" or key.startswith("_") or value is None:
            continue
        if isinstance(value, _capi.ScoreFit):
            value = np.frombuffer(bytes(value), dtype=np.uint8)
        elif isinstance(value, (int, np.integer)):
            value = np.array([value], dtype=np.int64)
        assert isinstance(value, np.ndarray), (key, type(value))
        arrays[key] = value
    return arrays


def text(message):
    return np.frombuffer(str(message).encode(), dtype=np.uint8)


def differences(got, want):
    """[] when the answer ``got`` equals ``want`` in keys, dtypes, shapes and bytes; else what differs"""
    out = []
    if sorted(got) != sorted(want):
        return [f"keys {sorted(got)} instead of {sorted(want)}"]
    for key in want:
        g, e = got[key], want[key]
        if g.dtype != e.dtype or g.shape != e.shape:
            out.append(f"{key}: {g.dtype}{g.shape} instead of {e.dtype}{e.shape}")
        elif np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(e).tobytes():
            at = np.flatnonzero(g.ravel() != e.ravel())
            out.append(f"{key}: {len(at)} of {g.size} entries differ, first at {at[:5].tolist()}: "
                       f"{g.ravel()[at[:5]].tolist()} instead of {e.ravel()[at[:5]].tolist()}")
    return out


# ---- the nodes --------------------------------------------------------------------------------------------------------

class Node(typing.NamedTuple):
    name: str
    family: str                   # the entry point
    form: str                     # "large", "small" or "" (a family with one form)
    query_length: int             # the longest query of the call
    span: typing.Optional[tuple]  # the slice of the call (None: every target)
    run: typing.Callable          # (db) -> dict of numpy arrays
    expected: typing.Callable     # () -> dict of numpy arrays; of a significance search: (a fresh handle's answer) -> ...
    fails: bool = False           # the call fails by design: the answer is its error
    fresh: bool = False           # `expected` takes the answer of the same call on a fresh handle


def cached(function):
    return functools.lru_cache(maxsize=None)(function)


def _search(name, mode, algorithm, span=None):
    lo, hi = bounds(span)
    s = side(name)
    run = lambda db: arrays_of(db.search(s.query, B62, *GAPS, mode, algorithm, lo, hi))   # noqa: E731
    return run, cached(lambda: flat_answer(checker(name, mode, algorithm, span)))


def _search_pssm(name, mode, algorithm, span=None):
    lo, hi = bounds(span)
    s = side(name)
    run = lambda db: arrays_of(db.search_pssm(s.rows, s.query, *GAPS, mode, algorithm, lo, hi))   # noqa: E731
    return run, cached(lambda: flat_answer(checker(name, mode, algorithm, span)))


def _search_batch(names, mode, algorithm, span=None):
    lo, hi = bounds(span)
    queries = [side(n).query for n in names]
    run = lambda db: arrays_of(db.search_batch(queries, B62, *GAPS, mode, algorithm, lo, hi))   # noqa: E731

    def expected():
        rows = [checker(n, mode, algorithm, span) for n in names]
        return {key: np.stack([r[key] for r in rows]) for key in rows[0]}
    return run, cached(expected)


def _top_cut(name, algorithm, span, bounded):
    """(k, min_score) of a top search. ``bounded``: a bound on the score and a k past the targets that reach it, so that
    the tail of the answer is the -1 padding; else the better half of those at or above the middle score"""
    scores = checker(name, "score", algorithm, span)["score"]
    cut = cut_of(scores)
    above = int(np.count_nonzero(scores >= cut))
    return (above + 5, cut) if bounded else (max(1, above // 2), None)


def _search_top_full(name, algorithm, span, bounded):
    """The "full" form of a top search as the Python layer makes it: the selection on the scores, then the chosen
    targets aligned in one pair list - two entry points in one node."""
    lo, hi = bounds(span)
    s = side(name)
    k, min_score = _top_cut(name, algorithm, span, bounded)

    def run(db):
        top = db.search_top(s.query, B62, *GAPS, "score", algorithm, lo, hi, k=k, min_score=min_score)
        chosen = top["target"][:top["count"]]
        pairs = db.align_pairs([s.query], np.zeros(len(chosen), dtype=np.int32), chosen, B62, *GAPS, "full", algorithm)
        out = arrays_of(top)
        out.update({"pair_" + key: value for key, value in arrays_of(pairs).items()})
        return out

    def expected():
        scores = checker(name, "score", algorithm, span)["score"]
        order = best_first(scores)
        order = order[:k] if min_score is None else order[scores[order] >= min_score][:k]
        out = {"count": np.array([len(order)], dtype=np.int64), "target": np.full(k, -1, dtype=np.int64),
               "score": np.full(k, -1, dtype=np.int32)}
        out["target"][:len(order)] = lo + order
        out["score"][:len(order)] = scores[order]
        pairs = pairs_answer([name], [0] * len(order), (lo + order).tolist(), algorithm)
        out.update({"pair_" + key: value for key, value in pairs.items()})
        return out
    return run, cached(expected)


def _search_batch_top(names, mode, algorithm, span=None):
    lo, hi = bounds(span)
    queries = [side(n).query for n in names]
    scores = lambda: np.stack([checker(n, mode, algorithm, span)["score"] for n in names])   # noqa: E731
    # one bound on the score for all queries, and a k past the most targets that reach it: every row ends in -1 padding
    rule = cached(lambda: (cut_of(scores()), int((scores() >= cut_of(scores())).sum(axis=1).max()) + 2))

    def run(db):
        min_score, k = rule()
        return arrays_of(db.search_batch_top(queries, B62, *GAPS, mode, algorithm, lo, hi, k=k, min_score=min_score))

    def expected():
        min_score, k = rule()
        out = {"count": np.zeros(len(names), dtype=np.int32), "target": np.full((len(names), k), -1, dtype=np.int64)}
        keys = ("score", "end_t", "end_q") if mode == "end" else ("score",)
        out.update({key: np.full((len(names), k), -1, dtype=np.int32) for key in keys})
        for i, n in enumerate(names):
            row = checker(n, mode, algorithm, span)
            order = best_first(row["score"])
            order = order[row["score"][order] >= min_score][:k]
            out["count"][i] = len(order)
            out["target"][i, :len(order)] = lo + order
            for key in keys:
                out[key][i, :len(order)] = row[key][order]
        assert 0 < out["count"].sum() and out["count"].max() < k
        return out
    return run, cached(expected)


def _search_hits_sorted(name, mode, algorithm, span=None):
    """`search_hits` with the hits put best first, as the Python layer's ``sort=True`` does on the host"""
    lo, hi = bounds(span)
    s = side(name)
    cut = cached(lambda: cut_of(checker(name, "score", algorithm, span)["score"]))

    def run(db):
        out = arrays_of(db.search_hits(s.query, B62, *GAPS, mode, algorithm, lo, hi, min_score=cut()))
        order = np.lexsort((out["target"], -out["score"].astype(np.int64)))
        return {key: value if key == "count" else value[order] for key, value in out.items()}

    def expected():
        row = checker(name, mode, algorithm, span)
        order = best_first(row["score"])
        order = order[row["score"][order] >= cut()]
        out = {"count": np.array([len(order)], dtype=np.int64), "target": (lo + order).astype(np.int64)}
        out.update({key: row[key][order] for key in row})
        return out
    return run, cached(expected)


def _search_batch_hits(names, mode, algorithm, span=None):
    lo, hi = bounds(span)
    queries = [side(n).query for n in names]
    cuts = cached(lambda: [cut_of(checker(n, "score", algorithm, span)["score"]) for n in names])
    run = lambda db: arrays_of(db.search_batch_hits(queries, B62, *GAPS, mode, algorithm, lo, hi, min_score=cuts()))   # noqa: E731

    def expected():
        rows = [checker(n, mode, algorithm, span) for n in names]
        found = [np.flatnonzero(r["score"] >= c) for r, c in zip(rows, cuts())]
        out = {"offsets": np.concatenate([[0], np.cumsum([len(f) for f in found])]).astype(np.int64),
               "target": np.concatenate(found).astype(np.int64) + lo}
        out.update({key: np.concatenate([r[key][f] for r, f in zip(rows, found)]) for key in rows[0]})
        return out
    return run, cached(expected)


def _search_significant(name, algorithm, span=None):
    lo, hi = bounds(span)
    s = side(name)
    run = lambda db: arrays_of(db.search_significant(s.query, B62, *GAPS, "score", algorithm, lo, hi, max_evalue=MAX_EVALUE))   # noqa: E731

    def expected(fresh):
        """``fresh``: the answer of `run` on a fresh handle - the fit is its fit, field for field, and the E-values are
        its E-values; the hits are the targets at or above the fit's thresholds on the checker's scores"""
        fit = _capi.ScoreFit.from_buffer_copy(fresh["fit"].tobytes())
        thresholds = np.array(fit.threshold, dtype=np.int64)[_capi.length_bins(world().lengths[lo:hi])]
        scores = checker(name, "score", algorithm, span)["score"]
        chosen = np.flatnonzero(scores >= thresholds)
        return {"count": np.array([len(chosen)], dtype=np.int64), "target": (lo + chosen).astype(np.int64),
                "score": scores[chosen], "evalue": fresh["evalue"], "fit": fresh["fit"]}
    return run, expected


def _search_batch_target_top(names, mode, algorithm, m, span=None):
    lo, hi = bounds(span)
    queries = [side(n).query for n in names]
    floor = cached(lambda: cut_of(np.stack([checker(n, "score", algorithm, span)["score"] for n in names])))
    run = lambda db: arrays_of(db.search_batch_target_top(queries, B62, *GAPS, mode, algorithm, lo, hi, m=m, min_score=floor()))   # noqa: E731

    def expected():
        rows = [checker(n, mode, algorithm, span) for n in names]
        score = np.stack([r["score"] for r in rows]).astype(np.int64)      # [query][target]
        n = score.shape[1]
        out = {"count": np.zeros(n, dtype=np.int32), "query": np.full((n, m), -1, dtype=np.int32)}
        keys = ("score", "end_t", "end_q") if mode == "end" else ("score",)
        out.update({key: np.full((n, m), -1, dtype=np.int32) for key in keys})
        for t in range(n):
            ranked = [i for i in best_first(score[:, t]).tolist() if score[i, t] >= floor()][:m]
            out["count"][t] = len(ranked)
            out["query"][t, :len(ranked)] = ranked
            for key in keys:
                out[key][t, :len(ranked)] = [rows[i][key][t] for i in ranked]
        assert 0 < out["count"].sum() < n * m
        return out
    return run, cached(expected)


def _pair_list(seed, pairs, names, span, always=()):
    """``pairs`` (query, target) pairs with repeats, the targets from the slice; ``always``: targets that occur"""
    lo, hi = bounds(span)
    rng = np.random.default_rng(seed)
    pair_target = rng.integers(lo, hi, size=pairs)
    pair_target[:len(always)] = always
    pair_target[pairs // 2:] = pair_target[:pairs - pairs // 2][::-1]        # every pair of the first half once more
    pair_query = rng.integers(0, len(names), size=pairs)
    return pair_query.astype(np.int32), pair_target.astype(np.int64)


def _align_pairs(names, algorithm, seed, pairs, span=None, always=()):
    pair_query, pair_target = _pair_list(seed, pairs, names, span, always)
    queries = [side(n).query for n in names]
    run = lambda db: arrays_of(db.align_pairs(queries, pair_query, pair_target, B62, *GAPS, "full", algorithm))   # noqa: E731
    return run, cached(lambda: pairs_answer(names, pair_query.tolist(), pair_target.tolist(), algorithm))


def _align_pairs_pssm(names, algorithm, seed, pairs, span=None, always=()):
    pair_query, pair_target = _pair_list(seed, pairs, names, span, always)
    rows, consensus = [side(n).rows for n in names], [side(n).query for n in names]
    run = lambda db: arrays_of(db.align_pairs_pssm(rows, consensus, pair_query, pair_target, *GAPS, "full", algorithm))   # noqa: E731
    return run, cached(lambda: pairs_answer(names, pair_query.tolist(), pair_target.tolist(), algorithm))


def _profile_columns(name, algorithm, seed, members, span=None, always=()):
    _, members_of = _pair_list(seed, members, [name], span, always)
    s = side(name)
    run = lambda db: arrays_of(db.profile_columns(s.query, B62, members_of, *GAPS, algorithm, return_msa=True))   # noqa: E731

    def expected():
        w = world()
        full = checker(name, "full", algorithm)
        rows = [_profile.project(full["aln"][t], full["start_q"][t], full["start_t"][t], w.targets[t], len(s.query), ALPHABET)
                for t in members_of.tolist()]
        msa = np.vstack([s.query[None, :]] + [r[None, :] for r in rows]).astype(np.uint8)
        counts, _, _, weights, weighted = _profile.columns(msa, ALPHABET)
        return {"counts": counts, "weighted": weighted, "member_weights": weights, "msa": msa}
    return run, cached(expected)


def _occurrences_one(name, algorithm, span=None, pssm=False, aligned=False):
    lo, hi = bounds(span)
    s = side(name)
    cut = cached(lambda: occurrence_cut(name, algorithm, span))

    def run(db):
        if pssm and aligned:
            out = db.search_occurrence_alignments_pssm(s.rows, s.query, *GAPS, algorithm, lo, hi, min_score=cut())
        elif pssm:
            out = db.search_occurrences_pssm(s.rows, *GAPS, algorithm, lo, hi, min_score=cut())
        elif aligned:
            out = db.search_occurrence_alignments(s.query, B62, *GAPS, algorithm, lo, hi, min_score=cut())
        else:
            out = db.search_occurrences(s.query, B62, *GAPS, algorithm, lo, hi, min_score=cut())
        return arrays_of(out)
    return run, cached(lambda: single_occurrences(name, algorithm, span, aligned))


def _occurrences_panel(names, algorithm, span=None, pssm=False, aligned=False):
    lo, hi = bounds(span)
    sides = [side(n) for n in names]
    cuts = cached(lambda: [occurrence_cut(n, algorithm, span) for n in names])

    def run(db):
        if pssm:
            out = db.search_batch_occurrences_pssm([s.rows for s in sides], *GAPS, algorithm, lo, hi, min_score=cuts())
        elif aligned:
            out = db.search_batch_occurrence_alignments([s.query for s in sides], B62, *GAPS, algorithm, lo, hi, min_score=cuts())
        else:
            out = db.search_batch_occurrences([s.query for s in sides], B62, *GAPS, algorithm, lo, hi, min_score=cuts())
        return arrays_of(out)
    return run, cached(lambda: panel_occurrences(names, algorithm, span, aligned))


_streams = threading.local()


def _device_scores(name, algorithm, span=None):
    """`search_device_scores` into a tensor of the caller's on a stream of the caller's (one `torch.cuda.Stream` per
    thread, made at its first use), read back after synchronising that stream"""
    lo, hi = bounds(span)
    s = side(name)

    def run(db):
        import torch
        if not hasattr(_streams, "stream"):
            _streams.stream = torch.cuda.Stream(device=f"cuda:{db.device}")
        stream = _streams.stream
        # (-7 in every entry, by a copy from the host on that stream: a fill would be the first torch kernel of the
        # process, and loading torch's kernels takes seconds)
        out = torch.empty((hi - lo,), dtype=torch.int32, device=f"cuda:{db.device}")
        with torch.cuda.stream(stream):
            out.copy_(torch.full((hi - lo,), -7, dtype=torch.int32), non_blocking=True)
        db.search_device_scores(s.query, B62, out.data_ptr(), stream.cuda_stream, *GAPS, algorithm, lo, hi)
        stream.synchronize()
        return {"score": out.cpu().numpy()}
    return run, cached(lambda: {"score": checker(name, "score", algorithm, span)["score"]})


def _too_many_pssm_hits(name, algorithm, span=None):
    """`search_pssm_hits` with ``max_hits`` one below the count: TooManyHits, the answer is its ``counts``"""
    lo, hi = bounds(span)
    s = side(name)

    @cached
    def rule():
        scores = checker(name, "score", algorithm, span)["score"]
        return cut_of(scores), int(np.count_nonzero(scores >= cut_of(scores)))

    def run(db):
        cut, count = rule()
        try:
            db.search_pssm_hits(s.rows, *GAPS, "score", algorithm, lo, hi, min_score=cut, max_hits=count - 1)
        except _capi.TooManyHits as error:
            return {"counts": np.array([error.counts], dtype=np.int64)}
        raise AssertionError("search_pssm_hits with max_hits below the count did not raise TooManyHits")
    return run, cached(lambda: {"counts": np.array([rule()[1]], dtype=np.int64)})


def _pair_outside(names, algorithm):
    """`align_pairs` with a target index one past the end in pair 3: code 101, the message is the answer"""
    queries = [side(n).query for n in names]
    pair_query = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    pair_target = np.array([3, NOISY_AT, EMPTY[0], TARGETS, 11], dtype=np.int64)
    message = (f"failed to align to Opal database (code={BAD_ARGUMENT}): pair 3: target index {TARGETS} outside "
               f"[0, {TARGETS})")

    def run(db):
        try:
            db.align_pairs(queries, pair_query, pair_target, B62, *GAPS, "full", algorithm)
        except RuntimeError as error:
            return {"message": text(error)}
        raise AssertionError("align_pairs with a target index past the end did not fail")
    return run, cached(lambda: {"message": text(message)})


def _release():
    def run(db):
        db.release_workspaces()
        return {}
    return run, lambda: {}


def _nodes():
    PANEL = ("q1", "q9", "q64", "q130")
    table = [
        # name, family, form, longest query, slice, (run, expected)
        ("search score sw 53", "search", "large", 53, None, _search("q53", "score", "sw")),
        ("search end nw 130", "search", "", 130, None, _search("q130", "end", "nw")),
        ("search full sw 65", "search", "", 65, None, _search("q65", "full", "sw")),
        ("search full hw 9 small", "search", "small", 9, SMALL, _search("q9", "full", "hw", SMALL)),
        ("search score sw 53 long target", "search", "", 53, TAIL, _search("q53", "score", "sw", TAIL)),
        ("search_pssm full ov", "search_pssm", "large", 53, None, _search_pssm("p53", "full", "ov")),
        ("search_pssm full ov small", "search_pssm", "small", 9, SMALL, _search_pssm("p9", "full", "ov", SMALL)),
        ("search_batch end sw", "search_batch", "large", 65, None, _search_batch(("q53", "q65", "q9"), "end", "sw")),
        ("search_batch end sw small", "search_batch", "small", 9, SMALL, _search_batch(("q9", "q7"), "end", "sw", SMALL)),
        ("search_top full", "search_top", "large", 53, None, _search_top_full("q53", "sw", None, True)),
        ("search_top full small", "search_top", "small", 9, SMALL, _search_top_full("q9", "sw", SMALL, False)),
        ("search_batch_top", "search_batch_top", "large", 65, None, _search_batch_top(("q53", "q65", "q30"), "end", "sw")),
        ("search_batch_top small", "search_batch_top", "small", 9, SMALL, _search_batch_top(("q9", "q7"), "end", "sw", SMALL)),
        ("search_hits sorted", "search_hits", "large", 53, None, _search_hits_sorted("q53", "end", "sw")),
        ("search_hits sorted small", "search_hits", "small", 9, SMALL, _search_hits_sorted("q9", "end", "sw", SMALL)),
        ("search_batch_hits", "search_batch_hits", "large", 130, None, _search_batch_hits(("q53", "q130", "q9"), "score", "nw")),
        ("search_batch_hits small", "search_batch_hits", "small", 9, SMALL, _search_batch_hits(("q9", "q7"), "score", "nw", SMALL)),
        ("search_significant", "search_significant", "large", 53, None, _search_significant("q53", "sw")),
        ("search_significant small", "search_significant", "small", 30, (20, 180), _search_significant("q30", "sw", (20, 180))),
        ("search_batch_target_top", "search_batch_target_top", "large", 65, None,
         _search_batch_target_top(("q53", "q65", "q30", "q9"), "end", "sw", 2)),
        ("search_batch_target_top small", "search_batch_target_top", "small", 9, SMALL,
         _search_batch_target_top(("q9", "q7", "q1"), "end", "sw", 2, SMALL)),
        ("align_pairs full", "align_pairs", "large", 130, None,
         _align_pairs(("q130", "q53", "q9"), "sw", 1, 300, None, EMPTY + (LONG_AT, NOISY_AT, TWICE_AT))),
        ("align_pairs full small", "align_pairs", "small", 9, SMALL, _align_pairs(("q9", "q7"), "sw", 2, 40, SMALL, (EMPTY[1],))),
        ("align_pairs_pssm", "align_pairs_pssm", "large", 65, None,
         _align_pairs_pssm(("p65", "p53"), "nw", 3, 120, None, EMPTY + (LONG_AT,))),
        ("align_pairs_pssm small", "align_pairs_pssm", "small", 9, SMALL,
         _align_pairs_pssm(("p9", "p7"), "nw", 4, 30, SMALL, (EMPTY[1],))),
        ("profile_columns", "profile_columns", "large", 65, None,
         _profile_columns("q65", "sw", 5, 150, None, EMPTY + (LONG_AT, NOISY_AT))),
        ("profile_columns small", "profile_columns", "small", 9, SMALL, _profile_columns("q9", "sw", 6, 30, SMALL, (EMPTY[1],))),
        ("search_occurrences hw 130", "search_occurrences", "large", 130, None, _occurrences_one("q130", "hw")),
        ("search_occurrences hw 9 small", "search_occurrences", "small", 9, SMALL, _occurrences_one("q9", "hw", SMALL)),
        ("search_occurrences_pssm sw 65", "search_occurrences_pssm", "large", 65, None, _occurrences_one("p65", "sw", None, pssm=True)),
        ("search_occurrences_pssm sw 9 small", "search_occurrences_pssm", "small", 9, SMALL,
         _occurrences_one("p9", "sw", SMALL, pssm=True)),
        ("search_occurrence_alignments", "search_occurrence_alignments", "large", 53, SHORT,
         _occurrences_one("q53", "hw", SHORT, aligned=True)),
        ("search_occurrence_alignments small", "search_occurrence_alignments", "small", 9, SMALL,
         _occurrences_one("q9", "sw", SMALL, aligned=True)),
        ("search_batch_occurrences", "search_batch_occurrences", "large", 130, None, _occurrences_panel(PANEL, "hw")),
        ("search_batch_occurrences small", "search_batch_occurrences", "small", 9, SMALL, _occurrences_panel(("q1", "q9"), "hw", SMALL)),
        ("search_batch_occurrences_pssm", "search_batch_occurrences_pssm", "large", 65, None,
         _occurrences_panel(("p65", "p7", "p53"), "sw", None, pssm=True)),
        ("search_batch_occurrences_pssm small", "search_batch_occurrences_pssm", "small", 9, SMALL,
         _occurrences_panel(("p9", "p7"), "sw", SMALL, pssm=True)),
        ("search_batch_occurrence_alignments", "search_batch_occurrence_alignments", "large", 130, SHORT,
         _occurrences_panel(PANEL, "sw", SHORT, aligned=True)),
        ("search_batch_occurrence_alignments small", "search_batch_occurrence_alignments", "small", 9, SMALL,
         _occurrences_panel(("q9", "q7"), "hw", SMALL, aligned=True)),
        ("search_device_scores", "search_device_scores", "large", 53, None, _device_scores("q53", "sw")),
        ("search_device_scores small", "search_device_scores", "small", 9, SMALL, _device_scores("q9", "sw", SMALL)),
        ("search_pssm_hits too many", "search_pssm_hits", "", 53, None, _too_many_pssm_hits("p53", "sw")),
        ("align_pairs target outside", "align_pairs (fails)", "", 53, None, _pair_outside(("q53", "q9"), "sw")),
        ("release_workspaces", "release_workspaces", "", 0, None, _release()),
    ]
    nodes = []
    for name, family, form, q, span, (run, expected) in table:
        nodes.append(Node(name, family, form, q, span, run, expected, fails=name in FAILING, fresh=family == "search_significant"))
    assert len({n.name for n in nodes}) == len(nodes)
    return tuple(nodes)


FAILING = ("search_pssm_hits too many", "align_pairs target outside")
NODES = _nodes()
FULL_NODES = ("search full sw 65", "search_pssm full ov", "align_pairs full", "profile_columns")   # `full`-mode work


def node(name):
    return next(n for n in NODES if n.name == name)


# ---- the 32-letter handle: the PSSM aligned panel with its single-PSSM and plain-panel forms --------------------------

def _nodes32():
    w = world32()
    names = tuple(f"m{i}" for i in range(12))
    sides = [w.sides[n] for n in names]
    cuts = cached(lambda: [occurrence_cut(n, "hw", None, 32) for n in names])

    def panel_pssm(db):
        return arrays_of(db.search_batch_occurrence_alignments_pssm([s.rows for s in sides], [s.query for s in sides], *GAPS, "hw",
                                                                    min_score=cuts()))

    def single_pssm(db):
        return arrays_of(db.search_occurrence_alignments_pssm(sides[3].rows, sides[3].query, *GAPS, "hw", min_score=cuts()[3]))

    def panel_plain(db):
        return arrays_of(db.search_batch_occurrence_alignments([s.query for s in sides[:4]], sides[0].matrix, *GAPS, "hw",
                                                               min_score=cuts()[:4]))
    return (
        Node("search_batch_occurrence_alignments_pssm", "search_batch_occurrence_alignments_pssm", "", 64, None, panel_pssm,
             cached(lambda: panel_occurrences(names, "hw", None, True, 32))),
        Node("search_occurrence_alignments_pssm", "search_occurrence_alignments_pssm", "", 64, None, single_pssm,
             cached(lambda: single_occurrences("m3", "hw", None, True, 32))),
        Node("search_batch_occurrence_alignments 32", "search_batch_occurrence_alignments", "", 64, None, panel_plain,
             cached(lambda: panel_occurrences(names[:4], "hw", None, True, 32))),
    )


NODES32 = _nodes32()


# ---- the orders --------------------------------------------------------------------------------------------------------

def circuit(n):
    """An Eulerian circuit of the complete directed graph with loops on n nodes (Hierholzer): n * n + 1 entries, every
    ordered pair consecutive exactly once; it begins and ends with node 0."""
    unused = [list(range(n)) for _ in range(n)]      # the successors of every node not yet taken
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


def segments(order, length):
    """``order`` cut into runs of ``length`` pairs (the last one of what is left); each run begins with the last node of
    the run before"""
    assert length >= 1
    return [order[at:at + length + 1] for at in range(0, len(order) - 1, length)]


def pairs_of(run):
    return list(zip(run[:-1], run[1:]))
