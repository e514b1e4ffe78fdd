"""Every occurrence of a query in each target, with where it starts and how it aligns (include/miopal.h,
miopalSearchOccurrences and miopalSearchOccurrencesAligned): the adapter a read carries twice, the binding sites of a
primer, the copies of a repeated domain - cut out from start to end.

Free functions that take an `Aligner`, not methods of it: the set of `Aligner`'s public methods is the reference's
plus a fixed table of extensions.

    sites = find_occurrences(aligner, "ETSEEES", database, 25)          # FullResult, several per target
    ends = find_occurrences(aligner, "ETSEEES", database, 25, mode="end")

    panel = find_occurrences_many(aligner, barcodes, database, 25)        # one list of EndResult per query
    trims = find_occurrence_alignments_many(aligner, barcodes, database, 25)   # ... of FullResult per query

``mode="end"`` is served by the occurrence search alone (EndResult: score and end cell); ``mode="full"`` by the aligned
form, whose start cells follow the checker's rule applied to each occurrence's end cell, and whose operations are the
global alignment of the rectangle between start and end.
"""
import typing

import numpy as np

from . import _capi
from .lib import (UINT32_MAX, Aligner, BaseDatabase, Pssm, ScoreResult, _empty_arrays, _max_hits_argument, _Profiles,
                  _QuerySide, _Request, _result_objects, _Sequences, _target_lengths)

_MODES = ("end", "full")
_ALGORITHMS = ("hw", "sw")


def _rule(mode, algorithm, min_score, window) -> None:
    """the faults of an occurrence request that need neither a database nor a device"""
    if mode not in _MODES:
        raise ValueError(f"occurrences are reported with mode 'end' or 'full', not {mode!r}")
    if algorithm not in _ALGORITHMS:
        raise ValueError(f"occurrences are defined for the algorithms 'hw' and 'sw', not {algorithm!r}")
    if isinstance(min_score, bool) or not isinstance(min_score, (int, np.integer)):
        raise TypeError(f"min_score must be an integer, not {type(min_score).__name__}")
    if not -(2 ** 31) <= int(min_score) < 2 ** 31:
        raise OverflowError("min_score does not fit a 32-bit integer")
    if window is not None:
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
            raise TypeError(f"window must be an integer or None, not {type(window).__name__}")
        if window < 0:
            raise ValueError("window must not be negative")
        if window >= 2 ** 31:
            raise OverflowError("window does not fit a 32-bit integer")
    if algorithm == "sw" and min_score < 1:
        raise ValueError("min_score must be at least 1 with algorithm 'sw'")


def _arrays(side: _QuerySide, database, min_score, window, algorithm, mode, start, end, device, max_hits):
    """(the arrays of the request, the target lengths or None): the device call behind `_Request`'s preamble"""
    side.check_type()
    _rule(mode, algorithm, min_score, window)
    request = _Request(side, database, mode, algorithm, start, end, device, lambda: _max_hits_argument(max_hits))
    max_hits = request.checked
    with request:
        if request.end == start or side.lengths[0] == 0:
            # (nothing to search, or nothing to search with: answered without a device)
            return dict(_empty_arrays(mode), count=0, target=np.zeros(0, dtype=np.int64)), None
        mirror = request.mirror()
        a = side.aligner
        rule = dict(algorithm=algorithm, start=start, end=request.end, min_score=int(min_score),
                    window=None if window is None else int(window), max_hits=max_hits)
        if isinstance(side, _Profiles):
            pssm = side.pssms[0]
            if mode == "end":
                out = mirror.search_occurrences_pssm(pssm.scores, a.gap_open, a.gap_extend, **rule)
            else:
                out = mirror.search_occurrence_alignments_pssm(pssm.scores, pssm.consensus, a.gap_open, a.gap_extend, **rule)
        elif mode == "end":
            out = mirror.search_occurrences(side.codes, a._matrix, a.gap_open, a.gap_extend, **rule)
        else:
            out = mirror.search_occurrence_alignments(side.codes, a._matrix, a.gap_open, a.gap_extend, **rule)
        out.pop("aln", None)
        return out, _target_lengths(mirror, mode)


def _objects(side, arrays, target_lengths, mode) -> typing.List[ScoreResult]:
    owner = np.zeros(len(arrays["target"]), dtype=np.int64)
    return _result_objects(mode, arrays["target"], owner, side.lengths, target_lengths, arrays)


def find_occurrences(aligner: Aligner, query, database: BaseDatabase, min_score: int, *,
                     window: typing.Optional[int] = None, algorithm: str = "hw", mode: str = "full", start: int = 0,
                     end: int = UINT32_MAX, device: int = 0,
                     max_hits: typing.Optional[int] = None) -> typing.List[ScoreResult]:
    """Every occurrence of ``query`` in each target of ``database[start:end]``: the columns where the last row of "hw"
    (the column maximum of "sw") reaches ``min_score``, thinned so that two occurrences of one target end more than
    ``window`` columns apart (None: the query's length; 0: every such column). One result per occurrence, by target
    index, then end column; a target may appear several times. ``mode="end"``: `EndResult`; ``mode="full"``:
    `FullResult` with the occurrence's start and alignment. With more than ``max_hits`` occurrences:
    `_capi.TooManyHits` (its ``counts`` their number), before any alignment work. A mode other than "end" and "full",
    an algorithm other than "hw" and "sw", a negative window and ``min_score < 1`` with "sw" raise before any device
    call; an empty slice or an empty query is answered without a device."""
    side = _Sequences(aligner, query, False)
    arrays, lengths = _arrays(side, database, min_score, window, algorithm, mode, start, end, device, max_hits)
    return _objects(side, arrays, lengths, mode)


def find_occurrences_pssm(aligner: Aligner, pssm: Pssm, database: BaseDatabase, min_score: int, *,
                          window: typing.Optional[int] = None, algorithm: str = "hw", mode: str = "full",
                          start: int = 0, end: int = UINT32_MAX, device: int = 0,
                          max_hits: typing.Optional[int] = None) -> typing.List[ScoreResult]:
    """`find_occurrences` with a `Pssm` in the place of the query and the aligner's matrix; the aligner gives the gap
    penalties, the PSSM's consensus tells matches from mismatches in the alignments."""
    side = _Profiles(aligner, pssm, False)
    arrays, lengths = _arrays(side, database, min_score, window, algorithm, mode, start, end, device, max_hits)
    return _objects(side, arrays, lengths, mode)


def find_occurrences_arrays(aligner: Aligner, query, database: BaseDatabase, min_score: int, *,
                            window: typing.Optional[int] = None, algorithm: str = "hw", mode: str = "full",
                            start: int = 0, end: int = UINT32_MAX, device: int = 0,
                            max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
    """`find_occurrences` without result objects: "count", "target" (int64), "score", "end_q" / "end_t" and, for
    "full", "start_q" / "start_t", "aln_flat" / "aln_off" - one entry per occurrence."""
    side = _Sequences(aligner, query, False)
    return _arrays(side, database, min_score, window, algorithm, mode, start, end, device, max_hits)[0]


# --- a panel of queries in one call (miopalSearchBatchOccurrences) ----------------------------------------------------

def _panel_values(values, name, none_allowed):
    """one cut or window, or one per query, as a list (their number is checked once the queries are known)"""
    many = not (values is None or isinstance(values, (int, np.integer, bool)))
    items = list(values) if many else [values]
    for v in items:
        if v is None and none_allowed:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            what = "an integer or None" if none_allowed else "an integer"
            raise TypeError(f"{name} must be {what}, or one per query, not {type(v).__name__}")
    return items, many


def _panel_arrays(aligner, queries, database, min_score, window, algorithm, mode, start, end, device, max_hits,
                  operations=None, pssm=False):
    """(the CSR of the request, the query side, the target lengths or None). ``operations`` None: the panel search
    (`find_occurrences_many`, mode "end"); a bool: the aligned form, with or without the operations. ``pssm``: the
    panel is a list of `Pssm` (the `..._pssm_many` functions)."""
    many, aligned = ("find_occurrences_pssm_many", "find_occurrence_alignments_pssm_many") if pssm else \
                    ("find_occurrences_many", "find_occurrence_alignments_many")
    if mode not in _MODES:
        raise ValueError(f"occurrences are reported with mode 'end' or 'full', not {mode!r}")
    if mode == "full" and operations is None:
        raise ValueError(f"the alignments of a panel's occurrences are not available yet from {many}, "
                         f"which reports mode 'end': {aligned} aligns a panel's occurrences")
    cuts, many_cuts = _panel_values(min_score, "min_score", False)
    windows, many_windows = _panel_values(window, "window", True)
    for cut in cuts or [1]:
        _rule(mode, algorithm, cut, None)
    for w in windows:
        _rule(mode, algorithm, 1, w)
    side = (_Profiles if pssm else _Sequences)(aligner, queries, True)
    request = _Request(side, database, mode, algorithm, start, end, device, lambda: _max_hits_argument(max_hits))
    for items, many, name in ((cuts, many_cuts, "min_score"), (windows, many_windows, "window")):
        if many and len(items) != len(side.lengths):
            raise ValueError(f"{name} must be one value or one per query ({len(side.lengths)}), got {len(items)}")
    rows = len(side.lengths)
    with request:
        if request.end == start or rows == 0 or max(side.lengths) == 0:
            # (nothing to search, or nothing to search with: answered without a device)
            out = dict(_empty_arrays(mode), offsets=np.zeros(rows + 1, dtype=np.int64), target=np.zeros(0, dtype=np.int64))
            if operations is False:
                del out["aln_flat"], out["aln_off"]
            return out, side, None
        mirror = request.mirror()
        rule = (aligner.gap_open, aligner.gap_extend, algorithm, start, request.end,
                cuts if many_cuts else cuts[0], windows if many_windows else windows[0], request.checked)
        if operations is None:
            ends = mirror.search_batch_occurrences_pssm if pssm else mirror.search_batch_occurrences
            return ends(side.arrays, *(() if pssm else (aligner._matrix,)), *rule), side, None
        if pssm:
            out = mirror.search_batch_occurrence_alignments_pssm(side.arrays, [p.consensus for p in side.pssms], *rule,
                                                                 operations)
        else:
            out = mirror.search_batch_occurrence_alignments(side.arrays, aligner._matrix, *rule, operations)
        out.pop("aln", None)
        return out, side, _target_lengths(mirror, mode)


def _panel_lists(mode, panel) -> typing.List[typing.List[ScoreResult]]:
    """one list of result objects per query from what `_panel_arrays` returned: "end" without an owner, "full" with
    each occurrence's query as its owner and the lengths of both sides"""
    out, side, target_lengths = panel
    offsets = out["offsets"]
    if mode == "end":
        flat = _result_objects(mode, out["target"], None, None, None, out)
    else:
        owner = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
        flat = _result_objects(mode, out["target"], owner, side.lengths, target_lengths, out)
    offsets = offsets.tolist()
    return [flat[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def find_occurrences_many(aligner: Aligner, queries, database: BaseDatabase, min_score, *, window=None,
                          algorithm: str = "hw", mode: str = "end", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                          max_hits: typing.Optional[int] = None) -> typing.List[typing.List[ScoreResult]]:
    """`find_occurrences` for a whole panel of queries - barcodes, primers, a kit's adapters - in one device call: a
    list with one list of `EndResult` per query, each what ``find_occurrences(aligner, query, ..., mode="end")``
    returns for that query. ``min_score`` and ``window``: one value or one per query (a window of None: that query's
    length). ``max_hits`` bounds the total over all queries; `_capi.TooManyHits` carries the CSR offsets in
    ``counts``. ``mode="full"`` raises ValueError - the alignments of a panel's occurrences are not available yet
    under this name: `find_occurrence_alignments_many` returns them. That and the other rule faults raise before any
    device call; an empty panel or slice is answered without a device."""
    return _panel_lists(mode, _panel_arrays(aligner, queries, database, min_score, window, algorithm, mode, start, end, device,
                                            max_hits))


def find_occurrences_many_arrays(aligner: Aligner, queries, database: BaseDatabase, min_score, *, window=None,
                                 algorithm: str = "hw", mode: str = "end", start: int = 0, end: int = UINT32_MAX,
                                 device: int = 0, max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
    """`find_occurrences_many` without result objects: a CSR - "offsets" (one entry per query plus one), "target"
    (int64), "score", "end_q" and "end_t"; entries offsets[i]:offsets[i + 1] belong to query i."""
    return _panel_arrays(aligner, queries, database, min_score, window, algorithm, mode, start, end, device, max_hits)[0]


# --- ... with where every occurrence starts and how it aligns (miopalSearchBatchOccurrencesAligned) ------------------
# (names of their own: find_occurrences_many(..., mode="full") keeps raising, which its tests pin)

def find_occurrence_alignments_many(aligner: Aligner, queries, database: BaseDatabase, min_score, *, window=None,
                                    algorithm: str = "hw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                                    max_hits: typing.Optional[int] = None) -> typing.List[typing.List[ScoreResult]]:
    """`find_occurrences(..., mode="full")` for a whole panel of queries in one device call: a list with one list of
    `FullResult` per query, each what ``find_occurrences(aligner, query, ..., mode="full")`` returns for that query -
    the occurrence's start, so that a read is trimmed at ``target_start``, and its alignment. ``min_score``,
    ``window`` and ``max_hits`` as in `find_occurrences_many`; once the total passes ``max_hits`` nothing more is
    aligned and `_capi.TooManyHits` carries the CSR offsets. The rule's faults raise before any device call; an empty
    panel or slice is answered without a device."""
    return _panel_lists("full", _panel_arrays(aligner, queries, database, min_score, window, algorithm, "full", start, end,
                                              device, max_hits, True))


def find_occurrence_alignments_many_arrays(aligner: Aligner, queries, database: BaseDatabase, min_score, *, window=None,
                                           algorithm: str = "hw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                                           max_hits: typing.Optional[int] = None,
                                           operations: bool = True) -> typing.Dict[str, typing.Any]:
    """`find_occurrence_alignments_many` without result objects: `find_occurrences_many_arrays`' CSR plus "start_q" /
    "start_t" and, with ``operations``, "aln_flat" / "aln_off" (one entry per occurrence plus one, starting at 0);
    entries offsets[i]:offsets[i + 1] belong to query i. ``operations=False``: starts only."""
    return _panel_arrays(aligner, queries, database, min_score, window, algorithm, "full", start, end, device, max_hits,
                         bool(operations))[0]


# --- a panel of PSSMs in one call (miopalSearchPssmBatchOccurrences, ...Aligned) --------------------------------------
# (the four functions above with a list of `Pssm` where the queries stand: a motif library, each PSSM beside its
# `Pssm.reverse_complement()` where both strands count)

def find_occurrences_pssm_many(aligner: Aligner, pssms, database: BaseDatabase, min_score, *, window=None,
                               algorithm: str = "hw", mode: str = "end", start: int = 0, end: int = UINT32_MAX,
                               device: int = 0,
                               max_hits: typing.Optional[int] = None) -> typing.List[typing.List[ScoreResult]]:
    """`find_occurrences_many` with a list of `Pssm` in the place of the queries and the aligner's matrix: one list of
    `EndResult` per PSSM, each what ``find_occurrences_pssm(aligner, pssm, ..., mode="end")`` returns for that PSSM. A
    window of None is that PSSM's height. ``mode="full"`` raises ValueError: `find_occurrence_alignments_pssm_many`
    returns the alignments."""
    return _panel_lists(mode, _panel_arrays(aligner, pssms, database, min_score, window, algorithm, mode, start, end, device,
                                            max_hits, pssm=True))


def find_occurrences_pssm_many_arrays(aligner: Aligner, pssms, database: BaseDatabase, min_score, *, window=None,
                                      algorithm: str = "hw", mode: str = "end", start: int = 0, end: int = UINT32_MAX,
                                      device: int = 0,
                                      max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
    """`find_occurrences_pssm_many` without result objects: `find_occurrences_many_arrays`' CSR, entries
    offsets[i]:offsets[i + 1] belonging to PSSM i."""
    return _panel_arrays(aligner, pssms, database, min_score, window, algorithm, mode, start, end, device, max_hits,
                         pssm=True)[0]


def find_occurrence_alignments_pssm_many(aligner: Aligner, pssms, database: BaseDatabase, min_score, *, window=None,
                                         algorithm: str = "hw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                                         max_hits: typing.Optional[int] = None
                                         ) -> typing.List[typing.List[ScoreResult]]:
    """`find_occurrence_alignments_many` with a list of `Pssm`: one list of `FullResult` per PSSM, each what
    ``find_occurrences_pssm(aligner, pssm, ..., mode="full")`` returns for that PSSM; the PSSMs' consensus tells
    matches from mismatches."""
    return _panel_lists("full", _panel_arrays(aligner, pssms, database, min_score, window, algorithm, "full", start, end,
                                              device, max_hits, True, pssm=True))


def find_occurrence_alignments_pssm_many_arrays(aligner: Aligner, pssms, database: BaseDatabase, min_score, *,
                                                window=None, algorithm: str = "hw", start: int = 0,
                                                end: int = UINT32_MAX, device: int = 0,
                                                max_hits: typing.Optional[int] = None,
                                                operations: bool = True) -> typing.Dict[str, typing.Any]:
    """`find_occurrence_alignments_pssm_many` without result objects: `find_occurrence_alignments_many_arrays`' CSR,
    entries offsets[i]:offsets[i + 1] belonging to PSSM i. ``operations=False``: starts only."""
    return _panel_arrays(aligner, pssms, database, min_score, window, algorithm, "full", start, end, device, max_hits,
                         bool(operations), pssm=True)[0]
