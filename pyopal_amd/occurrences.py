"""Every occurrence of a query in each target, with where it starts and how it aligns (include/miopal.h,
miopalSearchOccurrences and miopalSearchOccurrencesAligned): the adapter a read carries twice, the binding sites of a
primer, the copies of a repeated domain - cut out from start to end.

Free functions that take an `Aligner`, not methods of it: the set of `Aligner`'s public methods is the reference's
plus a fixed table of extensions.

    sites = find_occurrences(aligner, "ETSEEES", database, 25)          # FullResult, several per target
    ends = find_occurrences(aligner, "ETSEEES", database, 25, mode="end")

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
