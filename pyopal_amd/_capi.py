"""ctypes binding to libmiopal.so, the C ABI declared in include/opal.h and
include/miopal.h. This is the only way Python code in this repository reaches
the HIP kernels; there is no CPU fallback behind it."""

from __future__ import annotations

import ctypes
import os
import typing

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIOPAL_LIBRARY: another build of the same library (A/B timing of kernel variants, tools/ab_build.sh)
LIB_PATH = os.environ.get("MIOPAL_LIBRARY") or os.path.join(_HERE, "libmiopal.so")

OPAL_ERR_OVERFLOW = 1
OPAL_ERR_NO_SIMD_SUPPORT = 2
OPAL_ERR_INVALID_MODE = 3
MIOPAL_ERR_TOO_MANY_HITS = 103   # include/opal.h: more hits than max_hits (search_hits and its forms)
MIOPAL_MAX_TOP = 4096   # include/miopal.h: the largest k of miopalSearchTop / miopalSearchBatchTop
MIOPAL_MAX_TARGET_TOP = 8   # include/miopal.h: the largest m of miopalSearchBatchTargetTop
MIOPAL_STAT_BINS = 128   # include/miopal.h: the length bins of miopalSearchSignificant's statistics
MIOPAL_FIT_MAX_REFITS = 3
MIOPAL_PROFILE_WEIGHT_ONE = 1 << 32   # include/miopal.h: 1.0 of miopalProfileColumns' 32.32 fixed-point weights
PROFILE_UNCOVERED = 255   # an entry of a member's row that its alignment does not cover

SEARCH = {"score": 0, "end": 1, "full": 2}
MODE = {"nw": 0, "hw": 1, "ov": 2, "sw": 3}
OVERFLOW = {"simple": 0, "buckets": 1}


class OpalSearchResult(ctypes.Structure):
    _fields_ = [
        ("scoreSet", ctypes.c_int),
        ("score", ctypes.c_int),
        ("endLocationTarget", ctypes.c_int),
        ("endLocationQuery", ctypes.c_int),
        ("startLocationTarget", ctypes.c_int),
        ("startLocationQuery", ctypes.c_int),
        ("alignment", ctypes.POINTER(ctypes.c_ubyte)),
        ("alignmentLength", ctypes.c_int),
    ]


class ScoreFit(ctypes.Structure):
    """MiopalScoreFit (include/miopal.h): the statistics, the fit and the table of a significance search."""
    _fields_ = [
        ("targets", ctypes.c_int64), ("used", ctypes.c_int64),
        ("passes", ctypes.c_int32), ("degenerate", ctypes.c_int32),
        ("intercept", ctypes.c_double), ("slope", ctypes.c_double), ("sigma", ctypes.c_double), ("zCut", ctypes.c_double),
        ("binTargets", ctypes.c_int64 * MIOPAL_STAT_BINS), ("binLength", ctypes.c_int64 * MIOPAL_STAT_BINS),
        ("all", ctypes.c_int64 * 3 * MIOPAL_STAT_BINS), ("kept", ctypes.c_int64 * 3 * MIOPAL_STAT_BINS),
        ("ceiling", ctypes.c_int32 * MIOPAL_STAT_BINS), ("threshold", ctypes.c_int32 * MIOPAL_STAT_BINS),
    ]


def length_bins(lengths) -> np.ndarray:
    """The length bin of include/miopal.h for every entry of ``lengths`` (integers >= 0), in integers: 0 for 0,
    otherwise 1 + 4 e + m with e = floor(log2 L) and m the two bits below the leading one."""
    L = np.asarray(lengths, dtype=np.int64)
    if np.any(L < 0):
        raise ValueError("lengths must not be negative")
    e = np.zeros(L.shape, dtype=np.int64)
    for shift in (32, 16, 8, 4, 2, 1):   # floor(log2 L) by halving, no floating point
        up = (L >> (e + shift)) > 0
        e[up] += shift
    m = np.where(e >= 2, (L >> np.maximum(e - 2, 0)) & 3, (L << np.maximum(2 - e, 0)) & 3)
    return np.where(L == 0, 0, np.minimum(1 + 4 * e + m, MIOPAL_STAT_BINS - 1)).astype(np.int64)


_lib = None
_libc = None

EXPORTS = [
    # opal.h
    "opalInitSearchResult", "opalSearchResultIsEmpty", "opalSearchResultSetScore",
    "opalSearchDatabase", "opalSearchDatabaseCharSW",
    # miopal.h
    "miopalDeviceCount", "miopalLastError", "miopalDbCreate", "miopalDbCreateFlat", "miopalDbCreateSubset",
    "miopalDbDestroy", "miopalDbCount", "miopalDbTotalLength", "miopalDbDeviceBytes",
    "miopalSearch", "miopalSearchFlat", "miopalSearchFlatInto", "miopalSearchPssm", "miopalSearchDeviceScores", "miopalSetProfiling", "miopalLastKernelTime",
    "miopalLastRouting", "miopalLastWindowPlan", "miopalLastLaunchShape", "miopalLastFullRouting", "miopalSearchResults",
    "miopalReleaseCaches",
    "miopalSearchBatch", "miopalLastBatchRouting", "miopalSearchTop", "miopalSearchBatchTop",
    "miopalAlignPairs", "miopalLastPairRouting", "miopalSearchPssmTop", "miopalAlignPairsPssm",
    "miopalSearchHits", "miopalSearchPssmHits", "miopalSearchBatchHits", "miopalSearchBatchTargetTop",
    "miopalSearchSignificant", "miopalSearchPssmSignificant", "miopalSearchBatchSignificant",
    "miopalSetTuning", "miopalGetTuning", "miopalDbSetOption", "miopalDbReleaseWorkspaces",
    "miopalProfileColumns", "miopalProfileColumnsPssm",
    "miopalSearchOccurrences", "miopalSearchPssmOccurrences", "miopalLastOccurrenceRouting",
    "miopalSearchOccurrencesAligned", "miopalSearchPssmOccurrencesAligned", "miopalLastOccurrenceAlignRouting",
    "miopalSearchBatchOccurrences", "miopalLastBatchOccurrenceRouting", "miopalLastBatchOccurrenceGroups",
    "miopalSearchBatchOccurrencesAligned", "miopalLastBatchOccurrenceAlignRouting",
    "miopalSearchPssmBatchOccurrences", "miopalSearchPssmBatchOccurrencesAligned",
    # test hooks
    "miopalTestProfileColumns",
    "miopalSelfTest", "miopalTestInjectFault", "miopalTestSetLogicalDevices", "miopalTestSelectTop",
    "miopalTestSelectHits", "miopalTestSelectColumns", "miopalTestRowStats", "miopalTestSelectHitsBinned",
    "miopalTestPickOccurrences",
]


def _share_hip_runtime() -> None:
    """Make libmiopal.so and PyTorch-ROCm use ONE HIP runtime.

    PyTorch wheels bundle their own ``libamdhip64.so.7`` (torch/lib). A process
    that loads the system copy first (as libmiopal.so's RUNPATH would) and
    torch's copy second ends up with two runtimes, and the second one reports
    "No HIP GPUs are available". Loading torch's copy first, when torch is
    installed, lets libmiopal.so bind to it by SONAME; torch itself is not
    imported.
    """
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib() -> ctypes.CDLL:
    """Load libmiopal.so (built in-tree by ``__graft_entry__.build()`` or
    ``make -C pyopal_amd/csrc``). Raises if it is missing."""
    global _lib, _libc
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()')")
        _share_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        c_int, c_i64, c_vp, c_dbl = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
        pp, p_i64 = ctypes.POINTER(c_vp), ctypes.POINTER(c_i64)
        L.miopalDeviceCount.restype = c_int
        L.miopalLastError.restype = ctypes.c_char_p
        # (restype, argtypes) of everything else. The search entry points are made of a few pieces (include/miopal.h):
        # the handle with one of three query sides, the slice, and what the family adds behind it.
        one = [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int]           # db, query, length, gapOpen, gapExt, matrix, A
        pssm = [c_vp, c_vp, c_int, c_int, c_int, c_int]                # db, rows, length, gapOpen, gapExt, A
        pssm_full = [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int]     # db, rows, consensus, length, gapOpen, gapExt, A
        batch = [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int]   # db, queries, offsets, n, gapOpen, gapExt, matrix, A
        middle = [c_int, c_int, c_i64, c_i64]                          # searchType, mode, start, end
        pair_list = [c_vp, c_vp, c_i64]                                # pair queries, pair targets, pairs
        flat = [c_vp] * 5 + [pp]                                       # score, endT, endQ, startT, startQ, operations
        top = [c_int, c_int] + [c_vp] * 5                              # k, minScore, count, index, score, endT, endQ
        found = [pp] * 4                                               # target, score, endT, endQ
        columns = [c_int, c_vp, c_i64] + [c_vp] * 4                    # mode, targets, n, counts, weighted, weights, msa
        rows = [c_vp, c_vp, c_vp, c_int, c_i64]                        # (test hooks) score, endT, endQ, rows, stride
        table = {
            "miopalDbCreate": (c_int, [pp, c_vp, c_vp, c_i64, c_int, c_int]),
            "miopalDbCreateFlat": (c_int, [pp, c_vp, c_vp, c_i64, c_int, c_int]),
            "miopalDbCreateSubset": (c_int, [pp, c_vp, c_vp, c_i64]),
            "miopalDbDestroy": (None, [c_vp]),
            "miopalDbCount": (c_i64, [c_vp]), "miopalDbTotalLength": (c_i64, [c_vp]),
            "miopalDbDeviceBytes": (c_i64, [c_vp]), "miopalDbReleaseWorkspaces": (c_i64, [c_vp]),
            "miopalDbSetOption": (c_int, [c_vp, ctypes.c_char_p, c_i64]),
            "miopalSetTuning": (c_int, [ctypes.c_char_p, ctypes.c_char_p]),
            "miopalGetTuning": (ctypes.c_char_p, [ctypes.c_char_p]),
            "miopalSetProfiling": (None, [c_vp, c_int]),
            "miopalReleaseCaches": (None, []),
            "miopalLastFullRouting": (c_int, []),
            "miopalLastRouting": (None, [p_i64]), "miopalLastWindowPlan": (None, [p_i64]), "miopalLastLaunchShape": (None, [p_i64]),
            "miopalLastPairRouting": (None, [p_i64]),
            "miopalLastBatchRouting": (None, [p_i64]), "miopalLastOccurrenceRouting": (None, [p_i64]),
            "miopalLastOccurrenceAlignRouting": (None, [p_i64]),
            "miopalLastBatchOccurrenceRouting": (None, [p_i64]), "miopalLastBatchOccurrenceGroups": (None, [p_i64]),
            "miopalLastBatchOccurrenceAlignRouting": (None, [p_i64]),
            "miopalLastKernelTime": (c_int, [c_vp, ctypes.POINTER(ctypes.c_float)]),
            "miopalSearch": (c_int, one + middle + [c_vp] * 7),
            "miopalSearchFlat": (c_int, one + middle + flat + [c_vp]),
            "miopalSearchFlatInto": (c_int, one + middle + flat + [p_i64, c_vp]),
            "miopalSearchPssm": (c_int, pssm_full + middle + flat + [c_vp]),
            "miopalSearchDeviceScores": (c_int, one + middle[1:] + [c_vp, c_vp]),
            "miopalSearchBatch": (c_int, batch + middle + [c_vp] * 3),
            "miopalSearchBatchTargetTop": (c_int, batch + middle + top),
            "miopalAlignPairs": (c_int, batch[:4] + pair_list + batch[4:] + middle[:2] + flat + [c_vp]),
            "miopalAlignPairsPssm": (c_int, [c_vp] * 4 + [c_int] + pair_list + pssm[3:] + middle[:2] + flat + [c_vp]),
            "miopalProfileColumns": (c_int, one + columns),
            "miopalProfileColumnsPssm": (c_int, pssm_full + columns),
            "miopalSearchResults": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_i64, c_i64]),
            "opalSearchDatabase": (c_int, [c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int]),
            # test hooks
            "miopalSelfTest": (c_int, [c_int]),
            "miopalTestInjectFault": (None, [c_int, c_int, c_int]),
            "miopalTestSetLogicalDevices": (c_int, [c_int]),
            "miopalTestSelectTop": (c_int, rows + [c_int, c_int, c_i64] + [c_vp] * 6),
            "miopalTestSelectHits": (c_int, rows + [c_vp, c_i64, c_vp] + found),
            "miopalTestSelectHitsBinned": (c_int, rows + [c_vp, c_vp, c_i64, c_vp] + found),
            "miopalTestSelectColumns": (c_int, rows + [c_vp, c_vp, c_int, c_vp, c_int, c_int] + [c_vp] * 5),
            "miopalTestRowStats": (c_int, [c_vp, c_int, c_i64] + [c_vp] * 5),
            "miopalTestProfileColumns": (c_int, [c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
            # value, valueRow, rows, stride, length, minScore, window, hitOffsets, column, score, row
            "miopalTestPickOccurrences": (c_int, rows[1:] + [c_vp, c_int, c_int, c_vp] + found[:3]),
        }
        # top / hits / significant of every query side: one row of outputs, or (Batch) a count per query and a CSR
        for side, head in (("", one), ("Pssm", pssm), ("Batch", batch)):
            table[f"miopalSearch{side}Top"] = (c_int, head + middle + top)
            cut, counts = ([c_vp], [c_vp]) if side == "Batch" else ([c_int], [p_i64])
            table[f"miopalSearch{side}Hits"] = (c_int, head + middle + cut + [c_i64] + counts + found)
            cut = [c_vp, c_dbl] if side == "Batch" else [c_dbl, c_dbl]   # max E-value(s), exclude_z
            table[f"miopalSearch{side}Significant"] = (c_int, head + middle + cut + [c_i64, c_vp] + counts + found + [pp])
        # occurrences: no search type; minScore, window, maxHits, one count
        for side, head in (("", one), ("Pssm", pssm)):
            table[f"miopalSearch{side}Occurrences"] = (c_int, head + middle[1:] + [c_int, c_int, c_i64, p_i64] + found)
        # ... of a panel: one cut and one window per query, maxHits over all of them, the CSR's offsets
        table["miopalSearchBatchOccurrences"] = (c_int, batch + middle[1:] + [c_vp, c_vp, c_i64, c_vp] + found)
        # ... aligned: the PSSM with its consensus; behind the occurrences startT, startQ, operations, their offsets
        for side, head in (("", one), ("Pssm", pssm_full)):
            table[f"miopalSearch{side}OccurrencesAligned"] = (c_int, head + middle[1:] + [c_int, c_int, c_i64, p_i64] + found + [pp] * 4)
        table["miopalSearchBatchOccurrencesAligned"] = (c_int, table["miopalSearchBatchOccurrences"][1] + [pp] * 4)
        # ... of a panel of PSSMs: db, rows, [consensus,] row offsets, n, gapOpen, gapExt, A where `batch` stands
        for name, consensus in (("miopalSearchPssmBatchOccurrences", []), ("miopalSearchPssmBatchOccurrencesAligned", [c_vp])):
            table[name] = (c_int, [c_vp, c_vp] + consensus + [c_vp, c_int, c_int, c_int, c_int]
                           + table[name.replace("Pssm", "")][1][len(batch):])
        for name, (restype, argtypes) in table.items():
            getattr(L, name).restype = restype
            getattr(L, name).argtypes = argtypes
        _lib = L
        _libc = ctypes.CDLL(None)
        _libc.free.argtypes = [c_vp]
        _libc.free.restype = None
    return _lib


def last_error() -> str:
    msg = lib().miopalLastError()
    return msg.decode("utf-8", "replace") if msg else ""


class TooManyHits(RuntimeError):
    """MIOPAL_ERR_TOO_MANY_HITS: a hit search found more than ``max_hits``. ``counts``: what it would take - the
    number of hits (search_hits, search_pssm_hits) or the CSR offsets, one entry per query plus one
    (search_batch_hits). Nothing was allocated and the handle stays usable."""

    def __init__(self, message: str, counts=None):
        super().__init__(message)
        self.counts = counts


def raise_for(rc: int) -> None:
    """Error mapping of the reference plugin (src/pyopal/platform/pyx.in:102-107)."""
    if rc == 0:
        return
    if rc == MIOPAL_ERR_TOO_MANY_HITS:
        raise TooManyHits(f"more hits than max_hits (code={rc}): {last_error()}")
    if rc == OPAL_ERR_NO_SIMD_SUPPORT:
        raise RuntimeError("no supported SIMD backend available")
    if rc == OPAL_ERR_OVERFLOW:
        raise OverflowError("overflow detected while computing alignment scores")
    detail = last_error()
    raise RuntimeError(f"failed to align to Opal database (code={rc})" + (f": {detail}" if detail else ""))


def set_tuning(name: str, value: typing.Optional[str]) -> None:
    """Set (or, with None, unset) a tuning switch of the library for the searches that start from now on
    (include/miopal.h, miopalSetTuning; pyopal_amd/csrc/tuning.h lists the switches). The environment is
    only read once, when the library first looks at a switch: later changes go through here."""
    rc = lib().miopalSetTuning(name.encode(), None if value is None else str(value).encode())
    raise_for(rc)


def get_tuning(name: str) -> typing.Optional[str]:
    v = lib().miopalGetTuning(name.encode())
    return None if v is None else v.decode()


class tuning:
    """``with tuning(NO_BIASED="1", PAIR_STRIPS=None): ...`` - switches set (None: unset) for the block and
    put back afterwards. Process-wide, like the environment they replace: for tests and A/B tools."""

    def __init__(self, **switches):
        self._want = switches
        self._saved = {}

    def __enter__(self):
        for name, value in self._want.items():
            self._saved[name] = get_tuning(name)
            set_tuning(name, value)
        return self

    def __exit__(self, *exc):
        for name, value in self._saved.items():
            set_tuning(name, value)
        return False


def _ptr(a: typing.Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def select_top_rows(score: np.ndarray, k: int, min_score: typing.Optional[int] = None,
                    end_q: typing.Optional[np.ndarray] = None, end_t: typing.Optional[np.ndarray] = None,
                    start: int = 0) -> typing.Dict[str, typing.Any]:
    """miopalTestSelectTop (test hook): the device top-k selection alone on the rows of ``score`` (int32,
    (rows, stride); a 1-D array is one row), with ``end_q`` / ``end_t`` of the same shape beside them (both or
    neither). Returns search_batch_top's dict - "count" (rows,), "target" (int64, ``start`` + index), "score" and, with
    end arrays, "end_t" / "end_q", of shape (rows, k), best first, -1 past the count - plus "gave_up", the number of
    blocks that gave up waiting for the blocks before them (0). The C side checks the arguments."""
    score = np.ascontiguousarray(score, dtype=np.int32)
    if score.ndim == 1:
        score = score[None, :]
    if score.ndim != 2:
        raise ValueError("score must have shape (rows, stride)")
    rows, stride = score.shape
    ends = []
    for e in (end_q, end_t):
        if e is not None:
            e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1, e.shape[-1])
            if e.shape != score.shape:
                raise ValueError("end arrays must have the shape of score")
        ends.append(e)
    shape = (rows, max(k, 0))
    out = {"count": np.zeros(rows, dtype=np.int32), "target": np.empty(shape, dtype=np.int64),
           "score": np.empty(shape, dtype=np.int32)}
    if ends[0] is not None or ends[1] is not None:
        out.update(end_t=np.empty(shape, dtype=np.int32), end_q=np.empty(shape, dtype=np.int32))
    gave_up = ctypes.c_int(-1)
    rc = lib().miopalTestSelectTop(_ptr(score), _ptr(ends[1]), _ptr(ends[0]), rows, stride, k,
                                   _floor(min_score), start, _ptr(out["count"]),
                                   _ptr(out["target"]), _ptr(out["score"]), _ptr(out.get("end_t")),
                                   _ptr(out.get("end_q")), ctypes.byref(gave_up))
    raise_for(rc)
    out["gave_up"] = int(gave_up.value)
    return out


class _MallocBytes:
    """Owner of a buffer returned by the C ABI; numpy arrays made from it keep it alive."""

    def __init__(self, address: int, size: int, capacity: int = 0):
        self._address = address
        self._capacity = max(capacity, size)
        self.__array_interface__ = {"data": (address, False), "shape": (size,), "typestr": "|u1",
                                    "version": 3}

    def view(self, size: int) -> "_MallocView":
        return _MallocView(self, size)

    def __del__(self):
        if _libc is not None:   # (gone at interpreter shutdown: the process is about to return its memory anyway)
            _libc.free(ctypes.c_void_p(self._address))


class _MallocView:
    """The first ``size`` bytes of a _MallocBytes buffer that was written again (``reuse=``)."""

    def __init__(self, owner: _MallocBytes, size: int):
        self._owner = owner
        self.__array_interface__ = {"data": (owner._address, False), "shape": (size,), "typestr": "|u1",
                                    "version": 3}


def _take_malloced(pointer: ctypes.c_void_p, length: int, dtype) -> np.ndarray:
    """The ``length`` entries of ``dtype`` at a malloc'ed address the C ABI returned, as an array that takes the buffer
    over without a copy (freed with the array); NULL: an empty array."""
    if not pointer.value or length == 0:
        if pointer.value:
            _libc.free(pointer)
        return np.zeros(0, dtype=dtype)
    return np.asarray(_MallocBytes(pointer.value, length * np.dtype(dtype).itemsize)).view(dtype)


class _HitPointers:
    """The four output pointers of a hit search and the arrays made from them."""

    def __init__(self):
        self.target, self.score, self.end_t, self.end_q = (ctypes.c_void_p() for _ in range(4))

    def refs(self):
        return tuple(ctypes.byref(p) for p in (self.target, self.score, self.end_t, self.end_q))

    def arrays(self, total: int, ends: bool) -> typing.Dict[str, np.ndarray]:
        out = {"target": _take_malloced(self.target, total, np.int64), "score": _take_malloced(self.score, total, np.int32)}
        if ends:
            out.update(end_t=_take_malloced(self.end_t, total, np.int32), end_q=_take_malloced(self.end_q, total, np.int32))
        return out


class _AlignedPointers:
    """An aligned occurrence search's four outputs behind `_HitPointers`' (with ``operations``: all four) and their arrays."""

    def __init__(self, operations: bool):
        self.operations = operations
        self.start_t, self.start_q = ctypes.c_void_p(), ctypes.c_void_p()
        self.ops, self.ops_off = ctypes.c_void_p(), ctypes.c_void_p()

    def refs(self):
        return (ctypes.byref(self.start_t), ctypes.byref(self.start_q),
                ctypes.byref(self.ops) if self.operations else None, ctypes.byref(self.ops_off) if self.operations else None)

    def arrays(self, total: int) -> typing.Dict[str, typing.Any]:
        out = {"start_t": _take_malloced(self.start_t, total, np.int32), "start_q": _take_malloced(self.start_q, total, np.int32)}
        if self.operations:
            aoff = _take_malloced(self.ops_off, total + 1, np.int64)
            flat = _take_malloced(self.ops, int(aoff[-1]), np.uint8)
            out.update(aln_flat=flat, aln_off=aoff, aln=_LazyAlignments(flat, aoff))
        return out


def select_hits_rows(score: np.ndarray, min_score, end_q: typing.Optional[np.ndarray] = None,
                     end_t: typing.Optional[np.ndarray] = None, start: int = 0) -> typing.Dict[str, np.ndarray]:
    """miopalTestSelectHits (test hook): the device compaction alone on the rows of ``score`` (int32, (rows, stride); a
    1-D array is one row), with ``end_q`` / ``end_t`` of the same shape beside them (both or neither). ``min_score``:
    an integer or one per row. Returns search_batch_hits' dict: "offsets" (rows + 1,), "target" (int64, ``start`` +
    index), "score" and, with end arrays, "end_t" / "end_q", row after row, index ascending inside a row. The C side
    checks the arguments."""
    score = np.ascontiguousarray(score, dtype=np.int32)
    if score.ndim == 1:
        score = score[None, :]
    if score.ndim != 2:
        raise ValueError("score must have shape (rows, stride)")
    rows, stride = score.shape
    ends = []
    for e in (end_q, end_t):
        if e is not None:
            e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1, e.shape[-1])
            if e.shape != score.shape:
                raise ValueError("end arrays must have the shape of score")
        ends.append(e)
    thresholds = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, dtype=np.int32), (rows,)))
    offsets = np.zeros(rows + 1, dtype=np.int64)
    ptrs = _HitPointers()
    rc = lib().miopalTestSelectHits(_ptr(score), _ptr(ends[1]), _ptr(ends[0]), rows, stride, _ptr(thresholds), start,
                                    _ptr(offsets), *ptrs.refs())
    raise_for(rc)
    out = {"offsets": offsets}
    out.update(ptrs.arrays(int(offsets[-1]), ends[0] is not None))
    return out


def pick_occurrences_rows(value: np.ndarray, length, min_score: int, window: int,
                          value_row: typing.Optional[np.ndarray] = None) -> typing.Dict[str, np.ndarray]:
    """miopalTestPickOccurrences (test hook): the device picker of `DeviceDatabase.search_occurrences` alone on the rows
    of ``value`` (int32, (rows, stride); a 1-D array is one row), of which columns 0 .. length[r] - 1 are valid
    (``length``: an integer or one per row), with ``value_row`` of the same shape beside them or None (row -1
    throughout). Returns a CSR: "offsets" (rows + 1,), "column", "score" and "row", row after row, column ascending
    inside a row. The C side checks the arguments."""
    value = np.ascontiguousarray(value, dtype=np.int32)
    if value.ndim == 1:
        value = value[None, :]
    if value.ndim != 2:
        raise ValueError("value must have shape (rows, stride)")
    rows, stride = value.shape
    if value_row is not None:
        value_row = np.ascontiguousarray(value_row, dtype=np.int32).reshape(-1, np.shape(value_row)[-1])
        if value_row.shape != value.shape:
            raise ValueError("value_row must have the shape of value")
    lengths = np.ascontiguousarray(np.broadcast_to(np.asarray(length, dtype=np.int32), (rows,)))
    offsets = np.zeros(rows + 1, dtype=np.int64)
    column, score, row = (ctypes.c_void_p() for _ in range(3))
    rc = lib().miopalTestPickOccurrences(_ptr(value), _ptr(value_row), rows, stride, _ptr(lengths), min_score, window,
                                         _ptr(offsets), ctypes.byref(column), ctypes.byref(score), ctypes.byref(row))
    raise_for(rc)
    total = int(offsets[-1])
    return {"offsets": offsets, "column": _take_malloced(column, total, np.int32),
            "score": _take_malloced(score, total, np.int32), "row": _take_malloced(row, total, np.int32)}


def _check_occurrence_rule(algorithm, min_score, window) -> None:
    """what the C side refuses of an occurrence search's rule, refused before it is reached. ``min_score`` and
    ``window``: the one value each of a single search (a window of None is the query's length), or a panel's smallest"""
    if algorithm not in ("hw", "sw"):
        raise ValueError(f"occurrences are defined for the algorithms 'hw' and 'sw', not {algorithm!r}")
    if window is not None and window < 0:
        raise ValueError("window must not be negative")
    if algorithm == "sw" and min_score < 1:
        raise ValueError("min_score must be at least 1 with algorithm 'sw'")


def last_occurrence_routing() -> typing.List[int]:
    """miopalLastOccurrenceRouting: [targets of the count sweep, targets of the write sweep, chunks, strips per sweep]"""
    counts = (ctypes.c_int64 * 4)()
    lib().miopalLastOccurrenceRouting(counts)
    return list(counts)


def last_batch_occurrence_routing() -> typing.List[int]:
    """miopalLastBatchOccurrenceRouting: [queries on the panel kernels, queries on the single-query path, chunks, (query,
    target) pairs the write sweeps took] of the calling thread's last `search_batch_occurrences` call"""
    counts = (ctypes.c_int64 * 4)()
    lib().miopalLastBatchOccurrenceRouting(counts)
    return list(counts)


def last_batch_occurrence_groups() -> typing.List[int]:
    """miopalLastBatchOccurrenceGroups: [groups of panel queries over all chunks, the most queries in one group, the bytes
    of LDS of the largest group's rows] of the calling thread's last `search_batch_occurrences` call"""
    counts = (ctypes.c_int64 * 3)()
    lib().miopalLastBatchOccurrenceGroups(counts)
    return list(counts)


def _per_query(values, lengths, name) -> np.ndarray:
    """a cut or a window of a panel as the C ABI takes it: one int32 per query from a scalar or one value per query
    (None, as the scalar or as an entry: the query's own length)"""
    if values is None or np.ndim(values) == 0:
        values = [values] * len(lengths)
    values = list(values)
    if len(values) != len(lengths):
        raise ValueError(f"{name} must be one value or one per query ({len(lengths)}), got {len(values)}")
    return np.array([n if v is None else int(v) for v, n in zip(values, lengths)], dtype=np.int64)


def last_occurrence_align_routing() -> typing.List[int]:
    """miopalLastOccurrenceAlignRouting: [occurrences aligned one lane each, one wavefront each, chunks of the alignment
    stage, the longest target window] of the calling thread's last `search_occurrence_alignments` call"""
    counts = (ctypes.c_int64 * 4)()
    lib().miopalLastOccurrenceAlignRouting(counts)
    return list(counts)


def last_batch_occurrence_align_routing() -> typing.List[int]:
    """miopalLastBatchOccurrenceAlignRouting: [occurrences aligned one lane each, one wavefront each, sub-chunks of the
    alignment stage, the longest target window] of the calling thread's last `search_batch_occurrence_alignments`
    call, over its panel chunks and long queries"""
    counts = (ctypes.c_int64 * 4)()
    lib().miopalLastBatchOccurrenceAlignRouting(counts)
    return list(counts)


def _score_rows(score, end_q, end_t):
    """score as int32 (rows, stride) and the end arrays beside it, as the test hooks take them"""
    score = np.ascontiguousarray(score, dtype=np.int32)
    if score.ndim == 1:
        score = score[None, :]
    if score.ndim != 2:
        raise ValueError("score must have shape (rows, stride)")
    ends = []
    for e in (end_q, end_t):
        if e is not None:
            e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1, e.shape[-1])
            if e.shape != score.shape:
                raise ValueError("end arrays must have the shape of score")
        ends.append(e)
    return score, ends


def _bin_table(table, rows, name):
    table = np.asarray(table, dtype=np.int32)
    if table.shape not in ((MIOPAL_STAT_BINS,), (rows, MIOPAL_STAT_BINS)):
        raise ValueError(f"{name} must hold {MIOPAL_STAT_BINS} entries, or as many per row")
    return np.ascontiguousarray(np.broadcast_to(table, (rows, MIOPAL_STAT_BINS)))


def row_stats_rows(score: np.ndarray, length: np.ndarray, ceiling: typing.Optional[np.ndarray] = None,
                   skip: typing.Optional[np.ndarray] = None) -> typing.Dict[str, np.ndarray]:
    """miopalTestRowStats (test hook): the statistics kernels alone on the rows of ``score`` (int32, (rows, stride); a
    1-D array is one row) whose column i belongs to a target of ``length[i]``. ``ceiling``: (128,) or (rows, 128), the
    entries above it left out (None: none); ``skip``: one flag per row, non-zero - the row is not read. Returns
    "stats" (int64, (rows, 128, 3): n, sum, sum of squares per bin, wrapping) and "bin" (uint8, (stride,), the
    device's bins). The C side checks the arguments."""
    score, _ = _score_rows(score, None, None)
    rows, stride = score.shape
    length = np.ascontiguousarray(length, dtype=np.int32)
    if length.shape != (stride,):
        raise ValueError("length must hold one entry per column of score")
    table = None if ceiling is None else _bin_table(ceiling, rows, "ceiling")
    flags = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.int32)
    if flags is not None and flags.shape != (rows,):
        raise ValueError("skip must hold one flag per row")
    out = {"stats": np.zeros((rows, MIOPAL_STAT_BINS, 3), dtype=np.int64), "bin": np.zeros(stride, dtype=np.uint8)}
    rc = lib().miopalTestRowStats(_ptr(score), rows, stride, _ptr(length), _ptr(table), _ptr(flags), _ptr(out["stats"]),
                                  _ptr(out["bin"]))
    raise_for(rc)
    return out


def select_hits_binned_rows(score: np.ndarray, length: np.ndarray, threshold: np.ndarray,
                            end_q: typing.Optional[np.ndarray] = None, end_t: typing.Optional[np.ndarray] = None,
                            start: int = 0) -> typing.Dict[str, np.ndarray]:
    """miopalTestSelectHitsBinned (test hook): `select_hits_rows` with ``length`` (one per column) and ``threshold``
    ((128,) or (rows, 128)) in the place of ``min_score``: entry i of row r is kept iff score >=
    threshold[r, bin of length[i]]. Returns `select_hits_rows`' dict."""
    score, ends = _score_rows(score, end_q, end_t)
    rows, stride = score.shape
    length = np.ascontiguousarray(length, dtype=np.int32)
    if length.shape != (stride,):
        raise ValueError("length must hold one entry per column of score")
    table = _bin_table(threshold, rows, "threshold")
    offsets = np.zeros(rows + 1, dtype=np.int64)
    ptrs = _HitPointers()
    rc = lib().miopalTestSelectHitsBinned(_ptr(score), _ptr(ends[1]), _ptr(ends[0]), rows, stride, _ptr(length), _ptr(table),
                                          start, _ptr(offsets), *ptrs.refs())
    raise_for(rc)
    out = {"offsets": offsets}
    out.update(ptrs.arrays(int(offsets[-1]), ends[0] is not None))
    return out


def select_columns_rows(score: np.ndarray, m: int, min_score: typing.Optional[int] = None,
                        end_q: typing.Optional[np.ndarray] = None, end_t: typing.Optional[np.ndarray] = None,
                        pieces: typing.Optional[typing.Sequence[typing.Tuple[int, int]]] = None,
                        skip: typing.Optional[np.ndarray] = None) -> typing.Dict[str, np.ndarray]:
    """miopalTestSelectColumns (test hook): the device selection of search_batch_target_top alone - the ``m`` best
    rows of every column - on the rows of ``score`` (int32, (rows, stride); a 1-D array is one row), with ``end_q`` /
    ``end_t`` of the same shape beside them (both or neither). ``pieces``: (first row, rows) of every piece, folded in
    this order (None: all rows in one piece); ``skip``: one flag per row, non-zero - the row is never read. Returns
    search_batch_target_top's dict: "count" (stride,), "query" (the row), "score" and, with end arrays, "end_t" /
    "end_q", of shape (stride, m), best first, -1 past the count. The C side checks the arguments."""
    score = np.ascontiguousarray(score, dtype=np.int32)
    if score.ndim == 1:
        score = score[None, :]
    if score.ndim != 2:
        raise ValueError("score must have shape (rows, stride)")
    rows, stride = score.shape
    ends = []
    for e in (end_q, end_t):
        if e is not None:
            e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1, e.shape[-1])
            if e.shape != score.shape:
                raise ValueError("end arrays must have the shape of score")
        ends.append(e)
    pieces = np.ascontiguousarray([(0, rows)] if pieces is None else pieces, dtype=np.int32).reshape(-1, 2)
    first, counts = np.ascontiguousarray(pieces[:, 0]), np.ascontiguousarray(pieces[:, 1])
    flags = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8)
    if flags is not None and flags.shape != (rows,):
        raise ValueError("skip must hold one flag per row")
    shape = (stride, max(m, 0))
    out = {"count": np.zeros(stride, dtype=np.int32), "query": np.empty(shape, dtype=np.int32),
           "score": np.empty(shape, dtype=np.int32)}
    if ends[0] is not None or ends[1] is not None:
        out.update(end_t=np.empty(shape, dtype=np.int32), end_q=np.empty(shape, dtype=np.int32))
    rc = lib().miopalTestSelectColumns(_ptr(score), _ptr(ends[1]), _ptr(ends[0]), rows, stride, _ptr(first), _ptr(counts),
                                       len(pieces), _ptr(flags), m, _floor(min_score),
                                       _ptr(out["count"]), _ptr(out["query"]), _ptr(out["score"]), _ptr(out.get("end_t")),
                                       _ptr(out.get("end_q")))
    raise_for(rc)
    return out


def profile_columns_rows(msa: np.ndarray, alphabet_length: int) -> typing.Dict[str, np.ndarray]:
    """miopalTestProfileColumns (test hook): the count / terms / member weights / weighted kernels of `profile_columns`
    alone, on a multiple alignment the caller supplies - ``msa``: uint8 of shape (members, Q), entries a letter
    (< ``alphabet_length``), the gap (== ``alphabet_length``) or 255. Returns "counts" and "weighted" (int64,
    (Q, alphabet_length + 1)) and "member_weights" (int64, (members,)). The C side checks the arguments."""
    msa = np.ascontiguousarray(msa, dtype=np.uint8)
    if msa.ndim != 2:
        raise ValueError("msa must have shape (members, positions)")
    members, q = msa.shape
    width = max(int(alphabet_length), 0) + 1
    out = {"counts": np.zeros((q, width), dtype=np.int64), "weighted": np.zeros((q, width), dtype=np.int64),
           "member_weights": np.zeros(members, dtype=np.int64)}
    rc = lib().miopalTestProfileColumns(_ptr(msa), members, q, alphabet_length, _ptr(out["counts"]), _ptr(out["weighted"]),
                                        _ptr(out["member_weights"]))
    raise_for(rc)
    return out


class _LazyAlignments:
    """List-like view of the per-target operation arrays inside the flat buffer."""

    def __init__(self, flat: np.ndarray, offsets: np.ndarray):
        self._flat = flat
        self._off = offsets

    def __len__(self):
        return len(self._off) - 1

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        return self._flat[self._off[k]:self._off[k + 1]]

    def __iter__(self):
        for k in range(len(self)):
            yield self[k]


def _floor(min_score):
    """``min_score`` as the C ABI takes it: INT_MIN stands for no bound"""
    return -(2 ** 31) if min_score is None else min_score


def _bound(max_hits):
    """``max_hits`` as the C ABI takes it: -1 stands for no bound"""
    return -1 if max_hits is None else max_hits


def _packed(items, nothing):
    """A list of arrays laid end to end along their first axis -> (flat, offsets); ``nothing``: what stands for
    ``flat`` when there is not one entry in it."""
    offsets = np.zeros(len(items) + 1, dtype=np.int64)
    if items:
        np.cumsum([len(q) for q in items], out=offsets[1:])
    return (np.concatenate(items) if offsets[-1] else nothing), offsets


def _pssm_rows(row_scores, alphabet_length, shape):
    """the rows of a PSSM as the C ABI takes them; ``shape``: how the refusal of any other shape begins"""
    rows = np.ascontiguousarray(row_scores, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[1] != alphabet_length:
        raise ValueError(f"{shape}, {alphabet_length})")
    return rows


class _QuerySide(typing.NamedTuple):
    """What a call searches with, as the C ABI takes it: a query with a matrix, a PSSM, or a list of queries with a
    matrix, or a list of PSSMs (`DeviceDatabase._query_side`, `_pssm_side`, `_batch_side`, `_pssm_batch_side`)."""
    name: str                       # "", "Pssm", "Batch", "PssmBatch": the C functions that take it are miopalSearch<name>...
    queries: tuple                  # their arguments after the handle: (query, length) / (rows, [consensus,] length) /
                                    # (queries, offsets, n) / (rows, [consensus,] row offsets, n) ...
    scoring: tuple                  # ... and (gapOpen, gapExt, [matrix,] alphabet length)
    rows: typing.Optional[int]      # None: one query, one row of outputs; else the queries: a row each, or a CSR
    length: typing.Optional[int]    # of the one query
    keep: tuple                     # the arrays the pointers point into


class DeviceDatabase:
    """Owner of a MiopalDb handle (device-resident database)."""

    def __init__(self, residues: np.ndarray, offsets: np.ndarray, alphabet_length: int, device: int = 0):
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        handle = ctypes.c_void_p()
        rc = lib().miopalDbCreateFlat(ctypes.byref(handle), _ptr(residues), _ptr(offsets),
                                      len(offsets) - 1, alphabet_length, device)
        raise_for(rc)
        self._h = handle
        self.count = len(offsets) - 1
        self.offsets = offsets            # host copy: target k is residues[offsets[k]:offsets[k + 1]]
        self.alphabet_length = alphabet_length
        self.device = device

    @property
    def handle(self):
        return self._h

    def subset(self, indices) -> "DeviceDatabase":
        """A new resident database holding the targets ``indices`` of this one, gathered on the device
        from this one's residues (miopalDbCreateSubset: nothing crosses PCIe)."""
        idx = np.ascontiguousarray(indices, dtype=np.int64)
        handle = ctypes.c_void_p()
        rc = lib().miopalDbCreateSubset(ctypes.byref(handle), self._h, _ptr(idx) if len(idx) else None, len(idx))
        raise_for(rc)
        sub = DeviceDatabase.__new__(DeviceDatabase)
        sub._h = handle
        sub.count = len(idx)
        lengths = np.diff(self.offsets)[idx] if len(idx) else np.zeros(0, dtype=np.int64)
        sub.offsets = np.zeros(len(idx) + 1, dtype=np.int64)
        np.cumsum(lengths, out=sub.offsets[1:])
        sub.alphabet_length = self.alphabet_length
        sub.device = self.device
        return sub

    def close(self):
        if getattr(self, "_h", None):
            lib().miopalDbDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self) -> int:
        return int(lib().miopalDbDeviceBytes(self._h))

    def release_workspaces(self) -> int:
        """Free the idle per-search workspaces parked on the handle; returns the device bytes released."""
        return int(lib().miopalDbReleaseWorkspaces(self._h))

    def set_option(self, name: str, value: int) -> None:
        """Per-handle option (include/miopal.h, miopalDbSetOption): "reserve_cus", "small_search"."""
        raise_for(lib().miopalDbSetOption(self._h, name.encode(), int(value)))

    def _clamp(self, end: typing.Optional[int]) -> int:
        """the end of a slice: None is the end of the database, nothing reaches past it"""
        return self.count if end is None else min(end, self.count)

    # -- the query side of a call ---------------------------------------------------------------------------------
    def _query_side(self, query, matrix, gap_open, gap_extend, null_when_empty=False) -> _QuerySide:
        q = np.ascontiguousarray(query, dtype=np.uint8).ravel()
        S = np.ascontiguousarray(matrix, dtype=np.int32)
        return _QuerySide("", (None if null_when_empty and not len(q) else _ptr(q), len(q)),
                          (gap_open, gap_extend, _ptr(S), self.alphabet_length), None, len(q), (q, S))

    def _pssm_side(self, row_scores, consensus, gap_open, gap_extend, with_consensus=False,
                   shape="row_scores must have shape (query length",
                   per_row="consensus must have one entry per row of row_scores") -> _QuerySide:
        """``with_consensus``: the C function takes a consensus behind the rows (None: a null pointer)"""
        rows = _pssm_rows(row_scores, self.alphabet_length, shape)
        cons = None
        if consensus is not None:
            cons = np.ascontiguousarray(consensus, dtype=np.uint8).ravel()
            if len(cons) != len(rows):
                raise ValueError(per_row)
        pointers = (_ptr(rows), _ptr(cons)) if len(rows) else (None, None)
        return _QuerySide("Pssm", pointers[:2 if with_consensus else 1] + (len(rows),),
                          (gap_open, gap_extend, self.alphabet_length), None, len(rows), (rows, cons))

    def _batch_side(self, queries, matrix, gap_open, gap_extend) -> _QuerySide:
        qs = [np.ascontiguousarray(q, dtype=np.uint8).ravel() for q in queries]
        flat, offsets = _packed(qs, np.zeros(1, dtype=np.uint8))   # (a valid pointer for queries of length 0)
        S = np.ascontiguousarray(matrix, dtype=np.int32)
        return _QuerySide("Batch", (_ptr(flat), _ptr(offsets), len(qs)),
                          (gap_open, gap_extend, _ptr(S), self.alphabet_length), len(qs), None, (flat, offsets, S))

    def search(self, query: np.ndarray, matrix: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
               mode: str = "score", algorithm: str = "sw", start: int = 0,
               end: typing.Optional[int] = None,
               score_out: typing.Optional[np.ndarray] = None,
               reuse: typing.Optional[typing.Dict[str, typing.Any]] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearch with numpy outputs (same keys as tests/_oracle.search). ``score_out``: an
        int32 array of end - start entries to receive the scores (a caller that re-uses its result
        array; when it is pinned, device-visible host memory the kernel writes into it directly).
        ``reuse``: the result of an earlier search of the same slice and search type whose per-target
        arrays (scores, locations, operation offsets) and operations buffer are written again instead of
        fresh ones - the earlier result's arrays then hold the new values (a million targets: 36 MB of
        per-target pages and 67-360 MB of operations that need not be faulted in again, nor unmapped when
        the earlier result goes: 1.3 ms of a 11.5-ms `full` search for the arrays, 17 of 113 ms for the
        operations of a 300-residue query). An operations buffer that is too small stays with the earlier
        result, untouched."""
        end = self._clamp(end)
        q = np.ascontiguousarray(query, dtype=np.uint8)
        S = np.ascontiguousarray(matrix, dtype=np.int32)

        def call(st, score, et, eq, s_t, s_q, ops_ptr, ops_cap, aoff):
            return lib().miopalSearchFlatInto(self._h, _ptr(q), len(q), gap_open, gap_extend, _ptr(S),
                                              self.alphabet_length, st, MODE[algorithm], start, end,
                                              score, et, eq, s_t, s_q, ctypes.byref(ops_ptr), ctypes.byref(ops_cap), aoff)
        return self._flat_search(call, mode, max(end - start, 0), score_out, reuse)

    def _flat_search(self, call, mode, n, score_out=None, reuse=None) -> typing.Dict[str, typing.Any]:
        """The outputs of one flat search (`search`, `search_pssm`): the per-target arrays - fresh, or an earlier
        result's written again (``reuse``) - the C call, and the ownership of the operations buffer it returns or
        wrote in place. ``call(search type, score, end_t, end_q, start_t, start_q, ops_ptr, ops_cap, offsets)``
        makes the C call with these output pointers and returns its code."""
        st = SEARCH[mode]
        if score_out is not None and (score_out.dtype != np.int32 or score_out.shape != (n,) or
                                      not score_out.flags.c_contiguous):
            raise ValueError("score_out must be a contiguous int32 array with one entry per target of the slice")
        # the C side writes every entry of its outputs (locations of empty alignments are -1)
        def array(key, length, dtype, zeros=False):
            old = reuse.get(key) if reuse else None
            if (isinstance(old, np.ndarray) and old.dtype == dtype and old.shape == (length,) and
                    old.flags.c_contiguous and old.flags.writeable):
                if zeros:
                    old[:] = 0
                return old
            return np.zeros(length, dtype=dtype) if zeros else np.empty(length, dtype=dtype)

        out = {"score": score_out if score_out is not None else array("score", n, np.int32)}
        et = eq = s_t = s_q = aoff = None
        ops_ptr = ctypes.c_void_p()
        ops_cap = ctypes.c_int64(0)
        lent = reuse.get("_ops_owner") if reuse and st == 2 else None
        if isinstance(lent, _MallocBytes):
            ops_ptr = ctypes.c_void_p(lent._address)
            ops_cap = ctypes.c_int64(lent._capacity)
        else:
            lent = None
        if st >= 1:
            et = array("end_t", n, np.int32)
            eq = array("end_q", n, np.int32)
        if st == 2:
            s_t = array("start_t", n, np.int32)
            s_q = array("start_q", n, np.int32)
            aoff = array("aln_off", n + 1, np.int64, zeros=True)
        rc = call(st, _ptr(out["score"]), _ptr(et), _ptr(eq), _ptr(s_t), _ptr(s_q), ops_ptr, ops_cap, _ptr(aoff))
        raise_for(rc)
        if st >= 1:
            out.update(end_t=et, end_q=eq)
        if st == 2:
            total = int(aoff[-1]) if n else 0
            owner = None
            if lent is not None and ops_ptr.value == lent._address:
                # written in place: the earlier result's buffer, owned as before (and seen through its arrays too)
                owner = lent
                owner._capacity = max(owner._capacity, int(ops_cap.value))
                flat = np.asarray(owner.view(total))
            elif ops_ptr.value:
                # the array takes the malloc'ed buffer over (freed with the array) - no copy
                owner = _MallocBytes(ops_ptr.value, total, int(ops_cap.value))
                flat = np.asarray(owner)
            else:
                flat = np.zeros(0, dtype=np.uint8)
            out.update(start_t=s_t, start_q=s_q, aln_flat=flat, aln_off=aoff,
                       aln=_LazyAlignments(flat, aoff), _ops_owner=owner)
        return out

    def search_pssm(self, row_scores: np.ndarray, consensus: typing.Optional[np.ndarray] = None, gap_open: int = 3,
                    gap_extend: int = 1, mode: str = "score", algorithm: str = "sw", start: int = 0,
                    end: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssm: `search` with a position-specific scoring matrix in the place of (query, matrix).
        ``row_scores``: integers of shape (query length, alphabet length), entry [i, t] the score of query position
        i against target residue t. ``consensus``: one residue per position (or 255, "never a match"); only mode
        "full" reads it, to tell matches from mismatches, and requires it. Returns `search`'s dict."""
        end = self._clamp(end)
        side = self._pssm_side(row_scores, consensus, gap_open, gap_extend, with_consensus=True)

        def call(st, score, et, eq, s_t, s_q, ops_ptr, ops_cap, aoff):
            # (no lending form of this entry point: nothing is reused, the operations come in a buffer of their own)
            return lib().miopalSearchPssm(self._h, *side.queries, *side.scoring, st, MODE[algorithm], start, end,
                                          score, et, eq, s_t, s_q, ctypes.byref(ops_ptr), aoff)
        return self._flat_search(call, mode, max(end - start, 0))

    def search_batch(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray, gap_open: int = 3,
                     gap_extend: int = 1, mode: str = "score", algorithm: str = "sw", start: int = 0,
                     end: typing.Optional[int] = None) -> typing.Dict[str, np.ndarray]:
        """miopalSearchBatch: every query (encoded residues) against the slice [start, end). Returns 2-D int32
        arrays of shape (len(queries), end - start): "score", and for mode "end" also "end_t" / "end_q"; row i
        equals search(queries[i], ...). Mode "full" is refused (OPAL_ERR_INVALID_MODE)."""
        end = self._clamp(end)
        side = self._batch_side(queries, matrix, gap_open, gap_extend)
        shape = (side.rows, max(end - start, 0))
        out = {"score": np.empty(shape, dtype=np.int32)}
        if SEARCH[mode] >= 1:
            out.update(end_t=np.empty(shape, dtype=np.int32), end_q=np.empty(shape, dtype=np.int32))
        rc = lib().miopalSearchBatch(self._h, *side.queries, *side.scoring, SEARCH[mode], MODE[algorithm], start, end,
                                     _ptr(out["score"]), _ptr(out.get("end_t")), _ptr(out.get("end_q")))
        raise_for(rc)
        return out

    # -- top / hits / significant: one body per family, the query side an argument --------------------------------
    def _search_top(self, side: _QuerySide, mode, algorithm, start, end, k, min_score) -> typing.Dict[str, typing.Any]:
        shape = (k,) if side.rows is None else (side.rows, k)
        out = {"count": np.zeros(1 if side.rows is None else side.rows, dtype=np.int32),
               "target": np.empty(shape, dtype=np.int64), "score": np.empty(shape, dtype=np.int32)}
        if mode == "end":
            out.update(end_t=np.empty(shape, dtype=np.int32), end_q=np.empty(shape, dtype=np.int32))
        rc = getattr(lib(), f"miopalSearch{side.name}Top")(
            self._h, *side.queries, *side.scoring, SEARCH[mode], MODE[algorithm], start, self._clamp(end), k,
            _floor(min_score), _ptr(out["count"]), _ptr(out["target"]), _ptr(out["score"]), _ptr(out.get("end_t")),
            _ptr(out.get("end_q")))
        raise_for(rc)
        if side.rows is None:
            out["count"] = int(out["count"][0])
        return out

    def _search_hits(self, side: _QuerySide, mode, algorithm, start, end, min_score, max_hits):
        single = side.rows is None
        if single:
            cut = _floor(min_score)
        else:
            thresholds = np.ascontiguousarray(np.broadcast_to(np.asarray(_floor(min_score), dtype=np.int32), (side.rows,)))
            cut = _ptr(thresholds) if side.rows else None
        counts = ctypes.c_int64(-1) if single else np.zeros(side.rows + 1, dtype=np.int64)
        ptrs = _HitPointers()
        rc = getattr(lib(), f"miopalSearch{side.name}Hits")(
            self._h, *side.queries, *side.scoring, SEARCH[mode], MODE[algorithm], start, self._clamp(end), cut,
            _bound(max_hits), ctypes.byref(counts) if single else _ptr(counts), *ptrs.refs())
        return self._found(rc, counts, ptrs, mode)

    def _search_significant(self, side: _QuerySide, mode, algorithm, start, end, max_evalue, exclude_z, max_hits):
        # what the C side refuses, refused before it is reached: a cut that is not finite and positive, a NaN
        cuts = np.atleast_1d(np.asarray(max_evalue, dtype=np.float64))
        if not np.all(np.isfinite(cuts)) or not np.all(cuts > 0):
            raise ValueError("max_evalue must be finite and positive")
        if np.isnan(float(exclude_z)):
            raise ValueError("exclude_z must not be NaN")
        single = side.rows is None
        if single:
            cut = float(max_evalue)
        else:
            cuts = np.ascontiguousarray(np.broadcast_to(cuts, (side.rows,)))
            cut = _ptr(cuts) if side.rows else None
        fits = (ScoreFit * max(side.rows or 1, 1))()
        fit = {"fit": fits[0]} if single else {"fits": [fits[i] for i in range(side.rows)]}
        counts = ctypes.c_int64(-1) if single else np.zeros(side.rows + 1, dtype=np.int64)
        ptrs, ev = _HitPointers(), ctypes.c_void_p()
        rc = getattr(lib(), f"miopalSearch{side.name}Significant")(
            self._h, *side.queries, *side.scoring, SEARCH[mode], MODE[algorithm], start, self._clamp(end), cut,
            float(exclude_z), _bound(max_hits), ctypes.addressof(fits), ctypes.byref(counts) if single else _ptr(counts),
            *ptrs.refs(), ctypes.byref(ev))
        out = self._found(rc, counts, ptrs, mode, fit)
        out["evalue"] = _take_malloced(ev, len(out["target"]), np.float64)
        out.update(fit)
        if not single:
            out["_fits_owner"] = fits
        return out

    @staticmethod
    def _found(rc, counts, ptrs, mode, fit=None) -> typing.Dict[str, typing.Any]:
        """What a hit search found. One query (``counts`` a c_int64): "count" and the arrays; a list (``counts`` the
        offsets): the CSR with "offsets". TooManyHits carries the count or the offsets as ``counts``, and the fit(s) of
        a significance search as ``fit`` / ``fits``."""
        single = isinstance(counts, ctypes.c_int64)
        found = int(counts.value) if single else counts
        if rc == MIOPAL_ERR_TOO_MANY_HITS:
            err = TooManyHits(f"more hits than max_hits (code={rc}): {last_error()}", found)
            vars(err).update(fit or {})
            raise err
        raise_for(rc)
        out = {"count": found} if single else {"offsets": found}
        out.update(ptrs.arrays(found if single else int(found[-1]), mode == "end"))
        return out

    def search_top(self, query: np.ndarray, matrix: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                   mode: str = "score", algorithm: str = "sw", start: int = 0, end: typing.Optional[int] = None,
                   k: int = 10, min_score: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchTop: the k best targets of the slice, selected on the device. Returns "count" (an int),
        "target" (int64, absolute indices), "score" and for mode "end" "end_t" / "end_q", arrays of shape (k,):
        best first (score descending, index ascending), -1 past the count. ``min_score``: only targets scoring at
        least that many count (None: no bound). Mode "full" is refused (OPAL_ERR_INVALID_MODE)."""
        return self._search_top(self._query_side(query, matrix, gap_open, gap_extend), mode, algorithm, start, end, k, min_score)

    def search_pssm_top(self, row_scores: np.ndarray, gap_open: int = 3, gap_extend: int = 1, mode: str = "score",
                        algorithm: str = "sw", start: int = 0, end: typing.Optional[int] = None, k: int = 10,
                        min_score: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssmTop: `search_top` with a position-specific scoring matrix (``row_scores`` as in
        `search_pssm`) in the place of (query, matrix). Returns `search_top`'s dict; entry i equals what
        `search_pssm` gives for ``target[i]``."""
        return self._search_top(self._pssm_side(row_scores, None, gap_open, gap_extend), mode, algorithm, start, end, k, min_score)

    def _pssm_batch_side(self, pssm_rows, consensus, gap_open, gap_extend, with_consensus=False) -> _QuerySide:
        """a list of PSSMs as miopalAlignPairsPssm takes it: the rows end to end, [the consensus,] the row offsets"""
        rows = [_pssm_rows(r, self.alphabet_length, "every PSSM must have shape (rows") for r in pssm_rows]
        flat, offsets = _packed(rows, None)
        cons = None
        if consensus is not None:
            cs = [np.ascontiguousarray(c, dtype=np.uint8).ravel() for c in consensus]
            if [len(c) for c in cs] != [len(r) for r in rows]:
                raise ValueError("consensus must have one entry per row of every PSSM")
            cons = np.concatenate(cs) if offsets[-1] else None
        pointers = (_ptr(flat),) + ((_ptr(cons),) if with_consensus else ()) + (_ptr(offsets), len(rows))
        return _QuerySide("PssmBatch", pointers, (gap_open, gap_extend, self.alphabet_length), len(rows), None,
                          (flat, offsets, cons))

    def search_batch_top(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray, gap_open: int = 3,
                         gap_extend: int = 1, mode: str = "score", algorithm: str = "sw", start: int = 0,
                         end: typing.Optional[int] = None, k: int = 10,
                         min_score: typing.Optional[int] = None) -> typing.Dict[str, np.ndarray]:
        """miopalSearchBatchTop: search_top of every query in one batched call. "count" has one entry per query;
        the other arrays have shape (len(queries), k); row i equals search_top(queries[i], ...)."""
        return self._search_top(self._batch_side(queries, matrix, gap_open, gap_extend), mode, algorithm, start, end, k, min_score)

    def search_hits(self, query: np.ndarray, matrix: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                    mode: str = "score", algorithm: str = "sw", start: int = 0, end: typing.Optional[int] = None,
                    min_score: typing.Optional[int] = None,
                    max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchHits: every target of the slice scoring at least ``min_score`` (None: every target), compacted
        on the device. Returns "count" (an int), "target" (int64, absolute indices, ascending), "score" and for mode
        "end" "end_t" / "end_q", arrays of count entries that own the buffers the library allocated. With more than
        ``max_hits`` hits (None: no bound): TooManyHits, its ``counts`` the number of hits. Mode "full" is refused
        (OPAL_ERR_INVALID_MODE)."""
        return self._search_hits(self._query_side(query, matrix, gap_open, gap_extend), mode, algorithm, start, end, min_score, max_hits)

    def search_pssm_hits(self, row_scores: np.ndarray, gap_open: int = 3, gap_extend: int = 1, mode: str = "score",
                         algorithm: str = "sw", start: int = 0, end: typing.Optional[int] = None,
                         min_score: typing.Optional[int] = None,
                         max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssmHits: `search_hits` with a position-specific scoring matrix (``row_scores`` as in
        `search_pssm`) in the place of (query, matrix). Returns `search_hits`' dict; hit i equals what `search_pssm`
        gives for ``target[i]``."""
        return self._search_hits(self._pssm_side(row_scores, None, gap_open, gap_extend), mode, algorithm, start, end, min_score, max_hits)

    def search_batch_hits(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray, gap_open: int = 3,
                          gap_extend: int = 1, mode: str = "score", algorithm: str = "sw", start: int = 0,
                          end: typing.Optional[int] = None, min_score=None,
                          max_hits: typing.Optional[int] = None) -> typing.Dict[str, np.ndarray]:
        """miopalSearchBatchHits: search_hits of every query in one batched call. ``min_score``: an integer, one per
        query, or None. Returns a CSR: "offsets" (len(queries) + 1,) and "target", "score" (and "end_t" / "end_q") of
        offsets[-1] entries; entries offsets[i]:offsets[i + 1] equal search_hits(queries[i], ...). ``max_hits`` bounds
        the total; TooManyHits carries the offsets in ``counts``."""
        return self._search_hits(self._batch_side(queries, matrix, gap_open, gap_extend), mode, algorithm, start, end, min_score, max_hits)

    select_hits_rows = staticmethod(select_hits_rows)

    def _search_occurrences(self, side: _QuerySide, algorithm, start, end, min_score, window, max_hits):
        _check_occurrence_rule(algorithm, min_score, window)
        counts = ctypes.c_int64(-1)
        ptrs = _HitPointers()
        rc = getattr(lib(), f"miopalSearch{side.name}Occurrences")(
            self._h, *side.queries, *side.scoring, MODE[algorithm], start, self._clamp(end), min_score,
            side.length if window is None else window, _bound(max_hits), ctypes.byref(counts), *ptrs.refs())
        return self._found(rc, counts, ptrs, "end")

    def _search_occurrence_alignments(self, side: _QuerySide, algorithm, start, end, min_score, window, max_hits,
                                      operations):
        _check_occurrence_rule(algorithm, min_score, window)
        counts = ctypes.c_int64(-1)
        ptrs = _HitPointers()
        more = _AlignedPointers(operations)
        rc = getattr(lib(), f"miopalSearch{side.name}OccurrencesAligned")(
            self._h, *side.queries, *side.scoring, MODE[algorithm], start, self._clamp(end), min_score,
            side.length if window is None else window, _bound(max_hits), ctypes.byref(counts), *ptrs.refs(), *more.refs())
        out = self._found(rc, counts, ptrs, "end")
        out.update(more.arrays(out["count"]))
        return out

    def search_occurrences(self, query: np.ndarray, matrix: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                           algorithm: str = "hw", start: int = 0, end: typing.Optional[int] = None, min_score: int = 1,
                           window: typing.Optional[int] = None,
                           max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchOccurrences: every occurrence of the query in each target of the slice - the columns where the
        last row of "hw" (the column maximum of "sw") reaches ``min_score``, thinned by greedy peak picking so that two
        occurrences of a target lie more than ``window`` columns apart (None: the query's length; 0: every such
        column). Returns "count" (an int) and "target" (int64, absolute, ascending; a target may appear several
        times), "score", "end_t" (the column, ascending inside a target) and "end_q" (the row), arrays of count entries
        that own the buffers the library allocated. With more than ``max_hits`` occurrences: TooManyHits, its
        ``counts`` their number. An algorithm other than "hw" and "sw", a negative window and ``min_score < 1`` with
        "sw" raise ValueError before any device call."""
        return self._search_occurrences(self._query_side(query, matrix, gap_open, gap_extend), algorithm, start, end,
                                        min_score, window, max_hits)

    def search_occurrences_pssm(self, row_scores: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                                algorithm: str = "hw", start: int = 0, end: typing.Optional[int] = None,
                                min_score: int = 1, window: typing.Optional[int] = None,
                                max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssmOccurrences: `search_occurrences` with a position-specific scoring matrix (``row_scores`` as
        in `search_pssm`) in the place of (query, matrix); PSSMs too tall for the sweep's LDS table are refused."""
        return self._search_occurrences(self._pssm_side(row_scores, None, gap_open, gap_extend), algorithm, start, end,
                                        min_score, window, max_hits)

    def search_occurrence_alignments(self, query: np.ndarray, matrix: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                                     algorithm: str = "hw", start: int = 0, end: typing.Optional[int] = None,
                                     min_score: int = 1, window: typing.Optional[int] = None,
                                     max_hits: typing.Optional[int] = None,
                                     operations: bool = True) -> typing.Dict[str, typing.Any]:
        """miopalSearchOccurrencesAligned: `search_occurrences` with the other end of every occurrence. Returns
        `search_occurrences`' dict - the same arrays, byte for byte - plus "start_t" and "start_q" (where occurrence k
        begins in its target and in the query; the checker's start rule applied to the occurrence's end cell) and, with
        ``operations``, "aln_flat", "aln_off" and "aln": the operations of occurrence k are
        ``aln_flat[aln_off[k]:aln_off[k + 1]]``, encoded as `align_pairs` encodes them. ``operations=False``: starts
        only - no direction pass, no walk, no operation traffic - and no "aln*" keys."""
        return self._search_occurrence_alignments(self._query_side(query, matrix, gap_open, gap_extend), algorithm, start,
                                                  end, min_score, window, max_hits, operations)

    def search_occurrence_alignments_pssm(self, row_scores: np.ndarray, consensus: typing.Optional[np.ndarray] = None,
                                          gap_open: int = 3, gap_extend: int = 1, algorithm: str = "hw", start: int = 0,
                                          end: typing.Optional[int] = None, min_score: int = 1,
                                          window: typing.Optional[int] = None, max_hits: typing.Optional[int] = None,
                                          operations: bool = True) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssmOccurrencesAligned: `search_occurrence_alignments` with a position-specific scoring matrix
        (``row_scores`` and ``consensus`` as in `search_pssm`) in the place of (query, matrix). The consensus tells
        matches from mismatches and is required with ``operations`` (the C side refuses a call without one)."""
        return self._search_occurrence_alignments(
            self._pssm_side(row_scores, consensus, gap_open, gap_extend, with_consensus=True), algorithm, start, end,
            min_score, window, max_hits, operations)

    def search_batch_occurrences(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray, gap_open: int = 3,
                                 gap_extend: int = 1, algorithm: str = "hw", start: int = 0,
                                 end: typing.Optional[int] = None, min_score=1, window=None,
                                 max_hits: typing.Optional[int] = None) -> typing.Dict[str, np.ndarray]:
        """miopalSearchBatchOccurrences: `search_occurrences` of every query of a panel in one call. ``min_score`` and
        ``window``: one value or one per query; a window of None is that query's length. Returns a CSR: "offsets"
        (len(queries) + 1,) and "target", "score", "end_t", "end_q" of offsets[-1] entries; entries
        offsets[i]:offsets[i + 1] equal search_occurrences(queries[i], ...) byte for byte. ``max_hits`` bounds the
        total; TooManyHits carries the offsets in ``counts``. The rule's faults raise ValueError before any device
        call, as `search_occurrences`' do."""
        return self._search_batch_occurrences(self._batch_side(queries, matrix, gap_open, gap_extend), algorithm, start, end,
                                              min_score, window, max_hits)

    def search_batch_occurrences_pssm(self, row_scores: typing.Sequence[np.ndarray], gap_open: int = 3,
                                      gap_extend: int = 1, algorithm: str = "hw", start: int = 0,
                                      end: typing.Optional[int] = None, min_score=1, window=None,
                                      max_hits: typing.Optional[int] = None) -> typing.Dict[str, np.ndarray]:
        """miopalSearchPssmBatchOccurrences: `search_batch_occurrences` with a panel of position-specific scoring
        matrices (``row_scores[m]``: integers of shape (rows of PSSM m, alphabet length)) in the place of (queries,
        matrix). Returns `search_batch_occurrences`' dict; entries offsets[i]:offsets[i + 1] equal
        search_occurrences_pssm(row_scores[i], ...) byte for byte. A window of None is that PSSM's height."""
        return self._search_batch_occurrences(self._pssm_batch_side(row_scores, None, gap_open, gap_extend), algorithm, start,
                                              end, min_score, window, max_hits)

    def _search_batch_occurrences(self, side: _QuerySide, algorithm, start, end, min_score, window, max_hits, operations=None):
        """The panel occurrence searches, plain and PSSM: the per-query cuts and windows, the rule's faults, and the call of
        miopalSearch<side>Occurrences or, with ``operations`` (a bool: the aligned outputs with or without the operations), ...OccurrencesAligned."""
        more = None if operations is None else _AlignedPointers(operations)
        lengths = np.diff(side.keep[1]).tolist()
        cuts, windows = _per_query(min_score, lengths, "min_score"), _per_query(window, lengths, "window")
        _check_occurrence_rule(algorithm, cuts.min(initial=1), windows.min(initial=0))   # (a panel's smallest decide)
        if len(cuts) and (cuts.min() < -(2 ** 31) or cuts.max() >= 2 ** 31 or windows.max() >= 2 ** 31):
            raise OverflowError("min_score / window does not fit a 32-bit integer")
        cuts, windows = cuts.astype(np.int32), windows.astype(np.int32)
        offsets = np.zeros(side.rows + 1, dtype=np.int64)
        ptrs = _HitPointers()
        rc = getattr(lib(), f"miopalSearch{side.name}Occurrences" + ("Aligned" if more else ""))(
            self._h, *side.queries, *side.scoring, MODE[algorithm], start, self._clamp(end),
            _ptr(cuts) if side.rows else None, _ptr(windows) if side.rows else None, _bound(max_hits),
            _ptr(offsets), *ptrs.refs(), *(more.refs() if more else ()))
        out = self._found(rc, offsets, ptrs, "end")
        if more:
            out.update(more.arrays(int(offsets[-1])))
        return out

    def search_batch_occurrence_alignments(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray,
                                           gap_open: int = 3, gap_extend: int = 1, algorithm: str = "hw", start: int = 0,
                                           end: typing.Optional[int] = None, min_score=1, window=None,
                                           max_hits: typing.Optional[int] = None,
                                           operations: bool = True) -> typing.Dict[str, typing.Any]:
        """miopalSearchBatchOccurrencesAligned: `search_occurrence_alignments` of every query of a panel in one call.
        Returns `search_batch_occurrences`' dict - the same arrays, byte for byte - plus "start_t" and "start_q" and,
        with ``operations``, "aln_flat", "aln_off" (offsets[-1] + 1 entries, rebased to start at 0) and "aln": entries
        offsets[i]:offsets[i + 1] equal search_occurrence_alignments(queries[i], ...). ``operations=False``: starts
        only, and no "aln*" keys. ``max_hits`` bounds the total; TooManyHits carries the offsets in ``counts``, and
        what had been aligned by then is discarded."""
        return self._search_batch_occurrences(self._batch_side(queries, matrix, gap_open, gap_extend), algorithm, start, end,
                                              min_score, window, max_hits, operations)

    def search_batch_occurrence_alignments_pssm(self, row_scores: typing.Sequence[np.ndarray],
                                                consensus: typing.Optional[typing.Sequence[np.ndarray]] = None,
                                                gap_open: int = 3, gap_extend: int = 1, algorithm: str = "hw",
                                                start: int = 0, end: typing.Optional[int] = None, min_score=1,
                                                window=None, max_hits: typing.Optional[int] = None,
                                                operations: bool = True) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssmBatchOccurrencesAligned: `search_batch_occurrence_alignments` with a panel of PSSMs
        (``row_scores`` as in `search_batch_occurrences_pssm`; ``consensus[m]``: one residue or 255 per row of PSSM m,
        required with ``operations``) in the place of (queries, matrix). Entries offsets[i]:offsets[i + 1] equal
        search_occurrence_alignments_pssm(row_scores[i], consensus[i], ...)."""
        side = self._pssm_batch_side(row_scores, consensus, gap_open, gap_extend, with_consensus=True)
        return self._search_batch_occurrences(side, algorithm, start, end, min_score, window, max_hits, operations)

    pick_occurrences_rows = staticmethod(pick_occurrences_rows)
    last_occurrence_routing = staticmethod(last_occurrence_routing)
    last_batch_occurrence_routing = staticmethod(last_batch_occurrence_routing)
    last_batch_occurrence_groups = staticmethod(last_batch_occurrence_groups)
    last_batch_occurrence_align_routing = staticmethod(last_batch_occurrence_align_routing)
    last_occurrence_align_routing = staticmethod(last_occurrence_align_routing)

    def search_significant(self, query: np.ndarray, matrix: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                           mode: str = "score", algorithm: str = "sw", start: int = 0,
                           end: typing.Optional[int] = None, max_evalue: float = 1e-3, exclude_z: float = 5.0,
                           max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchSignificant: every target of the slice with an E-value of at most ``max_evalue``, the
        statistics gathered on the device from the search's own scores. Returns `search_hits`' dict plus "evalue"
        (float64, one per hit) and "fit" (a `ScoreFit` structure). TooManyHits carries the fit as ``fit``."""
        return self._search_significant(self._query_side(query, matrix, gap_open, gap_extend), mode, algorithm, start, end, max_evalue, exclude_z,
                                        max_hits)

    def search_pssm_significant(self, row_scores: np.ndarray, gap_open: int = 3, gap_extend: int = 1,
                                mode: str = "score", algorithm: str = "sw", start: int = 0,
                                end: typing.Optional[int] = None, max_evalue: float = 1e-3, exclude_z: float = 5.0,
                                max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchPssmSignificant: `search_significant` with a position-specific scoring matrix (``row_scores``
        as in `search_pssm`) in the place of (query, matrix)."""
        return self._search_significant(self._pssm_side(row_scores, None, gap_open, gap_extend), mode, algorithm, start, end, max_evalue, exclude_z,
                                        max_hits)

    def search_batch_significant(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray, gap_open: int = 3,
                                 gap_extend: int = 1, mode: str = "score", algorithm: str = "sw", start: int = 0,
                                 end: typing.Optional[int] = None, max_evalue=1e-3, exclude_z: float = 5.0,
                                 max_hits: typing.Optional[int] = None) -> typing.Dict[str, typing.Any]:
        """miopalSearchBatchSignificant: search_significant of every query in one batched call. ``max_evalue``: a
        number or one per query. Returns `search_batch_hits`' CSR plus "evalue" and "fits" (a list of `ScoreFit`
        structures, one per query). TooManyHits carries the offsets in ``counts`` and the fits in ``fits``."""
        return self._search_significant(self._batch_side(queries, matrix, gap_open, gap_extend), mode, algorithm, start, end, max_evalue, exclude_z,
                                        max_hits)

    row_stats_rows = staticmethod(row_stats_rows)
    select_hits_binned_rows = staticmethod(select_hits_binned_rows)

    def search_batch_target_top(self, queries: typing.Sequence[np.ndarray], matrix: np.ndarray, gap_open: int = 3,
                                gap_extend: int = 1, mode: str = "score", algorithm: str = "sw", start: int = 0,
                                end: typing.Optional[int] = None, m: int = 1,
                                min_score: typing.Optional[int] = None) -> typing.Dict[str, np.ndarray]:
        """miopalSearchBatchTargetTop: the ``m`` best queries of every target of the slice, selected on the device.
        Returns "count" (end - start,), "query" (int32, indices into ``queries``), "score" and for mode "end" "end_t" /
        "end_q", arrays of shape (end - start, m): best first (score descending, query index ascending), -1 past the
        count. ``min_score``: only queries scoring at least that many count (None: no bound). Row t equals the
        reduction of column t of `search_batch`. Mode "full" is refused (OPAL_ERR_INVALID_MODE)."""
        end = self._clamp(end)
        side = self._batch_side(queries, matrix, gap_open, gap_extend)
        n = max(end - start, 0)
        shape = (n, max(m, 0))
        out = {"count": np.zeros(n, dtype=np.int32), "query": np.empty(shape, dtype=np.int32),
               "score": np.empty(shape, dtype=np.int32)}
        if mode == "end":
            out.update(end_t=np.empty(shape, dtype=np.int32), end_q=np.empty(shape, dtype=np.int32))
        rc = lib().miopalSearchBatchTargetTop(self._h, *side.queries, *side.scoring, SEARCH[mode], MODE[algorithm], start,
                                              end, m, _floor(min_score), _ptr(out["count"]), _ptr(out["query"]),
                                              _ptr(out["score"]), _ptr(out.get("end_t")), _ptr(out.get("end_q")))
        raise_for(rc)
        return out

    select_columns_rows = staticmethod(select_columns_rows)

    def align_pairs(self, queries: typing.Sequence[np.ndarray], pair_query, pair_target, matrix: np.ndarray,
                    gap_open: int = 3, gap_extend: int = 1, mode: str = "score",
                    algorithm: str = "sw") -> typing.Dict[str, typing.Any]:
        """miopalAlignPairs: pair p aligns ``queries[pair_query[p]]`` (encoded residues) with target
        ``pair_target[p]`` (absolute index), in one call. Returns `search`'s keys with one entry per pair, in pair
        order: "score", for "end" and "full" also "end_t" / "end_q", for "full" also "start_t" / "start_q",
        "aln_flat", "aln_off" and "aln"; entry p equals ``search(queries[i], ..., start=j, end=j + 1)``."""
        side = self._batch_side(queries, matrix, gap_open, gap_extend)

        def call(st, pq, pt, n, score, et, eq, s_t, s_q, ops_ptr, aoff):
            return lib().miopalAlignPairs(self._h, *side.queries, pq, pt, n, *side.scoring, st, MODE[algorithm], score, et,
                                          eq, s_t, s_q, ctypes.byref(ops_ptr), aoff)
        return self._pair_list(call, pair_query, pair_target, mode)

    def align_pairs_pssm(self, pssm_rows: typing.Sequence[np.ndarray],
                         consensus: typing.Optional[typing.Sequence[np.ndarray]], pair_pssm, pair_target,
                         gap_open: int = 3, gap_extend: int = 1, mode: str = "score",
                         algorithm: str = "sw") -> typing.Dict[str, typing.Any]:
        """miopalAlignPairsPssm: `align_pairs` with a list of position-specific scoring matrices in the place of
        (queries, matrix). ``pssm_rows[m]``: integers of shape (rows of PSSM m, alphabet length); ``consensus[m]``:
        one residue (or 255) per row of PSSM m - required for mode "full", may be None otherwise. Pair p aligns PSSM
        ``pair_pssm[p]`` with target ``pair_target[p]``; returns `align_pairs`' dict, entry p equal to
        ``search_pssm(pssm_rows[i], consensus[i], ..., start=j, end=j + 1)``."""
        side = self._pssm_batch_side(pssm_rows, consensus, gap_open, gap_extend, with_consensus=True)

        def call(st, pq, pt, n, score, et, eq, s_t, s_q, ops_ptr, aoff):
            return lib().miopalAlignPairsPssm(self._h, *side.queries, pq, pt, n,
                                              gap_open, gap_extend, self.alphabet_length, st, MODE[algorithm], score,
                                              et, eq, s_t, s_q, ctypes.byref(ops_ptr), aoff)
        return self._pair_list(call, pair_pssm, pair_target, mode)

    def profile_columns(self, query: np.ndarray, matrix: np.ndarray, targets, gap_open: int = 3, gap_extend: int = 1,
                        algorithm: str = "sw", return_msa: bool = False) -> typing.Dict[str, typing.Any]:
        """miopalProfileColumns: the alignments of ``query`` (encoded residues) with the targets ``targets`` (absolute
        indices, any order, repeats allowed) - `align_pairs`' in mode "full" - projected onto the query's rows, counted
        and weighted on the device. Returns "counts" and "weighted" (int64, (Q, alphabet length + 1), the last column
        the gap letter), "member_weights" (int64, one per member, the query first; 32.32 fixed point) and "msa" (uint8,
        (members, Q); None unless ``return_msa``)."""
        return self._profile(self._query_side(query, matrix, gap_open, gap_extend, null_when_empty=True), algorithm, targets,
                             return_msa)

    def profile_columns_pssm(self, row_scores: np.ndarray, consensus: np.ndarray, targets, gap_open: int = 3,
                             gap_extend: int = 1, algorithm: str = "sw",
                             return_msa: bool = False) -> typing.Dict[str, typing.Any]:
        """miopalProfileColumnsPssm: `profile_columns` with a position-specific scoring matrix (``row_scores``: integers
        of shape (Q, alphabet length); ``consensus``: one residue or 255 per row, the query's own row of the multiple
        alignment) in the place of (query, matrix)."""
        side = self._pssm_side(row_scores, consensus, gap_open, gap_extend, with_consensus=True,
                               shape="row_scores must have shape (positions", per_row="consensus must have one entry per row")
        return self._profile(side, algorithm, targets, return_msa)

    def _profile(self, side: _QuerySide, algorithm, targets, return_msa) -> typing.Dict[str, typing.Any]:
        """One profile call (miopalProfileColumns, miopalProfileColumnsPssm) and its outputs."""
        pt = np.ascontiguousarray(targets, dtype=np.int64).ravel()
        n, q = len(pt), side.length
        width = self.alphabet_length + 1
        out = {"counts": np.zeros((q, width), dtype=np.int64), "weighted": np.zeros((q, width), dtype=np.int64),
               "member_weights": np.zeros(n + 1, dtype=np.int64),
               "msa": np.full((n + 1, q), PROFILE_UNCOVERED, dtype=np.uint8) if return_msa else None}
        rc = getattr(lib(), f"miopalProfileColumns{side.name}")(
            self._h, *side.queries, *side.scoring, MODE[algorithm], _ptr(pt) if n else None, n, _ptr(out["counts"]),
            _ptr(out["weighted"]), _ptr(out["member_weights"]), _ptr(out["msa"]))
        raise_for(rc)
        return out

    def _pair_list(self, call, pair_query, pair_target, mode) -> typing.Dict[str, typing.Any]:
        """The outputs of one pair-list call (`align_pairs`, `align_pairs_pssm`): ``call(search type, pair queries,
        pair targets, pairs, score, end_t, end_q, start_t, start_q, ops_ptr, offsets)`` makes the C call with these
        pointers and returns its code."""
        pq = np.ascontiguousarray(pair_query, dtype=np.int32).ravel()
        pt = np.ascontiguousarray(pair_target, dtype=np.int64).ravel()
        if len(pq) != len(pt):
            raise ValueError("pair_query and pair_target differ in length")
        n = len(pq)
        st = SEARCH[mode]
        out = {"score": np.empty(n, dtype=np.int32)}
        et = eq = s_t = s_q = aoff = None
        ops_ptr = ctypes.c_void_p()
        if st >= 1:
            et = np.empty(n, dtype=np.int32)
            eq = np.empty(n, dtype=np.int32)
        if st == 2:
            s_t = np.empty(n, dtype=np.int32)
            s_q = np.empty(n, dtype=np.int32)
            aoff = np.zeros(n + 1, dtype=np.int64)
        rc = call(st, _ptr(pq) if n else None, _ptr(pt) if n else None, n, _ptr(out["score"]), _ptr(et), _ptr(eq),
                  _ptr(s_t), _ptr(s_q), ops_ptr, _ptr(aoff))
        raise_for(rc)
        if st >= 1:
            out.update(end_t=et, end_q=eq)
        if st == 2:
            total = int(aoff[-1])
            if ops_ptr.value:
                flat_ops = np.asarray(_MallocBytes(ops_ptr.value, total))
            else:
                flat_ops = np.zeros(0, dtype=np.uint8)
            out.update(start_t=s_t, start_q=s_q, aln_flat=flat_ops, aln_off=aoff, aln=_LazyAlignments(flat_ops, aoff))
        return out

    @staticmethod
    def last_pair_routing() -> typing.Tuple[int, int, int, int]:
        """(pairs on the lane-per-pair forward kernel, pairs on the wavefront-per-pair kernel, pairs answered without
        a DP, chunks) for the calling thread's most recent align_pairs / align_pairs_pssm."""
        counts = (ctypes.c_int64 * 4)()
        lib().miopalLastPairRouting(counts)
        return tuple(int(c) for c in counts)

    @staticmethod
    def last_batch_routing() -> typing.Tuple[int, int, int, int]:
        """(pairs settled by the batch kernels, pairs on the wavefront-per-pair kernel, queries on the
        single-query path, batch-kernel launches) for the calling thread's most recent search_batch."""
        counts = (ctypes.c_int64 * 4)()
        lib().miopalLastBatchRouting(counts)
        return tuple(int(c) for c in counts)

    def search_device_scores(self, query: np.ndarray, matrix: np.ndarray, device_ptr: int,
                             stream: int = 0, gap_open: int = 3, gap_extend: int = 1,
                             algorithm: str = "sw", start: int = 0,
                             end: typing.Optional[int] = None) -> None:
        end = self._clamp(end)
        q = np.ascontiguousarray(query, dtype=np.uint8)
        S = np.ascontiguousarray(matrix, dtype=np.int32)
        rc = lib().miopalSearchDeviceScores(self._h, _ptr(q), len(q), gap_open, gap_extend, _ptr(S),
                                            self.alphabet_length, MODE[algorithm], start, end,
                                            ctypes.c_void_p(device_ptr), ctypes.c_void_p(stream))
        raise_for(rc)

    @staticmethod
    def last_routing() -> typing.Tuple[int, int, int, int]:
        """(targets on the wavefront-per-pair kernel, reserved, groups of 128 targets on the
        lane-per-target kernel, targets recomputed after leaving the 16-bit range) for the
        calling thread's most recent search."""
        counts = (ctypes.c_int64 * 4)()
        lib().miopalLastRouting(counts)
        return tuple(int(c) for c in counts)

    @staticmethod
    def last_window_plan() -> typing.Tuple[int, int, int, int]:
        """(overlap - 0: no windows -, stride of the view that was used, entries of that view, 1 when the windows
        were merged by key for end locations) for the score pass of the calling thread's most recent search
        (include/miopal.h, miopalLastWindowPlan)."""
        out = (ctypes.c_int64 * 4)()
        lib().miopalLastWindowPlan(out)
        return tuple(int(c) for c in out)

    @staticmethod
    def last_launch_shape() -> typing.Tuple[int, int, int, int]:
        """(compute units the handle sees, workgroups of the main persistent launch - 0: none -, wavefronts per
        workgroup, per-SIMD share of groups - 0: off) for the score pass of the calling thread's most recent search
        (include/miopal.h, miopalLastLaunchShape)."""
        out = (ctypes.c_int64 * 4)()
        lib().miopalLastLaunchShape(out)
        return tuple(int(c) for c in out)

    @staticmethod
    def last_full_routing() -> int:
        """Bits describing the start-cell and direction passes of the calling thread's most recent
        `full` search (include/miopal.h, miopalLastFullRouting)."""
        return int(lib().miopalLastFullRouting())

    def set_profiling(self, enabled: bool) -> None:
        lib().miopalSetProfiling(self._h, 1 if enabled else 0)

    def last_kernel_time(self) -> typing.Tuple[int, float]:
        ms = ctypes.c_float(0)
        n = lib().miopalLastKernelTime(self._h, ctypes.byref(ms))
        return int(n), float(ms.value)
