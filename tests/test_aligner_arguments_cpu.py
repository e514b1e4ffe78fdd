"""CPU tier of the extension entry points of `Aligner` (every public method but `align` and `iterated_search`): one
table of calls that are wrong in exactly one way, each with the exception and the message it must raise, and one
table of empty requests, each answered without a device and with the keys, dtypes and shapes written down here.
Nothing in this module reaches a device: `_capi.lib` raises for its duration."""
import numpy as np
import pytest

import pyopal_amd
from pyopal_amd import Pssm, _capi
from pyopal_amd.lib import BatchResultArrays, ProfileColumns, ResultArrays, ScoreFit, SignificantHits

SEQUENCES = ["MKVLA", "AAAA", "WWW"]
PAIRS = [(0, 1), (1, 0)]
TARGETS = [0, 2]

# name: (query side, the positional arguments after the database, the keywords it takes beside `device`)
ENTRY_POINTS = {
    "scores": ("one", (), "algorithm slice"),
    "align_arrays": ("one", (), "mode algorithm slice"),
    "align_pssm": ("pssm", (), "mode algorithm slice"),
    "align_pssm_arrays": ("pssm", (), "mode algorithm slice"),
    "align_many": ("many", (), "mode algorithm slice"),
    "align_many_arrays": ("many", (), "mode algorithm slice"),
    "align_pairs": ("many", (PAIRS,), "mode algorithm"),
    "align_pairs_pssm": ("pssms", (PAIRS,), "mode algorithm"),
    "profile_columns": ("one", (TARGETS,), "algorithm"),
    "top_hits": ("one", (3,), "mode algorithm slice"),
    "top_hits_many": ("many", (3,), "mode algorithm slice"),
    "top_hits_pssm": ("pssm", (3,), "mode algorithm slice"),
    "best_queries": ("many", (2,), "mode algorithm slice"),
    "best_queries_arrays": ("many", (2,), "mode algorithm slice"),
    "hits": ("one", (3,), "mode algorithm slice"),
    "hits_arrays": ("one", (3,), "mode algorithm slice"),
    "hits_many": ("many", (3,), "mode algorithm slice"),
    "hits_many_arrays": ("many", (3,), "mode algorithm slice"),
    "hits_pssm": ("pssm", (3,), "mode algorithm slice"),
    "hits_pssm_arrays": ("pssm", (3,), "mode algorithm slice"),
    "significant_hits": ("one", (1e-3,), "mode algorithm slice"),
    "significant_hits_arrays": ("one", (1e-3,), "mode algorithm slice"),
    "significant_hits_many": ("many", (1e-3,), "mode algorithm slice"),
    "significant_hits_many_arrays": ("many", (1e-3,), "mode algorithm slice"),
    "significant_hits_pssm": ("pssm", (1e-3,), "mode algorithm slice"),
    "significant_hits_pssm_arrays": ("pssm", (1e-3,), "mode algorithm slice"),
}

TOP = ("top_hits", "top_hits_many", "top_hits_pssm")
BEST = ("best_queries", "best_queries_arrays")
HITS = ("hits", "hits_arrays", "hits_many", "hits_many_arrays", "hits_pssm", "hits_pssm_arrays")
SIGNIFICANT = tuple("significant_" + name for name in HITS)
SLICED = tuple(name for name, (_, _, takes) in ENTRY_POINTS.items() if "slice" in takes)
MODES = ("score", "end", "full")


def side(form):
    return {"one": "MKV", "many": ["MKV", "A"], "pssm": Pssm.from_sequence("MKV"),
            "pssms": [Pssm.from_sequence("MKV"), Pssm.from_sequence("A")]}[form]


DNA = dict(db=lambda: pyopal_amd.Database(["ACGT"], alphabet="ACGT"))
NOT_A_DATABASE = r"Argument 'database' has incorrect type \(expected BaseDatabase, got list\)"
MATRIX_ALPHABET = "database and score matrix have different alphabets"
PSSM_ALPHABET = "database and PSSM have different alphabets"
NEGATIVE = "can't convert negative value to uint32_t"
# the two checks `align_arrays` (and `scores`, which is `align_arrays(...).score`) did not make before it shared the
# other entry points' preamble: a non-database was an AttributeError there, a None query a TypeError of memoryview's.
# These rows accept the earlier error or the family's; every other row is the same before and after.
GAIN = ("scores", "align_arrays")
GAIN_NOT_A_DATABASE = NOT_A_DATABASE + "|object has no attribute 'alphabet'"
GAIN_NONE_QUERY = "Argument 'query' must not be None|memoryview: a bytes-like object is required"

# (fault, entry points ("mode": every one that takes the keyword, ...), what the call changes, exception, message)
# "q": the query side, "db": the database, "args": the positional arguments after the database, the rest: keywords
FAULTS = [
    ("bad mode", "mode", dict(mode="sorted"), ValueError, "invalid search mode: 'sorted'"),
    ("bad algorithm", "algorithm", dict(algorithm="blast"), ValueError, "invalid algorithm: 'blast'"),
    ("negative start", "slice", dict(start=-1), OverflowError, NEGATIVE),
    ("negative end", "slice", dict(end=-1), OverflowError, NEGATIVE),
    ("end < start", "slice", dict(start=2, end=1), IndexError, "database slice end is lower than start"),
    ("start past the end", "slice", dict(start=10), IndexError, "database slice start is past the end of the database"),
    ("non-database", "all but gains", dict(db=lambda: ["MKV"]), TypeError, NOT_A_DATABASE),
    ("non-database (gain)", GAIN, dict(db=lambda: ["MKV"]), (TypeError, AttributeError), GAIN_NOT_A_DATABASE),
    ("alphabet mismatch", "one", DNA, ValueError, MATRIX_ALPHABET),
    ("alphabet mismatch", "many", DNA, ValueError, MATRIX_ALPHABET),
    ("alphabet mismatch", "pssm", DNA, ValueError, PSSM_ALPHABET),
    ("alphabet mismatch", "pssms", DNA, ValueError, PSSM_ALPHABET),
    ("alphabet mismatch of a Pssm", ("profile_columns",), dict(q=Pssm.from_sequence("MKV"), **DNA), ValueError,
     PSSM_ALPHABET),
    ("None query", "one but gains", dict(q=None), TypeError, "Argument 'query' must not be None"),
    ("None query (gain)", GAIN, dict(q=None), TypeError, GAIN_NONE_QUERY),
    ("None query", "many", dict(q=["MKV", None]), TypeError, "Argument 'query' must not be None"),
    ("non-Pssm", "pssm", dict(q="MKV"), TypeError, r"Argument 'pssm' has incorrect type \(expected Pssm, got str\)"),
    ("None Pssm", "pssm", dict(q=None), TypeError, r"Argument 'pssm' has incorrect type \(expected Pssm, got NoneType\)"),
    ("non-Pssm", "pssms", dict(q=[Pssm.from_sequence("MKV"), "A"]), TypeError,
     r"Argument 'pssms' has an item of incorrect type \(expected Pssm, got str\)"),
    ("alignments of a batch", ("align_many_arrays",), dict(mode="full"), ValueError,
     "align_many_arrays computes scores and end locations only"),
    # k
    ("k negative", TOP, dict(args=(-1,)), ValueError, r"k must be between 0 and 4096 \(MIOPAL_MAX_TOP\), got -1"),
    ("k too large", TOP, dict(args=(4097,)), ValueError, r"k must be between 0 and 4096 \(MIOPAL_MAX_TOP\), got 4097"),
    ("k a float", TOP, dict(args=(2.0,)), TypeError, "k must be an integer, not float"),
    ("k a bool", TOP, dict(args=(True,)), TypeError, "k must be an integer, not bool"),
    ("k None", TOP, dict(args=(None,)), TypeError, "k must be an integer, not NoneType"),
    # m
    ("m zero", BEST, dict(args=(0,)), ValueError, r"m must be between 1 and 8 \(MIOPAL_MAX_TARGET_TOP\), got 0"),
    ("m too large", BEST, dict(args=(9,)), ValueError, r"m must be between 1 and 8 \(MIOPAL_MAX_TARGET_TOP\), got 9"),
    ("m a float", BEST, dict(args=(1.0,)), TypeError, "m must be an integer, not float"),
    # max_hits
    ("max_hits negative", HITS + SIGNIFICANT, dict(max_hits=-1), ValueError, "max_hits must not be negative"),
    ("max_hits a float", HITS + SIGNIFICANT, dict(max_hits=1.5), TypeError, "max_hits must be an integer or None, not float"),
    ("max_hits a bool", HITS + SIGNIFICANT, dict(max_hits=True), TypeError, "max_hits must be an integer or None, not bool"),
    # min_score
    ("min_score a float", HITS, dict(args=(1.0,)), TypeError, "min_score must be an integer, not float"),
    ("min_score None", HITS, dict(args=(None,)), TypeError, "min_score must be an integer, not NoneType"),
    ("min_score too large", HITS, dict(args=(2 ** 31,)), OverflowError, "min_score does not fit a 32-bit integer"),
    ("min_score a list for one query", ("hits", "hits_arrays", "hits_pssm", "hits_pssm_arrays"), dict(args=([1],)), TypeError,
     "min_score must be an integer, not list"),
    ("min_score of the wrong count", ("hits_many", "hits_many_arrays"), dict(args=([1, 2, 3],)), ValueError,
     r"min_score must be an integer or hold one per query \(2\), got 3"),
    ("min_score with a float", ("hits_many", "hits_many_arrays"), dict(args=([1, 2.5],)), TypeError,
     "min_score must be an integer, not float"),
    # max_evalue, exclude_z
    ("max_evalue zero", SIGNIFICANT, dict(args=(0.0,)), ValueError, "max_evalue must be finite and positive"),
    ("max_evalue negative", SIGNIFICANT, dict(args=(-1e-3,)), ValueError, "max_evalue must be finite and positive"),
    ("max_evalue infinite", SIGNIFICANT, dict(args=(float("inf"),)), ValueError, "max_evalue must be finite and positive"),
    ("max_evalue NaN", SIGNIFICANT, dict(args=(float("nan"),)), ValueError, "max_evalue must be finite and positive"),
    ("max_evalue a string", SIGNIFICANT, dict(args=("1e-3",)), TypeError, "max_evalue must be a number, not str"),
    ("max_evalue of the wrong count", ("significant_hits_many", "significant_hits_many_arrays"), dict(args=([1e-3],)),
     ValueError, r"max_evalue must be a number or hold one per query \(2\), got 1"),
    ("exclude_z NaN", SIGNIFICANT, dict(exclude_z=float("nan")), ValueError, "exclude_z must not be NaN"),
    ("exclude_z a string", SIGNIFICANT, dict(exclude_z="5"), TypeError, "exclude_z must be a number, not str"),
    # pairs
    ("pairs of three", ("align_pairs",), dict(args=([(0, 1, 2)],)), ValueError,
     r"pairs must be a sequence of \(query_index, target_index\) integers"),
    ("pairs of floats", ("align_pairs",), dict(args=([(0.0, 1.0)],)), ValueError,
     r"pairs must be a sequence of \(query_index, target_index\) integers"),
    ("pairs of three", ("align_pairs_pssm",), dict(args=([(0, 1, 2)],)), ValueError,
     r"pairs must be a sequence of \(pssm_index, target_index\) integers"),
    ("pairs flat", ("align_pairs_pssm",), dict(args=([0, 1],)), ValueError,
     r"pairs must be a sequence of \(pssm_index, target_index\) integers"),
    ("query of a pair out of range", ("align_pairs",), dict(args=([(2, 0)],)), IndexError,
     "query index of a pair outside the queries"),
    ("query of a pair negative", ("align_pairs",), dict(args=([(-1, 0)],)), IndexError,
     "query index of a pair outside the queries"),
    ("PSSM of a pair out of range", ("align_pairs_pssm",), dict(args=([(2, 0)],)), IndexError,
     "PSSM index of a pair outside the PSSMs"),
    ("target of a pair out of range", ("align_pairs", "align_pairs_pssm"), dict(args=([(0, 3)],)), IndexError,
     "target index of a pair outside the database"),
    ("target of a pair negative", ("align_pairs", "align_pairs_pssm"), dict(args=([(0, -1)],)), IndexError,
     "target index of a pair outside the database"),
    # targets
    ("targets in two dimensions", ("profile_columns",), dict(args=([[0, 1]],)), ValueError,
     "targets must be a sequence of integer target indices"),
    ("targets of floats", ("profile_columns",), dict(args=([0.5],)), ValueError,
     "targets must be a sequence of integer target indices"),
    ("target out of range", ("profile_columns",), dict(args=([3],)), IndexError, "target index outside the database"),
    ("target negative", ("profile_columns",), dict(args=([-1],)), IndexError, "target index outside the database"),
]


def applies(where, name):
    form, _, takes = ENTRY_POINTS[name]
    if isinstance(where, tuple):
        return name in where
    if where == "all but gains":
        return name not in GAIN
    if where == "one but gains":
        return form == "one" and name not in GAIN
    if where in ("one", "many", "pssm", "pssms"):
        return form == where
    return where in takes.split()


FAULT_ROWS = [pytest.param(name, change, error, message, id=f"{name}-{fault}")
              for fault, where, change, error, message in FAULTS for name in ENTRY_POINTS if applies(where, name)]


@pytest.fixture(scope="module")
def aligner():
    return pyopal_amd.Aligner()


@pytest.fixture(autouse=True)
def no_device(aligner, monkeypatch):
    monkeypatch.setattr(_capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("device reached")))


def call(aligner, name, change):
    form, args, _ = ENTRY_POINTS[name]
    change = dict(change)
    q = change.pop("q", side(form))
    db = change.pop("db", lambda: pyopal_amd.Database(SEQUENCES))()
    args = change.pop("args", args)
    return getattr(aligner, name)(q, db, *args, **change)


def test_the_table_covers_every_extension_entry_point():
    public = {name for name in vars(pyopal_amd.Aligner) if not name.startswith("_")}
    assert public - {"align", "iterated_search"} == set(ENTRY_POINTS)
    assert {row.values[0] for row in FAULT_ROWS} == set(ENTRY_POINTS)


@pytest.mark.parametrize("name, change, error, message", FAULT_ROWS)
def test_one_fault_one_error(aligner, name, change, error, message):
    with pytest.raises(error, match=message):
        call(aligner, name, change)


# --- empty requests ---------------------------------------------------------------------------------------------------

I32, I64, U8, F64 = "int32", "int64", "uint8", "float64"


def entries(mode, n=0):
    """the per-entry arrays of an `*_arrays` dict: key -> (dtype, shape), ``n`` entries each"""
    out = {"score": (I32, (n,))}
    if mode != "score":
        out.update(end_q=(I32, (n,)), end_t=(I32, (n,)))
    if mode == "full":
        out.update(start_q=(I32, (n,)), start_t=(I32, (n,)), aln_flat=(U8, (0,)), aln_off=(I64, (n + 1,)))
    return out


def csr(mode, rows, extra=()):
    """the dict of `hits_arrays` (rows == 1) / `hits_many_arrays` with no hit in it"""
    out = {"offsets": (I64, (rows + 1,)), "target": (I64, (0,))}
    out.update(entries(mode))
    out.update({key: (F64, (0,)) for key in extra})
    return out


def table(mode, n, m):
    """the dict of `best_queries_arrays` over ``n`` targets none of which has a query"""
    out = {"count": (I32, (n,)), "query": (I32, (n, m)), "score": (I32, (n, m))}
    if mode == "end":
        out.update(end_q=(I32, (n, m)), end_t=(I32, (n, m)))
    if mode == "full":
        out["pairs"] = dict(entries("full"), query=(I32, (0,)), target=(I64, (0,)))
    return out


def shape_of(value):
    """what an answer looks like: arrays as (dtype, shape), the containers of this module as dicts of them"""
    if isinstance(value, np.ndarray):
        return (str(value.dtype), value.shape)
    if isinstance(value, dict):
        return {key: shape_of(v) for key, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [shape_of(v) for v in value]
    if isinstance(value, ResultArrays):
        return {"ResultArrays": (value.mode, value.start, value.query_length),
                "target_length": None if value.target_length is None else list(value.target_length),
                **{key: shape_of(getattr(value, key)) for key in
                   ("score", "query_end", "target_end", "query_start", "target_start", "operations", "operation_offsets")}}
    if isinstance(value, BatchResultArrays):
        return {"BatchResultArrays": (value.mode, value.start, value.query_lengths),
                **{key: shape_of(getattr(value, key)) for key in ("score", "query_end", "target_end")}}
    if isinstance(value, SignificantHits):
        return {"SignificantHits": value.results, "evalues": shape_of(value.evalues), "zscores": shape_of(value.zscores),
                "fit": shape_of(value.fit)}
    if isinstance(value, ScoreFit):
        return ("ScoreFit", value.degenerate, value.targets)
    if isinstance(value, ProfileColumns):
        return {"ProfileColumns": value.consensus.tolist(), "members": value.member_weights.tolist(),
                **{key: shape_of(getattr(value, key)) for key in ("counts", "weighted", "msa")}}
    return value


def result_arrays(mode, start, query_length):
    keys = entries(mode)
    return {"ResultArrays": (mode, start, query_length), "target_length": [] if mode == "full" else None,
            "score": keys["score"], "query_end": keys.get("end_q"), "target_end": keys.get("end_t"),
            "query_start": keys.get("start_q"), "target_start": keys.get("start_t"), "operations": keys.get("aln_flat"),
            "operation_offsets": keys.get("aln_off")}


def batch_arrays(mode, start, lengths, n):
    shape = (I32, (len(lengths), n))
    return {"BatchResultArrays": (mode, start, lengths), "score": shape, "query_end": shape if mode == "end" else None,
            "target_end": shape if mode == "end" else None}


NO_FIT = ("ScoreFit", True, 0)


def significant(mode, rows):
    return [{"SignificantHits": [], "evalues": (F64, (0,)), "zscores": (F64, (0,)), "fit": NO_FIT} for _ in range(rows)]


# name: what an empty slice [start, start) gives in ``mode`` (3-residue query / PSSM, the two queries "MKV" and "A")
EMPTY_SLICE = {
    "scores": lambda mode, start: (I32, (0,)),
    "align_arrays": lambda mode, start: result_arrays(mode, start, 3),
    "align_pssm": lambda mode, start: [],
    "align_pssm_arrays": lambda mode, start: result_arrays(mode, start, 3),
    "align_many": lambda mode, start: [[], []],
    "align_many_arrays": lambda mode, start: batch_arrays(mode, start, [3, 1], 0),
    "top_hits": lambda mode, start: [],
    "top_hits_many": lambda mode, start: [[], []],
    "top_hits_pssm": lambda mode, start: [],
    "best_queries": lambda mode, start: [],
    "best_queries_arrays": lambda mode, start: table(mode, 0, 2),
    "hits": lambda mode, start: [],
    "hits_arrays": lambda mode, start: csr(mode, 1),
    "hits_many": lambda mode, start: [[], []],
    "hits_many_arrays": lambda mode, start: csr(mode, 2),
    "hits_pssm": lambda mode, start: [],
    "hits_pssm_arrays": lambda mode, start: csr(mode, 1),
    "significant_hits": lambda mode, start: significant(mode, 1)[0],
    "significant_hits_arrays": lambda mode, start: dict(csr(mode, 1, ("evalue", "zscore")), fit=NO_FIT),
    "significant_hits_many": lambda mode, start: significant(mode, 2),
    "significant_hits_many_arrays": lambda mode, start: dict(csr(mode, 2, ("evalue", "zscore")), fits=[NO_FIT, NO_FIT]),
    "significant_hits_pssm": lambda mode, start: significant(mode, 1)[0],
    "significant_hits_pssm_arrays": lambda mode, start: dict(csr(mode, 1, ("evalue", "zscore")), fit=NO_FIT),
}

# (request, entry point, what the call changes, modes, the answer in ``mode``)
EMPTY = [
    ("k == 0", "top_hits", dict(args=(0,)), MODES, lambda mode: []),
    ("k == 0", "top_hits_many", dict(args=(0,)), MODES, lambda mode: [[], []]),
    ("k == 0", "top_hits_pssm", dict(args=(0,)), MODES, lambda mode: []),
    ("no queries", "align_many", dict(q=[]), MODES, lambda mode: []),
    ("no queries", "align_many_arrays", dict(q=[]), ("score", "end"), lambda mode: batch_arrays(mode, 0, [], 3)),
    ("no queries", "align_pairs", dict(q=[], args=([],)), MODES, lambda mode: []),
    ("no queries", "align_pairs_pssm", dict(q=[], args=([],)), MODES, lambda mode: []),
    ("no queries", "top_hits_many", dict(q=[]), MODES, lambda mode: []),
    ("no queries", "best_queries", dict(q=[]), MODES, lambda mode: [[], [], []]),
    ("no queries", "best_queries_arrays", dict(q=[]), MODES, lambda mode: table(mode, 3, 2)),
    ("no queries", "hits_many", dict(q=[]), MODES, lambda mode: []),
    ("no queries and no thresholds", "hits_many", dict(q=[], args=([],)), MODES, lambda mode: []),
    ("no queries", "hits_many_arrays", dict(q=[]), MODES, lambda mode: csr(mode, 0)),
    ("no queries", "significant_hits_many", dict(q=[]), MODES, lambda mode: []),
    ("no queries", "significant_hits_many_arrays", dict(q=[]), MODES,
     lambda mode: dict(csr(mode, 0, ("evalue", "zscore")), fits=[])),
    ("no pairs", "align_pairs", dict(args=([],)), MODES, lambda mode: []),
    ("no pairs", "align_pairs", dict(args=(np.zeros((0, 2), dtype=np.int64),)), MODES, lambda mode: []),
    ("no pairs", "align_pairs_pssm", dict(args=([],)), MODES, lambda mode: []),
]

EMPTY_ROWS = [pytest.param(name, dict(change, mode=mode), answer(mode), id=f"{name}-{request}-{mode}")
              for request, name, change, modes, answer in EMPTY for mode in modes]
EMPTY_ROWS += [pytest.param(name, dict(start=start, end=end, **({} if name == "scores" else {"mode": mode})),
                            EMPTY_SLICE[name](mode, start), id=f"{name}-empty slice {start}:{end}-{mode}")
               for name in SLICED for mode in (("score",) if name == "scores" else
                                               ("score", "end") if name == "align_many_arrays" else MODES)
               for start, end in ((1, 1), (3, 0xFFFFFFFF))]


def test_every_sliced_entry_point_has_an_empty_slice_row():
    assert set(EMPTY_SLICE) == set(SLICED)


@pytest.mark.parametrize("name, change, answer", EMPTY_ROWS)
def test_empty_requests_need_no_device(aligner, name, change, answer):
    assert shape_of(call(aligner, name, change)) == answer


@pytest.mark.parametrize("return_msa", (False, True))
def test_no_targets_is_the_profile_of_the_query(aligner, return_msa):
    for q in ("MKV", Pssm.from_sequence("MKV")):
        for targets in ([], np.zeros(0, dtype=np.int64)):
            got = shape_of(call(aligner, "profile_columns", dict(q=q, args=(targets,), return_msa=return_msa)))
            one = 3 * ProfileColumns.WEIGHT_ONE
            assert got == {"ProfileColumns": [12, 11, 19], "members": [one], "counts": (I64, (3, 25)),
                           "weighted": (I64, (3, 25)), "msa": (U8, (1, 3)) if return_msa else None}


def test_empty_tables_are_filled_with_minus_one(aligner):
    """(the values `shape_of` does not see: no query for any target)"""
    for change in (dict(q=[]), dict(start=1, end=1)):
        for mode in MODES:
            got = call(aligner, "best_queries_arrays", dict(change, mode=mode))
            assert not got["count"].any()
            for key in ("query", "score", "end_q", "end_t"):
                assert key not in got or np.all(got[key] == -1)
