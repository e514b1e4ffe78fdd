"""The eight entry points of the occurrence family against each other, on one small database: what the family's
shared host code - the checks, the request and output bundles, the chunk plan, the handover of the outputs, the
routing figures - serves in every form, and no single family file covers across forms.

The witnesses are the single-query calls, which test_gpu_occurrences.py and test_gpu_occurrence_alignments.py hold to
the checker; everything here is exact equality. Twelve targets of 0 .. 40 residues over 4 letters (one empty), HW and
SW at 3/1; a panel of five queries: an empty one, 6, 9 and 64 rows on the panel kernels, and 65 rows on the single
path. The cuts are chosen so that the queries of 6 and 64 rows and the long one have occurrences and the one of 9 rows
has none; the numpy recurrence of _occurrences.py says so on the CPU, and the test asserts it.
"""
import ctypes
import functools

import numpy as np
import pytest

import _occurrences

pytestmark = pytest.mark.gpu

A = 4
GAPS = (3, 1)
MATRIX = np.where(np.eye(A, dtype=bool), 2, -3).astype(np.int32)
HEIGHTS = (0, 6, 9, 64, 65)
CUTS = {"hw": (1, 6, 100, -60, -62), "sw": (1, 8, 100, 14, 14)}
WINDOWS = (None, 0, 3, None, 5)
FIVE = ("target", "score", "end_t", "end_q")
STARTS = ("start_t", "start_q")
OPS = ("aln_off", "aln_flat")
TOO_MANY = 103
# (name of the C function, PSSM?, aligned?)
FORMS = (("miopalSearchBatchOccurrences", False, False), ("miopalSearchBatchOccurrencesAligned", False, True),
         ("miopalSearchPssmBatchOccurrences", True, False), ("miopalSearchPssmBatchOccurrencesAligned", True, True))


@functools.lru_cache(maxsize=None)
def data():
    """(targets, panel): the queries first; every other target carries a copy of the short queries and a stretch of the
    long ones, so that there is something to find"""
    rng = np.random.default_rng(20240)
    panel = [rng.integers(0, A, size=h).astype(np.uint8) for h in HEIGHTS]
    lengths = [40, 0, 17, 33, 1, 40, 25, 38, 9, 31, 40, 22]
    targets = []
    for k, length in enumerate(lengths):
        t = rng.integers(0, A, size=length).astype(np.uint8)
        if k % 2 == 0 and length >= 22:
            t[2:8] = panel[1]
            t[length - 20:length] = panel[3 + k % 4 // 2][10:30]
        targets.append(t)
    return targets, panel


def windows_of(panel):
    return [len(q) if w is None else w for q, w in zip(panel, WINDOWS)]


@functools.lru_cache(maxsize=None)
def expected_counts(algorithm):
    """occurrences per query by the numpy recurrence and the rule restated in Python: no device"""
    targets, panel = data()
    counts = []
    for q, cut, window in zip(panel, CUTS[algorithm], windows_of(panel)):
        if len(q) == 0:
            counts.append(0)
            continue
        V, R = _occurrences.column_values(MATRIX[q], targets, *GAPS, algorithm)
        flat = _occurrences.flat_columns([V[k, :len(t)] for k, t in enumerate(targets)], [R[k, :len(t)] for k, t in enumerate(targets)])
        counts.append(len(_occurrences.expected_flat(*flat, cut, window)["target"]))
    return counts


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def db(capi):
    targets, _ = data()
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
    handle = capi.DeviceDatabase(np.concatenate(targets), offsets, A, device=0)
    yield handle
    handle.close()


@pytest.fixture(scope="module")
def answers(db):
    """per algorithm: the single calls (plain and aligned) query by query, and the four panel calls"""
    _, panel = data()
    pssms = [MATRIX[q] for q in panel]
    out = {}
    for algorithm in ("hw", "sw"):
        rule = dict(min_score=list(CUTS[algorithm]), window=list(WINDOWS))
        single = [dict(min_score=c, window=w) for c, w in zip(CUTS[algorithm], WINDOWS)]
        out[algorithm] = {
            "single": [db.search_occurrences(q, MATRIX, *GAPS, algorithm, **r) for q, r in zip(panel, single)],
            "single_aligned": [db.search_occurrence_alignments(q, MATRIX, *GAPS, algorithm, **r) for q, r in zip(panel, single)],
            "single_pssm": [db.search_occurrences_pssm(p, *GAPS, algorithm, **r) for p, r in zip(pssms, single)],
            "single_pssm_aligned": [db.search_occurrence_alignments_pssm(p, q, *GAPS, algorithm, **r)
                                    for p, q, r in zip(pssms, panel, single)],
            "panel": db.search_batch_occurrences(panel, MATRIX, *GAPS, algorithm, **rule),
            "panel_aligned": db.search_batch_occurrence_alignments(panel, MATRIX, *GAPS, algorithm, **rule),
            "panel_pssm": db.search_batch_occurrences_pssm(pssms, *GAPS, algorithm, **rule),
            "panel_pssm_aligned": db.search_batch_occurrence_alignments_pssm(pssms, panel, *GAPS, algorithm, **rule),
        }
    return out


def same(got, want, keys, context):
    for key in keys:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (context, key)


def stretch(csr, i, aligned):
    """query i of a CSR as a single call answers"""
    lo, hi = int(csr["offsets"][i]), int(csr["offsets"][i + 1])
    out = {"count": hi - lo}
    out.update({key: csr[key][lo:hi] for key in FIVE + (STARTS if aligned else ())})
    if aligned:
        off = csr["aln_off"]
        out["aln_off"] = off[lo:hi + 1] - off[lo]
        out["aln_flat"] = csr["aln_flat"][int(off[lo]):int(off[hi])]
    return out


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_the_cuts_leave_what_the_docstring_says(answers, algorithm):
    counts = expected_counts(algorithm)
    assert counts[0] == 0 and counts[1] > 0 and counts[2] == 0 and counts[3] > 0 and counts[4] > 0, counts
    assert np.diff(answers[algorithm]["panel"]["offsets"]).tolist() == counts
    assert [s["count"] for s in answers[algorithm]["single"]] == counts


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_every_form_equals_the_single_calls(answers, algorithm):
    got = answers[algorithm]
    for i in range(len(HEIGHTS)):
        for name, singles, aligned in (("panel", "single", False), ("panel_aligned", "single_aligned", True),
                                       ("panel_pssm", "single_pssm", False), ("panel_pssm_aligned", "single_pssm_aligned", True)):
            part, want = stretch(got[name], i, aligned), got[singles][i]
            assert part["count"] == want["count"], (name, i)
            same(part, want, FIVE + ((STARTS + OPS) if aligned else ()), (name, i))
    # the first five arrays of an aligned call are the plain call's
    for aligned, plain in (("panel_aligned", "panel"), ("panel_pssm_aligned", "panel_pssm")):
        same(got[aligned], got[plain], ("offsets",) + FIVE, aligned)
    for i in range(len(HEIGHTS)):
        for aligned, plain in (("single_aligned", "single"), ("single_pssm_aligned", "single_pssm")):
            assert got[aligned][i]["count"] == got[plain][i]["count"]
            same(got[aligned][i], got[plain][i], FIVE, (aligned, i))
    # the PSSM forms, built from the matrix's rows, are the plain forms
    same(got["panel_pssm"], got["panel"], ("offsets",) + FIVE, "pssm")
    same(got["panel_pssm_aligned"], got["panel_aligned"], ("offsets",) + FIVE + STARTS + OPS, "pssm aligned")
    for i in range(len(HEIGHTS)):
        same(got["single_pssm"][i], got["single"][i], FIVE, ("single pssm", i))
        same(got["single_pssm_aligned"][i], got["single_aligned"][i], FIVE + STARTS + OPS, ("single pssm aligned", i))
    total = int(got["panel_aligned"]["offsets"][-1])
    assert got["panel_aligned"]["aln_off"][0] == 0 and len(got["panel_aligned"]["aln_off"]) == total + 1


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_starts_only(db, answers, algorithm):
    _, panel = data()
    pssms = [MATRIX[q] for q in panel]
    rule = dict(min_score=list(CUTS[algorithm]), window=list(WINDOWS), operations=False)
    want = answers[algorithm]["panel_aligned"]
    for got in (db.search_batch_occurrence_alignments(panel, MATRIX, *GAPS, algorithm, **rule),
                db.search_batch_occurrence_alignments_pssm(pssms, None, *GAPS, algorithm, **rule)):
        same(got, want, ("offsets",) + FIVE + STARTS, "starts only")
        assert not [key for key in got if key.startswith("aln")], sorted(got)
    for i, q in enumerate(panel):
        r = dict(min_score=CUTS[algorithm][i], window=WINDOWS[i], operations=False)
        for got in (db.search_occurrence_alignments(q, MATRIX, *GAPS, algorithm, **r),
                    db.search_occurrence_alignments_pssm(pssms[i], None, *GAPS, algorithm, **r)):
            same(got, answers[algorithm]["single_aligned"][i], FIVE + STARTS, ("single starts only", i))
            assert not [key for key in got if key.startswith("aln")], sorted(got)


def raw_panel_call(capi, db, name, pssm, aligned, algorithm, max_hits):
    """the C function itself: (the code, hitOffsets, whether every output pointer is as it was)"""
    _, panel = data()
    flat = np.concatenate(panel)
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in panel])]).astype(np.int64)
    rows = np.ascontiguousarray(MATRIX[flat], dtype=np.int32)
    cuts = np.ascontiguousarray(CUTS[algorithm], dtype=np.int32)
    windows = np.ascontiguousarray(windows_of(panel), dtype=np.int32)
    hit_offsets = np.full(len(panel) + 1, -7, dtype=np.int64)
    ptrs = [ctypes.c_void_p(0x77) for _ in range(8 if aligned else 4)]
    if pssm:
        side = (rows.ctypes.data,) + ((flat.ctypes.data,) if aligned else ()) + (qoff.ctypes.data, len(panel), *GAPS, A)
    else:
        side = (flat.ctypes.data, qoff.ctypes.data, len(panel), *GAPS, MATRIX.ctypes.data, A)
    rc = getattr(capi.lib(), name)(db.handle, *side, capi.MODE[algorithm], 0, db.count, cuts.ctypes.data, windows.ctypes.data,
                                   max_hits, hit_offsets.ctypes.data, *[ctypes.byref(p) for p in ptrs])
    untouched = all(p.value == 0x77 for p in ptrs)
    if rc == 0:   # (the arrays are the caller's now)
        for p in ptrs:
            capi._libc.free(p)
    return rc, hit_offsets, untouched


@pytest.mark.parametrize("algorithm", ["hw", "sw"])
def test_max_hits(capi, db, answers, algorithm):
    _, panel = data()
    pssms = [MATRIX[q] for q in panel]
    whole = answers[algorithm]["panel_aligned"]
    total = int(whole["offsets"][-1])
    rule = dict(min_score=list(CUTS[algorithm]), window=list(WINDOWS))
    calls = {"miopalSearchBatchOccurrences": lambda **k: db.search_batch_occurrences(panel, MATRIX, *GAPS, algorithm, **rule, **k),
             "miopalSearchBatchOccurrencesAligned": lambda **k: db.search_batch_occurrence_alignments(panel, MATRIX, *GAPS, algorithm, **rule, **k),
             "miopalSearchPssmBatchOccurrences": lambda **k: db.search_batch_occurrences_pssm(pssms, *GAPS, algorithm, **rule, **k),
             "miopalSearchPssmBatchOccurrencesAligned": lambda **k: db.search_batch_occurrence_alignments_pssm(pssms, panel, *GAPS, algorithm, **rule, **k)}
    for name, pssm, aligned in FORMS:
        # one below the total: TooManyHits with the full offsets, every other output as it was
        with pytest.raises(capi.TooManyHits) as info:
            calls[name](max_hits=total - 1)
        assert np.array_equal(info.value.counts, whole["offsets"]), name
        rc, hit_offsets, untouched = raw_panel_call(capi, db, name, pssm, aligned, algorithm, total - 1)
        assert rc == TOO_MANY and "maxHits" in capi.last_error(), (name, rc)
        assert np.array_equal(hit_offsets, whole["offsets"]) and untouched, name
        # the total itself: the call succeeds, with the same answer
        got = calls[name](max_hits=total)
        same(got, whole, ("offsets",) + FIVE + ((STARTS + OPS) if aligned else ()), (name, "max_hits = total"))
        rc, hit_offsets, untouched = raw_panel_call(capi, db, name, pssm, aligned, algorithm, total)
        assert rc == 0 and np.array_equal(hit_offsets, whole["offsets"]) and not untouched, name


def test_reporters(db, answers):
    _, panel = data()
    algorithm = "hw"
    rule = dict(min_score=list(CUTS[algorithm]), window=list(WINDOWS))
    # a single search and a single aligned search: what the single-query reporters hold from here on
    db.search_occurrences(panel[4], MATRIX, *GAPS, algorithm, min_score=CUTS[algorithm][4], window=WINDOWS[4])
    db.search_occurrence_alignments(panel[1], MATRIX, *GAPS, algorithm, min_score=CUTS[algorithm][1], window=WINDOWS[1])
    routing, align_routing = db.last_occurrence_routing(), db.last_occurrence_align_routing()
    assert routing[0] == db.count and routing[3] == 1 and align_routing[2] >= 1, (routing, align_routing)
    db.search_occurrences(panel[4], MATRIX, *GAPS, algorithm, min_score=CUTS[algorithm][4], window=WINDOWS[4])
    routing = db.last_occurrence_routing()
    assert routing[0] == db.count and routing[1] > 0 and routing[3] == 2, routing
    # a panel call that holds the query of 65 rows: three queries on the panel kernels, one on the single path
    db.search_batch_occurrences(panel, MATRIX, *GAPS, algorithm, **rule)
    assert db.last_batch_occurrence_routing()[:2] == [3, 1]
    assert db.last_occurrence_routing() == routing and db.last_occurrence_align_routing() == align_routing
    # ... and an aligned one, whose long query runs the single-query stage
    got = db.search_batch_occurrence_alignments(panel, MATRIX, *GAPS, algorithm, **rule)
    assert db.last_batch_occurrence_routing()[:2] == [3, 1]
    stage = db.last_batch_occurrence_align_routing()
    assert stage[0] + stage[1] == int(got["offsets"][-1]) and stage[2] >= 2, stage
    assert db.last_occurrence_routing() == routing and db.last_occurrence_align_routing() == align_routing
    db.search_batch_occurrence_alignments_pssm([MATRIX[q] for q in panel], panel, *GAPS, algorithm, **rule)
    assert db.last_batch_occurrence_routing()[:2] == [3, 1]
    assert db.last_occurrence_routing() == routing and db.last_occurrence_align_routing() == align_routing
