"""The occurrence search of a panel over the case list of tests/_cases.py - alphabets of 2 to 32 letters, gap models
with open < extend and with a zero among them, matrices that are asymmetric, never positive, never negative or +-1:
the case's queries of every length of QUERY_LENGTHS (one row to three strips) as one panel against the case's targets,
held to the unchanged search_occurrences of one query at a time."""
import numpy as np
import pytest

import _cases
from _case_witnesses import cut_of
from test_gpu_batch_occurrences import GROUPINGS, assert_csr, group, singles

pytestmark = pytest.mark.gpu

CASES = _cases.cases()


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_panel_of_the_case_equals_singles(capi, tuning, case, grouping):
    """("filled": the queries of 1, 7 and 64 rows share one group; "spread": a group each)"""
    group(tuning, grouping)
    s, panel = case.search_set(), case.pair_set().queries
    assert sorted(len(q) for q in panel) == sorted(_cases.QUERY_LENGTHS)
    on_panel = sum(1 <= len(q) <= 64 for q in panel)
    db = capi.DeviceDatabase(s.residues, s.offsets, case.alphabet)
    try:
        for algorithm in ("hw", "sw"):
            cut = cut_of(algorithm)     # the cut of test_gpu_cases.py's occurrence test: the lowest there is
            cuts, windows = [cut] * len(panel), [None] * len(panel)
            got = db.search_batch_occurrences(panel, s.matrix, *case.gaps, algorithm, min_score=cut, window=None)
            routing = db.last_batch_occurrence_routing()
            want = singles(db, panel, s.matrix, case.gaps, algorithm, cuts, windows)
            assert_csr(got, want, (case.id, algorithm))
            assert routing[:3] == [on_panel, len(panel) - on_panel, 1], (case.id, algorithm, routing)
            assert db.last_batch_occurrence_groups()[:2] == ([1, on_panel] if grouping == "filled" else [on_panel, 1])
            if algorithm == "hw":
                # (every target that has a column has an occurrence of every query)
                assert np.all(np.diff(got["offsets"]) >= np.count_nonzero(s.lengths)), (case.id, got["offsets"])
    finally:
        db.close()
