"""The PSSM panel occurrence searches on the case list of tests/_cases.py: each case's queries of 1, 7, 64, 65 and 130
rows turned into PSSM rows (the matrix row of every residue; the query as consensus), as one panel against the case's
targets at the lowest cut, in both forms, held to the unchanged single-PSSM calls one PSSM at a time."""
import numpy as np
import pytest

import _cases
from _case_witnesses import cut_of
from test_gpu_batch_occurrence_alignments import assert_csr
from test_gpu_batch_occurrence_alignments_pssm import singles as aligned_singles
from test_gpu_batch_occurrences import assert_csr as assert_ends
from test_gpu_batch_occurrences_pssm import singles as end_singles

pytestmark = pytest.mark.gpu

CASES = _cases.cases()


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_pssm_panel_of_the_case_equals_singles(capi, case):
    s, queries = case.search_set(), case.pair_set().queries
    assert sorted(len(q) for q in queries) == sorted(_cases.QUERY_LENGTHS)
    on_panel = sum(1 <= len(q) <= 64 for q in queries)
    A = case.alphabet
    panel = [np.ascontiguousarray(s.matrix.reshape(A, A)[q]) for q in queries]
    db = capi.DeviceDatabase(s.residues, s.offsets, A)
    try:
        for algorithm in ("hw", "sw"):
            cut = cut_of(algorithm)
            cuts, windows = [cut] * len(panel), [None] * len(panel)
            got = db.search_batch_occurrences_pssm(panel, *case.gaps, algorithm, min_score=cut, window=None)
            assert db.last_batch_occurrence_routing()[:3] == [on_panel, len(panel) - on_panel, 1], (case.id, algorithm)
            assert_ends(got, end_singles(db, panel, case.gaps, algorithm, cuts, windows), (case.id, algorithm))
            if algorithm == "hw":
                assert np.all(np.diff(got["offsets"]) >= np.count_nonzero(s.lengths)), (case.id, got["offsets"])
            full = db.search_batch_occurrence_alignments_pssm(panel, queries, *case.gaps, algorithm, min_score=cut, window=None)
            assert db.last_batch_occurrence_routing()[:3] == [on_panel, len(panel) - on_panel, 1], (case.id, algorithm)
            assert_csr(full, aligned_singles(db, panel, queries, case.gaps, algorithm, cuts, windows), (case.id, algorithm, "aligned"))
    finally:
        db.close()
