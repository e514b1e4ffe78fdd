"""The chunk plan of the panel occurrence searches without a device (occurrence_plan.h; miopalSelfTest(7))."""
import pytest


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    return _capi


def test_occurrence_plan_against_hand_worked_literals(capi):
    # occurrence_plan.h, what decides the grid and the LDS size of every launch of a panel occurrence search: queries
    # per chunk (the bound over the slice, one query when the slice alone is larger, the cap), no empty trailing chunk,
    # the groups the count sweep wants (1024 for 2 000 reads on 256 CUs, 11 for 200 000), and for one chunk the pad rows
    # to a multiple of eight (residue list and row-source map), a group filled to the byte at 4 letters (8192 rows) and
    # to the last query at 32 (1240 rows), the row more that splits either, one query a group when more groups are
    # wanted than there are queries. The number of the first failing check comes back. Needs no device.
    assert capi.lib().miopalSelfTest(7) == 0
