"""The column kernels of the profile step alone (miopalTestProfileColumns: the count, terms, member-weights and weighted
kernels of profile_columns.hip on a multiple alignment the caller supplies), bit for bit against the integer reference
of tests/_profile.py: sizes around the 64 columns of a wavefront and the 128 members of its span, both alphabets, and
the columns whose terms are extreme."""
import numpy as np
import pytest

import _profile

pytestmark = pytest.mark.gpu

MEMBERS = [1, 63, 64, 65, 4097]
LENGTHS = [1, 64, 65, 300]


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def check(capi, msa, A, tag):
    got = capi.profile_columns_rows(msa, A)
    counts, k, terms, weights, weighted = _profile.columns(msa, A)
    np.testing.assert_array_equal(got["counts"], counts, err_msg=f"counts {tag}")
    np.testing.assert_array_equal(got["member_weights"], weights, err_msg=f"member weights {tag}")
    np.testing.assert_array_equal(got["weighted"], weighted, err_msg=f"weighted {tag}")
    assert got["counts"].dtype == got["weighted"].dtype == got["member_weights"].dtype == np.int64
    return got


def random_msa(rng, members, Q, A):
    """letters, the gap and 255; every column with its own share of letters, some columns sparse"""
    entries = np.concatenate([np.arange(A + 1), [255] * (A // 3)]).astype(np.uint8)
    msa = rng.choice(entries, size=(members, Q))
    few = rng.random(Q) < 0.3   # columns of two or three letters: large terms
    msa[:, few] = rng.choice(entries[[0, 1, A // 2, A, -1]], size=(members, int(few.sum())))
    return np.ascontiguousarray(msa, dtype=np.uint8)


@pytest.mark.parametrize("A", [24, 32])
@pytest.mark.parametrize("members", MEMBERS)
def test_random_matrices_match_the_reference(capi, members, A):
    rng = np.random.default_rng(1000 * A + members)
    for Q in LENGTHS:
        check(capi, random_msa(rng, members, Q, A), A, (members, Q, A))


def test_span_edges(capi):
    """128 members are one wavefront's span of the count and weighted kernels: one short of it, it, one more"""
    rng = np.random.default_rng(7)
    for members in (127, 128, 129, 257):
        check(capi, random_msa(rng, members, 70, 24), 24, members)


def test_one_letter_columns(capi):
    """every member on the same letter: k = 1, the count is the number of members, the term 2^32 / members"""
    for members in (3, 64, 1000):
        msa = np.tile(np.array([5, 0, 31, 7], dtype=np.uint8), (members, 1))
        got = check(capi, msa, 32, members)
        assert got["counts"][0, 5] == members and got["counts"].sum() == 4 * members
        assert np.all(got["member_weights"] == 4 * (2 ** 32 // members))
        assert got["weighted"][2, 31] == members * 4 * (2 ** 32 // members)


def test_columns_without_a_letter(capi):
    """a column of gaps and 255 only: k = 0, no term, its gap count and the gap's weighted sum still stand"""
    rng = np.random.default_rng(9)
    msa = random_msa(rng, 90, 66, 24)
    msa[:, 10] = rng.choice(np.array([24, 255], dtype=np.uint8), size=90)
    msa[:, 65] = 255
    got = check(capi, msa, 24, "gaps")
    assert got["counts"][10, :24].sum() == 0 and got["counts"][10, 24] == np.count_nonzero(msa[:, 10] == 24) > 0
    assert got["weighted"][10, :24].sum() == 0 and got["weighted"][10, 24] > 0
    assert got["counts"][65].sum() == 0 and got["weighted"][65].sum() == 0


def test_single_member(capi):
    """one member: every term is exactly 2^32"""
    msa = np.array([[3, 24, 255, 0, 23]], dtype=np.uint8)
    got = check(capi, msa, 24, "single")
    assert got["member_weights"].tolist() == [3 * 2 ** 32]
    assert got["weighted"][0, 3] == got["weighted"][1, 24] == 3 * 2 ** 32 and got["weighted"][2].sum() == 0


def test_all_letters_in_a_column(capi):
    """all 32 letters occur: k = 32, the smallest terms"""
    rng = np.random.default_rng(3)
    msa = random_msa(rng, 200, 5, 32)
    msa[:32, 2] = np.arange(32)
    got = check(capi, msa, 32, "all letters")
    assert np.all(got["counts"][2, :32] > 0)


def test_two_runs_give_the_same_answer(capi):
    """integer sums behind atomics: the order in which the blocks arrive does not show"""
    rng = np.random.default_rng(4)
    msa = random_msa(rng, 4097, 300, 24)
    first = capi.profile_columns_rows(msa, 24)
    second = capi.profile_columns_rows(msa, 24)
    for key in first:
        assert np.array_equal(first[key], second[key]), key
