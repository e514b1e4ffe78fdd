"""The compiler's resource remarks of the last in-tree build for the kernels of the profile columns
(pyopal_amd/csrc/profile_columns.rpt, written by the Makefile): the five kernels are small loops over bytes and LDS
counters; a spill or a scratch array in one of them is a mistake in its indexing (a counter table that left LDS for
private memory), not a trade-off."""
import pytest

from test_build_resources import kernels

KERNELS = ("profile_project_kernel", "columns_count_kernel", "columns_terms_kernel", "member_weights_kernel",
           "columns_weighted_kernel")


def test_profile_kernels_do_not_spill():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    mine = {n: k for n, k in ks.items() if k["file"] == "profile_columns.rpt"}
    for kernel in KERNELS:
        found = [n for n in mine if kernel in n]
        assert len(found) == 1, (kernel, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    bad = {n: k for n, k in mine.items()
           if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
