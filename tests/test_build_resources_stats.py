"""The compiler's resource remarks of the last in-tree build for the kernels of the score statistics and the binned
compaction (pyopal_amd/csrc/select_stats.rpt, written by the Makefile): memory-bound passes over the scores. The
statistics kernel keeps two runs of (bin, n, sum, sum of squares) per thread in registers - picked by comparison, never
by index, so that none of it lives in scratch - and the binned write holds a block's 16 scores per thread between its
ranking and its stores, like the write of select_hits.hip."""
import pytest

from test_build_resources import kernels

KERNELS = ("length_bins_kernel", "length_sums_kernel", "rows_stats_kernel", "hits_binned_count_kernel",
           "hits_binned_write_kernel")


def test_statistics_kernels_are_present_and_do_not_spill():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    stats = {n: k for n, k in ks.items() if k["file"] == "select_stats.rpt"}
    for kernel in KERNELS:
        assert any(kernel in n for n in stats), (kernel, sorted(stats))
    assert len(stats) == len(KERNELS), sorted(stats)
    bad = {n: k for n, k in stats.items()
           if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
