"""The compiler's resource remarks of the last in-tree build for the three kernels of the hit compaction
(pyopal_amd/csrc/select_hits.rpt, written by the Makefile): memory-bound passes over the scores; the write holds a
block's 16 scores per thread in registers between its ranking and its stores, so a spill there is another read of the
row."""
import pytest

from test_build_resources import kernels


def test_hit_selection_kernels_do_not_spill():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    hits = {n: k for n, k in ks.items() if k["file"] == "select_hits.rpt"}
    for kernel in ("hits_count_kernel", "hits_offsets_kernel", "hits_write_kernel"):
        assert any(kernel in n for n in hits), (kernel, sorted(hits))
    assert len(hits) == 3, sorted(hits)
    bad = {n: k for n, k in hits.items()
           if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
