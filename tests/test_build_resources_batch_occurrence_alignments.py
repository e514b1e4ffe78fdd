"""The compiler's resource remarks of the last in-tree build for the one kernel the alignment stage of the panel
occurrence search adds (pyopal_amd/csrc/occurrence_align_batch.rpt, written by the Makefile):
batch_occurrence_origins_kernel gathers the occurrences' target origins and finds their queries' origins by a
binary search; everything else the stage launches belongs to the pair list. A gather of a few loads and two stores per
thread has no business spilling or touching scratch memory - and it lives in a unit of its own: occurrence_align.rpt
and occurrences_batch.rpt keep the counts their own tests pin."""
import os

import pytest

from test_build_resources import CSRC, kernels

KERNEL = "batch_occurrence_origins_kernel"


def test_batch_occurrence_align_kernel_fits_its_registers():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    assert os.path.exists(os.path.join(CSRC, "occurrence_align_batch.rpt"))
    mine = {n: k for n, k in ks.items() if k["file"] == "occurrence_align_batch.rpt"}
    assert len(mine) == 1 and sum(KERNEL in n for n in mine) == 1, sorted(mine)
    bad = {n: k for n, k in mine.items() if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
    assert not [n for n, k in ks.items() if KERNEL in n and k["file"] != "occurrence_align_batch.rpt"]
