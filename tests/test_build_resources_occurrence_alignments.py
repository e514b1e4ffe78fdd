"""The compiler's resource remarks of the last in-tree build for the one kernel the alignment stage of the occurrence
search adds (pyopal_amd/csrc/occurrence_align.rpt, written by the Makefile): occurrence_pair_inputs_kernel gathers the
occurrences' target origins; everything else the stage launches belongs to the pair list. A gather of one load and
one store per thread has no business spilling or touching scratch memory."""
import os

import pytest

from test_build_resources import CSRC, kernels


def test_occurrence_align_kernel_fits_its_registers():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    assert os.path.exists(os.path.join(CSRC, "occurrence_align.rpt"))
    mine = {n: k for n, k in ks.items() if k["file"] == "occurrence_align.rpt"}
    assert len(mine) == 1 and sum("occurrence_pair_inputs_kernel" in n for n in mine) == 1, sorted(mine)
    bad = {n: k for n, k in mine.items() if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
    # ... and the kernel is nowhere else: occurrences.rpt keeps the count tests/test_build_resources_occurrences.py pins
    assert not [n for n, k in ks.items() if "occurrence_pair_inputs_kernel" in n and k["file"] != "occurrence_align.rpt"]
