"""The compiler's resource remarks of the last in-tree build for the kernels of the PSSM panel occurrence search
(pyopal_amd/csrc/occurrences_batch_pssm.rpt, written by the Makefile): the sweep of occurrences_batch.hip with its LDS
table filled from PSSM rows, held to what its sibling is held to - no spilled vector register, no scratch memory, two
wavefronts per SIMD at least."""
import os

import pytest

from test_build_resources import CSRC, kernels

SWEEPS = [f"occurrences_batch_pssm_sweep_kernelILi{region}ELb{write}EE" for region in (1, 3) for write in (0, 1)]


def test_pssm_batch_occurrence_kernels_fit_their_registers():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    assert os.path.exists(os.path.join(CSRC, "occurrences_batch_pssm.rpt"))
    unit = {n: k for n, k in ks.items() if k["file"] == "occurrences_batch_pssm.rpt"}
    # HW and SW, count and write: four sweeps and nothing else - the scan and the bounds kernel are the plain unit's
    for name in SWEEPS:
        assert sum(name in n for n in unit) == 1, (name, sorted(unit))
    assert len(unit) == 4, sorted(unit)
    bad = {n: k for n, k in unit.items() if k.get("VGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
    low = {n: k for n, k in unit.items() if k.get("Occupancy [waves/SIMD]", 0) < 2}
    assert not low, low
