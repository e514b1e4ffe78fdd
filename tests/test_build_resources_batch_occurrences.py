"""The compiler's resource remarks of the last in-tree build for the kernels of the panel occurrence search
(pyopal_amd/csrc/occurrences_batch.rpt, written by the Makefile). The sweep keeps 64 rows of H and E in registers like
the single-query sweep it restates: a spilled vector register or scratch memory there costs a factor, and it is held
to that sweep's bound of two wavefronts per SIMD."""
import os

import pytest

from test_build_resources import CSRC, kernels

SWEEPS = [f"occurrences_batch_sweep_kernelILi{region}ELb{write}EE" for region in (1, 3) for write in (0, 1)]


def test_batch_occurrence_kernels_fit_their_registers():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    assert os.path.exists(os.path.join(CSRC, "occurrences_batch.rpt"))
    unit = {n: k for n, k in ks.items() if k["file"] == "occurrences_batch.rpt"}
    # HW and SW, count and write: four sweeps; and the kernel that finds each query's stretch of the scan's list
    for name in SWEEPS:
        assert sum(name in n for n in unit) == 1, (name, sorted(unit))
    assert sum("occurrences_batch_bounds_kernel" in n for n in unit) == 1, sorted(unit)
    assert len(unit) == 5, sorted(unit)
    bad = {n: k for n, k in unit.items() if k.get("VGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
    low = {n: k for n, k in unit.items() if k.get("Occupancy [waves/SIMD]", 0) < 2}
    assert not low, low
