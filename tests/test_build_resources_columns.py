"""The compiler's resource remarks of the last in-tree build for the two kernels of the per-target selection
(pyopal_amd/csrc/select_columns.rpt, written by the Makefile): the fold keeps a column's M state entries - keys and end
locations - in registers while it walks a piece's rows, indexed by unrolled loops only; a spill or a scratch array
there is a memory round trip per row and column."""
import pytest

from test_build_resources import kernels


def test_column_selection_kernels_do_not_spill():
    ks = kernels()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    cols = {n: k for n, k in ks.items() if k["file"] == "select_columns.rpt"}
    for kernel in ("columns_fold_kernel", "columns_finish_kernel"):
        found = [n for n in cols if kernel in n]
        # M in {1, 2, 4, 8}, with and without end locations
        assert len(found) == 8, (kernel, sorted(cols))
    assert len(cols) == 16, sorted(cols)
    bad = {n: k for n, k in cols.items()
           if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad
