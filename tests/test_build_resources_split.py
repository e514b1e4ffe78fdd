"""The compiler's resource remarks (pyopal_amd/csrc/*.rpt, written by the Makefile) of the one-strip Smith-Waterman
kernel's two hand-out modes: the column split is a template parameter, so that the instantiation the dynamic hand-out
runs keeps its code and registers - the headline's <53, false> at the figures it had before the split existed - and
the split instantiations, which carry the plan of their interval in scalar registers and move the state of a cut
through buffer accesses, neither spill nor lose the third wavefront per SIMD."""
import re

import pytest

from test_build_resources import kernels

NAME = re.compile(r"interseq_pair_biased_kernelILi(\d+)ELb0ELb([01])EE")
FIELDS = ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")


def score_only():
    """{(rows, split): remarks} of interseq_pair_biased_kernel<rows, false, split>"""
    out = {}
    for name, k in kernels().items():
        m = NAME.search(name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = k
    return out


def total_sgprs(rows, split):
    # (test_build_resources.kernels() does not read this line of the remarks)
    import glob
    import os
    from test_build_resources import CSRC
    want = f"interseq_pair_biased_kernelILi{rows}ELb0ELb{int(split)}EE"
    for path in glob.glob(os.path.join(CSRC, "interseq_swb16_*.rpt")):
        inside = False
        for line in open(path, errors="replace"):
            if "Function Name:" in line:
                inside = want in line
            elif inside:
                m = re.search(r"remark:\s+TotalSGPRs: (\d+)", line)
                if m:
                    return int(m.group(1))
    return None


def test_split_instantiations_do_not_spill_and_keep_three_wavefronts():
    ks = score_only()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    split = {rows: k for (rows, on), k in ks.items() if on}
    assert sorted(split) == list(range(1, 65)), sorted(split)   # every row count of the dynamic form has its split form
    bad = {rows: {f: k.get(f) for f in FIELDS} for rows, k in split.items()
           if k.get("VGPRs Spill", 0) or k.get("SGPRs Spill", 0) or k.get("ScratchSize [bytes/lane]", 0)
           or k.get("Occupancy [waves/SIMD]", 0) < 3 or k.get("VGPRs", 999) > 168}
    assert not bad, bad


def test_dynamic_instantiation_of_the_headline_is_what_it_was():
    ks = score_only()
    if not ks:
        pytest.skip("no resource remarks: build with make -C pyopal_amd/csrc")
    k = ks[(53, False)]
    assert k["VGPRs"] == 142 and total_sgprs(53, False) == 62, (k, total_sgprs(53, False))
    assert k.get("VGPRs Spill", 0) == 0 and k.get("SGPRs Spill", 0) == 0 and k["ScratchSize [bytes/lane]"] == 0, k
    assert k["Occupancy [waves/SIMD]"] == 3, k
