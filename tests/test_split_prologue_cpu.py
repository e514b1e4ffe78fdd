"""The host side of the column split of the one-strip Smith-Waterman kernel, without a device (miopalSelfTest(6),
pyopal_amd/csrc/host.hip): the dynamic LDS its launch asks for - pair table, counters, and the copy of the profile the
table is built from - stays within the compute unit's 160 KB for every row count 1 .. 64 at 24 symbols (and for every
alphabet whose table the host accepts at all), and the plan of the intervals the host hands to the kernel is, chunk by
chunk, the definition: interval w of W = chunks [w C / W, (w + 1) C / W) of the launch's chunk sequence."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pyopal_amd", "csrc")], check=True)
    return _capi


def test_split_launch_lds_and_plan(capi):
    assert capi.lib().miopalSelfTest(6) == 0
