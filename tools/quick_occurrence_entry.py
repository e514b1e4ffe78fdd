#!/usr/bin/env python3
"""One single occurrence search at 2 000 targets of 300 residues (tools/quick_occurrences.py's small case), timed two
ways: the C entry point alone through ctypes with its arguments built once (the outputs freed inside the loop, as the
wrapper's arrays would free them), and DeviceDatabase.search_occurrences. 50 warm-up calls, then the median and the
10th percentile of 1500 calls, twice each, in microseconds, for a search that finds nothing, one with 1284 and one
with 5402 occurrences. TREE: the checkout whose pyopal_amd is timed (this one by default), so that two builds can be
run in turn from one copy of this script (profiles/occurrence_family_refactor.txt).

Usage: python tools/quick_occurrence_entry.py [TREE [LABEL]]"""
import ctypes
import os
import sys
import time

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
label = sys.argv[2] if len(sys.argv) > 2 else "here"
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "tests"))
import numpy as np   # noqa: E402
import _data   # noqa: E402
from pyopal_amd import _capi   # noqa: E402
from pyopal_amd.matrices import ScoringMatrix   # noqa: E402

assert os.path.abspath(_capi.__file__).startswith(tree), _capi.__file__
B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
rng = np.random.default_rng(2026)
n = 2000
off = np.arange(n + 1, dtype=np.int64) * 300
res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
db = _capi.DeviceDatabase(res, off, 24)
query = _data.encode(_data.README_QUERY)
lib = _capi.lib()
libc = ctypes.CDLL(None)
libc.free.argtypes = [ctypes.c_void_p]
side = db._query_side(query, B62, 11, 1)
fn = lib.miopalSearchOccurrences
REPS = 1500


def median_us(call):
    for _ in range(50):
        call()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2] * 1e6, t[len(t) // 10] * 1e6


for cut in (41, 5, -11):
    counts = ctypes.c_int64(-1)
    ptrs = [ctypes.c_void_p() for _ in range(4)]
    refs = [ctypes.byref(p) for p in ptrs]
    args = (db.handle, *side.queries, *side.scoring, 1, 0, n, cut, len(query), -1, ctypes.byref(counts), *refs)

    def raw():
        rc = fn(*args)
        assert rc == 0
        for p in ptrs:
            if p.value:
                libc.free(p)
                p.value = None

    def method():
        db.search_occurrences(query, B62, 11, 1, "hw", min_score=cut)

    r, r10 = median_us(raw)
    m, m10 = median_us(method)
    r2, _ = median_us(raw)
    m2, _ = median_us(method)
    print(f"{label:8s} cut {cut:4d} found {counts.value:6d}   C alone {r:8.1f} {r2:8.1f} (10th pct {r10:8.1f})   method {m:8.1f} {m2:8.1f} (10th pct {m10:8.1f})  us", flush=True)
db.close()
