"""Batched search against a Python loop of single searches on the same inputs (Aligner.align_many_arrays against
[align_arrays(q) for q in queries]): a warm-up, then the two forms alternately, the median of several calls.
Prints ms, GCUPS (true query lengths x target residues) and the batch routing counters per workload.
Usage: python tools/quick_batch.py [--reps N] [--quick]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pyopal_amd as pyopal  # noqa: E402
from pyopal_amd import _capi  # noqa: E402

LETTERS = list("ARNDCQEGHILKMFPSTWYV")


def seqs(rng, lengths):
    return ["".join(rng.choice(LETTERS, size=int(L))) for L in lengths]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="fewer queries (smoke of the tool)")
    args = ap.parse_args()
    lib = os.path.join(ROOT, "pyopal_amd", "libmiopal.so")
    print(f"library md5 {hashlib.md5(open(lib, 'rb').read()).hexdigest()[:12]}")
    rng = np.random.default_rng(2026)
    m = 100 if args.quick else 1000
    short = seqs(rng, rng.integers(20, 65, size=m))
    logn = np.minimum(np.maximum(rng.lognormal(np.log(300), 0.6, size=20000), 10), 8000).astype(int)
    workloads = [
        ("1000 q (20-64 aa) x 20k x 300 uniform", short, seqs(rng, np.full(20000, 300))),
        ("1000 q (20-64 aa) x 20k log-normal", short, seqs(rng, logn)),
        ("16 q x 1M x 300", short[:16], None),
        ("1000 q x 1000 x 300 (wavefront-per-pair route)", short, seqs(rng, np.full(1000, 300))),
    ]
    aligner = pyopal.Aligner(scoring_matrix="BLOSUM62")
    for name, queries, targets in workloads:
        if targets is None:
            # (a million targets of 300: residues straight into a Database would take minutes of Python)
            targets = seqs(rng, np.full(20000, 300)) * 50
        db = pyopal.Database(targets)
        cells = float(sum(len(q) for q in queries)) * float(db.total_length)
        for mode in ("score", "end"):
            loop = lambda: [aligner.align_arrays(q, db, mode=mode) for q in queries]  # noqa: E731
            batch = lambda: aligner.align_many_arrays(queries, db, mode=mode)  # noqa: E731
            loop()
            got = batch()
            routing = _capi.DeviceDatabase.last_batch_routing()
            # (the same answers: a check of the measurement, not a test)
            one = aligner.align_arrays(queries[0], db, mode=mode)
            assert np.array_equal(got[0].score, one.score)
            tl, tb = [], []
            for _ in range(args.reps):
                t = time.perf_counter(); batch(); tb.append(time.perf_counter() - t)
                t = time.perf_counter(); loop(); tl.append(time.perf_counter() - t)
            b, l_ = float(np.median(tb)), float(np.median(tl))
            print(f"{name:48s} {mode:5s}: batch {b * 1e3:9.2f} ms ({cells / b / 1e9:8.1f} GCUPS)  "
                  f"loop {l_ * 1e3:9.2f} ms ({cells / l_ / 1e9:8.1f} GCUPS)  x{l_ / b:5.2f}  "
                  f"routing (batch pairs, pair-kernel pairs, single-path queries, launches) {routing}", flush=True)


if __name__ == "__main__":
    main()
