"""Top-k selection on the device against the plain searches it replaces, same inputs, same process: a warm-up, then the
plain and the top call alternately, the median of several calls.
  - headline (Q = 53 x 1M x 300, SW, k = 100): DeviceDatabase.search_top against DeviceDatabase.search (miopalSearchTop
    against miopalSearch), score and end;
  - 1000 queries (20-64 aa) x 20k x 300, k = 10: Aligner.top_hits_many against Aligner.align_many_arrays;
  - 256 queries x 1M x 300, k = 10: Aligner.top_hits_many alone (the plain batch needs 1 GB of host output), and the
    plain batch's time beside it with --plain-1m.
Kernel times of the selection: run under rocprofv3 --kernel-trace --stats with --only-headline.
Usage: python tools/quick_top.py [--reps N] [--only-headline] [--plain-1m]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data  # noqa: E402
import pyopal_amd as pyopal  # noqa: E402
from pyopal_amd import _capi  # noqa: E402
from pyopal_amd.matrices import ScoringMatrix  # noqa: E402

LETTERS = list("ARNDCQEGHILKMFPSTWYV")


def seqs(rng, lengths):
    return ["".join(rng.choice(LETTERS, size=int(L))) for L in lengths]


def alternate(reps, plain, top):
    plain()
    top()
    tp, tt = [], []
    for _ in range(reps):
        t = time.perf_counter(); plain(); tp.append(time.perf_counter() - t)
        t = time.perf_counter(); top(); tt.append(time.perf_counter() - t)
    return float(np.median(tp)), float(np.median(tt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only-headline", action="store_true")
    ap.add_argument("--plain-1m", action="store_true", help="also time the plain 256 x 1M batch (1 GB of output)")
    args = ap.parse_args()
    lib = os.path.join(ROOT, "pyopal_amd", "libmiopal.so")
    print(f"library md5 {hashlib.md5(open(lib, 'rb').read()).hexdigest()[:12]}")
    B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
    rng = np.random.default_rng(2026)
    n = 1_000_000
    off = np.arange(n + 1, dtype=np.int64) * 300
    res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
    db = _capi.DeviceDatabase(res, off, 24)
    query = _data.encode(_data.README_QUERY)
    cells = 53.0 * n * 300
    for mode in ("score", "end"):
        got = db.search_top(query, B62, 3, 1, mode, "sw", k=100)
        full = db.search(query, B62, 3, 1, mode, "sw")
        order = np.lexsort((np.arange(n), -full["score"].astype(np.int64)))[:100]
        assert np.array_equal(got["target"], order) and np.array_equal(got["score"], full["score"][order])
        p, t = alternate(args.reps, lambda: db.search(query, B62, 3, 1, mode, "sw"),
                         lambda: db.search_top(query, B62, 3, 1, mode, "sw", k=100))
        print(f"headline Q=53 x 1M x 300 sw {mode:5s} k=100: plain {p * 1e3:7.3f} ms  top {t * 1e3:7.3f} ms  "
              f"top - plain {(t - p) * 1e3:+7.3f} ms  ({cells / t / 1e9:7.1f} GCUPS top)", flush=True)
    if args.only_headline:
        return
    aligner = pyopal.Aligner(scoring_matrix="BLOSUM62")
    short = seqs(rng, rng.integers(20, 65, size=1000))
    small = pyopal.Database(seqs(rng, np.full(20000, 300)))
    qcells = float(sum(len(q) for q in short))
    for mode in ("score", "end"):
        p, t = alternate(max(3, args.reps // 4), lambda: aligner.align_many_arrays(short, small, mode=mode),
                         lambda: aligner.top_hits_many(short, small, 10, mode=mode))
        c = qcells * small.total_length
        print(f"1000 q (20-64 aa) x 20k x 300 {mode:5s} k=10: align_many_arrays {p * 1e3:8.2f} ms  "
              f"top_hits_many {t * 1e3:8.2f} ms  ({c / p / 1e9:7.1f} / {c / t / 1e9:7.1f} GCUPS)", flush=True)
    queries = [np.frombuffer(pyopal.Alphabet().encode(q), dtype=np.uint8) for q in short[:256]]
    c = float(sum(len(q) for q in queries)) * n * 300
    for mode in ("score", "end"):
        db.search_batch_top(queries, B62, 3, 1, mode, "sw", k=10)
        tt = []
        for _ in range(3):
            t = time.perf_counter(); db.search_batch_top(queries, B62, 3, 1, mode, "sw", k=10)
            tt.append(time.perf_counter() - t)
        t = float(np.median(tt))
        line = f"256 q x 1M x 300 {mode:5s} k=10: search_batch_top {t * 1e3:8.2f} ms ({c / t / 1e9:7.1f} GCUPS)"
        if args.plain_1m:
            tp = []
            for _ in range(3):
                s = time.perf_counter(); db.search_batch(queries, B62, 3, 1, mode, "sw"); tp.append(time.perf_counter() - s)
            p = float(np.median(tp))
            line += f"  plain search_batch {p * 1e3:8.2f} ms ({c / p / 1e9:7.1f} GCUPS)"
        print(line, flush=True)


if __name__ == "__main__":
    main()
