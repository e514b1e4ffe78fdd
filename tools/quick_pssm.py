"""PSSM search (miopalSearchPssm) against the plain search of the sequence the PSSM is derived from, on one resident
handle: search_pssm(rows = matrix[q], consensus = q) and DeviceDatabase.search(q) compute the same thing on the same
kernels, so the ratio is what the row-indexed score source costs. Seeded data, a warm-up of every shape, then the two
calls alternated; median and spread (min .. max) of each, host clock around calls that end in a synchronise, and the
plain search's own run-to-run spread is the yardstick. --tree PATH times the library and Python package of another
checkout (built in place) instead of this one; a tree without search_pssm is timed on the plain search alone, which is
how the plain path of a commit is compared with its parent's. --out FILE appends every line printed to FILE
(profiles/pssm_vs_plain.txt is made of such runs).
  A  Q = 53 (README query), 1M x 300 uniform, SW: score / end / full        (the headline shape)
  B  Q = 300, 1M x 300 uniform, SW, full
  C  Q = 53, 500k log-normal targets, NW, score: leans on the side kernel (the int32 rung's row-indexed forms)
Usage: python tools/quick_pssm.py [--tree PATH] [--reps N] [--only A,B,C] [--label NAME] [--scale F] [--out FILE]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="A,B,C")
ap.add_argument("--label", default=None)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of the targets (a quick look)")
ap.add_argument("--out", default=None, help="append the printed lines to this file")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data  # noqa: E402
from pyopal_amd import _capi  # noqa: E402
from pyopal_amd.matrices import ScoringMatrix  # noqa: E402

LABEL = args.label or os.path.basename(ROOT)
B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)


def say(text):
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


def stats(t):
    return f"median {np.median(t) * 1e3:9.3f} ms  (min {min(t) * 1e3:9.3f} .. max {max(t) * 1e3:9.3f})"


def leg(name, db, query, mode, algorithm, cells):
    rows = np.ascontiguousarray(B62.reshape(24, 24)[query])
    calls = [("plain", lambda: db.search(query, B62, 3, 1, mode, algorithm))]
    if hasattr(db, "search_pssm"):
        calls.append(("pssm ", lambda: db.search_pssm(rows, query, 3, 1, mode, algorithm)))
    times = {n: [] for n, _ in calls}
    routing = {}
    for rep in range(args.reps + 2):   # (two warm-ups: the first builds the slice's packed view)
        for n, call in calls:
            t0 = time.perf_counter()
            call()
            if rep >= 2:
                times[n].append(time.perf_counter() - t0)
            routing[n] = (db.last_routing(), db.last_full_routing() if mode == "full" else 0)
    for n, _ in calls:
        say(f"[{LABEL}] {name} {mode:5s} {algorithm} {n}: {stats(times[n])}  {cells / np.median(times[n]) / 1e12:6.2f} TCUPS  "
            f"routing {routing[n]}")
    if len(calls) == 2:
        p, q = np.median(times["plain"]), np.median(times["pssm "])
        spread = (max(times["plain"]) - min(times["plain"])) / p
        say(f"[{LABEL}] {name} {mode:5s} {algorithm} pssm / plain = {q / p:.3f}  (plain's own spread {spread * 100:.1f} % of its median)")


def main():
    only = set(args.only.split(","))
    lib = os.path.join(ROOT, "pyopal_amd", "libmiopal.so")
    say(f"[{LABEL}] library md5 {hashlib.md5(open(lib, 'rb').read()).hexdigest()[:12]}, reps {args.reps}, scale {args.scale}")
    rng = np.random.default_rng(2026)
    q53 = _data.encode(_data.README_QUERY)
    q300 = _data.random_protein(rng, 300)
    if only & {"A", "B"}:
        n = int(1_000_000 * args.scale)
        off = np.arange(n + 1, dtype=np.int64) * 300
        res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
        db = _capi.DeviceDatabase(res, off, 24)
        if "A" in only:
            for mode in ("score", "end", "full"):
                leg("A 1M x 300 Q=53 ", db, q53, mode, "sw", 53.0 * n * 300)
        if "B" in only:
            leg("B 1M x 300 Q=300", db, q300, "full", "sw", 300.0 * n * 300)
        db.close()
    if "C" in only:
        n = int(500_000 * args.scale)
        lengths = np.clip(rng.lognormal(5.6, 0.6, size=n), 20, 8000).astype(np.int64)
        res, off = _data.random_db(rng, lengths)
        db = _capi.DeviceDatabase(res, off, 24)
        leg("C 500k log-normal Q=53", db, q53, "score", "nw", 53.0 * float(off[-1]))
        db.close()


if __name__ == "__main__":
    main()
