"""Pair-list alignment (miopalAlignPairs) against what it replaces. Seeded data, a warm-up of every shape, the median
of a few calls (and their spread, min .. max), host clock around calls that end in a synchronise. One process times ONE
tree (--tree: the root of a checkout with its library built, default this one), so that a job can alternate this
commit and its parent in one GPU visit; a tree without align_pairs (the parent) is timed on the calls it has.
  A  top_hits_many, 1000 queries of 20-64 aa x 20k x 300 uniform targets, k = 10, mode="full", SW and NW
  B  top_hits, one query of 53 aa x 1M x 300, mode="full", k = 10 and k = 4096
  C  10^6 pairs (1000 queries x their 1000 best of the 20k targets), score / end / full:
       this tree: align_pairs under the production routing, NO_PERPAIR and FORCE_LANE_PER_PAIR, alternated
       any tree:  the loop it replaces - per query a subset handle of its 1000 targets and one search of it
The forward kernel alone: run `--only forward` under rocprofv3 --kernel-trace --stats (a run of its own).
Usage: python tools/quick_pairs.py [--tree PATH] [--reps N] [--only A,B,C,forward] [--label NAME]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="A,B,C")
ap.add_argument("--label", default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data  # noqa: E402
import pyopal_amd as pyopal  # noqa: E402
from pyopal_amd import _capi  # noqa: E402
from pyopal_amd.matrices import ScoringMatrix  # noqa: E402

LETTERS = list("ARNDCQEGHILKMFPSTWYV")
LABEL = args.label or os.path.basename(ROOT)


def seqs(rng, lengths):
    return ["".join(rng.choice(LETTERS, size=int(L))) for L in lengths]


def timed(reps, call):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(min(t)) * 1e3, float(max(t)) * 1e3


def line(what, stats):
    print(f"[{LABEL}] {what}: median {stats[0]:9.2f} ms  (min {stats[1]:9.2f} .. max {stats[2]:9.2f})", flush=True)


def main():
    only = set(args.only.split(","))
    lib = os.path.join(ROOT, "pyopal_amd", "libmiopal.so")
    print(f"[{LABEL}] library md5 {hashlib.md5(open(lib, 'rb').read()).hexdigest()[:12]}, reps {args.reps}", flush=True)
    has_pairs = hasattr(_capi.DeviceDatabase, "align_pairs")
    B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
    rng = np.random.default_rng(2026)
    aligner = pyopal.Aligner(scoring_matrix="BLOSUM62")
    short = seqs(rng, rng.integers(20, 65, size=1000))
    small = pyopal.Database(seqs(rng, np.full(20000, 300)))
    if "A" in only:
        for algo in ("sw", "nw"):
            line(f"A top_hits_many 1000 q x 20k x 300 k=10 full {algo}",
                 timed(args.reps, lambda: aligner.top_hits_many(short, small, 10, mode="full", algorithm=algo)))
    if only & {"C", "forward"}:
        mirror = small._device_mirror(0)
        queries = [np.frombuffer(small.alphabet.encode(q), dtype=np.uint8) for q in short]
        top = mirror.search_batch_top(queries, B62, 3, 1, "score", "sw", k=1000)
        pair_target = np.ascontiguousarray(top["target"].reshape(-1))
        pair_query = np.repeat(np.arange(1000, dtype=np.int32), 1000)
        assert pair_target.min() >= 0
        cells = float(sum(len(q) for q in queries)) * 1000 * 300
        if "forward" in only and has_pairs:
            with _capi.tuning(FORCE_LANE_PER_PAIR="1"):
                for mode in ("score", "end"):
                    for _ in range(3):
                        mirror.align_pairs(queries, pair_query, pair_target, B62, 3, 1, mode, "sw")
            print(f"[{LABEL}] forward: 3 x score + 3 x end over 10^6 pairs, {cells:.3e} cells each", flush=True)
        if "C" in only:
            for mode in ("score", "end", "full"):
                if has_pairs:
                    routes = (("production", {}), ("NO_PERPAIR", {"NO_PERPAIR": "1"}),
                              ("FORCE_LANE_PER_PAIR", {"FORCE_LANE_PER_PAIR": "1"}))
                    times = {name: [] for name, _ in routes}
                    for rep in range(args.reps + 1):
                        for name, switches in routes:
                            with _capi.tuning(**switches):
                                t0 = time.perf_counter()
                                mirror.align_pairs(queries, pair_query, pair_target, B62, 3, 1, mode, "sw")
                                if rep:
                                    times[name].append(time.perf_counter() - t0)
                            if rep == 1:
                                times[name + " routing"] = mirror.last_pair_routing()
                    for name, _ in routes:
                        t = times[name]
                        line(f"C align_pairs 10^6 pairs {mode} sw, {name} (routing {times[name + ' routing']}, "
                             f"{cells / np.median(t) / 1e9:6.1f} GCUPS)",
                             (float(np.median(t)) * 1e3, min(t) * 1e3, max(t) * 1e3))

                def loop():
                    for i in range(1000):
                        sub = mirror.subset(pair_target[1000 * i:1000 * (i + 1)])
                        try:
                            sub.search(queries[i], B62, 3, 1, mode, "sw")
                        finally:
                            sub.close()
                line(f"C loop of 1000 subset handles + searches {mode} sw", timed(max(2, args.reps // 2), loop))
    if "B" in only:
        n = 1_000_000
        off = np.arange(n + 1, dtype=np.int64) * 300
        res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
        db = _capi.DeviceDatabase(res, off, 24)
        query = _data.encode(_data.README_QUERY)
        for k in (10, 4096):
            def parent_way():
                top = db.search_top(query, B62, 3, 1, "score", "sw", k=k)
                sub = db.subset(top["target"][:top["count"]])
                try:
                    sub.search(query, B62, 3, 1, "full", "sw")
                finally:
                    sub.close()
            line(f"B top-{k} of 1M x 300 then full, subset handle + search", timed(args.reps, parent_way))
            if has_pairs:
                def pair_way():
                    top = db.search_top(query, B62, 3, 1, "score", "sw", k=k)
                    t = top["target"][:top["count"]]
                    db.align_pairs([query], np.zeros(len(t), dtype=np.int32), t, B62, 3, 1, "full", "sw")
                line(f"B top-{k} of 1M x 300 then full, one align_pairs call", timed(args.reps, pair_way))
        db.close()


if __name__ == "__main__":
    main()
