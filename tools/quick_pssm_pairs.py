"""The k best hits and pair lists for PSSMs (miopalSearchPssmTop, miopalAlignPairsPssm) against the route a caller had
before them, timed in one process on one resident handle: search_pssm for all the scores, a top-k on the host, a
`subset` handle of the chosen targets and search_pssm(mode="full") on it. Seeded data, a warm-up of every shape, then
median and spread (min .. max) of --reps calls, host clock around calls that end in a synchronise. PSSMs derived from
random sequences under BLOSUM62 (24 letters), 1M targets of 300 residues. --out FILE appends every line printed to FILE
(profiles/pssm_top_pairs.txt is made of such runs).
  A  top hits with alignments, Q = 53 and Q = 300, k = 10 and k = 4096:
       new: search_pssm_top, then align_pairs_pssm of the chosen targets    old: the route above
  B  10^5 pairs of ONE 300-row PSSM (its table fits LDS: the lane-per-pair kernels), score and full:
       production routing, FORCE_LANE_PER_PAIR, NO_PERPAIR, alternated;     old: subset handle + search_pssm
  C  10^5 pairs over 200 PSSMs of 150 rows (30 000 rows: one wavefront per pair), score and full:
       production routing (no other route exists for this list);             old: per PSSM a subset handle + search_pssm
Usage: python tools/quick_pssm_pairs.py [--reps N] [--only A,B,C] [--label NAME] [--scale F] [--out FILE]"""
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
ap.add_argument("--scale", type=float, default=1.0, help="fraction of the targets and pairs (a quick look)")
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


def timed(calls):
    """every call once to warm up, then --reps rounds of all of them in turn -> {name: seconds per call}"""
    times = {name: [] for name, _ in calls}
    for rep in range(args.reps + 1):
        for name, call in calls:
            t0 = time.perf_counter()
            call()
            if rep >= 1:
                times[name].append(time.perf_counter() - t0)
    return times


def report(leg, times, notes):
    for name, t in times.items():
        say(f"[{LABEL}] {leg} {name:22s}: median {np.median(t) * 1e3:9.3f} ms  (min {min(t) * 1e3:9.3f} .. max "
            f"{max(t) * 1e3:9.3f})  {notes.get(name, '')}")


def derived(rng, length):
    query = _data.random_protein(rng, length)
    return np.ascontiguousarray(B62.reshape(24, 24)[query]), query


def host_top(score, k):
    """what sorted(results, key=score, reverse=True)[:k] costs on arrays: the k best, equal scores by index"""
    if k >= len(score):
        return np.argsort(-score.astype(np.int64), kind="stable").astype(np.int64)
    bound = np.partition(score, len(score) - k)[len(score) - k]   # the k-th largest
    above = np.flatnonzero(score > bound)
    chosen = np.concatenate([above, np.flatnonzero(score == bound)[:k - len(above)]])
    return chosen[np.lexsort((chosen, -score[chosen].astype(np.int64)))].astype(np.int64)


def subset_full(db, rows, cons, targets, mode="full"):
    sub = db.subset(targets)
    try:
        return sub.search_pssm(rows, cons, 3, 1, mode, "sw")
    finally:
        sub.close()


def main():
    only = set(args.only.split(","))
    lib = os.path.join(ROOT, "pyopal_amd", "libmiopal.so")
    say(f"[{LABEL}] library md5 {hashlib.md5(open(lib, 'rb').read()).hexdigest()[:12]}, reps {args.reps}, scale {args.scale}")
    rng = np.random.default_rng(2027)
    n = int(1_000_000 * args.scale)
    n_pairs = int(100_000 * args.scale)
    off = np.arange(n + 1, dtype=np.int64) * 300
    res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
    db = _capi.DeviceDatabase(res, off, 24)
    notes = {}

    if "A" in only:
        for length in (53, 300):
            rows, cons = derived(rng, length)
            for k in (10, 4096):
                def new():
                    top = db.search_pssm_top(rows, 3, 1, "score", "sw", 0, None, k)
                    hits = top["target"][:top["count"]]
                    out = db.align_pairs_pssm([rows], [cons], np.zeros(len(hits), dtype=np.int32), hits, 3, 1, "full", "sw")
                    notes["top + pair list"] = f"pair routing {db.last_pair_routing()}"
                    return hits, out

                def old():
                    score = db.search_pssm(rows, None, 3, 1, "score", "sw")["score"]
                    hits = host_top(score, k)
                    return hits, subset_full(db, rows, cons, hits)

                a, b = new(), old()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]["aln_flat"], b[1]["aln_flat"]), "the two routes disagree"
                times = timed([("top + pair list", new), ("search + host + subset", old)])
                report(f"A {n} x 300 Q={length:3d} k={k:4d} full", times, notes)

    if "B" in only:
        rows, cons = derived(rng, 300)
        targets = rng.integers(0, n, size=n_pairs).astype(np.int64)
        which = np.zeros(n_pairs, dtype=np.int32)
        for mode in ("score", "full"):
            calls = []
            for name, switch in (("production", None), ("FORCE_LANE_PER_PAIR", "FORCE_LANE_PER_PAIR"), ("NO_PERPAIR", "NO_PERPAIR")):
                def call(name=name, switch=switch):
                    with _capi.tuning(**({switch: "1"} if switch else {})):
                        out = db.align_pairs_pssm([rows], [cons], which, targets, 3, 1, mode, "sw")
                    notes[name] = f"pair routing {db.last_pair_routing()}"
                    return out
                calls.append((name, call))
            calls.append(("subset + search_pssm", lambda: subset_full(db, rows, cons, targets, mode)))
            want = calls[-1][1]()
            for name, call in calls[:-1]:
                got = call()
                assert all(np.array_equal(got[key], want[key]) for key in got if key[0] != "_" and key != "aln"), (name, mode)
            report(f"B {n_pairs} pairs, one PSSM of 300 rows, {mode:5s}", timed(calls), notes)

    if "C" in only:
        pssms = [derived(rng, 150) for _ in range(200)]
        which = rng.integers(0, len(pssms), size=n_pairs).astype(np.int32)
        targets = rng.integers(0, n, size=n_pairs).astype(np.int64)
        for mode in ("score", "full"):
            def new():
                out = db.align_pairs_pssm([p[0] for p in pssms], [p[1] for p in pssms], which, targets, 3, 1, mode, "sw")
                notes["production"] = f"pair routing {db.last_pair_routing()}"
                return out

            def old():
                return [subset_full(db, pssms[m][0], pssms[m][1], targets[which == m], mode) for m in range(len(pssms))]

            got, want = new(), old()
            for m in range(len(pssms)):
                assert np.array_equal(got["score"][which == m], want[m]["score"]), (m, mode)
            report(f"C {n_pairs} pairs, 200 PSSMs of 150 rows, {mode:5s}", timed([("production", new), ("loop of subsets", old)]), notes)
    db.close()


if __name__ == "__main__":
    main()
