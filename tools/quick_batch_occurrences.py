"""The occurrence search of a panel (miopalSearchBatchOccurrences) beside the loop of single-query calls it replaces,
in one process:
  - a panel of 96 queries of 8 .. 24 residues over 4 letters (match 5, mismatch -4, gaps 3/1) against reads of 150
    residues, HW, each query's cut its exact-match score; a copy of one panel query is planted in 0.5 % of the reads and
    the shortest queries also match by chance, so that about 1 % of the reads have a site;
  - at 200 000 reads and at 2 000 reads: the ONE call of search_batch_occurrences, and the loop of 96 search_occurrences
    calls (the code the batch form does not alter), alternating, a warm-up of each and then the median of --reps
    repetitions, host time of the whole call (every call ends in the download of its answer);
  - on the way the two answers are compared, array by array.
Writes profiles/batch_occurrences_timing.txt. Kernel times: a run of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/quick_batch_occurrences.py --batch-only --reps 3 --output /dev/null
whose figures are added to that file by hand.
Usage: python tools/quick_batch_occurrences.py [--reps N] [--reads N[,N...]] [--batch-only] [--output FILE]"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("target", "score", "end_t", "end_q")


def timed(call):
    t = time.perf_counter()
    call()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--reads", default="200000,2000")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "batch_occurrences_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    from pyopal_amd import _capi

    matrix = np.where(np.eye(4, dtype=bool), 5, -4).astype(np.int32).ravel()
    rng = np.random.default_rng(2026)
    panel = [rng.integers(0, 4, size=int(q)).astype(np.uint8) for q in rng.integers(8, 25, size=96)]
    cuts = [5 * len(q) for q in panel]
    lines = [f"tools/quick_batch_occurrences.py: a panel of {len(panel)} queries of 8 .. 24 residues over 4 letters against reads of "
             f"150 residues, HW at 3/1, cut = the exact-match score, window = the query's length; a warm-up, then the median of "
             f"{args.reps} repetitions, host time of the whole call, ms",
             f"library {hashlib.md5(open(_capi.LIB_PATH, 'rb').read()).hexdigest()[:12]}", ""]
    for n in (int(x) for x in args.reads.split(",")):
        reads = rng.integers(0, 4, size=(n, 150)).astype(np.uint8)
        for read in rng.choice(n, size=max(n // 200, 1), replace=False):
            q = panel[int(rng.integers(0, len(panel)))]
            at = int(rng.integers(0, 150 - len(q) + 1))
            reads[read, at:at + len(q)] = q
        db = _capi.DeviceDatabase(np.ascontiguousarray(reads.ravel()), np.arange(n + 1, dtype=np.int64) * 150, 4)
        batch = lambda: db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts)   # noqa: E731
        loop = lambda: [db.search_occurrences(q, matrix, 3, 1, "hw", min_score=c) for q, c in zip(panel, cuts)]   # noqa: E731
        got = batch()
        routing = db.last_batch_occurrence_routing()
        with_site = len(set(got["target"].tolist()))
        if not args.batch_only:
            parts = loop()
            assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum([p["count"] for p in parts])]))
            for key in KEYS:
                assert np.array_equal(got[key], np.concatenate([p[key] for p in parts])), key
        tb, tl = [], []
        for _ in range(args.reps):
            tb.append(timed(batch))
            if not args.batch_only:
                tl.append(timed(loop))
        b = float(np.median(tb)) * 1e3
        lines.append(f"  {n:7d} reads: {int(got['offsets'][-1])} occurrences, {with_site} reads with a site ({100.0 * with_site / n:.2f} %), "
                     f"routing {routing}")
        lines.append(f"      one call of search_batch_occurrences      {b:9.3f}   (min {min(tb) * 1e3:.3f}, max {max(tb) * 1e3:.3f})")
        if not args.batch_only:
            loop_ms = float(np.median(tl)) * 1e3
            lines.append(f"      loop of {len(panel)} search_occurrences calls       {loop_ms:9.3f}   (min {min(tl) * 1e3:.3f}, max {max(tl) * 1e3:.3f})")
            lines.append(f"      loop / one call                            {loop_ms / b:9.2f}")
        db.close()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
