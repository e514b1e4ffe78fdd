"""The aligned occurrence search of a panel (miopalSearchBatchOccurrencesAligned) beside the loop of single-query calls
it replaces, in one process:
  - tools/quick_batch_occurrences.py's panel and reads: 96 queries of 8 .. 24 residues over 4 letters (match 5, mismatch
    -4, gaps 3/1) against reads of 150 residues, HW, each query's cut its exact-match score, about 1 % of the reads with
    a site; at 200 000 reads and at 2 000 reads;
  - the ONE call of search_batch_occurrence_alignments and the loop of 96 search_occurrence_alignments calls (the code
    the panel form does not alter), with operations and starts only, and search_batch_occurrences alone beside them -
    what the stage costs on top of the sweeps; all alternating, a warm-up of each and then the median of --reps
    repetitions, host time of the whole call (every call ends in the download of its answer);
  - on the way the answers are compared, array by array.
Writes profiles/batch_occurrence_alignments_timing.txt. Kernel times: a run of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/quick_batch_occurrence_alignments.py --batch-only --reps 3 --output /dev/null
whose figures are added to that file by hand.
Usage: python tools/quick_batch_occurrence_alignments.py [--reps N] [--reads N[,N...]] [--batch-only] [--output FILE]"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("target", "score", "end_t", "end_q", "start_t", "start_q")


def timed(call):
    t = time.perf_counter()
    call()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--reads", default="200000,2000")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "batch_occurrence_alignments_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    from pyopal_amd import _capi

    matrix = np.where(np.eye(4, dtype=bool), 5, -4).astype(np.int32).ravel()
    rng = np.random.default_rng(2026)
    panel = [rng.integers(0, 4, size=int(q)).astype(np.uint8) for q in rng.integers(8, 25, size=96)]
    cuts = [5 * len(q) for q in panel]
    lines = [f"tools/quick_batch_occurrence_alignments.py: a panel of {len(panel)} queries of 8 .. 24 residues over 4 letters against "
             f"reads of 150 residues, HW at 3/1, cut = the exact-match score, window = the query's length; a warm-up, then the "
             f"median of {args.reps} repetitions, host time of the whole call, ms",
             f"library {hashlib.md5(open(_capi.LIB_PATH, 'rb').read()).hexdigest()[:12]}", ""]
    slower = []
    for n in (int(x) for x in args.reads.split(",")):
        reads = rng.integers(0, 4, size=(n, 150)).astype(np.uint8)
        for read in rng.choice(n, size=max(n // 200, 1), replace=False):
            q = panel[int(rng.integers(0, len(panel)))]
            at = int(rng.integers(0, 150 - len(q) + 1))
            reads[read, at:at + len(q)] = q
        db = _capi.DeviceDatabase(np.ascontiguousarray(reads.ravel()), np.arange(n + 1, dtype=np.int64) * 150, 4)
        ends = lambda: db.search_batch_occurrences(panel, matrix, 3, 1, "hw", min_score=cuts)   # noqa: E731
        calls = {}
        for ops in (True, False):
            calls[ops] = (
                lambda ops=ops: db.search_batch_occurrence_alignments(panel, matrix, 3, 1, "hw", min_score=cuts, operations=ops),
                lambda ops=ops: [db.search_occurrence_alignments(q, matrix, 3, 1, "hw", min_score=c, operations=ops)
                                 for q, c in zip(panel, cuts)])
        got = calls[True][0]()
        sweeps, stage = db.last_batch_occurrence_routing(), db.last_batch_occurrence_align_routing()
        with_site = len(set(got["target"].tolist()))
        ends()
        if not args.batch_only:
            for ops in (True, False):
                mine, parts = calls[ops][0](), calls[ops][1]()
                assert np.array_equal(mine["offsets"], np.concatenate([[0], np.cumsum([p["count"] for p in parts])]))
                for key in KEYS + (("aln_flat",) if ops else ()):
                    assert np.array_equal(mine[key], np.concatenate([p[key] for p in parts])), key
        else:
            calls[False][0]()
        times = {name: [] for name in ("ends", "full", "full loop", "starts", "starts loop")}
        for _ in range(args.reps):
            times["ends"].append(timed(ends))
            for ops, name in ((True, "full"), (False, "starts")):
                times[name].append(timed(calls[ops][0]))
                if not args.batch_only:
                    times[name + " loop"].append(timed(calls[ops][1]))
        ms = {name: float(np.median(t)) * 1e3 for name, t in times.items() if t}
        spread = lambda name: f"(min {min(times[name]) * 1e3:.3f}, max {max(times[name]) * 1e3:.3f})"   # noqa: E731
        lines.append(f"  {n:7d} reads: {int(got['offsets'][-1])} occurrences, {with_site} reads with a site ({100.0 * with_site / n:.2f} %), "
                     f"sweeps {sweeps}, stage {stage}")
        lines.append(f"      one call of search_batch_occurrences (ends only)            {ms['ends']:9.3f}   {spread('ends')}")
        for name, what in (("full", "with operations"), ("starts", "starts only")):
            lines.append(f"    {what}:")
            lines.append(f"      one call of search_batch_occurrence_alignments              {ms[name]:9.3f}   {spread(name)}")
            lines.append(f"        of which the stage (the call less the ends-only call)     {ms[name] - ms['ends']:9.3f}")
            if not args.batch_only:
                loop = ms[name + " loop"]
                lines.append(f"      loop of {len(panel)} search_occurrence_alignments calls               {loop:9.3f}   {spread(name + ' loop')}")
                lines.append(f"      loop / one call                                             {loop / ms[name]:9.2f}")
                if ms[name] > loop:
                    slower.append((n, what))
        db.close()
    if not args.batch_only:
        lines.append("")
        lines.append("the one call is no slower than the loop at either size: " +
                     ("yes" if not slower else "NO - slower at " + ", ".join(f"{n} reads {what}" for n, what in slower)))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
