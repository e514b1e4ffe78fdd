"""The aligned occurrence search (miopalSearchOccurrencesAligned: where every occurrence starts, and its operations) on
the headline database, beside the call it extends and the call whose later passes it shares, in one process:
  - miopalSearchOccurrences, Q = 53 x 1M x 300, HW at 11/1, the default window (the query's length), at the cuts that
    give about 1e3 and about 1e5 occurrences (tools/quick_occurrences.py's: 34 and 15 on this database);
  - miopalSearchOccurrencesAligned with starts only, and with operations; per case the routing of the alignment stage
    (miopalLastOccurrenceAlignRouting: lanes, wavefronts, chunks, longest window);
  - miopalAlignPairs `full` over the distinct targets of the same occurrences: the yardstick of the shared passes (it
    runs a forward pass over whole targets first, which the occurrence search has in its sweeps).
Per case: a warm-up call, then the median of --reps calls, host time of the whole call. On the way the best occurrence
of every target is held to the pair list's alignment of that target. Writes profiles/occurrence_alignments_quick.txt.
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/quick_occurrence_alignments.py --reps 2 --output /dev/null
(a run of its own, no counters); the figures of one such run are kept beside the table in
profiles/occurrence_alignments_kernel_trace.txt, which this tool does not write.
Usage: python tools/quick_occurrence_alignments.py [--reps N] [--targets N] [--output FILE]"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(reps, call):
    import numpy as np
    call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(time.perf_counter() - t)
    return float(np.median(times)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--targets", type=int, default=1_000_000)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "occurrence_alignments_quick.txt"))
    args = ap.parse_args()
    import numpy as np
    import _data
    from pyopal_amd import _capi
    from pyopal_amd.matrices import ScoringMatrix

    B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
    rng = np.random.default_rng(2026)
    n = args.targets
    off = np.arange(n + 1, dtype=np.int64) * 300
    res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
    db = _capi.DeviceDatabase(res, off, 24)
    query = _data.encode(_data.README_QUERY)
    lines = [f"tools/quick_occurrence_alignments.py: Q = {len(query)} x {n} x 300, HW at 11/1, window = Q; a warm-up and the "
             f"median of {args.reps} calls, host time of the whole call, ms",
             f"library {hashlib.md5(open(_capi.LIB_PATH, 'rb').read()).hexdigest()[:12]}", ""]

    plain = db.search(query, B62, 11, 1, "end", "hw")
    s = np.sort(plain["score"])
    for label, cut in (("~1e3", int(s[-min(1000, n)])), ("~1e5", int(s[-min(100_000, n)]))):
        call = lambda **kw: db.search_occurrence_alignments(query, B62, 11, 1, "hw", min_score=cut, **kw)   # noqa: E731
        want = db.search_occurrences(query, B62, 11, 1, "hw", min_score=cut)
        got = call()
        routing = db.last_occurrence_align_routing()
        only = call(operations=False)
        routing_only = db.last_occurrence_align_routing()
        for key in ("target", "score", "end_t", "end_q"):
            assert got[key].tobytes() == want[key].tobytes() == only[key].tobytes(), (label, key)
        assert np.array_equal(only["start_t"], got["start_t"]) and np.array_equal(only["start_q"], got["start_q"])
        # the best occurrence of every target is what the pair list's `full` alignment of that target finds
        distinct, first = np.unique(got["target"], return_index=True)
        pair_query = np.zeros(len(distinct), dtype=np.int32)
        pairs = db.align_pairs([query], pair_query, distinct, B62, 11, 1, "full", "hw")
        pair_routing = db.last_pair_routing()
        best = np.array([lo + int(np.argmax(got["score"][lo:hi])) for lo, hi in zip(first, list(first[1:]) + [got["count"]])])
        for mine, theirs in (("score", "score"), ("end_t", "end_t"), ("start_t", "start_t"), ("start_q", "start_q")):
            assert np.array_equal(got[mine][best], pairs[theirs]), (label, mine)
        assert all(got["aln"][k].tolist() == pairs["aln"][p].tolist() for p, k in enumerate(best[:2000].tolist()))
        ms = {"occurrences": median_ms(args.reps, lambda: db.search_occurrences(query, B62, 11, 1, "hw", min_score=cut)),
              "starts only": median_ms(args.reps, lambda: call(operations=False)),
              "starts + operations": median_ms(args.reps, call),
              "pair list, full": median_ms(args.reps, lambda: db.align_pairs([query], pair_query, distinct, B62, 11, 1, "full", "hw"))}
        lines.append(f"  cut {cut:4d} ({label}): {got['count']} occurrences in {len(distinct)} targets, "
                     f"{len(got['aln_flat'])} operations")
        lines.append(f"    miopalSearchOccurrences{'':45s} {ms['occurrences']:9.3f}")
        lines.append(f"    miopalSearchOccurrencesAligned, starts only      routing {str(routing_only):28s} {ms['starts only']:9.3f}")
        lines.append(f"    miopalSearchOccurrencesAligned, with operations  routing {str(routing):28s} {ms['starts + operations']:9.3f}")
        lines.append(f"    miopalAlignPairs full, the {len(distinct)} distinct targets, routing {str(list(pair_routing)):20s} "
                     f"{ms['pair list, full']:9.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.output, "w") as f:
        f.write(text)
    db.close()


if __name__ == "__main__":
    main()
