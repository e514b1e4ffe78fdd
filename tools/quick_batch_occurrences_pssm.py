"""The occurrence search of a panel of PSSMs (miopalSearchPssmBatchOccurrences, ...Aligned) beside the loop of single-PSSM
calls it replaces, in one process:
  - a library of 200 PSSMs of 6 .. 20 rows over 4 letters (A, C, G, T), HW at 3/1: a GC-rich motif each, its rows
    weight (4, 5 or 6, per position) on the motif's letter and -4 elsewhere, the cut the exact-match score, the window
    the PSSM's height; reads of 150 residues, AT-rich (0.45 / 0.05 / 0.05 / 0.45) so that the short motifs seldom match
    by chance, with a copy of one motif planted in 0.9 % of them: about 1 % of the reads hold a site;
  - at 200 000 reads and at 2 000 reads: the ONE call of search_batch_occurrences_pssm and the loop of 200
    search_occurrences_pssm calls (code this form does not alter), alternating, a warm-up of each and then the median
    of --reps repetitions, host time of the whole call (every call ends in the download of its answer); the same for
    the aligned form against the loop of search_occurrence_alignments_pssm, the motif as consensus;
  - the cost of the row-filled table: the same motifs as a panel of SEQUENCES through search_batch_occurrences, and
    as PSSMs whose rows are the matrix rows of those sequences - identical cells, so what differs is the table fill
    and the upload - alternating in the same way;
  - on the way the answers are compared, array by array.
Writes profiles/batch_occurrences_pssm_timing.txt. Kernel times: a run of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/quick_batch_occurrences_pssm.py --batch-only --reps 3 --output /dev/null
whose figures are added to that file by hand.
Usage: python tools/quick_batch_occurrences_pssm.py [--reps N] [--reads N[,N...]] [--batch-only] [--output FILE]"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("target", "score", "end_t", "end_q")
ALIGNED = KEYS + ("start_t", "start_q", "aln_flat")


def timed(call):
    t = time.perf_counter()
    call()
    return time.perf_counter() - t


def joined(parts, keys, np):
    out = {"offsets": np.concatenate([[0], np.cumsum([p["count"] for p in parts])])}
    for key in keys:
        out[key] = np.concatenate([p[key] for p in parts])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--reads", default="200000,2000")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "batch_occurrences_pssm_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    from pyopal_amd import _capi

    matrix = np.where(np.eye(4, dtype=bool), 5, -4).astype(np.int32).ravel()
    rng = np.random.default_rng(2027)
    motifs = [rng.choice(4, size=int(q), p=(0.05, 0.45, 0.45, 0.05)).astype(np.uint8) for q in rng.integers(6, 21, size=200)]
    panel = []
    for m in motifs:
        rows = np.full((len(m), 4), -4, dtype=np.int32)
        rows[np.arange(len(m)), m] = rng.integers(4, 7, size=len(m))
        panel.append(rows)
    cuts = [int(rows.max(axis=1).sum()) for rows in panel]
    as_rows = [np.ascontiguousarray(matrix.reshape(4, 4)[m]) for m in motifs]
    plain_cuts = [5 * len(m) for m in motifs]
    lines = [f"tools/quick_batch_occurrences_pssm.py: a library of {len(panel)} PSSMs of 6 .. 20 rows over 4 letters against reads of "
             f"150 residues, HW at 3/1, cut = the exact-match score, window = the PSSM's height; a warm-up, then the median of "
             f"{args.reps} repetitions, host time of the whole call, ms",
             f"library {hashlib.md5(open(_capi.LIB_PATH, 'rb').read()).hexdigest()[:12]}", ""]

    def compare(name, one, loop, reps, keys):
        """one warm-up of each (compared), then alternating repetitions -> the lines of the report"""
        got = one()
        if loop is not None:
            want = loop()
            assert np.array_equal(got["offsets"], want["offsets"]), name
            for key in keys:
                assert np.array_equal(got[key], want[key]), (name, key)
        t1, t2 = [], []
        for _ in range(reps):
            t1.append(timed(one))
            if loop is not None:
                t2.append(timed(loop))
        return got, t1, t2

    for n in (int(x) for x in args.reads.split(",")):
        reads = rng.choice(4, size=(n, 150), p=(0.45, 0.05, 0.05, 0.45)).astype(np.uint8)
        for read in rng.choice(n, size=max(n * 9 // 1000, 1), replace=False):
            m = motifs[int(rng.integers(0, len(motifs)))]
            at = int(rng.integers(0, 150 - len(m) + 1))
            reads[read, at:at + len(m)] = m
        db = _capi.DeviceDatabase(np.ascontiguousarray(reads.ravel()), np.arange(n + 1, dtype=np.int64) * 150, 4)
        skip = args.batch_only
        # ends
        one = lambda: db.search_batch_occurrences_pssm(panel, 3, 1, "hw", min_score=cuts)   # noqa: E731
        loop = lambda: joined([db.search_occurrences_pssm(r, 3, 1, "hw", min_score=c) for r, c in zip(panel, cuts)], KEYS, np)   # noqa: E731
        got, t1, t2 = compare("ends", one, None if skip else loop, args.reps, KEYS)
        one()
        routing, groups = db.last_batch_occurrence_routing(), db.last_batch_occurrence_groups()
        with_site = len(set(got["target"].tolist()))
        b = float(np.median(t1)) * 1e3
        lines.append(f"  {n:7d} reads: {int(got['offsets'][-1])} occurrences, {with_site} reads with a site ({100.0 * with_site / n:.2f} %), "
                     f"routing {routing}, groups {groups}")
        lines.append(f"      one call of search_batch_occurrences_pssm            {b:9.3f}   (min {min(t1) * 1e3:.3f}, max {max(t1) * 1e3:.3f})")
        if not skip:
            loop_ms = float(np.median(t2)) * 1e3
            lines.append(f"      loop of {len(panel)} search_occurrences_pssm calls            {loop_ms:9.3f}   (min {min(t2) * 1e3:.3f}, max {max(t2) * 1e3:.3f})")
            lines.append(f"      loop / one call                                      {loop_ms / b:9.2f}")
        # starts and alignments
        one = lambda: db.search_batch_occurrence_alignments_pssm(panel, motifs, 3, 1, "hw", min_score=cuts)   # noqa: E731
        loop = lambda: joined([db.search_occurrence_alignments_pssm(r, m, 3, 1, "hw", min_score=c)   # noqa: E731
                               for r, m, c in zip(panel, motifs, cuts)], ALIGNED, np)
        got, t1, t2 = compare("aligned", one, None if skip else loop, args.reps, ALIGNED)
        one()
        stage = db.last_batch_occurrence_align_routing()
        b = float(np.median(t1)) * 1e3
        lines.append(f"      one call of search_batch_occurrence_alignments_pssm  {b:9.3f}   (min {min(t1) * 1e3:.3f}, max {max(t1) * 1e3:.3f}), "
                     f"stage {stage}")
        if not skip:
            loop_ms = float(np.median(t2)) * 1e3
            lines.append(f"      loop of {len(panel)} search_occurrence_alignments_pssm calls  {loop_ms:9.3f}   (min {min(t2) * 1e3:.3f}, max {max(t2) * 1e3:.3f})")
            lines.append(f"      loop / one call                                      {loop_ms / b:9.2f}")
        # the row-filled table against the residue-filled one: identical cells
        one = lambda: db.search_batch_occurrences_pssm(as_rows, 3, 1, "hw", min_score=plain_cuts)   # noqa: E731
        plain = lambda: db.search_batch_occurrences(motifs, matrix, 3, 1, "hw", min_score=plain_cuts)   # noqa: E731
        got, t1, t2 = compare("table", one, plain, args.reps, KEYS)
        b, p = float(np.median(t1)) * 1e3, float(np.median(t2)) * 1e3
        lines.append(f"      the motifs as sequences, search_batch_occurrences    {p:9.3f}   (min {min(t2) * 1e3:.3f}, max {max(t2) * 1e3:.3f})")
        lines.append(f"      ... as PSSMs of the matrix's rows, ..._pssm           {b:9.3f}   (min {min(t1) * 1e3:.3f}, max {max(t1) * 1e3:.3f}), "
                     f"PSSM / plain {b / p:.3f}")
        lines.append("")
        db.close()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
