"""Hit searches (every target at or above a threshold, compacted on the device) against the routes they replace in the
PARENT build - the plain search plus a numpy filter on the host, and the top-k selection where 100 hits are wanted -
same inputs, one process per build, the two builds alternately. Per case: a warm-up call, then the median of 5.
  - headline (Q = 53 x 1M x 300, SW, 3/1), score and end: search_hits at a threshold that keeps about 100 targets,
    about 100 000, and every target (INT_MIN), against the parent's search + filter (and its search_top(k = 100));
  - 1000 queries (20-64 aa) x 20k x 300 and 256 queries x 1M x 300 at about 100 hits per query: search_batch_hits
    against the parent's search_batch + filter.
The parent is a built checkout of the parent commit (--parent DIR: its pyopal_amd package and tests/_data.py are
used, nothing of this tree). The thresholds come from the plain search's score quantiles in either process (the same
data, so the same numbers). Writes profiles/hits_quick.txt.
Kernel times of the three launches: rocprofv3 --kernel-trace --stats -- python tools/quick_hits.py --child new
--only-headline.
Usage: python tools/quick_hits.py --parent DIR [--rounds N] [--reps N] [--no-1m-batch]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = list("ARNDCQEGHILKMFPSTWYV")


def median_ms(reps, call):
    import numpy as np
    call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(time.perf_counter() - t)
    return float(np.median(times)) * 1e3


def child(which, tree, reps, only_headline, batch_1m):
    """One process of one build: `new` times the hit searches of this tree, `parent` the routes of the parent's."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import numpy as np
    import _data
    from pyopal_amd import _capi
    from pyopal_amd.matrices import ScoringMatrix

    new = which == "new"
    out = {"library": hashlib.md5(open(_capi.LIB_PATH, "rb").read()).hexdigest()[:12], "cases": {}}
    B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
    rng = np.random.default_rng(2026)
    n = 1_000_000
    off = np.arange(n + 1, dtype=np.int64) * 300
    res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
    db = _capi.DeviceDatabase(res, off, 24)
    query = _data.encode(_data.README_QUERY)

    def filtered(full, threshold):
        keep = np.nonzero(full["score"] >= threshold)[0]
        return {key: (keep if key == "target" else full[key][keep]) for key in list(full) + ["target"]}

    for mode in ("score", "end"):
        full = db.search(query, B62, 3, 1, mode, "sw")
        s = np.sort(full["score"])
        for label, threshold in (("100", int(s[-100])), ("100k", int(s[-100_000])), ("all", -(2 ** 31))):
            hits = int(np.count_nonzero(full["score"] >= threshold))
            case = f"headline {mode:5s} keep ~{label:4s} ({hits} hits)"
            if new:
                got = db.search_hits(query, B62, 3, 1, mode, "sw", min_score=threshold)
                want = filtered(full, threshold)
                assert got["count"] == hits and all(np.array_equal(got[key], want[key]) for key in want)
                out["cases"][case] = median_ms(reps, lambda: db.search_hits(query, B62, 3, 1, mode, "sw", min_score=threshold))
            else:
                out["cases"][case] = median_ms(reps, lambda: filtered(db.search(query, B62, 3, 1, mode, "sw"), threshold))
                if label == "100":
                    out["cases"][case + " [parent: search_top k=100]"] = median_ms(
                        reps, lambda: db.search_top(query, B62, 3, 1, mode, "sw", k=100))
        out["cases"][f"headline {mode:5s} plain search, no filter"] = median_ms(reps, lambda: db.search(query, B62, 3, 1, mode, "sw"))
    if only_headline:
        return out

    def batch(label, database, queries, mode, reps):
        # a threshold per query that keeps about 100 targets, from a sample of the plain scores of that query
        m = database.count
        thresholds = []
        for q in queries:
            sample = database.search(q, B62, 3, 1, "score", "sw", 0, min(m, 20_000))["score"]
            thresholds.append(int(np.sort(sample)[-max(1, (100 * len(sample)) // m)]))
        t = np.array(thresholds, dtype=np.int32)
        if new:
            got = database.search_batch_hits(queries, B62, 3, 1, mode, "sw", min_score=t)
            case = f"{label} {mode:5s} ({int(got['offsets'][-1]) // len(queries)} hits per query)"
            out["cases"][case] = median_ms(reps, lambda: database.search_batch_hits(queries, B62, 3, 1, mode, "sw", min_score=t))
        else:
            def route():
                dense = database.search_batch(queries, B62, 3, 1, mode, "sw")
                r, i = np.nonzero(dense["score"] >= t[:, None])
                return {key: dense[key][r, i] for key in dense}, np.bincount(r, minlength=len(queries))

            counts = route()[1]
            case = f"{label} {mode:5s} ({int(counts.sum()) // len(queries)} hits per query)"
            out["cases"][case] = median_ms(reps, route)

    short = [_data.encode("".join(rng.choice(LETTERS, size=int(L)))) for L in rng.integers(20, 65, size=1000)]
    m = 20_000
    small = _capi.DeviceDatabase(np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=m * 300)]),
                                 np.arange(m + 1, dtype=np.int64) * 300, 24)
    for mode in ("score", "end"):
        batch("1000 q (20-64 aa) x 20k x 300", small, short, mode, reps)
    if batch_1m:
        for mode in ("score", "end"):
            batch("256 q (20-64 aa) x 1M x 300", db, short[:256], mode, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2, help="processes per build, alternating")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-headline", action="store_true")
    ap.add_argument("--no-1m-batch", action="store_true")
    ap.add_argument("--child", choices=["new", "parent"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "hits_quick.txt"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.child, args.tree, args.reps, args.only_headline, not args.no_1m_batch)), flush=True)
        return
    if not args.parent:
        ap.error("--parent DIR is required")
    runs = {"new": [], "parent": []}
    for _ in range(args.rounds):
        for which, tree in (("new", ROOT), ("parent", os.path.abspath(args.parent))):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--tree", tree, "--reps", str(args.reps)]
            cmd += ["--only-headline"] if args.only_headline else []
            cmd += ["--no-1m-batch"] if args.no_1m_batch else []
            env = {k: v for k, v in os.environ.items() if k != "MIOPAL_LIBRARY"}
            done = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree, timeout=900)
            if done.returncode != 0:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                sys.exit(f"the {which} process failed with {done.returncode}")
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            runs[which].append(json.loads(line[len("RESULT "):]))
            print(f"{which}: done", flush=True)
    lines = [f"tools/quick_hits.py: {args.rounds} processes per build, alternating; per process a warm-up and the median of "
             f"{args.reps} calls (3 for 256 x 1M); below: the median over the processes, ms",
             f"this build {runs['new'][0]['library']} (hit searches)   parent {runs['parent'][0]['library']} "
             f"(plain search + numpy filter on the host; search_top where marked)", ""]
    for which in ("new", "parent"):
        lines.append("this build:" if which == "new" else "parent:")
        for case in runs[which][0]["cases"]:
            values = sorted(r["cases"][case] for r in runs[which])
            lines.append(f"  {case:72s} {values[len(values) // 2]:9.3f}   (processes: {', '.join(f'{v:.3f}' for v in values)})")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
