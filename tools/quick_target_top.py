"""The per-target selection (the m best queries of every target, folded on the device) against the route a caller has in
the PARENT build - the dense batched search plus a numpy reduction on the host - same inputs, one process per build,
the two builds alternately. Per case: a warm-up call, then the median and min..max of 5.
  - 256 queries (20-64 aa) x 1M x 300 and 1000 queries (20-64 aa) x 20k x 300, HW, 3/1, score and end, m = 1 and m = 8.
The parent is a built checkout of the parent commit (--parent DIR: its pyopal_amd package and tests/_data.py are
used, nothing of this tree). The first answer of this build is checked against the dense route of the same process on
the 20k case. Writes profiles/target_top_quick.txt.
Usage: python tools/quick_target_top.py --parent DIR [--rounds N] [--reps N] [--no-1m]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = list("ARNDCQEGHILKMFPSTWYV")


def timed_ms(reps, call):
    call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append((time.perf_counter() - t) * 1e3)
    return sorted(times)


def reduce_dense(np, dense, m):
    """column t of the dense [queries][targets] arrays: by (-score, query), the first m (every query a candidate;
    m <= queries): m arg-max passes, each of which takes the first of equal maxima - the lower query index - and
    strikes it out (no score of a search is INT_MIN). Faster here than one argpartition of 64-bit keys."""
    score = dense["score"]
    cols = np.arange(score.shape[1])
    work = score if m == 1 else score.copy()
    top = np.empty((m, score.shape[1]), dtype=np.int64)
    for j in range(m):
        top[j] = np.argmax(work, axis=0)
        if j + 1 < m:
            work[top[j], cols] = -(2 ** 31)
    cols = cols[None, :]
    out = {"query": top.T.astype(np.int32)}
    for key in dense:
        out[key] = np.ascontiguousarray(dense[key][top, cols].T)
    return out


def child(which, tree, reps, with_1m):
    """One process of one build: `new` times search_batch_target_top of this tree, `parent` the dense route."""
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
    short = [_data.encode("".join(rng.choice(LETTERS, size=int(L)))) for L in rng.integers(20, 65, size=1000)]

    def database(n):
        return _capi.DeviceDatabase(np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)]),
                                    np.arange(n + 1, dtype=np.int64) * 300, 24)

    def run(label, db, queries, check):
        for mode in ("score", "end"):
            for m in (1, 8):
                case = f"{label} {mode:5s} m = {m}"
                if new:
                    if check:
                        got = db.search_batch_target_top(queries, B62, 3, 1, mode, "hw", m=m)
                        want = reduce_dense(np, db.search_batch(queries, B62, 3, 1, mode, "hw"), m)
                        assert np.all(got["count"] == m) and all(np.array_equal(got[key], want[key]) for key in want), case
                    out["cases"][case] = timed_ms(reps, lambda: db.search_batch_target_top(queries, B62, 3, 1, mode, "hw", m=m))
                else:
                    out["cases"][case] = timed_ms(
                        reps, lambda: reduce_dense(np, db.search_batch(queries, B62, 3, 1, mode, "hw"), m))

    small = database(20_000)
    run("1000 q (20-64 aa) x 20k x 300", small, short, True)
    small.close()
    if with_1m:
        run("256 q (20-64 aa) x 1M x 300 ", database(1_000_000), short[:256], False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=1, help="processes per build, alternating")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--child", choices=["new", "parent"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "target_top_quick.txt"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.child, args.tree, args.reps, not args.no_1m)), flush=True)
        return
    if not args.parent:
        ap.error("--parent DIR is required")
    runs = {"new": [], "parent": []}
    for _ in range(args.rounds):
        for which, tree in (("new", ROOT), ("parent", os.path.abspath(args.parent))):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--tree", tree, "--reps", str(args.reps)]
            cmd += ["--no-1m"] if args.no_1m else []
            env = {k: v for k, v in os.environ.items() if k != "MIOPAL_LIBRARY"}
            done = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree, timeout=900)
            if done.returncode != 0:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                sys.exit(f"the {which} process failed with {done.returncode}")
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            runs[which].append(json.loads(line[len("RESULT "):]))
            print(f"{which}: done", flush=True)
    lines = [f"tools/quick_target_top.py: {args.rounds} process(es) per build, alternating; per process a warm-up and "
             f"{args.reps} calls; below: median (min .. max) over all calls of a build, ms; HW, BLOSUM62, 3/1",
             f"this build {runs['new'][0]['library']} (search_batch_target_top)   parent {runs['parent'][0]['library']} "
             f"(search_batch, dense, + numpy reduction on the host)", ""]
    lines.append(f"  {'case':46s} {'this build':>30s}   {'parent':>30s}")
    for case in runs["new"][0]["cases"]:
        cells = []
        for which in ("new", "parent"):
            values = sorted(v for r in runs[which] for v in r["cases"][case])
            cells.append(f"{values[len(values) // 2]:9.2f} ({values[0]:8.2f} .. {values[-1]:8.2f})")
        lines.append(f"  {case:46s} {cells[0]:>30s}   {cells[1]:>30s}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
