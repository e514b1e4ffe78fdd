"""Significance searches (E-value cut, statistics gathered on the device) against the route they replace in the PARENT
build - the plain search, the dense score row downloaded, and the same fit and filter in numpy on the host - same
inputs, one process per build, the two builds alternately. Per case: a warm-up call, then the median of 5.
  - headline (Q = 53 x 1M x 300, SW, 3/1), score and end, at max_evalue 1e-3 and 10 - and at 1e5, a tenth of the
    targets, so that the write pass has something to write: search_significant against the parent's search + numpy fit
    + filter; beside them this build's search_hits at a raw threshold with a comparable hit count, and the plain search;
  - a database of log-normal lengths (500k targets, median 300, 30 .. 3000), score, at 1e-3 and 10;
  - 256 queries (20-64 aa) x 1M x 300 through the batch form against the parent's search_batch + numpy per row.
The parent is a built checkout of the parent commit (--parent DIR: its pyopal_amd package and tests/_data.py are used,
nothing of this tree). The length bins and the per-bin lengths of a database are computed once, outside the timed
calls, in either route. Writes profiles/significant_quick.txt.
Kernel times of the statistics and binned passes: rocprofv3 --kernel-trace --stats -- python tools/quick_significant.py
--child new --no-1m-batch.
Usage: python tools/quick_significant.py --parent DIR [--rounds N] [--reps N] [--no-1m-batch]"""
import argparse
import hashlib
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = list("ARNDCQEGHILKMFPSTWYV")
BINS = 128
GUMBEL = math.pi / math.sqrt(6.0)
GAMMA = 0.5772156649015329


def median_ms(reps, call):
    import numpy as np
    call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(time.perf_counter() - t)
    return float(np.median(times)) * 1e3


def length_bins(lengths):
    import numpy as np
    L = np.asarray(lengths, dtype=np.int64)
    e = np.zeros(L.shape, dtype=np.int64)
    for shift in (32, 16, 8, 4, 2, 1):
        e[(L >> (e + shift)) > 0] += shift
    m = np.where(e >= 2, (L >> np.maximum(e - 2, 0)) & 3, (L << np.maximum(2 - e, 0)) & 3)
    return np.where(L == 0, 0, 1 + 4 * e + m)


class HostFit:
    """include/miopal.h's procedure in numpy, for one database slice: what a caller of the parent build has to do"""

    def __init__(self, lengths):
        import numpy as np
        self.bins = length_bins(lengths)
        self.targets = np.bincount(self.bins, minlength=BINS)
        total = np.bincount(self.bins, weights=np.asarray(lengths, dtype=np.float64), minlength=BINS)
        self.held = self.targets > 0
        self.held[0] = False
        self.x = np.zeros(BINS)
        self.x[self.held] = np.log(total[self.held] / self.targets[self.held])
        self.n = int(self.targets[1:].sum())

    def line(self, score, keep):
        import numpy as np
        b = self.bins if keep is None else self.bins[keep]
        s = score.astype(np.float64) if keep is None else score[keep].astype(np.float64)
        n = np.bincount(b, minlength=BINS).astype(np.float64)
        S = np.bincount(b, weights=s, minlength=BINS)
        Q = np.bincount(b, weights=s * s, minlength=BINS)
        n[0] = S[0] = Q[0] = 0
        used, x = n.sum(), self.x
        if used < 3:
            return None
        Sn, Snx, Snxx, Ss, Sxs = used, (n * x).sum(), (n * x * x).sum(), S.sum(), (x * S).sum()
        denom = Sn * Snxx - Snx * Snx
        slope, intercept = 0.0, Ss / Sn
        if np.count_nonzero(n) > 1 and denom > 0:
            slope = (Sn * Sxs - Snx * Ss) / denom
            intercept = (Ss - slope * Snx) / Sn
        mean = intercept + slope * x
        resid = (Q - 2 * mean * S + n * mean * mean).sum()
        if not resid > 0:
            return None
        return mean, math.sqrt(resid / (used - 2))

    def hits(self, score, max_evalue, exclude_z=5.0):
        """-> indices of the significant targets (the whole procedure: refits, table, filter)"""
        import numpy as np
        fit = self.line(score, None)
        ceiling = None
        for _ in range(3):
            if fit is None or not exclude_z > 0:
                break
            mean, sigma = fit
            nxt = np.where(self.held, np.floor(mean + exclude_z * sigma), np.inf)
            if ceiling is not None and np.array_equal(nxt, ceiling):
                break
            ceiling = nxt
            fit = self.line(score, score <= ceiling[self.bins])
        if fit is None:
            return np.zeros(0, dtype=np.int64)
        mean, sigma = fit
        p = max_evalue / self.n
        if p >= 1:
            table = np.where(self.held, -np.inf, np.inf)
        else:
            z_cut = -(math.log(-math.log1p(-p)) + GAMMA) / GUMBEL
            table = np.where(self.held, np.ceil(mean + z_cut * sigma), np.inf)
        return np.nonzero(score >= table[self.bins])[0]


def child(which, tree, reps, batch_1m):
    """One process of one build: `new` times the significance searches of this tree, `parent` the route of the parent's."""
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
    query = _data.encode(_data.README_QUERY)

    def single(label, db, off, modes, cuts=(1e-3, 10.0)):
        host = HostFit(np.diff(off))
        for mode in modes:
            full = db.search(query, B62, 3, 1, mode, "sw")
            for cut in cuts:
                want = host.hits(full["score"], cut)
                case = f"{label} {mode:5s} E <= {cut:g} ({len(want)} hits)"
                if new:
                    got = db.search_significant(query, B62, 3, 1, mode, "sw", max_evalue=cut)
                    # (the host route sums in doubles: a threshold may sit one score apart where a cut is nearly an integer)
                    assert abs(got["count"] - len(want)) <= max(2, len(want) // 50), (got["count"], len(want))
                    out["cases"][case] = median_ms(reps, lambda: db.search_significant(query, B62, 3, 1, mode, "sw", max_evalue=cut))
                    if len(want):
                        raw = int(np.sort(full["score"])[-len(want)])
                        out["cases"][case + " [search_hits at a raw threshold]"] = median_ms(
                            reps, lambda: db.search_hits(query, B62, 3, 1, mode, "sw", min_score=raw))
                else:
                    def route():
                        dense = db.search(query, B62, 3, 1, mode, "sw")
                        keep = host.hits(dense["score"], cut)
                        return {key: dense[key][keep] for key in dense}
                    out["cases"][case] = median_ms(reps, route)
            out["cases"][f"{label} {mode:5s} plain search, nothing else"] = median_ms(reps, lambda: db.search(query, B62, 3, 1, mode, "sw"))

    n = 1_000_000
    off = np.arange(n + 1, dtype=np.int64) * 300
    res = np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=n * 300)])
    db = _capi.DeviceDatabase(res, off, 24)
    single("headline 53 x 1M x 300", db, off, ("score", "end"), (1e-3, 10.0, 1e5))

    m = 500_000
    lengths = np.clip(np.exp(rng.normal(math.log(300), 0.5, size=m)), 30, 3000).astype(np.int64)
    off2 = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lengths, out=off2[1:])
    log_normal = _capi.DeviceDatabase(np.ascontiguousarray(_data.AA20_CODES[rng.integers(0, 20, size=int(off2[-1]))]), off2, 24)
    single("log-normal 53 x 500k", log_normal, off2, ("score",))
    log_normal.close()

    if batch_1m:
        short = [_data.encode("".join(rng.choice(LETTERS, size=int(L)))) for L in rng.integers(20, 65, size=256)]
        host = HostFit(np.diff(off))
        if new:
            got = db.search_batch_significant(short, B62, 3, 1, "score", "sw", max_evalue=10.0)
            case = f"256 q (20-64 aa) x 1M x 300 score E <= 10 ({int(got['offsets'][-1]) / 256:.1f} hits per query)"
            out["cases"][case] = median_ms(3, lambda: db.search_batch_significant(short, B62, 3, 1, "score", "sw", max_evalue=10.0))
        else:
            def route():
                dense = db.search_batch(short, B62, 3, 1, "score", "sw")["score"]
                return [host.hits(row, 10.0) for row in dense]
            total = sum(len(k) for k in route())
            case = f"256 q (20-64 aa) x 1M x 300 score E <= 10 ({total / 256:.1f} hits per query)"
            out["cases"][case] = median_ms(3, route)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=2, help="processes per build, alternating")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-1m-batch", action="store_true")
    ap.add_argument("--child", choices=["new", "parent"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "significant_quick.txt"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args.child, args.tree, args.reps, not args.no_1m_batch)), flush=True)
        return
    if not args.parent:
        ap.error("--parent DIR is required")
    runs = {"new": [], "parent": []}
    for _ in range(args.rounds):
        for which, tree in (("new", ROOT), ("parent", os.path.abspath(args.parent))):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--tree", tree, "--reps", str(args.reps)]
            cmd += ["--no-1m-batch"] if args.no_1m_batch else []
            env = {k: v for k, v in os.environ.items() if k != "MIOPAL_LIBRARY"}
            done = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree, timeout=900)
            if done.returncode != 0:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                sys.exit(f"the {which} process failed with {done.returncode}")
            line = [x for x in done.stdout.splitlines() if x.startswith("RESULT ")][-1]
            runs[which].append(json.loads(line[len("RESULT "):]))
            print(f"{which}: done", flush=True)
    lines = [f"tools/quick_significant.py: {args.rounds} processes per build, alternating; per process a warm-up and the "
             f"median of {args.reps} calls (3 for 256 x 1M); below: the median over the processes, ms",
             f"this build {runs['new'][0]['library']} (significance searches)   parent {runs['parent'][0]['library']} "
             f"(plain search, the dense row downloaded, fit and filter in numpy)", ""]
    for which in ("new", "parent"):
        lines.append("this build:" if which == "new" else "parent:")
        for case in runs[which][0]["cases"]:
            values = sorted(r["cases"][case] for r in runs[which])
            lines.append(f"  {case:86s} {values[len(values) // 2]:9.3f}   (processes: {', '.join(f'{v:.3f}' for v in values)})")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
