"""Aligner.profile_columns (alignments projected, counted and weighted on the device) against the route a caller had
before it: align_pairs(mode="full"), the operations over PCIe, projection and counting in numpy on the host. One
process, the routes alternating; per route a warm-up call, then the median and min .. max of --reps calls (wall clock
around calls that return host arrays). 10 000 members drawn from a database of 300-residue targets, a 300-residue
query, Smith-Waterman, BLOSUM62, 11/1; two databases: random targets (the headline's shape: short local alignments) and
a family of mutated copies of the query (alignments that span it - what the hits of a search look like).
The host route comes in two forms: Aligner.align_pairs (result objects, alignment strings) and
DeviceDatabase.align_pairs (flat arrays), each followed by the same vectorised numpy projection and the integer
reference's arithmetic. The first answers of the three routes are compared bit for bit.
--trace: the device route only, a few calls, for a kernel trace of its own.
Usage: python tools/quick_profile_columns.py [--reps N] [--targets N] [--members N] [--output FILE] [--trace]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
A = 24
ONE = 1 << 32


def host_columns(msa):
    """tests/_profile.py's arithmetic (uint64, no floats) on a finished multiple alignment"""
    members, Q = msa.shape
    counts = np.stack([np.count_nonzero(msa == a, axis=0) for a in range(A + 1)], axis=1).astype(np.int64)
    k = np.count_nonzero(counts[:, :A] > 0, axis=1).astype(np.int64)
    terms = np.zeros((Q, A + 1), dtype=np.uint64)
    held = counts[:, :A] > 0
    terms[:, :A][held] = np.uint64(ONE) // (k[:, None] * counts[:, :A]).astype(np.uint64)[held]
    weights = terms[np.arange(Q)[None, :], np.where(msa < A, msa, A)].sum(axis=1, dtype=np.uint64)
    weighted = np.stack([((msa == a) * weights[:, None]).sum(axis=0, dtype=np.uint64) for a in range(A + 1)], axis=1)
    return counts, weighted.astype(np.int64), weights.astype(np.int64)


def host_project(query, flat, ops_off, start_q, start_t, residues, offsets, targets):
    """every alignment of a pair list at once: the row and the target residue of each operation from running sums"""
    n = len(targets)
    msa = np.full((n + 1, len(query)), 255, dtype=np.uint8)
    msa[0] = query
    lens = np.diff(ops_off)
    owner = np.repeat(np.arange(n), lens)
    on_q, on_t = flat != 2, flat != 1
    before_q = np.cumsum(on_q) - on_q
    before_t = np.cumsum(on_t) - on_t
    first = np.minimum(ops_off[:-1], max(len(flat) - 1, 0))
    row = start_q[owner] + before_q - before_q[first][owner]
    col = offsets[targets][owner] + start_t[owner] + before_t - before_t[first][owner]
    both = on_q & on_t
    msa[1 + owner[both], row[both]] = residues[col[both]]
    gap = on_q & ~on_t
    msa[1 + owner[gap], row[gap]] = A
    return msa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--targets", type=int, default=20_000)
    ap.add_argument("--members", type=int, default=10_000)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "profile_columns.txt"))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()

    import _data
    import pyopal_amd
    from pyopal_amd import _capi
    if _capi.lib().miopalDeviceCount() < 1:
        sys.exit("no gfx950 device visible: nothing is measured without one")
    rng = np.random.default_rng(2027)
    letters = np.frombuffer(_data.NCBI.encode(), dtype=np.uint8)
    query = _data.random_protein(rng, 300)
    aligner = pyopal_amd.Aligner("BLOSUM62", gap_open=11, gap_extend=1)
    ops_table = np.zeros(256, dtype=np.uint8)
    for code, letter in enumerate(b"MDIX"):
        ops_table[letter] = code

    def family():
        seqs = []
        for _ in range(args.targets):
            s = _data.mutate(rng, query, rate=0.3)
            seqs.append(np.resize(s, 300) if len(s) >= 300 else np.concatenate([s, _data.random_protein(rng, 300 - len(s))]))
        return seqs

    lines = [f"tools/quick_profile_columns.py: {args.members} members drawn from {args.targets} targets of 300 residues, "
             f"query of 300, SW, BLOSUM62, 11/1; a warm-up and {args.reps} calls per route, alternating; "
             f"median (min .. max), ms, wall clock", ""]
    for label, seqs in (("random targets", [_data.random_protein(rng, 300) for _ in range(args.targets)]),
                        ("family of the query", family())):
        database = pyopal_amd.Database([letters[s].tobytes().decode() for s in seqs])
        residues = np.concatenate(seqs)
        offsets = np.arange(args.targets + 1, dtype=np.int64) * 300
        targets = rng.choice(args.targets, size=args.members, replace=False).astype(np.int64)
        q = letters[query].tobytes().decode()
        pairs = np.stack([np.zeros(args.members, dtype=np.int64), targets], axis=1)
        mirror = database._device_mirror(0)
        B62 = np.frombuffer(aligner._int_matrix, dtype=np.int32)

        def device():
            c = aligner.profile_columns(q, database, targets)
            return c.counts, c.weighted, c.member_weights

        def objects():
            results = aligner.align_pairs([q], database, pairs, mode="full")
            flat = ops_table[np.frombuffer("".join(r.alignment for r in results).encode("ascii"), dtype=np.uint8)]
            off = np.concatenate([[0], np.cumsum([len(r.alignment) for r in results])]).astype(np.int64)
            sq = np.array([r.query_start for r in results], dtype=np.int64)
            st = np.array([r.target_start for r in results], dtype=np.int64)
            return host_columns(host_project(query, flat, off, sq, st, residues, offsets, targets))

        def arrays():
            out = mirror.align_pairs([query], pairs[:, 0], targets, B62, 11, 1, "full", "sw")
            return host_columns(host_project(query, out["aln_flat"], out["aln_off"], out["start_q"].astype(np.int64),
                                             out["start_t"].astype(np.int64), residues, offsets, targets))

        if args.trace:
            for _ in range(3):
                device()
            continue
        routes = (("device: Aligner.profile_columns", device), ("host: Aligner.align_pairs + numpy", objects),
                  ("host: DeviceDatabase.align_pairs + numpy", arrays))
        first = [call() for _, call in routes]   # (the warm-up of every route, and the check)
        for other in first[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(first[0], other)), label
        ops = int(mirror.align_pairs([query], pairs[:, 0], targets, B62, 11, 1, "full", "sw")["aln_off"][-1])
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, call in routes:
                t = time.perf_counter()
                call()
                times[name].append((time.perf_counter() - t) * 1e3)
        lines.append(f"{label}: {ops} operations in the {args.members} alignments ({ops / args.members:.1f} per member); "
                     f"the three routes agree bit for bit")
        for name, _ in routes:
            v = sorted(times[name])
            lines.append(f"    {name:44s} {v[len(v) // 2]:9.2f} ({v[0]:8.2f} .. {v[-1]:8.2f})")
        lines.append("")
    if args.trace:
        return
    text = "\n".join(lines)
    print(text)
    with open(args.output, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
