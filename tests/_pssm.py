"""Inputs and witnesses of the PSSM tests (tests/test_pssm_cpu.py, tests/test_gpu_pssm.py).

The CPU checker takes (query, matrix), not a PSSM, and the tests rest on one identity: a PSSM whose rows are drawn
from at most A distinct row vectors IS an ordinary search over an A-letter alphabet - query[i] = the class of row
i, matrix[c] = class c's row (asymmetric: the checker does not care), consensus[i] = query[i]. The library is
handed the Q x A rows and cannot know that they repeat; classes come in random order, so a row addressed by the
wrong position gives a wrong score."""
import numpy as np

A32 = 32


def class_pssm(rng, length, alphabet=A32, low=-8, high=12, values=None):
    """-> (classes uint8[length], matrix int32[alphabet * alphabet], rows int32[length, alphabet]).
    `values`: the entries are drawn from this short list instead of [low, high] (ties-rich rows)."""
    if values is not None:
        table = rng.choice(np.asarray(values, dtype=np.int32), size=(alphabet, alphabet)).astype(np.int32)
    else:
        table = rng.integers(low, high + 1, size=(alphabet, alphabet)).astype(np.int32)
    classes = rng.integers(0, alphabet, size=length).astype(np.uint8)
    return classes, np.ascontiguousarray(table.ravel()), np.ascontiguousarray(table[classes])


def random_db(rng, lengths, alphabet=A32):
    """-> (residues uint8 over the whole alphabet, offsets int64)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return rng.integers(0, alphabet, size=int(off[-1])).astype(np.uint8), off


def db_lengths(rng, count=700, longest=180):
    """~count lengths in 0 .. longest: zero-length targets among them, every length near a strip edge at least once"""
    lengths = rng.integers(0, longest + 1, size=count)
    lengths[[3, 77, count - 1]] = 0
    lengths[[5, 6, 7, 8]] = [1, 63, 64, 65]
    lengths[11] = longest
    return lengths


def with_repeat(residues, offsets, k=20):
    """the database with target k appended once more (a repeated target: equal results at two indices)"""
    piece = residues[offsets[k]:offsets[k + 1]]
    return np.concatenate([residues, piece]), np.concatenate([offsets, [offsets[-1] + len(piece)]])


def assert_same(got, want, context):
    """every array of `want` (a tests/_oracle.search dict) equals got's, alignments operation by operation"""
    for key in want:
        if key == "aln":
            assert len(got[key]) == len(want[key]), (context, key)
            for k, (a, b) in enumerate(zip(got[key], want[key])):
                assert np.array_equal(a, b), (context, key, k, a.tolist(), b.tolist())
        else:
            assert np.array_equal(got[key], want[key]), (context, key, np.flatnonzero(got[key] != want[key])[:8])


def dp_scores(rows, targets, gap_open, gap_extend, algorithm):
    """Second witness, scores only, "sw" and "nw": the affine-gap recurrence written out, one numpy lane per target.
    rows[i][t] = score of position i against residue t; a gap of k residues costs open + (k - 1) * extend, or k
    openings where that is cheaper (the checker's borders)."""
    rows = np.asarray(rows, dtype=np.int64)
    nw, Q, n = algorithm == "nw", len(rows), len(targets)
    lens = np.array([len(t) for t in targets], dtype=np.int64)
    T = np.zeros((n, max(int(lens.max()), 1)), dtype=np.int64)
    for k, t in enumerate(targets):
        T[k, :len(t)] = t
    NEG = -(10 ** 9)
    border = (lambda k: -min(gap_open + k * gap_extend, (k + 1) * gap_open) if k >= 0 else 0) if nw else (lambda k: 0)
    Hprev = np.repeat(np.array([border(i) for i in range(Q)], dtype=np.int64)[:, None], n, axis=1)   # column -1
    Eprev = np.full((Q, n), NEG, dtype=np.int64)
    best = np.full(n, border(Q - 1) if nw else 0, dtype=np.int64)   # (an empty target: the left border's last cell)
    for j in range(int(lens.max())):
        s = rows[:, T[:, j]]
        E = np.maximum(Hprev - gap_open, Eprev - gap_extend)
        H = np.empty((Q, n), dtype=np.int64)
        up_h, up_f, diag = np.full(n, border(j)), np.full(n, NEG), np.full(n, border(j - 1))
        for i in range(Q):
            f = np.maximum(up_h - gap_open, up_f - gap_extend)
            h = np.maximum(np.maximum(diag + s[i], E[i]), f)
            if not nw:
                h = np.maximum(h, 0)
            diag, H[i], up_h, up_f = Hprev[i], h, h, f
        if nw:
            best = np.where(lens - 1 == j, H[Q - 1], best)
        else:
            best = np.where(j < lens, np.maximum(best, H.max(axis=0)), best)
        Hprev, Eprev = H, E
    return best.astype(np.int32)
