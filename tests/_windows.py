"""A model of the windowed views of long targets, and the databases of the window tests
(tests/test_windows_cpu.py holds them to their purpose with the checker alone, tests/test_gpu_windows.py runs them).

Smith-Waterman and HW searches cut a target of more than stride + overlap residues into windows
[x stride, x stride + stride + overlap) (pyopal_amd/csrc/host_view.inc, buildView) and merge the windows' results on
the device: the highest score, then the smallest column, then the smallest row (pack.hip, scatter_keyed_kernel).
Plain Python and numpy; nothing here touches a GPU, and every database is a function of its arguments and a seed."""
import numpy as np

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
DNA4 = np.where(np.eye(4, dtype=bool), 5, -4).astype(np.int32).ravel()   # 4 letters, match +5 / mismatch -4


def segment_stride(overlap):
    """the shortest stride of an overlap (host_view.inc, segmentStride)"""
    return max(256, (overlap * 3 // 5 + 63) // 64 * 64)


def windows(L, overlap, stride):
    """-> [(first column, length)] of a target of L residues (windowsOf and the s0 / len loop of buildView)"""
    window = stride + overlap
    if L <= window:
        return [(0, L)]
    w = 1 + (L - overlap - 1) // stride
    return [(x * stride, min(window, L - x * stride)) for x in range(w)]


def entries(lengths, overlap, stride):
    """the number of entries of the view of targets of these lengths"""
    return sum(len(windows(int(L), overlap, stride)) for L in lengths)


def merged(results):
    """results: (first column, score, end_t, end_q) of each window of one target, end_t inside the window (-1, -1:
    no cell, a Smith-Waterman score of 0 or an empty target) -> (score, end_t, end_q) of the target: the maximum
    score, then the smallest column first + end_t, then the smallest row."""
    best = None
    for first, score, end_t, end_q in results:
        cell = (int(score), -(first + int(end_t)), -int(end_q)) if end_t >= 0 else (int(score), 1, 1)
        if best is None or cell > best:
            best = cell
    return (best[0], -best[1], -best[2])


def window_results(query, seqs, matrix, gaps, algorithm, overlap, stride):
    """the checker on every window of every target, as a target of its own
    -> per target [(first column, score, end_t, end_q)]"""
    cuts = [windows(len(s), overlap, stride) for s in seqs]
    res, off = _oracle.flatten([s[a:a + n] for s, cut in zip(seqs, cuts) for a, n in cut])
    r = _oracle.search(query, res, off, matrix, gaps[0], gaps[1], "end", algorithm)
    out, at = [], 0
    for cut in cuts:
        out.append([(a, int(r["score"][at + x]), int(r["end_t"][at + x]), int(r["end_q"][at + x]))
                    for x, (a, _) in enumerate(cut)])
        at += len(cut)
    return out


def cross_window_ties(per_target):
    """targets (indices into window_results' list) with two windows whose own first maxima tie at the target's
    optimum in different cells: only the merge's order decides which of them is reported"""
    out = []
    for k, rows in enumerate(per_target):
        top = max(r[1] for r in rows)
        cells = {(r[0] + r[2], r[3]) for r in rows if r[1] == top and r[2] >= 0}
        if len(cells) >= 2:
            out.append(k)
    return out


# ---- the tie databases --------------------------------------------------------------------------------------------
# (seeds chosen so that each holds the cross-window ties test_windows_cpu.py asks for, under Smith-Waterman and HW)
TIE_KINDS = {"dna4": dict(seed=41, alphabet=4, qlen=12, matrix=DNA4),
             "protein24": dict(seed=42, alphabet=24, qlen=8, matrix=B62)}
TIE_GAPS = (3, 1)
TIE_PLAN = (128, 256)   # the (overlap, stride) planWindows chooses for both: what the CPU tier cuts them by


def _letters(rng, alphabet, n):
    return rng.integers(0, 4, size=n).astype(np.uint8) if alphabet == 4 else _data.random_protein(rng, n)


def tie_db(kind, window=384):
    """-> (query, list of targets, matrix, alphabet length, indices of the constructed targets and their first
    copy's end column). 200 random targets of 1500 .. 2000 residues, then targets with the exact query twice and
    three times, the copies more than `window` columns apart: no window holds two of them."""
    k = TIE_KINDS[kind]
    rng = np.random.default_rng(k["seed"])
    q = _letters(rng, k["alphabet"], k["qlen"])
    seqs = [_letters(rng, k["alphabet"], int(n)) for n in rng.integers(1500, 2001, size=200)]
    built = {}
    for copies in (2, 3, 2, 3):
        first = int(rng.integers(5, 200))
        step = window + len(q) + int(rng.integers(1, 300))
        t = _letters(rng, k["alphabet"], first + copies * step + int(rng.integers(0, 400)))
        for c in range(copies):
            t[first + c * step:first + c * step + len(q)] = q
        built[len(seqs)] = first + len(q) - 1
        seqs.append(t)
    return q, seqs, k["matrix"], k["alphabet"], built


# ---- the length transitions (a) -----------------------------------------------------------------------------------
def transition_lengths(overlap, stride):
    """every length at which windowsOf or the last window's length changes, then the degenerate ones"""
    W = stride + overlap
    return [W - 1, W, W + 1, stride + overlap + stride // 2, 2 * stride + overlap, 2 * stride + overlap + 1,
            3 * stride + overlap, 3 * stride + overlap + 1, 0, 1, 2, overlap + 1]


def transition_db(seed, q, overlap, stride, fillers=150):
    """-> (targets, number of listed ones). The listed lengths twice - a mutated copy of the query ending on the
    target's last column, then one starting at column 0 (cut to the target where it is shorter) - and short fillers."""
    rng = np.random.default_rng(seed)
    seqs = []
    for at_end in (True, False):
        for L in transition_lengths(overlap, stride):
            t = _data.random_protein(rng, L)
            copy = _data.mutate(rng, q, 0.15)
            m = min(len(copy), L)
            if at_end:
                t[L - m:] = copy[len(copy) - m:]
            else:
                t[:m] = copy[:m]
            seqs.append(t)
    listed = len(seqs)
    seqs += [_data.random_protein(rng, int(n)) for n in rng.integers(20, 400, size=fillers)]
    return seqs, listed


# ---- the seam sweep (b) -------------------------------------------------------------------------------------------
def seam_aims(overlap, stride, span):
    """-> [(offset of the planted alignment, column it is aimed at)]: its last column over the last columns of
    windows 0 and 1 (k stride + overlap - 1) +- 3, its first column over the first columns of windows 1 and 2
    (k stride) +- 3, and its last column over those"""
    out = []
    for k in (1, 2):
        out += [(e - span + 1, e) for e in range(k * stride + overlap - 3, k * stride + overlap + 3)]
        out += [(s, s) for s in range(k * stride - 3, k * stride + 3)]
        out += [(e - span + 1, e) for e in range(k * stride - 3, k * stride + 3)]
    return out


def planted(first, second, filler, g):
    """the two halves of the query's best partners with g unrelated residues between them"""
    return np.concatenate([first, filler[:g], second]).astype(np.uint8)


def seam_db(seed, first, second, g, overlap, stride, letters=None):
    """-> (targets, aims): one target of 3 stride + overlap / 2 residues per aim of seam_aims, the planted alignment
    at that offset. `letters`: the background's generator (rng, n), default random protein."""
    rng = np.random.default_rng(seed)
    letters = letters or _data.random_protein
    filler = letters(rng, 512)
    piece = planted(first, second, filler, g)
    aims = seam_aims(overlap, stride, len(piece))
    seqs = []
    for at, _ in aims:
        t = letters(rng, 3 * stride + overlap // 2)
        t[at:at + len(piece)] = piece
        seqs.append(t)
    return seqs, aims


def widest_join(seed, q, matrix, gaps, limit=200):
    """the largest g for which the checker still joins the two halves of q across g unrelated residues: its
    Smith-Waterman alignment of a lone target takes the whole query and spans len(q) + g columns. (The joined
    alignment scores both halves minus the gap, either half alone scores itself: the halves are joined while the gap
    costs less than the weaker half, so no optimal alignment of q spans more than len(q) + that g.)"""
    rng = np.random.default_rng(seed)
    filler = _data.random_protein(rng, 512)   # (seam_db's filler under the same seed)
    half = len(q) // 2
    seqs = []
    for g in range(limit):
        pad = np.full(8, _data.encode("P")[0], dtype=np.uint8)
        seqs.append(np.concatenate([pad, planted(q[:half], q[half:], filler, g), pad]))
    res, off = _oracle.flatten(seqs)
    r = _oracle.search(q, res, off, matrix, gaps[0], gaps[1], "full", "sw")
    joined = [g for g in range(limit) if r["start_q"][g] == 0 and r["end_q"][g] == len(q) - 1
              and r["end_t"][g] - r["start_t"][g] + 1 == len(q) + g]
    return max(joined)


def covers(ref, aims):
    """which of the checker's `full` alignments cover the column their target was aimed at"""
    cols = np.array([c for _, c in aims])
    return (ref["start_t"] <= cols) & (cols <= ref["end_t"])
