"""The witness of the occurrence tests (tests/test_occurrences_cpu.py pins it on hand-worked rows; the GPU tests hold
the device picker and the search to it): the rule of include/miopal.h, miopalSearchOccurrences, restated in Python,
and the recurrence behind the values it picks from, written out twice - column by column for many short targets
(`column_values`) and row by row for one long target (`row_values`), each held to the other and to the C checker."""
import numpy as np

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


def pick(values, min_score, window, rows=None):
    """Greedy peak picking with a suppression window over one target's column values -> [(column, value, row)];
    ``rows``: the row reported with each column (None: -1)."""
    out, cand = [], None
    for j, v in enumerate(np.asarray(values).tolist()):
        if cand is not None and j - cand[0] > window:
            out.append(cand)
            cand = None
        if v >= min_score and (cand is None or v > cand[1]):
            cand = (j, v, -1 if rows is None else int(rows[j]))
    if cand is not None:
        out.append(cand)
    return out


def pick_rows(value, lengths, min_score, window, value_row=None):
    """`pick` over the rows of a (rows, stride) array, as `_capi.pick_occurrences_rows` answers: a dict of "offsets",
    "column", "score" and "row"."""
    value = np.atleast_2d(value)
    lengths = np.broadcast_to(np.asarray(lengths), (len(value),))
    offsets, found = [0], []
    for r in range(len(value)):
        found += pick(value[r, :lengths[r]], min_score, window, None if value_row is None else np.atleast_2d(value_row)[r])
        offsets.append(len(found))
    table = np.array(found, dtype=np.int64).reshape(-1, 3)
    return {"offsets": np.array(offsets, dtype=np.int64), "column": table[:, 0].astype(np.int32),
            "score": table[:, 1].astype(np.int32), "row": table[:, 2].astype(np.int32)}


# ---- the recurrence, one numpy lane per target ----------------------------------------------------------------------

def column_values(rows, targets, gap_open, gap_extend, algorithm, neg=-(10 ** 9)):
    """-> (v, r), both [targets][longest]: column j of target k holds, for "hw", H[Q - 1][j] under HW's borders (the top
    row free, the left column one gap of i + 1 residues or i + 1 openings, whichever is cheaper) and r = Q - 1; for
    "sw" the column's maximum with the floor at 0 and the smallest row that reaches it. rows[i][t]: the score of query
    position i against residue t. Columns behind a target hold nothing meaningful. ``neg``: the witness's minus
    infinity, below every true value of the scoring model (test_gpu_int32_edges.py passes -2^60)."""
    rows = np.asarray(rows, dtype=np.int64)
    hw, Q, n = algorithm == "hw", len(rows), len(targets)
    longest = max(max((len(t) for t in targets), default=0), 1)
    T = np.zeros((n, longest), dtype=np.int64)
    for k, t in enumerate(targets):
        T[k, :len(t)] = t
    NEG = neg
    left = [-min(gap_open + i * gap_extend, (i + 1) * gap_open) if hw else 0 for i in range(Q)]
    Hprev = np.repeat(np.array(left, dtype=np.int64)[:, None], n, axis=1)   # column -1
    Eprev = np.full((Q, n), NEG, dtype=np.int64)
    V = np.zeros((n, longest), dtype=np.int64)
    R = np.zeros((n, longest), dtype=np.int64)
    for j in range(longest):
        s = rows[:, T[:, j]]
        E = np.maximum(Hprev - gap_open, Eprev - gap_extend)
        H = np.empty((Q, n), dtype=np.int64)
        up_h, up_f, diag = np.zeros(n, dtype=np.int64), np.full(n, NEG), np.zeros(n, dtype=np.int64)   # the free top row
        for i in range(Q):
            f = np.maximum(up_h - gap_open, up_f - gap_extend)
            h = np.maximum(np.maximum(diag + s[i], E[i]), f)
            if not hw:
                h = np.maximum(h, 0)
            diag, H[i], up_h, up_f = Hprev[i], h, h, f
        if hw:
            V[:, j], R[:, j] = H[Q - 1], Q - 1
        else:
            V[:, j], R[:, j] = H.max(axis=0), H.argmax(axis=0)   # (argmax: the first, the smallest row)
        Hprev, Eprev = H, E
    return V, R


# ---- the same recurrence row by row, for one long target -------------------------------------------------------------

def row_values(rows, target, gap_open, gap_extend, algorithm, tied=None):
    """`column_values` for ONE target, iterated over the Q rows and vectorised over the columns: what a target of tens of
    thousands of residues needs. -> (v[L], r[L]). Valid for open >= extend only. Per row i, from H and F of the row
    above: F = max(Hup - open, Fup - ext); base = max(diagonal + score, F), floored at 0 for "sw"; the gap along the
    row is E[j] = max over k < j of (base[k] + k * ext) - open - (j - 1) * ext, the border cell entering as k = -1; and
    H = max(base, E). `base` stands in for H under the running maximum because a gap opened from a cell that is itself
    the end of such a gap never beats that gap extended - the step that needs open >= extend. "hw" keeps the last row;
    "sw" keeps a running column maximum and the smallest row that reaches it, never the Q x L matrix.
    ``tied``: a bool array of L entries, set where a column's maximum ("sw") is reached again in a later strip of 64
    rows than the one of its smallest row - the columns at which a device sweep has a tie to break between strips."""
    assert gap_open >= gap_extend >= 0 and algorithm in ("hw", "sw")
    rows = np.asarray(rows, dtype=np.int64)
    target = np.asarray(target, dtype=np.int64)
    hw, Q, L = algorithm == "hw", len(rows), len(target)
    NEG = -(10 ** 15)
    left = [-min(gap_open + i * gap_extend, (i + 1) * gap_open) if hw else 0 for i in range(Q)]
    j = np.arange(L, dtype=np.int64)
    Hup, Fup = np.zeros(L, dtype=np.int64), np.full(L, NEG, dtype=np.int64)   # the free top row
    v = np.full(L, NEG, dtype=np.int64)
    r = np.full(L, Q - 1 if hw else -1, dtype=np.int64)
    if tied is not None:
        tied[:] = False
    for i in range(Q):
        F = np.maximum(Hup - gap_open, Fup - gap_extend)
        diag = np.concatenate([[left[i - 1] if i > 0 else 0], Hup[:-1]]) if L else Hup
        base = np.maximum(diag + rows[i][target], F)
        if not hw:
            base = np.maximum(base, 0)
        ahead = np.concatenate([[left[i] - gap_extend], (base + j * gap_extend)[:-1]]) if L else base
        E = np.maximum.accumulate(ahead) - gap_open - (j - 1) * gap_extend
        H = np.maximum(base, E)
        if not hw:
            take = H > v
            if tied is not None:
                tied[take] = False
                tied[(H == v) & (i // 64 > r // 64)] = True
            v, r = np.where(take, H, v), np.where(take, i, r)
        Hup, Fup = H, F
    return (Hup if hw else v), r


def flat_columns(values, rows):
    """per-target (v, r) pairs -> every column of every target in one row: (V, R, offsets), int64 throughout"""
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in values])]).astype(np.int64)
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.int64) for p in parts]) if len(parts) else np.zeros(0, dtype=np.int64)   # noqa: E731
    return cat(values), cat(rows), offsets


def expected_flat(V, R, offsets, min_score, window, first=0, last=None):
    """the four arrays of an answer from `flat_columns`' row, for the targets [first, last) of it. window 0 keeps every
    column at or above the cut, which is all that `pick` does then (tests/test_occurrences_cpu.py pins it) and is taken
    in one numpy expression; any other window goes through `pick`."""
    last = len(offsets) - 1 if last is None else last
    lo, hi = offsets[first], offsets[last]
    if window == 0:
        at = lo + np.flatnonzero(V[lo:hi] >= min_score)
        target = np.searchsorted(offsets, at, side="right") - 1   # (the last target that begins at or before: the non-empty one)
        table = np.stack([target, V[at], at - offsets[target], R[at]], axis=1).astype(np.int64)
    else:
        out = [(k, v, j, r) for k in range(first, last)
               for j, v, r in pick(V[offsets[k]:offsets[k + 1]], min_score, window, R[offsets[k]:offsets[k + 1]])]
        table = np.array(out, dtype=np.int64).reshape(-1, 4)
    return {"target": table[:, 0], "score": table[:, 1].astype(np.int32), "end_t": table[:, 2].astype(np.int32),
            "end_q": table[:, 3].astype(np.int32)}
