"""The witness of the aligned occurrence search (miopalSearchOccurrencesAligned): where an occurrence starts, stated as
the reversed pass of oracle/opal_oracle.c's head applied to the occurrence's end cell, and its operations, taken from
the CPU checker on the rectangle between start and end. tests/test_occurrence_alignments_cpu.py pins `starts` against
the C checker and on hand-worked cases.

The start rule for the occurrence (v, r, j) of a target t under a query of rows q:
  - the reversed prefixes q[r], q[r - 1] .. q[0] and t[j], t[j - 1] .. t[0] under NW borders (both penalised with
    the border gap);
  - the region is the last row (all of q consumed) for "hw" and all cells for "sw";
  - candidates are scanned column by column, row by row inside a column, and a candidate replaces the best only when
    strictly greater: the first cell that holds the maximum;
  - the cell (a, b) gives startQuery = r - a, startTarget = j - b;
  - the degenerate optimum of "hw": when the maximum is not v and v is the border gap over q[0 .. r], the target span
    is empty - startQuery = 0, startTarget = j + 1.
The recurrence is written one numpy lane per occurrence and one vector of rows per lane. The gap consuming the query
inside a column (F) comes in two forms: the running maximum that it is when opening costs at least extending, and
the checker's own statement, row by row, for any non-negative gap costs; `starts` takes the first where it is valid
and the second elsewhere, and tests/test_cases_cpu.py holds the two to each other and both to the C checker.
"""
import numpy as np

import _oracle

NEG = -(10 ** 12)
DEL = 1   # OPAL_ALIGN_DEL: a query residue against a gap


def border(k, gap_open, gap_extend):
    """the border cell k residues into a border gap (oracle/opal_oracle.c, border())"""
    return -min(gap_open + k * gap_extend, (k + 1) * gap_open)


def column_running(h0, top, gap_open, gap_extend):
    """H of one column from h0 = max(diagonal, E) ([lanes][rows]) and the border cell above it. Valid for
    open >= extend only: F[a] = max over the rows above, the border row included, of H - open - (rows between) x ext,
    where h0 stands in for H because a gap opened from a cell that is itself the end of such a gap never beats that gap
    extended."""
    step = (np.arange(h0.shape[1]) - 1) * gap_extend
    above = np.concatenate([np.full((len(h0), 1), top, dtype=np.int64), h0[:, :-1]], axis=1) + step[None, :]
    F = np.maximum.accumulate(above, axis=1) - gap_open - step[None, :]
    return np.maximum(h0, F)


def column_by_rows(h0, top, gap_open, gap_extend):
    """the same column as oracle/opal_oracle.c's dp_pass states it, for any gap costs:
    F[a] = max(F[a - 1] - ext, H[a - 1] - open), H[a] = max(h0[a], F[a]), the border cell above row 0"""
    H = np.empty_like(h0.T)
    f, up = np.full(len(h0), NEG, dtype=np.int64), np.full(len(h0), top, dtype=np.int64)
    for a, h in enumerate(np.ascontiguousarray(h0.T)):
        f = np.maximum(f - gap_extend, up - gap_open)
        up = H[a] = np.maximum(h, f)
    return H.T


def starts(rows, targets, occurrences, gap_open, gap_extend, algorithm, by_rows=None):
    """rows[i][t]: the score of query position i against residue t ([Q][A]); targets: a list of uint8 arrays;
    occurrences: (target, score, end_t, end_q) per occurrence. -> (start_t, start_q) int32 arrays. Raises when an
    occurrence's score is neither the reversed maximum nor ("hw") the border gap: such a cell is no occurrence.
    Any non-negative gap costs; ``by_rows``: the form of F (None: the running maximum where open >= extend)."""
    assert gap_open >= 0 and gap_extend >= 0 and algorithm in ("hw", "sw")
    by_rows = gap_open < gap_extend if by_rows is None else by_rows
    assert by_rows or gap_open >= gap_extend
    column = column_by_rows if by_rows else column_running
    rows = np.asarray(rows, dtype=np.int64)
    occ = np.asarray(occurrences, dtype=np.int64).reshape(-1, 4)
    n = len(occ)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    score, J, R = occ[:, 1], occ[:, 2], occ[:, 3]
    height, width = int(R.max()) + 1, int(J.max()) + 1
    # the reversed target of every lane, padded: column b holds t[j - b]
    T = np.zeros((n, width), dtype=np.int64)
    for k, (t, j) in enumerate(zip(occ[:, 0].tolist(), J.tolist())):
        T[k, :j + 1] = targets[t][j::-1]
    a = np.arange(height)
    row_of = np.clip(R[:, None] - a[None, :], 0, None)            # row a of lane k is query position r - a
    valid = a[None, :] <= R[:, None]
    candidate = (a[None, :] == R[:, None]) if algorithm == "hw" else valid
    left = np.array([border(i, gap_open, gap_extend) for i in range(height)], dtype=np.int64)
    Hprev = np.repeat(left[None, :], n, axis=0)                   # column -1
    Eprev = np.full((n, height), NEG, dtype=np.int64)
    best = np.full(n, NEG, dtype=np.int64)
    best_a = np.full(n, -1, dtype=np.int64)
    best_b = np.full(n, -1, dtype=np.int64)
    for b in range(width):
        s = rows[row_of, T[:, b][:, None]]
        top = border(b, gap_open, gap_extend)
        top_prev = border(b - 1, gap_open, gap_extend) if b > 0 else 0
        E = np.maximum(Eprev - gap_extend, Hprev - gap_open)
        diag = np.concatenate([np.full((n, 1), top_prev, dtype=np.int64), Hprev[:, :-1]], axis=1)
        h0 = np.maximum(diag + s, E)
        H = column(h0, top, gap_open, gap_extend)
        seen = np.where(candidate, H, NEG)
        column_best = seen.max(axis=1)
        first = seen.argmax(axis=1)
        take = (b <= J) & (column_best > best)
        best = np.where(take, column_best, best)
        best_a = np.where(take, first, best_a)
        best_b = np.where(take, b, best_b)
        Hprev, Eprev = H, E
    start_q, start_t = R - best_a, J - best_b
    for k in np.flatnonzero(best != score):
        if algorithm == "hw" and score[k] == border(int(R[k]), gap_open, gap_extend):
            start_q[k], start_t[k] = 0, J[k] + 1
        else:
            raise AssertionError(f"occurrence {k}: score {score[k]}, reversed maximum {best[k]}")
    return start_t.astype(np.int32), start_q.astype(np.int32)


def operations(query, matrix, targets, occurrences, start_t, start_q, gap_open, gap_extend):
    """the checker's global alignment of q[start_q .. end_q] with t[start_t .. end_t], one uint8 array per
    occurrence; an empty target span (the degenerate "hw" optimum) is all query-consuming gaps"""
    occ = np.asarray(occurrences, dtype=np.int64).reshape(-1, 4)
    out = [None] * len(occ)
    pieces = {}
    for k, ((t, _, j, r), st, sq) in enumerate(zip(occ.tolist(), np.asarray(start_t).tolist(), np.asarray(start_q).tolist())):
        if st > j:   # (the checker answers an empty target with no alignment at all: the gap over the query, written out)
            out[k] = np.full(r - sq + 1, DEL, dtype=np.uint8)
        else:
            pieces.setdefault((sq, r), []).append((k, targets[t][st:j + 1]))
    for (sq, r), members in pieces.items():
        residues, offsets = _oracle.flatten([piece for _, piece in members])
        got = _oracle.search(query[sq:r + 1], residues, offsets, matrix, gap_open, gap_extend, "full", "nw")
        for (k, _), ops in zip(members, got["aln"]):
            out[k] = np.asarray(ops, dtype=np.uint8)
    return out
