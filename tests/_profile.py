"""The numpy reference of the profile-column tests (tests/test_profile_cpu.py, tests/test_gpu_profile_columns.py,
tests/test_gpu_profile.py): the definition of include/miopal.h (miopalProfileColumns) written out in integers - Python
ints and numpy.uint64, no floats."""
import numpy as np

UNCOVERED = 255
ONE = 1 << 32   # MIOPAL_PROFILE_WEIGHT_ONE


def project(ops, start_q, start_t, target, Q, A):
    """A member's row: `ops` (0 match, 1 deletion, 2 insertion, 3 mismatch) walked from (start_q, start_t) over the
    residues `target`; uint8[Q], 255 where the alignment does not cover the query."""
    row = np.full(Q, UNCOVERED, dtype=np.uint8)
    i, t = int(start_q), int(start_t)
    for op in np.asarray(ops).tolist():
        if op == 0 or op == 3:
            row[i] = target[t]
            i += 1
            t += 1
        elif op == 1:
            row[i] = A
            i += 1
        else:
            assert op == 2, op
            t += 1
    return row


def columns(msa, A):
    """-> (counts int64[Q][A + 1], k int64[Q], terms uint64[Q][A + 1], weights int64[members], weighted int64[Q][A + 1])
    of the multiple alignment `msa` (uint8[members][Q]; entries < A, == A or 255)."""
    msa = np.asarray(msa, dtype=np.uint8)
    members, Q = msa.shape
    counts = np.zeros((Q, A + 1), dtype=np.int64)
    for a in range(A + 1):
        counts[:, a] = np.count_nonzero(msa == a, axis=0)
    k = np.count_nonzero(counts[:, :A] > 0, axis=1).astype(np.int64)
    terms = np.zeros((Q, A + 1), dtype=np.uint64)
    held = counts[:, :A] > 0
    divisor = (k[:, None] * counts[:, :A]).astype(np.uint64)
    terms[:, :A][held] = np.uint64(ONE) // divisor[held]
    # a member's letters pick their terms; the gap and 255 pick the zero column A
    pick = np.where(msa < A, msa, A).astype(np.int64)
    per_entry = terms[np.arange(Q)[None, :], pick]
    weights = per_entry.sum(axis=1, dtype=np.uint64).astype(np.int64)
    weighted = np.zeros((Q, A + 1), dtype=np.int64)
    for a in range(A + 1):
        weighted[:, a] = ((msa == a) * weights[:, None].astype(np.uint64)).sum(axis=0, dtype=np.uint64).astype(np.int64)
    return counts, k, terms, weights, weighted


def columns_plain(msa, A):
    """`columns` once more with Python integers, entry by entry (small inputs: the reference's own witness)."""
    msa = np.asarray(msa)
    members, Q = msa.shape
    counts = [[0] * (A + 1) for _ in range(Q)]
    for s in range(members):
        for i in range(Q):
            if msa[s, i] <= A:
                counts[i][int(msa[s, i])] += 1
    k = [sum(1 for a in range(A) if counts[i][a] > 0) for i in range(Q)]
    terms = [[(ONE // (k[i] * counts[i][a])) if a < A and counts[i][a] > 0 else 0 for a in range(A + 1)] for i in range(Q)]
    weights = [sum(terms[i][int(msa[s, i])] for i in range(Q) if msa[s, i] < A) for s in range(members)]
    weighted = [[sum(weights[s] for s in range(members) if msa[s, i] == a) for a in range(A + 1)] for i in range(Q)]
    return (np.array(counts, dtype=np.int64).reshape(Q, A + 1), np.array(k, dtype=np.int64),
            np.array(terms, dtype=np.uint64).reshape(Q, A + 1), np.array(weights, dtype=np.int64),
            np.array(weighted, dtype=np.int64).reshape(Q, A + 1))
