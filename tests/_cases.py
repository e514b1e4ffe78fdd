"""One list of scoring systems and inputs for the entry points that have a 32-bit lane kernel of their own (pair lists,
PSSMs, occurrences, aligned occurrences, the batch search, profile columns): tests/test_cases_cpu.py holds the numpy
witnesses to the C checker on every case, tests/test_gpu_cases.py holds the kernels to both.

Five axes - alphabet, gap model, matrix kind, residue span, query length - and not their product: case (i, j) takes gap
model i and matrix kind j, and the three narrower axes are linear in (i, j) so that every pair of values of two
different axes occurs in some case (tests/test_cases_cpu.py asserts it). Everything else is drawn from the case's seed.
A plain module: no fixture, nothing that changes how a test runs."""
import functools
import typing

import numpy as np

ALPHABETS = (2, 4, 20, 32)
GAPS = ((0, 0), (0, 2), (1, 3), (2, 2), (3, 1), (5, 0), (11, 1), (40, 12))     # (open, extend)
KINDS = ("asymmetric", "symmetric", "nonpositive", "nonnegative", "plusminus")
SPANS = ("whole", "two")
QUERY_LENGTHS = (1, 7, 64, 65, 130)     # one row, inside a strip, a full strip, its edge, three strips
AXES = {"alphabet": ALPHABETS, "gaps": GAPS, "kind": KINDS, "span": SPANS, "q": QUERY_LENGTHS}
TARGETS = 130        # lane per target: two full wavefronts and a ragged third
LONGEST = 200
PAIRS = 300


class SearchSet(typing.NamedTuple):
    """what a one-query entry point is given: `rows` is the query as a PSSM (the matrix rows of its residues, tests/_pssm.py's
    class identity), `copy` and `twice` the targets that hold a noisy copy of the query and the query two times over"""
    matrix: np.ndarray      # int32[A * A]
    query: np.ndarray       # uint8[Q]
    rows: np.ndarray        # int32[Q][A]
    targets: list           # uint8 arrays
    residues: np.ndarray
    offsets: np.ndarray     # int64[targets + 1]
    lengths: np.ndarray
    letters: np.ndarray     # the residues in use
    copy: int
    twice: int


class PairSet(typing.NamedTuple):
    """what a pair-list entry point is given, over the targets of the case's SearchSet: a query of every length of
    QUERY_LENGTHS (the case's own among them) and pairs in random order, with repeats"""
    queries: list           # uint8 arrays
    pair_query: np.ndarray  # int32[pairs]
    pair_target: np.ndarray  # int64[pairs]


class Case(typing.NamedTuple):
    index: int
    alphabet: int
    gaps: tuple
    kind: str
    span: str
    q: int

    @property
    def seed(self):
        return 7000 + self.index

    @property
    def id(self):
        return f"{self.index:02d}-a{self.alphabet}-g{self.gaps[0]}.{self.gaps[1]}-{self.kind}-{self.span}-q{self.q}"

    def search_set(self) -> SearchSet:
        return _search_set(self)

    def pair_set(self) -> PairSet:
        return _pair_set(self)


def cases():
    """the list, the same records at every call"""
    return list(_cases())


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for i, gaps in enumerate(GAPS):
        for j, kind in enumerate(KINDS):
            out.append(Case(len(out), ALPHABETS[(i + j) % 4], gaps, kind, SPANS[(j + i // 4) % 2],
                            QUERY_LENGTHS[(i + 2 * j) % 5]))
    return tuple(out)


def letters_of(case, rng):
    """the residues a case's sequences are written in: all of them, or two - one drawn, and the alphabet's last.
    (At two letters the two spans are the same residues: the pair (alphabet 2, span two) of the census is covered in
    name only; a two-letter span inside a wider table is what the cases of 4, 20 and 32 letters add.)"""
    if case.span == "whole" or case.alphabet == 2:
        return np.arange(case.alphabet, dtype=np.uint8)
    return np.array([rng.integers(0, case.alphabet - 1), case.alphabet - 1], dtype=np.uint8)


def matrix_of(case, rng, letters):
    A = case.alphabet
    m = rng.integers(-4, 12, size=(A, A))
    sparse = rng.random((A, A)) < 0.3
    if case.kind == "symmetric":
        m = np.triu(m) + np.triu(m, 1).T
    elif case.kind == "nonpositive":
        m = np.where(sparse, 0, -1 - (m + 4) % 6)
    elif case.kind == "nonnegative":
        m = np.where(sparse, 0, m + 4)
    elif case.kind == "plusminus":
        m = np.where(m % 2 == 0, 1, -1)
    # the residues in use see both sides of the kind: a zero and a non-zero entry, a +1 and a -1
    a, b = int(letters[0]), int(letters[-1])
    if case.kind in ("nonpositive", "nonnegative"):
        m[a, b] = 0
        m[b, a] = -3 if case.kind == "nonpositive" else 5
    elif case.kind == "plusminus":
        m[a, b], m[b, a] = 1, -1
    return np.ascontiguousarray(m.ravel(), dtype=np.int32)


def noisy(rng, letters, seq):
    """a copy with a tenth of its residues substituted, two residues dropped and two put in (where there is room)"""
    out = np.array(seq, dtype=np.uint8)
    swap = rng.random(len(out)) < 0.1
    out[swap] = letters[rng.integers(0, len(letters), size=int(swap.sum()))]
    if len(out) >= 7:
        cut, put = sorted(rng.choice(np.arange(1, len(out) - 2), size=2, replace=False).tolist())
        out = np.concatenate([out[:cut], out[cut + 2:put], letters[rng.integers(0, len(letters), size=2)], out[put:]])
    return out


@functools.lru_cache(maxsize=None)
def _search_set(case):
    rng = np.random.default_rng(case.seed)
    letters = letters_of(case, rng)
    matrix = matrix_of(case, rng, letters)
    draw = lambda n: letters[rng.integers(0, len(letters), size=int(n))]   # noqa: E731
    query = draw(case.q)
    lengths = rng.integers(0, LONGEST + 1, size=TARGETS)
    edges = sorted({0, 1, LONGEST, case.q - 1, case.q, case.q + 1})
    lengths[:len(edges)] = edges
    lengths[len(edges)] = 0       # (a second empty target, wherever the shuffle puts it)
    rng.shuffle(lengths)
    targets = [draw(n) for n in lengths]
    free = [k for k in range(TARGETS) if lengths[k] not in edges]
    copy, twice = (int(k) for k in rng.choice(free, size=2, replace=False))
    targets[copy] = np.concatenate([draw(rng.integers(0, 30)), noisy(rng, letters, query), draw(rng.integers(0, 30))])
    targets[twice] = np.concatenate([query, query])
    lengths = np.array([len(t) for t in targets], dtype=np.int64)
    offsets = np.zeros(TARGETS + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    residues = np.ascontiguousarray(np.concatenate(targets), dtype=np.uint8)
    rows = np.ascontiguousarray(matrix.reshape(case.alphabet, case.alphabet)[query])
    for array in (matrix, query, rows, residues, offsets, lengths, letters, *targets):
        array.setflags(write=False)
    return SearchSet(matrix, query, rows, targets, residues, offsets, lengths, letters, copy, twice)


@functools.lru_cache(maxsize=None)
def _pair_set(case):
    s = case.search_set()
    rng = np.random.default_rng(case.seed + 500)
    queries = [s.query if n == case.q else s.letters[rng.integers(0, len(s.letters), size=n)] for n in QUERY_LENGTHS]
    pq = rng.integers(0, len(queries), size=PAIRS - 20)
    pt = rng.integers(0, TARGETS, size=PAIRS - 20)
    pq[:30], pt[:30] = pq[30:60], pt[30:60]     # repeats
    empty = np.flatnonzero(s.lengths == 0)
    special = np.array([(i, t) for i in range(len(queries)) for t in (*empty, s.copy, s.twice)])
    pq, pt = np.concatenate([pq, special[:, 0]]), np.concatenate([pt, special[:, 1]])
    order = rng.permutation(len(pq))
    pq, pt = pq[order].astype(np.int32), pt[order].astype(np.int64)
    for array in (pq, pt, *queries):
        array.setflags(write=False)
    return PairSet(queries, pq, pt)
