"""Inputs for the tests at the edges of the static range rules (test_range_edges_cpu.py, test_gpu_range_edges.py) and
of the 32-bit rule behind them (test_int32_edges_cpu.py, test_gpu_int32_edges.py: INT32_AXES and what follows it).

NW, HW and OV run on 16-bit patterns when inequalities over the scoring model say so (score_ranges.h:
globalOneStripFits, globalStripsFit, fitsPlain, fitsDiag, fitsUnsigned; perpair_packed.hip: packedScanFits,
packedTraceFits). Nothing is flagged or redone afterwards, so a test of such a rule needs

  * a scoring model whose extreme entries are what the rule reads and nothing else: `edge_matrix`,
  * targets that drive the kernel's values to both ends of the range the rule promises: `family`,
  * the last value the ROUTER admits, not a copy of the formula: `last_admitted`.

No fixtures and nothing that changes how tests run.
"""
import numpy as np

ALPHABET = 24
# two ordinary letters and the one every pairing of which scores `low`
LETTER_A, LETTER_B, LETTER_C = 3, 17, 9
# the model the axes of the GPU tests start from: match / mild / low, open / ext
BASE = dict(match=11, mild=-1, low=-4, open=3, ext=1)
QUERY_FORMS = ("one", "alternating", "random")


def edge_matrix(A, match, mild, low, c):
    """A x A scores, flat int32: `match` on the diagonal, `mild` between ordinary letters, `low` for every pairing with
    letter `c` but c against itself. Its maximum is `match` and its minimum `low` whatever else it holds."""
    assert low <= mild <= match and 0 <= c < A
    m = np.full((A, A), mild, dtype=np.int32)
    m[c, :] = low
    m[:, c] = low
    np.fill_diagonal(m, match)
    return m.ravel()


def model_matrix(model, A=ALPHABET, c=LETTER_C):
    return edge_matrix(A, model["match"], model["mild"], model["low"], c)


def edge_query(form, Q, seed=0, letters=(LETTER_A, LETTER_B)):
    """A query of two ordinary letters: all one letter, alternating, or random."""
    a, b = letters
    if form == "one":
        q = np.full(Q, a)
    elif form == "alternating":
        q = np.where(np.arange(Q) % 2 == 0, a, b)
    elif form == "random":
        q = np.where(np.random.default_rng(1000 + seed + Q).integers(0, 2, size=Q) == 0, a, b)
    else:
        raise ValueError(form)
    return q.astype(np.uint8)


def pc(k, c=LETTER_C):
    return np.full(int(k), c, dtype=np.uint8)


def family(q, c=LETTER_C, long=3000, seed=0, n_random=200, max_random=None, letters=(LETTER_A, LETTER_B)):
    """The edge family of targets for query `q` (list of uint8 arrays). A copy of the query takes the patterns to the
    top of the range (Q * match); runs of letter `c` take them to the bottom: before, after, inside and instead of the
    query, short, as long as the query, four times as long and `long` residues (HW and OV rebase their column shift
    many times on these when ext is large). Then 200 random strings over the three letters, 1 .. 3 Q + 1 residues
    (`max_random` caps that)."""
    Q = len(q)
    cat = lambda *parts: np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]).astype(np.uint8)
    seqs = [
        q.copy(),
        cat(q, q),
        cat(pc(7, c), q, pc(5, c)),
        pc(1, c), pc(Q, c), pc(4 * Q, c), pc(long, c),
        cat(q[:Q // 2], pc(Q, c), q[Q // 2:]),      # a high run, a deep valley, a high run
        cat(pc(Q, c), q),
        cat(q, pc(Q, c)),
        cat(pc(long, c), q),
        cat(q, pc(long, c)),
        np.delete(q, Q // 2),
        q[:1].copy(),
        np.zeros(0, dtype=np.uint8),
    ]
    rng = np.random.default_rng(77 + seed + Q)
    three = np.array([letters[0], letters[1], c], dtype=np.uint8)
    top = 3 * Q + 1 if max_random is None else min(3 * Q + 1, max_random)
    for n in rng.integers(1, top + 1, size=n_random):
        seqs.append(three[rng.integers(0, 3, size=int(n))])
    return seqs


# A search of few targets sends every leading group of 128 targets whose longest has more than 512 columns to the
# wavefront-per-pair kernel beside the packed launch (host_search.inc, planSideCut). What has to meet the kernel under
# test therefore has at most STAYS columns, and the longer targets of a database are made a whole number of groups,
# so that no short target leaves with them.
STAYS, GROUP = 512, 128


def lanes_members(q, c=LETTER_C):
    """The `long` members of the family once more at the greatest length that stays in the lanes of a small search."""
    Q = len(q)
    if Q + 8 > STAYS:
        return []
    k = STAYS - Q
    return [pc(STAYS, c), np.concatenate([pc(k, c), q]).astype(np.uint8), np.concatenate([q, pc(k, c)]).astype(np.uint8)]


def whole_groups(seqs, c=LETTER_C, letters=(LETTER_A, LETTER_B), seed=0):
    """`seqs` plus random strings of 513 .. 640 residues until the targets beyond STAYS columns fill whole groups."""
    rng = np.random.default_rng(5 + seed)
    three = np.array([letters[0], letters[1], c], dtype=np.uint8)
    beyond = sum(1 for s in seqs if len(s) > STAYS)
    out = list(seqs)
    for _ in range((-beyond) % GROUP):
        out.append(three[rng.integers(0, 3, size=int(rng.integers(STAYS + 1, 641)))])
    return out


def last_admitted(search, lo, hi):
    """The last v in [lo, hi) with search(v) true, by bisection over one integer parameter, every other one fixed.
    search(v) runs one tiny search and says whether the routing word names the kernel under test. `lo` must be
    admitted and `hi` must not: a probe that cannot find both sides fails the test."""
    assert lo < hi, (lo, hi)
    assert search(lo), f"the probe's low end {lo} is not admitted: the rule under test decides nothing here"
    assert not search(hi), f"the probe's high end {hi} is still admitted: the rule under test decides nothing here"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if search(mid):
            lo = mid
        else:
            hi = mid
    return lo


# ---- the models that both tiers use -----------------------------------------------------------------------------
# The GPU tier takes its thresholds from the router; what is fixed here is the far end of every probe and the sizes
# it runs at. The CPU tier asserts that the checker's 32-bit sums stay below 2^29 over all of it.
# axis -> (parameter(s) probed, low end, high end); the other parameters stay at BASE. The `low` axis probes -low.
AXES = {
    "match": (("match",), 11, 20000),
    "low": (("low",), 4, 1024),
    "open": (("open",), 3, 30000),
    "open=ext": (("open", "ext"), 1, 5000),
}


def axis_model(axis, v, base=BASE):
    m = dict(base)
    for name in AXES[axis][0]:
        m[name] = -v if name == "low" else v
    return m


# ---- the edge of the 32-bit rule (test_int32_edges_cpu.py, test_gpu_int32_edges.py) ----------------------------------
# Every entry point refuses a model with int32Bound >= 2^29 (score_ranges.h):
#   2 |open| + (Q + longest) |ext| + min(Q, longest) mag + mag,   mag = the largest absolute substitution score.
# Each axis takes one term of that bound (`mixed`: all of them) to the last value that is admitted; the other
# parameters stay at BASE. axis -> (model of v, low end of the probe). There is no axis of ext alone: with open < ext
# the borders are made of openings and the extension is never used.
INT32_AXES = {
    "match": (lambda v: dict(BASE, match=v), BASE["match"]),                      # the top of the range, Q * match
    "low": (lambda v: dict(BASE, low=-v), -BASE["low"]),                          # transient diag + score sums only
    "open": (lambda v: dict(BASE, open=v, ext=1), BASE["open"]),                  # borders less open beside minus infinity
    "open=ext": (lambda v: dict(BASE, open=v, ext=v), BASE["ext"]),               # deep true values, the column scale j * ext
    "mixed": (lambda v: dict(BASE, match=v, low=-v, open=16 * v, ext=max(v // 8, 1)), BASE["match"]),
}
INT32_HIGH = 1 << 29      # refused on every axis
INT32_Q = (1, 33, 64, 65, 130)   # one row, one strip, the edge of a strip, two strips, three strips
INT32_LONG = 300


def int32_model(axis, v):
    return INT32_AXES[axis][0](int(v))


def int32_forms(axis):
    """the query forms an axis runs with: all one letter as well where the lowest score is at its far end"""
    return ("random", "one") if axis in ("low", "mixed") else ("random",)


def int32_family(form, Q):
    """(query, targets): about 55 targets of at most INT32_LONG + Q residues (4 Q where that is more) - the smallest family that still has a
    copy of the query, runs of the low letter on every side of it, an empty target, and lanes shorter than the
    longest target of their wavefront"""
    q = edge_query(form, Q)
    return q, family(q, long=INT32_LONG, n_random=40)


def int32_formula(model, Q, longest):
    """int32Bound of score_ranges.h, for the CPU tier (which has no router to ask); the GPU tier probes the router"""
    mag = max(abs(model["match"]), abs(model["mild"]), abs(model["low"]))
    return 2 * abs(model["open"]) + (Q + longest) * abs(model["ext"]) + min(Q, longest) * mag + mag


def int32_formula_last(axis, Q, longest):
    """the largest v of `axis` with the formula's bound below 2^29"""
    return last_admitted(lambda v: int32_formula(int32_model(axis, v), Q, longest) < (1 << 29), INT32_AXES[axis][1], INT32_HIGH)


ONE_STRIP_Q = (2, 33, 60)
STRIPS_Q = (65, 147, 333)
PACKED_Q = (7, 64, 130)
LONG = 3000
# the general kernel's flavours: (name, Q, model) - ext 60 keeps the longest packed target near 450 columns, match 500
# at Q = 63 / 64 puts min(Q, L) * match on both sides of 32000; `low` -200 keeps the unsigned flavour out of the signed
# shifted one's test (min + ext + open < 0)
GENERAL_MODELS = {
    "plain": [("ext60", 33, dict(match=11, mild=-1, low=-4, open=60, ext=60)),
              ("match500-Q64", 64, dict(match=500, mild=-1, low=-4, open=3, ext=1))],
    "diag": [("ext60", 33, dict(match=11, mild=-1, low=-200, open=60, ext=60)),
             ("match500-Q64", 64, dict(match=500, mild=-1, low=-200, open=3, ext=1)),
             ("match500-Q63", 63, dict(match=500, mild=-1, low=-200, open=3, ext=1))],
    "unsigned": [("ext60", 33, dict(match=11, mild=-1, low=-4, open=60, ext=60)),
                 ("match420-Q64", 64, dict(match=420, mild=-1, low=-4, open=3, ext=1))],
}
# CPU tier only: the checker against the numpy recurrence far beyond anything a 16-bit kernel takes
EXTREME = dict(match=4000, mild=-1, low=-1023, open=9000, ext=819)


def shared_models():
    """(tag, Q, longest target, model): every fixed model of the GPU tier and the far end of every probe."""
    out = []
    for qs, long in ((ONE_STRIP_Q, LONG + max(ONE_STRIP_Q)), (STRIPS_Q, LONG + max(STRIPS_Q)), (PACKED_Q, 700)):
        for axis, (_, lo, hi) in AXES.items():
            for v in (lo, hi):
                out.append((f"{axis}={v}", max(qs), long, axis_model(axis, v)))
    for flavour, models in GENERAL_MODELS.items():
        for tag, Q, m in models:
            out.append((f"{flavour} {tag}", Q, STAYS + 8, m))
    # the query-length axis of the strips kernel: BLOSUM62 (11 / -4) 11 / 1, queries up to 4000 residues
    out.append(("Q axis", 4000, 4 * 4000, dict(match=11, mild=-1, low=-4, open=11, ext=1)))
    out.append(("trace ext 40", max(PACKED_Q), 700, dict(BASE, open=42, ext=40)))
    # HW in windows beside the shifted flavours, signed (low = -3 ext) and unsigned (low = -4)
    for ext, low in ((60, -180), (200, -600), (820, -2460), (200, -4), (600, -4)):
        out.append((f"HW windows ext {ext} low {low}", max(ONE_STRIP_Q), LONG + max(ONE_STRIP_Q),
                    dict(match=11, mild=-1, low=low, open=ext, ext=ext)))
    # the topGap pair of the `open` axis: opening as cheap as extending, and cheaper
    for go in (1, 0):
        out.append((f"topGap open {go}", max(STRIPS_Q), LONG + max(STRIPS_Q), dict(BASE, open=go, ext=1)))
    # unsignedDiagUsable's clauses, from both sides, and the far end of its probe along `open`
    for go, ge, low in ((5, 5, -4), (4, 5, -4), (3, 1, -5), (5, 4, -9), (5, 4, -10), (4000, 1, -4)):
        out.append((f"unsigned usable {go}/{ge} low {low}", 33, STAYS + 8, dict(BASE, open=go, ext=ge, low=low)))
    out.append(("plain match500-Q63", 63, STAYS + 8, dict(match=500, mild=-1, low=-4, open=3, ext=1)))
    out.append(("trace range clause ext 120", 260, 700 + 260, dict(BASE, open=122, ext=120)))
    return out
