"""The inputs of the call-order tests (tests/_call_mix.py) held to their purpose, without a device: the circuit and its
segments cover every ordered pair of nodes exactly once, every node has an answer to be compared with, every small form
lies strictly inside its large form, and the numpy witnesses behind the answers agree with the C checker where they are
not the checker itself."""
import numpy as np

import _call_mix as mix
import _oracle
from pyopal_amd import _capi


def test_the_circuit_covers_every_ordered_pair_once():
    for n in (1, 2, 3, 7, len(mix.NODES)):
        order = mix.circuit(n)
        assert len(order) == n * n + 1 and order[0] == order[-1] == 0
        pairs = mix.pairs_of(order)
        assert len(set(pairs)) == len(pairs) == n * n
        assert set(pairs) == {(a, b) for a in range(n) for b in range(n)}


def test_the_segments_cover_the_same_pairs():
    n = len(mix.NODES)
    order = mix.circuit(n)
    for length in (1, 7, 100, 242, n * n, n * n + 5):
        runs = mix.segments(order, length)
        assert all(2 <= len(run) <= length + 1 for run in runs)
        assert all(a[-1] == b[0] for a, b in zip(runs, runs[1:]))
        pairs = [p for run in runs for p in mix.pairs_of(run)]
        assert pairs == mix.pairs_of(order)


def stand_in(node):
    """in the place of a fresh handle's answer to a significance search: a fit whose every threshold is the middle
    score of the checker's, and no E-values"""
    fit = _capi.ScoreFit()
    cut = mix.cut_of(mix.checker({"search_significant": "q53", "search_significant small": "q30"}[node.name], "score", "sw", node.span)["score"])
    for b in range(_capi.MIOPAL_STAT_BINS):
        fit.threshold[b] = cut
    return {"fit": np.frombuffer(bytes(fit), dtype=np.uint8), "evalue": np.zeros(0)}


def test_every_node_has_an_answer():
    families = set()
    for node in mix.NODES + mix.NODES32:
        want = node.expected(stand_in(node)) if node.fresh else node.expected()
        families.add(node.family)
        if node.name == "release_workspaces":
            assert want == {}
            continue
        assert want and all(isinstance(a, np.ndarray) for a in want.values()), node.name
        if node.fails:
            assert sorted(want) in (["counts"], ["message"]) and want[sorted(want)[0]].size > 0, node.name
            continue
        # not empty, and not every target (or every column of every target) of the slice
        lo, hi = mix.bounds(node.span, mix.world32() if node in mix.NODES32 else mix.world())
        for key, a in want.items():
            if key not in ("aln_flat", "evalue"):
                assert a.size > 0, (node.name, key)
        if "count" in want and "target" in want and want["count"].shape == (1,):
            found = int(want["count"][0])
            assert 0 < found, node.name
            if "occurrence" not in node.family:
                assert found < hi - lo, node.name
        if "offsets" in want:
            assert want["offsets"][-1] > 0 and np.all(np.diff(want["offsets"]) >= 0), node.name
            if "occurrence" in node.family:
                assert np.all(np.diff(want["offsets"]) > 0), (node.name, np.diff(want["offsets"]))
        if "aln_off" in want:
            assert want["aln_off"][-1] == len(want["aln_flat"]) > 0, node.name
    assert len(families) >= 21 and len(mix.NODES) == 44


def test_the_answers_hold_what_the_database_was_built_for():
    w = mix.world()
    assert len(w.lengths) == mix.TARGETS and w.lengths[mix.LONG_AT] == mix.LONGEST and np.all(w.lengths[list(mix.EMPTY)] == 0)
    assert np.count_nonzero(w.lengths == 0) == 2 and np.delete(w.lengths, mix.LONG_AT).max() <= 300
    # the noisy copy and the double are the best targets of their queries
    assert int(np.argmax(mix.checker("q130", "score", "sw")["score"])) == mix.NOISY_AT
    assert int(np.argmax(mix.checker("q53", "score", "sw")["score"])) == mix.TWICE_AT
    twice = mix.node("search_occurrence_alignments").expected()
    assert np.count_nonzero(twice["target"] == mix.TWICE_AT) == 2
    # pairs on the empty targets, repeats, the long target
    pairs = mix.node("align_pairs full").expected()
    assert len(pairs["score"]) == 300 and np.count_nonzero(np.diff(pairs["aln_off"]) == 0) >= 2
    # the padding behind the count of the top searches
    top = mix.node("search_top full").expected()
    assert top["target"][-1] == -1 and top["target"][int(top["count"][0]) - 1] >= 0
    assert np.all(mix.node("search_batch_top").expected()["target"][:, -1] == -1)
    # the strip workspace of the long query, the two runs of the PSSM panel
    assert mix.node("search_occurrences hw 130").query_length > 64
    assert sum(len(s.query) for s in mix.world32().sides.values()) == 768


def test_every_small_form_is_strictly_inside_its_large_form():
    by_family = {}
    for node in mix.NODES:
        if node.form:
            by_family.setdefault(node.family, {})[node.form] = node
    assert len(by_family) >= 19
    for family, forms in by_family.items():
        assert sorted(forms) == ["large", "small"], family
        large, small = forms["large"], forms["small"]
        assert small.query_length < large.query_length, family
        (lo, hi), (slo, shi) = mix.bounds(large.span), mix.bounds(small.span)
        assert lo <= slo < shi <= hi and (shi - slo) < (hi - lo), family
    # every entry point of the handle that searches is a family, or a node of the 32-letter handle
    families = {n.family for n in mix.NODES + mix.NODES32}
    for name in ("search", "search_pssm", "search_batch", "search_top", "search_batch_top", "search_hits", "search_batch_hits",
                 "search_pssm_hits", "search_significant", "search_batch_target_top", "align_pairs", "align_pairs_pssm",
                 "profile_columns", "search_occurrences", "search_occurrences_pssm", "search_occurrence_alignments",
                 "search_occurrence_alignments_pssm", "search_batch_occurrences", "search_batch_occurrences_pssm",
                 "search_batch_occurrence_alignments", "search_batch_occurrence_alignments_pssm", "search_device_scores",
                 "release_workspaces"):
        assert name in families and hasattr(_capi.DeviceDatabase, name), name


def test_the_column_witness_agrees_with_the_checker():
    """the best column value of every target is the checker's score of it ("hw": the last row's maximum, "sw": the
    matrix's), for a plain query of three strips with the long target, a PSSM, and a PSSM of the 32-letter database"""
    for name, algorithm, w in (("q130", "hw", 24), ("q53", "sw", 24), ("p65", "sw", 24), ("q9", "hw", 24), ("m3", "hw", 32)):
        V, R, offsets = mix.column_witness(name, algorithm, w)
        scores = mix.checker(name, "score", algorithm, None, w)["score"]
        ends = mix.checker(name, "end", algorithm, None, w)
        for k in range(len(offsets) - 1):
            column = V[offsets[k]:offsets[k + 1]]
            if len(column) == 0 or (algorithm == "sw" and scores[k] == 0):
                continue
            assert column.max() == scores[k], (name, algorithm, k)
            at = int(ends["end_t"][k])
            assert column[at] == scores[k] and R[offsets[k] + at] == ends["end_q"][k], (name, algorithm, k)


def test_the_aligned_witness_agrees_with_the_checker():
    """an occurrence that is its target's best under "sw" starts where the checker's alignment starts and has its operations"""
    for node, name, w in ((mix.node("search_occurrence_alignments small"), "q9", 24), (mix.NODES32[1], "m3", 32)):
        want = node.expected()
        algorithm = "sw" if w == 24 else "hw"
        full = mix.checker(name, "full", algorithm, None, w)
        checked = 0
        for k in range(int(want["count"][0])):
            t = int(want["target"][k])
            if want["score"][k] == full["score"][t] and want["end_t"][k] == full["end_t"][t] and want["end_q"][k] == full["end_q"][t]:
                ops = want["aln_flat"][want["aln_off"][k]:want["aln_off"][k + 1]]
                if algorithm == "hw" and full["start_t"][t] < 0:
                    continue
                assert (want["start_t"][k], want["start_q"][k]) == (full["start_t"][t], full["start_q"][t]), (node.name, k)
                assert ops.tolist() == full["aln"][t].tolist(), (node.name, k)
                checked += 1
        assert checked >= 3, (node.name, checked)


def test_the_selections_restate_the_checker():
    """spot checks of the numpy selections: each hit is at or above its cut and nothing else is; the best queries of a
    target are the best"""
    hits = mix.node("search_batch_hits").expected()
    for i, name in enumerate(("q53", "q130", "q9")):
        scores = mix.checker(name, "score", "nw")["score"]
        lo, hi = hits["offsets"][i], hits["offsets"][i + 1]
        cut = hits["score"][lo:hi].min()
        assert np.array_equal(hits["target"][lo:hi], np.flatnonzero(scores >= cut)) and 0 < hi - lo < mix.TARGETS
    best = mix.node("search_batch_target_top").expected()
    stack = np.stack([mix.checker(n, "score", "sw")["score"] for n in ("q53", "q65", "q30", "q9")])
    full = best["count"] == 2
    assert full.any() and not full.all()
    assert np.array_equal(best["score"][full, 0], stack[:, full].max(axis=0))
    # the profile of the query alone beside members that cover nothing is not what the node asks for
    profile = mix.node("profile_columns").expected()
    assert profile["msa"].shape == (151, 65) and np.all(profile["msa"][0] == mix.side("q65").query)
    assert np.all(profile["msa"][1] == 255) and (profile["msa"][1:] != 255).any() and profile["counts"].sum() > 65
    assert _oracle.search(mix.side("q65").query, mix.world().residues, mix.world().offsets, mix.B62, 3, 1, "score", "sw")["score"][mix.EMPTY[0]] == 0
