"""Every entry point after every other on one handle. A call borrows a workspace of the handle (slots that are reused
with their contents, or freed and allocated again uninitialised; state kept across calls on purpose: the column split's
flags and plan, the sorted jobs of a slice, the PSSM rows, the view cache, kernel timings; staged downloads of a call
that failed), so what one call leaves behind is what the next one finds. The nodes of tests/_call_mix.py are run along
an Eulerian circuit of all ordered pairs (A, then B), (A, A) included, cut into segments with one handle each, and every
array of every answer is compared with the CPU witnesses' for dtype, shape and bytes - in two regimes: the default bound
on parked workspaces, under which a test-sized handle never trims, and MIOPAL_PARKED_WORKSPACE_MB=0, under which the
end of every call frees whatever that call did not use and the next call meets fresh allocations. Four threads on one
handle run rotations of a segment; the 32-letter handle interleaves the PSSM aligned panel (two runs of its alignment
stage) with its single-PSSM and plain-panel forms.

The routing reports are not compared: they may depend on measured timings.

Measured durations: profiles/call_order_tests.txt."""
import threading

import numpy as np
import pytest

import _call_mix as mix

pytestmark = pytest.mark.gpu

NODES = mix.NODES
ORDER = mix.circuit(len(NODES))
SEGMENT = 121                                   # pairs per segment: 16 segments of the 44 x 44 pairs
RUNS = mix.segments(ORDER, SEGMENT)
REGIMES = ("default", "trim")
THREADS = 4


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


def open_handle(capi, w=None):
    w = w or mix.world()
    return capi.DeviceDatabase(w.residues, w.offsets, w.alphabet)


@pytest.fixture(scope="module")
def answers(capi):
    """node name -> the expected answer, computed once and never changed. The significance searches take their fit from
    the same call on a fresh handle."""
    out = {}
    for node in NODES + mix.NODES32:
        if node.fresh:
            db = open_handle(capi)
            try:
                out[node.name] = node.expected(node.run(db))
            finally:
                db.close()
            assert 0 < out[node.name]["count"][0] < np.diff(mix.bounds(node.span))[0], node.name
        else:
            out[node.name] = node.expected()
    return out


def enter(tuning, regime):
    if regime == "trim":
        tuning.setenv("MIOPAL_PARKED_WORKSPACE_MB", "0")


class Unexpected(Exception):
    """a node raised where it must answer: the handle, and after a device fault the process, is in no state to go on"""


def stop(failures):
    """ends the session: after a call that raised - a device fault, perhaps - nothing more is started on the device"""
    pytest.exit("a call of the call-order tests raised:\n" + "\n".join(failures[:20]), returncode=1)


def call(db, node, answers, previous, regime, failures, where=""):
    """one node on the handle; what differs from its expected answer goes to ``failures`` under the pair's name"""
    pair = f"({previous.name if previous else 'a fresh handle'}, then {node.name}) [{regime}{where}]"
    try:
        got = node.run(db)
    except Exception as error:   # noqa: BLE001 (whatever the call raised is the finding)
        failures.append(f"{pair}: {type(error).__name__}: {error}")
        raise Unexpected(failures[-1]) from error
    for difference in mix.differences(got, answers[node.name]):
        failures.append(f"{pair}: {difference}")
    return node


def run_order(db, order, nodes, answers, regime, failures, where=""):
    previous = None
    for index in order:
        previous = call(db, nodes[index], answers, previous, regime, failures, where)
    # the end of a run: the idle workspaces released, then the first node again
    db.release_workspaces()
    call(db, nodes[order[0]], answers, mix.node("release_workspaces"), regime, failures, where)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("segment", range(len(RUNS)))
def test_every_pair_of_the_circuit(capi, tuning, answers, segment, regime):
    enter(tuning, regime)
    failures = []
    db = open_handle(capi)
    try:
        run_order(db, RUNS[segment], NODES, answers, regime, failures)
    except Unexpected:
        stop(failures)
    finally:
        db.close()
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("full", ("search full sw 65", "search_pssm full ov"))
def test_trimming_happens(capi, tuning, answers, full):
    """With the bound at 0 a score search behind a `full` one gives back what only the `full` one used - the direction
    bits, the operations - so the handle holds fewer bytes after it than right after the `full` search; under the
    default bound nothing is given back. The bytes in question are those of the handle's parked workspaces, which
    `release_workspaces` reports as it frees them - so the `full` search runs twice, once to be measured and once in
    front of the score search. `device_bytes` is read beside them and printed: it counts the resident database and
    its packed views, which trimming does not touch and which grow when the score search builds a view of its own."""
    score = mix.node("search score sw 53")
    held = {}
    for regime in REGIMES:
        enter(tuning, regime)
        failures = []
        db = open_handle(capi)
        try:
            call(db, mix.node(full), answers, None, regime, failures)
            mirror_full = db.device_bytes()
            after_full = db.release_workspaces()
            previous = call(db, mix.node(full), answers, mix.node("release_workspaces"), regime, failures)
            call(db, score, answers, previous, regime, failures)
            mirror_score = db.device_bytes()
            after_score = db.release_workspaces()
        except Unexpected:
            stop(failures)
        finally:
            db.close()
        assert not failures, "\n".join(failures)
        held[regime] = (after_full, after_score)
        print(f"{full}, {regime}: {after_full} bytes of workspaces parked after the full search, {after_score} after the "
              f"score search behind it (database and views: {mirror_full}, then {mirror_score})")
    assert 0 < held["trim"][1] < held["trim"][0], held
    assert held["default"][1] >= held["default"][0] > 0, held


def rotations(run, threads):
    """``threads`` rotations of a run, evenly spaced"""
    run = list(run)
    return [run[len(run) * t // threads:] + run[:len(run) * t // threads] for t in range(threads)]


def threads_on_one_handle(db, orders, nodes, answers, regime):
    failures = [[] for _ in orders]
    raised = []

    def worker(t):
        try:
            run_order(db, orders[t], nodes, answers, regime, failures[t], f", thread {t}")
        except Unexpected as error:
            raised.append(str(error))
    pool = [threading.Thread(target=worker, args=(t,)) for t in range(len(orders))]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    if raised:
        stop(raised)
    return [f for per_thread in failures for f in per_thread]


@pytest.mark.parametrize("regime", REGIMES)
def test_four_threads_on_one_handle(capi, tuning, answers, regime):
    """each thread a different rotation of the segment that visits the most nodes"""
    enter(tuning, regime)
    run = max(RUNS, key=lambda r: len(set(r)))
    assert len(set(run)) >= len(NODES) * 3 // 4
    db = open_handle(capi)
    try:
        failures = threads_on_one_handle(db, rotations(run, THREADS), NODES, answers, regime)
    finally:
        db.close()
    assert not failures, "\n".join(failures[:20])


# The pairs that failed on the tree, kept as a case of their own: a query of several strips on a workspace that has just
# been allocated, beside the searches of three other threads - (release_workspaces, then search_batch_hits) and
# (release_workspaces, then search end nw 130) with the bound at 0 read "-2" and "6439 (pair, strip) units gave up
# waiting" from the give-up counter of the wavefront-per-pair strips kernel, which was zeroed on the null stream and
# read before the zero had landed (host_search.inc).
FRESH_STRIP_COUNTER = ("release_workspaces", "search_batch_hits", "release_workspaces", "search end nw 130",
                       "release_workspaces", "search_occurrences hw 130", "search score sw 53 long target")


@pytest.mark.parametrize("regime", REGIMES)
def test_fresh_strip_counter_beside_other_threads(capi, tuning, answers, regime):
    enter(tuning, regime)
    run = [NODES.index(mix.node(name)) for name in FRESH_STRIP_COUNTER] * 6
    db = open_handle(capi)
    try:
        failures = threads_on_one_handle(db, rotations(run, THREADS), NODES, answers, regime)
    finally:
        db.close()
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("regime", REGIMES)
def test_four_threads_on_the_pssm_panel_handle(capi, tuning, answers, regime):
    """the 32-letter handle: the PSSM aligned panel, its single-PSSM form and the plain panel, every pair of them, each
    thread a different rotation"""
    enter(tuning, regime)
    run = mix.circuit(len(mix.NODES32)) * 2
    db = open_handle(capi, mix.world32())
    try:
        failures = threads_on_one_handle(db, rotations(run, THREADS), mix.NODES32, answers, regime)
    finally:
        db.close()
    assert not failures, "\n".join(failures[:20])
