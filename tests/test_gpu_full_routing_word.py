"""The routing word of the passes behind the score / end pass (include/miopal.h, miopalLastFullRouting) pinned case by
case: which kernels take the start-cell scan and the direction pass, whether the operations leave batch by batch, is a
decision of the host's plan (pyopal_amd/csrc/full_plan.h, host_full.inc) - a change of that code that is meant to
change no routing must leave every word as tests/golden/full_routing_words.json recorded it. The same for
miopalLastPairRouting of one align_pairs call in `full` mode on the same pairs (host_pairs.inc takes its estimates
from the same header). Every result is held to the CPU checker bit for bit, so that a word is never pinned on a
wrong answer.

Database: 700 targets of 1 to 349 residues (test_gpu_full_packed.py's shape), MIOPAL_NO_SMALL_SEARCH set (conftest.py).
Cases: four modes x Q in {1, 64, 65, 260} x BLOSUM62 / BLOSUM50 at gaps 3/1 x seven sets of switches.
"""
import json
import os

import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "full_routing_words.json")
MATRICES = {name: np.array(ScoringMatrix.from_name(name).int_array(), dtype=np.int32) for name in ("BLOSUM62", "BLOSUM50")}
ALGOS = ("sw", "nw", "hw", "ov")
QS = (1, 64, 65, 260)
SWITCHES = {
    "none": (),
    "force_lane": ("MIOPAL_FORCE_LANE_PER_PAIR", "MIOPAL_NO_HYBRID_TRACE"),
    "no_perpair": ("MIOPAL_NO_PERPAIR",),
    "no_packed_scan": ("MIOPAL_NO_PACKED_SCAN",),
    "no_packed_trace": ("MIOPAL_NO_PACKED_TRACE",),
    "no_profile": ("MIOPAL_NO_PERPAIR_PROFILE",),
    "host_traceback": ("MIOPAL_HOST_TRACEBACK",),
}


def database():
    rng = np.random.default_rng(7)
    return _data.random_db(rng, rng.integers(1, 350, size=700))


def query(qlen):
    return _data.random_protein(np.random.default_rng(100 + qlen), qlen)


def key_of(algo, matrix_name, qlen, switches):
    return f"{algo}/{matrix_name}/Q{qlen}/{switches}"


def run_cases(capi, db, algo, matrix_name, set_tuning):
    """(key, routing word, pair routing, search result, pair-list result, query) of every Q and set of switches;
    `set_tuning(name, value)` is miopalSetTuning (the `tuning` fixture's setenv, or _capi.set_tuning)."""
    matrix = MATRICES[matrix_name]
    pairs_q = np.zeros(700, dtype=np.int32)
    pairs_t = np.arange(700, dtype=np.int64)
    for qlen in QS:
        q = query(qlen)
        for name, switches in SWITCHES.items():
            for s in switches:
                set_tuning(s, "1")
            try:
                got = db.search(q, matrix, 3, 1, "full", algo)
                word = capi.DeviceDatabase.last_full_routing()
                listed = db.align_pairs([q], pairs_q, pairs_t, matrix, 3, 1, "full", algo)
                counts = list(capi.DeviceDatabase.last_pair_routing())
            finally:
                for s in switches:
                    set_tuning(s, None)
            yield key_of(algo, matrix_name, qlen, name), word, counts, got, listed, q


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def words():
    with open(FIXTURE) as f:
        return json.load(f)["words"]


@pytest.fixture(scope="module")
def targets():
    return database()


def test_the_fixture_holds_every_case(words):
    want = {key_of(a, m, q, s) for a in ALGOS for m in MATRICES for q in QS for s in SWITCHES}
    assert set(words) == want


@pytest.mark.parametrize("matrix_name", list(MATRICES))
@pytest.mark.parametrize("algo", ALGOS)
def test_routing_words_and_results(capi, tuning, words, targets, algo, matrix_name):
    res, off = targets
    refs = {}
    db = capi.DeviceDatabase(res, off, 24)
    try:
        def set_tuning(name, value):
            if value is None:
                tuning.delenv(name)
            else:
                tuning.setenv(name, value)

        for key, word, counts, got, listed, q in run_cases(capi, db, algo, matrix_name, set_tuning):
            assert word == words[key]["full"], (key, word, words[key]["full"])
            assert counts == words[key]["pairs"], (key, counts, words[key]["pairs"])
            if len(q) not in refs:
                refs[len(q)] = _oracle.search(q, res, off, MATRICES[matrix_name], 3, 1, "full", algo)
            compare(got, refs[len(q)], "full", key)
            compare(listed, refs[len(q)], "full", key + " (pair list)")
    finally:
        db.close()
