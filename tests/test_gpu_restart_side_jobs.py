"""A score pass that starts over when its side jobs are already on the side stream (host_search.inc, scorePassImpl).

Targets longer than the packed view takes (kLongTarget, 8192 residues) are forked to the side stream before the packed
launch. When that launch - here a multi-strip pair-table kernel - is refused (MIOPAL_TEST_REFUSE_PAIR_LAUNCH stands
for a runtime that refuses its dynamic LDS), the pass starts over on the general kernel: the side jobs must not be
enqueued twice, must still be joined, and are still counted, once. Every result bit for bit against the CPU checker."""
import numpy as np
import pytest

import _data
import _oracle
from pyopal_amd.matrices import ScoringMatrix

pytestmark = pytest.mark.gpu

B62 = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
STRIPS_KERNEL = {"sw": 2 + 4, "nw": 2 + 5}   # miopalLastRouting counts[1]: 2 + kPairSwStrips / kPairGlobalStrips
N_LONG = 3


@pytest.fixture(scope="module")
def capi():
    from pyopal_amd import _capi
    assert _capi.lib().miopalDeviceCount() >= 1, "no gfx950 device visible"
    return _capi


@pytest.fixture(scope="module")
def side_set(capi):
    # a query of three strips; 600 targets of 1 .. 300 residues (five groups of the packed view) and three of
    # 8200 .. 9000, which the view keeps out (longIds), relatives of the query among both
    rng = np.random.default_rng(130)
    query = _data.random_protein(rng, 130)
    seqs = [_data.random_protein(rng, int(k)) for k in rng.integers(1, 301, size=600)]
    seqs[17] = _data.mutate(rng, query, 0.1)
    for k in (8200, 8611, 9000):
        seq = _data.random_protein(rng, k)
        relative = _data.mutate(rng, query, 0.2)
        seq[4000:4000 + len(relative)] = relative
        seqs.insert(int(rng.integers(0, len(seqs))), seq)
    res, off = _oracle.flatten(seqs)
    db = capi.DeviceDatabase(res, off, 24)
    yield db, res, off, query
    db.close()


@pytest.mark.parametrize("mode", ["score", "end"])
@pytest.mark.parametrize("algo", ["sw", "nw"])
def test_refused_strips_launch_with_side_jobs_forked(capi, side_set, algo, mode):
    db, res, off, query = side_set
    want = _oracle.search_parallel(query, res, off, B62, 3, 1, mode, algo)

    def check(got, tag):
        for key in ("score", "end_t", "end_q"):
            if key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=f"{algo} {mode} {tag} {key}")

    # (Smith-Waterman would cut the long targets into windows, which stay in the packed view: MIOPAL_NO_SEGMENTS keeps them
    # whole, as NW targets always are, so that they leave for the side stream)
    switches = {"PAIR_STRIPS": "1", **({"NO_SEGMENTS": "1"} if algo == "sw" else {})}
    with capi.tuning(**switches):
        got = db.search(query, B62, 3, 1, mode, algo)
        routing = capi.DeviceDatabase.last_routing()
        assert routing[1] & 31 == STRIPS_KERNEL[algo], routing
        # (the packed groups hold at most 75 chunks, below the 128 chunks at which a group may leave for the side
        # kernel at all: the three long targets are all there is on the side)
        assert routing[0] == N_LONG, routing
        check(got, "strips")
        with capi.tuning(TEST_REFUSE_PAIR_LAUNCH="1"):
            got = db.search(query, B62, 3, 1, mode, algo)
            routing = capi.DeviceDatabase.last_routing()
            assert (routing[1] & 15) == 1, routing      # the general kernel took over
            # the long targets are still counted, and once: enqueued or counted again they would be 2 N_LONG
            assert N_LONG <= routing[0] < 2 * N_LONG, routing
            check(got, "refused")
