"""The autograd nodes of the encoder blocks (MHAFunction, MHACrossFunction, MHAClsFunction, MHAClsAssocFunction, FFNFunction) do,
case by case, what tests/golden/block_calls.json and tests/golden/block_bits.json recorded (tools/record_block_bits.py, run on the
commit named in the fixtures' header: the one before the nodes were given one shared block shell): the same node, the same C entry
points in the same order with the weight gradients delivered at the same places, the same dropout sites, rates, seeds and shapes -
and the same bits in the output, the probabilities, the input gradients and every parameter gradient.  The cases are in
tests/util_block_bits.py.

block_calls.json is the contract of that refactor: what the host side of the blocks asks of the library, and in which order.  A
later change that moves kernel bits on purpose re-records block_bits.json with the tool (``--bits-only``) and leaves the traces
alone; one that changes the launches on purpose re-records both and says so."""
import json
import os

import pytest

import util_block_bits as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = sorted({k.split("/")[0] for k in U.CASES})


def _load(name, key):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)[key]


@pytest.fixture(scope="module")
def recorded():
    return _load("block_calls.json", "traces"), _load("block_bits.json", "digests")


@pytest.fixture(scope="module")
def replayed():
    return U.run_all()


def test_the_same_cases_are_replayed(recorded, replayed):
    assert sorted(recorded[0]) == sorted(replayed[0]) == sorted(U.CASES)
    assert sorted(recorded[1]) == sorted(replayed[1])


@pytest.mark.parametrize("family", FAMILIES)
def test_calls_deliveries_and_dropout_sites_are_the_recorded_ones(recorded, replayed, family):
    names = [k for k in U.CASES if k.split("/")[0] == family]
    assert names
    for name in names:
        want, got = recorded[0][name], json.loads(json.dumps(replayed[0][name]))
        assert got["node"] == want["node"] == U.CASES[name]["node"], name
        assert got["calls"] == want["calls"], name
        assert got["dropout"] == want["dropout"], name


@pytest.mark.parametrize("family", FAMILIES)
def test_bits_are_the_recorded_ones(recorded, replayed, family):
    keys = [k for k in recorded[1] if k.split("/")[0] == family]
    assert keys
    moved = [k for k in keys if replayed[1].get(k) != recorded[1][k]]
    assert not moved, f"{len(moved)} of {len(keys)} results of {family} differ from the recorded ones: {moved[:8]}"
