"""The three f32-row LayerNorm backward entry points (lstc_layernorm_bwd, lstc_layernorm_bwd_drop_pack, lstc_layernorm_bwd_drop)
give, call by call, the bits recorded in tests/golden/ln_bwd_bits.json (tools/record_ln_bwd_bits.py, run on the commit before the
one-wave-per-row kernel of the other vector widths was folded into the wave-pair kernel): dx, df and the pack at every width, the
partial planes at d = 512 / 1024 / 2048, and the return code of every refusal.  The calls are in tests/util_ln_bwd_bits.py."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_bwd_bits.json")
FAMILIES = ("bwd", "drop_pack", "drop", "rc")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def replayed():
    import util_ln_bwd_bits as U
    return U.all_digests()


def test_the_same_calls_are_replayed(recorded, replayed):
    assert sorted(recorded) == sorted(replayed)
    assert {k.split("/")[0] for k in recorded} == set(FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_bits_are_the_recorded_ones(recorded, replayed, family):
    keys = [k for k in recorded if k.split("/")[0] == family]
    assert keys
    moved = [k for k in keys if replayed.get(k) != recorded[k]]
    assert not moved, f"{len(moved)} of {len(keys)} results of {family} differ from the recorded ones: {moved[:8]}"
