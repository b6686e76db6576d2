"""The CLS concat (fixed / len / var layouts, pack, gather; forward and backward) and the f32 CLS passes give, call by call, the bits
recorded in tests/golden/cls_concat_bits.json (tools/record_cls_concat_bits.py, run on the commit before the three layouts were
folded into one kernel text each).  The calls and their shapes are in tests/util_cls_layouts.py."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cls_concat_bits.json")
FAMILIES = ("fwd", "bwd", "fwd_pack", "fwd_pack_only", "gather", "gather_pack", "gather_pack_only", "len_fwd", "len_bwd", "var_fwd",
            "var_bwd", "dot_fixed", "dot_len", "dot_var", "wsum_fixed", "wsum_var", "outer_fixed", "outer_var")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def replayed():
    import util_cls_layouts as U
    return U.all_digests()


def test_the_same_calls_are_replayed(recorded, replayed):
    assert sorted(recorded) == sorted(replayed)
    assert {k.split("/")[0] for k in recorded} == set(FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_bits_are_the_recorded_ones(recorded, replayed, family):
    keys = [k for k in recorded if k.split("/")[0] == family]
    assert keys
    moved = [k for k in keys if replayed.get(k) != recorded[k]]
    assert not moved, f"{len(moved)} of {len(keys)} calls of {family} give other bits than recorded: {moved[:8]}"
