"""The case table of tests/util_block_bits.py, held to what it says without a device: the two fixtures carry exactly its keys, every
node class and every arm of the blocks is there, and where an arm is chosen by a pure-Python predicate (attn_packed_inputs,
attn_fwd_pack, attn_bwd_packs, _padded_hidden, packed_out_shape, act_rows_ok, cls_pack_ok) the predicate gives the arm the case is
named for at the case's shape - so a case cannot quietly record some other arm."""
import json
import os

import pytest

import util_block_bits as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARMS = {
    "MHAFunction": {"separate", "fused", "masked", "unpadded_fused", "unpadded_separate", "dedup_fused", "dedup_separate", "maybe_pack",
                    "packed_qkv", "packed_o_fused_bwd", "packed_o_split_bwd", "act"},
    "FFNFunction": {"aligned", "padded_256", "padded_32", "no_ln", "maybe_pack", "packed_hidden", "act"},
    "MHACrossFunction": {"square", "rect", "same_kv_fused", "same_kv_separate"},
    "MHAClsFunction": {"kv_masked"},
    "MHAClsAssocFunction": {"assoc_plain", "assoc_len", "assoc_var", "assoc_pack"},
}


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_fixtures_hold_exactly_the_table():
    calls, bits = _load("block_calls.json"), _load("block_bits.json")
    assert sorted(calls["traces"]) == sorted(U.CASES)
    assert {k.split(":")[0] for k in bits["digests"]} == set(U.CASES)
    assert calls["commit"] == bits["commit"] and len(bits["commit"]) >= 7 and calls["seed"] == bits["seed"] == U.SEED
    for name, trace in calls["traces"].items():
        assert trace["node"] == U.CASES[name]["node"], name
        assert trace["calls"] and any(c.startswith("deliver:") for c in trace["calls"]), name
        for what in ["out", "probs"] + ([] if U.CASES[name]["kind"] == "dedup" else ["dx0"]):
            assert f"{name}:{what}" in bits["digests"], (name, what)
    for name in ("block_calls.json", "block_bits.json"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20


def test_every_node_and_arm_is_in_the_table():
    assert {c["node"] for c in U.CASES.values()} == set(U.NODES) == set(ARMS)
    for node, arms in ARMS.items():
        assert {c["arm"] for c in U.CASES.values() if c["node"] == node} == arms, node
    cls = [c for c in U.CASES.values() if c["node"] == "MHAClsAssocFunction"]
    assert sum(c["p_attn"] > 0 and c["p_fc"] > 0 for c in cls) >= 2
    assert {c["act16_out"] for c in U.CASES.values() if c["arm"] == "act" and c["kind"] == "mha"} == {True, False}
    kv = next(c for c in U.CASES.values() if c["node"] == "MHAClsFunction")
    assert kv["dm"] in (512, 1024, 2048) and kv["p_fc"] > 0 and kv["ln"]      # where layernorm_bwd_branch would fuse the dropout replay


def test_dropout_sites_recorded_follow_the_rates():
    """Two draws per attention block with both rates on, attention first; none with both off."""
    traces = _load("block_calls.json")["traces"]
    for name, c in U.CASES.items():
        sites = [s[0] for s in traces[name]["dropout"]]
        if c["kind"] == "ffn":
            assert sites == (["blk.dropout"] if c["p"] > 0 else []), name
        elif c["kind"] != "dedup":
            tag = "#cls" if c["kind"] == "cls" else ""
            want = (["blk.attn_dropout" + tag] if c["p_attn"] > 0 else []) + (["blk.dropout" + tag] if c["p_fc"] > 0 else [])
            assert sites == want, name
            seeds = [s[2] for s in traces[name]["dropout"]]
            assert all((b - a) % (1 << 64) == 1 for a, b in zip(seeds, seeds[1:])), name      # next_seed() is linear in its counter


@pytest.mark.parametrize("name", [k for k, c in U.CASES.items() if c["kind"] in ("mha", "ffn", "cls")])
def test_predicates_give_the_arm_the_case_is_named_for(name):
    c, p = U.CASES[name], U.predicates(U.CASES[name])
    arm = c["arm"]
    if c["kind"] == "mha":
        want = {"packed_qkv": dict(packed_inputs=True, qkv_pack=True, o_pack=True),
                "act": dict(packed_inputs=True, qkv_pack=True, o_pack=True, act_rows=True),
                "packed_o_fused_bwd": dict(packed_inputs=False, fwd_pack=True, bwd_packs=True),
                "packed_o_split_bwd": dict(packed_inputs=False, fwd_pack=True, bwd_packs=True)}.get(
                    arm, dict(packed_inputs=False, fwd_pack=False, bwd_packs=False, act_rows=False))
        assert c["fuse"] == (arm not in ("separate", "unpadded_separate", "packed_o_split_bwd")), name
    elif c["kind"] == "ffn":
        want = {"aligned": dict(padded_hidden=256, hidden_pack=False), "padded_256": dict(padded_hidden=256, hidden_pack=False),
                "padded_32": dict(padded_hidden=32, hidden_pack=False), "no_ln": dict(padded_hidden=c["F"], hidden_pack=False),
                "maybe_pack": dict(padded_hidden=c["F"], hidden_pack=False),
                "packed_hidden": dict(padded_hidden=c["F"], hidden_pack=True, act_rows=False),
                "act": dict(padded_hidden=c["F"], hidden_pack=True, out_pack=True, act_rows=True)}[arm]
        assert (c["F"] != want["padded_hidden"]) == arm.startswith("padded_"), name
    else:
        want = dict(cls_pack=arm == "assoc_pack")
    assert {k: p[k] for k in want} == want, (name, p)
