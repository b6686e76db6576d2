"""The cases behind tests/golden/block_calls.json and tests/golden/block_bits.json: every hand-written autograd node of the
encoder blocks (MHAFunction in its f32 and bf16-stream forms, MHACrossFunction, MHAClsFunction, MHAClsAssocFunction, FFNFunction),
driven through models.MultiHeadAttention / models.FFN on the smallest shapes that reach each of their arms.

A case runs under ``torch.manual_seed(SEED)`` and ``Fn.reset_rng(0)``, builds its module and inputs from the CPU generator, runs the
forward and the backward of a weighted sum, and leaves
  a trace   the autograd node that ran, the ordered C entry points with ``deliver:<weight>`` markers where a weight gradient was
            handed over, and the ``record_dropout()`` list (site, p, seed, shape);
  digests   SHA-256 of the raw bytes of the output, the returned probabilities, the input gradient(s) and every parameter gradient.
tools/record_block_bits.py writes both into the fixtures; tests/test_block_bits_gpu.py replays and compares;
tests/test_block_bits_host.py holds the table itself to the arms it names.  The table and ``predicates`` need no device."""
import hashlib

import torch

SEED = 20251020
DEV = "cuda"
NODES = ("MHAFunction", "MHACrossFunction", "MHAClsFunction", "MHAClsAssocFunction", "FFNFunction")
LENGTHS = (1, 16, 33)          # patch tokens per sequence of the unpadded cases


def _mha(mode, arm, **kw):
    base = dict(node="MHAFunction", kind="mha", mode=mode, arm=arm, N=3, S=17, dm=64, H=2, dk=32, dv=32, fuse=False, bias=False, ln=True,
                p_attn=0.0, p_fc=0.0, mask=False, seqs=False, act=False, act16_out=False)
    base.update(kw)
    return base


def _ffn(mode, arm, **kw):
    base = dict(node="FFNFunction", kind="ffn", mode=mode, arm=arm, N=3, S=17, dm=64, F=256, ln=True, p=0.0, act=False, act16_out=False)
    base.update(kw)
    return base


def _cross(arm, **kw):
    base = dict(node="MHACrossFunction", kind="cross", mode="fp32", arm=arm, N=3, Sq=17, Sk=17, dm=64, H=2, dk=32, dv=16, fuse=False,
                bias=False, ln=True, p_attn=0.0, p_fc=0.0, mask=False, same_kv=False)
    base.update(kw)
    return base


def _cls(node, mode, arm, **kw):
    base = dict(node=node, kind="cls", mode=mode, arm=arm, N=3, S=17, dm=64, H=2, dk=32, dv=32, bias=True, ln=True, p_attn=0.0, p_fc=0.0,
                mask=False, lengths=False, seqs=False, act=False, assoc=node == "MHAClsAssocFunction")
    base.update(kw)
    return base


_BF = dict(N=16, S=16)          # M = N * S = 256: one tile row of the packed bf16 kernels

CASES = {
    # ---- MHAFunction, exact f32, d_model = 64, H = 2
    "mha/fp32/separate_dk32_dv16": _mha("fp32", "separate", dv=16),
    "mha/fp32/fused_bias_drop_S49": _mha("fp32", "fused", N=2, S=49, fuse=True, bias=True, p_attn=0.1, p_fc=0.2),
    "mha/fp32/fused_keymask_no_ln": _mha("fp32", "masked", fuse=True, mask=True, ln=False),
    "mha/fp32/unpadded_fused": _mha("fp32", "unpadded_fused", fuse=True, bias=True, p_attn=0.1, p_fc=0.2, seqs=True),
    "mha/fp32/unpadded_separate": _mha("fp32", "unpadded_separate", bias=True, p_attn=0.1, p_fc=0.2, seqs=True),
    "mha/fp32/dedup_fused": dict(node="MHAFunction", kind="dedup", mode="fp32", arm="dedup_fused", fuse=True),
    "mha/fp32/dedup_separate": dict(node="MHAFunction", kind="dedup", mode="fp32", arm="dedup_separate", fuse=False),
    # ---- f32x3 with thresholds 0: the maybe_pack arms
    "mha/f32x3/fused": _mha("f32x3", "maybe_pack", N=8, S=16, dm=128, dk=64, dv=64, fuse=True, bias=True, p_attn=0.1, p_fc=0.2),
    "ffn/f32x3/F256": _ffn("f32x3", "maybe_pack", N=8, S=16, dm=128, F=256, p=0.1),
    # ---- bf16 with thresholds 0, M = 256
    "mha/bf16/packed_qkv": _mha("bf16", "packed_qkv", dm=256, H=4, dk=64, dv=64, fuse=True, bias=True, p_attn=0.1, p_fc=0.2, **_BF),
    "mha/bf16/packed_o_fused_bwd": _mha("bf16", "packed_o_fused_bwd", dm=256, H=8, dk=32, dv=32, fuse=True, bias=True, p_attn=0.1, **_BF),
    "mha/bf16/packed_o_split_bwd": _mha("bf16", "packed_o_split_bwd", dm=256, H=8, dk=32, dv=32, bias=True, p_fc=0.2, **_BF),
    "mha/bf16/act_out16": _mha("bf16", "act", dm=1024, H=4, dk=64, dv=64, fuse=True, bias=True, p_attn=0.1, p_fc=0.2, act=True,
                               act16_out=True, **_BF),
    "mha/bf16/act_out32": _mha("bf16", "act", dm=1024, H=4, dk=64, dv=64, fuse=True, bias=True, p_attn=0.1, p_fc=0.2, act=True, **_BF),
    # ---- FFNFunction
    "ffn/fp32/F256": _ffn("fp32", "aligned", p=0.1),
    "ffn/fp32/F250_padded_256": _ffn("fp32", "padded_256", F=250, p=0.1),
    "ffn/fp32/F30_padded_32": _ffn("fp32", "padded_32", F=30),
    "ffn/fp32/no_ln_drop": _ffn("fp32", "no_ln", ln=False, p=0.2),
    "ffn/bf16/packed_hidden": _ffn("bf16", "packed_hidden", dm=256, F=512, p=0.1, **_BF),
    "ffn/bf16/act": _ffn("bf16", "act", dm=1024, F=1024, p=0.1, act=True, act16_out=True, **_BF),
    # ---- MHACrossFunction
    "cross/square_bias": _cross("square", bias=True, p_attn=0.1, p_fc=0.2),
    "cross/rect_mask": _cross("rect", Sq=5, mask=True, p_attn=0.1),
    "cross/same_kv_adjacent": _cross("same_kv_fused", Sq=5, fuse=True, same_kv=True, p_fc=0.2),
    "cross/same_kv_separate": _cross("same_kv_separate", Sq=5, same_kv=True),
    # ---- MHAClsFunction: d_model = 512, the width at which layernorm_bwd_branch would take lstc_layernorm_bwd_drop
    "cls/kv_mask_drop_d512": _cls("MHAClsFunction", "fp32", "kv_masked", dm=512, mask=True, p_attn=0.2, p_fc=0.2),
    # ---- MHAClsAssocFunction
    "cls/assoc_plain": _cls("MHAClsAssocFunction", "fp32", "assoc_plain", p_attn=0.1, p_fc=0.2),
    "cls/assoc_key_lengths": _cls("MHAClsAssocFunction", "fp32", "assoc_len", lengths=True),
    "cls/assoc_unpadded": _cls("MHAClsAssocFunction", "fp32", "assoc_var", seqs=True, p_attn=0.1, p_fc=0.2, dm=512),
    "cls/assoc_pack": _cls("MHAClsAssocFunction", "bf16", "assoc_pack", dm=1024, H=4, dk=64, dv=64, act=True, p_attn=0.1, p_fc=0.2, **_BF),
}


class mode:
    """``with mode(case):`` - the compute mode of a case with the packed kernels' size thresholds at zero."""

    def __init__(self, case):
        self.name = case["mode"]

    def __enter__(self):
        from lstc_vad_amd import functional as Fn
        Fn.set_compute_dtype(self.name)
        if self.name != "fp32":
            Fn.set_x3_threshold(0, 0, 0)

    def __exit__(self, *exc):
        from lstc_vad_amd import functional as Fn
        Fn.set_compute_dtype("fp32")
        Fn.set_x3_threshold()
        return False


def predicates(c):
    """The pure-Python routing predicates of a case, evaluated in its mode: what the node bodies consult to choose an arm."""
    from lstc_vad_amd import functional as Fn
    with mode(c):
        if c["kind"] == "ffn":
            M, Fp = c["N"] * c["S"], Fn._padded_hidden(c["F"])
            return dict(padded_hidden=Fp, hidden_pack=Fn.packed_out_shape(M, Fp), out_pack=Fn.packed_out_shape(M, c["dm"]),
                        act_rows=Fn.act_rows_ok(M, c["dm"]))
        if c["kind"] == "mha":
            N, S, H, dk, dv = c["N"], c["S"], c["H"], c["dk"], c["dv"]
            return dict(packed_inputs=Fn.attn_packed_inputs(N, S, H, dk, dv), fwd_pack=Fn.attn_fwd_pack(N, S, H, dv),
                        bwd_packs=Fn.attn_bwd_packs(N, S, H, dk, dv), qkv_pack=Fn.packed_out_shape(N * S, H * (2 * dk + dv)),
                        o_pack=Fn.packed_out_shape(N * S, H * dv), act_rows=Fn.act_rows_ok(N * S, c["dm"]))
        if c["kind"] == "cls":
            return dict(cls_pack=Fn.cls_pack_ok(c["N"], c["S"], c["H"], c["dm"]))
    return {}


# ------------------------------------------------------------------------------------------------------ running a case
def digest(t, tile=None):
    """SHA-256 of a tensor's bytes; of a bf16 pack view, of its tile area (``tile`` bytes: lstc_pack1_bytes allots more than
    the kernels write)."""
    if t is None:
        return "none"
    torch.cuda.synchronize()
    raw = t.detach().contiguous().view(-1).view(torch.uint8)
    if t.dtype == torch.bfloat16:
        raw = raw[:tile]
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _leaf(g, *shape):
    return _randn(g, *shape).requires_grad_(True)


def _pack_leaf(g, N, S, dm):
    """A bf16-stream input with a gradient: the bf16 view of the lstc_pack1 buffer of seeded [N * S, d] rows."""
    from lstc_vad_amd import _lib, functional as Fn
    t = Fn._act_tensor(Fn.pack3(_randn(g, N * S, dm), kind=_lib.BF16P)).detach().requires_grad_(True)
    return t, Fn.PackedAct(t, (N, S, dm))


def _attention(c):
    from lstc_vad_amd.models import MultiHeadAttention
    m = MultiHeadAttention(c["H"], c["dm"], c["dk"], c["dv"], layerNorm=c["ln"], attn_dropout=c["p_attn"], fc_dropout=c["p_fc"],
                           relative_pe=c["bias"], window_size=4, window_depth=3).to(DEV).train()
    m._site = "blk."
    if c.get("fuse"):
        m.fuse_qkv_()
    return m


def _build_mha(c, g):
    from lstc_vad_amd import functional as Fn
    m = _attention(c)
    N, S, dm = c["N"], c["S"], c["dm"]
    if c["seqs"]:
        lay = Fn.unpadded_layout(list(LENGTHS))
        x = _leaf(g, 1, lay.M, dm)
        return m, [x], lambda: m(x, x, x, seqs=lay)
    if c["act"]:
        m._act16_out = c["act16_out"]
        t, x = _pack_leaf(g, N, S, dm)
        return m, [t], lambda: m(x, x, x, return_attn=True)
    x = _leaf(g, N, S, dm)
    mask = None
    if c["mask"]:
        mask = (torch.arange(S)[None, :] < torch.tensor([S, S - 5, 2])[:N, None]).view(N, 1, 1, S)
    return m, [x], lambda: m(x, x, x, mask=mask, return_attn=True)


def _build_dedup(c, g):
    """Layer 0 of the encoder of tests/test_dedup_rows_gpu.py on its batch of four 10-clip videos: the input is the fused gather's."""
    import test_dedup_rows_gpu as DR
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.feed import ResidentBank
    enc = DR._encoder(c["fuse"])
    idx, clips = DR._windows([[10] * DR.BS, [10] * DR.BS])
    bank = DR._bank(clips)
    (nf, _), = ResidentBank(bank).gather(idx, lazy=True)
    x = enc._embed((bank, nf.idx_flat, idx.size // DR.L, DR.L, nf))
    assert Fn._dedup_rows, "the fused gather left no DedupRows: the case would run the ordinary projections"
    m = enc.layer_stack[0].slf_attn
    return m, [], lambda: m(x, x, x, return_attn=True)


def _build_cross(c, g):
    m = _attention(dict(c, bias=c["bias"]))
    N, Sq, Sk, dm = c["N"], c["Sq"], c["Sk"], c["dm"]
    q, k = _leaf(g, N, Sq, dm), _leaf(g, N, Sk, dm)
    v = k if c["same_kv"] else _leaf(g, N, Sk, dm)
    mask = None
    if c["mask"]:
        mask = (torch.rand(N, 1, Sq, Sk, generator=g) > 0.3)
        mask[..., 0] = True
    return m, [q, k] + ([] if c["same_kv"] else [v]), lambda: m.forward_cross(q, k, v, mask=mask, return_attn=True)


def _build_cls(c, g):
    from lstc_vad_amd import functional as Fn
    m = _attention(c)
    m.cls_assoc = c["assoc"]
    N, S, dm = c["N"], c["S"], c["dm"]
    if c["seqs"]:
        lay = Fn.unpadded_layout(list(LENGTHS))
        x = _leaf(g, 1, lay.M, dm)
        return m, [x], lambda: (m.forward_cls(x, seqs=lay), None)
    if c["act"]:
        t, x = _pack_leaf(g, N, S, dm)
        return m, [t], lambda: (m.forward_cls(x), None)
    x = _leaf(g, N, S, dm)
    mask = (torch.rand(N, 1, S, S, generator=g) > 0.3) if c["mask"] else None
    if mask is not None:
        mask[..., 0] = True
    klen = torch.tensor([S, 9, 1][:N], dtype=torch.int32, device=DEV) if c["lengths"] else None
    return m, [x], lambda: (m.forward_cls(x, mask=mask, key_lengths=klen), None)


def _build_ffn(c, g):
    from lstc_vad_amd.models.FFN import PositionwiseFeedForward
    m = PositionwiseFeedForward(c["dm"], c["F"], dropout=c["p"], layerNorm=c["ln"]).to(DEV).train()
    m._site = "blk."
    N, S, dm = c["N"], c["S"], c["dm"]
    if c["act"]:
        m._act16_out = c["act16_out"]
        t, x = _pack_leaf(g, N, S, dm)
        return m, [t], lambda: (m(x), None)
    x = _leaf(g, N, S, dm)
    return m, [x], lambda: (m(x), None)


_BUILD = dict(mha=_build_mha, dedup=_build_dedup, cross=_build_cross, cls=_build_cls, ffn=_build_ffn)


def run_case(name):
    """-> (trace, digests) of one case on the loaded library."""
    from lstc_vad_amd import _lib as L, functional as Fn
    from util import _LibSpy
    c = CASES[name]
    real_load, real_deliver = L.load, Fn.deliver
    with mode(c):
        try:
            torch.manual_seed(SEED)
            Fn.reset_rng(0)
            Fn.drop_producer_packs()
            g = torch.Generator().manual_seed(SEED)
            module, leaves, call = _BUILD[c["kind"]](c, g)
            names = {id(p): k for k, p in module.named_parameters()}
            spy = _LibSpy(real_load())

            def deliver(w, grad):
                spy.calls.append("deliver:" + names[id(w)])
                return real_deliver(w, grad)
            L.load, Fn.deliver = (lambda: spy), deliver
            with Fn.record_dropout() as notes:
                out, probs = call()[:2]
                t = out.t if isinstance(out, Fn.PackedAct) else out
                wgt = _randn(g, *t.shape)
                (t.float() * wgt).sum().backward()
            torch.cuda.synchronize()
        finally:
            L.load, Fn.deliver = real_load, real_deliver
            Fn.drop_producer_packs()
    trace = dict(node=type(t.grad_fn).__name__.replace("Backward", ""), calls=list(spy.calls),
                 dropout=[[site, p, seed, list(shape)] for site, p, seed, shape in notes])
    tile = c["N"] * c["S"] * c["dm"] * 2 if c.get("act") else None
    bits = {"out": digest(t, tile), "probs": digest(probs)}
    for i, x in enumerate(leaves):
        bits[f"dx{i}"] = digest(x.grad, tile)
    for k, p in module.named_parameters():
        bits["d/" + k] = digest(p.grad)
    return trace, {f"{name}:{k}": v for k, v in bits.items()}


def run_all():
    """-> ({case: trace}, {case:result: sha256}) over the whole table."""
    traces, digests = {}, {}
    for name in CASES:
        traces[name], bits = run_case(name)
        digests.update(bits)
    return traces, digests
