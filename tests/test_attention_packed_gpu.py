"""The packed-operand bf16 attention kernels (csrc/attention_pk.hip attn_fwd3_kernel / attn_bwd3_kernel, reached through
LstcAttnDesc.in_pack_cols > 0) against a float64 model of the contract with the kernels' rounding points
(tests/util_attn_packed.py, whose docstring states the model and the bars), arm by arm of what fill_packed_inputs / attn_bwd
(csrc/attention.hip) accept.  tests/test_attn_packed_ref_host.py is the CPU twin: the model without roundings is the contract,
an f32 evaluation of it stays under half of every bar, six kinds of wrong kernel land past four.

The backward is pinned independently of the forward: it runs on a P the test writes (the f32 of the f64 softmax, zeros in the
padding columns); one case per tile count also feeds it the forward's own probabilities under the same bars.

M = N S must be a multiple of 256: N = 256 for odd S, the smallest valid N for even S.  H = 4, d_k = d_v = 64, dropout 0.2
replayed through functional.dropout_mask and the models' own (sliced) index unless a test says otherwise.  The worst error of
every section against its bar is in profiles/attention_packed_errors.txt (written when LSTC_ATTN_PACKED_ERRORS names a file)."""
import functools
import types

import pytest
import torch

import util_attn_packed as A
from util_attn_short import _Hooks

pytestmark = pytest.mark.gpu

DEV = "cuda"
EVEN_N = {2: 128, 16: 16, 32: 8, 34: 128, 48: 16, 64: 4, 66: 128, 80: 16, 96: 8}


def _build(S, H=4, dk=64, dv=64, p_drop=A.P_DROP, bias=True, table_rows=None):
    """Inputs, packs, keep mask, the f64 model (forward; backward on the written P) of one shape."""
    c = types.SimpleNamespace(S=S, H=H, dk=dk, dv=dv, p_drop=p_drop, N=256 if S % 2 else EVEN_N[S], seed=500 + S)
    c.M = c.N * S
    assert c.M % 256 == 0
    c.q, c.k, c.v, c.do, c.table, c.index = A.inputs(c.N, S, H, dk, dv, seed=7 * S + dk + 3 * dv + H, table_rows=table_rows)
    if not bias:
        c.table = c.index = None
    c.keep = A.keep_mask(c.N, H, S, c.seed, p_drop)
    c.shape = (c.N, S, H, dk, dv)
    c.bias = (c.table, c.index)
    c.p64, c.o, c.bo = A.model_fwd(c.q, c.k, c.v, *c.shape, *c.bias, c.keep, p_drop)
    c.pbuf, c.pview = A.written_probs(c.p64)
    c.dq, c.dk_, c.dv_, c.dt = A.model_bwd(c.do, c.q, c.k, c.v, c.pview, *c.shape, *c.bias, c.keep, p_drop)
    c.qkv, c.dop = A.pack(torch.cat([c.q, c.k, c.v], 1)), A.pack(c.do)
    c.fused = H * (2 * dk + dv)
    return c


_case = functools.lru_cache(maxsize=None)(_build)       # H = 4, d = 64 shapes, shared by the sections; never written afterwards


def _check_fwd(section, c, probs, o_pack, case):
    A.check_probs(section, probs[..., : c.S], c.p64, case)
    A.check_out(section, "O", A.unpack(o_pack, c.M, c.H * c.dv), c.o, c.bo, c.S, case)


def _split(c, g):
    a, b = c.H * c.dk, 2 * c.H * c.dk
    return g[:, :a], g[:, a:b], g[:, b:]


def _check_bwd(section, c, fused_pack, dtable, case):
    for name, got, (ref, bound) in zip(A.OUTS[1:], _split(c, A.unpack(fused_pack, c.M, c.fused)), (c.dq, c.dk_, c.dv_)):
        A.check_out(section, name, got, ref, bound, c.S, case)
    if c.table is not None and dtable is not None:
        A.check_table(section, dtable, c.dt, case)


def _raw(c, **kw):
    return A.raw_fwd3(c.qkv, *c.shape, *c.bias, c.seed, p_drop=c.p_drop, **kw)


def _raw_bwd(c, probs=None, do=None, qkv=None, **kw):
    return A.raw_bwd3(c.dop if do is None else do, c.qkv if qkv is None else qkv, c.pbuf if probs is None else probs,
                      *c.shape, *c.bias, c.seed, p_drop=c.p_drop, **kw)


# ------------------------------------------------------------------------------------- 1. sequence lengths

SWEEP_S = [1, 2, 3, 16, 17, 31, 32, 33, 34, 48, 49, 63, 64, 65, 66, 80, 81, 95, 96]


def _functional(c, own_probs):
    """functional.attn_fwd / attn_bwd on the fused packs, as the bf16-mode autograd nodes call them."""
    F = A.Fn()
    kind = A.L().BF16P
    qkv, dop = F.Packed(c.qkv, c.M, c.fused, kind), F.Packed(c.dop, c.M, c.H * c.dv, kind)
    with _Hooks(0, "bf16"):
        o, probs = F.attn_fwd(qkv, None, None, *c.shape, *c.bias, c.p_drop, c.seed)
        assert probs.shape == c.p64.shape and probs.stride(2) == (c.S + 3) // 4 * 4
        g = F.attn_bwd(dop, qkv, None, None, c.pview, *c.shape, *c.bias, c.p_drop, c.seed)
        g_own = F.attn_bwd(dop, qkv, None, None, probs, *c.shape, *c.bias, c.p_drop, c.seed) if own_probs else None
        torch.cuda.synchronize()
    return o, probs, g, g_own


@pytest.mark.parametrize("S", SWEEP_S)
def test_sequence_length_sweep(S):
    """Every S at which the kernels change their tile count or the tail of a tile (T = 1, 2, 3; one row, one key past a tile
    edge, the last row of a tile), fused layout through functional.attn_fwd / attn_bwd, dropout 0.2, sliced model index.  At
    S = 17, 49, 81 the backward also runs on the forward's own probabilities."""
    c = _case(S)
    o, probs, g, g_own = _functional(c, own_probs=S in (17, 49, 81))
    _check_fwd("1 sweep fwd", c, probs, o.buf, (S,))
    _check_bwd("1 sweep bwd", c, g[0].buf, g[3], (S,))
    if S == 1:      # no (i, j) pair carries a bias
        assert float(g[3].abs().max()) == 0.0
    if g_own is not None:
        _check_bwd("1 sweep bwd on the forward's P", c, g_own[0].buf, g_own[3], (S,))


@pytest.mark.parametrize("S", [17, 49, 81])
def test_sequence_lengths_without_dropout_and_table(S):
    c = _build(S, p_drop=0.0, bias=False)
    o, probs, g, g_own = _functional(c, own_probs=True)
    assert g[3] is None
    _check_fwd("1 no dropout, no table fwd", c, probs, o.buf, (S,))
    _check_bwd("1 no dropout, no table bwd", c, g[0].buf, None, (S,))
    _check_bwd("1 no dropout, no table bwd own P", c, g_own[0].buf, None, (S,))


# ------------------------------------------------------------------------------------- 2. widths and heads

@pytest.mark.parametrize("dk,dv", [(64, 128), (128, 64), (64, 256), (256, 64), (192, 192), (256, 256)])
@pytest.mark.parametrize("S", [17, 49, 81])
def test_head_widths(S, dk, dv):
    """d_k != d_v both ways (the ring carries d_k / 32 logit units and d_v / 64 output units forward; d_v / 32, d_k / 64, d_v / 64,
    d_k / 64 units backward), two to eight tiles per head, H = 2, through the raw descriptor (functional's predicates ask for
    H d_v >= 256).  d_k = 128, 192: 1 / sqrt(d_k) is no power of two - the kernel multiplies the f32 logits by the f32 scale."""
    c = _build(S, H=2, dk=dk, dv=dv)
    probs, o = _raw(c)
    _check_fwd("2 widths fwd", c, probs, o, (S, dk, dv))
    (g,), dt = _raw_bwd(c)
    _check_bwd("2 widths bwd", c, g, dt, (S, dk, dv))


@pytest.mark.parametrize("H", [1, 3, 8])
def test_head_counts(H):
    c = _build(49, H=H)
    probs, o = _raw(c)
    _check_fwd("2 heads fwd", c, probs, o, (49, H))
    (g,), dt = _raw_bwd(c)
    _check_bwd("2 heads bwd", c, g, dt, (49, H))


@pytest.mark.parametrize("dk", [32, 96])
@pytest.mark.parametrize("S", [17, 49, 81])
def test_forward_at_key_widths_the_backward_refuses(S, dk):
    """The forward takes d_k % 32 == 0 (one and three logit units), the backward d_k % 64 == 0 only: LSTC_E_UNSUPPORTED."""
    c = _build(S, H=2, dk=dk, dv=64)
    probs, o = _raw(c)
    _check_fwd("2 forward only", c, probs, o, (S, dk))
    with pytest.raises(RuntimeError, match=r"code -4"):
        _raw_bwd(c)


# ------------------------------------------------------------------------------------- 3. operand placement

@functools.lru_cache(maxsize=None)
def _fused_run(S):
    """The raw fused call of the default shape: (P buffer, O pack, dQ | dK | dV pack, dtable), held to the bars once here."""
    c = _case(S)
    probs, o = _raw(c)
    _check_fwd("3 placement: fused raw call", c, probs, o, (S,))
    (g,), dt = _raw_bwd(c)
    _check_bwd("3 placement: fused raw call", c, g, dt, (S,))
    return probs, o, g, dt


def _widened(t, at, cols, seed):
    """[M, cols] of noise with ``t`` in the columns from ``at`` on (bf16-representable, as everything a pack holds)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(t.shape[0], cols, device=DEV, generator=g).bfloat16().float()
    w[:, at: at + t.shape[1]] = t
    return w


@pytest.mark.parametrize("kind", ["separate_inputs", "wide_inputs", "wide_dO", "separate_outputs", "wide_outputs", "probs_ld"])
@pytest.mark.parametrize("S", [17, 81])
def test_operand_placement(S, kind):
    """The arms of the C ABI that functional.py never takes, each bit for bit the fused call of the same operands:
    separate_inputs   three packs of H d columns, Q_col0 = K_col0 = V_col0 = 0;
    wide_inputs       one pack 64 columns wider, the blocks at columns 32, 288, 544 (odd multiples of 32), noise around them;
    wide_dO           a dO pack of H d_v + 64 columns, dO_col0 = 32;
    separate_outputs  pack_cols = 0: three output packs, the column blocks of the fused output;
    wide_outputs      an output pack 64 columns wider, pre-filled with a bf16 pattern: the blocks at 32, 288, 544 hold the fused
                      output's values, every other column keeps the pattern;
    probs_ld          pitch 32 T against S rounded up to 4: the same P and O bits, zeros in [S, probs_ld), and a backward on the
                      written P at either pitch gives the same bits."""
    c = _case(S)
    probs0, o0, g0, dt0 = _fused_run(S)
    Hd, M = c.H * c.dk, c.M
    blocks = (32, 32 + Hd, 32 + 2 * Hd)
    assert all((b // 32) % 2 == 1 for b in blocks)
    if kind in ("separate_inputs", "wide_inputs"):
        if kind == "separate_inputs":
            kw = dict(qkv=tuple(A.pack(t) for t in (c.q, c.k, c.v)), in_cols=Hd, col0=(0, 0, 0))
        else:
            wide = torch.randn(M, 3 * Hd + 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(S)).bfloat16().float()
            for b, t in zip(blocks, (c.q, c.k, c.v)):
                wide[:, b: b + Hd] = t
            kw = dict(qkv=A.pack(wide), in_cols=3 * Hd + 64, col0=blocks)
        probs, o = A.raw_fwd3(kw["qkv"], *c.shape, *c.bias, c.seed, in_cols=kw["in_cols"], col0=kw["col0"])
        assert A.same_bits(probs, probs0) and torch.equal(o, o0)
        (g,), dt = _raw_bwd(c, **kw)
        assert torch.equal(g, g0) and torch.equal(dt, dt0)
    elif kind == "wide_dO":
        (g,), dt = _raw_bwd(c, do=A.pack(_widened(c.do, 32, c.H * c.dv + 64, S)), do_cols=c.H * c.dv + 64, do0=32)
        assert torch.equal(g, g0) and torch.equal(dt, dt0)
    elif kind == "separate_outputs":
        outs, dt = _raw_bwd(c, pack_cols=0)
        assert len(outs) == 3 and torch.equal(dt, dt0)
        for name, got, want in zip(A.OUTS[1:], outs, _split(c, A.unpack(g0, M, c.fused))):
            assert A.same_bits(A.unpack(got, M, Hd), want.contiguous()), name
    elif kind == "wide_outputs":
        cols = c.fused + 64
        pattern = (torch.arange(M * cols, device=DEV) % 251).float().view(M, cols) - 125.0        # integers: exact in bf16
        out = A.pack(pattern)
        (g,), dt = _raw_bwd(c, pack_cols=cols, out_col0=blocks, out=out)
        assert g is out and torch.equal(dt, dt0)
        got, want = A.unpack(g, M, cols), A.unpack(g0, M, c.fused)
        assert A.same_bits(got[:, :32].contiguous(), pattern[:, :32].contiguous())
        assert A.same_bits(got[:, 32 + 3 * Hd:].contiguous(), pattern[:, 32 + 3 * Hd:].contiguous())
        assert A.same_bits(got[:, 32: 32 + 3 * Hd].contiguous(), want)
    else:
        T = -(-S // 32)
        assert probs0.shape[3] == (S + 3) // 4 * 4 < 32 * T
        probs, o = _raw(c, probs_ld=32 * T)
        assert probs.shape[3] == 32 * T
        assert A.same_bits(probs[..., :S].contiguous(), probs0[..., :S].contiguous()) and torch.equal(o, o0)
        for buf in (probs, probs0):      # raw_fwd3 hands the kernel a buffer of NaN
            assert float(buf[..., S:].abs().max()) == 0.0
        (g,), dt = _raw_bwd(c, probs=A.written_probs(c.p64, 32 * T)[0])
        assert torch.equal(g, g0) and torch.equal(dt, dt0)


# ------------------------------------------------------------------------------------- 4. sequences per workgroup

@functools.lru_cache(maxsize=None)
def _npw_run(S, n, rerun=False):
    c = _case(S)
    probs, o = _raw(c, variant=100 + n)
    (g,), dt = _raw_bwd(c, chunks=A.chunks_for(c.N, n))
    return probs, o, g, dt


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("S", [17, 49, 81])
def test_sequences_per_workgroup(S, n):
    """A workgroup walks n sequences - forward LstcAttnDesc.variant = 100 + n, backward dtable_chunks = ceil(256 / n) - and its
    ring of staged units runs across them: the producer's tail waits, slots that change sequence mid-ring and, at n = 3 and 5, a
    last workgroup with one sequence.  Every n meets the bars; P, O and dQ | dK | dV are bit for bit those of n = 1 (no operand
    of a sequence's sums depends on what shares its workgroup); two runs are bit-identical, the table gradient included; across
    n the table gradient sums other partial tables and is held to the f64 bar only."""
    c = _case(S)
    assert c.N == 256 and (n not in (3, 5) or c.N % n == 1)
    one, got, again = _npw_run(S, 1), _npw_run(S, n), _npw_run(S, n, True)
    assert got is not again
    _check_fwd("4 per workgroup fwd", c, got[0], got[1], (S, n))
    _check_bwd("4 per workgroup bwd", c, got[2], got[3], (S, n))
    for name, a, b, b2 in zip(("P", "O", "dQ | dK | dV", "dtable"), got, one, again):
        assert A.same_bits(a, b2) if a.dtype == torch.float32 else torch.equal(a, b2), (name, "run to run")
        if name != "dtable":
            assert A.same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b), (name, "n", n, "against n = 1")


# ------------------------------------------------------------------------------------- 5. table-gradient arms

@pytest.mark.parametrize("S", [17, 49, 81])
def test_table_gradient_by_atomics_and_without(S):
    """dtable_chunks = 0 (a C caller; functional.attn_bwd always asks for partial tables): every workgroup adds its table into
    one zeroed [rows, H] table with float atomics - against f64 at the bar (the order of those adds is not fixed: no bitwise
    claim).  dtable = NULL with the bias present: no table work at all.  dQ, dK, dV do not touch the table: both give, bit for
    bit, those of the partial-table call."""
    c = _case(S)
    _, _, g0, _ = _fused_run(S)
    (g, ), dt = _raw_bwd(c, table_grad="atomic")
    _check_bwd("5 atomic table", c, g, dt, (S,))
    assert torch.equal(g, g0)
    (g, ), dt = _raw_bwd(c, table_grad=None)
    assert dt is None and torch.equal(g, g0)


def test_large_table_near_the_lds_budget():
    """S = 81, H = 2, a 5000-row table under an injective index that reaches its last row: attn_bwd3_kernel<3, 5> holds three
    per-wave tables of 5000 floats beside its ring and image, 128352 B of the 160 KB (the launcher's own arithmetic, restated in
    util_attn_packed.bwd3_lds; the first generation's footprint, which lstc_attn_bwd checks first, is 154496 B).  Table rows fit
    the 16 bits the kernel keeps per pair.  Partial tables and atomics, both against f64."""
    S, H, rows = 81, 2, 5000
    assert max(A.bwd3_lds(3, rows), A.bwd_lds(3, rows)) <= 160 * 1024 and rows < 0xFFFF
    c = _build(S, H=H, table_rows=rows)
    assert int(c.index.max()) == rows - 1 and float(c.dt[rows - 1].abs().max()) > 0.0
    probs, o = _raw(c)
    _check_fwd("5 large table fwd", c, probs, o, (rows,))
    (g,), dt = _raw_bwd(c)
    _check_bwd("5 large table bwd", c, g, dt, (rows,))
    (g2,), dt2 = _raw_bwd(c, table_grad="atomic")
    _check_bwd("5 large table bwd, atomics", c, g2, dt2, (rows,))
    assert torch.equal(g, g2)
