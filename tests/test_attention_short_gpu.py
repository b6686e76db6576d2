"""The row-operand attention kernels for S <= 96 (csrc/attention.hip: the first-generation attn_fwd_kernel / attn_bwd_kernel,
the staged attn_fwd2_kernel / attn_bwd2_kernel; csrc/attention_pk.hip: the lane-=-query attn_fwd3f_kernel) against a float64
restatement of the contract (include/lstc_hip.h, "attention"; tests/util.py attn_reference, on the device), arm by arm of the
dispatch in attn_fwd / attn_bwd.

Bars, exact-f32 products: P within 2e-6; O, dQ, dK, dV and the table gradient within 2e-5 * max|ref| + 1e-6.  Every fp32 case
with S >= 2 also checks that the O bar sees one lost key (the f64 O without key S - 1 is more than 4 bars away).  bf16 products
(LSTC_BF16 on the staged kernels): relative Frobenius error of O and every gradient above 10x the exact run's and below 8e-3, the
exact run's below 1e-5; P within 4e-6 of the f64 softmax of the RNE-rounded operands the kernel contracts.

A test cannot see a kernel's name, so the dispatch is stated as bitwise identities between LstcAttnDesc.variant = 0, 1, 2, 3
(tests/util_attn_short.py forward_groups) and asserted on P and O wherever all four variants run.

Inputs follow the long sweep (tests/test_attention_sweep_gpu.py): the models' own index, sliced whenever S - 1 < 16 L, a table
scaled by 0.4, attention dropout 0.2 replayed through functional.dropout_mask.  The worst error of every section against its bar
is in profiles/attention_short_errors.txt (written when LSTC_ATTN_SHORT_ERRORS names a file)."""
import functools

import pytest
import torch

import util_attn_short as A
from util import attn_layout, attn_reference, attn_rounded_probs

pytestmark = pytest.mark.gpu

DEV = A.DEV
GRADS = ("dQ", "dK", "dV", "dtable")


def _reference(q, k, v, do, N, S, H, dk, dv, table, index, seed):
    keep = A.keep_mask(N, H, S, seed)
    return attn_reference(q, k, v, do, N, S, H, dk, dv, table, index, keep, A.P_DROP), keep


# ------------------------------------------------------------------------------------- 0. O base off a 16-B boundary

@pytest.mark.parametrize("S,forced,twin", [(17, 0, 2), (81, 0, 2), (49, 3, 1)])
def test_forward_into_an_output_base_off_a_16_byte_boundary(S, forced, twin):
    """attn_fwd3f_kernel alone writes O rows as 16-B stores (a3_f4, csrc/attention_pk.hip); fill_params' vec_v looks at V, ldv
    and ldo, not at the base of O.  The launcher therefore asks for a 16-B aligned O before it takes that kernel: a C caller
    with aligned Q, K, V, ldo % 4 == 0 and an O base one float past a 16-B boundary gets the next arm - attn_fwd2_kernel at
    T = 1 and 3, the first generation at T = 2 (variant 3 forced) - whose O rows leave as 4-B stores: bit for bit the
    variant-``twin`` run into an aligned O, and within the f64 bars.
    The same question for the backward: attn_bwd2_kernel writes dQ, dK, dV with raw_buffer_store_b32 (RTL_COMPUTE) and the
    first-generation kernels with scalar stores (lds_times_rows), so their bases need 4-B alignment only; the 16-B accesses
    of the staged kernels are the LDS-DMA reads of Q, K (forward) and dO, V (backward), which vec_qk / vec_v do check."""
    N, H, d, seed = 3, 2, 64, 900 + S
    q, k, v, do, table, index = A.inputs(N, S, H, d, d, seed=S * 13)
    M, ldo = N * S, H * d
    buf = torch.full((M * ldo + 8,), float("nan"), device=DEV)
    o_off = buf[1: 1 + M * ldo].view(M, ldo)
    assert o_off.data_ptr() % 16 == 4 and ldo % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (q, k, v))
    p_off, _ = A.raw_fwd(q, k, v, o_off, N, S, H, d, d, table, index, seed, variant=forced)
    p_al, o_al = A.raw_fwd(q, k, v, torch.empty(M, ldo, device=DEV), N, S, H, d, d, table, index, seed, variant=twin)
    assert A.same_bits(p_off, p_al) and A.same_bits(o_off, o_al)
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + M * ldo:]).all())      # nothing written around the view
    ref, _ = _reference(q, k, v, None, N, S, H, d, d, table, index, seed)
    A.check_exact("0 unaligned O", (p_off, o_off), ref[:2], (S, forced), names=("P", "O"))


# ------------------------------------------------------------------------------------- 2. sequence lengths

SWEEP_S = [1, 2, 3, 16, 17, 31, 32, 33, 34, 48, 49, 63, 64, 65, 66, 80, 81, 95, 96]
SWEEP_S_32_96 = [2, 17, 31, 32, 65, 81, 95, 96]
SWEEP = [(S, 64, 64) for S in SWEEP_S] + [(S, 32, 96) for S in SWEEP_S_32_96]
SWEEP_BF16 = [(S, 64, 64) for S in SWEEP_S] + [(S, 32, 96) for S in SWEEP_S]


@functools.lru_cache(maxsize=None)
def _sweep_case(S, dk, dv):
    """Inputs, the f64 reference and the fp32 variant-0 forward and backward of one sweep shape (shared by the fp32 and the
    bf16 test of that shape; nothing in it is written afterwards)."""
    N, H, seed = 3, 2, 101 + S
    ins = A.inputs(N, S, H, dk, dv, seed=S * 7 + dk)
    q, k, v, do, table, index = ins
    ref, keep = _reference(q, k, v, do, N, S, H, dk, dv, table, index, seed)
    return N, H, seed, ins, ref, keep


@pytest.mark.parametrize("S,dk,dv", SWEEP)
def test_sequence_length_sweep_fp32(S, dk, dv):
    """Every S at which a short kernel changes its tile count or the tail of a tile (T = 1, 2, 3; one row, one key past a
    tile edge, the last row of a tile), N = 3, H = 2: the forward under variants 0 .. 3 (first generation, attn_fwd2, attn_fwd3f
    as forward_groups says), the backward under variants 0 (attn_bwd2) and 1 (first generation) on the P of the variant-0
    forward, all against f64.  (32, 96): d_v a multiple of 32 but not of 64 - the default there is attn_fwd2_kernel<1, false, 4>
    (S <= 32) and <3, false, 8> (64 < S <= 96).
    The hook reaches the descriptor: at one shape per T the P of the first generation and of attn_fwd3f differ in some bit
    (their logits are the same bits - both contract k = s and k = 16 + s of a 32-feature chunk at MFMA step s - but attn_fwd3f
    sums a softmax row inside the lane and across the two lane halves, the first generation across the wave); at S = 81 the
    table gradients of attn_bwd2_kernel<3, ., 8> (eight per-wave tables) and of the first generation (four) differ likewise.
    attn_fwd2 against the first generation CANNOT be told apart this way in fp32 mode: read side by side, the two stage the
    same sixteen floats per lane and chunk into the same mma8 sequence, run the same row softmax and the same P V block order,
    and measured on an MI355X their P and O are bit-identical at every shape of this file; so are dQ, dK, dV of attn_bwd2 and
    the first-generation backward, and at T <= 2 the table gradient too.  That pair is told apart in bf16 mode
    (test_sequence_length_sweep_bf16), where only the staged kernels round their operands."""
    N, H, seed, (q, k, v, do, table, index), ref, keep = _sweep_case(S, dk, dv)
    res = A.forward_all_variants(q, k, v, N, S, H, dk, dv, table, index, seed)
    for var in (0, 1, 2, 3):
        A.check_exact(f"2 sweep fwd variant {var}", res[var], ref[:2], (S, dk, dv), names=("P", "O"))
    for var in (0, 1):
        got = A.bwd(do, q, k, v, res[0][0], N, S, H, dk, dv, table, index, seed, variant=var)
        if S == 1:          # no (i, j) pair carries a bias: the table gradient is zero, and so is the f64 one (None)
            assert float(got[3].abs().max()) == 0.0
        A.check_exact(f"2 sweep bwd variant {var}", got, ref[2:], (S, dk, dv), names=GRADS)
    if S >= 2:
        A.check_sensitive(q, k, v, N, S, H, dk, dv, table, index, keep, ref[1])
    if (dk, dv) == (64, 64) and S in (17, 49, 81):
        assert not A.same_bits(res[1][0], res[3][0]), "variant 3 gave the first generation's bits: the hook did not arrive"
    if (dk, dv) == (64, 64) and S == 81:
        assert not A.same_bits(got[3], A.bwd(do, q, k, v, res[0][0], N, S, H, dk, dv, table, index, seed, variant=0)[3]), \
            "backward: variant 0 gave the first generation's table gradient"


@pytest.mark.parametrize("S,dk,dv", SWEEP_BF16)
def test_sequence_length_sweep_bf16(S, dk, dv):
    """LSTC_BF16 on the staged kernels attn_fwd2_kernel<T, true, NW> / attn_bwd2_kernel<T, true, NW>, T = 1, 2, 3.  Their
    Q K^T rounds where the long kernel's tile_xt does: a = Q * scale is an f32 product, then mma8<true> rounds a and K to bf16
    (RNE) and accumulates in f32 - so P goes against attn_rounded_probs at its 4e-6.  O and the gradients against the band.
    Variants 0 and 2 are the staged kernel; 1 and 3 the first generation, whose products are exact in both modes: its bits
    are those of the fp32-mode variant-1 run - and differ from the staged kernel's (the hook arrives in this mode too)."""
    N, H, seed, (q, k, v, do, table, index), ref, keep = _sweep_case(S, dk, dv)
    res = A.forward_all_variants(q, k, v, N, S, H, dk, dv, table, index, seed, mode="bf16")
    exact1 = A.fwd(q, k, v, N, S, H, dk, dv, table, index, seed, variant=1)
    assert A.same_bits(res[1][0], exact1[0]) and A.same_bits(res[1][1], exact1[1])
    if S >= 2:
        assert not A.same_bits(res[0][0], res[1][0]), "bf16 mode, variant 0 gave the first generation's P"
        assert not A.same_bits(res[0][1], res[1][1]), "bf16 mode, variant 0 gave the first generation's O"
    p_rounded = attn_rounded_probs(q, k, N, S, H, dk, table, index)
    err_p = float((res[0][0].double() - p_rounded).abs().max())
    A.record("2 sweep bf16 P vs rounded", "P", err_p, 4e-6, (S, dk, dv))
    assert err_p < 4e-6, ("P vs softmax of the rounded operands", err_p)
    got = res[0][1:] + tuple(A.bwd(do, q, k, v, res[0][0], N, S, H, dk, dv, table, index, seed, mode="bf16"))
    p32, o32 = A.fwd(q, k, v, N, S, H, dk, dv, table, index, seed)
    exact = (o32,) + tuple(A.bwd(do, q, k, v, p32, N, S, H, dk, dv, table, index, seed))
    A.check_band("2 sweep", got, exact, ref[1:], (S, dk, dv))


# ------------------------------------------------------------------------------------- 3. head widths

WIDTHS = [(32, 32), (32, 64), (64, 32), (64, 128), (128, 64), (96, 96), (160, 160), (256, 256), (32, 256), (256, 32), (64, 96),
          (96, 64), (16, 16), (48, 48), (8, 8), (24, 40), (20, 20), (6, 10)]


@pytest.mark.parametrize("dk,dv", WIDTHS)
@pytest.mark.parametrize("S", [17, 49, 81])
def test_head_width_matrix(S, dk, dv):
    """d_k != d_v both ways through every staged kernel (attn_fwd2 / attn_bwd2 chunk d_k and d_v separately, attn_fwd3f's ring
    carries d_k / 32 logit units and d_v / 64 output units), one to eight 32-column tiles, and the widths the staged kernels
    refuse (not multiples of 32; 20, 6, 10: not even float4 rows), which run the first generation under every variant.
    fp32: forward under all four variants, backward under 0 and 1, against f64.  bf16: multiples of 32 against the band; every
    other width computes exact-f32 products (include/lstc_hip.h, LstcAttnDesc.dtype): bit for bit the fp32-mode results."""
    N = H = 2
    seed = 7 * S + dk
    q, k, v, do, table, index = A.inputs(N, S, H, dk, dv, seed=1000 * S + 10 * dk + dv)
    ref, keep = _reference(q, k, v, do, N, S, H, dk, dv, table, index, seed)
    res = A.forward_all_variants(q, k, v, N, S, H, dk, dv, table, index, seed)
    exact = {}
    for var in (0, 1):
        A.check_exact(f"3 widths fwd variant {var}", res[var], ref[:2], (S, dk, dv), names=("P", "O"))
        exact[var] = A.bwd(do, q, k, v, res[0][0], N, S, H, dk, dv, table, index, seed, variant=var)
        A.check_exact(f"3 widths bwd variant {var}", exact[var], ref[2:], (S, dk, dv), names=GRADS)
    A.check_sensitive(q, k, v, N, S, H, dk, dv, table, index, keep, ref[1])
    if dk % 32 == 0 and dv % 32 == 0:
        res16 = A.forward_all_variants(q, k, v, N, S, H, dk, dv, table, index, seed, mode="bf16")
        assert A.same_bits(res16[1][0], res[1][0]) and A.same_bits(res16[1][1], res[1][1])
        got = res16[0][1:] + tuple(A.bwd(do, q, k, v, res16[0][0], N, S, H, dk, dv, table, index, seed, mode="bf16"))
        A.check_band("3 widths", got, res[0][1:] + tuple(exact[0]), ref[1:], (S, dk, dv))
    else:
        p16, o16 = A.fwd(q, k, v, N, S, H, dk, dv, table, index, seed, mode="bf16")
        g16 = A.bwd(do, q, k, v, p16, N, S, H, dk, dv, table, index, seed, mode="bf16")
        for name, a, b in zip(A.NAMES, (p16, o16) + tuple(g16), res[0] + tuple(exact[0])):
            assert A.same_bits(a, b), ("bf16 mode outside the staged kernels", name, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------- 4. operand layouts

@pytest.mark.parametrize("kind", ["odd_ld", "offset", "strides", "fused"])
@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("S", [17, 49, 81])
def test_operand_layouts(S, d, kind):
    """Forward and backward on operands, and into outputs, of one layout (O takes dO's).  A row stride that is no multiple of
    4 or a base off a 16-B boundary is not vectorisable: every variant runs the first generation (one set of bits), whose
    tile_abt then loads through load16's scalar path - the same sixteen floats per lane and the same mma8 sequence as its
    float4 path, so the bits are also those of the variant-1 run on contiguous aligned copies.  The fused Q | K | V buffer (all
    bases aligned, row stride 3 H d) stays vectorisable: the staged-kernel identities of forward_groups hold (d = 64; d = 80 is
    no multiple of 32).  Everything against f64."""
    N, H, seed = 2, 2, 31 * S + d
    q, k, v, do, table, index = A.inputs(N, S, H, d, d, seed=S + 3 * d)
    ql, kl, vl, dol = attn_layout(kind, (q, k, v, do))
    vec = all(t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in (ql, kl, vl, dol))
    assert vec == (kind == "fused") and (kind != "fused" or ql.stride(0) == 3 * H * d)

    def outputs():
        views = attn_layout(kind, tuple(torch.full_like(t, float("nan")) for t in (q, k, v, do)))
        return views[:3], views[3]

    ref, keep = _reference(q, k, v, do, N, S, H, d, d, table, index, seed)
    res = A.forward_all_variants(q, k, v, N, S, H, d, d, table, index, seed, vectorisable=vec,
                                 run=lambda var: A.raw_fwd(ql, kl, vl, outputs()[1], N, S, H, d, d, table, index, seed, variant=var))
    grads = {}
    for var in (0, 1):
        A.check_exact(f"4 layouts fwd variant {var}", res[var], ref[:2], (S, d, kind), names=("P", "O"))
        grads[var] = A.bwd(dol, ql, kl, vl, res[0][0], N, S, H, d, d, table, index, seed, variant=var, out=outputs()[0])
        A.check_exact(f"4 layouts bwd variant {var}", grads[var], ref[2:], (S, d, kind), names=GRADS)
    A.check_sensitive(q, k, v, N, S, H, d, d, table, index, keep, ref[1])
    if kind == "fused" and d == 64 and S != 49:      # the default there is attn_fwd3f, not the first generation's bits
        assert not A.same_bits(res[0][0], res[1][0]), "fused Q | K | V: the default forward gave the first generation's P"
    if kind == "fused" and d == 64 and S == 81:      # eight per-wave tables against four: attn_bwd2 ran
        assert not A.same_bits(grads[0][3], grads[1][3]), "fused Q | K | V: variant 0 gave the first generation's table gradient"
    if not vec:
        p1, o1 = A.fwd(q, k, v, N, S, H, d, d, table, index, seed, variant=1)
        g1 = A.bwd(do, q, k, v, p1, N, S, H, d, d, table, index, seed, variant=1)
        for var in (0, 1):
            for name, a, b in zip(A.NAMES, res[var] + tuple(grads[var]), (p1, o1) + tuple(g1)):
                assert A.same_bits(a, b), (kind, "variant", var, "vs first generation on contiguous copies", name)


# ------------------------------------------------------------------------------------- 5. several sequences per workgroup

@pytest.mark.parametrize("N,S", [(257, 33), (257, 65), (257, 96), (385, 33), (385, 65), (385, 96), (2049, 2), (2049, 17)])
def test_lane_query_forward_with_several_sequences_per_workgroup(N, S):
    """attn_fwd3f_kernel's producer ring runs across the n_per_wg = N H / 1024 (/ 8192 at S <= 32) sequences of a workgroup:
    2 and 3 sequences with a last chunk of one (H = 8, d_k = 32, d_v = 64: one logit unit and one output unit per sequence,
    so every ring slot changes sequence).  Variant 3 throughout (S = 33 needs it; elsewhere it is the default's kernel).
    P and O of the first and the last 4 sequences against f64, all of them against the first generation at the bars of
    test_f32_lane_query_attention_forward_matches_the_first_generation.  A sequence's result does not depend on what shares
    its workgroup: windows of 4 sequences rerun as a call of their own (4 H < the divisor: one sequence per workgroup) give the
    same bits - O without dropout, whose counter is the sequence's index in the call; P is written before dropout."""
    H, dk, dv, seed = 8, 32, 64, 77 + S
    per = (N * H) // (8192 if S <= 32 else 1024)
    assert per in (2, 3) and N % per == 1
    q, k, v, _, table, index = A.inputs(N, S, H, dk, dv, seed=N + S)
    p3, o3 = A.fwd(q, k, v, N, S, H, dk, dv, table, index, seed, variant=3)
    p1, o1 = A.fwd(q, k, v, N, S, H, dk, dv, table, index, seed, variant=1)
    err_p, err_o = float((p3 - p1).abs().max()), float((o3 - o1).abs().max())
    A.record("5 fwd3f vs first generation", "P", err_p, 2e-6, (N, S))
    A.record("5 fwd3f vs first generation", "O", err_o, 2e-5 * max(1.0, float(o1.abs().max())), (N, S))
    assert err_p < 2e-6 and err_o < 2e-5 * max(1.0, float(o1.abs().max())), (err_p, err_o)
    keep = A.keep_mask(N, H, S, seed)
    for name, sl in (("first 4", slice(0, 4)), ("last 4", slice(N - 4, N))):
        rows = slice(sl.start * S, sl.stop * S)
        ref = attn_reference(q[rows], k[rows], v[rows], None, 4, S, H, dk, dv, table, index, keep[sl], A.P_DROP)
        A.check_exact("5 fwd3f several per workgroup", (p3[sl], o3[rows]), ref[:2], (N, S, name), names=("P", "O"))
        if S >= 2:
            A.check_sensitive(q[rows], k[rows], v[rows], 4, S, H, dk, dv, table, index, keep[sl], ref[1])
    p0, o0 = A.fwd(q, k, v, N, S, H, dk, dv, table, index, seed, variant=3, p_drop=0.0)
    assert A.same_bits(p0, p3)
    for n0 in (0, 1, per, N // 2, N - 5, N - 4):
        rows = slice(n0 * S, (n0 + 4) * S)
        ps, os_ = A.fwd(q[rows], k[rows], v[rows], 4, S, H, dk, dv, table, index, seed, variant=3, p_drop=0.0)
        assert A.same_bits(ps, p0[n0: n0 + 4]) and A.same_bits(os_, o0[rows]), ("window at sequence", n0)


@functools.lru_cache(maxsize=None)
def _bwd_chunk_case(S):
    N, H, d, seed = 7, 2, 64, 5 * S
    ins = A.inputs(N, S, H, d, d, seed=S + d)
    q, k, v, do, table, index = ins
    probs, _ = A.fwd(q, k, v, N, S, H, d, d, table, index, seed)
    ref, _ = _reference(q, k, v, do, N, S, H, d, d, table, index, seed)
    return N, H, d, seed, ins, probs, ref


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("npw", [1, 2, 3, 5])
@pytest.mark.parametrize("S", [17, 49, 81])
def test_backward_workgroups_with_several_sequences(S, npw, variant, monkeypatch):
    """N = 7 sequences in chunks of npw (uneven last chunk at 2, 3, 5): a workgroup of attn_bwd2_kernel (variant 0) or
    attn_bwd_kernel (variant 1) reuses its LDS images (dP / dA, Pd, dA^T, the staging ring) and adds into its per-wave bias
    tables across its sequences.  Every gradient against f64; two runs bit-identical, the table gradient included.  dQ, dK,
    dV bit-identical to the one-sequence-per-workgroup run: both kernels write each (row, column) of a sequence from one wave
    (RTL_COMPUTE / lds_times_rows: wave = 32-column tile, lane = column) with a sum order fixed by the tile loops, and no
    operand of those sums depends on the chunk.  The table gradient sums its partial tables in chunk order: f64 bars only."""
    N, H, d, seed, (q, k, v, do, table, index), probs, ref = _bwd_chunk_case(S)
    F = A.Fn()
    seen = []
    colsum = F.colsum
    monkeypatch.setattr(F, "colsum", lambda parts, *a, **kw: (seen.append(parts.shape[0]), colsum(parts, *a, **kw))[1])
    run = lambda n: A.bwd(do, q, k, v, probs, N, S, H, d, d, table, index, seed, variant=variant, npw=n)
    one, got, again = run(1), run(npw), run(npw)
    per = -(-N // -(-N // npw))
    assert seen == [N, -(-N // per), -(-N // per)] and (npw == 1 or (per >= 2 and N % per != 0)), (seen, per)
    A.check_exact(f"5 bwd several per workgroup variant {variant}", got, ref[2:], (S, npw), names=GRADS)
    for name, a, b, b2 in zip(GRADS, got, one, again):
        assert A.same_bits(a, b2), (name, "run to run")
        if name != "dtable":
            assert A.same_bits(a, b), (name, "npw", npw, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------- 6. table-gradient arms

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("S", [17, 49, 81])
def test_table_gradient_by_atomics(S, variant):
    """LstcAttnDesc.dtable_chunks = 0 (a C caller; functional.attn_bwd always asks for partial tables): every workgroup adds
    its table into one zeroed [rows, H] table with float atomics - against f64 at the bar (the order of those adds is not
    fixed: no bitwise claim).  dQ, dK, dV do not touch the table: bit for bit those of the partial-table call."""
    N, H, d, seed = 5, 3, 64, 40 + S
    q, k, v, do, table, index = A.inputs(N, S, H, d, d, seed=3 * S + 1)
    probs, _ = A.fwd(q, k, v, N, S, H, d, d, table, index, seed)
    ref, _ = _reference(q, k, v, do, N, S, H, d, d, table, index, seed)
    out = lambda: tuple(torch.full_like(t, float("nan")) for t in (q, k, v))
    atom = A.raw_bwd(do, q, k, v, probs, out(), N, S, H, d, d, table, index, seed, variant=variant, chunks=0)
    part = A.raw_bwd(do, q, k, v, probs, out(), N, S, H, d, d, table, index, seed, variant=variant, chunks=N)
    A.check_exact(f"6 atomic table variant {variant}", atom, ref[2:], (S,), names=GRADS)
    A.check_exact(f"6 partial tables variant {variant}", part, ref[2:], (S,), names=GRADS)
    for name, a, b in zip(GRADS[:3], atom, part):
        assert A.same_bits(a, b), name


@pytest.mark.parametrize("rows,shift,falls_back", [(1300, 1100, True), (600, 400, False)])
def test_staged_backward_falls_back_when_its_tables_pass_the_lds_budget(rows, shift, falls_back):
    """S = 81, d = 64: attn_bwd2_kernel<3, ., 8> needs 123648 + 32 table_rows bytes of LDS, the first generation 74496 + 16
    table_rows.  1300 rows put the staged kernel past 160 KB (165248 B) and the first generation at 95296 B: variant 0 runs the
    first generation - variant 1's bits, dtable included.  600 rows (142848 B) stay on the staged kernel.  The index is
    index[i][j] = j - i + (S - 2) + shift: injective within a row, as the backward requires, and reaching rows near the end of
    the table.  Both against f64."""
    N, S, H, d, seed = 2, 81, 2, 64, 600 + rows
    g = torch.Generator(device=DEV).manual_seed(rows)
    q, k, v, do = (torch.randn(N * S, H * d, device=DEV, generator=g) for _ in range(4))
    table = 0.4 * torch.randn(rows, H, device=DEV, generator=g)
    i = torch.arange(S - 1, device=DEV)
    index = (i[None, :] - i[:, None] + (S - 2) + shift).contiguous()
    assert int(index.min()) == shift and int(index.max()) == 2 * (S - 2) + shift < rows and index.dtype == torch.int64
    assert (123648 + 32 * rows > 160 * 1024) == falls_back and 74496 + 16 * rows <= 160 * 1024
    probs, o = A.fwd(q, k, v, N, S, H, d, d, table, index, seed)
    ref, _ = _reference(q, k, v, do, N, S, H, d, d, table, index, seed)
    A.check_exact("6 lds fallback fwd", (probs, o), ref[:2], (rows,), names=("P", "O"))
    g0 = A.bwd(do, q, k, v, probs, N, S, H, d, d, table, index, seed, variant=0)
    g1 = A.bwd(do, q, k, v, probs, N, S, H, d, d, table, index, seed, variant=1)
    A.check_exact("6 lds fallback bwd variant 0", g0, ref[2:], (rows,), names=GRADS)
    A.check_exact("6 lds fallback bwd variant 1", g1, ref[2:], (rows,), names=GRADS)
    if falls_back:
        for name, a, b in zip(GRADS, g0, g1):
            assert A.same_bits(a, b), name
    else:       # eight per-wave tables against four: another sum order, so the staged kernel did run
        assert not A.same_bits(g0[3], g1[3])
