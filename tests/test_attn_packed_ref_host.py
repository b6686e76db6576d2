"""CPU twin of tests/test_attention_packed_gpu.py: the float64 model of the packed-operand attention kernels
(tests/util_attn_packed.py) is the contract when its roundings are taken out, an f32 evaluation of the same chain stays under
half of every bar the GPU file applies, wrong kernels of six kinds land far outside them, and every refusal of lstc_attn_bwd /
lstc_attn_fwd that the GPU file relies on happens before a launch."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import util_attn_packed as A
from util import attn_reference, host_dropout_keep

CPU = "cpu"


def _keep(N, H, S, seed, p_drop=A.P_DROP):
    n = N * H * S * S
    return torch.from_numpy(host_dropout_keep(np.arange(n), p_drop, seed).reshape(N, H, S, S).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _case(S, d, N, H=4):
    """Inputs, keep mask and the f64 model (forward, and backward on the f32 of its own P) of one shape; nothing in it is written
    afterwards."""
    seed = 300 + S
    ins = A.inputs(N, S, H, d, d, seed=11 * S + d, device=CPU)
    q, k, v, do, table, index = ins
    keep = _keep(N, H, S, seed)
    p64, o, bo = A.model_fwd(q, k, v, N, S, H, d, d, table, index, keep, A.P_DROP)
    p32 = p64.float()
    grads = A.model_bwd(do, q, k, v, p32, N, S, H, d, d, table, index, keep, A.P_DROP)
    return ins, keep, p64, p32, ((o, bo),) + tuple(grads[:3]), grads[3]


@pytest.mark.parametrize("S", [1, 2, 17, 49])
def test_model_without_roundings_is_the_contract(S):
    """No bf16 rounding anywhere, backward on the f64 P: P, O, dQ, dK, dV and the table gradient of util.attn_reference (torch
    autograd of the contract's forward) to 1e-12."""
    N, H, d, seed = 3, 2, 64, 50 + S
    q, k, v, do, table, index = A.inputs(N, S, H, d, d, seed=S, device=CPU)
    keep = _keep(N, H, S, seed)
    ref = attn_reference(q, k, v, do, N, S, H, d, d, table, index, keep, A.P_DROP)
    p, o, _ = A.model_fwd(q, k, v, N, S, H, d, d, table, index, keep, A.P_DROP, rounding=False)
    (dq, _), (dk, _), (dv, _), dt = A.model_bwd(do, q, k, v, p, N, S, H, d, d, table, index, keep, A.P_DROP, rounding=False)
    for name, a, b in zip(("P", "O", "dQ", "dK", "dV", "dtable"), (p, o, dq, dk, dv, dt), ref):
        if b is None:       # S = 1: no (i, j) pair carries a bias, autograd never saw the table
            assert S == 1 and name == "dtable"
            continue
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    if S == 1:      # dA = P (dP - dP P) with P = 1: zero in every arithmetic - the GPU file demands exact zeros there
        assert float(dq.abs().max()) == 0.0 and float(dk.abs().max()) == 0.0 and float(dt.abs().max()) == 0.0


@pytest.mark.parametrize("S,d", [(2, 64), (17, 64), (49, 64), (96, 64), (81, 256)])
def test_f32_chain_with_output_rounding_stays_under_half_of_every_bar(S, d):
    """The model evaluated as the kernels evaluate it - every sum in f32, the outputs rounded to bf16 - against the f64 model, at
    the N = 256 of the GPU file's odd S: under HALF of each bar (P, stat, excess, share, and the table gradient, whose f32 sum
    runs over all 256 sequences), so the bars leave the kernels room for nothing but another summation order."""
    N, H = 256, 4
    (q, k, v, do, table, index), keep, p64, p32, outs, dt64 = _case(S, d, N)
    f32 = dict(dt=torch.float32, round_out=True)
    p, o, _ = A.model_fwd(q, k, v, N, S, H, d, d, table, index, keep, A.P_DROP, **f32)
    A.check_probs("host f32 chain", p, p64, (S, d), factor=0.5)
    (dq, _), (dk, _), (dv, _), dt = A.model_bwd(do, q, k, v, p32, N, S, H, d, d, table, index, keep, A.P_DROP, **f32)
    for name, got, (ref, bound) in zip(A.OUTS, (o, dq, dk, dv), outs):
        A.check_out("host f32 chain", name, got, ref, bound, S, (S, d), factor=0.5)
    A.check_table("host f32 chain", dt, dt64, (S, d), factor=0.5)


@pytest.mark.parametrize("mutant", sorted(A.MUTANTS))
@pytest.mark.parametrize("S", [49, 96])
def test_wrong_kernels_land_past_four_bars(S, mutant):
    """Each mutant of the model moves ``stat`` of every result it touches past 4 bars (and leaves the others alone)."""
    N, H, d = 8, 4, 64
    (q, k, v, do, table, index), keep, p64, p32, outs, _ = _case(S, d, N)
    _, o, _ = A.model_fwd(q, k, v, N, S, H, d, d, table, index, keep, A.P_DROP, mutant=mutant)
    (dq, _), (dk, _), (dv, _), _ = A.model_bwd(do, q, k, v, p32, N, S, H, d, d, table, index, keep, A.P_DROP, mutant=mutant)
    for name, got, (ref, bound) in zip(A.OUTS, (o, dq, dk, dv), outs):
        stat = A.measure(got, ref, bound, S)[0]
        if name in A.MUTANTS[mutant]:
            assert stat > 4 * A.BAR_STAT, (mutant, name, stat)
        else:
            assert stat == 0.0, (mutant, name, stat)


def test_measure_counts_a_result_where_the_reference_is_zero():
    ref, bound = torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64)
    ref[0, 0] = bound[0, 0] = 1.0
    got = ref.clone()
    assert A.measure(got, ref, bound, 2) == (0.0, 0.0, 0.0)      # zeros on a zero reference and bound are no error
    got[1, 1] = 1e-3          # token index 1 has a zero reference: any value there is infinitely far
    stat, worst, share = A.measure(got, ref, bound, 2)
    assert stat == float("inf") and worst == float("inf") and share == 1 / 8
    assert A.measure(got, torch.zeros_like(ref), bound, 2) is None


# ---------------------------------------------------------------------------------------------------- refusals before a launch

@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _packed_desc(S=49, N=256, H=4, d=64):
    from lstc_vad_amd._lib import AttnDesc
    p = AttnDesc()
    p.Q = p.K = p.V = p.probs = p.O_pack = p.dO = p.dQ_pack = p.dK_pack = p.dV_pack = 4096
    p.N, p.S, p.H, p.dk, p.dv, p.dtype, p.scale = N, S, H, d, d, 1, d ** -0.5
    p.in_pack_cols, p.K_col0, p.V_col0, p.probs_ld = 3 * H * d, H * d, 2 * H * d, (S + 3) // 4 * 4
    p.dO_pack_cols, p.pack_cols, p.dK_col0, p.dV_col0 = H * d, 3 * H * d, H * d, 2 * H * d
    p.ldo = H * d
    return p


def test_packed_backward_refusals_the_gpu_file_relies_on(lib):
    """Each returns before a launch (no GPU here): packed inputs with d_k = 96 or 32 (the forward takes d_k % 32, the backward
    needs d_k % 64) - LSTC_E_UNSUPPORTED; dO_pack_cols = 0 (packed Q | K | V with a row-operand dO) - LSTC_E_UNSUPPORTED; a table
    past the LDS budget - LSTC_E_RANGE."""
    for dk in (96, 32):
        p = _packed_desc()
        p.dk, p.in_pack_cols, p.K_col0, p.V_col0 = dk, 4 * (2 * dk + 64), 4 * dk, 8 * dk
        p.pack_cols, p.dK_col0, p.dV_col0 = p.in_pack_cols, p.K_col0, p.V_col0
        assert p.in_pack_cols % 64 == 0 and lib.lstc_attn_bwd(C.byref(p), None) == -4, dk
    p = _packed_desc()
    p.dO_pack_cols = 0
    assert lib.lstc_attn_bwd(C.byref(p), None) == -4
    # S = 81 (T = 3): lstc_attn_bwd first holds every S <= 128 call to the first generation's footprint, 74496 + 16 table_rows
    # bytes, then attn_bwd3_kernel<3, 5> to its own, 68352 + 12 table_rows (util_attn_packed.bwd3_lds): 5584 rows are the most
    # a packed S = 81 call can carry, and the 5000-row table of the GPU file fits both
    p = _packed_desc(S=81)
    p.table = p.index = p.dtable = 4096
    p.index_ld, p.dtable_chunks = 80, 256
    p.table_rows = (160 * 1024 - 74496) // 16 + 1
    assert p.table_rows == 5585 and A.bwd3_lds(3, p.table_rows) <= 160 * 1024 < A.bwd_lds(3, p.table_rows)
    for chunks in (256, 0):
        p.dtable_chunks = chunks
        assert lib.lstc_attn_bwd(C.byref(p), None) == -5, chunks
    assert A.bwd3_lds(3, 5000) == 128352 and A.bwd_lds(3, 5000) == 154496 and max(A.bwd3_lds(3, 5000), A.bwd_lds(3, 5000)) <= 160 * 1024


@pytest.mark.parametrize("S", [17, 49, 81, 96])
def test_probability_pitch_past_the_key_tiles_is_refused(lib, S):
    """include/lstc_hip.h, probs_ld: attn_fwd3_kernel stores the 16-B groups of a row's 32 T key columns and no others, and
    attn_bwd3_kernel reads the same ones - a pitch past 32 T would hold columns that the forward leaves unwritten, against the
    header's "zeros in the padding columns".  The launcher refuses it (LSTC_E_SHAPE), forward and backward; a pitch below S or
    off a multiple of 4 likewise."""
    T = -(-S // 32)
    for pld in (32 * T + 4, 32 * T + 32, (S - 1) // 4 * 4, S + 1, S + 2):
        assert pld > 32 * T or pld < S or pld % 4
        p = _packed_desc(S=S)
        p.probs_ld = pld
        assert lib.lstc_attn_fwd(C.byref(p), None) == -2, (S, pld)
        assert lib.lstc_attn_bwd(C.byref(p), None) == -2, (S, pld)
