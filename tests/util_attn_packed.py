"""Helpers of tests/test_attention_packed_gpu.py and tests/test_attn_packed_ref_host.py: a float64 model of the packed-operand
bf16 attention kernels (csrc/attention_pk.hip attn_fwd3_kernel / attn_bwd3_kernel) with the kernels' rounding points, the bars
it is compared under, and lstc_attn_fwd / lstc_attn_bwd through a descriptor built here with every packed field settable.

The model is pure torch and runs on CPU and GPU tensors alike.  Its inputs are bf16-representable, so every product of two
operands is exact in f64.  Rounding points, as read from the kernels:
  forward   A = scale (Q K^T) + bias (Q is NOT pre-scaled: the f32 logits of the bf16 operands are multiplied by the f32 scale);
            P = softmax(A), what ``probs`` receives; Pd = bf16(P keep / (1 - p)) (RNE of the f32 value); O = sum_j Pd V, rounded
            once to bf16 on the way out.
  backward  on a given P: dP = dO V^T; dpk = dP keep / (1 - p); rs = sum_j dpk P; dA = P (dpk - rs); dtable[index] += dA[1:, 1:]
            from the unrounded dA; dQ = scale sum_j bf16(dA) K; dK = scale sum_i bf16(dA) Q; dV = sum_i bf16(P keep / (1 - p)) dO;
            dQ, dK, dV rounded once to bf16 on the way out.
The model returns the UNROUNDED outputs (the kernels' output rounding is inside the bars) and, with each contraction, its
magnitude bound sum |a| |b|.

Bars (none measured on the kernels; tests/test_attn_packed_ref_host.py holds an f32 evaluation of the model under half of each):
  P against the f64 softmax                                 4e-6
  O, dQ, dK, dV  stat, per token position                   <= 2^-8     relative Frobenius error over every sequence, head and
                                                                        column of one token index, maximum over the indices
  O, dQ, dK, dV  excess = |got - ref| - 2^-8 |ref|          <= 2^-7 bound, every element (every bf16 operand on its other
                                                                        neighbour)
  O, dQ, dK, dV  share of elements with excess > 1e-5 bound <= 2e-3
  dtable against f64                                        2e-5 max|ref| + 1e-6
A reference that is zero everywhere (dQ and dK at S = 1) demands exact zeros; every result must be finite."""
import atexit
import ctypes as C
import os

import torch

P_DROP = 0.2
BAR_P, BAR_STAT, BAR_EXCESS, EXCESS_FLOOR, BAR_SHARE = 4e-6, 2.0 ** -8, 2.0 ** -7, 1e-5, 2e-3
OUTS = ("O", "dQ", "dK", "dV")
MUTANTS = {          # a wrong kernel the bars must see -> the results it moves
    "pair": OUTS,               # one (i, j) pair lost at the last query row
    "key": OUTS,                # key S - 1 lost for every query
    "noscale": OUTS,            # the dropout scale 1 / (1 - p) dropped
    "rs_nokeep": ("dQ", "dK"),  # rs taken without the keep factor
    "dq_unscaled": ("dQ",),     # dQ built from unscaled dA
    "vswap": ("O", "dQ", "dK"), # one V row swapped with its neighbour
}


def Fn():
    from lstc_vad_amd import functional
    return functional


def L():
    from lstc_vad_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- inputs

def model_index(S, device):
    """The models' index for S tokens at 16 patches (wider than S - 1 whenever S - 1 < 16 L) and its table row count."""
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d
    n = max(1, -(-(S - 1) // 16))
    return relative_position_index_3d(n, 4).to(device), (2 * n - 1) * 49


def shifted_index(S, rows, device):
    """index[i][j] = j - i + (S - 2) + shift, injective within a row (the backward's precondition), its largest entry the last
    row of a ``rows``-row table."""
    i = torch.arange(S - 1, device=device)
    index = (i[None, :] - i[:, None] + (S - 2) + (rows - 1 - 2 * (S - 2))).contiguous()
    assert int(index.min()) >= 0 and int(index.max()) == rows - 1 and index.dtype == torch.int64
    return index


def inputs(N, S, H, dk, dv, seed, device="cuda", table_rows=None):
    """As util_attn_short.inputs - Q, K [N S, H d_k], V, dO [N S, H d_v], the table scaled by 0.4, the models' index - with every
    value rounded to bf16 (kept as f32).  ``table_rows``: a table of that many rows under ``shifted_index``."""
    g = torch.Generator(device=device).manual_seed(seed)
    q, k = (torch.randn(N * S, H * dk, device=device, generator=g) for _ in range(2))
    v, do = (torch.randn(N * S, H * dv, device=device, generator=g) for _ in range(2))
    if table_rows is None:
        index, rows = model_index(S, device)
    else:
        index, rows = shifted_index(S, table_rows, device), table_rows
    table = 0.4 * torch.randn(rows, H, device=device, generator=g)
    q, k, v, do, table = (t.bfloat16().float() for t in (q, k, v, do, table))
    return q, k, v, do, table, index


def keep_mask(N, H, S, seed, p_drop=P_DROP, device="cuda"):
    return Fn().dropout_mask((N, H, S, S), p_drop, seed, device) if p_drop > 0 else None


# ---------------------------------------------------------------------------------------------------- the model

def bf16(x):
    """RNE to bf16 of the f32 value of ``x`` (the kernels round f32 registers), back in the dtype of ``x``."""
    return x.float().bfloat16().to(x.dtype)


def _heads(t, N, S, H, dt):
    return t.detach().to(dt).reshape(N, S, H, -1).transpose(1, 2)


def _merge(t):
    N, H, S, d = t.shape
    return t.transpose(1, 2).reshape(N * S, H * d)


def _scale(dk):
    return float(torch.tensor(1.0 / dk ** 0.5, dtype=torch.float32))         # LstcAttnDesc.scale is a float


def _keep_factor(keep, p_drop, dt, mutant):
    if keep is None or p_drop <= 0:
        return None
    return keep.to(dt) if mutant == "noscale" else keep.to(dt) / (1.0 - p_drop)


def _lose(m, S, mutant):
    """The A operand of a token contraction ([N, H, query, key]) under a mutant that loses pairs."""
    if mutant == "pair":
        m = m.clone()
        m[:, :, S - 1, S // 2] = 0
    elif mutant == "key":
        m = m.clone()
        m[:, :, :, S - 1] = 0
    return m


def _swap_rows(vd, S):
    j = S // 2 - 1 if S > 2 else 0
    perm = list(range(S))
    perm[j], perm[j + 1] = perm[j + 1], perm[j]
    return vd[:, :, perm]


def model_fwd(q, k, v, N, S, H, dk, dv, table, index, keep, p_drop, dt=torch.float64, rounding=True, round_out=False, mutant=None):
    """(P [N, H, S, S], O [N S, H d_v], bound of O) in the arithmetic ``dt``.  ``rounding``: the bf16 rounding of Pd;
    ``round_out``: the output's rounding too (the kernel's own last step, which the f64 reference leaves to the bars)."""
    qd, kd, vd = (_heads(t, N, S, H, dt) for t in (q, k, v))
    a = torch.matmul(qd, kd.transpose(-1, -2)) * _scale(dk)
    if table is not None and S > 1:
        ix = index[: S - 1, : S - 1].reshape(-1).to(table.device)
        bias = table.detach().to(dt)[ix].view(S - 1, S - 1, H).permute(2, 0, 1)
        a = a + torch.nn.functional.pad(bias, (1, 0, 1, 0))
    p = torch.softmax(a, -1)
    kf = _keep_factor(keep, p_drop, dt, mutant)
    pd = p if kf is None else p * kf
    if rounding:
        pd = bf16(pd)
    pd = _lose(pd, S, mutant)
    if mutant == "vswap":
        vd = _swap_rows(vd, S)
    o, bound = torch.matmul(pd, vd), torch.matmul(pd.abs(), vd.abs())
    if round_out:
        o = bf16(o)
    return p, _merge(o), _merge(bound)


def model_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, keep, p_drop, dt=torch.float64, rounding=True, round_out=False,
              mutant=None):
    """((dQ, bound), (dK, bound), (dV, bound), dtable or None) on the given P ([N, H, S, S]) in the arithmetic ``dt``."""
    qd, kd, vd, dod = (_heads(t, N, S, H, dt) for t in (q, k, v, do))
    p = probs.detach().to(dt)
    scale = _scale(dk)
    dp = torch.matmul(dod, (_swap_rows(vd, S) if mutant == "vswap" else vd).transpose(-1, -2))
    kf = _keep_factor(keep, p_drop, dt, mutant)
    dpk = dp if kf is None else dp * kf
    rs = ((dp if mutant == "rs_nokeep" else dpk) * p).sum(-1, keepdim=True)
    da = p * (dpk - rs)
    dtable = None
    if table is not None:
        dtable = torch.zeros(table.shape[0], H, dtype=dt, device=p.device)
        if S > 1:
            ix = index[: S - 1, : S - 1].reshape(-1).to(p.device)
            dtable.index_add_(0, ix, da[:, :, 1:, 1:].sum(0).permute(1, 2, 0).reshape(-1, H))
    pd = p if kf is None else p * kf
    if rounding:
        da, pd = bf16(da), bf16(pd)
    da, pd = _lose(da, S, mutant), _lose(pd, S, mutant)
    dq = torch.matmul(da, kd) * (1.0 if mutant == "dq_unscaled" else scale)
    bq = torch.matmul(da.abs(), kd.abs()) * scale
    dk_ = torch.matmul(da.transpose(-1, -2), qd) * scale
    bk = torch.matmul(da.abs().transpose(-1, -2), qd.abs()) * scale
    dv_ = torch.matmul(pd.transpose(-1, -2), dod)
    bv = torch.matmul(pd.abs().transpose(-1, -2), dod.abs())
    if round_out:
        dq, dk_, dv_ = bf16(dq), bf16(dk_), bf16(dv_)
    return (_merge(dq), _merge(bq)), (_merge(dk_), _merge(bk)), (_merge(dv_), _merge(bv)), dtable


def written_probs(p64, probs_ld=None):
    """The P a backward test writes: the f32 of the f64 softmax in a zeroed buffer of pitch ``probs_ld`` (default: S rounded up to
    4).  Returns (the buffer [N, H, S, probs_ld], its [N, H, S, S] view)."""
    N, H, S, _ = p64.shape
    pld = (S + 3) // 4 * 4 if probs_ld is None else probs_ld
    buf = torch.zeros(N, H, S, pld, device=p64.device)
    buf[..., :S] = p64.float()
    return buf, buf[..., :S]


# ---------------------------------------------------------------------------------------------------- bars

def bar_table(ref):
    return 2e-5 * float(ref.abs().max()) + 1e-6


def measure(got, ref, bound, S):
    """(stat, worst excess / bound, share) of one of O, dQ, dK, dV ([N S, cols]) against the model and its bound; None for a
    reference that is zero everywhere.  A token index, or an element, whose reference (bound) is zero counts only if the result
    there is not: then it is infinitely far."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    if float(ref.abs().max()) == 0.0:
        return None
    err = got - ref
    num = err.view(-1, S, err.shape[1]).pow(2).sum((0, 2)).sqrt()
    den = ref.view(-1, S, ref.shape[1]).pow(2).sum((0, 2)).sqrt()
    stat = float(torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, float("inf"), 0.0).to(num.dtype)).max())
    excess = err.abs() - BAR_STAT * ref.abs()
    ratio = torch.where(bound > 0, excess / bound.clamp_min(1e-300), torch.where(excess > 0, float("inf"), 0.0).to(excess.dtype))
    return stat, float(ratio.max()), float((excess > EXCESS_FLOOR * bound).double().mean())


WORST = {}      # (section, what) -> (err / bar, err, bar, case)


def _dump():
    path = os.environ.get("LSTC_ATTN_PACKED_ERRORS")
    if path and WORST:
        with open(path, "w") as f:
            f.write(f"{'section':<34} {'what':<14} {'worst':<13} {'bar':<12} {'err/bar':<8} at\n")
            for (sec, name), (r, e, b, case) in sorted(WORST.items()):
                f.write(f"{sec:<34} {name:<14} {e:<13.3e} {b:<12.3e} {r:<8.3f} {case}\n")


atexit.register(_dump)


def record(section, name, err, b, case):
    r = err / b
    if (section, name) not in WORST or r > WORST[(section, name)][0]:
        WORST[(section, name)] = (r, err, b, case)


def check_probs(section, got, p64, case, factor=1.0):
    got = got.double()
    assert got.shape == p64.shape and bool(torch.isfinite(got).all()), (section, case, "P")
    err = float((got - p64).abs().max())
    record(section, "P", err, BAR_P, case)
    assert err <= factor * BAR_P, (section, case, "P", err)


def check_out(section, name, got, ref, bound, S, case, factor=1.0):
    """One of O, dQ, dK, dV under the three bars (``factor``: the share of each bar allowed - the host twin asks for half)."""
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (section, case, name)
    m = measure(got, ref, bound, S)
    if m is None:
        assert float(got.abs().max()) == 0.0, (section, case, name, "a reference that is zero everywhere demands exact zeros")
        return
    bad = {}
    for what, val, b in zip(("stat", "excess", "share"), m, (BAR_STAT, BAR_EXCESS, BAR_SHARE)):
        record(section, f"{name} {what}", val, b, case)
        if not val <= factor * b:
            bad[what] = (val, factor * b)
    assert not bad, (section, case, name, "value > bar", bad)


def check_table(section, got, ref, case, factor=1.0):
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (section, case, "dtable")
    err, b = float((got - ref).abs().max()), bar_table(ref)
    record(section, "dtable", err, b, case)
    assert err <= factor * b, (section, case, "dtable", err, b)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------- packs and raw calls

def pack(t):
    """lstc_pack1 of an f32 [rows, K] matrix (K a multiple of 64, rows of 256: the pack has no padding): its bytes."""
    assert t.shape[0] % 256 == 0 and t.shape[1] % 64 == 0
    return Fn().pack3(t.contiguous(), False, kind=L().BF16P).buf


def pack_bytes(rows, K):
    return int(L().load().lstc_pack1_bytes(rows, K))


def empty_pack(rows, K, fill=0xFF):
    """An output pack whose every bf16 is 0xFFFF (a NaN) until it is written."""
    return torch.full((pack_bytes(rows, K),), fill, device="cuda", dtype=torch.uint8)


def unpack(buf, rows, K, col0=0, cols=None):
    """f32 values of columns col0 .. col0 + cols of an lstc_pack1 buffer of a [rows, K] matrix."""
    from test_hip_parity import _unpack1
    full = _unpack1(buf, rows, K)
    return full[:, col0: col0 + (K - col0 if cols is None else cols)].contiguous()


def default_npw(N, S, H):
    """Sequences per workgroup the launchers of the packed-input kernels pick (csrc/attention.hip attn_fwd / attn_bwd)."""
    return min(16, max(1, (N * H) // (8192 if S <= 32 else 1024)))


def bwd3_lds(T, table_rows):
    """Dynamic LDS of attn_bwd3_kernel<T, NB> in bytes (csrc/attention_pk.hip bwd3_go: the ring of NB slots of two [32 T][64 B]
    halves, the [32 T][72 B] transposition image, T per-wave tables), NB as attn3_bwd_launch picks it."""
    return {1: 9, 2: 8, 3: 5}[T] * 2 * (32 * T) * 64 + (32 * T) * 72 + T * table_rows * 4


def bwd_lds(T, table_rows):
    """The first generation's footprint, which lstc_attn_bwd holds every S <= 128 call to before it picks a kernel."""
    return (2 * (32 * T) * (32 * T + 1) + 4 * table_rows) * 4


def chunks_for(N, npw):
    """dtable_chunks that makes lstc_attn_bwd walk ``npw`` sequences per workgroup (it derives ceil(N / chunks) and refuses a
    count that does not come back)."""
    chunks = -(-N // npw)
    assert -(-N // (-(-N // chunks))) == chunks, (N, npw)
    return chunks


def _desc3(qkv, N, S, H, dk, dv, table, index, seed, p_drop, in_cols, col0, variant):
    lib = L()
    ops = (qkv,) * 3 if torch.is_tensor(qkv) else tuple(qkv)
    d = lib.AttnDesc()
    d.N, d.S, d.H, d.dk, d.dv = N, S, H, dk, dv
    d.dtype = lib.BF16
    if table is not None:
        assert table.dtype == torch.float32 and index.dtype == torch.int64 and index.is_contiguous()
        d.index_ld, d.table_rows = index.shape[1], table.shape[0]
        d.table, d.index = table.data_ptr(), index.data_ptr()
    d.scale = 1.0 / (dk ** 0.5)
    d.dropout_p, d.dropout_seed = float(p_drop), int(seed)
    d.Q, d.K, d.V = (t.data_ptr() for t in ops)
    d.in_pack_cols = H * (2 * dk + dv) if in_cols is None else in_cols
    d.Q_col0, d.K_col0, d.V_col0 = (0, H * dk, 2 * H * dk) if col0 is None else col0
    for t in ops:       # every operand pack holds whole 128-row blocks of in_pack_cols columns
        assert t.is_cuda and t.dtype == torch.uint8 and t.numel() == pack_bytes(N * S, d.in_pack_cols)
    d.variant = variant
    return d


def raw_fwd3(qkv, N, S, H, dk, dv, table, index, seed, *, in_cols=None, col0=None, probs_ld=None, variant=0, p_drop=P_DROP):
    """lstc_attn_fwd on packed operands through a descriptor built here.  ``qkv``: one pack holding the three column blocks at
    ``col0`` of its ``in_cols`` columns (default: the fused layout), or three packs of ``in_cols`` columns each.  Returns (the
    probability buffer [N, H, S, probs_ld], NaN where nothing was written; the O pack, 0xFFFF where nothing was written)."""
    lib = L()
    pld = (S + 3) // 4 * 4 if probs_ld is None else probs_ld
    probs = torch.full((N, H, S, pld), float("nan"), device="cuda")
    o = empty_pack(N * S, H * dv)
    d = _desc3(qkv, N, S, H, dk, dv, table, index, seed, p_drop, in_cols, col0, variant)
    d.O_pack, d.ldo, d.probs, d.probs_ld = o.data_ptr(), H * dv, probs.data_ptr(), pld
    lib.check(lib.load().lstc_attn_fwd(C.byref(d), lib.stream_ptr()), "lstc_attn_fwd")
    torch.cuda.synchronize()
    return probs, o


def raw_bwd3(do, qkv, probs, N, S, H, dk, dv, table, index, seed, *, in_cols=None, col0=None, do_cols=None, do0=0, pack_cols=None,
             out_col0=None, out=None, table_grad="parts", chunks=None, variant=0, p_drop=P_DROP):
    """lstc_attn_bwd on packed operands through a descriptor built here.  ``probs``: the buffer [N, H, S, probs_ld].  ``do``: a
    pack of ``do_cols`` columns (default H d_v) with dO at column ``do0``.  Outputs: ``pack_cols`` > 0 (default: the fused
    H (2 d_k + d_v)) - ONE pack, ``out`` or a fresh one, the blocks at ``out_col0``; ``pack_cols`` = 0 - three packs.
    ``table_grad``: "parts" (``chunks`` partial tables, default the launcher's own sequences per workgroup; summed here in f64),
    "atomic" (dtable_chunks = 0 into a zeroed table) or None (dtable = NULL).  Returns (the tuple of output packs, dtable)."""
    lib = L()
    M = N * S
    assert probs.is_contiguous() and probs.shape[:3] == (N, H, S)
    d = _desc3(qkv, N, S, H, dk, dv, table, index, seed, p_drop, in_cols, col0, variant)
    d.dO, d.dO_pack_cols, d.dO_col0 = do.data_ptr(), H * dv if do_cols is None else do_cols, do0
    assert do.numel() == pack_bytes(M, d.dO_pack_cols)
    d.probs, d.probs_ld = probs.data_ptr(), probs.shape[3]
    fused = H * (2 * dk + dv)
    pack_cols = fused if pack_cols is None else pack_cols
    if pack_cols > 0:
        outs = (empty_pack(M, pack_cols) if out is None else out,) * 3
        assert outs[0].numel() == pack_bytes(M, pack_cols)
        d.pack_cols = pack_cols
        d.dQ_col0, d.dK_col0, d.dV_col0 = (0, H * dk, 2 * H * dk) if out_col0 is None else out_col0
    else:
        outs = (empty_pack(M, H * dk), empty_pack(M, H * dk), empty_pack(M, H * dv))
    d.dQ_pack, d.dK_pack, d.dV_pack = (t.data_ptr() for t in outs)
    dtab = None
    if table is not None and table_grad is not None:
        if table_grad == "parts":
            chunks = chunks_for(N, default_npw(N, S, H)) if chunks is None else chunks
            dtab = torch.full((chunks, table.shape[0], H), float("nan"), device="cuda")
            d.dtable_chunks = chunks
        else:
            dtab = torch.zeros(1, table.shape[0], H, device="cuda")
        d.dtable = dtab.data_ptr()
    lib.check(lib.load().lstc_attn_bwd(C.byref(d), lib.stream_ptr()), "lstc_attn_bwd")
    torch.cuda.synchronize()
    if dtab is not None:
        dtab = dtab.double().sum(0)
    return (outs if pack_cols == 0 else outs[:1]), dtab
