"""Attention operands whose logits are EXACT in every arithmetic the kernels use and span [-32640, +65280] at S = 512: the recipe of
tests/test_softmax_range_host.py and tests/test_softmax_range_gpu.py.

The suite's other attention inputs (randn, scale 1 / sqrt(d_k), table * 0.4) keep every logit within about +-6, where softmax's
shift invariance makes the row maximum numerically irrelevant.  Here, for query row i with peak key j*(i),

    logit(i, j) = scale * (2 j* j - j^2 + r_i),    r_i = s_i j*^2,  s_i = -1, 0, +1 cycling over the rows,  scale = 1 / 8

(the rows counted through the whole case, (n, h, i) flat: a one-row case such as the CLS query cycles over its (n, h))

which is -(j - j*)^2 / 8 plus the row constant (1 + s_i) j*^2 / 8: a soft peak about +-6 keys wide, exact zeros in P beyond about
27 keys (expf underflows), and neighbouring rows whose maxima differ by tens of thousands.

Exactness.  Q carries (2 j*, -1, r_i) and K carries (j, j^2, 1).  Every integer is split into 8-bit chunks times 2^0, 2^8, 2^16 and
every chunk product gets its own feature column (4 + 3 + 3 = 10 columns, at seeded positions of d_k >= 16; the rest is zero).  An
operand entry is a chunk times a power of two - at most 8 significant bits - so it survives RNE to bf16, a product of two entries
has at most 16 bits, and every partial sum in any order is an integer below 2^24 (times 1 / 8 where Q was scaled first).  The f32
arms, the RNE-to-bf16 arms and the packed bf16 arms therefore contract the same integers; only expf, the sum and the division
round.  ``build`` asserts all of it on the host.  The "sharp" variant multiplies Q by 16 (neighbours of the peak at -2), S <= 129.

The relative bias is integers / 8 with |value| < 32 (the bound of csrc/attention_common.h under which -1e9f + bias rounds back to
-1e9f); logit + bias stays on the 1 / 8 grid below 2^24 / 8.

``formulas`` states the attention contract (include/lstc_hip.h) in one arithmetic, float64 or float32, with the |term| sums that
util_rowops.tol takes; the host file holds its float64 form against the suite's references.  ``MISTAKES`` are float32 row
softmaxes with one seeded mistake each."""
import atexit
import math
import os
import types

import torch

SCALE = 0.125
P_DROP = 0.2
F64, F32 = torch.float64, torch.float32


# ---------------------------------------------------------------------------------------------------- peaks

def multiplier(Sk):
    """The smallest m >= 7 coprime to Sk: row g -> (m g + c) mod Sk visits every key in Sk consecutive rows."""
    m = 7
    while math.gcd(m, Sk) != 1:
        m += 1
    return m


def peaks_rows(N, H, Sq, Sk, c=0):
    """j*(n, h, i) = (m (i + Sq (h + H n)) + c) mod Sk -> int64 [N, H, Sq]; neighbouring rows peak m keys apart."""
    g = torch.arange(N * H * Sq, dtype=torch.int64).view(N, H, Sq)
    return (multiplier(Sk) * g + c) % Sk


def edge_keys(S):
    """Key 0, key S - 1 and both sides of every 32-key edge (which holds every 64-key edge) below S."""
    e = {0, S - 1}
    for b in range(32, S, 32):
        e.update((b - 1, b))
    return sorted(e)


def peaks_edges(N, H, Sq, Sk):
    """The rows' peaks cycle through ``edge_keys(Sk)`` -> int64 [N, H, Sq] (the few-row kernels: CLS query, few-query)."""
    e = torch.tensor(edge_keys(Sk), dtype=torch.int64)
    return e[torch.arange(N * H * Sq) % len(e)].view(N, H, Sq)


def rows_for_edges(Sk, H, Sq=1):
    """The smallest N >= 2 at which N H Sq rows hold every edge key."""
    return max(2, -(-len(edge_keys(Sk)) // (H * Sq)))


# ---------------------------------------------------------------------------------------------------- operands

def _chunks(x, n):
    """Non-negative int64 -> n 8-bit chunks, least significant first."""
    return [(x >> (8 * c)) & 255 for c in range(n)]


def build(N, H, Sq, Sk, dk, seed, peaks=None, sharp=False, shared_k=False, coverage="all"):
    """-> namespace(q [N, H, Sq, dk] f32 (NOT scaled), k [N, H, Sk, dk] f32, logits8 int64 [N, H, Sq, Sk] = logit / scale,
    peaks, s [N, H, Sq]).  ``shared_k``: one set of columns for every head and K the same for every head (the CLS passes read one
    token matrix).  ``coverage``: "all" - every key is some row's peak; "edges" - ``edge_keys(Sk)`` all are; None - no demand."""
    assert dk >= 16 and (not sharp or max(Sq, Sk) <= 129)
    peaks = peaks_rows(N, H, Sq, Sk) if peaks is None else peaks
    assert peaks.shape == (N, H, Sq) and int(peaks.min()) >= 0 and int(peaks.max()) < Sk
    hit = set(peaks.reshape(-1).tolist())
    if coverage == "all":
        assert hit == set(range(Sk)), ("not every key is a peak", Sk, len(hit))
    elif coverage == "edges":
        assert set(edge_keys(Sk)) <= hit, ("an edge key is no peak", Sk)
    s = (torch.arange(N * H * Sq, dtype=torch.int64).view(N, H, Sq) % 3) - 1      # over the flat row: one-row cases cycle too
    j = torch.arange(Sk, dtype=torch.int64)
    a, r = 2 * peaks, s * peaks * peaks
    a0, a1 = _chunks(a, 2)
    r0, r1, r2 = _chunks(r.abs(), 3)
    sg = r.sign()
    j0, j1 = _chunks(j, 2)
    c0, c1, c2 = _chunks(j * j, 3)
    one, e8, e16 = torch.ones_like(j), 256, 65536
    m1 = -torch.ones_like(a)
    qcols = [a0, a0 * e8, a1 * e8, a1 * e16, m1, m1 * e8, m1 * e16, sg * r0, sg * r1 * e8, sg * r2 * e16]
    kcols = [j0, j1, j0, j1, c0, c1, c2, one, one, one]
    amp = 16 if sharp else 1
    q = torch.zeros(N, H, Sq, dk, dtype=F64)
    k = torch.zeros(N, H, Sk, dk, dtype=F64)
    g = torch.Generator().manual_seed(seed)
    for h in range(H):
        if h == 0 or not shared_k:
            pos = torch.randperm(dk, generator=g)[: len(qcols)]
        for p, qc, kc in zip(pos.tolist(), qcols, kcols):
            q[:, h, :, p] = (amp * qc[:, h]).to(F64)
            k[:, h, :, p] = kc.to(F64)
    want = amp * (a.unsqueeze(-1) * j - j * j + r.unsqueeze(-1))                      # int64 [N, H, Sq, Sk]
    c = types.SimpleNamespace(q=q.float(), k=k.float(), logits8=want, peaks=peaks, s=s, N=N, H=H, Sq=Sq, Sk=Sk, dk=dk, sharp=sharp)
    verify(c)
    if Sk >= 33:        # some row maximum (1 + s) j*^2 / 8 lies above 88, where expf without the maximum overflows
        assert float(want.max()) * SCALE / amp > 88.0, ("no row maximum above 88", Sq, Sk, float(want.max()) * SCALE)
    return c


def cls_build(S, H, dm=64, N=None):
    """The one-row case of the CLS-query kernels and the cls_dot passes: N sequences (default: the fewest that hold every edge
    key), the peaks over (n, h) at ``edge_keys(S)``, one token matrix for all heads."""
    N = rows_for_edges(S, H) if N is None else N
    return build(N, H, 1, S, dm, seed=13 * S, peaks=peaks_edges(N, H, 1, S), shared_k=True, coverage="edges")


def few_build(Sq, Sk, H):
    """The case of the few-query kernels: Sq <= 16 rows per (n, h), the peaks cycling through ``edge_keys(Sk)``."""
    N = rows_for_edges(Sk, H, Sq)
    return build(N, H, Sq, Sk, 64, seed=Sq + 3 * Sk, peaks=peaks_edges(N, H, Sq, Sk), coverage="edges")


def verify(c):
    """Host assertions of the recipe: every operand entry survives a bf16 round trip; the float32 CPU product under three
    different column permutations equals the float64 product bit for bit; both are the intended integer matrix; the same for
    the operands scaled first (Q / 8)."""
    for t in (c.q, c.k):
        assert torch.equal(t.bfloat16().float(), t), "an operand entry has more than 8 significant bits"
    want = c.logits8.to(F64)
    assert float(want.abs().max()) < 2.0 ** 24
    p64 = torch.matmul(c.q.double(), c.k.double().transpose(-1, -2))
    assert torch.equal(p64, want), "the float64 product is not the intended integer matrix"
    g = torch.Generator().manual_seed(c.dk)
    for perm in (torch.arange(c.dk), torch.arange(c.dk).flip(0), torch.randperm(c.dk, generator=g)):
        p32 = torch.matmul(c.q[..., perm], c.k[..., perm].transpose(-1, -2))
        assert p32.dtype == F32 and torch.equal(p32.double(), want), "a float32 summation order is not exact"
        s32 = torch.matmul(c.q[..., perm] * SCALE, c.k[..., perm].transpose(-1, -2))
        assert torch.equal(s32.double(), want * SCALE), "the pre-scaled float32 product is not exact"


def rows(t):
    """[N, H, S, d] -> the row-operand layout [N S, H d]."""
    N, H, S, d = t.shape
    return t.transpose(1, 2).reshape(N * S, H * d).contiguous()


def heads(t, N, S, H):
    """[N S, H d] -> [N, H, S, d]."""
    return t.reshape(N, S, H, -1).transpose(1, 2)


def values(N, H, Sq, Sk, dv, seed):
    """V [N, H, Sk, dv] and dO [N, H, Sq, dv] ~ randn."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, H, Sk, dv, generator=g), torch.randn(N, H, Sq, dv, generator=g)


def bias_table(S, H, seed, index_rows):
    """table [rows, H]: integers in [-255, 255] / 8 (|value| < 32, 8 significant bits)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-255, 256, (index_rows, H), generator=g).float() / 8.0
    assert float(t.abs().max()) < 32 and torch.equal(t.bfloat16().float(), t)
    return t


def gather_bias(table, index, S):
    """[H, S, S] bias of the contract: table[index[i - 1, j - 1], h] on the lower-right (S - 1)^2 corner, 0 on row and column 0."""
    H = table.shape[1]
    if S == 1:
        return torch.zeros(H, 1, 1, dtype=table.dtype, device=table.device)
    ix = index[: S - 1, : S - 1].reshape(-1).to(table.device)
    return torch.nn.functional.pad(table[ix].view(S - 1, S - 1, H).permute(2, 0, 1), (1, 0, 1, 0))


def peak_mask(peaks, Sk, halfwidth=3):
    """bool [N, H, Sq, Sk], True = kept: every second row (i + n odd, so that one-row cases alternate over the sequences) loses its
    peak and the peak's +-``halfwidth`` neighbours, so the raw logits under the mask exceed the row's kept maximum."""
    N, H, Sq = peaks.shape
    j = torch.arange(Sk).view(1, 1, 1, Sk)
    near = (j - peaks.unsqueeze(-1)).abs() <= halfwidth
    odd = ((torch.arange(Sq).view(1, 1, Sq, 1) + torch.arange(N).view(N, 1, 1, 1)) % 2 == 1)
    return ~(near & odd)


# ---------------------------------------------------------------------------------------------------- the contract, one arithmetic

def formulas(q, k, v, do, scale, dtype, bias=None, kept=None, keep=None, p_drop=0.0):
    """The attention contract in the arithmetic ``dtype`` with plain torch ops: q [N, H, Sq, dk], k [N, H, Sk, dk], v [N, H, Sk,
    dv], do [N, H, Sq, dv] or None; ``bias`` [H, Sq, Sk]; ``kept`` bool, broadcasts against [N, H, Sq, Sk] (False: the logit is
    -1e9, no gradient to q . k, the bias gradient still flows); ``keep`` the dropout mask.  Returns a dict: P, O, dQ, dK, dV,
    dbias [H, Sq, Sk] and, under "terms", the sums of |terms| of dQ, dK, dbias (util_rowops.tol's ``terms_abs``)."""
    q, k, v = (t.to(dtype) for t in (q, k, v))
    a = torch.matmul(q * scale, k.transpose(-1, -2))
    if bias is not None:
        a = a + bias.to(dtype)
    if kept is not None:
        kept = kept.to(a.device).expand(a.shape)
        a = torch.where(kept, a, torch.full_like(a, -1e9))
    p = torch.softmax(a, -1)
    kf = keep.to(dtype) / (1.0 - p_drop) if keep is not None and p_drop > 0 else None
    pd = p if kf is None else p * kf
    out = {"P": p, "O": torch.matmul(pd, v)}
    if do is None:
        return out
    do = do.to(dtype)
    dp = torch.matmul(do, v.transpose(-1, -2))
    dpk = dp if kf is None else dp * kf
    rs = (dpk * p).sum(-1, keepdim=True)
    da = p * (dpk - rs)
    daq = da if kept is None else torch.where(kept, da, torch.zeros_like(da))
    out.update(dV=torch.matmul(pd.transpose(-1, -2), do), dQ=torch.matmul(daq, k) * scale,
               dK=torch.matmul(daq.transpose(-1, -2), q) * scale, dbias=da.sum(0))
    out["terms"] = {"dQ": torch.matmul(daq.abs(), k.abs()) * scale, "dK": torch.matmul(daq.abs().transpose(-1, -2), q.abs()) * scale,
                    "dbias": da.abs().sum(0)}
    return out


def table_grad(dbias, index, table_rows):
    """[H, S, S] bias gradient -> [rows, H] table gradient (index_add over the lower-right corner)."""
    H, S, _ = dbias.shape
    out = torch.zeros(table_rows, H, dtype=dbias.dtype, device=dbias.device)
    if S > 1:
        ix = index[: S - 1, : S - 1].reshape(-1).to(dbias.device)
        out.index_add_(0, ix, dbias[:, 1:, 1:].permute(1, 2, 0).reshape(-1, H))
    return out


# ---------------------------------------------------------------------------------------------------- seeded mistakes (float32)

def softmax_ok(a, kept=None):
    if kept is not None:
        a = torch.where(kept, a, torch.full_like(a, -1e9))
    m = a.max(-1, keepdim=True).values
    e = torch.exp(a - m)
    return e / e.sum(-1, keepdim=True)


def _no_max(a, kept=None):
    e = torch.exp(a)
    return e / e.sum(-1, keepdim=True)


def _max_first_32(a, kept=None):
    m = a[..., :32].max(-1, keepdim=True).values
    e = torch.exp(a - m)
    return e / e.sum(-1, keepdim=True)


def _max_per_half(a, kept=None):
    """Lanes 0 .. 31 hold the keys with j mod 64 < 32, lanes 32 .. 63 the others; each half shifts by its own maximum (the
    exchange between the halves is lost), the sum is the common one."""
    S = a.shape[-1]
    half = (torch.arange(S) // 32) % 2 == 1
    if not bool(half.any()):
        return softmax_ok(a)
    neg = torch.full_like(a, float("-inf"))
    m0 = torch.where(~half, a, neg).max(-1, keepdim=True).values
    m1 = torch.where(half, a, neg).max(-1, keepdim=True).values
    e = torch.exp(a - torch.where(half, m1, m0))
    return e / e.sum(-1, keepdim=True)


def _online_no_rescale(a, kept=None):
    """Online max / sum over 32-key tiles; the running sum is NOT rescaled by expf(m - mn) when the maximum rises."""
    S = a.shape[-1]
    m = torch.full_like(a[..., :1], float("-inf"))
    l = torch.zeros_like(m)
    for t0 in range(0, S, 32):
        tile = a[..., t0: t0 + 32]
        m = torch.maximum(m, tile.max(-1, keepdim=True).values)
        l = l + torch.exp(tile - m).sum(-1, keepdim=True)
    return torch.exp(a - m) / l


def _fill_after_max(a, kept):
    """The maximum is taken over the raw logits; the mask fill comes after it."""
    m = a.max(-1, keepdim=True).values
    e = torch.exp(torch.where(kept, a, torch.full_like(a, -1e9)) - m)
    return e / e.sum(-1, keepdim=True)


MISTAKES = {"a no maximum": _no_max, "b maximum of the first 32 keys": _max_first_32, "c maximum per lane half": _max_per_half,
            "d online sum not rescaled": _online_no_rescale, "e mask fill after the maximum": _fill_after_max}


def failed_rows(p, ref64, bar=2e-6):
    """Rows of ``p`` with a non-finite value or farther than ``bar`` from the float64 rows -> bool [..., rows]."""
    p = p.double()
    return ~torch.isfinite(p).all(-1) | ((p - ref64).abs().nan_to_num(posinf=1.0).max(-1).values > bar)


# ---------------------------------------------------------------------------------------------------- recording

WORST = {}      # (arm, what) -> (err / bar, err, bar, case)


def _dump():
    path = os.environ.get("LSTC_SOFTMAX_RANGE_ERRORS")
    if path and WORST:
        with open(path, "w") as f:
            f.write(f"{'arm':<34} {'what':<8} {'max|err|':<13} {'bar':<12} {'err/bar':<8} at\n")
            for (arm, name), (r, e, b, case) in sorted(WORST.items()):
                f.write(f"{arm:<34} {name:<8} {e:<13.3e} {b:<12.3e} {r:<8.3f} {case}\n")


atexit.register(_dump)


def record(arm, name, err, b, case):
    r = err / b
    if (arm, name) not in WORST or r > WORST[(arm, name)][0]:
        WORST[(arm, name)] = (r, err, b, case)


def bar(name, ref):
    """The project's bars against float64 (tests/test_attention_sweep_gpu.py, util_mask.bar)."""
    return 2e-6 if name == "P" else 2e-5 * float(ref.abs().max()) + 1e-6


def check(arm, name, got, ref, case, b=None):
    """``got`` finite and within ``b`` (default: the project's bar) of the float64 ``ref``; the figure is printed and recorded
    before the assertion."""
    got = got.double()
    assert got.shape == ref.shape, (arm, case, name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (arm, case, name, "non-finite")
    err = float((got - ref.to(got.device)).abs().max())
    b = bar(name, ref) if b is None else b
    record(arm, name, err, b, case)
    print(f"{arm} {case} {name}: {err:.3e} / {b:.3e}")
    assert err <= b, (arm, case, name, err, b)
