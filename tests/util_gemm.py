"""References of the GEMM kernels (csrc/gemm_f32.hip, gemm_bf16c.hip, gemm_pk.hip, gemm_bf16p.hip) and of lstc_splitk_finish in
plain numpy / torch, the four input families and the case tables the GPU file runs.  No project kernel is called here:
tests/test_gemm_ref_host.py checks these functions on the CPU (fma32 against libm's fmaf, the tolerance rule against a second
summation order for every listed case) before tests/test_gemm_f64_gpu.py checks the kernels against them.

The tolerance is util_rowops.tol, reused: per output tensor 8 * max(e32, 4 * 2**-24 * B), e32 the error of a plain torch float32
evaluation (a @ b plus the epilogue in float32) on the same operands, B the largest sum of |terms| added into one output element."""
import numpy as np
import torch

from util_rowops import EPS32, tol  # noqa: F401  (tol and EPS32 are re-exported: one rule, not restated)

F64, F32 = torch.float64, torch.float32
LSTC_F32, LSTC_BF16, LSTC_F32X3, LSTC_BF16P = 0, 1, 2, 3
BIAS, RELU, DROPOUT, RESIDUAL, RELU_MASK, ACCUM, OUT_F32 = 1, 2, 4, 8, 16, 32, 64
OUT_PACK, RELU_MASK_PACK, RESIDUAL_PACK = 128, 256, 512
NO_QTAIL = 1 << 30
DTYPE_NAMES = {LSTC_F32: "f32", LSTC_BF16: "bf16c", LSTC_F32X3: "f32x3", LSTC_BF16P: "bf16p"}


# ------------------------------------------------------------------------------------------- fused multiply-add
def fma32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, vectorised over float32 arrays (numpy broadcasting).

    The product of two float32 is exact in float64 (48 bits).  TwoSum gives s = RN64(p + c) and the exact remainder e; where
    e != 0 and the last bit of s is even, s moves one ulp toward e - round to odd - and a float64 rounded to odd rounds to
    float32 (53 >= 2 * 24 + 2 bits) as the exact sum would.  A plain float64(a * b + c).astype(float32) rounds twice and differs
    whenever the exact sum sits within a float64 ulp of a float32 tie."""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy() if s.ndim else np.array(s).view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (e > 0) == (s > 0)                       # the remainder points away from zero: the magnitude grows by one ulp
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def fmaf_chain(A, B, rows=None, cols=None, order=None):
    """acc = 0; for k in ``order`` (default 0 .. K-1): acc = fma32(A[:, k], B[k, :], acc), for A [M, K] and B [K, N] float32.
    ``rows`` / ``cols``: index arrays - only that sub-block of the product is formed (a large product checked on chosen rows).
    Returns float32 [len(rows), len(cols)]."""
    A = np.asarray(A, dtype=np.float32)
    B = np.asarray(B, dtype=np.float32)
    if rows is not None:
        A = A[np.asarray(rows)]
    if cols is not None:
        B = B[:, np.asarray(cols)]
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k in (range(A.shape[1]) if order is None else order):
        acc = fma32(A[:, k][:, None], B[k, :][None, :], acc)
    return acc


def mfma_issue_order(K, bk=32):
    """The k order in which csrc/gemm_f32.hip feeds one output element's accumulator, in every variant (they share read_frag): inside every 32-deep K tile the lane halves
    of v_mfma_f32_32x32x2_f32 hold k = j and k = 16 + j (read_frag: 16 h + 8 half + j), issue by issue j = 0 .. 7, then 8 .. 15:
    0, 16, 1, 17, ... 7, 23, 8, 24, ... 15, 31.  A zero-filled K tail contributes fma(0, 0, acc) = acc and is left out."""
    out = []
    for t0 in range(0, K, bk):
        for half in (0, 1):
            for j in range(8):
                for h in (0, 1):
                    k = t0 + 16 * h + 8 * half + j
                    if k < K:
                        out.append(k)
    return out


# ------------------------------------------------------------------------------------------- number formats
def bf16_round(x):
    """float32 -> bfloat16 (round to nearest even) -> float32, through torch.bfloat16."""
    return torch.as_tensor(x, dtype=F32).to(torch.bfloat16).to(F32)


def bf16_round_bits(x):
    """The same rounding restated on the bit pattern (finite inputs): add 0x7fff + the kept part's last bit, clear the low half."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def pack3_scale(x):
    """The power of two lstc_pack3 scales a tensor by: absmax lands in [2**14, 2**15) (1 for an all-zero tensor)."""
    m = float(torch.as_tensor(x).abs().max())
    if m == 0.0:
        return 1.0
    return 2.0 ** (14 - int(np.floor(np.log2(m))))


def pack3_planes(x):
    """(h, l, s): h = f16(x s), l = f16(x s - h) as float64 tensors, s = pack3_scale(x).  x s and x s - h are exact in float32."""
    x = torch.as_tensor(x, dtype=F32)
    s = pack3_scale(x)
    xs = x * s
    h = xs.to(torch.float16).to(F32)
    l = (xs - h).to(torch.float16).to(F32)
    return h.to(F64), l.to(F64), s


def pack3_emulation(A, B):
    """What the f32x3 format itself can deliver for A [M, K] @ B [K, N], in float64: the three plane products csrc/gemm_pk.hip forms
    (hh, hl, lh - the l l product is the one left out), summed in float64 and unscaled by 1 / (s_a s_b)."""
    ah, al, sa = pack3_planes(A)
    bh, bl, sb = pack3_planes(B)
    return (ah @ bh + ah @ bl + al @ bh) / (sa * sb)


# ------------------------------------------------------------------------------------------- product + epilogue
def epilogue(acc, flags=0, alpha=1.0, bias=None, keep=None, p=0.0, residual=None, relu_src=None, c_old=None):
    """The header's order on an accumulator tensor of any float dtype: v = alpha acc; += bias; relu; dropout (``keep`` [M, N] bool,
    kept values times 1 / (1 - p)); += residual; *= (relu_src > 0); then store, or += old C with ACCUM."""
    dt = acc.dtype
    v = acc * torch.tensor(alpha, dtype=dt)
    if flags & BIAS:
        v = v + bias.to(dt)[None, :]
    if flags & RELU:
        v = torch.clamp_min(v, 0.0)
    if flags & DROPOUT:
        scale = torch.tensor(1.0, dtype=dt) / (torch.tensor(1.0, dtype=dt) - torch.tensor(p, dtype=F32).to(dt))
        v = torch.where(keep, v * scale, torch.zeros((), dtype=dt))
    if flags & RESIDUAL:
        v = v + residual.to(dt)
    if flags & RELU_MASK:
        v = torch.where(relu_src > 0, v, torch.zeros((), dtype=dt))
    if flags & ACCUM:
        v = v + c_old.to(dt)
    return v


def ref64(A, B, **epi):
    """The product A [M, K] @ B [K, N] and the full epilogue in float64."""
    return epilogue(torch.as_tensor(A).to(F64) @ torch.as_tensor(B).to(F64), **epi)


def eval32(A, B, **epi):
    """The "plain torch float32 evaluation" of the tolerance rule: a @ b plus the epilogue, all float32."""
    return epilogue(torch.as_tensor(A).to(F32) @ torch.as_tensor(B).to(F32), **epi)


def terms_abs(A, B, flags=0, alpha=1.0, bias=None, p=0.0, residual=None, c_old=None, absprod=None, **_):
    """B of the tolerance rule, per output element: |alpha| (|A| @ |B|) + |bias| (both times 1 / (1 - p) under dropout), + |residual|
    + |old C|.  ``absprod``: |A| @ |B| in float64 when the caller already has it."""
    if absprod is None:
        absprod = torch.as_tensor(A).to(F64).abs() @ torch.as_tensor(B).to(F64).abs()
    t = abs(alpha) * absprod
    if flags & BIAS:
        t = t + bias.to(F64).abs()[None, :]
    if flags & DROPOUT:
        t = t / (1.0 - p)
    if flags & RESIDUAL:
        t = t + residual.to(F64).abs()
    if flags & ACCUM:
        t = t + c_old.to(F64).abs()
    return t


def tolerance(ref, f32, terms, fmt64=None, packed_out=False):
    """util_rowops.tol of one output tensor, with the two reference-side additions the packed formats need:
    ``fmt64`` (LSTC_F32X3): the float64 value the f16-plane format itself delivers (pack3_emulation through the same epilogue) - the
    bound becomes 8 * max(e32, e_fmt, floor), e_fmt = max |fmt64 - ref|;
    ``packed_out`` (LSTC_EPI_OUT_PACK): a per-element allowance 2**-8 |ref| for the one RNE rounding to bf16 on store (8 significand
    bits: half an ulp is 2**-8 of the value just above a power of two, so this term alone is tight - measured ratios reach 0.99) -
    returns a tensor then."""
    t = tol(ref, f32, terms)
    if fmt64 is not None:
        t = max(t, 8.0 * float((fmt64 - ref).abs().max()))
    if packed_out:
        return t + 2.0 ** -8 * ref.abs()
    return t


def gemm_splits(dtype, K, split_k):
    """The header's formula for lstc_gemm_splits: ceil(kt / ceil(kt / split_k)), kt = K tiles of 64 (bf16 kernels) or 32."""
    if K <= 0:
        return 0
    bk = 64 if dtype in (LSTC_BF16, LSTC_BF16P) else 32
    s = max(split_k, 1)
    kt = -(-K // bk)
    per = -(-kt // s)
    return -(-kt // per)


# ------------------------------------------------------------------------------------------- inputs
FAMILIES = ("randn", "range", "cancel", "int")


def gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def operands(family, M, N, K, *key):
    """(A [M, K], B [K, N]) float32 on the CPU.
    randn:  standard normal.
    range:  randn with every seventh row of A times 1e3 and one column of B times 1e-3 (dynamic range inside one tensor).
    cancel: |randn| in A, B's sign alternating along k: the sums are small against the sum of |terms|.
    int:    integers in [-4, 4]: for K <= 4096 every product and partial sum is exact in f32, in bf16 operands and in the f16
            planes under a power-of-two scale, so every kernel and every summation order must return the float64 result exactly.
    spike:  (f32x3 only) randn with ONE element of A 1e6 times the rest: it alone sets the tensor's scale."""
    g = gen(M, N, K, (FAMILIES + ("spike",)).index(family), *key)
    if family == "int":
        return (torch.randint(-4, 5, (M, K), generator=g).to(F32), torch.randint(-4, 5, (K, N), generator=g).to(F32))
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    if family == "range":
        A[::7] *= 1e3
        B[:, N // 2] *= 1e-3
    elif family == "cancel":
        A = A.abs()
        B = B.abs() * (1.0 - 2.0 * (torch.arange(K) % 2).to(F32))[:, None]
    elif family == "spike":
        A[M // 2, K // 3] = 1e6
    return A, B


def aux_operands(family, M, N, *key):
    """(bias [N], residual [M, N], relu_src [M, N], old C [M, N]) of a family: integers for ``int``, randn otherwise.  relu_src has
    exact zeros and negative zeros on its first diagonal: the mask is ``> 0``, both are dropped."""
    g = gen(M, N, 77, FAMILIES.index(family) if family in FAMILIES else 9, *key)
    if family == "int":
        d = lambda *s: torch.randint(-4, 5, s, generator=g).to(F32)
    else:
        d = lambda *s: torch.randn(*s, generator=g)
    bias, res, src, old = d(N), d(M, N), d(M, N), d(M, N)
    i = torch.arange(min(M, N))
    src[i, i] = torch.where(i % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))
    return bias, res, src, old


# ------------------------------------------------------------------------------------------- case tables
# One entry per launch form the GPU file reaches.  Keys: id (names the kernel instantiation reached), dtype, M, N, K, layout ("NT"
# X W^T | "NN" dY W | "TN" dY^T X), variant, flags, alpha, split, batch; a_off / b_odd / c_odd: A one float off 16-B alignment, B with
# an odd leading dimension, C (and residual / mask) with an odd leading dimension - the scalar-load and scalar-epilogue paths.
ALL = BIAS | RELU | DROPOUT | RESIDUAL | RELU_MASK | ACCUM
EPI_SETS = [("bias", BIAS), ("relu", RELU), ("dropout", DROPOUT), ("residual", RESIDUAL), ("relu_mask", RELU_MASK), ("accum", ACCUM),
            ("bias_relu", BIAS | RELU), ("bias_dropout_residual", BIAS | DROPOUT | RESIDUAL), ("relu_mask_accum", RELU_MASK | ACCUM),
            ("all", ALL)]
# alpha of each EPI_SETS row: every row with a bias has alpha != 1, so a bias added before the alpha multiply shows
ALPHAS = (0.75, -2.0, 1.0, 0.75, -2.0, 1.0, -2.0, 0.75, 1.0, -2.0)
assert len(ALPHAS) == len(EPI_SETS) and all(a != 1.0 for a, (_, f) in zip(ALPHAS, EPI_SETS) if f & BIAS)


def make_case(id, dtype, M, N, K, layout="NT", variant=0, flags=0, alpha=1.0, split=0, batch=0, a_off=0, b_odd=0, c_odd=0, **kw):
    d = dict(id=id, dtype=dtype, M=M, N=N, K=K, layout=layout, variant=variant, flags=flags, alpha=alpha, split=split, batch=batch,
             a_off=a_off, b_odd=b_odd, c_odd=c_odd)
    d.update(kw)
    return d


def _f32_cases():
    out = []
    for lay in ("NT", "NN", "TN"):
        for (M, N, K) in ((300, 200, 100), (257, 132, 68), (128, 128, 32), (129, 1, 36), (1, 260, 4)):
            for v in (0, 4):
                if lay == "TN" and M % 4:            # an M-contiguous A of odd width is not a float4 operand: PIPE 3, listed below
                    continue
                if lay == "NN" and N % 4:
                    continue
                out.append(make_case("pipe5_v%d-%s-%dx%dx%d" % (v, lay, M, N, K), LSTC_F32, M, N, K, lay, v))
        for tag, a_off, b_odd in (("a_off", 1, 0), ("b_odd_ld", 0, 1), ("a_off_b_odd_ld", 1, 1)):
            out.append(make_case("pipe3_%s-%s-300x200x100" % (tag, lay), LSTC_F32, 300, 200, 100, lay, 0, a_off=a_off, b_odd=b_odd))
        out.append(make_case("pipe3_v8_aligned-%s-300x200x100" % lay, LSTC_F32, 300, 200, 100, lay, 8))
        out.append(make_case("tile64_v11-%s-65x63x67" % lay, LSTC_F32, 65, 63, 67, lay, 11))
        out.append(make_case("tile64_v11-%s-300x200x96" % lay, LSTC_F32, 300, 200, 96, lay, 11))
    for v in (4, 8, 11):
        for K in (1, 2, 3, 31, 32, 33, 63, 64, 65, 67):
            # a K that is no multiple of 4 is not a float4 operand in the K-contiguous layouts: variant 4 then runs PIPE 3's scalar loads
            out.append(make_case("kedge_v%d-NT-70x66x%d" % (v, K), LSTC_F32, 70, 66, K, "NT", v))
        for K in (1, 33, 64, 67):
            out.append(make_case("kedge_v%d-TN-72x68x%d" % (v, K), LSTC_F32, 72, 68, K, "TN", v))
    # epilogue matrix: float4 epilogue (everything aligned, N % 4 == 0) and scalar epilogue (odd ldc)
    for i, (name, fl) in enumerate(EPI_SETS):
        alpha = ALPHAS[i]
        out.append(make_case("epi_aligned_%s-NT-257x132x68" % name, LSTC_F32, 257, 132, 68, "NT", 0, fl, alpha))
        out.append(make_case("epi_scalar_%s-NT-257x131x67" % name, LSTC_F32, 257, 131, 67, "NT", 0, fl, alpha, c_odd=1))
    out.append(make_case("epi_aligned_all-NN-300x200x100", LSTC_F32, 300, 200, 100, "NN", 0, ALL, 0.75))
    out.append(make_case("epi_v11_bias_dropout_residual-NT-300x200x96", LSTC_F32, 300, 200, 96, "NT", 11, BIAS | DROPOUT | RESIDUAL, -2.0))
    # persistent walk and its fallbacks
    out.append(make_case("persist_v12_epi1-NT-256x512x128", LSTC_F32, 256, 512, 128, "NT", 12))
    out.append(make_case("persist_v12_epi2_residual-NT-256x512x128", LSTC_F32, 256, 512, 128, "NT", 12, RESIDUAL))
    out.append(make_case("persist_v12_epi2_accum-NN-256x512x128", LSTC_F32, 256, 512, 128, "NN", 12, ACCUM, 0.75))
    out.append(make_case("persist_v12_fallback_3ktiles-NT-256x512x96", LSTC_F32, 256, 512, 96, "NT", 12))
    out.append(make_case("persist_v12_fallback_ktail-NT-256x512x100", LSTC_F32, 256, 512, 100, "NT", 12))
    # split-K with atomics
    out.append(make_case("splitk_atomic_3slices-TN-132x260x160", LSTC_F32, 132, 260, 160, "TN", 0, split=4))
    out.append(make_case("splitk_atomic_scalar_loads-TN-130x260x515", LSTC_F32, 130, 260, 515, "TN", 0, split=3))
    # batch
    for lay in ("NT", "TN"):
        out.append(make_case("batch3-%s-68x36x40" % lay, LSTC_F32, 68, 36, 40, lay, 0, batch=3))
        out.append(make_case("batch3_accum-%s-68x36x40" % lay, LSTC_F32, 68, 36, 40, lay, 0, ACCUM, 0.75, batch=3))
    return out


def _bf16c_cases():
    out = []
    D = LSTC_BF16
    for v in (0, 1, 2):
        for lay in ("NT", "NN", "TN"):
            out.append(make_case("bf16c_v%d-%s-300x200x132" % (v, lay), D, 300, 200, 132, lay, v))
        out.append(make_case("bf16c_v%d_scalar_loads-NT-257x131x67" % v, D, 257, 131, 67, "NT", v, a_off=1, b_odd=1, c_odd=1))
        if v:                                                # the four <VA, VB> instantiations of both tiles (1: 128 x 128, 2: 256 x 128)
            for lay in ("NT", "NN", "TN"):
                out.append(make_case("bf16c_v%d_a_off_only-%s-300x200x132" % (v, lay), D, 300, 200, 132, lay, v, a_off=1))
                out.append(make_case("bf16c_v%d_b_odd_ld_only-%s-300x200x132" % (v, lay), D, 300, 200, 132, lay, v, b_odd=1))
                out.append(make_case("bf16c_v%d_a_off_b_odd_ld-%s-300x200x132" % (v, lay), D, 300, 200, 132, lay, v, a_off=1, b_odd=1))
        out.append(make_case("bf16c_v%d_all-NT-257x131x67" % v, D, 257, 131, 67, "NT", v, ALL, 0.75, c_odd=1))
        out.append(make_case("bf16c_v%d_out_f32_bias_dropout_residual-NN-300x200x132" % v, D, 300, 200, 132, "NN", v, OUT_F32 | BIAS | DROPOUT | RESIDUAL, -2.0))
        out.append(make_case("bf16c_v%d_batch3-NT-68x36x72" % v, D, 68, 36, 72, "NT", v, batch=3))
    for i, (name, fl) in enumerate(EPI_SETS):
        out.append(make_case("bf16c_epi_%s-NT-300x200x132" % name, D, 300, 200, 132, "NT", 0, fl, ALPHAS[i]))
    for K in (63, 64, 65, 127, 128, 129):
        out.append(make_case("bf16c_kedge-NT-70x66x%d" % K, D, 70, 66, K, "NT", 0))
        out.append(make_case("bf16c_kedge-TN-72x68x%d" % K, D, 72, 68, K, "TN", 0))
    out.append(make_case("bf16c_v0_picks_128x128_K4096-NT-130x130x4096", D, 130, 130, 4096, "NT", 0))
    out.append(make_case("bf16c_v0_picks_256x128_K4032-NT-130x130x4032", D, 130, 130, 4032, "NT", 0))
    out.append(make_case("bf16c_splitk3-TN-132x260x515", D, 132, 260, 515, "TN", 0, split=3))
    out.append(make_case("bf16c_batch3_accum-TN-68x36x72", D, 68, 36, 72, "TN", 0, ACCUM, batch=3))
    return out


def _f32x3_cases():
    out = []
    D = LSTC_F32X3
    for (M, N, K) in ((300, 520, 100), (257, 131, 67), (128, 128, 32), (64, 1, 32)):
        out.append(make_case("pk2s_nt-%dx%dx%d" % (M, N, K), D, M, N, K, "NT", 0, c_odd=N % 4 != 0))
    out.append(make_case("pk2s_nt_kmajor_sources-NN-300x520x100", D, 300, 520, 100, "NN", 3))
    for i, (name, fl) in enumerate(EPI_SETS):
        out.append(make_case("pk2s_nt_epi_f4_%s-300x520x100" % name, D, 300, 520, 100, "NT", 0, fl, ALPHAS[i]))
        out.append(make_case("pk2s_nt_epi_scalar_%s-257x131x67" % name, D, 257, 131, 67, "NT", 0, fl, ALPHAS[i], c_odd=1))
    out.append(make_case("pkw_nt_v2-300x520x132", D, 300, 520, 132, "NT", 2, ALL, 0.75))
    out.append(make_case("pkw_nt_v2-NN-512x200x96", D, 512, 200, 96, "NN", 2, RELU_MASK))
    out.append(make_case("pk2s_tr-128x384x1152", D, 128, 384, 1152, "TR", 0))
    out.append(make_case("pk2s_tr-256x128x384", D, 256, 128, 384, "TR", 3))
    out.append(make_case("pkw_tr_v2-512x256x640", D, 512, 256, 640, "TR", 2))
    out.append(make_case("pkw_tr_default_K8192-256x128x8192", D, 256, 128, 8192, "TR", 0, families=("randn", "range")))
    out.append(make_case("pk2s_tr_default_K8192_M384-384x128x8192", D, 384, 128, 8192, "TR", 0, families=("randn", "range")))
    out.append(make_case("pk2s_tr_split_partials_15of16-128x128x4224", D, 128, 128, 4224, "TR", 0, split=16, partials=True,
                  families=("randn", "range", "cancel")))
    out.append(make_case("pk2s_nt_split_atomic-130x260x515", D, 130, 260, 515, "NT", 3, split=3, c_odd=1))
    return out


def _bf16p_cases():
    out = []
    D = LSTC_BF16P
    for (M, N, K, fl) in ((300, 200, 100, 0), (600, 520, 1000, ALL), (512, 512, 64, 0)):
        out.append(make_case("bf16p_persistent_no_qtail-%dx%dx%d" % (M, N, K), D, M, N, K, "NT", NO_QTAIL, fl, 0.75 if fl else 1.0, qtail=False))
        out.append(make_case("bf16p_qtail-%dx%dx%d" % (M, N, K), D, M, N, K, "NT", 0, fl, 0.75 if fl else 1.0, qtail=True))
    out.append(make_case("bf16p_persistent_scalar_epilogue-257x131x67", D, 257, 131, 67, "NT", NO_QTAIL, ALL, 0.75, c_odd=1, qtail=False))
    out.append(make_case("bf16p_persistent_kmajor_sources-NN-300x200x132", D, 300, 200, 132, "NN", NO_QTAIL, RELU_MASK | ACCUM, qtail=False))
    for i, (name, fl) in enumerate(EPI_SETS):
        out.append(make_case("bf16p_qtail_epi_%s-300x200x100" % name, D, 300, 200, 100, "NT", 0, fl, ALPHAS[i], qtail=True))
    for K in (63, 64, 65, 127, 128, 129, 191):
        out.append(make_case("bf16p_kedge_no_qtail-70x68x%d" % K, D, 70, 68, K, "NT", NO_QTAIL, qtail=False))
        out.append(make_case("bf16p_kedge_qtail-70x68x%d" % K, D, 70, 68, K, "NT", 0, qtail=True))
    for (M, N, K) in ((256, 256, 384), (300, 523, 640), (96, 40, 128)):
        out.append(make_case("bf16p_tr-%dx%dx%d" % (M, N, K), D, M, N, K, "TR", 0, c_odd=N % 4 != 0))
    out.append(make_case("bf16p_tr_split_partials_6of7-256x256x1152", D, 256, 256, 1152, "TR", 0, split=7, partials=True))
    out.append(make_case("bf16p_tr_split_atomic-300x523x640", D, 300, 523, 640, "TR", 0, split=3, c_odd=1))
    # the packed epilogues, on BOTH kernels: variant 0 sends these few tiles to gemm_bf16p_q_kernel<EPK> (all of them are tail),
    # NO_QTAIL to the persistent gemm_bf16p_kernel<false, true, EPK> - the form the bf16 activation stream runs at full size.
    # RELU_MASK_PACK alone (EPK 3) has no quarter-tile form: the persistent kernel under either variant.
    for (M, N, K) in ((512, 256, 256), (1024, 768, 320)):
        for kern, v, q in (("q_kernel", 0, True), ("persistent", NO_QTAIL, False)):
            sh = "%dx%dx%d" % (M, N, K)
            out.append(make_case("bf16p_%s_epk1_out_pack-%s" % (kern, sh), D, M, N, K, "NT", v, OUT_PACK | BIAS | RELU, 0.75, qtail=q))
            out.append(make_case("bf16p_%s_epk2_out_pack_relu_mask_pack-%s" % (kern, sh), D, M, N, K, "NT", v, OUT_PACK | RELU_MASK | RELU_MASK_PACK,
                                 qtail=q))
            out.append(make_case("bf16p_%s_epk4_out_pack_residual_pack_bias_dropout-%s" % (kern, sh), D, M, N, K, "NT", v,
                                 OUT_PACK | RESIDUAL | RESIDUAL_PACK | BIAS | DROPOUT, 0.75, qtail=q))
        out.append(make_case("bf16p_persistent_epk3_relu_mask_pack-%dx%dx%d" % (M, N, K), D, M, N, K, "NT", 0, RELU_MASK | RELU_MASK_PACK, -2.0,
                             qtail=False))
    return out


def cu_cases(n_cu):
    """The cases whose shapes are computed from the compute-unit count (the GPU file passes the device's; the host sweep a nominal
    256): the persistent walk's second round, the default's row split, and bf16p with more tiles than CUs."""
    slots = 2 * n_cu
    M = 128 * (slots + 8)
    fams = ("randn", "int")
    return dict(
        persist=make_case("persist_v12_epi1_second_round-NT-%dx128x128" % M, LSTC_F32, M, 128, 128, "NT", 12, families=fams),
        rowsplit_epi=make_case("rowsplit_v0_bias_dropout_residual-NT-%dx128x36" % M, LSTC_F32, M, 128, 36, "NT", 0, BIAS | DROPOUT | RESIDUAL, 0.75,
                               families=fams),
        rowsplit_plain=make_case("rowsplit_v0_plain-NT-%dx128x36" % M, LSTC_F32, M, 128, 36, "NT", 0, families=fams),
        bf16p_qtail=make_case("bf16p_persistent_then_q_kernel-NT-%dx256x64" % (256 * (n_cu + 16)), LSTC_BF16P, 256 * (n_cu + 16), 256, 64, "NT", 0,
                              BIAS | RESIDUAL, 0.75, families=fams, qtail=True),
        bf16p_second_trip=make_case("bf16p_persistent_second_trip-NT-%dx256x64" % (256 * (n_cu + 16)), LSTC_BF16P, 256 * (n_cu + 16), 256, 64, "NT",
                                    NO_QTAIL, BIAS | RESIDUAL, 0.75, families=fams, qtail=False))


CASES = {LSTC_F32: _f32_cases(), LSTC_BF16: _bf16c_cases(), LSTC_F32X3: _f32x3_cases(), LSTC_BF16P: _bf16p_cases()}
DROP_P = 0.3


def case_families(case):
    """The families a case runs: all four unless the case names its own (K > 4096 leaves the ``int`` family's exact range)."""
    fams = case.get("families", FAMILIES)
    if case["dtype"] == LSTC_F32X3 and "families" not in case:
        fams = fams + ("spike",)
    return fams


def drop_p(family):
    """p = 0.3 everywhere but the ``int`` family: 1 / (1 - 0.3) is not a float32, so a kept integer times it rounds, and the float64
    reference would differ from a correct kernel by that rounding.  p = 0.5 scales by exactly 2 and keeps the equality demand."""
    return 0.5 if family == "int" else DROP_P


def case_problem(case, family, z=0):
    """Everything one (case, family, batch index) needs on the CPU: logical A [M, K], B [K, N] AS THE KERNEL SEES THEM (rounded to
    bf16 for the bf16 dtypes), bias, residual, relu_src, old C.  The dropout keep mask comes from the caller."""
    M, N, K = case["M"], case["N"], case["K"]
    fam_ops = "randn" if family == "spike" else family
    A, B = operands(family, M, N, K, z)
    bias, res, src, old = aux_operands(fam_ops, M, N, z)
    if case["dtype"] in (LSTC_BF16, LSTC_BF16P):
        A, B = bf16_round(A), bf16_round(B)
    return A, B, bias, res, src, old


def epi_kwargs(case, family, bias, res, src, old, keep):
    fl = case["flags"] & ALL
    return dict(flags=fl, alpha=case["alpha"], bias=bias, keep=keep, p=drop_p(family), residual=res, relu_src=src, c_old=old)


_PRODUCTS = {}


def products(case, family, z=0):
    """The operands of (case, family, batch index) and everything about them that does not depend on the epilogue, computed ONCE and
    shared by every test that needs it (read-only): A, B, bias, res, src, old as ``case_problem`` (A, B rounded to bf16 for the bf16
    dtypes: the reference's operands), A_raw, B_raw the unrounded operands the device is given; acc64 = A @ B in float64, acc32 the
    torch float32 product, absprod = |A| @ |B| in float64, emu = pack3_emulation (LSTC_F32X3 only, else None)."""
    x3 = case["dtype"] == LSTC_F32X3
    key = (case["dtype"] in (LSTC_BF16, LSTC_BF16P), x3, case["M"], case["N"], case["K"], family, z)
    hit = _PRODUCTS.get(key)
    if hit is None:
        A, B, bias, res, src, old = case_problem(case, family, z)
        A_raw, B_raw = operands(family, case["M"], case["N"], case["K"], z)      # what the device gets: the kernel does the rounding
        A64, B64 = A.to(F64), B.to(F64)
        hit = dict(A=A, B=B, A_raw=A_raw, B_raw=B_raw, bias=bias, res=res, src=src, old=old, acc64=A64 @ B64, acc32=A @ B, absprod=A64.abs() @ B64.abs(),
                   emu=pack3_emulation(A, B) if x3 else None)
        while len(_PRODUCTS) >= 48:
            _PRODUCTS.pop(next(iter(_PRODUCTS)))
        _PRODUCTS[key] = hit
    return hit


def case_reference(case, family, keep, z=0, **override):
    """(ref64, float32 evaluation, terms_abs, format emulation or None) of a case's full epilogue on the shared products."""
    P = products(case, family, z)
    kw = epi_kwargs(case, family, P["bias"], P["res"], P["src"], P["old"], keep)
    kw.update(override)
    ref = epilogue(P["acc64"], **kw)
    f32 = epilogue(P["acc32"], **kw)
    terms = terms_abs(None, None, absprod=P["absprod"], **kw)
    fmt = epilogue(P["emu"], **kw) if P["emu"] is not None else None
    return ref, f32, terms, fmt
