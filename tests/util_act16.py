"""The six kernels only the bf16 activation stream uses - ln_fwd_act, ln_bwd_act, dropout_apply_pack_kernel,
colsum_pack1_kernel (csrc/rowops.hip) and cls_dot_pk / cls_wsum_pk / cls_outer_pk (csrc/attention.hip): the lstc_pack1 layout written
and read in plain torch, raw ctypes calls with every argument settable, float64 references on the values the packs hold, and the
checks both test files share.  tests/test_act_stream_ref_host.py checks this file on the CPU before
tests/test_act_stream_f64_gpu.py holds the kernels to it.  Every function here works on whatever device its inputs live on.

ONE tolerance rule, the project's (util_rowops.tol through util_gemm.tolerance): per f32 output tensor 8 * max(e32, floor), e32 the
error of a plain torch float32 evaluation of the same formulas and floor = 4 * 2**-24 * (largest sum of |terms| of one element); a
packed bf16 output adds 2**-8 |ref| per element for its one RNE rounding; the two kernels that contract an f32 operand as a bf16
hi + lo pair (cls_dot_pk, cls_outer_pk) get ``fmt64``: the float64 value of exactly the products the format keeps, so the bound is
8 * max(e32, e_fmt, floor).  cls_wsum_pk contracts the f32 weights unsplit (fmaf on the vector unit): its e_fmt is zero and it is
held to the plain rule.  No kernel needed a rounding point added to its model (as util_attn_packed.py had to): every bar is the
rule as stated.  The worst err / tol is recorded per section, packed outputs apart from f32 ones - a packed output's bar is mostly
its 2**-8 |ref| rounding allowance, which an RNE rounding just above a power of two uses up (ratios near 1 are that, not drift)."""
import atexit
import functools
import os

import numpy as np
import torch

import util_gemm as G
import util_rowops as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
TILE = 4096                     # elements of one 128-row x 32-k tile
EPS = 1e-6
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED, E_RANGE = -1, -2, -3, -4, -5


def bf16(t):
    return t.to(BF16).to(F32)


def p32(p):
    """The dropout rate as the C ABI receives it (a float)."""
    return float(np.float32(p))


# =========================================================================================== the lstc_pack1 layout, on the host
def kbp(K):
    """32-k tiles per row block, padded to an even number."""
    return 2 * ((K + 63) // 64)


def rbp(rows):
    """128-row blocks, padded to an even number."""
    return 2 * ((rows + 255) // 256)


def grid_elems(rows, K):
    return rbp(rows) * kbp(K) * TILE


@functools.lru_cache(maxsize=6)
def _offsets(rows, K, device, bad_xor_row):
    r = torch.arange(rows, device=device).view(-1, 1)
    k = torch.arange(K, device=device).view(1, -1)
    rr, kb, ch = r & 127, k >> 5, (k & 31) >> 3
    x = (rr >> 2) & 3
    if bad_xor_row >= 0:                                     # the defect of test_act_stream_ref_host.py: one row's chunk XOR is off
        x = torch.where(r == bad_xor_row, (x + 1) & 3, x)
    return (((r >> 7) * kbp(K) + kb) * TILE + rr * 32 + ((ch ^ x) << 3) + (k & 7)).reshape(-1)


def pack_offsets(rows, K, device="cpu", bad_xor_row=-1):
    """Element offset of (row, k) in the pack of a [rows, K] matrix, flattened row-major (csrc/lstc_common.h p1_offset): tile
    (row >> 7, k >> 5) of the [RBp, KBp] tile grid, row rr = row & 127 at rr * 32, 16-B chunk (k & 31) >> 3 XOR (rr >> 2) & 3."""
    return _offsets(int(rows), int(K), str(device), int(bad_xor_row))


def pack_write(x, bad_xor_row=-1):
    """The lstc_pack1 image of a bf16-representable f32 matrix: a bfloat16 tensor of grid_elems(rows, K) elements, zeros in the
    padding rows and columns."""
    rows, K = x.shape
    assert torch.equal(bf16(x), x), "pack_write takes values bf16 holds exactly"
    buf = torch.zeros(grid_elems(rows, K), dtype=BF16, device=x.device)
    buf[pack_offsets(rows, K, x.device, bad_xor_row)] = x.reshape(-1).to(BF16)
    return buf


def pack_read(buf, rows, K):
    """f32 [rows, K] out of a pack (a bfloat16 tensor, or the uint8 buffer that holds one)."""
    h = buf.view(BF16) if buf.dtype == torch.uint8 else buf
    return h[pack_offsets(rows, K, buf.device)].view(rows, K).to(F32)


def bits(t):
    """bfloat16 / float32 values as integers: equality of bits, not of values (NaN, -0)."""
    return t if t.dtype in (torch.uint8, torch.bool) else t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# =========================================================================================== raw calls
def _L():
    from lstc_vad_amd import _lib
    return _lib


def rc(name, *args):
    """The entry point's return code; tensors become device pointers, None NULL, the stream is appended (NULL on a machine without a
    GPU, where only refusals - which return before any launch - are called, with small integers standing in for pointers)."""
    L = _L()
    a = [L.dev_ptr(t) if torch.is_tensor(t) else t for t in args]
    return getattr(L.load(), name)(*a, L.stream_ptr() if torch.cuda.is_available() else None)


def call(name, *args):
    _L().check(rc(name, *args), name)


def pack_bytes(rows, K):
    return int(_L().load().lstc_pack1_bytes(rows, K))


def in_pack(x, dev):
    """Device buffer of lstc_pack1_bytes(rows, K) bytes holding the HOST-written pack of ``x``; 0xFF behind the tile grid."""
    rows, K = x.shape
    buf = torch.full((pack_bytes(rows, K),), 0xFF, dtype=torch.uint8, device=dev)
    buf[:2 * grid_elems(rows, K)] = pack_write(x.to(dev)).view(torch.uint8)
    return buf


def out_pack(rows, K, dev):
    """An output pack: lstc_pack1_bytes(rows, K) bytes of 0xFF (every bf16 of it a NaN until written)."""
    return torch.full((pack_bytes(rows, K),), 0xFF, dtype=torch.uint8, device=dev)


def slack_intact(buf, rows, K):
    """The bytes behind the tile grid still hold 0xFF."""
    tail = buf[2 * grid_elems(rows, K):]
    return tail.numel() > 0 and bool((tail == 0xFF).all())


def guarded(shape, dev, src=None, pad=4):
    """An f32 device tensor of ``shape`` (NaN until written) with ``pad`` NaN floats in front and behind; 16-B aligned for pad = 4.
    Returns (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), float("nan"), device=dev, dtype=F32)
    view = buf[pad:pad + n].view(*shape)
    if src is not None:
        view.copy_(src.to(F32))
    return view, buf


def guards_ok(buf, pad=4):
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())


def device_keep(n, p, seed, dev):
    """lstc_dropout_mask over n flat indices: bool [n]."""
    m = torch.empty((n,), dtype=torch.uint8, device=dev)
    call("lstc_dropout_mask", m, n, float(p), int(seed))
    return m.bool()


def host_keep(n, p, seed):
    """The same mask from the numpy restatement of the counter hash (util.host_dropout_keep), at the rate the ABI receives."""
    from util import host_dropout_keep
    return torch.from_numpy(host_dropout_keep(np.arange(n), p32(p), seed))


def drop_scale(p, dtype=F64):
    """1 / (1 - p) as ``dtype`` arithmetic on the float rate (the kernels: 1.f / (1.f - p))."""
    one = torch.tensor(1.0, dtype=dtype)
    return one / (one - torch.tensor(p32(p), dtype=F32).to(dtype))


def refusals(A, B):
    """(label, entry point, arguments, code) of every refusal the GPU file relies on (include/lstc_hip.h).  ``A`` stands for any
    16-B aligned operand and ``B`` for one 8 bytes off: integers on a machine without a GPU, one large device buffer on the GPU -
    every call returns before a launch."""
    s = 0x1234567800000001
    return [
        ("ln_fwd d=768", "lstc_layernorm_fwd_act", (None, A, A, A, A, None, A, A, 256, 768, EPS), E_UNSUPPORTED),
        ("ln_fwd rows % 256", "lstc_layernorm_fwd_act", (None, A, A, A, A, None, A, A, 255, 1024, EPS), E_UNSUPPORTED),
        ("ln_fwd x and x_pack", "lstc_layernorm_fwd_act", (A, A, A, A, A, None, A, A, 256, 1024, EPS), E_NULL),
        ("ln_fwd neither x nor x_pack", "lstc_layernorm_fwd_act", (None, None, A, A, A, None, A, A, 256, 1024, EPS), E_NULL),
        ("ln_fwd neither y nor y_pack", "lstc_layernorm_fwd_act", (None, A, A, A, None, None, A, A, 256, 1024, EPS), E_NULL),
        ("ln_fwd misaligned x_pack", "lstc_layernorm_fwd_act", (None, B, A, A, A, None, A, A, 256, 1024, EPS), E_ALIGN),
        ("ln_fwd misaligned y_pack", "lstc_layernorm_fwd_act", (None, A, A, A, None, B, A, A, 256, 1024, EPS), E_ALIGN),
        ("ln_bwd d=768", "lstc_layernorm_bwd_act", (None, A, A, A, A, A, A, A, 4, 256, 768, 0.0, s, A), E_UNSUPPORTED),
        ("ln_bwd rows % 256", "lstc_layernorm_bwd_act", (None, A, A, A, A, A, A, A, 4, 128, 1024, 0.0, s, A), E_UNSUPPORTED),
        ("ln_bwd dy and dy_pack", "lstc_layernorm_bwd_act", (A, A, A, A, A, A, A, A, 4, 256, 1024, 0.0, s, A), E_NULL),
        ("ln_bwd neither dy nor dy_pack", "lstc_layernorm_bwd_act", (None, None, A, A, A, A, A, A, 4, 256, 1024, 0.0, s, A), E_NULL),
        ("ln_bwd dropout_p = 1", "lstc_layernorm_bwd_act", (None, A, A, A, A, A, A, A, 4, 256, 1024, 1.0, s, A), E_SHAPE),
        ("ln_bwd n_partial = 0", "lstc_layernorm_bwd_act", (None, A, A, A, A, A, A, A, 0, 256, 1024, 0.0, s, A), E_SHAPE),
        ("ln_bwd misaligned df_pack", "lstc_layernorm_bwd_act", (None, A, A, A, A, A, A, A, 4, 256, 1024, 0.0, s, B), E_ALIGN),
        ("ln_bwd misaligned dx_pack", "lstc_layernorm_bwd_act", (None, A, A, A, A, A, B, A, 4, 256, 1024, 0.0, s, A), E_ALIGN),
        ("dropout rows % 256", "lstc_dropout_apply_pack", (A, A, 128, 64, 0.3, s), E_UNSUPPORTED),
        ("dropout d % 64", "lstc_dropout_apply_pack", (A, A, 256, 96, 0.3, s), E_UNSUPPORTED),
        ("dropout dropout_p = 1", "lstc_dropout_apply_pack", (A, A, 256, 64, 1.0, s), E_SHAPE),
        ("dropout misaligned y_pack", "lstc_dropout_apply_pack", (A, B, 256, 64, 0.3, s), E_ALIGN),
        ("colsum misaligned pack", "lstc_colsum_pack1", (B, 256, 64, A, 1, A, 0), E_ALIGN),
        ("colsum n_partial = 0", "lstc_colsum_pack1", (A, 256, 64, A, 0, A, 0), E_SHAPE),
        ("cls_dot H=9", "lstc_cls_dot_pack", (A, A, A, A, 256, 2, 9, 512, 0, 0.0, s), E_UNSUPPORTED),
        ("cls_dot S=129", "lstc_cls_dot_pack", (A, A, A, A, 256, 129, 8, 512, 0, 0.0, s), E_RANGE),
        ("cls_dot d=768", "lstc_cls_dot_pack", (A, A, A, A, 256, 2, 8, 768, 0, 0.0, s), E_UNSUPPORTED),
        ("cls_dot rows % 256", "lstc_cls_dot_pack", (A, A, A, A, 255, 2, 8, 512, 0, 0.0, s), E_UNSUPPORTED),
        ("cls_dot misaligned pack", "lstc_cls_dot_pack", (A, B, A, A, 256, 2, 8, 512, 0, 0.0, s), E_ALIGN),
        ("cls_dot mode 1 without probs", "lstc_cls_dot_pack", (A, A, A, None, 256, 2, 8, 512, 1, 0.0, s), E_NULL),
        ("cls_dot mode 3", "lstc_cls_dot_pack", (A, A, A, A, 256, 2, 8, 512, 3, 0.0, s), E_UNSUPPORTED),
        ("cls_wsum H=9", "lstc_cls_wsum_pack", (A, A, A, 256, 2, 9, 512), E_UNSUPPORTED),
        ("cls_wsum S=129", "lstc_cls_wsum_pack", (A, A, A, 256, 129, 8, 512), E_RANGE),
        ("cls_wsum d=768", "lstc_cls_wsum_pack", (A, A, A, 256, 2, 8, 768), E_UNSUPPORTED),
        ("cls_outer H=9", "lstc_cls_outer_pack", (A, A, A, A, None, A, 256, 2, 9, 512), E_UNSUPPORTED),
        ("cls_outer S=129", "lstc_cls_outer_pack", (A, A, A, A, None, A, 256, 129, 8, 512), E_RANGE),
        ("cls_outer d=768", "lstc_cls_outer_pack", (A, A, A, A, None, A, 256, 2, 8, 768), E_UNSUPPORTED),
        ("cls_outer misaligned pack", "lstc_cls_outer_pack", (A, A, A, A, None, B, 256, 2, 8, 512), E_ALIGN),
        ("cls_outer misaligned add0", "lstc_cls_outer_pack", (A, A, A, A, B, A, 256, 2, 8, 512), E_ALIGN),
    ]


# =========================================================================================== reporting
WORST = {}      # kernel family -> (err / tol, err, tol, case + what)


def _dump():
    path = os.environ.get("LSTC_ACT_STREAM_ERRORS")
    if path and WORST:
        with open(path, "w") as f:
            f.write(f"{'section':<30} {'err/tol':<8} {'max|err|':<12} {'tol':<12} at\n")
            for fam, (r, e, t, where) in sorted(WORST.items()):
                f.write(f"{fam:<30} {r:<8.3f} {e:<12.3e} {t:<12.3e} {where}\n")


atexit.register(_dump)


def report():
    for fam in sorted(WORST):
        print("act-stream worst err/tol  %-30s %.3f  (err %.3e tol %.3e: %s)" % ((fam,) + WORST[fam]))


class Checks:
    """The comparisons of one case; ``done`` asserts them together so a failure shows every output's figures."""

    def __init__(self, family, case, record=True):
        self.family, self.case, self.bad, self.record = family, case, [], record

    def ratio(self, what, got, ref64, f32, terms, fmt64=None, packed=False):
        """err / tol of one output tensor under the rule (elementwise worst for a packed output); printed and recorded."""
        got = got.detach().to(F64)
        assert got.shape == ref64.shape, (self.case, what, got.shape, ref64.shape)
        t = G.tolerance(ref64, f32, terms, fmt64=fmt64, packed_out=packed)
        t = t if torch.is_tensor(t) else torch.full_like(ref64, t)
        diff = (got - ref64).abs()
        if not bool(torch.isfinite(got).all()):
            r, e, tt = float("inf"), float("inf"), float(t.min())
        else:
            q = torch.where(t > 0, diff / t, torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
            i = int(q.reshape(-1).argmax()) if q.numel() else 0
            r, e, tt = (float(q.reshape(-1)[i]), float(diff.reshape(-1)[i]), float(t.reshape(-1)[i])) if q.numel() else (0.0, 0.0, 0.0)
        print("%s %s %s: err %.3e tol %.3e ratio %.3f" % (self.family, self.case, what, e, tt, r))
        fam = self.family + (" (packed)" if packed else "")
        if self.record and r >= WORST.get(fam, (-1.0,))[0]:
            WORST[fam] = (r, e, tt, "%s %s" % (self.case, what))
        return r

    def close(self, what, got, ref64, f32, terms, fmt64=None, packed=False):
        r = self.ratio(what, got, ref64, f32, terms, fmt64, packed)
        if not r <= 1.0:
            self.bad.append((what, "err/tol", r))

    def beyond(self, what, got, ref64, f32, terms, fmt64=None, packed=False):
        """The reverse: a DEFECTIVE result must land outside the bar."""
        r = self.ratio(what, got, ref64, f32, terms, fmt64, packed)
        if not r > 1.0:
            self.bad.append((what, "defect inside the bar, err/tol", r))

    def equal(self, what, a, b):
        if a.shape != b.shape or not torch.equal(bits(a), bits(b)):
            n = int((bits(a) != bits(b)).sum()) if a.shape == b.shape else -1
            self.bad.append((what, "bits differ at %d elements" % n))

    def true(self, what, cond):
        if not bool(cond):
            self.bad.append((what, "false"))

    def done(self):
        assert not self.bad, (self.family, self.case, self.bad)


# =========================================================================================== LayerNorm on packs
LN_FAMILIES = ("randn", "shifted100", "constant_row")


@functools.lru_cache(maxsize=16)
def ln_inputs(rows, d, family):
    """(x, gamma, beta, const) on the CPU; x is rounded to bf16 so a pack and an f32 tensor hold the same values.  randn: 2 randn
    + 0.3; shifted100: + 100 (a one-pass variance loses its digits; bf16 steps of 0.5 there); constant_row: row rows // 2 is 2.0
    everywhere (variance 0: rstd = 1 / sqrt(eps), y = beta)."""
    g = G.gen(rows, d, LN_FAMILIES.index(family), 16)
    x = torch.randn(rows, d, generator=g) * 2 + 0.3
    const = None
    if family == "shifted100":
        x = x + 100.0
    elif family == "constant_row":
        const = rows // 2
        x[const] = 2.0
    gamma = 1.0 + 0.5 * torch.randn(d, generator=g)
    beta = torch.randn(d, generator=g)
    return bf16(x), gamma, beta, const


def ln_fwd_refs(x, gamma, beta):
    """((y, mean, rstd) float64, the same float32, their terms_abs): util_rowops' statement, on the device of ``x``."""
    return (R.ln_fwd(x, gamma, beta, EPS), R.ln_fwd(x, gamma, beta, EPS, dtype=F32), R.ln_fwd_terms(x, gamma, beta, EPS))


def ln_row_groups(rows, const, device):
    """A constant row's terms (|x| rstd = 2000) would set every other row's tolerance: it is checked on its own."""
    if const is None:
        return [("", torch.arange(rows, device=device))]
    return [("", torch.tensor([r for r in range(rows) if r != const], device=device)), ("const_row ", torch.tensor([const], device=device))]


def check_ln_fwd(ck, tag, refs, const, y=None, mean=None, rstd=None, ypack=None):
    """y (f32), mean, rstd under the rule; a packed y under the rule + 2**-8 |ref| per element."""
    ref, f32, terms = refs
    rows = ref[0].shape[0]
    for gname, idx in ln_row_groups(rows, const, ref[0].device):
        for name, got, i, pk in (("y", y, 0, False), ("mean", mean, 1, False), ("rstd", rstd, 2, False), ("y_pack", ypack, 0, True)):
            if got is not None:
                ck.close("%s %s%s" % (tag, gname, name), got[idx], ref[i][idx], f32[i][idx], terms[i][idx], packed=pk)


def ln_bwd_refs(dy, x, gamma, mean32, rstd32, keep, p):
    """Everything the backward is held to, from the SAME inputs the kernel gets (mean / rstd as the f32 it reads), as a dict of
    (float64 reference, float32 restatement, terms_abs) triples:
      dx, df = dx keep / (1 - p)            [rows, d]
      cg, cb, cd                            [rows, d]: what a row adds into dgamma (dy xhat), dbeta (dy), the df column sums (df
                                            BEFORE any rounding) - summed over a workgroup's rows by ``plane_sums``."""
    out = {}
    dx64, _, _ = R.ln_bwd(dy, x, gamma, mean32, rstd32)
    dx32, _, _ = R.ln_bwd(dy, x, gamma, mean32, rstd32, dtype=F32)
    tdx, _, _ = R.ln_bwd_terms(dy, x, gamma, mean32, rstd32)
    out["dx"] = (dx64, dx32, tdx)
    k64 = keep.to(F64)
    s64, s32 = drop_scale(p).to(x.device), drop_scale(p, F32).to(x.device)
    out["df"] = (dx64 * k64 * s64, dx32 * keep.to(F32) * s32, tdx * k64 * s64)
    xh = lambda dt: (x.to(dt) - mean32.to(dt)[:, None]) * rstd32.to(dt)[:, None]
    a = (x.to(F64).abs() + mean32.to(F64).abs()[:, None]) * rstd32.to(F64)[:, None]
    out["cg"] = (dy.to(F64) * xh(F64), dy.to(F32) * xh(F32), dy.to(F64).abs() * a)
    out["cb"] = (dy.to(F64), dy.to(F32), dy.to(F64).abs())
    out["cd"] = out["df"]
    return out


def owner(rows, n_partial, device="cpu"):
    """The workgroup of every row: w takes rows 2w and 2w + 1, then every 2 n_partial further (include/lstc_hip.h)."""
    return (torch.arange(rows, device=device) % (2 * n_partial)) // 2


def plane_sums(contrib, n_partial, own=None):
    """[n_partial, d]: per workgroup, the sum of its rows' contributions in contrib's dtype; a workgroup without rows stays zero."""
    own = owner(contrib.shape[0], n_partial, contrib.device) if own is None else own
    return torch.zeros((n_partial, contrib.shape[1]), dtype=contrib.dtype, device=contrib.device).index_add_(0, own, contrib)


def plane_refs(triple, n_partial):
    """(ref64, f32, terms) of one partial plane [n_partial, d] and of its sum over the workgroups [d]."""
    c64, c32, ct = triple
    per = (plane_sums(c64, n_partial), plane_sums(c32, n_partial), plane_sums(ct, n_partial))
    tot = (c64.sum(0), c32.sum(0), ct.sum(0))
    return per, tot


# =========================================================================================== dropout replay / column sums
def dropout_refs(x, keep, p):
    """y = bf16(f32(x) * f32(1 / (1 - p))) where kept: the float64 product, its f32 restatement and |product| as terms."""
    k64 = keep.to(F64)
    ref = x.to(F64) * k64 * drop_scale(p).to(x.device)
    f32 = x.to(F32) * keep.to(F32) * drop_scale(p, F32).to(x.device)
    return ref, f32, ref.abs()


def colsum_groups(rows, n_partial):
    """(np, per): lstc_colsum_pack1 launches np = min(RB, n_partial) row-block groups of per = ceil(RB / np) 128-row blocks each,
    RB the pack's even number of row blocks; a trailing group may be empty."""
    RB = rbp(rows)
    np_ = min(RB, n_partial)
    return np_, -(-RB // np_)


def colsum_partial_refs(x, n_partial):
    """[np, K] float64 / float32 / terms: the column sums of every row-block group (rows beyond the matrix are zeros)."""
    rows, K = x.shape
    np_, per = colsum_groups(rows, n_partial)
    grp = torch.arange(rows, device=x.device) // (128 * per)
    f = lambda t: torch.zeros((np_, K), dtype=t.dtype, device=x.device).index_add_(0, grp, t)
    return f(x.to(F64)), f(x.to(F32)), f(x.to(F64).abs())


# =========================================================================================== CLS passes over a packed X
CLS_FAMILIES = ("randn", "range", "int")


def cls_inputs(N, S, H, d, family, dev="cpu"):
    """U, U2 [N, H, d], W, W2 [N, H, S], add0 [N, d], X [N, S, d] (bf16 values) and softmax rows P_in [N, H, S] for mode 2.
    randn: U 0.05 randn (scores of order 1), the rest randn.  range: the same with every (n, h) row of U, U2, W, W2 scaled by a
    power of two spread over 2**-10 .. 2**10.  int: integers in [-3, 3] (X [-4, 4], add0 [-8, 8]): every product and sum is exact
    in f32, every dX value in bf16."""
    g = torch.Generator(device=dev).manual_seed(hash((N, S, H, d, CLS_FAMILIES.index(family), 5)) % (2 ** 31))
    if family == "int":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=dev).to(F32)
        U, U2, W, W2 = ri(-3, 3, N, H, d), ri(-3, 3, N, H, d), ri(-3, 3, N, H, S), ri(-3, 3, N, H, S)
        add0, X = ri(-8, 8, N, d), ri(-4, 4, N, S, d)
    else:
        rn = lambda *s: torch.randn(*s, generator=g, device=dev)
        U, U2, W, W2, add0, X = 0.05 * rn(N, H, d), rn(N, H, d), rn(N, H, S), rn(N, H, S), rn(N, d), bf16(rn(N, S, d))
        if family == "range":
            e = lambda: torch.exp2(torch.randint(-10, 11, (N, H, 1), generator=g, device=dev).to(F32))
            U, U2, W, W2 = U * e(), U2 * e(), W * e(), W2 * e()
    Pin = torch.softmax(torch.randn(N, H, S, generator=g, device=dev), -1)
    return U, U2, W, W2, add0, X, Pin


def split(v):
    """(hi, lo) float64: hi = bf16(v), lo = bf16(v - hi) - split8 of csrc/attention.hip (v - hi is exact in f32)."""
    v = v.to(F32)
    hi = bf16(v)
    return hi.to(F64), bf16(v - hi).to(F64)


def cls_keep_rows(keep_full, N, H, S):
    """The mask of query row 0 out of the mask over the whole [N, H, S, S] tensor (flat index ((n H + h) S + 0) S + j)."""
    return keep_full.view(N, H, S, S)[:, :, 0, :]


def cls_dot(U, X, mode, Pin=None, keep=None, p=0.0, dtype=F64, fmt=False):
    """(out, probs).  mode 0: out = U . X over c; 1: probs = softmax_j, out = dropout(probs); 2: out = P (dP - sum_j dP P) with
    dP = dot keep / (1 - p), P = ``Pin``.  fmt: U enters as the hi + lo pair the kernel contracts (float64)."""
    if fmt:
        hi, lo = split(U)
        Ue = hi + lo
    else:
        Ue = U.to(dtype)
    s = torch.einsum("nhc,njc->nhj", Ue, X.to(Ue.dtype))
    if mode == 0:
        return s, None
    k = torch.ones_like(s) if keep is None else keep.to(s.dtype)
    sc = drop_scale(p, s.dtype).to(s.device)
    if mode == 1:
        P = torch.softmax(s, -1)
        return P * k * sc, P
    dP = s * k * sc
    P = Pin.to(s.dtype)
    return P * (dP - (dP * P).sum(-1, keepdim=True)), None


def cls_dot_terms(U, X, mode, Pin=None, keep=None, p=0.0):
    """terms_abs of (out, probs).  B = sum_c |U X| per score.  softmax: d p_j = p_j (d s_j - sum_k p_k d s_k), at most
    2 p_j max_k |d s_k|, so a probability's terms are p_j (2 max_j B + 1) (the 1: its own rounding), times keep / (1 - p) for the
    dropped copy.  mode 2: P (B' + sum_j P B') with B' = B keep / (1 - p)."""
    B = torch.einsum("nhc,njc->nhj", U.to(F64).abs(), X.to(F64).abs())
    if mode == 0:
        return B, None
    k = torch.ones_like(B) if keep is None else keep.to(F64)
    sc = drop_scale(p).to(B.device)
    if mode == 1:
        _, P = cls_dot(U, X, 1)
        tp = P * (2.0 * B.amax(-1, keepdim=True) + 1.0)
        return tp * k * sc, tp
    Bk = B * k * sc
    P = Pin.to(F64)
    return P * (Bk + (Bk * P).sum(-1, keepdim=True)), None


def cls_wsum(W, X, dtype=F64):
    return torch.einsum("nhj,njc->nhc", W.to(dtype), X.to(dtype))


def cls_wsum_terms(W, X):
    return torch.einsum("nhj,njc->nhc", W.to(F64).abs(), X.to(F64).abs())


def cls_outer(W1, U1, W2, U2, add0=None, dtype=F64, fmt=None, heads=None):
    """dX [N, S, d] = sum_h W1 U1 + W2 U2 (+ add0 on row 0 of every sequence).  fmt = "kept": the six hi / lo products the kernel
    forms (U hi W hi + U lo W hi + U hi W lo per operand pair; lo x lo dropped), in float64; "hi_only": only hi x hi (the defect of
    the host file).  heads: contract the first ``heads`` heads only (a defect too)."""
    def prod(W, U):
        if heads is not None:
            W, U = W[:, :heads], U[:, :heads]
        e = lambda a, b: torch.einsum("nhj,nhc->njc", a, b)
        if fmt is None:
            return e(W.to(dtype), U.to(dtype))
        (wh, wl), (uh, ul) = split(W), split(U)
        return e(wh, uh) if fmt == "hi_only" else e(wh, uh) + e(wh, ul) + e(wl, uh)
    o = prod(W1, U1) + prod(W2, U2)
    if add0 is not None:
        o[:, 0, :] += add0.to(o.dtype)
    return o


def cls_outer_terms(W1, U1, W2, U2, add0=None):
    a = lambda t: t.to(F64).abs()
    t = torch.einsum("nhj,nhc->njc", a(W1), a(U1)) + torch.einsum("nhj,nhc->njc", a(W2), a(U2))
    if add0 is not None:
        t[:, 0, :] += a(add0)
    return t
