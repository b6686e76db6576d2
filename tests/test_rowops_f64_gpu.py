"""The plain row-wise, head, loss and optimizer kernels (csrc/rowops.hip, csrc/loss.hip) against the float64 references of
tests/util_rowops.py, branch by branch: every parametrised case is named after the kernel instantiation it reaches.

The fused and packed forms are pinned to these kernels elsewhere (tests/test_hip_parity.py, tests/test_act16_gpu.py); nothing
else pins these kernels themselves.  Inputs are drawn on the CPU and every reference is computed there, in float64.

One tolerance rule (util_rowops.tol): per output tensor, 8 * max(e32, 4 * 2**-24 * B) with e32 the error of a plain torch float32
evaluation of the same formulas on the same input and B the largest sum of |terms| added into one output element.  Every check
prints err / tol; the worst ratio per kernel family is printed when the module finishes."""
import ctypes as C
import math

import pytest
import torch

import util_rowops as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = -777.25
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for fam in sorted(WORST):
        print("rowops-f64 worst err/tol  %-12s %.3f  (%s)" % ((fam,) + WORST[fam]))


def _L():
    from lstc_vad_amd import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.check(getattr(L.load(), name)(*args, L.stream_ptr()), name)


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def _buf(shape, src=None, off=0, fill=GUARD):
    """A device tensor of ``shape`` that starts ``off`` floats into a larger buffer (off = 1: not 16-byte aligned), with guard
    values in front of it and one behind.  Returns (view, whole buffer)."""
    n = int(math.prod(shape))
    buf = torch.full((off + n + 1,), fill, device=DEV, dtype=F32)
    view = buf[off:off + n].view(*shape)
    if src is not None:
        view.copy_(src.to(F32))
    assert (view.data_ptr() % 16 == 0) == (off % 4 == 0)
    return view, buf


def _guards_ok(buf, off):
    return bool((buf[:off] == GUARD).all()) and float(buf[-1]) == GUARD


class Checks:
    """Collects the comparisons of one test; ``done`` asserts them together so a failure shows every output's figures."""

    def __init__(self, family, case):
        self.family, self.case, self.bad = family, case, []

    def close(self, what, got, ref64, f32, terms):
        got = got.detach().cpu().to(F64)
        assert got.shape == ref64.shape, (self.case, what, got.shape, ref64.shape)
        t = R.tol(ref64, f32, terms)
        err = float((got - ref64).abs().max()) if torch.isfinite(got).all() else float("inf")
        ratio = err / t if t > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %s %s: err %.3e tol %.3e ratio %.3f" % (self.family, self.case, what, err, t, ratio))
        if ratio >= WORST.get(self.family, (-1.0, ""))[0]:
            WORST[self.family] = (ratio, "%s %s" % (self.case, what))
        if not ratio <= 1.0:
            self.bad.append((what, err, t))

    def true(self, what, cond):
        if not cond:
            self.bad.append((what, "false"))

    def done(self):
        assert not self.bad, (self.family, self.case, self.bad)


# ============================================================================================ LayerNorm
EPS = 1e-6
# (d, forward branch, backward branch, operands one float off 16-byte alignment)
# ln_bwd_pair<NVH, 0>: the second wave of a row's pair owns the float4 columns from 64 * NVH on - none (d = 4 ... 256), one (260, 516,
# 1028), a part (768, 2044) or all it has registers for (512, 1024, 2048)
LN_WIDTHS = [
    (4, "ln_fwd_vec1", "ln_bwd_pair_1_0", False), (8, "ln_fwd_vec1", "ln_bwd_pair_1_0", False),
    (24, "ln_fwd_vec1", "ln_bwd_pair_1_0", False),
    (100, "ln_fwd_vec1_partial_lanes", "ln_bwd_pair_1_0_partial_lanes", False), (256, "ln_fwd_vec1", "ln_bwd_pair_1_0", False),
    (260, "ln_fwd_vec2", "ln_bwd_pair_1_0", False), (512, "ln_fwd_vec2", "ln_bwd_pair_1_0", False),
    (516, "ln_fwd_vec4", "ln_bwd_pair_2_0", False), (768, "ln_fwd_vec4", "ln_bwd_pair_2_0", False),
    (1024, "ln_fwd_vec4", "ln_bwd_pair_2_0", False), (1028, "ln_fwd_vec8", "ln_bwd_pair_4_0", False),
    (2044, "ln_fwd_vec8", "ln_bwd_pair_4_0", False), (2048, "ln_fwd_vec8", "ln_bwd_pair_4_0", False),
    (37, "ln_fwd_generic", "ln_bwd_generic", False), (2050, "ln_fwd_generic", "ln_bwd_generic", False),
    (2052, "ln_fwd_generic", "ln_bwd_generic", False), (64, "ln_fwd_generic_unaligned", "ln_bwd_generic_unaligned", True),
]
LN_FAMILIES = ("randn", "shifted100", "constant_row")


def _ln_inputs(rows, d, family, *key):
    g = _gen(rows, d, LN_FAMILIES.index(family), *key)
    x = torch.randn(rows, d, generator=g)
    const = None
    if family == "shifted100":
        x = x + 100.0                       # a one-pass variance E[x^2] - E[x]^2 would lose its digits here
    elif family == "constant_row":
        const = rows // 2
        x[const] = 2.0                      # variance 0 (and a sum float32 forms exactly): rstd = 1 / sqrt(eps), y = beta
    gamma = 1.0 + 0.5 * torch.randn(d, generator=g)
    beta = torch.randn(d, generator=g)
    return x, gamma, beta, const


def _ln_fwd_gpu(x, gamma, beta, off):
    rows, d = x.shape
    xd, xb = _buf((rows, d), x, off)
    yd, yb = _buf((rows, d), None, off)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    mean = torch.full((rows,), float("nan"), device=DEV)
    rstd = torch.full((rows,), float("nan"), device=DEV)
    P = _L().dev_ptr
    _call("lstc_layernorm_fwd", P(xd), P(gd), P(bd), P(yd), P(mean), P(rstd), rows, d, EPS)
    torch.cuda.synchronize()
    return xd, yd, mean, rstd, gd, bd, _guards_ok(yb, off) and _guards_ok(xb, off) and torch.equal(xd.cpu(), x)


def _ln_fwd_check(ck, tag, x, gamma, beta, const, y, mean, rstd):
    ref = R.ln_fwd(x, gamma, beta, EPS)
    f32 = R.ln_fwd(x, gamma, beta, EPS, dtype=F32)
    terms = R.ln_fwd_terms(x, gamma, beta, EPS)
    rows = x.shape[0]
    # the constant row's terms (|x| rstd = 2000) would set the tolerance of every other row: it is checked on its own
    groups = [("", torch.arange(rows))] if const is None else \
        [("", torch.tensor([r for r in range(rows) if r != const], dtype=torch.long)), ("const_row ", torch.tensor([const]))]
    for gname, idx in groups:
        if idx.numel() == 0:
            continue
        for name, got, i in (("y", y, 0), ("mean", mean, 1), ("rstd", rstd, 2)):
            ck.close("%s %s%s" % (tag, gname, name), got[idx.to(got.device)], ref[i][idx], f32[i][idx], terms[i][idx])


# worst err / tol measured on an MI355X: 0.078 (ln_fwd_vec8, d = 2048, rows = 1, randn, y)
@pytest.mark.parametrize("rows", [1, 5, 37])
@pytest.mark.parametrize("d,branch,_b,unaligned", LN_WIDTHS, ids=["%s-d%d" % (w[1], w[0]) for w in LN_WIDTHS])
def test_layernorm_fwd(d, branch, _b, unaligned, rows):
    ck = Checks("ln_fwd", "%s d=%d rows=%d" % (branch, d, rows))
    for family in LN_FAMILIES:
        x, gamma, beta, const = _ln_inputs(rows, d, family)
        _, y, mean, rstd, _, _, intact = _ln_fwd_gpu(x, gamma, beta, 1 if unaligned else 0)
        ck.true(family + " x unchanged, floats around y unchanged", intact)
        _ln_fwd_check(ck, family, x, gamma, beta, const, y, mean, rstd)
    ck.done()


def test_layernorm_fwd_grid_stride_second_trip():
    """rows = 16400 > 4096 workgroups x 4 waves: the last 16 rows are a wave's second trip (ln_fwd_vec<1>, d = 24)."""
    ck = Checks("ln_fwd", "ln_fwd_vec1 d=24 rows=16400")
    x, gamma, beta, const = _ln_inputs(16400, 24, "constant_row")
    _, y, mean, rstd, _, _, intact = _ln_fwd_gpu(x, gamma, beta, 0)
    ck.true("guards", intact)
    _ln_fwd_check(ck, "second_trip", x, gamma, beta, const, y, mean, rstd)
    ck.done()


LN_BWD_SHAPES = [(1, 1), (5, 4), (5, 1), (37, 9), (300, 512)]
LN_BWD_IDS = ["rows1-np1", "rows5-np4_more_workgroups_than_rows_dead_slots", "rows5-np1_one_workgroup_walks_every_row", "rows37-np9",
              "rows300-np512_idle_workgroups"]


def _ln_bwd_id(d, branch):
    """The case id: the branch label, except that d = 512 / 1024 / 2048 keep the ids they have had since the wave-pair kernel was
    called ln_bwd_pack2 - the same kernel instantiations and the same assertions, so their record in test reports goes on."""
    return "%s-d%d" % (branch.replace("ln_bwd_pair", "ln_bwd_pack2") if d in (512, 1024, 2048) else branch, d)


# worst err / tol measured on an MI355X: 0.059 (ln_bwd_generic, d = 2052, rows = 37, n_partial = 9, forward + backward, dx)
@pytest.mark.parametrize("rows,n_partial", LN_BWD_SHAPES, ids=LN_BWD_IDS)
@pytest.mark.parametrize("d,_f,branch,unaligned", LN_WIDTHS, ids=[_ln_bwd_id(w[0], w[2]) for w in LN_WIDTHS])
def test_layernorm_bwd(d, _f, branch, unaligned, rows, n_partial):
    """dx, the per-workgroup partial rows, and dgamma / dbeta after the column sum: once with the KERNEL's saved mean / rstd
    promoted to float64 (the backward alone) and once with the reference's own statistics (forward + backward together).
    (rows, n_partial): more workgroups than rows, dead slots of the wave-pair kernel, one workgroup walking every row."""
    from lstc_vad_amd import functional as Fn
    P = _L().dev_ptr
    off = 1 if unaligned else 0
    ck = Checks("ln_bwd", "%s d=%d rows=%d np=%d" % (branch, d, rows, n_partial))
    x, gamma, beta, _ = _ln_inputs(rows, d, "randn", 7)
    x = 0.3 + 1.5 * x
    dy = torch.randn(rows, d, generator=_gen(rows, d, n_partial, 11))
    xd, _, mean, rstd, gd, _, _ = _ln_fwd_gpu(x, gamma, beta, off)
    dyd, dyb = _buf((rows, d), dy, off)
    dxd, dxb = _buf((rows, d), None, off)
    partial = torch.full((2, n_partial, d), float("nan"), device=DEV)
    _call("lstc_layernorm_bwd", P(dyd), P(xd), P(gd), P(mean), P(rstd), P(dxd), P(partial), n_partial, rows, d)
    sums = Fn.colsum_planes(partial)
    torch.cuda.synchronize()
    ck.true("floats around dx unchanged", _guards_ok(dxb, off) and _guards_ok(dyb, off))
    # workgroups that own no row: 2 rows per workgroup in the wave-pair kernel, 4 (one per wave) in the generic one
    per_wg = 2 if "pair" in branch else 4
    idle0 = (rows + per_wg - 1) // per_wg
    ck.true("partial finite", bool(torch.isfinite(partial).all()))
    ck.true("idle workgroups' partial rows are exact zeros", bool((partial[:, idle0:, :] == 0).all()))
    own = R.ln_fwd(x, gamma, beta, EPS)
    own32 = R.ln_fwd(x, gamma, beta, EPS, dtype=F32)
    for tag, m, r, m32, r32 in (("alone", mean.cpu().to(F64), rstd.cpu().to(F64), mean.cpu(), rstd.cpu()),
                                ("fwd+bwd", own[1], own[2], own32[1], own32[2])):
        ref = R.ln_bwd(dy, x, gamma, m, r)
        f32 = R.ln_bwd(dy, x, gamma, m32, r32, dtype=F32)
        terms = R.ln_bwd_terms(dy, x, gamma, m, r)
        ck.close(tag + " dx", dxd, ref[0], f32[0], terms[0])
        ck.close(tag + " dgamma", sums[0], ref[1], f32[1], terms[1])
        ck.close(tag + " dbeta", sums[1], ref[2], f32[2], terms[2])
        ck.close(tag + " partial rows summed", partial.cpu().to(F64).sum(1), torch.stack([ref[1], ref[2]]),
                 torch.stack([f32[1], f32[2]]), torch.stack([terms[1], terms[2]]))
    if d in (512, 1024, 2048):
        # the widths lstc_layernorm_bwd_drop accepts: the wave-pair kernel's MODE 0 and MODE 2 promise the same dx bit for bit
        # (p = 0: df = dx as well)
        dx2, df = torch.empty(rows, d, device=DEV), torch.empty(rows, d, device=DEV)
        partial3 = torch.empty(3, n_partial, d, device=DEV)
        _call("lstc_layernorm_bwd_drop", P(dyd), P(xd), P(gd), P(mean), P(rstd), P(dx2), P(df), P(partial3), n_partial, rows, d,
              0.0, 5)
        torch.cuda.synchronize()
        ck.true("dx bit-identical to lstc_layernorm_bwd_drop(p=0)", torch.equal(dx2, dxd) and torch.equal(df, dxd))
        ck.true("partials bit-identical to lstc_layernorm_bwd_drop(p=0)", torch.equal(partial3[:2], partial))
    ck.done()


# ============================================================================================ column sums
def _colsum_gpu(x, cols, n_partial, out0, off_out=0):
    rows, ld = x.shape
    P = _L().dev_ptr
    xd = x.to(DEV)
    partial = torch.full((max(min(rows, n_partial), 1) * cols,), float("nan"), device=DEV)
    out, outb = _buf((cols,), out0 if out0 is not None else None, off_out)
    _call("lstc_colsum", P(xd), rows, cols, ld, P(partial), n_partial, P(out), int(out0 is not None))
    torch.cuda.synchronize()
    assert _guards_ok(outb, off_out)
    return out


# worst err / tol measured on an MI355X: 0.069 (two-pass, rows = 4, cols = 1, accumulate)
@pytest.mark.parametrize("cols", [1, 3, 64, 65, 260])
@pytest.mark.parametrize("rows", [1, 4, 12, 13, 129, 1000])
def test_colsum(rows, cols):
    """lstc_colsum (one-pass colsum_few where rows <= 12, rows <= n_partial and columns / ld / bases allow float4; the two-pass
    form otherwise) and lstc_colsum_batched over 3 planes, ld > cols, accumulate on and off, against the float64 sum."""
    P = _L().dev_ptr
    ck = Checks("colsum", "rows=%d cols=%d" % (rows, cols))
    g = _gen(rows, cols, 3)
    for ld in (cols + 4, cols + 3):
        x3 = 0.5 + torch.randn(3, rows, ld, generator=g)
        out0 = torch.randn(cols, generator=g)
        for n_partial in sorted({min(rows, 128), 7}):
            few = rows <= 12 and rows <= n_partial and cols % 4 == 0 and ld % 4 == 0
            tag = "%s ld=%d np=%d" % ("colsum_few" if few else "two_pass", ld, n_partial)
            x = x3[0]
            ref, f32, terms = R.colsum(x[:, :cols]), R.colsum(x[:, :cols], F32), R.colsum_terms(x[:, :cols])
            ck.close(tag + " write", _colsum_gpu(x, cols, n_partial, None), ref, f32, terms)
            ck.close(tag + " accumulate", _colsum_gpu(x, cols, n_partial, out0), ref + out0.to(F64), f32 + out0,
                     terms + out0.to(F64).abs())
            xd = x3.to(DEV)
            npb = min(rows, n_partial)
            partial = torch.full((3 * npb * cols,), float("nan"), device=DEV)
            outb = torch.full((3, cols), float("nan"), device=DEV)
            _call("lstc_colsum_batched", P(xd), 3, rows, cols, ld, rows * ld, P(partial), n_partial, P(outb))
            torch.cuda.synchronize()
            ck.close("batched ld=%d np=%d" % (ld, n_partial), outb, torch.stack([R.colsum(p[:, :cols]) for p in x3]),
                     torch.stack([R.colsum(p[:, :cols], F32) for p in x3]), torch.stack([R.colsum_terms(p[:, :cols]) for p in x3]))
    ck.done()


@pytest.mark.parametrize("rows", [1, 4, 12], ids=lambda r: "colsum_few_vs_two_pass-r%d" % r)
def test_colsum_few_and_two_pass(rows):
    """The same few rows through colsum_few and (``out`` one float off alignment) through pass 1 + pass 2: each against the
    float64 sum, and bit-identical to each other as csrc/rowops.hip promises."""
    ck = Checks("colsum", "few_vs_two_pass rows=%d" % rows)
    cols, ld = 260, 264
    x = 0.5 + torch.randn(rows, ld, generator=_gen(rows, 99))
    ref, f32, terms = R.colsum(x[:, :cols]), R.colsum(x[:, :cols], F32), R.colsum_terms(x[:, :cols])
    few = _colsum_gpu(x, cols, rows, None)
    two = _colsum_gpu(x, cols, rows, None, off_out=1)
    ck.close("colsum_few", few, ref, f32, terms)
    ck.close("two_pass", two, ref, f32, terms)
    ck.true("bit-identical", torch.equal(few, two))
    ck.done()


# ============================================================================================ CLS concat
CLS_SHAPES = [(1, 2, 4, "cls_concat_fwd_vec4"), (3, 17, 24, "cls_concat_fwd_vec4"), (5, 50, 37, "cls_concat_fwd_scalar"),
              (2, 82, 260, "cls_concat_fwd_vec4_two_column_groups")]


# worst err / tol measured on an MI355X: 0.098 (vec4, N = 2, S = 82, d = 260, the mean token)
@pytest.mark.parametrize("N,S,d,branch", CLS_SHAPES, ids=["%s-%dx%dx%d" % (s[3], s[0], s[1], s[2]) for s in CLS_SHAPES])
def test_cls_concat_fwd(N, S, d, branch):
    """Mean and learned token, with and without ``pos``, with and without the x / x_hi split at n_lo in {0, 1, N}.  The copied
    tokens must be exact; only the mean token and the sums with ``pos`` get a tolerance."""
    P = _L().dev_ptr
    ck = Checks("cls_concat", "%s N=%d S=%d d=%d" % (branch, N, S, d))
    g = _gen(N, S, d)
    x = 0.5 + torch.randn(N, S - 1, d, generator=g)
    cls, pos = torch.randn(d, generator=g), torch.randn(S, d, generator=g)
    xd, clsd, posd = x.to(DEV), cls.to(DEV), pos.to(DEV)
    dummy = torch.full((4,), float("nan"), device=DEV)
    for n_lo in (None, 0, 1, N):
        if n_lo is None:
            lo, hi, a_lo, a_hi, a_n = x, None, xd, None, 0
        else:
            lo, hi = x[:n_lo], x[n_lo:]
            # the side that holds no sequence is never read: a 4-float NaN buffer stands in for it
            a_lo = lo.contiguous().to(DEV) if n_lo > 0 else dummy
            a_hi = hi.contiguous().to(DEV) if n_lo < N else dummy
            a_n = n_lo
        for use_cls in (False, True):
            for use_pos in (False, True):
                tag = "n_lo=%s %s%s" % (n_lo, "learned" if use_cls else "mean", "+pos" if use_pos else "")
                y = torch.full((N, S, d), float("nan"), device=DEV)
                _call("lstc_cls_concat_fwd", P(a_lo), P(a_hi), a_n, P(clsd) if use_cls else None, P(posd) if use_pos else None,
                      P(y), N, S, d)
                torch.cuda.synchronize()
                kw = dict(cls=cls if use_cls else None, pos=pos if use_pos else None, x_hi=hi, n_lo=a_n)
                ref, f32, terms = R.cls_concat_fwd(lo, **kw), R.cls_concat_fwd(lo, dtype=F32, **kw), R.cls_concat_terms(lo, **kw)
                yc = y.cpu()
                if use_pos:
                    ck.close(tag + " tokens", yc[:, 1:], ref[:, 1:], f32[:, 1:], terms[:, 1:])
                else:
                    ck.true(tag + " tokens copied exactly", torch.equal(yc[:, 1:], x))
                if use_cls and not use_pos:
                    ck.true(tag + " token 0 = cls exactly", torch.equal(yc[:, 0], cls.expand(N, d)))
                else:
                    ck.close(tag + " token 0", yc[:, 0], ref[:, 0], f32[:, 0], terms[:, 0])
    ck.done()


@pytest.mark.parametrize("mean_cls", [0, 1])
@pytest.mark.parametrize("N,S,d,_b", CLS_SHAPES, ids=["cls_concat_bwd-%dx%dx%d" % (s[0], s[1], s[2]) for s in CLS_SHAPES])
def test_cls_concat_bwd(N, S, d, _b, mean_cls):
    P = _L().dev_ptr
    ck = Checks("cls_concat", "bwd N=%d S=%d d=%d mean_cls=%d" % (N, S, d, mean_cls))
    dy = torch.randn(N, S, d, generator=_gen(N, S, d, 5))
    dyd = dy.to(DEV)
    dx, dxb = _buf((N, S - 1, d), None, 0)
    _call("lstc_cls_concat_bwd", P(dyd), P(dx), N, S, d, mean_cls)
    torch.cuda.synchronize()
    ck.true("guard", _guards_ok(dxb, 0))
    if mean_cls:
        ck.close("dx", dx, R.cls_concat_bwd(dy, 1), R.cls_concat_bwd(dy, 1, F32),
                 dy[:, 1:].to(F64).abs() + dy[:, :1].to(F64).abs() / (S - 1))
    else:
        ck.true("dx copied exactly", torch.equal(dx.cpu(), dy[:, 1:]))
    ck.done()


# ============================================================================================ head output
def _head_case(c, rows, saturated):
    g = _gen(c, rows, int(saturated), 21)
    x = torch.randn(rows, 32, generator=g)
    W = torch.randn(c, 32, generator=g) / 32 ** 0.5
    b = 0.3 * torch.randn(c, generator=g)
    if saturated:                           # logits (c = 1) / logit differences (c = 2) of +-40
        x = 0.01 * x
        x[:, 0] = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)
        W = 0.1 * W
        W[:, 0] = torch.tensor([40.0]) if c == 1 else torch.tensor([20.0, -20.0])
    dout = torch.randn(rows, c, generator=g)
    return x, W, b, dout


HEAD_CASES = [(c, rows, False) for c in (1, 2) for rows in (1, 63, 64, 257, 1000)] + [(1, 130, True), (2, 130, True)]


def _head_id(case):
    c, rows, sat = case
    note = "_saturated_pm40" if sat else "_idle_waves" if rows < 64 else "" if rows % 256 == 0 else "_ragged_rows"
    return "head_out_fwd_bwd_c%d-r%d%s" % (c, rows, note)


# worst err / tol measured on an MI355X: 0.016 (c = 1, rows = 1000, dx)
@pytest.mark.parametrize("case", HEAD_CASES, ids=[_head_id(c) for c in HEAD_CASES])
def test_head_out(case):
    """head_out_fwd_kernel and head_out_bwd_kernel: out, dx and the fixed-order dW / db reduction of ONE workgroup, for row
    counts that leave whole waves idle (< 64) or are no multiple of 256.  dW and db are pre-filled with NaN: they must be
    written, not added to.  The backward is given the kernel's own ``out``, as in the product."""
    c, rows, saturated = case
    P = _L().dev_ptr
    ck = Checks("head", _head_id(case))
    x, W, b, dout = _head_case(c, rows, saturated)
    xd, Wd, bd, dd = x.to(DEV), W.to(DEV), b.to(DEV), dout.to(DEV)
    out, outb = _buf((rows, c), None, 0, fill=float("nan"))
    _call("lstc_head_out_fwd", P(xd), P(Wd), P(bd), P(out), rows, c)
    dx = torch.full((rows, 32), float("nan"), device=DEV)
    dW = torch.full((c, 32), float("nan"), device=DEV)
    db = torch.full((c,), float("nan"), device=DEV)
    _call("lstc_head_out_bwd", P(xd), P(Wd), P(out), P(dd), P(dx), P(dW), P(db), rows, c)
    torch.cuda.synchronize()
    ref_o, f32_o = R.head_fwd(x, W, b), R.head_fwd(x, W, b, F32)
    ref, f32 = R.head_bwd(x, W, ref_o, dout), R.head_bwd(x, W, f32_o, dout, F32)
    terms = R.head_terms(x, W, b, dout)
    if saturated:
        z = x.to(F64) @ W.to(F64).t()
        ck.true("logits reach +-40", float((z if c == 1 else z[:, :1] - z[:, 1:]).abs().min()) > 39.0)
    ck.close("out", out, ref_o, f32_o, terms[0])
    ck.close("dx", dx, ref[0], f32[0], terms[1])
    ck.close("dW", dW, ref[1], f32[1], terms[2])
    ck.close("db", db, ref[2], f32[2], terms[3])
    ck.done()


# ============================================================================================ loss
LAMBDAS = dict(lambda_1=0.05, lambda_MIL=0.9, lambda_aux=0.8, lambda_normal=0.2, lambda_abnormal=2.0)
# seeds chosen on the CPU so that, in float64, no hinge argument and no gap between a video's two largest part means lies within
# 1e-4 of zero (asserted below): (mode, bs, part_num, score_len) -> seed
LOSS_SEEDS = {(0, 3, 2, 2): 1, (0, 130, 2, 2): 5, (1, 3, 4, 1): 1, (1, 130, 3, 1): 4, (2, 3, 2, 2): 1, (2, 130, 2, 2): 2,
              (0, 6, 2, 2): 1, (1, 6, 4, 1): 1, (2, 6, 2, 2): 1}


def _loss_inputs(mode, bs, pn, Ls, seed):
    """Scores beyond [0, 1] for modes 0 and 1, so that the hinge 1 - abn + nor takes both signs (the kernel does not ask for
    probabilities); mode 2's BCE takes logarithms of o and 1 - o: (0.05, 0.95)."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * bs * pn * Ls
    if mode == 1:
        out = 3.0 * torch.rand(n, 2, generator=g) - 1.0
    elif mode == 0:
        out = 3.0 * torch.rand(n, 1, generator=g) - 1.0
    else:
        out = 0.05 + 0.9 * torch.rand(n, 1, generator=g)
    labels = {L: torch.rand(bs, pn * L, generator=g) for L in (1, 3)}
    targets = torch.rand(2 * bs * pn, 2, generator=g)
    return out, labels, targets


def _loss_gpu(mode, out, bs_g, bs_l, rank_off, pn, Ls, l1_skip, phase, bag, abn_labels=None, label_len=1, targets=None):
    L = _L()
    d = L.LossDesc()
    d.mode, d.bs_global, d.bs_local, d.rank_off = mode, bs_g, bs_l, rank_off
    d.part_num, d.score_len, d.label_len, d.l1_skip = pn, Ls, label_len, l1_skip
    d.lambda_1, d.lambda_MIL, d.lambda_aux = LAMBDAS["lambda_1"], LAMBDAS["lambda_MIL"], LAMBDAS["lambda_aux"]
    d.lambda_normal, d.lambda_abnormal = LAMBDAS["lambda_normal"], LAMBDAS["lambda_abnormal"]
    od = out.contiguous().to(DEV)
    ld = abn_labels.contiguous().to(DEV) if abn_labels is not None else None
    td = targets.contiguous().to(DEV) if targets is not None else None
    dout = torch.full_like(od, float("nan"))
    sc = torch.full((5,), float("nan"), device=DEV)
    d.out, d.abn_labels, d.targets, d.bag = L.dev_ptr(od), L.dev_ptr(ld), L.dev_ptr(td), L.dev_ptr(bag)
    d.dout, d.scalars, d.phase = L.dev_ptr(dout), L.dev_ptr(sc), phase
    L.check(L.load().lstc_vad_loss(C.byref(d), L.stream_ptr()), "lstc_vad_loss")
    torch.cuda.synchronize()
    return sc.cpu(), dout.cpu()


def _loss_variant(variant, labels, targets):
    if variant == "labels_L1":
        return dict(abn_labels=labels[1], label_len=1)
    if variant == "labels_L3":
        return dict(abn_labels=labels[3], label_len=3)
    if variant == "targets":
        return dict(targets=targets)
    return {}


def _assert_margins(mode, out, bs, pn, Ls):
    hinge, gap = R.loss_margins(mode, out, bs, pn, Ls)
    print("loss margins: hinge %.3e top-2 gap %.3e" % (hinge, gap))
    assert hinge > 1e-4 and gap > 1e-4, ("input too close to a discontinuity of the loss: choose another seed", hinge, gap)


LOSS_SHAPES = {0: [(3, 2, 2), (130, 2, 2)], 1: [(3, 4, 1), (130, 3, 1)], 2: [(3, 2, 2), (130, 2, 2)]}
LOSS_CASES = [(m, s, v, skip) for m in (0, 1, 2) for s in LOSS_SHAPES[m]
              for v in (("no_aux",) if m == 0 else ("labels_L1", "labels_L3", "targets", "no_aux")) for skip in ("skip_bs", "skip_normal_half")]


def _loss_id(case):
    m, (bs, pn, Ls), v, skip = case
    return "vad_loss_mode%d-bs%d_pn%d_L%d%s-%s-%s" % (m, bs, pn, Ls, "_second_trip" if 2 * bs > 256 else "", v, skip)


# worst err / tol measured on an MI355X: 0.082 (mode 2, bs = 130, labels of length 3, the BCE scalar)
@pytest.mark.parametrize("case", LOSS_CASES, ids=[_loss_id(c) for c in LOSS_CASES])
def test_vad_loss_single_rank(case):
    """All five scalars and d(loss)/d(out) of one launch (phase 2) against the float64 loss built from the oracle's pieces.
    bs = 130: 2 * bs_local = 260 > 256 threads, so every per-video loop of the kernel makes its second trip.  l1_skip takes the
    two values the training scripts pass: bs (a flat score vector sliced at batch_size) and bs * part_num * score_len."""
    mode, (bs, pn, Ls), variant, skip = case
    ck = Checks("loss", _loss_id(case))
    out, labels, targets = _loss_inputs(mode, bs, pn, Ls, LOSS_SEEDS[(mode, bs, pn, Ls)])
    _assert_margins(mode, out, bs, pn, Ls)
    l1_skip = bs if skip == "skip_bs" else bs * pn * Ls
    aux = _loss_variant(variant, labels, targets)
    sc, dout = _loss_gpu(mode, out, bs, bs, 0, pn, Ls, l1_skip, 2, None, **aux)
    ref = R.loss_ref(mode, out, bs, pn, Ls, l1_skip, **LAMBDAS, **aux)
    f32 = R.loss_ref(mode, out, bs, pn, Ls, l1_skip, dtype=F32, **LAMBDAS, **aux)
    terms = R.loss_terms(mode, out, bs, pn, Ls, l1_skip, **LAMBDAS, **aux)
    for i, name in enumerate(("loss", "mil", "err", "l1", "aux")):
        ck.close(name, sc[i:i + 1], ref[0][i:i + 1], f32[0][i:i + 1], terms[0][i:i + 1])
    ck.close("dout", dout, ref[1], f32[1], terms[1])
    ck.done()


SHARD_CASES = [(m, skip) for m in (0, 1, 2) for skip in ("skip_bs", "skip_normal_half")]


@pytest.mark.parametrize("mode,skip", SHARD_CASES, ids=["vad_loss_mode%d-sharded_2+4-%s" % c for c in SHARD_CASES])
def test_vad_loss_sharded(mode, skip):
    """bs_global = 6 split over two ranks as 2 + 4 (rank_off 0 and 2): phase 0 per rank, the emulated exchange (the sum of the
    ranks' zero-padded bag vectors), phase 1 per rank.  The SUM of the ranks' scalars and their ``dout`` put back in global
    order are compared with the single float64 loss."""
    bs, (pn, Ls) = 6, ((4, 1) if mode == 1 else (2, 2))
    rpv = pn * Ls
    ck = Checks("loss", "mode%d sharded 2+4 %s" % (mode, skip))
    out, labels, _ = _loss_inputs(mode, bs, pn, Ls, LOSS_SEEDS[(mode, bs, pn, Ls)])
    _assert_margins(mode, out, bs, pn, Ls)
    l1_skip = bs if skip == "skip_bs" else bs * rpv
    aux = dict(abn_labels=labels[3], label_len=3) if mode else {}
    ranks = [(0, 2), (2, 4)]
    shard = lambda off, bl: (out[R.shard_rows(bs, rpv, off, bl)], dict(aux, abn_labels=labels[3][off:off + bl]) if mode else {})
    bags = []
    for off, bl in ranks:
        o_r, aux_r = shard(off, bl)
        bag = torch.zeros(2 * bs, device=DEV)
        _loss_gpu(mode, o_r, bs, bl, off, pn, Ls, l1_skip, 0, bag, **aux_r)
        bags.append(bag)
    total = bags[0] + bags[1]                                   # what the sum-all-reduce leaves on every rank
    c = 2 if mode == 1 else 1
    bag_ref = out.to(F64)[:, c - 1].reshape(2 * bs, pn, Ls).mean(-1).max(-1)[0]
    ck.close("bag", total, bag_ref, out[:, c - 1].reshape(2 * bs, pn, Ls).mean(-1).max(-1)[0], out.abs().max())
    sc_sum = torch.zeros(5, dtype=F64)
    dout = torch.full(out.shape, float("nan"))
    for off, bl in ranks:
        o_r, aux_r = shard(off, bl)
        sc, g = _loss_gpu(mode, o_r, bs, bl, off, pn, Ls, l1_skip, 1, total.clone(), **aux_r)
        sc_sum += sc.to(F64)
        dout[R.shard_rows(bs, rpv, off, bl)] = g
    ref = R.loss_ref(mode, out, bs, pn, Ls, l1_skip, **LAMBDAS, **aux)
    f32 = R.loss_ref(mode, out, bs, pn, Ls, l1_skip, dtype=F32, **LAMBDAS, **aux)
    terms = R.loss_terms(mode, out, bs, pn, Ls, l1_skip, **LAMBDAS, **aux)
    for i, name in enumerate(("loss", "mil", "err", "l1", "aux")):
        ck.close("sum of ranks " + name, sc_sum[i:i + 1], ref[0][i:i + 1], f32[0][i:i + 1], terms[0][i:i + 1])
    ck.close("dout", dout, ref[1], f32[1], terms[1])
    ck.done()


# ============================================================================================ Adagrad, norms, clip
ADA_N = [1, 3, 4, 5, 1027, 8191, 8192, 8193, 16389]
LR, ADA_EPS = 1e-2, 1e-10


def _ada_id(n, off):
    if off:
        return "adagrad_unaligned_fallback-n%d" % n
    return "adagrad_vec4%s-n%d" % ("_scalar_tail" if n % 4 else "", n)


def _ada_tensors(n, off, *key):
    g = _gen(n, off, *key)
    w = torch.randn(n, generator=g)
    g1, g2 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    g1[::7] = 0.0                            # a zero gradient: with no weight decay the update is 0 / (0 + eps) = 0
    return w, g1, g2


# worst err / tol measured on an MI355X: 0.088 (n = 4, weight decay 1e-3, gscale 0.37, state after step 1)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "views_one_float_in"])
@pytest.mark.parametrize("n", ADA_N)
def test_adagrad_step(n, off):
    """adagrad_kernel against the update rule itself over two consecutive steps: the float4 body, the scalar tail (n % 4 != 0)
    and the scalar fallback for operands that are not 16-byte aligned; the floats on either side of each view stay as they were."""
    P = _L().dev_ptr
    ck = Checks("adagrad", _ada_id(n, off))
    w0, g1, g2 = _ada_tensors(n, off)
    for wd in (0.0, 1e-3):
        for gscale in (1.0, 0.37):
            tag = "wd=%g gscale=%g" % (wd, gscale)
            (w, wb), (s, sb) = _buf((n,), w0, off), _buf((n,), torch.zeros(n), off)
            rw, rs, fw, fs = w0.to(F64), torch.zeros(n, dtype=F64), w0.clone(), torch.zeros(n)
            tw, ts = rw.abs(), rs.clone()
            for step, grad in enumerate((g1, g2)):
                gd, gb = _buf((n,), grad, off)
                _call("lstc_adagrad_step", P(w), P(gd), P(s), n, LR, wd, ADA_EPS, gscale)
                torch.cuda.synchronize()
                # terms from the state before the step; errors of step 1 carry over: the two steps' terms add
                t = R.adagrad_terms(rw, grad, rs, LR, wd, ADA_EPS, gscale)
                tw, ts = tw + t[0], ts + t[1]
                rw, rs = R.adagrad(rw, grad, rs, LR, wd, ADA_EPS, gscale)
                fw, fs = R.adagrad(fw, grad, fs, LR, wd, ADA_EPS, gscale, dtype=F32)
                ck.close("%s step %d w" % (tag, step + 1), w, rw, fw, tw)
                ck.close("%s step %d state" % (tag, step + 1), s, rs, fs, ts)
                ck.true(tag + " grad unchanged", torch.equal(gd.cpu(), grad) and _guards_ok(gb, off))
            ck.true(tag + " floats around w / state unchanged", _guards_ok(wb, off) and _guards_ok(sb, off))
    ck.done()


def _multi_list(count=50):
    """``count`` tensors of the mixed sizes of ADA_N, every third one a view one float into its buffer, each with its own
    hyper-parameters.  8193 and 16389 end inside a workgroup's 8192-element slice; 50 > 48 takes two launches."""
    items = []
    for i in range(count):
        n, off = ADA_N[i % len(ADA_N)], 1 if i % 3 == 2 else 0
        w, g1, g2 = _ada_tensors(n, off, i)
        items.append(dict(n=n, off=off, w=w, g=(g1, g2), lr=LR * (1 + i % 4), wd=(0.0, 1e-3)[i % 2], gscale=(1.0, 0.37)[(i // 2) % 2]))
    return items


def test_adagrad_multi_two_launches_50_tensors():
    """adagrad_multi_kernel (50 tensors: 48 + 2 over two launches; tensors that end inside a workgroup's slice; aligned and
    unaligned ones mixed) against float64 over two steps, and bit for bit against adagrad_kernel run tensor by tensor."""
    L = _L()
    P = L.dev_ptr
    ck = Checks("adagrad", "adagrad_multi 50 tensors")
    items = _multi_list()
    for it in items:
        (it["dev_w"], it["wb"]), (it["dev_s"], it["sb"]) = _buf((it["n"],), it["w"], it["off"]), _buf((it["n"],), torch.zeros(it["n"]), it["off"])
        (it["one_w"], _), (it["one_s"], _) = _buf((it["n"],), it["w"], it["off"]), _buf((it["n"],), torch.zeros(it["n"]), it["off"])
        it["rw"], it["rs"], it["fw"], it["fs"] = it["w"].to(F64), torch.zeros(it["n"], dtype=F64), it["w"].clone(), torch.zeros(it["n"])
        it["tw"], it["ts"] = it["rw"].abs(), it["rs"].clone()
    for step in range(2):
        arr = (L.AdagradItem * len(items))()
        keep = []
        for a, it in zip(arr, items):
            gd, _ = _buf((it["n"],), it["g"][step], it["off"])
            keep.append(gd)
            a.w, a.grad, a.state, a.n = P(it["dev_w"]), P(gd), P(it["dev_s"]), it["n"]
            a.lr, a.weight_decay, a.eps, a.grad_scale = it["lr"], it["wd"], ADA_EPS, it["gscale"]
            _call("lstc_adagrad_step", P(it["one_w"]), P(gd), P(it["one_s"]), it["n"], it["lr"], it["wd"], ADA_EPS, it["gscale"])
        _call("lstc_adagrad_multi", arr, len(items))
        torch.cuda.synchronize()
        for i, it in enumerate(items):
            hp = (it["lr"], it["wd"], ADA_EPS, it["gscale"])
            t = R.adagrad_terms(it["rw"], it["g"][step], it["rs"], *hp)
            it["tw"], it["ts"] = it["tw"] + t[0], it["ts"] + t[1]
            it["rw"], it["rs"] = R.adagrad(it["rw"], it["g"][step], it["rs"], *hp)
            it["fw"], it["fs"] = R.adagrad(it["fw"], it["g"][step], it["fs"], *hp, dtype=F32)
            tag = "step %d tensor %d (n=%d%s)" % (step + 1, i, it["n"], ", unaligned" if it["off"] else "")
            ck.close(tag + " w", it["dev_w"], it["rw"], it["fw"], it["tw"])
            ck.close(tag + " state", it["dev_s"], it["rs"], it["fs"], it["ts"])
            ck.true(tag + " bit-identical to lstc_adagrad_step", torch.equal(it["dev_w"], it["one_w"]) and torch.equal(it["dev_s"], it["one_s"]))
            ck.true(tag + " guards", _guards_ok(it["wb"], it["off"]) and _guards_ok(it["sb"], it["off"]))
    ck.done()


# worst err / tol measured on an MI355X: 0.047 (lstc_sqnorm_accum, n = 4)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "view_one_float_in"])
@pytest.mark.parametrize("n", ADA_N)
def test_sqnorm_accum_and_scale(n, off):
    """lstc_sqnorm_accum (adds onto what ``out`` holds) and lstc_scale, against float64."""
    P = _L().dev_ptr
    ck = Checks("norm_clip", "sqnorm_accum/scale n=%d off=%d" % (n, off))
    x = torch.randn(n, generator=_gen(n, off, 31))
    xd, xb = _buf((n,), x, off)
    for start in (0.0, 3.5):
        out = torch.full((1,), start, device=DEV)
        _call("lstc_sqnorm_accum", P(xd), n, P(out))
        torch.cuda.synchronize()
        ck.close("sqnorm_accum from %g" % start, out, (R.sqnorm([x]) + start).reshape(1), (R.sqnorm([x], F32) + start).reshape(1),
                 R.sqnorm([x]) + start)
    _call("lstc_scale", P(xd), n, 0.37)
    torch.cuda.synchronize()
    ck.close("scale", xd, x.to(F64) * 0.37, x * 0.37, x.to(F64).abs() * 0.37)
    ck.true("guards", _guards_ok(xb, off))
    ck.done()


def test_sqnorm_multi_and_clip_scale_multi_50_tensors():
    """lstc_sqnorm_multi (sum of squares and its root over the 50-tensor list, two launches + the partial sum) and
    lstc_clip_scale_multi with a ``max_norm`` that clips and one that does not: the tensors must then be untouched bit for bit."""
    L = _L()
    P = L.dev_ptr
    ck = Checks("norm_clip", "sqnorm_multi/clip_scale_multi 50 tensors")
    items = _multi_list()
    arr = (L.VecItem * len(items))()
    for a, it in zip(arr, items):
        it["x"] = it["g"][0]
        it["xd"], it["xb"] = _buf((it["n"],), it["x"], it["off"])
        a.x, a.n = P(it["xd"]), it["n"]
    lib = L.load()
    need = int(lib.lstc_sqnorm_multi_scratch(arr, len(items)))
    ck.true("scratch = one float per 8192-element slice", need == sum((it["n"] + 8191) // 8192 for it in items))
    scratch = torch.full((need,), float("nan"), device=DEV)
    out = torch.full((2,), float("nan"), device=DEV)
    _call("lstc_sqnorm_multi", arr, len(items), P(scratch), need, P(out))
    torch.cuda.synchronize()
    xs = [it["x"] for it in items]
    sq, sq32 = R.sqnorm(xs), R.sqnorm(xs, F32)
    ck.close("sum of squares", out[:1], sq.reshape(1), sq32.reshape(1), sq)
    ck.close("norm", out[1:], sq.sqrt().reshape(1), sq32.sqrt().reshape(1), sq.sqrt())
    norm = float(sq.sqrt())
    _call("lstc_clip_scale_multi", arr, len(items), P(out), 2.0 * norm)
    torch.cuda.synchronize()
    ck.true("coefficient >= 1: untouched bit for bit", all(torch.equal(it["xd"].cpu(), it["x"]) for it in items))
    max_norm = 0.5 * norm
    _call("lstc_clip_scale_multi", arr, len(items), P(out), max_norm)
    torch.cuda.synchronize()
    coef = R.clip_coef(sq, max_norm)
    coef32 = torch.tensor(max_norm, dtype=F32) / (sq32.sqrt() + torch.tensor(1e-6, dtype=F32))
    ck.true("coefficient clips", coef < 1.0)
    for i, it in enumerate(items):
        ck.close("clipped tensor %d (n=%d)" % (i, it["n"]), it["xd"], it["x"].to(F64) * coef, it["x"] * coef32, it["x"].to(F64).abs())
        ck.true("guards %d" % i, _guards_ok(it["xb"], it["off"]))
    ck.done()
