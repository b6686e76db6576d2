"""The GEMM kernels (csrc/gemm_f32.hip, gemm_bf16c.hip, gemm_pk.hip, gemm_bf16p.hip), lstc_splitk_finish and the operand packs
against the float64 references of tests/util_gemm.py, dispatch branch by dispatch branch, through the C ABI (lstc_gemm on a
_lib.GemmDesc - functional.gemm's routing thresholds would hide branches).  Every parametrised case is named after the kernel
instantiation it reaches, and restates that branch's dispatch condition before the launch.

Every operand lives inside a larger buffer: A and B between NaNs, with NaN pad columns where the leading dimension is wider than
the row; C, residual and relu_src between guard values, with guard pad columns.  After the launch everything around C must be
bit-identical and the operands unchanged; packs are allocated at lstc_pack*_bytes and 0xFF-filled (NaN) before packing.

One tolerance rule (util_gemm.tolerance = util_rowops.tol): per output tensor 8 * max(e32, 4 * 2**-24 * B); for the bf16 dtypes
reference, e32 and B are computed on the bf16-rounded operands (no bf16 allowance: the kernels accumulate in f32); LSTC_F32X3 adds
the f16-plane format's own error e_fmt; a packed bf16 output adds 2**-8 |ref| per element.  The ``int`` family must come out EQUAL
to the float64 reference for every dtype, form and summation order.  Every check prints err / tol; the worst ratio per family is
printed when the module finishes."""
import ctypes as C

import numpy as np
import pytest
import torch

import util_gemm as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = -777.25
NAN = float("nan")
WORST = {}
SEED = 20250


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for fam in sorted(WORST):
        print("gemm-f64 worst err/tol  %-14s %.3f  (%s)" % ((fam,) + WORST[fam]))


def _L():
    from lstc_vad_amd import _lib
    return _lib


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Checks:
    """Collects the comparisons of one test; ``done`` asserts them together so a failure shows every output's figures."""

    def __init__(self, family, case):
        self.family, self.case, self.bad = family, case, []

    def close(self, what, got, ref64, t):
        """``t``: the tolerance, one number or a tensor shaped like the output."""
        got = got.detach().cpu().to(F64)
        assert got.shape == ref64.shape, (self.case, what, got.shape, ref64.shape)
        if torch.isfinite(got).all():
            d = (got - ref64).abs()
            err = float(d.max())
            ratio = float((d / t).max()) if torch.is_tensor(t) else (err / t if t > 0 else (0.0 if err == 0 else float("inf")))
        else:
            err = ratio = float("inf")
        tmax = float(t.max()) if torch.is_tensor(t) else t
        print("%s %s %s: err %.3e tol %.3e ratio %.3f" % (self.family, self.case, what, err, tmax, ratio))
        if ratio >= WORST.get(self.family, (-1.0, ""))[0]:
            WORST[self.family] = (ratio, "%s %s" % (self.case, what))
        if not ratio <= 1.0:
            self.bad.append((what, err, tmax))

    def equal(self, what, got, ref):
        """torch.equal (so -0 == +0) of two tensors of one dtype; reports how many elements differ."""
        got, ref = got.detach().cpu(), ref.detach().cpu()
        ok = got.shape == ref.shape and torch.equal(got, ref)
        n = -1 if got.shape != ref.shape else int((got != ref).sum())
        print("%s %s %s: equal %s (%d differ)" % (self.family, self.case, what, ok, n))
        if not ok:
            self.bad.append((what, "not equal", n))

    def true(self, what, cond):
        if not cond:
            self.bad.append((what, "false"))

    def done(self):
        assert not self.bad, (self.family, self.case, self.bad)


# ============================================================================================ buffers
def _ld(cols, odd):
    """A leading dimension wider than the row: a multiple of 4 (float4 rows stay possible), or with ``odd`` no multiple of 4."""
    if odd:
        return cols + (3 if (cols + 3) % 4 else 1)
    return cols + 4 + (-cols) % 4


def _bits(t):
    return t.contiguous().view(torch.int32)


class Placed:
    """``srcs``: a list (the problems of a batch) of [rows, cols] CPU tensors, placed ``off`` floats into ONE buffer, rows ``ld``
    apart, problems ``stride`` apart (not the dense stride), ``pad`` in the pad columns, ``guard`` in front, between and behind.
    off = 4: 16-byte aligned; off = 5: one float off."""

    def __init__(self, srcs, ld, off, pad, guard, gap=12):
        rows, cols = srcs[0].shape
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.stride = rows * ld + (gap if len(srcs) > 1 else 0)
        host = torch.full((off + self.stride * len(srcs) + 8,), guard, dtype=F32)
        inside = torch.zeros(host.numel(), dtype=torch.bool)
        for z, s in enumerate(srcs):
            v = host[off + z * self.stride: off + z * self.stride + rows * ld].view(rows, ld)
            v[:] = pad
            v[:, :cols] = s.to(F32)
            inside[off + z * self.stride: off + z * self.stride + rows * ld].view(rows, ld)[:, :cols] = True
        self.host, self.inside = host, inside
        self.dev = host.to(DEV)
        assert (self.ptr(0) % 16 == 0) == (off % 4 == 0)

    def view(self, z=0):
        o = self.off + z * self.stride
        return self.dev[o: o + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def ptr(self, z=0):
        return self.dev.data_ptr() + 4 * (self.off + z * self.stride)

    def unchanged(self):
        return torch.equal(_bits(self.dev.cpu()), _bits(self.host))

    def outside_unchanged(self):
        """Everything but the matrices themselves - guards, pad columns, the gaps of a batch - is bit-identical to before."""
        out = ~self.inside
        return torch.equal(_bits(self.dev.cpu())[out], _bits(self.host)[out])


def _pack(kind, view_ptr, rows, K, ld, k_major):
    """lstc_pack1 / lstc_pack3 of a device matrix into a 0xFF-filled (NaN) buffer of exactly lstc_pack*_bytes, 64 guard bytes behind."""
    L = _L()
    lib = L.load()
    nbytes = int((lib.lstc_pack1_bytes if kind == 1 else lib.lstc_pack3_bytes)(rows, K))
    buf = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[nbytes:] = 0xA5
    L.check((lib.lstc_pack1 if kind == 1 else lib.lstc_pack3)(view_ptr, rows, K, ld, k_major, buf.data_ptr(), L.stream_ptr()), "lstc_pack%d" % kind)
    return buf, nbytes


def _unpack1(pack, rows, K):
    L = _L()
    out = torch.full((rows, K), NAN, device=DEV, dtype=F32)
    L.check(L.load().lstc_unpack1_rows(pack.data_ptr(), rows, K, 0, 1, rows, out.data_ptr(), K, L.stream_ptr()), "lstc_unpack1_rows")
    return out


def _keep_mask(M, N, p, seed):
    L = _L()
    m = torch.empty(M * N, dtype=torch.uint8, device=DEV)
    L.check(L.load().lstc_dropout_mask(m.data_ptr(), M * N, p, seed, L.stream_ptr()), "lstc_dropout_mask")
    return m.cpu().view(M, N).bool()


# ============================================================================================ one launch
def _stored(layout, A, B):
    """(A as stored, B as stored, transA, transB) of logical A [M, K], B [K, N]."""
    if layout == "NT":
        return A, B.t().contiguous(), 0, 1
    if layout == "NN":
        return A, B, 0, 0
    return A.t().contiguous(), B, 1, 0                 # TN, and TR (the packed weight-gradient form on packs of the sources)


def _aligned16(p):
    return p % 16 == 0


def _assert_branch(case, d, pa, pb, n_cu):
    """Restates the dispatch condition of the branch the case's id names (csrc/*.hip, the *_impl functions) and asserts it BEFORE the
    launch: on a chip with another CU count, or after a change of the routing, the case fails loudly instead of testing another
    branch."""
    kind = case["id"].split("-")[0]
    dt, M, N, K = case["dtype"], d.M, d.N, d.K
    fl = d.flags
    naux = bool(fl & G.RESIDUAL) + bool(fl & G.RELU_MASK) + bool(fl & G.ACCUM)
    batch = max(d.batch, 1)
    if dt in (G.LSTC_F32, G.LSTC_BF16):
        va = _aligned16(pa) and d.lda % 4 == 0 and (M if d.transA else K) % 4 == 0 and (batch == 1 or d.batch_stride_a % 4 == 0)
        vb = _aligned16(pb) and d.ldb % 4 == 0 and (K if d.transB else N) % 4 == 0 and (batch == 1 or d.batch_stride_b % 4 == 0)
    if dt == G.LSTC_F32:
        splits = G.gemm_splits(dt, K, d.split_k)
        al = N % 4 == 0 and N >= 4 and d.ldc % 4 == 0 and _aligned16(d.C) and (not fl & G.RESIDUAL or d.ldr % 4 == 0) and \
            (not fl & G.RELU_MASK or d.ld_relu % 4 == 0)
        epi_f4 = (2 if naux else 1) if (al and naux <= 1 and (batch == 1 or d.batch_stride_c % 4 == 0) and splits == 1) else 0
        if d.variant == 0 and splits == 1 and batch == 1 and not d.transA and not kind.startswith("rowsplit"):
            assert ((M + 127) // 128) * ((N + 127) // 128) < 2 * n_cu, "the default would split the rows of this product"
        if kind.startswith("pipe5") or kind.startswith("epi_aligned"):
            assert va and vb and d.variant in (0, 4), (va, vb)
        if kind.startswith("pipe3"):
            if d.variant == 8:
                assert va and vb                                   # PIPE 3 by request, on operands PIPE 5 would take
            else:
                assert va == (not case["a_off"]) and vb == (not case["b_odd"]) and not (va and vb), (va, vb)
        if kind.startswith("epi_aligned"):                         # float4 epilogue; more than one per-element operand: the scalar form
            assert epi_f4 == (0 if naux > 1 else 2 if naux else 1), (epi_f4, naux)
        if kind.startswith("epi_scalar"):
            assert epi_f4 == 0
        if kind.startswith("persist_v12_epi"):
            assert va and vb and K % 32 == 0 and K // 32 >= 4 and epi_f4 == int(kind[len("persist_v12_epi")]) and \
                (min(2 * n_cu, ((M + 127) // 128) * ((N + 127) // 128)) & ~7) >= 8
        if kind.startswith("persist_v12_fallback"):
            assert va and vb and (K % 32 != 0 or K // 32 < 4)
        if kind.startswith("splitk"):
            assert splits > 1 and fl == 0
            if "3slices" in kind:
                assert d.split_k == 4 and splits == 3
    elif dt == G.LSTC_BF16:
        if "picks_128x128" in kind:
            assert d.variant == 0 and case["layout"] == "NT" and K >= 4096
        if "picks_256x128" in kind:
            assert d.variant == 0 and K < 4096
        if "scalar_loads" in kind or "a_off" in kind or "b_odd" in kind:       # which of the four <VA, VB> instantiations
            assert va == (not case["a_off"]) and vb == (not case["b_odd"]), (va, vb)
    elif dt == G.LSTC_F32X3:
        tr = case["layout"] == "TR"
        wide = (d.variant == 2 and (not tr or M % 256 == 0)) or (d.variant == 0 and tr and M % 256 == 0 and K >= 8192)
        assert kind.startswith("pkw") == wide and ("_tr" in kind) == tr, (wide, tr)
        if "epi_f4" in kind:
            assert N % 4 == 0 and d.ldc % 4 == 0
    else:
        tr = case["layout"] == "TR"
        vec = N % 4 == 0 and (bool(fl & G.OUT_PACK) or d.ldc % 4 == 0) and (not fl & G.RESIDUAL or bool(fl & G.RESIDUAL_PACK) or d.ldr % 4 == 0) \
            and (not fl & G.RELU_MASK or bool(fl & G.RELU_MASK_PACK) or d.ld_relu % 4 == 0)
        items = ((M + 255) // 256) * ((N + 255) // 256)
        tail = items % n_cu
        epk3 = bool(fl & G.RELU_MASK_PACK) and not fl & G.OUT_PACK
        qtail = (not tr and G.gemm_splits(dt, K, d.split_k) == 1 and vec and not epk3 and not d.variant & G.NO_QTAIL
                 and tail > 0 and 4 * tail <= 2 * n_cu)                       # 2 = P1_QTAIL_ROUNDS
        if "qtail" in case:
            assert case["qtail"] == qtail, (qtail, vec, tail)
        if "scalar_epilogue" in kind:
            assert not vec


def _launch(case, family, ck, seed=SEED, keep_products=False):
    """Places the operands, restates the branch, launches once, checks the memory around the operands and the output, and returns
    (got per batch problem as CPU float32 [M, N], keep mask or None, reference pieces per problem)."""
    L = _L()
    lib = L.load()
    dt, M, N, K, layout = case["dtype"], case["M"], case["N"], case["K"], case["layout"]
    fl = case["flags"]
    batch = max(case["batch"], 1)
    packed = dt in (G.LSTC_F32X3, G.LSTC_BF16P)
    partials = bool(case.get("partials"))
    probs = [G.products(case, family, z) for z in range(batch)]
    As, Bs, tA, tB = zip(*[_stored(layout, P["A_raw"], P["B_raw"]) for P in probs])
    tA, tB = tA[0], tB[0]
    pa = Placed(list(As), _ld(As[0].shape[1], False), 5 if case["a_off"] else 4, NAN, NAN)
    pb = Placed(list(Bs), _ld(Bs[0].shape[1], case["b_odd"]), 4, NAN, NAN)
    odd = bool(case["c_odd"])
    c_off = 5 if case.get("c_off") else 4                      # c_off: C, residual and relu_src one float off 16-byte alignment
    n_slots = case["split"] if partials else 1
    if partials:
        ldc = N                                                # split z writes C + z * M * N: dense partial slabs
        c_src = [torch.full((M, N), GUARD) for _ in range(n_slots)]
        pc = Placed(c_src, ldc, 4, GUARD, GUARD, gap=0)
    else:
        ldc = _ld(N, odd)
        if fl & G.ACCUM:
            c_src = [P["old"] for P in probs]
        elif case["split"] > 1:
            c_src = [torch.zeros(M, N) for _ in probs]         # split-K with atomics: the caller zeroes C
        else:
            c_src = [torch.full((M, N), GUARD) for _ in probs]
        pc = Placed(c_src, ldc, c_off, GUARD, GUARD)
    P0 = probs[0]
    pr = Placed([P0["res"]], _ld(N, odd) + (0 if odd else 4), c_off, GUARD, GUARD)
    ps = Placed([P0["src"]], _ld(N, odd) + (0 if odd else 8), c_off, GUARD, GUARD)
    bias = torch.cat([torch.full((4,), GUARD), P0["bias"], torch.full((4,), GUARD)]).to(DEV)

    d = L.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldr, d.ld_relu = pa.ld, pb.ld, pc.ld, pr.ld, ps.ld
    d.transA, d.transB, d.dtype, d.flags = tA, tB, dt, fl
    d.alpha, d.dropout_p, d.dropout_seed = case["alpha"], G.drop_p(family), seed
    d.split_k, d.variant, d.batch = case["split"], case["variant"], case["batch"]
    d.batch_stride_a, d.batch_stride_b = pa.stride, pb.stride
    d.batch_stride_c = M * N if partials else (pc.stride if batch > 1 else 0)
    d.A, d.B, d.C = pa.ptr(), pb.ptr(), pc.ptr()
    d.bias = bias.data_ptr() + 16 if fl & G.BIAS else None
    d.residual = pr.ptr() if fl & G.RESIDUAL else None
    d.relu_src = ps.ptr() if fl & G.RELU_MASK else None
    packs = []
    res_vals, src_vals = P0["res"], P0["src"]
    out_pack = None
    if packed:
        kind = 1 if dt == G.LSTC_BF16P else 3
        if layout == "TR":                                      # packs of the k-major SOURCES [K, M], [K, N]
            bufa, na = _pack(kind, pa.ptr(), K, M, pa.ld, 0)
            bufb, nb = _pack(kind, pb.ptr(), K, N, pb.ld, 0)
            d.transA, d.transB = 1, 0
        else:                                                   # packs of [M, K] and [N, K], lstc_pack* transposing k-major sources
            bufa, na = _pack(kind, pa.ptr(), M, K, pa.ld, 1 if tA else 0)
            bufb, nb = _pack(kind, pb.ptr(), N, K, pb.ld, 0 if tB else 1)
            d.transA, d.transB = 0, 1
        packs = [(bufa, na), (bufb, nb)]
        d.A, d.B = bufa.data_ptr(), bufb.data_ptr()
        if fl & G.RESIDUAL_PACK:
            bufr, nr = _pack(1, pr.ptr(), M, N, pr.ld, 0)
            packs.append((bufr, nr))
            d.residual = bufr.data_ptr()
            res_vals = _unpack1(bufr, M, N).cpu()               # the residual pack's own values
        if fl & G.RELU_MASK_PACK:
            bufs, ns = _pack(1, ps.ptr(), M, N, ps.ld, 0)
            packs.append((bufs, ns))
            d.relu_src = bufs.data_ptr()
            src_vals = _unpack1(bufs, M, N).cpu()
        if fl & G.OUT_PACK:
            nout = int(lib.lstc_pack1_bytes(M, N))
            out_pack = torch.full((nout + 64,), 0xFF, dtype=torch.uint8, device=DEV)
            out_pack[nout:] = 0xA5
            d.C = out_pack.data_ptr()
    pack_snap = [b.clone() for b, _ in packs]
    torch.cuda.synchronize()
    _assert_branch(case, d, pa.ptr(), pb.ptr(), _cus())
    L.check(lib.lstc_gemm(C.byref(d), L.stream_ptr()), "lstc_gemm " + case["id"])
    torch.cuda.synchronize()

    ck.true(family + " A and the NaNs around it unchanged", pa.unchanged())
    ck.true(family + " B and the NaNs around it unchanged", pb.unchanged())
    ck.true(family + " residual / relu_src unchanged", pr.unchanged() and ps.unchanged())
    ck.true(family + " packs unchanged", all(torch.equal(b, s) for (b, _), s in zip(packs, pack_snap)))
    ck.true(family + " guards and pad columns of C bit-identical", pc.outside_unchanged())
    if out_pack is not None:
        ck.true(family + " bytes behind the output pack unchanged", bool((out_pack[-64:] == 0xA5).all()))
        ck.true(family + " C buffer untouched by a packed output", pc.unchanged())
        got = [_unpack1(out_pack, M, N).cpu()]
    elif partials:
        n_used = int(lib.lstc_gemm_splits(dt, K, case["split"]))
        ck.true(family + " lstc_gemm_splits = header formula", n_used == G.gemm_splits(dt, K, case["split"]) and n_used < n_slots)
        slabs = [pc.view(z).cpu() for z in range(n_slots)]
        ck.true(family + " the slots behind the last slice keep their guard", all(bool((s == GUARD).all()) for s in slabs[n_used:]))
        ck.true(family + " partials finite", all(bool(torch.isfinite(s).all()) for s in slabs[:n_used]))
        got = [torch.stack(slabs[:n_used]).to(F64).sum(0)]      # the caller sums exactly lstc_gemm_splits partials
    else:
        got = [pc.view(z).cpu() for z in range(batch)]
    keep = _keep_mask(M, N, G.drop_p(family), seed) if fl & G.DROPOUT else None
    return got, keep, dict(residual=res_vals, relu_src=src_vals)


def _check_case(case, family, ck, got, keep, over):
    """close against ref64 (equal for ``int``), and the structure of the epilogue."""
    fl = case["flags"]
    for z, g in enumerate(got):
        P = G.products(case, family, z)
        ref, f32, terms, fmt = G.case_reference(case, family, keep, z, **over)
        tag = family if len(got) == 1 else "%s z=%d" % (family, z)
        if family == "int":
            assert case["K"] <= 4096
            if fl & G.OUT_PACK:                                 # the stored value is the exact integer result rounded once to bf16
                ck.equal(tag + " C == bf16(float64 reference)", g.to(F32), G.bf16_round(ref.to(F32)))
            else:
                ck.equal(tag + " C == float64 reference", g.to(F64), ref)
        else:
            ck.close(tag + " C", g, ref, G.tolerance(ref, f32, terms, fmt, packed_out=bool(fl & G.OUT_PACK)))
        if fl & G.OUT_PACK or not fl & (G.DROPOUT | G.RELU_MASK):
            continue
        # structure: what a dropped or masked element must hold EXACTLY - the stages behind the dropout applied to 0 in float32
        g32 = g.to(F32)
        rest = fl & (G.RESIDUAL | G.RELU_MASK | G.ACCUM)
        zero_path = G.epilogue(torch.zeros(g.shape, dtype=F32), flags=rest, residual=over["residual"], relu_src=over["relu_src"], c_old=P["old"])
        if fl & G.DROPOUT:
            ck.true(tag + " a dropped element holds residual (+ old C) exactly, 0 without", torch.equal(g32[~keep], zero_path[~keep]))
            far = (ref.to(F32) - zero_path).abs() > 1e-3         # kept elements whose value is visibly not the dropped one
            ck.true(tag + " kept elements are not the dropped value", bool((g32[keep & far] != zero_path[keep & far]).all()) and int((keep & far).sum()) > 0)
        if fl & G.RELU_MASK:
            masked = ~(over["relu_src"] > 0)
            base = P["old"].to(F32) if fl & G.ACCUM else torch.zeros(g.shape, dtype=F32)
            ck.true(tag + " ReLU-mask zeros sit exactly where relu_src <= 0", torch.equal(g32[masked], base[masked]) and int(masked.sum()) > 0)


_CHAINS = {}


def _chain_rows(M):
    """All rows of a small product; of a larger one the first and last 16 and the rows around every 128-row tile boundary."""
    if M <= 80:
        return np.arange(M)
    r = set(range(16)) | set(range(M - 16, M))
    for b in range(128, M, 128):
        r |= set(range(b - 4, min(b + 4, M)))
    return np.array(sorted(r))


def _chain(case, family, rows=None, z=0):
    M, N, K = case["M"], case["N"], case["K"]
    rows = _chain_rows(M) if rows is None else rows
    key = (M, N, K, family, z, rows.tobytes())
    if key not in _CHAINS:
        P = G.products(case, family, z)
        if len(_CHAINS) >= 32:
            _CHAINS.pop(next(iter(_CHAINS)))
        _CHAINS[key] = torch.from_numpy(G.fmaf_chain(P["A"].numpy(), P["B"].numpy(), rows, None, G.mfma_issue_order(K)))
    return rows, _CHAINS[key]


def _run(case):
    ck = Checks(G.DTYPE_NAMES[case["dtype"]], case["id"])
    for family in G.case_families(case):
        got, keep, over = _launch(case, family, ck)
        _check_case(case, family, ck, got, keep, over)
        if case["dtype"] == G.LSTC_F32 and case["flags"] == 0 and case["alpha"] == 1.0 and case["split"] <= 1 and family in ("randn", "range"):
            for z, g in enumerate(got):
                rows, chain = _chain(case, family, z=z)
                ck.equal("%s z=%d C == fmaf chain bit for bit (%d rows)" % (family, z, len(rows)), g[torch.from_numpy(rows)], chain)
    ck.done()


# ============================================================================================ the case tables
def _ids(dtype):
    return [c["id"] for c in G.CASES[dtype]]


# worst err / tol measured on an MI355X: 0.119 (pipe3_v8_aligned-TN-300x200x100, range); the chain: equal in all 184 comparisons
@pytest.mark.parametrize("case", G.CASES[G.LSTC_F32], ids=_ids(G.LSTC_F32))
def test_gemm_f32(case):
    _run(case)


# worst err / tol measured on an MI355X: 0.053 (bf16c_v0_picks_256x128_K4032-NT-130x130x4032, randn)
@pytest.mark.parametrize("case", G.CASES[G.LSTC_BF16], ids=_ids(G.LSTC_BF16))
def test_gemm_bf16c(case):
    _run(case)


# worst err / tol measured on an MI355X: 0.131 (pk2s_nt_epi_scalar_all-257x131x67, spike)
@pytest.mark.parametrize("case", G.CASES[G.LSTC_F32X3], ids=_ids(G.LSTC_F32X3))
def test_gemm_f32x3(case):
    _run(case)


# worst err / tol measured on an MI355X: 0.050 with an f32 output; 0.993 (bf16p_out_pack-1024x768x320, randn) with a packed one, where
# the 2**-8 |ref| allowance is exactly half a bf16 ulp just above a power of two
@pytest.mark.parametrize("case", G.CASES[G.LSTC_BF16P], ids=_ids(G.LSTC_BF16P))
def test_gemm_bf16p(case):
    _run(case)


# ============================================================================================ shapes computed from the CU count
def test_gemm_f32_persistent_walk_over_more_tiles_than_slots():
    """variant 12 on slots + 8 tiles of 128 x 128 (slots = 2 * CUs): eight workgroups walk a second tile.  float64 on everything;
    the chain bit for bit on the first and last 256 rows and across the boundary between the first and the second round."""
    slots = 2 * _cus()
    M = 128 * (slots + 8)
    case = G.cu_cases(_cus())["persist"]
    assert case["M"] == M
    ck = Checks("f32", case["id"])
    for family in case["families"]:
        got, keep, over = _launch(case, family, ck)
        _check_case(case, family, ck, got, keep, over)
        if family == "randn":
            rows = np.concatenate([np.arange(256), np.arange(128 * slots - 8, 128 * slots + 8), np.arange(M - 256, M)])
            rows, chain = _chain(case, family, rows)
            ck.equal("randn C == fmaf chain bit for bit (first / last 256 rows, round boundary)", got[0][torch.from_numpy(rows)], chain)
    ck.done()


def test_gemm_f32_default_row_split_tail_offsets_and_dropout_index():
    """variant 0 on slots + 8 tiles of 128 x 128 at K = 36: full = 1, rem = 8 <= 30 % of the slots - the last 1024 rows run on the
    64 x 64 tile with row_off = 128 * slots.  With bias + dropout + residual and ldc, ldr = N + 4 / N + 8: the tail's row offset into
    C and the residual and the dropout counter (row + row_off) * N + col are what is under test; the plain form is checked bit for
    bit against the chain on the 256 rows around the split."""
    slots = 2 * _cus()
    M, N, K = 128 * (slots + 8), 128, 36
    tiles = (M // 128) * 1
    full, rem = tiles // slots, tiles % slots
    assert full == 1 and rem == 8 and rem * 10 <= slots * 3, (full, rem, slots)
    epi, plain = G.cu_cases(_cus())["rowsplit_epi"], G.cu_cases(_cus())["rowsplit_plain"]
    assert (epi["M"], epi["N"], epi["K"]) == (M, N, K) == (plain["M"], plain["N"], plain["K"])
    for case in (epi, plain):
        ck = Checks("f32", case["id"])
        for family in case["families"]:
            got, keep, over = _launch(case, family, ck)
            _check_case(case, family, ck, got, keep, over)
            if case is plain and family == "randn":
                rows = np.arange(128 * slots - 128, 128 * slots + 128)
                rows, chain = _chain(case, family, rows)
                ck.equal("randn C == fmaf chain bit for bit (256 rows around the split)", got[0][torch.from_numpy(rows)], chain)
        ck.done()


@pytest.mark.parametrize("variant,name", [(0, "persistent_then_qtail"), (G.NO_QTAIL, "persistent_second_trip")])
def test_gemm_bf16p_more_tiles_than_cus(variant, name):
    """CUs + 16 tiles of 256 x 256 at K = 64.  variant 0: one whole round on the persistent kernel, the 16 tiles behind it as 64
    quarter items (4 * 16 <= 2 * CUs); NO_QTAIL: 16 workgroups of the persistent kernel take a second tile."""
    n_cu = _cus()
    tiles = n_cu + 16
    assert 4 * 16 <= 2 * n_cu
    case = G.cu_cases(n_cu)["bf16p_qtail" if variant == 0 else "bf16p_second_trip"]
    assert case["M"] == 256 * tiles and case["variant"] == variant and case["qtail"] == (variant == 0)
    ck = Checks("bf16p", case["id"])
    for family in case["families"]:
        got, keep, over = _launch(case, family, ck)
        _check_case(case, family, ck, got, keep, over)
    ck.done()


# ============================================================================================ scalar against float4 epilogue
# (dtype, M, N, K, layout, variant, id prefix): the smallest shapes that reach each pair of epilogues.  LSTC_BF16 has one epilogue only.
AGREE = [(G.LSTC_F32, 257, 132, 68, "NT", 0, "agree_f32_pipe5"),                    # epilogue_f4 against epilogue_scalar of PIPE 5
         (G.LSTC_F32X3, 300, 520, 100, "NT", 0, "agree_pk2s"),                      # gemm_pk 128 x 128 kernel
         (G.LSTC_F32X3, 512, 200, 96, "NN", 2, "pkw_agree"),                        # 256 x 128 kernel (_assert_branch keys it on the "pkw" prefix: keep it)
         (G.LSTC_BF16P, 300, 200, 100, "NT", G.NO_QTAIL, "agree_bf16p_wide"),       # wide epilogue on part-filled tiles
         (G.LSTC_BF16P, 512, 512, 64, "NT", G.NO_QTAIL, "agree_bf16p_fastepi")]     # pipelined epilogue on whole 256 x 256 tiles
AGREE_SETS = [(n, f, a) for (n, f), a in zip(G.EPI_SETS, G.ALPHAS) if bool(f & G.RESIDUAL) + bool(f & G.RELU_MASK) + bool(f & G.ACCUM) <= 1]


@pytest.mark.parametrize("dtype,M,N,K,layout,variant,tag", AGREE, ids=[a[-1] for a in AGREE])
def test_scalar_and_float4_epilogues_agree_bitwise(dtype, M, N, K, layout, variant, tag):
    """The same product and flags twice through lstc_gemm: everything 16-byte aligned (float4 / wide / pipelined epilogue), then with
    C, residual and relu_src one float off at the same leading dimensions (the one-column-per-lane epilogue).  Both launches run the
    same K loop and both epilogues are the one chain of csrc/lstc_common.h in float32 without contraction: C must be bit-identical,
    the guards around it untouched.  Every EPI_SETS row with at most one per-element operand, with its alpha, dropout at DROP_P."""
    assert len(AGREE_SETS) == 8
    ck = Checks(G.DTYPE_NAMES[dtype], tag)
    for name, fl, alpha in AGREE_SETS:
        got = []
        for c_off in (0, 1):
            case = G.make_case("%s_%s-%s-%dx%dx%d" % (tag, name, layout, M, N, K), dtype, M, N, K, layout, variant, fl, alpha, c_off=c_off)
            if dtype == G.LSTC_BF16P:
                case["qtail"] = False
            g, _, _ = _launch(case, "randn", ck)                  # (asserts the guards and pad columns of C itself)
            got.append(g[0])
        ck.equal("%s C (aligned) == C (one float off)" % name, got[0], got[1])
    ck.done()


# ============================================================================================ lstc_splitk_finish
SKF_FLAGS = [("plain", 0)] + G.EPI_SETS


# worst err / tol measured on an MI355X: 0.090 (all flags, splits = 7, randn)
@pytest.mark.parametrize("splits", [1, 2, 7])
@pytest.mark.parametrize("name,flags", SKF_FLAGS, ids=[n for n, _ in SKF_FLAGS])
def test_splitk_finish(name, flags, splits):
    """Random parts (not real partial products) summed in chunk order and pushed through the epilogue, ldc / ldr / ld_relu wider than
    N: against the float64 sum, and - the header promises the order - bit for bit against the float32 sum in chunk order with the
    float32 epilogue for the plain sum."""
    L = _L()
    M, N = 37, 68
    ck = Checks("splitk_finish", "%s splits=%d" % (name, splits))
    for family in ("randn", "int"):
        g = G.gen(M, N, splits, flags, family == "int")
        draw = (lambda *s: torch.randint(-4, 5, s, generator=g).to(F32)) if family == "int" else (lambda *s: torch.randn(*s, generator=g))
        parts = draw(splits, M, N)
        if family == "randn":
            parts[0] *= 1e3                                       # the first chunk dominates: a last-to-first sum rounds differently
        bias_v, res_v, src_v, old_v = G.aux_operands(family, M, N, splits)
        pp = Placed([p.reshape(1, M * N) for p in parts], M * N, 4, NAN, NAN, gap=8)
        part_stride = max(pp.stride, M * N)                       # M * N + 8 between the chunks: not the dense stride
        pc = Placed([old_v if flags & G.ACCUM else torch.full((M, N), GUARD)], N + 4, 4, GUARD, GUARD)
        pr = Placed([res_v], N + 8, 4, GUARD, GUARD)
        ps = Placed([src_v], N + 12, 4, GUARD, GUARD)
        bias = bias_v.to(DEV)
        p, seed = G.drop_p(family), SEED + splits
        L.check(L.load().lstc_splitk_finish(pp.ptr(), splits, part_stride, M, N, bias.data_ptr() if flags & G.BIAS else None,
                                            pr.ptr() if flags & G.RESIDUAL else None, pr.ld, ps.ptr() if flags & G.RELU_MASK else None, ps.ld,
                                            pc.ptr(), pc.ld, flags, p, seed, 1, 0, 0, L.stream_ptr()), "lstc_splitk_finish")
        torch.cuda.synchronize()
        ck.true(family + " parts / operands unchanged, C's guards and pads bit-identical",
                pp.unchanged() and pr.unchanged() and ps.unchanged() and pc.outside_unchanged())
        keep = _keep_mask(M, N, p, seed) if flags & G.DROPOUT else None
        kw = dict(flags=flags, alpha=1.0, bias=bias_v, keep=keep, p=p, residual=res_v, relu_src=src_v, c_old=old_v)
        acc64 = parts.to(F64).sum(0)
        acc32 = torch.zeros(M, N)
        for i in range(splits):
            acc32 = acc32 + parts[i]                              # float32, chunk order
        ref = G.epilogue(acc64, **kw)
        terms = G.terms_abs(None, None, absprod=parts.to(F64).abs().sum(0), **kw)
        got = pc.view().cpu()
        if family == "int":
            ck.equal("int C == float64 reference", got.to(F64), ref)
        else:
            ck.close("randn C", got, ref, G.tolerance(ref, G.epilogue(acc32, **kw), terms))
        if flags & ~G.ACCUM == 0 or family == "int":
            ck.equal(family + " C == float32 sum in chunk order, bit for bit", got, G.epilogue(acc32, **kw))
    ck.done()


@pytest.mark.parametrize("accum", [0, 1], ids=["plain", "accum"])
def test_splitk_finish_groups(accum):
    """groups = 4 with strides of their own (parts and C), plain and with ACCUM."""
    L = _L()
    M, N, splits, groups = 9, 36, 3, 4
    ck = Checks("splitk_finish", "groups4 accum=%d" % accum)
    g = G.gen(M, N, splits, groups, accum)
    parts = torch.randn(groups, splits, M, N, generator=g)
    parts[:, 0] *= 1e3
    old = torch.randn(groups, M, N, generator=g)
    part_stride = M * N + 4
    gsp = splits * part_stride + 16
    host = torch.full((4 + groups * gsp + 8,), NAN)
    for q in range(groups):
        for i in range(splits):
            o = 4 + q * gsp + i * part_stride
            host[o:o + M * N] = parts[q, i].reshape(-1)
    pdev = host.to(DEV)
    pc = Placed([old[q] if accum else torch.full((M, N), GUARD) for q in range(groups)], N + 4, 4, GUARD, GUARD, gap=20)
    L.check(L.load().lstc_splitk_finish(pdev.data_ptr() + 16, splits, part_stride, M, N, None, None, 0, None, 0, pc.ptr(), pc.ld,
                                        G.ACCUM if accum else 0, 0.0, 0, groups, gsp, pc.stride, L.stream_ptr()), "lstc_splitk_finish")
    torch.cuda.synchronize()
    ck.true("guards, pads and gaps of C bit-identical, parts unchanged", pc.outside_unchanged() and torch.equal(_bits(pdev.cpu()), _bits(host)))
    for q in range(groups):
        acc32 = torch.zeros(M, N)
        for i in range(splits):
            acc32 = acc32 + parts[q, i]
        kw = dict(flags=G.ACCUM if accum else 0, c_old=old[q])
        ref = G.epilogue(parts[q].to(F64).sum(0), **kw)
        got = pc.view(q).cpu()
        ck.close("group %d C" % q, got, ref, G.tolerance(ref, G.epilogue(acc32, **kw), G.terms_abs(None, None, absprod=parts[q].to(F64).abs().sum(0), **kw)))
        ck.equal("group %d C == float32 sum in chunk order, bit for bit" % q, got, G.epilogue(acc32, **kw))
    ck.done()


# ============================================================================================ pack padding
PACK_SHAPES = [(1, 1), (70, 33), (129, 100), (257, 67), (300, 132)]


@pytest.mark.parametrize("k_major", [0, 1], ids=["k_contiguous", "k_major"])
@pytest.mark.parametrize("rows,K", PACK_SHAPES, ids=["%dx%d" % s for s in PACK_SHAPES])
def test_pack1_writes_every_byte_and_rounds_rne(rows, K, k_major):
    """lstc_pack1 into a 0xFF-filled buffer of lstc_pack1_bytes: every byte in front of the documented slack (P1_SLACK, the last
    lstc_pack1_bytes - tiles * 8192 bytes) is written - values inside the matrix are the RNE bf16 of the source (read back through
    lstc_unpack1_rows), everything outside is zero, no 0xFFFF (NaN) element is left."""
    L = _L()
    ck = Checks("pack1", "%dx%d k_major=%d" % (rows, K, k_major))
    x = torch.randn(rows, K, generator=G.gen(rows, K, k_major))
    src = x.t().contiguous() if k_major else x
    ps = Placed([src], _ld(src.shape[1], True), 5, NAN, NAN)          # an unaligned source with an odd leading dimension and NaN pads
    buf, nbytes = _pack(1, ps.ptr(), rows, K, ps.ld, k_major)
    torch.cuda.synchronize()
    rbp, kbp = -(-rows // 128), -(-K // 32)
    rbp, kbp = rbp + rbp % 2, kbp + kbp % 2
    tiles_bytes = rbp * kbp * 128 * 32 * 2
    ck.true("lstc_pack1_bytes = even tile grid + the 64-KiB slack", nbytes - tiles_bytes == 65536)
    body = buf[:tiles_bytes].view(torch.int16).cpu()
    ck.true("no 0xFFFF element left in the tiles", not bool((body == -1).any()))
    ck.true("guard bytes behind the pack unchanged", bool((buf[nbytes:] == 0xA5).all()) and ps.unchanged())
    vals = body.to(torch.int32).bitwise_and(0xFFFF).bitwise_left_shift(16).view(F32)
    ck.true("the tiles hold the matrix's %d values and zeros" % (rows * K), bool(torch.isfinite(vals).all()) and
            int((vals != 0).sum()) == int((G.bf16_round(x) != 0).sum()))
    Kp = K + (-K) % 8
    if Kp == K:
        ck.equal("unpack(pack) == bf16 RNE of the source", _unpack1(buf, rows, K).cpu(), G.bf16_round(x))
    else:                                                            # lstc_unpack1_rows takes K % 8 == 0: read the zero-padded columns too
        full = _unpack1(buf, rows, Kp).cpu()
        ck.equal("unpack(pack) == bf16 RNE of the source", full[:, :K], G.bf16_round(x))
        ck.true("K padding reads back as zeros", bool((full[:, K:] == 0).all()))
    ck.done()


@pytest.mark.parametrize("k_major", [0, 1], ids=["k_contiguous", "k_major"])
@pytest.mark.parametrize("rows,K", PACK_SHAPES, ids=["%dx%d" % s for s in PACK_SHAPES])
def test_pack3_writes_every_tile_and_reads_back_through_an_identity_product(rows, K, k_major):
    """lstc_pack3 into a 0xFF-filled buffer: no NaN f16 is left in the rows / 128 x K / 32 tiles it owns (the spare row block of an
    odd count and the trailer behind its first 8 bytes are documented slack), and X @ I through LSTC_F32X3 returns h + l of every
    element - the planes' own sum - exactly."""
    L = _L()
    lib = L.load()
    ck = Checks("pack3", "%dx%d k_major=%d" % (rows, K, k_major))
    x = torch.randn(rows, K, generator=G.gen(rows, K, k_major, 3))
    src = x.t().contiguous() if k_major else x
    ps = Placed([src], _ld(src.shape[1], True), 5, NAN, NAN)
    buf, nbytes = _pack(3, ps.ptr(), rows, K, ps.ld, k_major)
    eye = torch.eye(K)
    pe = Placed([eye], _ld(K, False), 4, NAN, NAN)
    bufe, _ = _pack(3, pe.ptr(), K, K, pe.ld, 0)
    torch.cuda.synchronize()
    tiles_bytes = -(-rows // 128) * -(-K // 32) * 2 * 4096 * 2
    body = buf[:tiles_bytes].view(torch.float16).cpu()
    ck.true("every f16 of the owned tiles is written (finite)", bool(torch.isfinite(body.to(F32)).all()))
    ck.true("the planes hold nothing outside the matrix", int((body != 0).sum()) <= 2 * rows * K)
    ck.true("guard bytes behind the pack unchanged, source unchanged", bool((buf[nbytes:] == 0xA5).all()) and ps.unchanged())
    trailer = buf[tiles_bytes:tiles_bytes + 8].view(F32).cpu()
    s = G.pack3_scale(x)
    ck.true("trailer = absmax bits, 1 / scale", float(trailer[0]) == float(x.abs().max()) and float(trailer[1]) == 1.0 / s)
    pc = Placed([torch.full((rows, K), GUARD)], _ld(K, False), 4, GUARD, GUARD)
    d = L.GemmDesc()
    d.M, d.N, d.K, d.ldc, d.transA, d.transB, d.dtype, d.alpha = rows, K, K, pc.ld, 0, 1, G.LSTC_F32X3, 1.0
    d.A, d.B, d.C = buf.data_ptr(), bufe.data_ptr(), pc.ptr()
    L.check(lib.lstc_gemm(C.byref(d), L.stream_ptr()), "lstc_gemm identity")
    torch.cuda.synchronize()
    h, l, s = G.pack3_planes(x)
    ck.equal("X @ I == (h + l) / s", pc.view().cpu().to(F64), (h + l) / s)
    ck.true("guards of C", pc.outside_unchanged())
    ck.done()
