"""The kernels only the bf16 activation stream uses, arm by arm, through the C ABI with every argument set by the test, against the
float64 references of tests/util_act16.py (checked on the CPU by tests/test_act_stream_ref_host.py):

  1  lstc_layernorm_fwd_act   ln_fwd_act<NC, XP, YF, YP>: 2 widths x 6 arms, three input families, the grid-stride second trip
  2  lstc_layernorm_bwd_act   ln_bwd_act<NCH, DYP, DX>: 2 widths x 4 arms x six loop shapes (1, 2, 43, 77, 128 iterations, dead
                              tail, rowless workgroups), dropout off and on
  3  lstc_dropout_apply_pack  four shapes (KBp = 2, 10, 64; the second trip), p = 0 and 0.3
  4  lstc_colsum_pack1        four shapes (one group, an empty group, rows and K off the tile, more groups than blocks), accumulate
  5  lstc_cls_dot_pack / _wsum_pack / _outer_pack   the S edges of the 16-token blocks, H = 1 .. 8 x d = 512 / 1024 / 2048

Every parametrised case is named after the instantiation it reaches and restates that arm's dispatch condition before the launch.
Input packs are written on the host (util_act16.pack_write), output packs start as 0xFF and are read on the host; f32 outputs sit
between NaN guards.  One tolerance rule (util_rowops.tol; packed outputs + 2**-8 |ref| per element; split operands + e_fmt), every
check prints err / tol, the worst ratio per section is printed at the end and written to the file LSTC_ACT_STREAM_ERRORS names
(profiles/act_stream_errors.txt).  mean / rstd of the backward come from the float64 reference, not from the forward under test.

Measured on an MI355X, worst err / tol: f32 outputs 0.080 (ln_fwd_act), 0.053 (ln_bwd_act planes), 0.008 (colsum_pack1), 0.131
(cls_dot_pk), 0.109 (cls_wsum_pk); packed outputs 0.85 - 0.99, which is their one RNE rounding against its own 2**-8 |ref| allowance
(half a bf16 ulp just above a power of two), not drift.  No case found a kernel defect."""
import functools

import pytest
import torch

import util_act16 as A
import util_gemm as G
import util_rowops as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
SEED = 0x9E3779B900000005          # a 64-bit seed whose high word is not zero
NT = 256                           # threads of a workgroup (csrc/lstc_common.h)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    A.report()


def _grid(rows, K):
    """Bytes of the pack's tile grid; the shapes of sections 1 - 3 and 5 fill it exactly."""
    return 2 * A.grid_elems(rows, K)


# ============================================================================================ 0  the host pack is lstc_pack1's
@pytest.mark.parametrize("rows,K", [(256, 64), (256, 320), (640, 200), (768, 1024)])
def test_host_pack_is_bitwise_lstc_pack1(rows, K):
    x = A.bf16(torch.randn(rows, K, generator=G.gen(rows, K))).to(DEV)
    dst = A.out_pack(rows, K, DEV)
    A.call("lstc_pack1", x, rows, K, K, 0, dst)
    torch.cuda.synchronize()
    assert torch.equal(dst[:_grid(rows, K)], A.pack_write(x).view(torch.uint8)) and A.slack_intact(dst, rows, K)
    assert torch.equal(A.bits(A.pack_read(dst, rows, K)), A.bits(x))


def test_refusals():
    """include/lstc_hip.h: d = 768, rows % 256, H = 9, S = 129, both or neither of x / x_pack (dy / dy_pack), dropout_p = 1, a
    misaligned pack pointer - each returns its code and launches nothing (one large buffer stands for every operand)."""
    big = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    for label, name, args, code in A.refusals(big, big[8:]):
        assert A.rc(name, *args) == code, label
    torch.cuda.synchronize()
    assert int(big.max()) == 0


# ============================================================================================ 1  lstc_layernorm_fwd_act
@functools.lru_cache(maxsize=8)
def _fwd_case(rows, d, family):
    x, gamma, beta, const = A.ln_inputs(rows, d, family)
    x, gamma, beta = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    return dict(x=x, gamma=gamma, beta=beta, const=const, xp=A.in_pack(x, DEV), refs=A.ln_fwd_refs(x, gamma, beta))


def _run_fwd(c, XP, YF, YP):
    rows, d = c["x"].shape
    y, yb = A.guarded((rows, d), DEV) if YF else (None, None)
    mean, mb = A.guarded((rows,), DEV)
    rstd, rb = A.guarded((rows,), DEV)
    yp = A.out_pack(rows, d, DEV) if YP else None
    x_in, xp_in = c["x"].clone(), c["xp"].clone()
    A.call("lstc_layernorm_fwd_act", None if XP else x_in, xp_in if XP else None, c["gamma"], c["beta"], y, yp, mean, rstd, rows, d, A.EPS)
    torch.cuda.synchronize()
    intact = (A.guards_ok(mb) and A.guards_ok(rb) and (not YF or A.guards_ok(yb)) and (not YP or A.slack_intact(yp, rows, d)) and
              torch.equal(x_in, c["x"]) and torch.equal(xp_in, c["xp"]))
    return y, yp, mean, rstd, intact


def _check_fwd(ck, tag, c, XP, YF, YP):
    rows, d = c["x"].shape
    y, yp, mean, rstd, intact = _run_fwd(c, XP, YF, YP)
    ck.true(tag + " guards, pack slack and inputs unchanged", intact)
    ypv = A.pack_read(yp, rows, d) if YP else None
    A.check_ln_fwd(ck, tag, c["refs"], c["const"], y, mean, rstd, ypv)
    if YF and YP:
        ck.equal(tag + " pack == bf16(y)", ypv, A.bf16(y))
    if (XP, YF, YP) != (True, True, True):          # the same values through another arm: the same bits
        y0, yp0, mean0, rstd0, _ = _run_fwd(c, True, True, True)
        ck.equal(tag + " mean == the (pack -> f32 + pack) arm's", mean, mean0)
        ck.equal(tag + " rstd == the (pack -> f32 + pack) arm's", rstd, rstd0)
        if YF:
            ck.equal(tag + " y == the (pack -> f32 + pack) arm's", y, y0)
        if YP:
            ck.equal(tag + " y_pack == the (pack -> f32 + pack) arm's", yp[:_grid(rows, d)], yp0[:_grid(rows, d)])


FWD_ARMS = [(d, XP, YF, YP) for d in (1024, 2048) for XP in (True, False) for (YF, YP) in ((True, True), (True, False), (False, True))]


def _fwd_id(a):
    d, XP, YF, YP = a
    return "ln_fwd_act_NC%d_%s_to_%s" % (d // 512, "xpack" if XP else "xf32", "f32_and_pack" if YF and YP else "f32" if YF else "pack")


@pytest.mark.parametrize("d,XP,YF,YP", FWD_ARMS, ids=[_fwd_id(a) for a in FWD_ARMS])
def test_layernorm_fwd_act(d, XP, YF, YP):
    rows = 256
    assert rows % 256 == 0 and d in (1024, 2048) and d // 512 in (2, 4)          # NC = d / 512 chunks of 8 columns per lane
    ck = A.Checks("1 ln_fwd_act", _fwd_id((d, XP, YF, YP)))
    for family in A.LN_FAMILIES:
        _check_fwd(ck, family, _fwd_case(rows, d, family), XP, YF, YP)
    ck.done()


@pytest.mark.parametrize("XP", [True, False], ids=["ln_fwd_act_NC2_xpack_second_trip", "ln_fwd_act_NC2_xf32_second_trip"])
def test_layernorm_fwd_act_grid_stride_second_trip(XP):
    """At most 4096 workgroups of four waves, one row per wave and trip: rows 16384 .. 16639 are a second trip."""
    rows, d = 16640, 1024
    assert rows > 4096 * (NT // 64) and rows % 256 == 0
    ck = A.Checks("1 ln_fwd_act", "NC2 %s rows=%d" % ("xpack" if XP else "xf32", rows))
    c = _fwd_case(rows, d, "constant_row")
    y, yp, mean, rstd, intact = _run_fwd(c, XP, True, True)
    ck.true("guards, pack slack and inputs unchanged", intact)
    ypv = A.pack_read(yp, rows, d)
    A.check_ln_fwd(ck, "second_trip", c["refs"], c["const"], y, mean, rstd, ypv)
    ck.equal("pack == bf16(y)", ypv, A.bf16(y))
    ck.done()


# ============================================================================================ 2  lstc_layernorm_bwd_act
# (rows, n_partial, iterations, live rows of the last iteration, workgroups without a row, id)
BWD_LOOPS = [
    (256, 1, 128, 2, 0, "128_iterations"),
    (256, 3, 43, 4, 0, "43_iterations_dead_tail_4_of_6"),
    (256, 64, 2, 128, 0, "two_iterations"),
    (256, 128, 1, 256, 0, "one_iteration_no_prefetch"),
    (256, 200, 1, 256, 72, "72_rowless_workgroups"),
    (768, 5, 77, 8, 0, "77_iterations_dead_tail_8_of_10"),
]
BWD_ARMS = [(d, DYP, DX) for d in (1024, 2048) for DYP in (True, False) for DX in (True, False)]


def _bwd_id(a):
    d, DYP, DX = a
    return "ln_bwd_act_NCH%d_%s_%s" % (d // 1024, "dypack" if DYP else "dyf32", "dx" if DX else "nodx")


@functools.lru_cache(maxsize=None)
def _bwd_case(rows, d, p):
    x, gamma, beta, _ = A.ln_inputs(rows, d, "randn")
    dy = A.bf16(torch.randn(rows, d, generator=G.gen(rows, d, 3)))
    x, gamma, beta, dy = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    _, mean, rstd = R.ln_fwd(x, gamma, beta, A.EPS)
    mean32, rstd32 = mean.to(F32), rstd.to(F32)
    keep = A.device_keep(rows * d, p, SEED, DEV).view(rows, d) if p > 0 else torch.ones(rows, d, dtype=torch.bool, device=DEV)
    return dict(x=x, gamma=gamma, dy=dy, mean=mean32, rstd=rstd32, keep=keep, xp=A.in_pack(x, DEV), dyp=A.in_pack(dy, DEV),
                refs=A.ln_bwd_refs(dy, x, gamma, mean32, rstd32, keep, p))


def _run_bwd(c, DYP, DX, n_partial, p):
    rows, d = c["x"].shape
    ins = [c[k].clone() for k in ("dy", "dyp", "xp", "gamma", "mean", "rstd")]
    dy, dyp, xp, gamma, mean, rstd = ins
    partial, pb = A.guarded((3, n_partial, d), DEV)          # exactly 3 * n_partial * d floats between the guards
    dxp = A.out_pack(rows, d, DEV) if DX else None
    dfp = A.out_pack(rows, d, DEV)
    A.call("lstc_layernorm_bwd_act", None if DYP else dy, dyp if DYP else None, xp, gamma, mean, rstd, dxp, partial, n_partial, rows, d,
           float(p), SEED, dfp)
    torch.cuda.synchronize()
    intact = (A.guards_ok(pb) and A.slack_intact(dfp, rows, d) and (not DX or A.slack_intact(dxp, rows, d)) and
              all(torch.equal(a, c[k]) for a, k in zip(ins, ("dy", "dyp", "xp", "gamma", "mean", "rstd"))))
    return dxp, dfp, partial, intact


@pytest.mark.parametrize("rows,n_partial,iters,last_live,rowless,_id", BWD_LOOPS, ids=[l[-1] for l in BWD_LOOPS])
@pytest.mark.parametrize("d,DYP,DX", BWD_ARMS, ids=[_bwd_id(a) for a in BWD_ARMS])
def test_layernorm_bwd_act(d, DYP, DX, rows, n_partial, iters, last_live, rowless, _id):
    stride = 2 * n_partial                                   # a workgroup's wave pairs take rows 2w, 2w + 1, then every stride further
    assert -(-rows // stride) == iters and rows - (iters - 1) * stride == last_live and max(0, n_partial - rows // 2) == rowless
    assert rows % 256 == 0 and d // 1024 in (1, 2)           # NCH = d / 1024 chunks per lane and half row
    for p in (0.0, 0.2):
        ck = A.Checks("2 ln_bwd_act", "%s %s p=%g" % (_bwd_id((d, DYP, DX)), _id, p))
        c = _bwd_case(rows, d, p)
        refs, keep = c["refs"], c["keep"]
        dxp, dfp, partial, intact = _run_bwd(c, DYP, DX, n_partial, p)
        ck.true("guards around partial, pack slack, every input unchanged", intact)
        df = A.pack_read(dfp, rows, d)
        ck.close("df_pack", df, *refs["df"], packed=True)
        ck.true("df is +0 where the mask drops", (A.bits(df)[~keep] == 0).all())
        if DX:
            dx = A.pack_read(dxp, rows, d)
            ck.close("dx_pack", dx, *refs["dx"], packed=True)
            ck.true("df == 0 exactly where the mask drops or dx rounds to zero", torch.equal(df == 0, ~keep | (dx == 0)))
            if p == 0.0:
                ck.equal("p = 0: df_pack == dx_pack", dfp[:_grid(rows, d)], dxp[:_grid(rows, d)])
        for i, (key, name) in enumerate((("cg", "dgamma"), ("cb", "dbeta"), ("cd", "df column sums"))):
            per, tot = A.plane_refs(refs[key], n_partial)
            ck.close(name + " plane per workgroup", partial[i], *per)
            ck.close(name + " planes summed in float64", partial[i].to(F64).sum(0), *tot)
        if rowless:
            ck.true("planes of workgroups without a row are zeros", (A.bits(partial[:, n_partial - rowless:]) == 0).all())
        if (DYP, DX) != (True, True):                        # dy's form and dx's presence change nothing else
            _, dfp0, partial0, _ = _run_bwd(c, True, True, n_partial, p)
            ck.equal("df_pack == the (dy pack, dx) arm's", dfp[:_grid(rows, d)], dfp0[:_grid(rows, d)])
            ck.equal("partial == the (dy pack, dx) arm's", partial, partial0)
        ck.done()


# ============================================================================================ 3  lstc_dropout_apply_pack
DROP_SHAPES = [(256, 64, "KBp2"), (256, 320, "KBp10_not_a_power_of_two"), (512, 2048, "KBp64"), (2304, 2048, "KBp64_second_trip")]


@pytest.mark.parametrize("p", [0.0, 0.3], ids=["p0", "p0.3"])
@pytest.mark.parametrize("rows,d,_id", DROP_SHAPES, ids=["dropout_apply_pack_" + s[-1] for s in DROP_SHAPES])
def test_dropout_apply_pack(rows, d, _id, p):
    chunks = rows * d // 8                                   # one 16-B chunk per thread and trip, at most 2048 workgroups
    assert rows % 256 == 0 and d % 64 == 0 and A.kbp(d) == d // 32 and (chunks > 2048 * NT) == _id.endswith("second_trip")
    ck = A.Checks("3 dropout_apply_pack", "%dx%d %s p=%g" % (rows, d, _id, p))
    x = A.bf16(torch.randn(rows, d, generator=G.gen(rows, d, 8))).to(DEV)
    xp = A.in_pack(x, DEV)
    xp_in, yp = xp.clone(), A.out_pack(rows, d, DEV)
    A.call("lstc_dropout_apply_pack", xp_in, yp, rows, d, float(p), SEED)
    keep = A.device_keep(rows * d, p, SEED, DEV).view(rows, d)
    torch.cuda.synchronize()
    y = A.pack_read(yp, rows, d)
    ck.true("input unchanged, bytes behind the tile grid unchanged", torch.equal(xp_in, xp) and A.slack_intact(yp, rows, d))
    ck.close("y_pack", y, *A.dropout_refs(x, keep, p), packed=True)
    ck.true("the kept set is the mask's", torch.equal(y == 0, ~keep | (x == 0)) and (A.bits(y)[~keep] == 0).all())
    if p == 0.0:
        ck.true("p = 0 keeps everything", keep.all())
        ck.equal("p = 0: a bit-exact copy", yp[:_grid(rows, d)], xp[:_grid(rows, d)])
    else:
        ck.true("the mask drops about p", abs(float((~keep).float().mean()) - p) < 0.01)
    ck.done()


# ============================================================================================ 4  lstc_colsum_pack1
COLSUM_SHAPES = [(256, 64, 1, "one_group"), (768, 320, 4, "RB6_over_4_groups_last_group_empty"),
                 (640, 200, 8, "rows_and_K_off_the_tile_KB7_KBp8"), (1280, 2048, 64, "more_groups_than_row_blocks")]


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("rows,K,n_partial,_id", COLSUM_SHAPES, ids=["colsum_pack1_" + s[-1] for s in COLSUM_SHAPES])
def test_colsum_pack1(rows, K, n_partial, _id, accumulate):
    """``partial`` holds exactly n_partial * K floats, the size include/lstc_hip.h promises ([n_partial, K])."""
    np_, per = A.colsum_groups(rows, n_partial)
    RB = A.rbp(rows)
    assert np_ == min(RB, n_partial) and per == -(-RB // np_)
    if _id.endswith("last_group_empty"):
        assert (np_ - 1) * per >= RB
    if _id.startswith("rows_and_K_off"):
        assert rows % 256 and K % 32 and (K + 31) // 32 == 7 and A.kbp(K) == 8 and RB == (rows + 127) // 128 + 1
    if _id.startswith("more_groups"):
        assert n_partial > RB and per == 1
    ck = A.Checks("4 colsum_pack1", "%dx%d np=%d %s accumulate=%d" % (rows, K, n_partial, _id, accumulate))
    g = G.gen(rows, K, 4)
    x = A.bf16(torch.randn(rows, K, generator=g)).to(DEV)
    out0 = torch.randn(K, generator=g).to(DEV)
    xp = A.in_pack(x, DEV)
    xp_in = xp.clone()
    partial, pb = A.guarded((n_partial, K), DEV)
    out, ob = A.guarded((K,), DEV, src=out0)
    A.call("lstc_colsum_pack1", xp_in, rows, K, partial, n_partial, out, accumulate)
    torch.cuda.synchronize()
    ck.true("guards around partial and out, input unchanged", A.guards_ok(pb) and A.guards_ok(ob) and torch.equal(xp_in, xp))
    ck.close("partial rows of the row-block groups", partial[:np_], *A.colsum_partial_refs(x, n_partial))
    ck.true("partial rows no group owns are not written", torch.isnan(partial[np_:]).all())
    ref, f32, terms = R.colsum(x), R.colsum(x, F32), R.colsum_terms(x)
    if accumulate:
        ref, f32, terms = ref + out0.to(F64), f32 + out0, terms + out0.to(F64).abs()
    ck.close("out", out, ref, f32, terms)
    ck.done()


# ============================================================================================ 5  the CLS passes over a packed X
CLS_N = 256                                                  # N * S is a multiple of 256 for every S
S_SWEEP = [(S, 8, 512) for S in (1, 2, 16, 17, 32, 33, 64, 65, 96, 97, 127, 128)]
HD_MATRIX = [(49, H, d) for H in (1, 2, 3, 4, 5, 7, 8) for d in (512, 1024, 2048)]


def _rbt(S):
    return 2 if S <= 32 else 4 if S <= 64 else 6 if S <= 96 else 8          # LSTC_RB_DISPATCH: blocks of 16 tokens


def _ht(H):
    return 2 if H <= 2 else 4 if H <= 4 else 8                              # LSTC_H8_DISPATCH


def _cls_id(S, H, d, family):
    return "cls_dot_pk_RBT%d-cls_outer_pk_RBT%d-cls_wsum_pk_HT%d_d%d-S%d-H%d-%s" % (_rbt(S), _rbt(S), _ht(H), d, S, H, family)


CLS_CASES = ([(S, H, d, f) for (S, H, d) in S_SWEEP + HD_MATRIX for f in ("randn", "range")] + [(49, 8, 2048, "int"), (97, 3, 512, "int")])


def _twice(run):
    """Two runs of one launch into fresh outputs: (first run's outputs, bit-identical?)."""
    a, b = run(), run()
    same = all(torch.equal(A.bits(u), A.bits(v)) for u, v in zip(a, b) if u is not None)
    return a, same


@pytest.mark.parametrize("S,H,d,family", CLS_CASES, ids=[_cls_id(*c) for c in CLS_CASES])
def test_cls_passes_over_a_pack(S, H, d, family):
    N = CLS_N
    assert (N * S) % 256 == 0 and 1 <= S <= 128 and 1 <= H <= 8 and d in (512, 1024, 2048)
    assert 16 * (_rbt(S) - 2) < S <= 16 * _rbt(S) or S <= 32              # the smallest RBT whose 16-token blocks cover S
    WPR = d // 512                                                          # waves per row of the weighted sum; RP = 4 / WPR row phases
    assert WPR in (1, 2, 4) and H <= _ht(H) and (H > _ht(H) // 2 or H == 1)
    exact = family == "int"
    U, U2, W, W2, add0, X, Pin = A.cls_inputs(N, S, H, d, family, DEV)
    xp = A.in_pack(X.view(N * S, d), DEV)
    xp_in = xp.clone()
    ck = A.Checks("5 cls_dot_pk", _cls_id(S, H, d, family))

    # ---- dot: mode 0, then softmax + dropout (1) and its backward (2), dropout off and on
    def dot(mode, p, probs_in=None):
        def run():
            out, ob = A.guarded((N, H, S), DEV)
            probs, pb = A.guarded((N, H, S), DEV, src=probs_in) if mode else (None, None)
            A.call("lstc_cls_dot_pack", U, xp_in, out, probs, N, S, H, d, mode, float(p), SEED)
            torch.cuda.synchronize()
            ck.true("mode %d p=%g guards" % (mode, p), A.guards_ok(ob) and (pb is None or A.guards_ok(pb)))
            return out, probs
        (out, probs), same = _twice(run)
        ck.true("mode %d p=%g two runs bit-identical" % (mode, p), same)
        return out, probs

    def dot_refs(mode, keep, p):
        kw = dict(Pin=Pin, keep=keep, p=p)
        return (A.cls_dot(U, X, mode, **kw), A.cls_dot(U, X, mode, dtype=F32, **kw), A.cls_dot_terms(U, X, mode, **kw),
                A.cls_dot(U, X, mode, fmt=True, **kw))

    out, _ = dot(0, 0.0)
    ref, f32, terms, fmt = dot_refs(0, None, 0.0)
    ck.close("mode 0 out", out, ref[0], f32[0], terms[0], fmt64=fmt[0])
    if exact:
        ck.true("int: mode 0 out EQUALS float64", torch.equal(out.to(F64), ref[0]))
    for p in (0.0, 0.3):
        keep = A.cls_keep_rows(A.device_keep(N * H * S * S, p, SEED, DEV), N, H, S) if p > 0 else torch.ones(N, H, S, dtype=torch.bool, device=DEV)
        ref, f32, terms, fmt = dot_refs(1, keep, p)
        out, probs = dot(1, p)
        ck.close("mode 1 p=%g probs" % p, probs, ref[1], f32[1], terms[1], fmt64=fmt[1])
        ck.close("mode 1 p=%g out" % p, out, ref[0], f32[0], terms[0], fmt64=fmt[0])
        ck.close("mode 1 p=%g probs rows sum to 1" % p, probs.to(F64).sum(-1), ref[1].sum(-1), f32[1].sum(-1), terms[1].sum(-1),
                 fmt64=fmt[1].sum(-1))
        ck.true("mode 1 p=%g dropped positions are the mask's" % p, torch.equal(out == 0, ~keep | (probs == 0)))
        ref, f32, terms, fmt = dot_refs(2, keep, p)
        out, probs = dot(2, p, probs_in=Pin)
        ck.close("mode 2 p=%g out" % p, out, ref[0], f32[0], terms[0], fmt64=fmt[0])
        ck.equal("mode 2 p=%g probs is an input" % p, probs, Pin)
    ck.done()

    # ---- weighted sum
    ck = A.Checks("5 cls_wsum_pk", _cls_id(S, H, d, family))

    def wsum():
        Y, yb = A.guarded((N, H, d), DEV)
        A.call("lstc_cls_wsum_pack", W, xp_in, Y, N, S, H, d)
        torch.cuda.synchronize()
        ck.true("guards", A.guards_ok(yb))
        return (Y,)
    (Y,), same = _twice(wsum)
    ck.true("two runs bit-identical", same)
    ref = A.cls_wsum(W, X)
    ck.close("Y", Y, ref, A.cls_wsum(W, X, F32), A.cls_wsum_terms(W, X))
    if exact:
        ck.true("int: Y EQUALS float64", torch.equal(Y.to(F64), ref))
    ck.true("the input pack is unchanged", torch.equal(xp_in, xp))
    ck.done()

    # ---- outer product into a pack, with and without the CLS rows' extra term
    ck = A.Checks("5 cls_outer_pk", _cls_id(S, H, d, family))
    got = {}
    for name, extra in (("add0 NULL", None), ("add0", add0)):
        def outer():
            dxp = A.out_pack(N * S, d, DEV)
            A.call("lstc_cls_outer_pack", W, U, W2, U2, extra, dxp, N, S, H, d)
            torch.cuda.synchronize()
            ck.true(name + " bytes behind the tile grid unchanged", A.slack_intact(dxp, N * S, d))
            return (dxp,)
        (dxp,), same = _twice(outer)
        ck.true(name + " two runs bit-identical", same)
        dX = A.pack_read(dxp, N * S, d).view(N, S, d)
        got[name] = dX
        ref = A.cls_outer(W, U, W2, U2, extra)
        ck.close(name + " dX_pack", dX, ref, A.cls_outer(W, U, W2, U2, extra, dtype=F32), A.cls_outer_terms(W, U, W2, U2, extra),
                 fmt64=A.cls_outer(W, U, W2, U2, extra, fmt="kept"), packed=True)
        if exact:
            ck.true("int: " + name + " dX EQUALS float64", torch.equal(dX.to(F64), ref))
    ck.equal("rows 1 .. S - 1 do not carry add0", got["add0"][:, 1:], got["add0 NULL"][:, 1:])
    if family != "range":       # (range: products of order 2**20 swallow an add0 of order 1 in bf16; the float64 bar above holds row 0)
        ck.true("row 0 of every sequence carries add0", (got["add0"][:, 0] != got["add0 NULL"][:, 0]).any(-1).all())
    ck.done()
