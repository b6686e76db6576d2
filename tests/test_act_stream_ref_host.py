"""CPU twin of tests/test_act_stream_f64_gpu.py.  tests/util_act16.py is checked before the kernels are held to it:

* the references are right: the float64 LayerNorm backward with its dropout replay and the three CLS passes agree with torch
  autograd of the plain formulas to 1e-12; the host pack writer and reader are inverses and agree with test_hip_parity._unpack1;
* the bars can see what they are for: at the shapes of the GPU file, each reference evaluated WITH one of eight defects lands
  beyond its tolerance;
* the rule is not vacuous: tol = 8 * max(e32, ...) >= 8 e32, so the float32 restatement of every reference sits at or under 1/8 of
  its bar by construction - asserted for every reference the GPU file uses, which also proves that each of them HAS a restatement
  and terms of the right shape;
* every refusal the GPU file relies on is returned by the library before any launch."""
import os

import pytest
import torch

import util_act16 as A
import util_gemm as G
import util_rowops as R

F64, F32 = torch.float64, torch.float32
SEED = 0x9E3779B900000005          # a 64-bit seed whose high word is not zero


def _ck(case):
    return A.Checks("host", case, record=False)


def _ln_bwd_setup(rows=256, d=1024, p=0.2):
    x, gamma, beta, _ = A.ln_inputs(rows, d, "randn")
    dy = A.bf16(torch.randn(rows, d, generator=G.gen(rows, d, 3)))
    _, mean, rstd = R.ln_fwd(x, gamma, beta, A.EPS)
    m32, r32 = mean.to(F32), rstd.to(F32)
    keep = A.host_keep(rows * d, p, SEED).view(rows, d) if p > 0 else torch.ones(rows, d, dtype=torch.bool)
    return x, gamma, dy, m32, r32, keep, A.ln_bwd_refs(dy, x, gamma, m32, r32, keep, p)


# ============================================================================================= the references are right
def test_layernorm_backward_reference_is_autograd_of_the_plain_formula():
    """z = LayerNorm(dropout(f) + x0): d/dx0 = dx, d/df = df = dx keep / (1 - p), d/dgamma, d/dbeta and the column sums of df,
    with the statistics in float64 (no f32 rounding between forward and backward): 1e-12."""
    rows, d, p = 12, 1024, 0.2
    g = G.gen(rows, d, 1)
    x0, f = torch.randn(rows, d, generator=g, dtype=F64), torch.randn(rows, d, generator=g, dtype=F64)
    gamma, beta = torch.randn(d, generator=g, dtype=F64), torch.randn(d, generator=g, dtype=F64)
    dz = torch.randn(rows, d, generator=g, dtype=F64)
    keep = A.host_keep(rows * d, p, SEED).view(rows, d)
    x0.requires_grad_(True); f.requires_grad_(True); gamma.requires_grad_(True); beta.requires_grad_(True)
    s = f * keep.to(F64) * A.drop_scale(p) + x0
    z = torch.nn.functional.layer_norm(s, (d,), gamma, beta, A.EPS)
    (z * dz).sum().backward()
    sd = s.detach()
    _, mean, rstd = R.ln_fwd(sd, gamma.detach(), beta.detach(), A.EPS)
    refs = A.ln_bwd_refs(dz, sd, gamma.detach(), mean, rstd, keep, p)
    for name, got, want in (("dx", refs["dx"][0], x0.grad), ("df", refs["df"][0], f.grad), ("dgamma", refs["cg"][0].sum(0), gamma.grad),
                            ("dbeta", refs["cb"][0].sum(0), beta.grad), ("dbias", refs["cd"][0].sum(0), f.grad.sum(0))):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    # the per-workgroup planes partition the rows: every row has one owner, the planes add up to the column sums
    for n_partial in (1, 3, 5, 6, 200):
        own = A.owner(rows, n_partial)
        assert own.max() < n_partial and torch.equal(own, torch.tensor([(r % (2 * n_partial)) // 2 for r in range(rows)]))
        assert float((A.plane_sums(refs["cg"][0], n_partial).sum(0) - gamma.grad).abs().max()) <= 1e-12 * float(gamma.grad.abs().max())


def test_cls_pass_references_are_autograd_of_each_other():
    """L = <g_s, dot(U, X)> + <g_y, wsum(W, X)>: dL/dX = outer(g_s, U, W, g_y) and dL/dU = wsum(g_s, X); mode 2 of the dot is the
    gradient of <dot, dropout(softmax(s))> with respect to s.  1e-12."""
    N, S, H, d, p = 3, 17, 3, 64, 0.3
    g = G.gen(N, S, H, d)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    U, X, W, gs, gy = rn(N, H, d), rn(N, S, d), rn(N, H, S), rn(N, H, S), rn(N, H, d)
    U.requires_grad_(True); X.requires_grad_(True)
    (A.cls_dot(U, X, 0)[0] * gs).sum().add((A.cls_wsum(W, X) * gy).sum()).backward()
    assert float((A.cls_outer(gs, U.detach(), W, gy) - X.grad).abs().max()) <= 1e-12 * float(X.grad.abs().max())
    assert float((A.cls_wsum(gs, X.detach()) - U.grad).abs().max()) <= 1e-12 * float(U.grad.abs().max())
    keep = A.cls_keep_rows(A.host_keep(N * H * S * S, p, SEED), N, H, S)
    s = rn(N, H, S).requires_grad_(True)
    dot = A.cls_dot(U.detach(), X.detach(), 0)[0]
    (torch.softmax(s, -1) * keep.to(F64) * A.drop_scale(p) * dot).sum().backward()
    got, _ = A.cls_dot(U.detach(), X.detach(), 2, Pin=torch.softmax(s.detach(), -1), keep=keep, p=p)
    assert float((got - s.grad).abs().max()) <= 1e-12 * max(1.0, float(s.grad.abs().max()))
    out, P = A.cls_dot(U.detach(), X.detach(), 1, keep=keep, p=p)
    assert float((P.sum(-1) - 1).abs().max()) < 1e-14 and torch.equal(out == 0, ~keep)
    # add0 lands on row 0 of every sequence and nowhere else
    add0 = rn(N, d)
    diff = A.cls_outer(gs, U.detach(), W, gy, add0) - A.cls_outer(gs, U.detach(), W, gy)
    assert float((diff[:, 0, :] - add0).abs().max()) <= 1e-12 and float(diff[:, 1:, :].abs().max()) == 0.0


@pytest.mark.parametrize("rows,K", [(256, 64), (256, 320), (640, 200), (768, 1024), (100, 40)])
def test_host_pack_writer_and_reader_are_inverses_and_agree_with_unpack1(rows, K):
    from test_hip_parity import _unpack1
    x = A.bf16(torch.randn(rows, K, generator=G.gen(rows, K)))
    x[0, 0] = -0.0
    buf = A.pack_write(x)
    assert buf.numel() == A.grid_elems(rows, K) and buf.numel() % (2 * A.TILE) == 0
    assert torch.equal(A.bits(A.pack_read(buf, rows, K)), A.bits(x))
    assert torch.equal(A.bits(_unpack1(buf.view(torch.uint8), rows, K)), A.bits(x))
    off = A.pack_offsets(rows, K)
    assert off.unique().numel() == rows * K                                            # one place per element
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    mask[off] = False
    assert bool((A.bits(buf)[mask] == 0).all())                                        # everything else: +0, as lstc_pack1 pads
    # the layout as the header states it, element by element on a few coordinates
    for r, k in ((0, 0), (5, 9), (rows - 1, K - 1), (min(rows - 1, 131), min(K - 1, 33))):
        rr, ch = r & 127, (k & 31) >> 3
        want = ((r >> 7) * A.kbp(K) + (k >> 5)) * 4096 + rr * 32 + ((ch ^ ((rr >> 2) & 3)) << 3) + (k & 7)
        assert int(off[r * K + k]) == want and A.kbp(K) % 2 == 0 and A.rbp(rows) % 2 == 0


# ============================================================================================= the bars see the defects
def test_bar_sees_dead_tail_rows_taking_row_0():
    """rows = 256, n_partial = 3: iteration 42 holds rows 252 .. 257, workgroup 2's two slots are dead and clamped to row 0.
    Treated as live they add row 0 into workgroup 2's planes twice more (and rewrite row 0's dx with the same values)."""
    _, _, _, _, _, _, refs = _ln_bwd_setup()
    ck = _ck("dead tail, np=3")
    for key in ("cg", "cb", "cd"):
        (ref, f32, terms), (tref, tf32, tterms) = A.plane_refs(refs[key], 3)
        bad = ref.clone()
        bad[2] += 2 * refs[key][0][0]
        ck.beyond(key + " plane", bad.to(F32), ref, f32, terms)
        ck.beyond(key + " sum", bad.sum(0).to(F32), tref, tf32, tterms)
    ck.done()


def test_bar_sees_a_reused_reduction_slot():
    """One iteration of one workgroup reads the LDS slot of the iteration two back (the buffer has two slots, indexed by it & 1):
    its rows' dx are formed with the m1, m2 of the row 2 * stride earlier."""
    x, gamma, dy, m32, r32, keep, refs = _ln_bwd_setup()
    d, n_partial, w, it = x.shape[1], 5, 1, 7
    stride = 2 * n_partial
    xh = (x.to(F64) - m32.to(F64)[:, None]) * r32.to(F64)[:, None]
    gd = dy.to(F64) * gamma.to(F64)
    m1, m2 = gd.sum(-1) / d, (gd * xh).sum(-1) / d
    bad = refs["dx"][0].clone()
    for slot in (0, 1):
        r = it * stride + 2 * w + slot
        bad[r] = r32.to(F64)[r] * (gd[r] - m1[r - 2 * stride] - xh[r] * m2[r - 2 * stride])
    ck = _ck("reduction slot reused")
    ck.beyond("dx_pack", A.bf16(bad.to(F32)), *refs["dx"], packed=True)
    ck.beyond("df_pack", A.bf16((bad * keep * A.drop_scale(0.2)).to(F32)), *refs["df"], packed=True)
    ck.done()


@pytest.mark.parametrize("rows,d", [(256, 64), (256, 320)])
def test_bar_sees_a_dropout_counter_off_by_8(rows, d):
    """One 16-B chunk (8 columns) of one row takes the mask of the flat indices 8 further."""
    p = 0.3
    x = A.bf16(torch.randn(rows, d, generator=G.gen(rows, d, 8)))
    keep = A.host_keep(rows * d + 8, p, SEED)
    good = keep[:rows * d].view(rows, d)
    r, c0 = 77, 24
    bad = good.clone()
    bad[r, c0:c0 + 8] = keep[r * d + c0 + 8:r * d + c0 + 16]
    assert not torch.equal(bad, good)
    ref, f32, terms = A.dropout_refs(x, good, p)
    ck = _ck("dropout counter + 8")
    ck.close("the correct replay", A.bf16(A.dropout_refs(x, good, p)[1]), ref, f32, terms, packed=True)
    ck.beyond("y_pack", A.bf16(A.dropout_refs(x, bad, p)[1]), ref, f32, terms, packed=True)
    ck.done()


def test_bar_sees_an_unwritten_partial_plane():
    """A workgroup that writes nothing leaves what the buffer held: NaN in the GPU file (every output starts as NaN), and a
    stale finite value is caught as well - in a plane with rows and in a plane without (n_partial = 200: exact zeros)."""
    _, _, _, _, _, _, refs = _ln_bwd_setup()
    ck = _ck("plane unwritten")
    for n_partial, w in ((64, 5), (200, 150)):
        (ref, f32, terms), _ = A.plane_refs(refs["cb"], n_partial)
        for stale in (float("nan"), 1e-3):
            bad = ref.to(F32).clone()
            bad[w] = stale
            ck.beyond("np=%d plane %d = %s" % (n_partial, w, stale), bad, ref, f32, terms)
    assert float(A.plane_refs(refs["cb"], 200)[0][0][128:].abs().max()) == 0.0          # the rowless planes' reference: zeros
    ck.done()


def test_bar_sees_the_empty_row_group_of_colsum_pack1():
    """(768, 320) over 4 groups: RB = 6, per = 2, group 3 starts at row block 6 and owns nothing.  Left unzeroed, whatever its
    partial row held is added into the result."""
    rows, K, n_partial = 768, 320, 4
    assert A.colsum_groups(rows, n_partial) == (4, 2) and A.rbp(rows) == 6
    x = A.bf16(torch.randn(rows, K, generator=G.gen(rows, K, 4)))
    pref, pf32, pterms = A.colsum_partial_refs(x, n_partial)
    assert float(pref[3].abs().max()) == 0.0 and float(pterms[3].max()) == 0.0
    ck = _ck("colsum empty group")
    for what, stale in (("NaN (the GPU file's fill)", torch.full((K,), float("nan"))), ("an earlier call's sums", pref[0].to(F32))):
        bad = pref.to(F32).clone()
        bad[3] = stale
        ck.beyond("partial, " + what, bad, pref, pf32, pterms)
        ck.beyond("out, " + what, bad.sum(0), R.colsum(x), R.colsum(x, F32), R.colsum_terms(x))
    ck.done()


def test_bar_sees_a_dropped_head_at_h3():
    """H = 3 runs the HT = 4 text with one zero lane; a kernel that stopped at H - 1 loses head 2."""
    N, S, H, d = 256, 49, 3, 512
    U, U2, W, W2, add0, X, Pin = A.cls_inputs(N, S, H, d, "randn")
    ck = _ck("head 2 dropped")
    ref = A.cls_dot(U, X, 0)[0]
    bad = ref.to(F32).clone()
    bad[:, 2] = 0
    ck.beyond("dot", bad, ref, A.cls_dot(U, X, 0, dtype=F32)[0], A.cls_dot_terms(U, X, 0)[0], fmt64=A.cls_dot(U, X, 0, fmt=True)[0])
    ref = A.cls_wsum(W, X)
    bad = ref.to(F32).clone()
    bad[:, 2] = 0
    ck.beyond("wsum", bad, ref, A.cls_wsum(W, X, F32), A.cls_wsum_terms(W, X))
    ref = A.cls_outer(W, U, W2, U2, add0)
    ck.beyond("outer", A.bf16(A.cls_outer(W, U, W2, U2, add0, heads=2).to(F32)), ref, A.cls_outer(W, U, W2, U2, add0, dtype=F32),
              A.cls_outer_terms(W, U, W2, U2, add0), fmt64=A.cls_outer(W, U, W2, U2, add0, fmt="kept"), packed=True)
    ck.done()


def test_bar_sees_dropped_hi_x_lo_products_on_the_range_family():
    """The outer product keeps six of the eight hi / lo products.  With only hi x hi (operands rounded to bf16 before the product)
    the result leaves the packed bar + e_fmt on the range family; with the six kept ones it stays inside."""
    N, S, H, d = 256, 49, 8, 512
    U, U2, W, W2, add0, X, _ = A.cls_inputs(N, S, H, d, "range")
    ref, f32, terms = A.cls_outer(W, U, W2, U2, add0), A.cls_outer(W, U, W2, U2, add0, dtype=F32), A.cls_outer_terms(W, U, W2, U2, add0)
    kept = A.cls_outer(W, U, W2, U2, add0, fmt="kept")
    ck = _ck("outer hi x lo dropped")
    ck.close("six products", A.bf16(kept.to(F32)), ref, f32, terms, fmt64=kept, packed=True)
    ck.beyond("hi x hi only", A.bf16(A.cls_outer(W, U, W2, U2, add0, fmt="hi_only").to(F32)), ref, f32, terms, fmt64=kept, packed=True)
    ck.done()


def test_bar_sees_a_wrong_chunk_xor_in_one_tile_row():
    """A pack written with row 133's chunk XOR off by one: read back with the right layout, that row's 16-B chunks are permuted."""
    rows, d, p = 256, 64, 0.0
    x = A.bf16(torch.randn(rows, d, generator=G.gen(rows, d, 9)))
    got = A.pack_read(A.pack_write(x, bad_xor_row=133), rows, d)
    assert torch.equal(got[:133], x[:133]) and torch.equal(got[134:], x[134:]) and not torch.equal(got[133], x[133])
    ck = _ck("chunk XOR")
    ck.beyond("y_pack", got, *A.dropout_refs(x, torch.ones(rows, d, dtype=torch.bool), p), packed=True)
    ck.done()


# ============================================================================================= the rule is not vacuous
def _under_an_eighth(ck, what, ref, f32, terms, fmt64=None, packed=False):
    r = ck.ratio(what, f32, ref, f32, terms, fmt64, packed)
    ck.true(what + ": f32 restatement <= tol / 8", r <= 0.125)
    ck.true(what + ": a non-trivial bar", float(torch.as_tensor(terms).abs().max()) > 0)


@pytest.mark.parametrize("d", [1024, 2048])
@pytest.mark.parametrize("family", A.LN_FAMILIES)
def test_rule_layernorm_references(d, family):
    """tol = 8 max(e32, floor) >= 8 e32: the f32 restatement is at most an eighth of every bar, by construction."""
    rows = 256
    x, gamma, beta, const = A.ln_inputs(rows, d, family)
    ref, f32, terms = A.ln_fwd_refs(x, gamma, beta)
    ck = _ck("rule ln d=%d %s" % (d, family))
    for gname, idx in A.ln_row_groups(rows, const, "cpu"):
        for i, name in enumerate(("y", "mean", "rstd")):
            _under_an_eighth(ck, gname + name, ref[i][idx], f32[i][idx], terms[i][idx])
        _under_an_eighth(ck, gname + "y_pack", ref[0][idx], f32[0][idx], terms[0][idx], packed=True)
    if const is not None:       # variance 0: rstd = 1 / sqrt(eps) and y = beta, in float64 exactly and in the f32 restatement under the rule
        assert float(ref[2][const]) == A.EPS ** -0.5 and torch.equal(ref[0][const], beta.to(F64))
    if family == "randn":
        _, _, _, _, _, _, b = _ln_bwd_setup(rows, d, 0.2)
        for key in ("dx", "df"):
            _under_an_eighth(ck, key, *b[key], packed=True)
        for n_partial in (1, 3, 64, 128, 200):
            for key in ("cg", "cb", "cd"):
                per, tot = A.plane_refs(b[key], n_partial)
                _under_an_eighth(ck, "%s planes np=%d" % (key, n_partial), *per)
                _under_an_eighth(ck, "%s sum np=%d" % (key, n_partial), *tot)
    ck.done()


def test_rule_dropout_and_colsum_references():
    ck = _ck("rule dropout / colsum")
    for rows, d in ((256, 64), (256, 320), (512, 2048)):
        x = A.bf16(torch.randn(rows, d, generator=G.gen(rows, d, 8)))
        keep = A.host_keep(rows * d, 0.3, SEED).view(rows, d)
        _under_an_eighth(ck, "dropout %dx%d" % (rows, d), *A.dropout_refs(x, keep, 0.3), packed=True)
    for rows, K, n_partial in ((256, 64, 1), (768, 320, 4), (640, 200, 8), (1280, 2048, 64)):
        x = A.bf16(torch.randn(rows, K, generator=G.gen(rows, K, 4)))
        _under_an_eighth(ck, "colsum partial %dx%d" % (rows, K), *A.colsum_partial_refs(x, n_partial))
        _under_an_eighth(ck, "colsum out %dx%d" % (rows, K), R.colsum(x), R.colsum(x, F32), R.colsum_terms(x))
    ck.done()


@pytest.mark.parametrize("family", ["randn", "range"])
@pytest.mark.parametrize("S,H,d", [(1, 8, 512), (49, 3, 1024), (128, 8, 512)])
def test_rule_cls_references(S, H, d, family):
    N, p = 256, 0.3
    U, U2, W, W2, add0, X, Pin = A.cls_inputs(N, S, H, d, family)
    keep = A.cls_keep_rows(A.host_keep(N * H * S * S, p, SEED), N, H, S)
    ck = _ck("rule cls S=%d H=%d d=%d %s" % (S, H, d, family))
    for mode in (0, 1, 2):
        kw = dict(Pin=Pin, keep=keep, p=p)
        ref, f32, terms, fmt = (A.cls_dot(U, X, mode, **kw), A.cls_dot(U, X, mode, dtype=F32, **kw), A.cls_dot_terms(U, X, mode, **kw),
                                A.cls_dot(U, X, mode, fmt=True, **kw))
        _under_an_eighth(ck, "dot mode %d out" % mode, ref[0], f32[0], terms[0], fmt64=fmt[0])
        if mode == 1:
            _under_an_eighth(ck, "dot mode 1 probs", ref[1], f32[1], terms[1], fmt64=fmt[1])
    _under_an_eighth(ck, "wsum", A.cls_wsum(W, X), A.cls_wsum(W, X, F32), A.cls_wsum_terms(W, X))
    _under_an_eighth(ck, "outer", A.cls_outer(W, U, W2, U2, add0), A.cls_outer(W, U, W2, U2, add0, dtype=F32),
                     A.cls_outer_terms(W, U, W2, U2, add0), fmt64=A.cls_outer(W, U, W2, U2, add0, fmt="kept"), packed=True)
    ck.done()


def test_int_family_is_exact_in_f32_and_in_bf16():
    """Every product and sum of the int family is an integer below 2**24, every dX value one below 2**8: the f32 restatement EQUALS
    the float64 reference, and the format's hi + lo split loses nothing - so the GPU file may demand equality."""
    N, S, H, d = 256, 49, 8, 2048
    U, U2, W, W2, add0, X, _ = A.cls_inputs(N, S, H, d, "int")
    assert torch.equal(A.cls_dot(U, X, 0, dtype=F32)[0].to(F64), A.cls_dot(U, X, 0)[0])
    assert torch.equal(A.cls_dot(U, X, 0, fmt=True)[0], A.cls_dot(U, X, 0)[0])
    assert torch.equal(A.cls_wsum(W, X, F32).to(F64), A.cls_wsum(W, X))
    ref = A.cls_outer(W, U, W2, U2, add0)
    assert float(ref.abs().max()) <= 256 and torch.equal(A.bf16(ref.to(F32)).to(F64), ref)
    assert torch.equal(A.cls_outer(W, U, W2, U2, add0, fmt="kept"), ref)


# ============================================================================================= refusals
def test_every_refusal_happens_before_a_launch():
    """Run on the host library the way tests/test_cabi_host.py does: 16 stands for an aligned pointer, 24 for one 8 bytes off."""
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for label, name, args, code in A.refusals(16, 24):
        assert getattr(lib, name)(*args, None) == code, label
