"""Padded (ragged) batches on the GPU: per-sequence lengths through the CLS concat, the re-associated CLS attention and the
encoder, and ragged batched scoring.

Kernel level, against the float64 references of tests/util_ragged.py (checked on the CPU by tests/test_ragged_host.py): the
concat under the one tolerance rule of tests/util_rowops.tol, lstc_cls_dot_len under the bars tests/test_attn_mask_gpu.py applies
to the CLS kernels (util_mask.bar).  Model level, against the oracle run on every sequence ALONE (oracle.lstc_oracle, float32 on
the CPU): outputs within 1e-4 absolute (the north_star bar of tests/test_hip_parity.py), parameter gradients within
2e-4 of the tensor's maximum + 1e-7 (tests/test_hip_parity.py:94).  Every model-level test also runs the control arm - the
existing un-padded path on each length group - at the same bar, so a failure names the arm.  Padding holds NaN wherever a
result must not depend on it."""
import pytest
import torch

import util_ragged as R
from util import _LibSpy
from util_mask import bar
from util_rowops import tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _lib():
    from lstc_vad_amd import _lib
    return _lib


def _bitwise_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ---------------------------------------------------------------------------------------------------- 1. CLS concat with lengths
def _concat_fwd(x, lens, cls, pos, S):
    L = _lib()
    N, T, d = x.shape
    y = torch.full((N, S, d), float("nan"), device=DEV)
    L.check(L.load().lstc_cls_concat_len_fwd(L.dev_ptr(x), L.dev_ptr(lens), L.dev_ptr(cls), L.dev_ptr(pos), L.dev_ptr(y), N, S, d,
                                             L.stream_ptr()), "lstc_cls_concat_len_fwd")
    return y


def _concat_bwd(dy, lens, mean_cls):
    L = _lib()
    N, S, d = dy.shape
    dx = torch.full((N, S - 1, d), float("nan"), device=DEV)
    dtok = torch.full((S, d), float("nan"), device=DEV)
    L.check(L.load().lstc_cls_concat_len_bwd(L.dev_ptr(dy), L.dev_ptr(lens), L.dev_ptr(dx), L.dev_ptr(dtok), N, S, d, int(mean_cls),
                                             L.stream_ptr()), "lstc_cls_concat_len_bwd")
    return dx, dtok


def _misaligned(t):
    """A copy of ``t`` 4 bytes off a 16-byte boundary: the entry points then take their 4-byte path."""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    v.copy_(t)
    return v


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("N,d,lens", [(6, 36, [1, 2, 16, 33, 48, 49]), (6, 30, [1, 2, 16, 33, 48, 49]), (3, 2048, [1, 33, 49])])
def test_cls_concat_len_kernels_against_f64(N, d, lens, learned, with_pos):
    """lstc_cls_concat_len_fwd / _bwd: d = 36 the 16-byte path, d = 30 the 4-byte path, d = 2048 several workgroups per row.  NaN in
    the padding of x reaches nothing; rows past L_n of y and dx are bitwise zero; the 4-byte path gives the 16-byte path's bits."""
    T, S = 49, 50
    g = torch.Generator().manual_seed(100 + d + 2 * learned + with_pos)
    x = torch.randn(N, T, d, generator=g) + 0.5
    cls = torch.randn(d, generator=g) if learned else None
    pos = torch.randn(S, d, generator=g) if with_pos else None
    dy = torch.randn(N, S, d, generator=g)
    xn = x.clone()
    for n, L in enumerate(lens):
        xn[n, L:] = float("nan")
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    y = _concat_fwd(dev(xn), lens_d, dev(cls), dev(pos), S)
    dx, dtok = _concat_bwd(dev(dy), lens_d, not learned)
    torch.cuda.synchronize()
    ref = R.cls_concat_len_fwd(xn, lens, cls, pos)
    t_y = tol(ref, R.cls_concat_len_fwd(xn, lens, cls, pos, dtype=F32), R.cls_concat_len_terms(xn, lens, cls, pos))
    rdx, rtok = R.cls_concat_len_bwd(dy, lens, not learned)
    fdx, ftok = R.cls_concat_len_bwd(dy, lens, not learned, dtype=F32)
    adx, atok = R.cls_concat_len_bwd_terms(dy, lens, not learned)
    errs = {"y": (float((y.cpu().double() - ref).abs().max()), t_y),
            "dx": (float((dx.cpu().double() - rdx).abs().max()), tol(rdx, fdx, adx)),
            "dtok": (float((dtok.cpu().double() - rtok).abs().max()), tol(rtok, ftok, atok))}
    print(N, d, learned, with_pos, {k: "%.3e / %.3e" % v for k, v in errs.items()})
    for t in (y, dx, dtok):
        assert torch.isfinite(t).all()
    for n, L in enumerate(lens):
        assert _bitwise_zero(y[n, L + 1:]) and _bitwise_zero(dx[n, L:]), n
    assert all(e <= t for e, t in errs.values()), errs
    if d % 4 == 0:
        # the summation order does not depend on the access width: misaligned operands take the 4-byte kernels
        y4 = _concat_fwd(_misaligned(dev(xn)), lens_d, dev(cls), dev(pos), S)
        dx4, dtok4 = _concat_bwd(_misaligned(dev(dy)), lens_d, not learned)
        torch.cuda.synchronize()
        assert torch.equal(y4, y) and torch.equal(dx4, dx) and torch.equal(dtok4, dtok)


def test_cls_concat_len_full_lengths_equal_the_unlengthed_kernels():
    """lens = S - 1 everywhere: the un-lengthed twins' results (same per-column sequential sums)."""
    Fn = _Fn()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 49, 36, generator=g).to(DEV)
    dy = torch.randn(4, 50, 36, generator=g).to(DEV)
    lens = torch.full((4,), 49, dtype=torch.int32, device=DEV)
    y = _concat_fwd(x, lens, None, None, 50)
    dx, _ = _concat_bwd(dy, lens, True)
    xr = x.clone().requires_grad_(True)
    y0 = Fn.ClsConcatFunction.apply(xr, None, None)
    y0.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(y, y0.detach()) and torch.equal(dx, xr.grad)


# ---------------------------------------------------------------------------------------------------- 2. lstc_cls_dot_len
DOT_CASES = [((4, 2, 2, 64), [[1, 2, 2, 1]]),
             ((5, 49, 2, 64), [[1, 2, 49, 30, 48]]),
             ((4, 65, 8, 64), [[1, 2, 64, 65], [65, 64, 33, 2]]),
             ((3, 128, 16, 32), [[1, 64, 128], [2, 65, 127]])]


def _dot_inputs(N, S, H, d, seed):
    g = torch.Generator().manual_seed(seed)
    U = torch.randn(N, H, d, generator=g) * (d ** -0.5)
    G = torch.randn(N, H, d, generator=g)
    X = torch.randn(N, S, d, generator=g)
    return U, G, X


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("shape,klens", DOT_CASES)
def test_cls_dot_len_against_f64(shape, klens, p_drop):
    """Mode 1 (softmax over the keys j < klen, dropout replayed from lstc_dropout_mask), with modes 0 and 2 behind it.  The rows
    X[n, j >= klen] hold NaN; probs and out are bitwise 0 there."""
    Fn = _Fn()
    N, S, H, d = shape
    seed = 77 + S
    U, G, X = _dot_inputs(N, S, H, d, 31 * S + H)
    keep = Fn.dropout_mask((N, H, S, S), p_drop, seed, DEV)[:, :, 0].cpu() if p_drop > 0 else None
    for klen in klens:
        Xn = X.clone()
        for n, kl in enumerate(klen):
            Xn[n, kl:] = float("nan")
        kd = torch.tensor(klen, dtype=torch.int32, device=DEV)
        Ud, Gd, Xd = U.to(DEV), G.to(DEV), Xn.to(DEV)
        raw, _ = Fn.cls_dot_len(Ud, Xd, kd, 0)
        out, probs = Fn.cls_dot_len(Ud, Xd, kd, 1, None, p_drop, seed)
        ds, _ = Fn.cls_dot_len(Gd, Xd, kd, 2, probs, p_drop, seed)
        torch.cuda.synchronize()
        r_raw, _ = R.cls_dot_len(U, Xn, klen, 0)
        r_out, r_p = R.cls_dot_len(U, Xn, klen, 1, keep=keep, p_drop=p_drop)
        r_ds, _ = R.cls_dot_len(G, Xn, klen, 2, probs=probs.cpu().double(), keep=keep, p_drop=p_drop)
        errs = {}
        for name, kind, got, ref in (("raw", "O", raw, r_raw), ("P", "P", probs, r_p), ("out", "O", out, r_out), ("ds", "O", ds, r_ds)):
            assert torch.isfinite(got).all(), (klen, name)
            errs[name] = (float((got.cpu().double() - ref).abs().max()), bar(kind, ref))
            for n, kl in enumerate(klen):
                assert _bitwise_zero(got[n, :, kl:]), (klen, name, n)
        print(shape, klen, p_drop, {k: "%.3e / %.3e" % v for k, v in errs.items()})
        assert all(e <= b for e, b in errs.values()), (klen, errs)
        assert float((probs.sum(-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("shape", [c[0] for c in DOT_CASES])
def test_cls_dot_len_at_full_length_is_cls_dot_bit_for_bit(shape, p_drop):
    Fn = _Fn()
    N, S, H, d = shape
    U, G, X = (t.to(DEV) for t in _dot_inputs(N, S, H, d, 5 * S + H))
    kd = torch.full((N,), S, dtype=torch.int32, device=DEV)
    for mode, u in ((0, U), (1, U)):
        a = Fn.cls_dot_len(u, X, kd, mode, None, p_drop, 1234)
        b = Fn.cls_dot(u, X, mode, None, p_drop, 1234)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and (mode == 0 or torch.equal(a[1], b[1])), mode
    probs = b[1]
    a, _ = Fn.cls_dot_len(G, X, kd, 2, probs, p_drop, 1234)
    b, _ = Fn.cls_dot(G, X, 2, probs, p_drop, 1234)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 3. model level
LENS_A = [1, 5, 16, 32, 48]          # S = 49: first-generation masked kernels + re-associated CLS form
LENS_B = [16, 100, 144]              # S = 145: key-tiled masked kernels + masked CLS-query kernels
CASES = {"a": (3, LENS_A, {}), "b": (9, LENS_B, {}),
         "a_cls_learned": (3, LENS_A, {"CLS_learned": True}),
         "a_position": (3, LENS_A, {"position_encoding": True}),
         "a_input_ln": (3, LENS_A, {"input_layerNorm": True}),
         "a_src_mask": (3, LENS_A, {})}


def _band(S):
    """A band mask [S, S] that keeps the CLS column and row: no query row is fully masked."""
    i = torch.arange(S)
    m = (i[:, None] - i[None, :]).abs() <= 6
    m[:, 0] = True
    m[0, :] = True
    return m


_built = {}


def _case(name, dropout=0.0):
    """(encoder on the GPU, oracle parameters, oracle cfg, sequences on the CPU, band or None); built once per (case, dropout) -
    the sequences and the parameter values are never modified."""
    key = (name, dropout)
    if key not in _built:
        from lstc_vad_amd.models import Encoder
        depth, lens, extra = CASES[name]
        kw = R.encoder_kw(depth, dropout, **extra)
        torch.manual_seed(17 + depth)
        enc = Encoder(**kw)
        with torch.no_grad():
            for layer in enc.layer_stack:
                layer.slf_attn.relative_position_bias_table.normal_(0.0, 0.4)
                for ln in (layer.slf_attn.layer_norm, layer.pos_ffn.layer_norm):
                    ln.weight.add_(0.1 * torch.randn_like(ln.weight))
                    ln.bias.add_(0.1 * torch.randn_like(ln.bias))
            enc.layer_norm.weight.add_(0.1 * torch.randn_like(enc.layer_norm.weight))       # used with input_layerNorm only
            enc.layer_norm.bias.add_(0.1 * torch.randn_like(enc.layer_norm.bias))
        P = {k: v.detach().clone() for k, v in enc.state_dict().items()}
        g = torch.Generator().manual_seed(23)
        seqs = [torch.randn(L, 32, generator=g) for L in lens]
        band = _band(depth * 16 + 1) if name == "a_src_mask" else None
        _built[key] = (enc.to(DEV), P, R.oracle_cfg(kw), seqs, band)
    return _built[key]


def _oracle_alone(P, cfg, seq, band):
    L = seq.shape[0]
    with torch.no_grad():
        return R.oracle_encoder_masked(P, seq[None], cfg, None if band is None else band[:L + 1, :L + 1])[0]


@pytest.mark.parametrize("name", list(CASES))
def test_padded_batch_matches_oracle_on_every_sequence_alone(name):
    """forward rows 0..L_n and forward_cls row n within 1e-4 of the oracle on x[n:n+1, :L_n]; the control arm (each sequence through
    the un-padded path) at the same bar; probabilities of padded keys are 0 and every row sums to 1."""
    enc, P, cfg, seqs, band = _case(name)
    enc.eval()
    x, lens = R.pad_sequences(seqs, enc.layer_stack[0].slf_attn.relative_position_index.shape[0])
    x = x.to(DEV)
    mask = None if band is None else band.to(DEV)
    with torch.no_grad():
        full, attn = enc(x, src_mask=mask, return_attn=True, lengths=lens)
        cls = enc.forward_cls(x, src_mask=mask, lengths=torch.tensor(lens, device=DEV))        # device lengths: no host check
        torch.cuda.synchronize()
        assert torch.isfinite(full).all() and torch.isfinite(cls).all()
        errs = {}
        for n, (seq, L) in enumerate(zip(seqs, lens)):
            ref = _oracle_alone(P, cfg, seq, band)
            m1 = None if band is None else band[:L + 1, :L + 1].to(DEV)
            ctl_full = enc(seq[None].to(DEV), src_mask=m1)
            ctl_cls = enc.forward_cls(seq[None].to(DEV), src_mask=m1)
            errs[L] = {"control forward": float((ctl_full[0].cpu() - ref).abs().max()),
                       "control forward_cls": float((ctl_cls[0].cpu() - ref[0]).abs().max()),
                       "padded forward": float((full[n, :L + 1].cpu() - ref).abs().max()),
                       "padded forward_cls": float((cls[n].cpu() - ref[0]).abs().max())}
            for a in attn:
                assert _bitwise_zero(a[n, :, :, L + 1:]) and float((a[n].sum(-1) - 1).abs().max()) < 1e-5
        print(name, {L: {k: "%.2e" % v for k, v in e.items()} for L, e in errs.items()})
        bad = {(L, k): v for L, e in errs.items() for k, v in e.items() if not v < 1e-4}
        assert not bad, bad


@pytest.mark.parametrize("name", ["a", "b", "a_cls_learned", "a_position", "a_input_ln"])
def test_padded_batch_parameter_gradients_match_oracle_autograd(name):
    """Gradients of forward_cls(x, lengths).sum() in training mode (dropout 0) against the oracle's autograd summed over the
    sequences run alone: per tensor within 2e-4 * max|g| + 1e-7 (tests/test_hip_parity.py:94).  Control arm: the un-padded path,
    one call per sequence, gradients accumulated."""
    from oracle import lstc_oracle as orc
    enc, P, cfg, seqs, _ = _case(name)
    enc.train()
    Pg = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    total = sum(orc.encoder_forward(Pg, s[None], cfg, training=True)[:, 0].sum() for s in seqs)
    total.backward()
    x, lens = R.pad_sequences(seqs, enc.layer_stack[0].slf_attn.relative_position_index.shape[0])
    arms = {}
    enc.zero_grad(set_to_none=True)
    enc.forward_cls(x.to(DEV), lengths=lens).sum().backward()
    arms["padded"] = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters() if p.grad is not None}
    enc.zero_grad(set_to_none=True)
    for s in seqs:
        enc.forward_cls(s[None].to(DEV)).sum().backward()
    arms["control"] = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters() if p.grad is not None}
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    want = {k for k, v in Pg.items() if v.is_floating_point() and v.grad is not None}
    bad = {}
    for arm, grads in arms.items():
        assert set(grads) == want, (arm, set(grads) ^ want)
        for k, g in grads.items():
            ref = Pg[k].grad
            err, t = float((g - ref).abs().max()), 2e-4 * float(ref.abs().max()) + 1e-7
            assert torch.isfinite(g).all(), (arm, k)
            if not err < t:
                bad[(arm, k)] = (err, t)
    print(name, "worst err / bar", {arm: max(float((g - Pg[k].grad).abs().max()) / (2e-4 * float(Pg[k].grad.abs().max()) + 1e-7)
                                                 for k, g in grads.items()) for arm, grads in arms.items()})
    assert not bad, bad


@pytest.mark.parametrize("name", ["a", "b"])
def test_padding_gets_exact_zero_gradient_and_changes_no_bit(name):
    """All dropout rates 0.2, training mode: x.grad[n, L_n:] is bitwise zero and every parameter gradient finite with NaN in the
    padding; the outputs are the bits of the same call (same seeds) with zeros in the padding."""
    Fn = _Fn()
    enc, _, _, seqs, _ = _case(name, dropout=0.2)
    enc.train()
    T = enc.layer_stack[0].slf_attn.relative_position_index.shape[0]
    x_nan, lens = R.pad_sequences(seqs, T)
    x_zero, _ = R.pad_sequences(seqs, T, fill=0.0)
    outs = []
    for x in (x_zero, x_nan):
        Fn.reset_rng(4000)
        torch.manual_seed(1)
        with torch.no_grad():
            outs.append((enc.forward_cls(x.to(DEV), lengths=lens), enc(x.to(DEV), lengths=lens)))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    xg = x_nan.to(DEV).requires_grad_(True)
    enc.zero_grad(set_to_none=True)
    enc.forward_cls(xg, lengths=lens).sum().backward()
    torch.cuda.synchronize()
    for n, L in enumerate(lens):
        assert _bitwise_zero(xg.grad[n, L:]), n
        assert torch.isfinite(xg.grad[n, :L]).all() and float(xg.grad[n, :L].abs().max()) > 0
    for k, p in enc.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k
    enc.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------------- 4. routing
def _spy(monkeypatch):
    L = _lib()
    spy = _LibSpy(L.load())
    monkeypatch.setattr(L, "load", lambda: spy)
    return spy


NEW_SYMBOLS = {"lstc_cls_concat_len_fwd", "lstc_cls_concat_len_bwd", "lstc_cls_dot_len"}


def test_lengths_route_the_cls_layer_to_the_reassociated_form(monkeypatch):
    """(a): the CLS-only layer runs MHAClsAssocFunction on lstc_cls_dot_len - no K / V projection of the padded batch, no masked
    CLS-query kernel; the full layers run the masked first-generation kernels.  (b), S = 145: the K/V-projecting form with the
    masked CLS-query kernels.  A ``src_mask`` beside the lengths sends (a) to the K/V-projecting form as well."""
    Fn = _Fn()
    for name, assoc in (("a", True), ("b", False), ("a_src_mask", False)):
        enc, _, _, seqs, band = _case(name)
        enc.train()
        x, lens = R.pad_sequences(seqs, enc.layer_stack[0].slf_attn.relative_position_index.shape[0])
        seen = {"assoc": 0, "kv": 0}
        for cls_name, key in (("MHAClsAssocFunction", "assoc"), ("MHAClsFunction", "kv")):
            real = getattr(Fn, cls_name).forward

            def fwd(ctx, *a, _real=real, _key=key):
                seen[_key] += 1
                return _real(ctx, *a)
            monkeypatch.setattr(getattr(Fn, cls_name), "forward", staticmethod(fwd))
        spy = _spy(monkeypatch)
        enc.forward_cls(x.to(DEV), src_mask=None if band is None else band.to(DEV), lengths=lens).sum().backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        enc.zero_grad(set_to_none=True)
        assert seen == ({"assoc": 1, "kv": 0} if assoc else {"assoc": 0, "kv": 1}), (name, seen)
        c = spy.calls
        assert c.count("lstc_cls_concat_len_fwd") == 1 and "lstc_cls_concat_fwd" not in c
        assert c.count("lstc_attn_fwd_masked") == 2 and c.count("lstc_attn_bwd_masked") == 2 and "lstc_attn_fwd" not in c
        if assoc:
            assert c.count("lstc_cls_dot_len") == 2 and "lstc_cls_dot" not in c and "lstc_attn_cls_fwd_masked" not in c
            assert c.count("lstc_cls_wsum") == 2 and c.count("lstc_cls_outer") == 1
        else:
            assert c.count("lstc_attn_cls_fwd_masked") == 1 and c.count("lstc_attn_cls_bwd_masked") == 1 and "lstc_cls_dot_len" not in c


def test_without_lengths_the_call_sequence_is_unchanged(monkeypatch):
    """``lengths=None`` launches what it launched before lengths existed: the recorded sequence of C entry points of a training
    step through forward_cls and of an evaluation forward (tests/golden/ragged_calls.json, recorded on the commit before this
    feature), and none of the new symbols."""
    import json
    import os
    from util import GOLDEN
    want = json.load(open(os.path.join(GOLDEN, "ragged_calls.json")))
    for name in ("a", "b"):
        enc, _, _, seqs, _ = _case(name)
        x = torch.stack([seqs[-1], seqs[-1].flip(0)]).to(DEV)
        spy = _spy(monkeypatch)
        enc.train()
        enc.forward_cls(x).sum().backward()
        n_train = len(spy.calls)
        enc.eval()
        with torch.no_grad():
            enc(x, return_attn=True)
        torch.cuda.synchronize()
        monkeypatch.undo()
        enc.zero_grad(set_to_none=True)
        got = {"train_forward_cls": spy.calls[:n_train], "eval_forward": spy.calls[n_train:]}
        assert not NEW_SYMBOLS & set(spy.calls)
        assert got == want[name], name


# ---------------------------------------------------------------------------------------------------- 5. scoring
def test_ragged_scoring_matches_grouped_scoring_and_the_oracle():
    """40 sequences of 1, 2 and 3 parts at P = 16 plus a few single-clip ones (1, 3 and 7 tokens): ``ragged=True`` within 1e-4 of
    ``ragged=False``, both within 1e-4 of the oracle on every sequence alone, results in input order."""
    from lstc_vad_amd.models import Classifier
    from lstc_vad_amd.scoring import ltn_sequence_scores
    from oracle import lstc_oracle as orc
    enc, P, cfg, _, _ = _case("a")
    enc.eval()
    torch.manual_seed(41)
    head = Classifier(32, 0.0)
    hP = {k: v.detach().clone() for k, v in head.state_dict().items()}
    head = head.to(DEV).eval()
    g = torch.Generator().manual_seed(42)
    lens = [16 * (1 + int(v)) for v in torch.randint(0, 3, (40,), generator=g)] + [1, 3, 7, 1]
    seqs = [torch.randn(L, 32, generator=g) for L in lens]
    dseqs = [s.to(DEV) for s in seqs]
    with torch.no_grad():
        grouped = ltn_sequence_scores(enc, head, dseqs).cpu()
        ragged = ltn_sequence_scores(enc, head, dseqs, ragged=True).cpu()
        small = ltn_sequence_scores(enc, head, dseqs, max_batch=16, ragged=True).cpu()        # several padded batches
        ref = torch.stack([orc.head_forward(hP, orc.encoder_forward(P, s[None], cfg)[:, 0], "classifier", 0.0)[0, 1] for s in seqs])
    errs = {"grouped vs oracle": float((grouped - ref).abs().max()), "ragged vs oracle": float((ragged - ref).abs().max()),
            "ragged vs grouped": float((ragged - grouped).abs().max()), "ragged in batches of 16 vs oracle": float((small - ref).abs().max())}
    print({k: "%.2e" % v for k, v in errs.items()})
    assert float(ref.max() - ref.min()) > 1e-3          # the scores tell the sequences apart: order mistakes would show
    assert all(v < 1e-4 for v in errs.values()), errs
