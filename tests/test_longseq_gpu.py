"""Long-sequence attention (128 < S <= 512, csrc/attention_long.hip) on the GPU: the kernels against a float64 restatement of
the attention contract (include/lstc_hip.h), bit-reproducible backward, and the layers above them - Encoder forward / forward_cls,
return_attn, a training step against the oracle, the command line and part scoring - at sequence lengths the short kernels
refuse."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import attn_reference, attn_rounded_probs

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel_index(S, ld):
    """1-D relative offsets of a ld + 1 token window, [ld, ld] (top-left (S-1) x (S-1) block read): within one row distinct
    columns hit distinct table rows, as for the models' 3-D / 2-D indices."""
    i = torch.arange(ld).view(-1, 1)
    j = torch.arange(ld).view(1, -1)
    return (j - i + ld - 1).long(), 2 * ld - 1


def _run(N, S, H, dk, bias, sliced, p_drop, seed=11, bf16=False):
    from lstc_vad_amd import functional as Fn
    dv = dk
    g = torch.Generator(device="cpu").manual_seed(1000 * S + dk + (7 if bias else 0) + (3 if sliced else 0))
    qkv = torch.randn(N * S, H * (2 * dk + dv), generator=g).to(DEV)
    q, k, v = qkv[:, : H * dk], qkv[:, H * dk: 2 * H * dk], qkv[:, 2 * H * dk:]
    do = torch.randn(N * S, H * dv, generator=g).to(DEV)
    table = index = None
    if bias:
        index, rows = _rel_index(S, (S - 1) + (37 if sliced else 0))
        table = (0.5 * torch.randn(rows, H, generator=g)).to(DEV)
        index = index.to(DEV)
    prev = Fn.get_compute_dtype()
    Fn.set_compute_dtype("bf16" if bf16 else "fp32")
    try:
        o, probs = Fn.attn_fwd(q, k, v, N, S, H, dk, dv, table, index, p_drop, seed)
        g3 = torch.empty_like(qkv)          # dQ / dK / dV with the row strides of Q / K / V (column blocks of one buffer)
        out = (g3[:, : H * dk], g3[:, H * dk: 2 * H * dk], g3[:, 2 * H * dk:])
        dq, dk_, dv_, dtab = Fn.attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, p_drop, seed, out=out)
    finally:
        Fn.set_compute_dtype(prev)
    keep = Fn.dropout_mask((N, H, S, S), p_drop, seed, DEV) if p_drop > 0 else None
    ref = attn_reference(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop)
    return (probs, o, dq, dk_, dv_, dtab), ref, (q, k, table, index)


SHAPES = [(4, 129, 2, 16), (8, 145, 2, 32), (2, 257, 8, 256), (1, 512, 1, 64)]


@pytest.mark.parametrize("bias,sliced,p_drop", [(False, False, 0.0), (True, False, 0.2), (True, True, 0.0), (True, True, 0.2)])
@pytest.mark.parametrize("shape", SHAPES)
def test_long_attention_matches_float64(shape, bias, sliced, p_drop):
    """Exact-f32 products at the short path's bars: P within 1e-6, the rest within 2e-5 of the tensor's maximum + 1e-6."""
    got, ref, _ = _run(*shape, bias, sliced, p_drop)
    names = ("probs", "O", "dQ", "dK", "dV", "dtable")
    for name, a, b in zip(names, got, ref):
        if b is None:
            assert a is None, name
            continue
        a, b = a.double(), b.to(a.device)
        assert torch.isfinite(a).all(), name
        err = float((a - b).abs().max())
        bar = 1e-6 if name == "probs" else 2e-5 * float(b.abs().max()) + 1e-6
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("shape", [(4, 129, 2, 16), (2, 257, 8, 256)])
def test_long_attention_bf16_products_track_float64(shape):
    """bf16 products: P within 4e-6 of the f64 softmax of the logits of the RNE-rounded operands (K and Q * scale); O and every
    gradient with a relative Frobenius error above 10x the exact-f32 run's (the bf16 path ran) and below 8e-3."""
    got, ref, (q, k, table, index) = _run(*shape, True, True, 0.2, bf16=True)
    exact, _, _ = _run(*shape, True, True, 0.2)
    N, S, H, dk = shape
    err_p = float((got[0].double() - attn_rounded_probs(q, k, N, S, H, dk, table, index)).abs().max())
    assert err_p < 4e-6, err_p
    for name, a, e, b in zip(("O", "dQ", "dK", "dV", "dtable"), got[1:], exact[1:], ref[1:]):
        err = float((a.double() - b).norm() / b.norm())
        err_exact = float((e.double() - b).norm() / b.norm())
        assert err_exact < 1e-5 and 10 * err_exact < err < 8e-3, (name, err, err_exact)


def test_long_backward_is_bit_reproducible():
    from lstc_vad_amd import functional as Fn
    N, S, H, dk, dv = 8, 145, 2, 32, 32
    g = torch.Generator(device="cpu").manual_seed(5)
    q, k, v, do = (torch.randn(N * S, H * dk, generator=g).to(DEV) for _ in range(4))
    index, rows = _rel_index(S, S + 15)
    table, index = torch.randn(rows, H, generator=g).to(DEV), index.to(DEV)
    _, probs = Fn.attn_fwd(q, k, v, N, S, H, dk, dv, table, index, 0.2, 77)
    r1 = Fn.attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, 0.2, 77)
    r2 = Fn.attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, 0.2, 77)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)


def _encoder(part_len, n_patch, d=32, H=2, dk=16, dropout=0.0):
    from lstc_vad_amd.models import Encoder
    ws = int(round(n_patch ** 0.5))
    torch.manual_seed(0)
    return Encoder(n_layers=3, MHA_attn_dropout=dropout, MHA_fc_dropout=dropout, FFN_dropout=dropout, weight_init=True,
                   n_head=H, d_k=dk, d_v=dk, d_model=d, d_inner=2 * d, MHA_layerNorm=True, FFN_layerNorm=True,
                   relative_pe=True, window_size=ws, window_depth=part_len)


@pytest.mark.parametrize("part_len,n_patch,dk", [(9, 16, 16), (16, 16, 32)])
def test_forward_cls_equals_full_forward_row0_long(part_len, n_patch, dk):
    enc = _encoder(part_len, n_patch, dk=dk).to(DEV).eval()
    S = part_len * n_patch
    x = torch.randn(6, S, 32, device=DEV)
    with torch.no_grad():
        full = enc(x)
        cls = enc.forward_cls(x)
    assert full.shape == (6, S + 1, 32)
    assert float((cls - full[:, 0]).abs().max()) < 5e-6


def test_return_attn_probabilities_are_normalised_rows():
    enc = _encoder(9, 16).to(DEV).eval()
    x = torch.randn(3, 144, 32, device=DEV)
    with torch.no_grad():
        out, attns = enc(x, return_attn=True)
    assert out.shape == (3, 145, 32)
    for a in attns:
        assert a.shape == (3, 2, 145, 145)
        assert float((a.sum(-1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("cls_only", [False, True])
def test_training_step_gradients_match_oracle_at_s145(cls_only):
    """One LTN step at part_len 9 x 16 patches (S = 145) through TrainStep against the oracle evaluated in float64 (non-zero
    bias tables): scores, loss and EVERY parameter gradient at the bars of the golden step test (2e-4 of the tensor's
    maximum).  cls_only=True runs the last layer on the S <= 512 instantiation of the CLS-query kernels."""
    _training_step_matches_oracle(9, 16, cls_only)


@pytest.mark.parametrize("cls_only", [False, True])
@pytest.mark.parametrize("part_len,n_patch", [(8, 16), (31, 16), (31, 9)])
def test_training_step_gradients_match_oracle_long(part_len, n_patch, cls_only):
    """As the S = 145 step at S = 129 (the first long length), 497 (part_len 31: the largest bias table the models build, 61 x 49
    rows, 47 KB of per-wave LDS tables in the backward) and 280 (9 patches, window 3: the 61 x 25-row table)."""
    _training_step_matches_oracle(part_len, n_patch, cls_only)


def _oracle_ltn_f64(orc, enc_P, head_P, ecfg, st, nf, af, al):
    """The LTN branch of oracle.forward_loss with parameters, features and activations in float64 (forward_loss casts the
    features to f32): the same oracle functions, without the reference's own f32 rounding.  At S = 497 that rounding alone
    moved the f32 oracle's gradients by up to 11x the bar on some CPUs (ReLU-edge units), while the product stays within
    half of it."""
    bs, pn, L, Pn, d = st.batch_size, st.part_num, st.part_len, st.n_patch, ecfg.d_model
    x = torch.cat([nf.double().reshape(bs * pn, L * Pn, d), af.double().reshape(bs * pn, L * Pn, d)], 0)
    enc = orc.encoder_forward(enc_P, x, ecfg, True, None)
    cls = enc[:, 0, :].reshape(bs * 2, pn, d)
    outputs = orc.head_forward(head_P, cls, "classifier", st.head_dropout, True, None).reshape(bs * 2 * pn, -1)
    ce = orc.ce_loss(outputs, orc.soft_targets(al, bs, pn, L).double().reshape(bs * 2 * pn, -1))
    mil, _, _ = orc.mil_loss(outputs[:, 1], bs, pn, 1, st.lambda_1)
    return outputs, st.lambda_MIL * mil + st.lambda_CE * ce


def _training_step_matches_oracle(part_len, n_patch, cls_only):
    from argparse import Namespace
    from lstc_vad_amd import synthetic as syn
    from lstc_vad_amd.engine import TrainStep
    from lstc_vad_amd.models import Classifier, Encoder
    from oracle import lstc_oracle as orc
    torch.manual_seed(0)
    ekw = dict(n_head=2, d_k=16, d_v=16, d_model=32, d_inner=64, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True,
               window_size=int(round(n_patch ** 0.5)), window_depth=part_len)
    bs, pn, L, P, d = 2, 3, part_len, n_patch, 32
    args = Namespace(batch_size=bs, part_num=pn, part_len=L, n_patch=P, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8,
                     temporal_only=False, clip_grad=False)
    enc = Encoder(n_layers=3, MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0, weight_init=True, **ekw)
    head = Classifier(d, 0.0)
    with torch.no_grad():      # a non-zero bias table, so its gradient is exercised
        for name, prm in enc.named_parameters():
            if "relative_position_bias_table" in name:
                prm.normal_(0.0, 0.5)
    enc_P = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in enc.state_dict().items()}
    head_P = {k: v.detach().double().requires_grad_(True) for k, v in head.state_dict().items()}
    nf, _, af, al = (torch.from_numpy(x) for x in syn.training_batch(bs, pn, L, P, d, seed=3, threshold=0.6))
    enc, head = enc.to(DEV).train(), head.to(DEV).train()
    ts = TrainStep(args, "LTN", enc, head, 1e-4, 1e-2, 1e-3, cls_only=cls_only)
    loss, scalars, outputs = ts.forward_loss(nf.to(DEV), af.to(DEV), al.to(DEV))
    ts.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    ecfg = orc.EncoderCfg(n_layers=3, MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0, **ekw)
    st = orc.StepCfg(mode="LTN", batch_size=bs, part_num=pn, part_len=L, n_patch=P, head_dropout=0.0)
    ref_outputs, ref_loss = _oracle_ltn_f64(orc, enc_P, head_P, ecfg, st, nf, af, al)
    ref_loss.backward()
    assert float((outputs.detach().cpu().double() - ref_outputs.detach().reshape(outputs.shape)).abs().max()) < 1e-4
    assert abs(float(scalars[0]) - float(ref_loss.detach())) < 2e-5
    n = 0
    for mod, refp in ((enc, enc_P), (head, head_P)):
        for k, p in mod.named_parameters():
            g = refp[k].grad
            if g is None:
                assert p.grad is None, k
                continue
            tol = 2e-4 * float(g.abs().max()) + 1e-7
            err = float((p.grad.cpu().double() - g).abs().max())
            assert err < tol, (k, err, tol)
            n += 1
    assert n > 20


def test_part_scores_at_part_len_9_with_a_short_tail():
    from lstc_vad_amd import scoring
    from lstc_vad_amd.models import Classifier
    enc = _encoder(9, 16).to(DEV).eval()
    head = Classifier(32, 0.0).to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(2)
    feats = torch.randn(31, 16, 32, generator=g).to(DEV)         # 3 whole parts of 9 clips and a tail of 4 (re-windowed)
    with torch.no_grad():
        scores, ranges = scoring.ltn_part_scores(enc, head, feats, 9)
        scores_cut, _ = scoring.ltn_part_scores(enc, head, feats, 9, tail="short")    # the tail as a 65-token sequence
    assert len(ranges) == 4 and scores.shape[0] == 4
    assert torch.isfinite(scores).all() and torch.isfinite(scores_cut).all()
    from lstc_vad_amd.metrics import roc_auc
    auc = roc_auc(scores.detach().cpu().numpy().reshape(-1), np.array([0, 1, 0, 1]))
    assert np.isfinite(auc)


def test_command_line_trains_at_part_len_9(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "Train", "temporal_transformer_shanghaitech.py"), "--synthetic", "--part_len", "9",
           "--batch_size", "4", "--MHA_layerNorm", "--FFN_layerNorm", "--relative_position_encoding", "--steps", "3",
           "--log_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(x) for x in re.findall(r"\]: loss (\S+),", r.stdout + r.stderr)]
    assert len(losses) >= 1, (r.stdout + r.stderr)[-2000:]
    assert all(math.isfinite(x) for x in losses), losses
