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

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel_index(S, ld):
    """1-D relative offsets of a ld + 1 token window, [ld, ld] (top-left (S-1) x (S-1) block read): within one row distinct
    columns hit distinct table rows, as for the models' 3-D / 2-D indices."""
    i = torch.arange(ld).view(-1, 1)
    j = torch.arange(ld).view(1, -1)
    return (j - i + ld - 1).long(), 2 * ld - 1


def _reference(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop):
    """float64 restatement: A = (Q scale) K^T + bias; P = softmax(A); O = (P * keep / (1-p)) V; gradients by autograd."""
    qd, kd, vd = (t.double().view(N, S, H, -1).transpose(1, 2).requires_grad_(True) for t in (q, k, v))
    td = table.double().requires_grad_(True) if table is not None else None
    a = torch.matmul(qd * (1.0 / math.sqrt(dk)), kd.transpose(-1, -2))
    if td is not None:
        ix = index[: S - 1, : S - 1].reshape(-1)
        bias = td[ix].view(S - 1, S - 1, H).permute(2, 0, 1)
        a = torch.cat([a[:, :, :1, :], torch.cat([a[:, :, 1:, :1], a[:, :, 1:, 1:] + bias], -1)], 2)
    p = torch.softmax(a, -1)
    pd = p * keep.double() / (1.0 - p_drop) if p_drop > 0 else p
    o = torch.matmul(pd, vd)
    o.backward(do.double().view(N, S, H, dv).transpose(1, 2))
    g = lambda t: t.grad.transpose(1, 2).reshape(N * S, -1)
    return (p.detach(), o.detach().transpose(1, 2).reshape(N * S, H * dv), g(qd), g(kd), g(vd),
            td.grad if td is not None else None)


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
    keep = Fn.dropout_mask((N, H, S, S), p_drop, seed, DEV) if p_drop > 0 else torch.ones((N, H, S, S), device=DEV)
    ref = _reference(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop)
    return (probs, o, dq, dk_, dv_, dtab), ref


SHAPES = [(4, 129, 2, 16), (8, 145, 2, 32), (2, 257, 8, 256), (1, 512, 1, 64)]


@pytest.mark.parametrize("bias,sliced,p_drop", [(False, False, 0.0), (True, False, 0.2), (True, True, 0.0), (True, True, 0.2)])
@pytest.mark.parametrize("shape", SHAPES)
def test_long_attention_matches_float64(shape, bias, sliced, p_drop):
    got, ref = _run(*shape, bias, sliced, p_drop)
    names = ("probs", "O", "dQ", "dK", "dV", "dtable")
    for name, a, b in zip(names, got, ref):
        if b is None:
            assert a is None, name
            continue
        a, b = a.double(), b.to(a.device)
        assert torch.isfinite(a).all(), name
        err = float((a - b).abs().max())
        bar = 1e-6 if name == "probs" else 2e-4 * float(b.abs().max()) + 1e-7
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("shape", [(4, 129, 2, 16), (2, 257, 8, 256)])
def test_long_attention_bf16_products_track_float64(shape):
    got, ref = _run(*shape, True, True, 0.2, bf16=True)
    for name, a, b in zip(("probs", "O", "dQ", "dK", "dV", "dtable"), got, ref):
        a, b = a.double().flatten(), b.to(a.device).flatten()
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
        assert cos > 0.999, (name, cos)


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
    """One LTN step at part_len 9 x 16 patches (S = 145) through TrainStep against the oracle (non-zero bias tables): scores,
    loss and EVERY parameter gradient at the bars of the golden step test (2e-4 of the tensor's maximum).  cls_only=True runs the
    last layer on the S <= 512 instantiation of the CLS-query kernels."""
    from argparse import Namespace
    from lstc_vad_amd import synthetic as syn
    from lstc_vad_amd.engine import TrainStep
    from lstc_vad_amd.models import Classifier, Encoder
    from oracle import lstc_oracle as orc
    torch.manual_seed(0)
    ekw = dict(n_head=2, d_k=16, d_v=16, d_model=32, d_inner=64, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True,
               window_size=4, window_depth=9)
    bs, pn, L, P, d = 2, 3, 9, 16, 32
    args = Namespace(batch_size=bs, part_num=pn, part_len=L, n_patch=P, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8,
                     temporal_only=False, clip_grad=False)
    enc = Encoder(n_layers=3, MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0, weight_init=True, **ekw)
    head = Classifier(d, 0.0)
    with torch.no_grad():      # a non-zero bias table, so its gradient is exercised
        for name, prm in enc.named_parameters():
            if "relative_position_bias_table" in name:
                prm.normal_(0.0, 0.5)
    enc_P = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in enc.state_dict().items()}
    head_P = {k: v.detach().clone().requires_grad_(True) for k, v in head.state_dict().items()}
    nf, _, af, al = (torch.from_numpy(x) for x in syn.training_batch(bs, pn, L, P, d, seed=3, threshold=0.6))
    enc, head = enc.to(DEV).train(), head.to(DEV).train()
    ts = TrainStep(args, "LTN", enc, head, 1e-4, 1e-2, 1e-3, cls_only=cls_only)
    loss, scalars, outputs = ts.forward_loss(nf.to(DEV), af.to(DEV), al.to(DEV))
    ts.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    ecfg = orc.EncoderCfg(n_layers=3, MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0, **ekw)
    st = orc.StepCfg(mode="LTN", batch_size=bs, part_num=pn, part_len=L, n_patch=P, head_dropout=0.0)
    ref = orc.forward_loss(enc_P, head_P, ecfg, st, nf, af, al, training=True)
    ref["loss"].backward()
    assert float((outputs.detach().cpu() - ref["outputs"].detach().reshape(outputs.shape)).abs().max()) < 1e-4
    assert abs(float(scalars[0]) - float(ref["loss"].detach())) < 2e-5
    n = 0
    for mod, refp in ((enc, enc_P), (head, head_P)):
        for k, p in mod.named_parameters():
            g = refp[k].grad
            if g is None:
                assert p.grad is None, k
                continue
            tol = 2e-4 * float(g.abs().max()) + 1e-7
            assert float((p.grad.cpu() - g).abs().max()) < tol, (k, float((p.grad.cpu() - g).abs().max()), tol)
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
