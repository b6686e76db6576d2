"""float64 references of the two kernels of padded (ragged) batches - the length-aware CLS concat (csrc/rowops.hip,
lstc_cls_concat_len_fwd / _bwd) and the re-associated CLS attention with key lengths (csrc/attention.hip, lstc_cls_dot_len) - in
plain torch, with the ``terms_abs`` that tests/util_rowops.tol wants, and the shared recipes of the model-level tests.  No project
kernel is called here: tests/test_ragged_host.py checks these functions against torch.autograd before tests/test_ragged_gpu.py
checks the kernels against them.

A reference never reads the padding of its input (``x[n, L_n:]``, ``X[n, klen_n:]``): a sequence is sliced out first, so the
padding may hold NaN.  Every reference takes a ``dtype``: float64 is the reference proper, float32 the restatement of ``tol``."""
import torch

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------- CLS concat with lengths
def cls_concat_len_fwd(x, lens, cls=None, pos=None, dtype=F64):
    """x [N, S-1, d], lens [N] -> y [N, S, d]: y[n, 0] = ``cls`` or mean(x[n, :L]); y[n, 1 + t] = x[n, t] for t < L; ``pos`` [S, d]
    added on rows 0..L; rows past L are zero.  Differentiable in x (real tokens), cls and pos."""
    N, T, d = x.shape
    rows = []
    for n in range(N):
        L = int(lens[n])
        xs = x[n, :L].to(dtype)
        c0 = cls.to(dtype).reshape(1, d) if cls is not None else xs.sum(0, keepdim=True) / L
        y = torch.cat([c0, xs], 0)
        if pos is not None:
            y = y + pos.to(dtype)[:L + 1]
        rows.append(torch.cat([y, torch.zeros(T - L, d, dtype=dtype)], 0))
    return torch.stack(rows)


def cls_concat_len_terms(x, lens, cls=None, pos=None):
    """terms_abs of y: the same sums over absolute values."""
    ab = lambda t: None if t is None else torch.nan_to_num(t.to(F64)).abs()
    return cls_concat_len_fwd(ab(x), lens, ab(cls), ab(pos))


def cls_concat_len_bwd(dy, lens, mean_cls, dtype=F64):
    """(dx [N, S-1, d], dtok [S, d]): dx[n, t] = dy[n, t + 1] + (mean_cls ? dy[n, 0] / L : 0) for t < L, zero beyond;
    dtok[t] = sum over the sequences with t <= L_n of dy[n, t] (row 0: d cls_token; rows 0..S-1: d pos)."""
    dy = dy.to(dtype)
    N, S, d = dy.shape
    dx = torch.zeros(N, S - 1, d, dtype=dtype)
    dtok = torch.zeros(S, d, dtype=dtype)
    for n in range(N):
        L = int(lens[n])
        dx[n, :L] = dy[n, 1:L + 1] + (dy[n, :1] / L if mean_cls else 0.0)
        dtok[:L + 1] += dy[n, :L + 1]
    return dx, dtok


def cls_concat_len_bwd_terms(dy, lens, mean_cls):
    return cls_concat_len_bwd(dy.to(F64).abs(), lens, mean_cls)


# ------------------------------------------------------------------------------------------- cls_dot with key lengths
def cls_dot_len(U, X, klen, mode, probs=None, keep=None, p_drop=0.0, dtype=F64):
    """lstc_cls_dot_len: U [N, H, d], X [N, S, d], klen [N] (keys per sequence, CLS counted) -> (out [N, H, S], probs).
    mode 0: out = U . X over the keys j < klen, 0 beyond.  mode 1: probs = softmax over j < klen, out = probs * keep / (1 - p),
    both 0 beyond.  mode 2: ``probs`` given, dP = (U . X) * keep / (1 - p), out = P * (dP - sum_j dP P), 0 beyond.
    ``keep`` [N, H, S]: the dropout keep decisions of query row 0 (None: no dropout)."""
    N, S, d = X.shape
    H = U.shape[1]
    out = torch.zeros(N, H, S, dtype=dtype)
    pr = torch.zeros(N, H, S, dtype=dtype) if mode == 1 else probs
    for n in range(N):
        kl = int(klen[n])
        dot = U[n].to(dtype) @ X[n, :kl].to(dtype).t()                      # [H, kl]
        kp = keep[n, :, :kl].to(dtype) / (1.0 - p_drop) if keep is not None and p_drop > 0 else 1.0
        if mode == 0:
            out[n, :, :kl] = dot
        elif mode == 1:
            p = torch.softmax(dot, -1)
            pr[n, :, :kl] = p
            out[n, :, :kl] = p * kp
        else:
            p = probs[n, :, :kl].to(dtype)
            dp = dot * kp
            out[n, :, :kl] = p * (dp - (dp * p).sum(-1, keepdim=True))
    return out, pr


# ------------------------------------------------------------------------------------------- padded batches
def pad_sequences(seqs, t_max=None, fill=float("nan")):
    """list of [L_i, d] -> (x [N, t_max, d] with ``fill`` behind every sequence, lengths)."""
    t_max = t_max or max(s.shape[0] for s in seqs)
    x = torch.full((len(seqs), t_max, seqs[0].shape[1]), fill, dtype=seqs[0].dtype, device=seqs[0].device)
    for n, s in enumerate(seqs):
        x[n, :s.shape[0]] = s
    return x, [int(s.shape[0]) for s in seqs]


def encoder_kw(window_depth, dropout=0.0, **extra):
    """The small encoder of the model-level tests: 3 layers, 2 heads of 16, d_model 32, relative bias over window_depth x 4 x 4."""
    kw = dict(n_layers=3, n_head=2, d_k=16, d_v=16, d_model=32, d_inner=64, MHA_layerNorm=True, FFN_layerNorm=True,
              relative_pe=True, window_size=4, window_depth=window_depth, MHA_attn_dropout=dropout, MHA_fc_dropout=dropout,
              FFN_dropout=dropout, position_dropout=dropout)
    kw.update(extra)
    return kw


def oracle_cfg(kw):
    from oracle import lstc_oracle as orc
    names = set(orc.EncoderCfg.__dataclass_fields__)
    return orc.EncoderCfg(**{k: v for k, v in kw.items() if k in names})


def oracle_encoder_masked(P, x, cfg, mask=None, training=False):
    """oracle.lstc_oracle.encoder_forward with the reference's ``src_mask`` step restated (models/MultiHeadAttention.py:105-106:
    ``attn.masked_fill(mask == 0, -1e9)`` on the scaled logits, before the relative bias) - the oracle itself never passes a mask.
    Everything else is the oracle's own code (``ffn_forward``, the concat and the bias gather are copied from it line by line);
    tests/test_ragged_host.py checks that ``mask=None`` reproduces ``encoder_forward`` bit for bit.  No dropout, no 2-D bias."""
    import torch.nn.functional as F
    from oracle import lstc_oracle as orc
    assert not cfg.relative_pe_2D and not training
    if cfg.input_layerNorm:
        x = F.layer_norm(x, (cfg.d_model,), P["layer_norm.weight"], P["layer_norm.bias"], 1e-6)
    cls = P["cls_token"].expand(x.shape[0], -1, -1) if cfg.CLS_learned else x.mean(dim=1, keepdim=True)
    x = torch.cat([cls, x], dim=1)
    if cfg.position_encoding:
        x = x + P["position_enc"][:, : x.shape[1], :]
    N, S, _ = x.shape
    H, dk, dv = cfg.n_head, cfg.d_k, cfg.d_v
    for i in range(cfg.n_layers):
        pre = f"layer_stack.{i}.slf_attn."
        q = (x @ P[pre + "w_qs.weight"].t()).view(N, S, H, dk).transpose(1, 2)
        k = (x @ P[pre + "w_ks.weight"].t()).view(N, S, H, dk).transpose(1, 2)
        v = (x @ P[pre + "w_vs.weight"].t()).view(N, S, H, dv).transpose(1, 2)
        logits = (q / (dk ** 0.5)) @ k.transpose(2, 3)
        if mask is not None:
            logits = logits.masked_fill(mask == 0, -1e9)
        if cfg.relative_pe:
            idx = P[pre + "relative_position_index"][: S - 1, : S - 1].reshape(-1)
            bias = P[pre + "relative_position_bias_table"][idx].reshape(S - 1, S - 1, H).permute(2, 0, 1)
            logits = torch.cat([logits[:, :, :1, :],
                                torch.cat([logits[:, :, 1:, :1], logits[:, :, 1:, 1:] + bias.unsqueeze(0)], 3)], 2)
        attn = torch.softmax(logits, dim=-1)
        o = (attn @ v).transpose(1, 2).reshape(N, S, H * dv)
        y = o @ P[pre + "fc.weight"].t() + x
        if cfg.MHA_layerNorm:
            y = F.layer_norm(y, (cfg.d_model,), P[pre + "layer_norm.weight"], P[pre + "layer_norm.bias"], 1e-6)
        x = orc.ffn_forward(P, f"layer_stack.{i}.pos_ffn.", y, cfg, False) if cfg.FFN_need else y
    return x
