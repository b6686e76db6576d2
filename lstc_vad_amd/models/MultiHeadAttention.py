"""Drop-in for the reference ``models/MultiHeadAttention.py`` (class surfaces: ``ScaledDotProductAttention`` :9-23,
``MultiHeadAttention`` :28-30, forward :93-132).

Parameters keep the reference names (``w_qs/w_ks/w_vs/fc`` bias-free ``nn.Linear`` holders, ``layer_norm``,
``relative_position_bias_table`` + buffer ``relative_position_index``) so published checkpoints load; the
arithmetic runs in ``MHAFunction`` (GEMM -> fused attention core -> GEMM epilogue -> LayerNorm kernels).
"""
import torch
from torch import nn

from ..functional import (GatherRowsFunction, MHAClsAssocFunction, MHAClsFunction, MHACrossFunction, MHAFunction, PackedAct, SDPAFunction,
                          attn_mask_arg, dropout_apply, next_seed)


def relative_position_index_3d(window_depth: int, window_size: int) -> torch.Tensor:
    """int64 [L*ws^2, L*ws^2]: token t = (d, h, w) row-major over (depth, height, width);
    entry = (dd+L-1)(2ws-1)^2 + (dh+ws-1)(2ws-1) + (dw+ws-1) — same table the reference registers (:56-73)."""
    n = window_depth * window_size * window_size
    t = torch.arange(n)
    dd = (t // (window_size * window_size)).view(-1, 1) - (t // (window_size * window_size)).view(1, -1)
    dh = ((t // window_size) % window_size).view(-1, 1) - ((t // window_size) % window_size).view(1, -1)
    dw = (t % window_size).view(-1, 1) - (t % window_size).view(1, -1)
    span = 2 * window_size - 1
    return ((dd + window_depth - 1) * span * span + (dh + window_size - 1) * span + (dw + window_size - 1)).long()


def key_padding_mask(key_lengths, S, mask=None):
    """bool [N, 1, 1, S]: key j of sequence n is kept while j < key_lengths[n] (clamped to [1, S]); and-ed with ``mask`` (anything
    that broadcasts against [N, H, S, S], zero = masked) when one is given.  Plain torch on the tensor's own device, no host sync."""
    kl = key_lengths.to(torch.int64).clamp(1, S)
    m = (torch.arange(S, device=kl.device)[None, :] < kl[:, None]).view(-1, 1, 1, S)
    if mask is None:
        return m
    mask = (mask != 0).to(kl.device)
    return m & mask.reshape((1,) * (4 - mask.dim()) + tuple(mask.shape))


def relative_position_index_2d(window_size: int) -> torch.Tensor:
    """2-D variant (:79-89): entry = (dh+ws-1)(2ws-1) + (dw+ws-1)."""
    t = torch.arange(window_size * window_size)
    dh = (t // window_size).view(-1, 1) - (t // window_size).view(1, -1)
    dw = (t % window_size).view(-1, 1) - (t % window_size).view(1, -1)
    span = 2 * window_size - 1
    return ((dh + window_size - 1) * span + (dw + window_size - 1)).long()


class ScaledDotProductAttention(nn.Module):
    """The reference's scaled dot-product attention (:9-23) on the rectangular HIP kernels (csrc/attention_x.hip):
    q [b, H, len_q, d_k], k [b, H, len_k, d_k], v [b, H, len_k, d_v], len_q and len_k independent (1..512 each), no relative bias.
    ``dropout`` is the rate holder (state-less); the mask comes from the HIP RNG."""

    def __init__(self, temperature, attn_dropout=0.1):
        super().__init__()
        self.temperature = temperature
        self.dropout = nn.Dropout(attn_dropout)

    def forward(self, q, k, v, mask=None, relative_pe=False, window_size=4):
        """Returns ``(output [b, H, len_q, d_v], attn [b, H, len_q, len_k])``.  ``mask``: anything torch broadcasts against
        [b, H, len_q, len_k], any dtype, zero = masked (:19-20).  ``attn`` is the softmax in ``eval()`` and the dropped, rescaled
        probabilities in training (:21 returns ``dropout(softmax(...))``); it carries no gradient.  ``relative_pe`` and
        ``window_size`` are accepted and unused, as upstream."""
        if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise ValueError(f"expected [b, H, len, d] tensors, got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        if k.shape[3] != q.shape[3]:
            raise ValueError(f"d_k of q ({q.shape[3]}) and k ({k.shape[3]}) differ")
        if v.shape[2] != k.shape[2]:
            raise ValueError(f"len_k ({k.shape[2]}) and len_v ({v.shape[2]}) differ")
        if not (q.is_cuda and k.is_cuda and v.is_cuda):
            raise RuntimeError("lstc_vad_amd: tensor is not on a HIP device; the hot path is HIP-only (no CPU fallback)")
        if mask is not None:
            mask = attn_mask_arg(mask, q.shape[0], q.shape[1], q.shape[2], device=q.device, Sk=k.shape[2])
        p = self.dropout.p if self.training else 0.0
        seed = next_seed() if p > 0 else 0
        out, probs = SDPAFunction.apply(q, k, v, mask, 1.0 / self.temperature, p, seed)
        if p > 0:
            return out, dropout_apply(probs, p, seed)
        return out, probs


class MultiHeadAttention(nn.Module):
    def __init__(self, n_head, d_model, d_k, d_v, layerNorm=False,
                 attn_dropout=0.1, fc_dropout=0.1, relative_pe=False, window_size=3,
                 window_depth=3, conv_patch=False, relative_pe_2D=False):
        super().__init__()
        self.n_head, self.d_k, self.d_v, self.d_model = n_head, d_k, d_v, d_model
        self.layerNorm_flag = layerNorm
        self.w_qs = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_ks = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_vs = nn.Linear(d_model, n_head * d_v, bias=False)
        self.fc = nn.Linear(n_head * d_v, d_model, bias=False)
        self.dropout = nn.Dropout(fc_dropout)            # rate holders (state-less); masks come from the HIP RNG
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-6)
        self.temperature = d_k ** 0.5
        self.attn_dropout = nn.Dropout(attn_dropout)
        self.relative_pe, self.relative_pe_2D = relative_pe, relative_pe_2D
        self.window_size, self.window_depth = window_size, window_depth
        if relative_pe:
            rows = (2 * window_depth - 1) * (2 * window_size - 1) ** 2
            self.relative_position_bias_table = nn.Parameter(torch.zeros(rows, n_head))
            self.register_buffer("relative_position_index", relative_position_index_3d(window_depth, window_size))
            nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        if relative_pe_2D:
            self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, n_head))
            self.register_buffer("relative_position_index", relative_position_index_2d(window_size))
            nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        self._site = ""
        self._act16_out = False        # bf16 activation stream: hand the result on as a PackedAct (set per call by Encoder)
        self.cls_assoc = True          # last-layer CLS attention without materialising K / V (see functional)

    def fuse_qkv_(self):
        """Re-home w_qs / w_ks / w_vs as consecutive row blocks of ONE [2*H*dk + H*dv, d_model] buffer (the Parameters,
        their names and values are unchanged; only ``.data`` is re-pointed).  MHAFunction then runs one projection GEMM
        instead of three (X is read once), one weight-gradient GEMM and one input-gradient GEMM.  Call after the module
        sits on its final device; ``load_state_dict`` / the optimizer keep working (they update ``.data`` in place)."""
        ws = [self.w_qs.weight, self.w_ks.weight, self.w_vs.weight]
        flat = torch.empty((sum(w.shape[0] for w in ws), ws[0].shape[1]), device=ws[0].device, dtype=ws[0].dtype)
        off = 0
        with torch.no_grad():
            for w in ws:
                flat[off: off + w.shape[0]].copy_(w.data)
                w.data = flat[off: off + w.shape[0]]
                off += w.shape[0]
        return self

    def _cls_assoc_ok(self, S):
        return self.d_model % 4 == 0 and self.n_head <= 16 and S <= 128 and self.n_head * self.d_model <= 16384 and self.cls_assoc

    def cls_takes_pack(self, N, S):
        """Can ``forward_cls`` read its input as a PackedAct (functional.cls_pack_ok: lstc_cls_dot_pack and friends)?"""
        from ..functional import cls_pack_ok
        return self._cls_assoc_ok(S) and cls_pack_ok(N, S, self.n_head, self.d_model)

    def forward_cls(self, x, mask=None, key_lengths=None, seqs=None):
        """CLS-query attention for the last encoder layer: x [N, S, d] -> [N, d] (== ``forward(x, x, x, mask)[0][:, 0]``).
        ``seqs``: an unpadded batch (functional.SeqLayout), x [1, M, d] -> [N, d], the CLS row of every sequence: the re-associated
        form over sequence offsets (lstc_cls_dot_var ...) where ``_cls_assoc_ok`` holds, else the whole block on the M rows and a
        gather of its CLS rows (correct, slower; no kernel of its own).  No mask, no key lengths, f32 activations.
        ``mask`` as in ``forward``; only its query row 0 is read.
        ``key_lengths``: int32 [N] on the device, the keys of each sequence of a padded batch (the CLS token counted, 1..S; the
        kernels clamp): keys beyond them do not exist.  Alone, and where the re-associated form applies (``_cls_assoc_ok``), it
        runs that form with lstc_cls_dot_len - no K / V projection of the padded batch; with a ``mask`` as well, or S > 128, the
        K/V-projecting form takes the key-padding mask of the lengths, and-ed with ``mask``."""
        cfg = dict(n_head=self.n_head, d_k=self.d_k, d_v=self.d_v, layer_norm=self.layerNorm_flag,
                   attn_dropout=self.attn_dropout.p, fc_dropout=self.dropout.p, training=self.training,
                   site=self._site)
        if seqs is not None:
            if mask is not None or key_lengths is not None or isinstance(x, PackedAct):
                raise NotImplementedError("an unpadded batch takes no mask, no key lengths and f32 activations")
            if not self._cls_assoc_ok(seqs.S_max):
                full = self.forward(x, x, x, seqs=seqs)[0]
                return GatherRowsFunction.apply(full.view(seqs.M, -1), seqs.on(x.device, self.n_head)["row0_64"])
            cfg.update(seqs=seqs)
            fn = MHAClsAssocFunction
        elif key_lengths is not None:
            if isinstance(x, PackedAct):
                raise NotImplementedError("key lengths need the f32 activations (Encoder keeps the bf16 stream off when lengths are given)")
            if mask is None and self._cls_assoc_ok(x.shape[1]):
                cfg.update(key_lengths=key_lengths)
                fn = MHAClsAssocFunction
            else:
                cfg.update(mask=attn_mask_arg(key_padding_mask(key_lengths, x.shape[1], mask), x.shape[0], self.n_head, x.shape[1],
                                              device=x.device))
                fn = MHAClsFunction
        elif mask is not None:
            # the re-associated form does its softmax inside lstc_cls_dot and stays unmasked: the K/V-projecting form takes the mask
            if isinstance(x, PackedAct):
                raise NotImplementedError("an attention mask needs the f32 activations (Encoder keeps the bf16 stream off when one is given)")
            cfg.update(mask=attn_mask_arg(mask, x.shape[0], self.n_head, x.shape[1], device=x.device))
            fn = MHAClsFunction
        elif isinstance(x, PackedAct):       # bf16 activation stream: Encoder checked cls_takes_pack(); the pack's bf16 view goes through autograd
            cfg.update(act_shape=x.shape)
            fn, x = MHAClsAssocFunction, x.t
        else:
            # re-associated form (no K/V projection GEMMs) whenever its alignment rules hold, else the K/V-projecting form
            fn = MHAClsAssocFunction if self._cls_assoc_ok(x.shape[1]) else MHAClsFunction
        return fn.apply(x, self.w_qs.weight, self.w_ks.weight, self.w_vs.weight, self.fc.weight,
                                    self.layer_norm.weight if self.layerNorm_flag else None,
                                    self.layer_norm.bias if self.layerNorm_flag else None,
                                    self.relative_position_bias_table if (self.relative_pe or self.relative_pe_2D) else None,
                                    cfg)

    def forward(self, q, k, v, mask=None, return_attn=False, return_attn_v=False, seqs=None):
        """``mask``: anything torch broadcasts against [N, H, S, S], any dtype, zero = masked (reference :105-106: the logit of a
        masked position is -1e9 before the relative bias and the softmax; a fully masked row comes out uniform).
        ``seqs``: an unpadded batch (functional.SeqLayout): q [1, M, d] holds the tokens of all sequences back to back and the
        attention core runs over the sequence offsets (lstc_attn_var_fwd / _bwd); everything else is row-wise and runs as it does
        on M rows.  No mask, no returned probabilities (they are ragged), f32 activations; the caller (Encoder) has checked the
        lengths against the relative index."""
        if not (q is k and k is v):
            raise NotImplementedError("only self-attention (q is k is v) here: three different inputs, with lengths of their own, "
                                      "go through forward_cross")
        has_bias = self.relative_pe or self.relative_pe_2D
        if seqs is not None:
            if mask is not None or return_attn or return_attn_v or isinstance(q, PackedAct):
                raise NotImplementedError("an unpadded batch takes no mask, returns no probabilities and needs f32 activations")
        elif self.relative_pe_2D and q.shape[1] - 1 != self.window_size ** 2:
            raise RuntimeError("relative_pe_2D needs window_size**2 patch tokens (models/MultiHeadAttention.py:114)")
        cfg = dict(n_head=self.n_head, d_k=self.d_k, d_v=self.d_v, layer_norm=self.layerNorm_flag,
                   attn_dropout=self.attn_dropout.p, fc_dropout=self.dropout.p, training=self.training,
                   site=self._site)
        if seqs is not None:
            cfg.update(seqs=seqs)
        act = isinstance(q, PackedAct)
        if mask is not None:
            if act:
                raise NotImplementedError("an attention mask needs the f32 activations (Encoder keeps the bf16 stream off when one is given)")
            cfg.update(mask=attn_mask_arg(mask, q.shape[0], self.n_head, q.shape[1], device=q.device))
        if act:        # bf16 activation stream (functional.PackedAct): the pack's bf16 view goes through autograd, the shape rides in cfg
            if return_attn_v:
                raise NotImplementedError("return_attn_v needs the f32 activations (Encoder keeps them when it is asked for)")
            cfg.update(act_shape=q.shape, act16_out=self._act16_out)
            shape, q = q.shape, q.t
        out, probs = MHAFunction.apply(
            q, self.w_qs.weight, self.w_ks.weight, self.w_vs.weight, self.fc.weight,
            self.layer_norm.weight if self.layerNorm_flag else None,
            self.layer_norm.bias if self.layerNorm_flag else None,
            self.relative_position_bias_table if has_bias else None,
            self.relative_position_index if has_bias else None, cfg)
        if act and self._act16_out:
            out = PackedAct(out, shape)
        if return_attn_v:
            N, S = q.shape[0], q.shape[1]
            from ..functional import gemm
            vv = gemm(q.contiguous().view(N * S, -1), self.w_vs.weight, trans_b=True)
            return out, probs, vv.view(N, S, self.n_head, self.d_v).transpose(1, 2)
        if not return_attn:
            return out, None
        return out, probs

    def forward_cross(self, q, k, v, mask=None, return_attn=False, return_attn_v=False):
        """Cross-attention, the reference's ``forward`` for three different inputs (:93-132): q [N, len_q, d_model], k and v
        [N, len_k, d_model]; the residual is the query input.  Returns ``forward``'s tuple: ``(out [N, len_q, d_model], attn)`` with
        ``attn`` [N, H, len_q, len_k] the probabilities before dropout (None unless asked for), and with ``return_attn_v`` a third
        value [N, H, len_k, d_v], the projection of the key-side input ``v``.
        ``mask``: anything torch broadcasts against [N, H, len_q, len_k], any dtype, zero = masked.
        len_q == len_k runs the square kernels (relative bias and mask as in ``forward``), len_q != len_k the rectangular ones
        (the few-query kernels for short len_q); passing one tensor as k and v projects it once when the weights are fused.
        ``relative_pe`` / ``relative_pe_2D`` need len_q == len_k: the reference adds its bias slice [:len_q-1, :len_q-1] to
        ``attn[:, :, 1:, 1:]``, which does not broadcast otherwise.  Its one accident, len_q == 2 (a 1 x 1 bias spread over every
        key), is refused like every other unequal pair.  Every refusal is raised before any launch."""
        if any(isinstance(t, PackedAct) for t in (q, k, v)):
            raise NotImplementedError("forward_cross takes f32 activations (no PackedAct inputs)")
        if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
            raise ValueError(f"expected [N, len, d_model] tensors, got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        if not (q.shape[0] == k.shape[0] == v.shape[0]):
            raise ValueError(f"batch sizes differ: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        if not (q.shape[2] == k.shape[2] == v.shape[2] == self.d_model):
            raise ValueError(f"d_model is {self.d_model}: got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
        if k.shape[1] != v.shape[1]:
            raise ValueError(f"len_k ({k.shape[1]}) and len_v ({v.shape[1]}) differ")
        N, len_q, len_k = q.shape[0], q.shape[1], k.shape[1]
        has_bias = self.relative_pe or self.relative_pe_2D
        if has_bias and len_q != len_k:
            raise ValueError(f"the relative position bias needs len_q == len_k (got {len_q} and {len_k}): the reference's bias slice "
                             "does not broadcast over a rectangular attention")
        if self.relative_pe_2D and len_q - 1 != self.window_size ** 2:
            raise RuntimeError("relative_pe_2D needs window_size**2 patch tokens (models/MultiHeadAttention.py:114)")
        if has_bias and len_q - 1 > self.relative_position_index.shape[0]:
            raise ValueError(f"len_q - 1 = {len_q - 1} patch tokens exceed the relative position index "
                             f"({self.relative_position_index.shape[0]} tokens)")
        cfg = dict(n_head=self.n_head, d_k=self.d_k, d_v=self.d_v, layer_norm=self.layerNorm_flag,
                   attn_dropout=self.attn_dropout.p, fc_dropout=self.dropout.p, training=self.training,
                   site=self._site)
        if mask is not None:
            cfg.update(mask=attn_mask_arg(mask, N, self.n_head, len_q, device=q.device, Sk=len_k))
        if not (q.is_cuda and k.is_cuda and v.is_cuda):
            raise RuntimeError("lstc_vad_amd: tensor is not on a HIP device; the hot path is HIP-only (no CPU fallback)")
        out, probs = MHACrossFunction.apply(
            q, k, v, self.w_qs.weight, self.w_ks.weight, self.w_vs.weight, self.fc.weight,
            self.layer_norm.weight if self.layerNorm_flag else None,
            self.layer_norm.bias if self.layerNorm_flag else None,
            self.relative_position_bias_table if has_bias else None,
            self.relative_position_index if has_bias else None, cfg)
        if return_attn_v:
            from ..functional import gemm
            vv = gemm(v.contiguous().view(N * len_k, -1), self.w_vs.weight, trans_b=True)
            return out, probs, vv.view(N, len_k, self.n_head, self.d_v).transpose(1, 2)
        if not return_attn:
            return out, None
        return out, probs
