"""Drop-in for the reference ``models/Encoder.py`` (:4-74)."""
import torch
from torch import nn

from ..functional import (ClsConcatFunction, ClsConcatLenFunction, ClsConcatSpanFunction, ClsConcatVarFunction, DropoutFunction,
                          LayerNormFunction, PackedAct, UNPADDED_MAX_TOKENS, act_chain_ok, drop_producer_packs, lengths_arg, span_starts,
                          unpadded_layout)
from .EncoderLayer import EncoderLayer
from .MultiHeadAttention import key_padding_mask


class Encoder(nn.Module):
    def __init__(self, n_layers, n_head, d_k, d_v, d_model, d_inner,
                 MHA_attn_dropout=0.1, MHA_fc_dropout=0.1, MHA_layerNorm=False,
                 FFN_dropout=0.1, FFN_layerNorm=True,
                 weight_init=True, CLS_learned=False, position_dropout=0.1, position_encoding=False,
                 max_position_tokens=100, relative_pe=False, window_size=4, window_depth=3, conv_patch=False,
                 input_layerNorm=False, relative_pe_2D=False, FFN_need=True):
        super().__init__()
        self.CLS_learned = CLS_learned
        if CLS_learned:
            self.cls_token = nn.Parameter(torch.randn(1, 1, d_model))
        self.position_encoding = position_encoding
        if position_encoding:
            self.position_dropout = nn.Dropout(position_dropout)
            self.position_enc = nn.Parameter(torch.randn(1, max_position_tokens, d_model))
        self.layer_stack = nn.ModuleList([
            EncoderLayer(d_model, d_inner, n_head, d_k, d_v, MHA_attn_dropout=MHA_attn_dropout,
                         MHA_fc_dropout=MHA_fc_dropout, MHA_layerNorm=MHA_layerNorm, FFN_dropout=FFN_dropout,
                         FFN_layerNorm=FFN_layerNorm, relative_pe=relative_pe, window_size=window_size,
                         window_depth=window_depth, conv_patch=conv_patch, relative_pe_2D=relative_pe_2D,
                         FFN_need=FFN_need)
            for _ in range(n_layers)])
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-6)
        self.input_layerNorm = input_layerNorm
        for i, layer in enumerate(self.layer_stack):      # dropout-site names = reference module paths
            layer.slf_attn._site = f"layer_stack.{i}.slf_attn."
            layer.pos_ffn._site = f"layer_stack.{i}.pos_ffn."
        if weight_init:
            self._reset_parameters()

    def _reset_parameters(self):
        # xavier-uniform on every parameter with dim > 1, bias table / cls / pos-enc included (reference :38-41)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def used_parameters(self):
        """Parameters that receive a gradient for this configuration.  The reference creates LayerNorms it
        never calls (``layer_norm`` unless input_layerNorm, ``slf_attn.layer_norm`` unless MHA_layerNorm, ...);
        Adagrad skips them (grad is None) and so must the gradient all-reduce (SURVEY 7 'Unused parameters')."""
        skip = set()
        if not self.input_layerNorm:
            skip.update(id(p) for p in self.layer_norm.parameters())
        for layer in self.layer_stack:
            if not layer.slf_attn.layerNorm_flag:
                skip.update(id(p) for p in layer.slf_attn.layer_norm.parameters())
            if not layer.FFN_need:
                skip.update(id(p) for p in layer.pos_ffn.parameters())
            elif not layer.pos_ffn.layerNorm_flag:
                skip.update(id(p) for p in layer.pos_ffn.layer_norm.parameters())
        return [p for p in self.parameters() if id(p) not in skip]

    @staticmethod
    def _gather_spec(x):
        """``x`` = (bank [clips, P, d], clip_idx int64 [N * Lc] on the device, N, Lc): sequences still to be gathered out of an
        HBM-resident feature bank (engine.TrainStep on a feed.LazyRows batch) -> (N, S - 1, d)."""
        bank, idx, N, Lc = x[:4]
        return N, Lc * bank.shape[1], bank.shape[2]

    def _act_chain(self, enc_output, enc_output_hi, layers) -> bool:
        """bf16 mode: do ``layers`` (the full encoder layers of this call) run on the bf16 activation stream?  Only when nothing in
        front of them needs a gradient or an f32 copy (no input LayerNorm, learned CLS token or position table) and every block
        qualifies (functional.act_chain_ok)."""
        if self.input_layerNorm or self.CLS_learned or self.position_encoding:
            return False
        if not self.training:
            # evaluation keeps f32 activations between the blocks: whether the stream applies depends on the launch's
            # row count (whole 256-row pack tiles), and scoring.py batches by pool, by video or by rank shard - a video's score,
            # hence pseudo-label thresholds and AUC-based checkpoint selection, must not depend on what shares its launch
            return False
        if isinstance(enc_output, tuple):
            N, Sm1, d = self._gather_spec(enc_output)
            return act_chain_ok(N, Sm1 + 1, d, layers)
        if enc_output.requires_grad or enc_output.dtype != torch.float32 or not enc_output.is_cuda or enc_output.dim() != 3:
            return False
        N = enc_output.shape[0] + (enc_output_hi.shape[0] if enc_output_hi is not None else 0)
        return act_chain_ok(N, enc_output.shape[1] + 1, enc_output.shape[2], layers)

    def _embed(self, enc_output, enc_output_hi=None, pack_only=False):
        if isinstance(enc_output, tuple):
            # batch formation fused into the CLS concat (lstc_cls_concat_gather_fwd): the gathered batch is never written
            # an optional fifth entry, the feed.LazyRows behind ``idx``, travels on to the concat (layer 0 on distinct rows)
            bank, idx, N, Lc = enc_output[:4]
            if self.input_layerNorm:
                raise RuntimeError("Encoder: a gather spec cannot feed the input LayerNorm (materialise the batch first)")
            out = ClsConcatFunction.apply(bank, self.cls_token if self.CLS_learned else None,
                                          self.position_enc if self.position_encoding else None, None, pack_only, (idx, N, Lc) + tuple(enc_output[4:5]))
            if pack_only:
                return PackedAct(out, (N, Lc * bank.shape[1] + 1, bank.shape[2]))
            if self.position_encoding and self.training and self.position_dropout.p > 0:
                out = DropoutFunction.apply(out, self.position_dropout.p, "position_dropout")
            return out
        if pack_only:
            N = enc_output.shape[0] + (enc_output_hi.shape[0] if enc_output_hi is not None else 0)
            t = ClsConcatFunction.apply(enc_output, None, None, enc_output_hi, True)
            return PackedAct(t, (N, enc_output.shape[1] + 1, enc_output.shape[2]))
        if self.input_layerNorm:
            if enc_output_hi is not None:
                enc_output, enc_output_hi = torch.cat([enc_output, enc_output_hi], 0), None
            enc_output = LayerNormFunction.apply(enc_output, self.layer_norm.weight, self.layer_norm.bias)
        enc_output = ClsConcatFunction.apply(enc_output, self.cls_token if self.CLS_learned else None,
                                             self.position_enc if self.position_encoding else None, enc_output_hi)
        if self.position_encoding and self.training and self.position_dropout.p > 0:
            enc_output = DropoutFunction.apply(enc_output, self.position_dropout.p, "position_dropout")
        return enc_output

    def _lengths(self, enc_output, enc_output_hi, lengths):
        """A padded batch: refuse what does not take lengths, check them -> (lens int32 [N] on the input's device, kept-keys mask
        [N, 1, 1, S]).  Every refusal is raised before any launch (and before the input's device matters)."""
        if isinstance(enc_output, PackedAct):
            raise NotImplementedError("Encoder: lengths need f32 activations (no PackedAct input)")
        if isinstance(enc_output, tuple):
            raise ValueError("Encoder: a gather spec cannot carry lengths (materialise the padded batch first)")
        if enc_output_hi is not None:
            raise ValueError("Encoder: lengths describe one padded batch: concatenate enc_output and enc_output_hi first")
        if enc_output.dim() != 3:
            raise ValueError(f"Encoder: lengths need a padded batch [N, S - 1, d_model], got {tuple(enc_output.shape)}")
        N, S = enc_output.shape[0], enc_output.shape[1] + 1
        lens, host = lengths_arg(lengths, N, S, enc_output.device)
        attn0 = self.layer_stack[0].slf_attn
        if attn0.relative_pe_2D:
            # the 2-D bias needs exactly window_size**2 patch tokens per sequence: only a batch without padding qualifies
            if host is None or any(v != attn0.window_size ** 2 for v in host):
                raise ValueError("Encoder: relative_pe_2D needs window_size**2 patch tokens in every sequence - lengths must be given "
                                 f"on the host and all equal {attn0.window_size ** 2}")
        if not enc_output.is_cuda:
            raise RuntimeError("lstc_vad_amd: tensor is not on a HIP device; the hot path is HIP-only (no CPU fallback)")
        return lens, key_padding_mask(lens + 1, S)

    def _embed_len(self, enc_output, lens, kept):
        """``_embed`` of a padded batch: the input LayerNorm sees the padding as zeros (its rows come out as beta and the concat drops
        them), the CLS concat reads the real tokens only and leaves exact zeros behind them."""
        if self.input_layerNorm:
            enc_output = torch.where(kept[:, 0, 0, 1:, None], enc_output, enc_output.new_zeros(()))
            enc_output = LayerNormFunction.apply(enc_output, self.layer_norm.weight, self.layer_norm.bias)
        enc_output = ClsConcatLenFunction.apply(enc_output, self.cls_token if self.CLS_learned else None,
                                                self.position_enc if self.position_encoding else None, lens)
        if self.position_encoding and self.training and self.position_dropout.p > 0:
            enc_output = DropoutFunction.apply(enc_output, self.position_dropout.p, "position_dropout")
        return enc_output

    def _forward_cls_len(self, enc_output, src_mask, lens, kept):
        enc_output = self._embed_len(enc_output, lens, kept)
        mask = kept if src_mask is None else key_padding_mask(lens + 1, enc_output.shape[1], src_mask)
        n = len(self.layer_stack)
        for i, layer in enumerate(self.layer_stack[:-1]):
            layer.pos_ffn._emit_pack = i + 1 < n - 1
            layer.slf_attn._act16_out = layer.pos_ffn._act16_out = False
            enc_output = layer(enc_output, slf_attn_mask=mask)[0]
        out = self.layer_stack[-1].forward_cls(enc_output, slf_attn_mask=src_mask, key_lengths=lens + 1)
        drop_producer_packs()
        return out

    def forward_cls(self, enc_output, enc_output_hi=None, src_mask=None, lengths=None):
        """``forward(x, src_mask)[:, 0, :]`` without computing the rows nobody reads: the train / eval loops consume only the
        CLS token of the last layer (Train/temporal_transformer_shanghaitech.py:123,
        Train/spatio_transformer_shanghaitech.py:97), so the last layer evaluates its query, output projection and
        FFN for that token alone (K/V still use every token).  Saves ~25 % of the step's FLOPs at 3 layers.
        ``lengths``: a padded batch, as in ``forward``; row n is what ``forward_cls(x[n:n+1, :lengths[n]])`` returns."""
        if lengths is not None:
            lens, kept = self._lengths(enc_output, enc_output_hi, lengths)
            return self._forward_cls_len(enc_output, src_mask, lens, kept)
        # enc_output_hi: optional second half of the batch (the abnormal sequences) so the caller need not cat
        # src_mask: the full layers get the mask, the CLS-only last layer its query row 0; the bf16 activation stream stays off
        n = len(self.layer_stack)
        act = src_mask is None and self._act_chain(enc_output, enc_output_hi, list(self.layer_stack[:-1]))
        enc_output = self._embed(enc_output, enc_output_hi, pack_only=act)
        # the CLS-only layer reads the stream's pack too when its re-associated form applies (lstc_cls_dot_pack ...), else f32 rows
        cls_pack = act and isinstance(enc_output, PackedAct) and \
            self.layer_stack[-1].slf_attn.cls_takes_pack(enc_output.shape[0], enc_output.shape[1])
        for i, layer in enumerate(self.layer_stack[:-1]):
            layer.pos_ffn._emit_pack = i + 1 < n - 1          # f32 activations: the CLS-only last layer reads no packed operand
            # bf16 activation stream: every block hands a pack on
            layer.slf_attn._act16_out, layer.pos_ffn._act16_out = act, act and (i + 1 < n - 1 or cls_pack)
            enc_output = layer(enc_output, slf_attn_mask=src_mask)[0]
        out = self.layer_stack[-1].forward_cls(enc_output, slf_attn_mask=src_mask)
        drop_producer_packs()
        return out

    def _unpadded(self, x, lengths, enc_output_hi=None, src_mask=None, return_attn=False, return_attn_v=False,
                  max_tokens=UNPADDED_MAX_TOKENS):
        """An unpadded batch: refuse what the route does not take and check the lengths -> functional.SeqLayout.  Every refusal is
        raised before any launch, and before the input's device matters."""
        if src_mask is not None or return_attn or return_attn_v:
            raise NotImplementedError("Encoder: the unpadded route takes no src_mask and returns no attention probabilities "
                                      "(they are ragged); use forward(x, lengths=...) on a padded batch")
        if isinstance(x, PackedAct):
            raise NotImplementedError("Encoder: an unpadded batch needs f32 activations (no PackedAct input)")
        if isinstance(x, tuple):
            raise ValueError("Encoder: a gather spec cannot feed the unpadded route (materialise the tokens first)")
        if enc_output_hi is not None:
            raise ValueError("Encoder: an unpadded batch is one matrix: concatenate enc_output and enc_output_hi first")
        if x.dim() != 2:
            raise ValueError(f"Encoder: an unpadded batch is [sum of lengths, d_model], got {tuple(x.shape)}")
        lay = unpadded_layout(lengths, max_tokens)
        if lay.in0[-1] != x.shape[0]:
            raise ValueError(f"Encoder: the lengths sum to {lay.in0[-1]} tokens, the input has {x.shape[0]} rows")
        self._layout_fits(lay)
        if not x.is_cuda:
            raise RuntimeError("lstc_vad_amd: tensor is not on a HIP device; the hot path is HIP-only (no CPU fallback)")
        return lay

    def _layout_fits(self, lay):
        """ValueError where a sequence of the unpadded layout ``lay`` is beyond what the attention bias or the position table hold."""
        attn0 = self.layer_stack[0].slf_attn
        if attn0.relative_pe_2D and any(v != attn0.window_size ** 2 for v in lay.lengths):
            raise ValueError(f"Encoder: relative_pe_2D needs window_size**2 = {attn0.window_size ** 2} patch tokens in every sequence")
        if (attn0.relative_pe or attn0.relative_pe_2D) and lay.S_max - 1 > attn0.relative_position_index.shape[0]:
            raise ValueError(f"Encoder: {lay.S_max - 1} patch tokens exceed the relative position index "
                             f"({attn0.relative_position_index.shape[0]} tokens)")
        if self.position_encoding and lay.S_max > self.position_enc.shape[1]:
            raise ValueError(f"Encoder: {lay.S_max} tokens exceed max_position_tokens = {self.position_enc.shape[1]}")
        if lay.S_max > UNPADDED_MAX_TOKENS and (attn0.d_k % 16 or attn0.d_v % 16):
            raise ValueError(f"Encoder: a sequence above {UNPADDED_MAX_TOKENS} tokens needs d_k and d_v multiples of 16 (the key-tiled "
                             f"attention kernels), got d_k = {attn0.d_k}, d_v = {attn0.d_v}")

    def _embed_unpadded(self, x, lay):
        """``_embed`` of an unpadded batch -> [1, M, d_model]: the input LayerNorm is row-wise, the concat knows the offsets."""
        if self.input_layerNorm:
            x = LayerNormFunction.apply(x, self.layer_norm.weight, self.layer_norm.bias)
        x = ClsConcatVarFunction.apply(x, self.cls_token if self.CLS_learned else None,
                                       self.position_enc if self.position_encoding else None, lay)
        if self.position_encoding and self.training and self.position_dropout.p > 0:
            x = DropoutFunction.apply(x, self.position_dropout.p, "position_dropout")
        return x.view(1, lay.M, -1)

    def forward_unpadded(self, enc_output, lengths, src_mask=None, return_attn=False, return_attn_v=False,
                         max_tokens=UNPADDED_MAX_TOKENS):
        """``forward`` of an UNPADDED batch: ``enc_output`` [sum L_n, d_model] holds the patch tokens of N sequences back to back,
        ``lengths`` (a Python sequence or a CPU tensor of N integers; on the host, because the output size depends on their sum)
        their token counts L_n, 1 <= L_n <= 127.  Returns [M, d_model], M = sum (L_n + 1): rows ``row0[n] .. row0[n] + L_n`` (row0 =
        the running sum of L_n + 1) are what ``forward(x_n[None])`` returns for sequence n alone, in ``eval()`` and in training with
        every dropout rate 0.  With dropout on, the counters run over the unpadded rows and the ragged probabilities: a valid draw,
        but not the draw the sequence would have got alone.  The GEMMs, LayerNorm, FFN, dropout and residual run on the M real
        rows; the attention core and the CLS concat run over the sequence offsets (lstc_attn_var_*, lstc_cls_concat_var_*).
        Refused before any launch: ``src_mask``, ``return_attn``, ``return_attn_v`` (NotImplementedError), a gather spec, a
        PackedAct, ``relative_pe_2D`` unless every length is window_size**2, a sequence above 128 tokens, beyond the relative
        index or beyond ``max_position_tokens`` (ValueError).  The bf16 activation stream, packed attention operands and the layer-0
        distinct-rows path are off, as with a mask.
        ``max_tokens`` (default 128, at most 512): the longest sequence the call takes, CLS token included.  Above 128 the
        sequences of more than 128 tokens run on the key-tiled offset kernels (lstc_attn_var_long_*; d_k and d_v multiples of 16,
        else ValueError) and the others where they always ran, so a sequence's result does not depend on its neighbours' lengths."""
        lay = self._unpadded(enc_output, lengths, None, src_mask, return_attn, return_attn_v, max_tokens)
        h = self._embed_unpadded(enc_output, lay)
        for i, layer in enumerate(self.layer_stack):
            layer.pos_ffn._emit_pack = i + 1 < len(self.layer_stack)
            layer.slf_attn._act16_out = layer.pos_ffn._act16_out = False
            h = layer(h, seqs=lay)[0]
        drop_producer_packs()
        return h.view(lay.M, -1)

    def forward_cls_unpadded(self, enc_output, lengths, enc_output_hi=None, src_mask=None, max_tokens=UNPADDED_MAX_TOKENS):
        """``forward_unpadded(x, lengths)[row0[:-1]]`` -> [N, d_model], the CLS row of every sequence, without computing the other
        rows of the last layer: its re-associated form over sequence offsets where it applies (``_cls_assoc_ok``), else the full
        block and a gather of the CLS rows.  Row n is what ``forward_cls(x_n[None])`` returns for sequence n alone; in exact-f32
        ``eval()`` bit for bit.  Arguments and refusals as in ``forward_unpadded``; a batch with a sequence above 128 tokens
        (``max_tokens``) takes the full last block and the gather."""
        lay = self._unpadded(enc_output, lengths, enc_output_hi, src_mask, max_tokens=max_tokens)
        h = self._embed_unpadded(enc_output, lay)
        n = len(self.layer_stack)
        for i, layer in enumerate(self.layer_stack[:-1]):
            layer.pos_ffn._emit_pack = i + 1 < n - 1
            layer.slf_attn._act16_out = layer.pos_ffn._act16_out = False
            h = layer(h, seqs=lay)[0]
        out = self.layer_stack[-1].forward_cls(h, seqs=lay)
        drop_producer_packs()
        return out

    def forward_cls_spans(self, bank, starts, lengths, max_tokens=UNPADDED_MAX_TOKENS):
        """``forward_cls_unpadded`` fed from SPANS of an HBM-resident bank: ``bank`` is [R, d_model] float32 on the device (or
        [clips, P, d_model], viewed as its clips * P rows), sequence n the rows ``starts[n] .. starts[n] + lengths[n] - 1``.  ``starts``
        and ``lengths`` are host integers (Python sequences or CPU tensors); the lengths obey ``forward_cls_unpadded``'s rules.  Spans
        may overlap, repeat and come in any order.  Returns [N, d_model]: row n is what ``forward_cls_unpadded(bank[starts[n] :
        starts[n] + L_n], [L_n])`` returns - in ``eval()`` bit for bit in every compute mode, because only the CLS concat differs
        (lstc_cls_concat_span_fwd) and it writes the same bits; the tokens are never materialised.  The bank takes no gradient; in
        training mode ``cls_token`` and ``position_enc`` get theirs.  Refused before any launch, and before the bank's device
        matters: ``input_layerNorm`` (it would need the tokens materialised), a bank that requires grad, a span outside [0, R], a
        different number of starts and lengths (ValueError), a PackedAct (NotImplementedError)."""
        if isinstance(bank, PackedAct):
            raise NotImplementedError("Encoder: spans need an f32 bank (no PackedAct input)")
        if self.input_layerNorm:
            raise ValueError("Encoder: spans of a bank cannot feed the input LayerNorm (materialise the tokens and use forward_cls_unpadded)")
        if not torch.is_tensor(bank) or bank.dim() not in (2, 3) or bank.dtype != torch.float32:
            raise ValueError("Encoder: spans need a float32 bank [rows, d_model] or [clips, P, d_model], got "
                             f"{tuple(bank.shape) if torch.is_tensor(bank) else type(bank).__name__}")
        if bank.requires_grad:
            raise ValueError("Encoder: a bank takes no gradient (detach it, or materialise the tokens and use forward_cls_unpadded)")
        rows = bank.reshape(-1, bank.shape[-1]) if bank.is_contiguous() else None
        if rows is None:
            raise ValueError("Encoder: spans need a contiguous bank")
        lay = unpadded_layout(lengths, max_tokens)
        src0 = span_starts(starts, lay, rows.shape[0])
        self._layout_fits(lay)
        if not bank.is_cuda:
            raise RuntimeError("lstc_vad_amd: tensor is not on a HIP device; the hot path is HIP-only (no CPU fallback)")
        src0 = torch.tensor(src0, dtype=torch.int64).to(bank.device)
        h = ClsConcatSpanFunction.apply(rows, src0, self.cls_token if self.CLS_learned else None,
                                        self.position_enc if self.position_encoding else None, lay)
        if self.position_encoding and self.training and self.position_dropout.p > 0:
            h = DropoutFunction.apply(h, self.position_dropout.p, "position_dropout")
        h = h.view(1, lay.M, -1)
        n = len(self.layer_stack)
        for i, layer in enumerate(self.layer_stack[:-1]):
            layer.pos_ffn._emit_pack = i + 1 < n - 1
            layer.slf_attn._act16_out = layer.pos_ffn._act16_out = False
            h = layer(h, seqs=lay)[0]
        out = self.layer_stack[-1].forward_cls(h, seqs=lay)
        drop_producer_packs()
        return out

    def forward(self, enc_output, src_mask=None, return_attn=False, return_attn_v=False, lengths=None):
        """``lengths`` (a Python sequence, a CPU tensor or a device tensor of N integers) makes ``enc_output`` [N, S - 1, d_model] a
        PADDED batch: sequence n has ``lengths[n]`` real patch tokens ``x[n, :lengths[n]]`` (1 <= lengths[n] <= S - 1, the CLS token
        not counted) and the rest of its row is padding that is never read (it may hold NaN).  Rows 0..lengths[n] of the result
        are what ``forward(x[n:n+1, :lengths[n]])`` returns, in ``eval()`` and in training with every dropout rate 0; the rows past
        them are finite and otherwise unspecified, the returned probabilities of padded keys are 0 and the input gradient of the
        padding is 0.  With dropout on, element (n, h, i, j) of an attention mask keeps its counter over the padded S (and the
        other sites theirs over the padded rows): a valid draw, but not the draw the sequence would have got alone.
        Lengths on the host are range-checked (ValueError) before any launch; a device tensor costs no host sync and is clamped
        to [1, S - 1] by the kernels.  ``src_mask`` is and-ed with the key padding.  Refused: a gather spec, a PackedAct input,
        ``relative_pe_2D`` unless every length is window_size**2.  The bf16 activation stream is off, as with a mask."""
        attn_list, v_list = [], []
        if lengths is not None:
            lens, kept = self._lengths(enc_output, None, lengths)
            enc_output = self._embed_len(enc_output, lens, kept)
            if src_mask is not None:
                kept = key_padding_mask(lens + 1, enc_output.shape[1], src_mask)
            src_mask, act = kept, False
        else:
            act = not return_attn_v and src_mask is None and self._act_chain(enc_output, None, list(self.layer_stack))
            enc_output = self._embed(enc_output, None, pack_only=act)
        for i, layer in enumerate(self.layer_stack):
            layer.pos_ffn._emit_pack = i + 1 < len(self.layer_stack)      # the last layer's output goes to the caller
            layer.slf_attn._act16_out, layer.pos_ffn._act16_out = act, act and i + 1 < len(self.layer_stack)
            res = layer(enc_output, slf_attn_mask=src_mask, return_attn=return_attn, return_attn_v=return_attn_v)
            enc_output = res[0]
            if return_attn or return_attn_v:
                attn_list.append(res[1])
            if return_attn_v:
                v_list.append(res[2])
        drop_producer_packs()
        if return_attn_v:
            return enc_output, attn_list, v_list
        if return_attn:
            return enc_output, attn_list
        return enc_output
