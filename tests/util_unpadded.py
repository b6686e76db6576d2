"""float64 references of the kernels of unpadded batches (include/lstc_hip.h: lstc_attn_var_fwd / _bwd, lstc_cls_concat_var_fwd /
_bwd, lstc_cls_dot_var / _wsum_var / _outer_var) in plain torch, every one built sequence by sequence on references the suite
already has (util_mask.attn_reference_masked with mask=None, util_ragged.cls_concat_len_* and cls_dot_len on a batch of one), and
the shared recipes of the tests.  No project kernel is called here: tests/test_unpadded_host.py checks these functions against
torch.autograd on each sequence alone before tests/test_unpadded_gpu.py checks the kernels against them.

Layout (functional.SeqLayout): sequence n has L_n patch tokens and S_n = L_n + 1 tokens; x [sum L_n, d] and the activations
[M, d], M = sum S_n, hold the sequences back to back; the probabilities are one flat buffer, sequence n's [H, S_n, S_n] block at
prob0[n]."""
import torch

import util_ragged as R
from util_mask import attn_reference_masked

F64, F32 = torch.float64, torch.float32

# the smallest set that crosses every 32-token tile edge of S (2 .. 128) and both softmax lane groups, in an unsorted order
LENGTHS = [63, 1, 127, 15, 32, 96, 2, 64, 31, 95]


def offsets(lens, H):
    """(in0, row0, prob0), each N + 1 long, straight from the definition."""
    in0, row0, prob0 = [0], [0], [0]
    for L in lens:
        in0.append(in0[-1] + L)
        row0.append(row0[-1] + L + 1)
        prob0.append(prob0[-1] + H * (L + 1) * (L + 1))
    return in0, row0, prob0


# ------------------------------------------------------------------------------------------- CLS concat
def concat_var_fwd(x, lens, cls=None, pos=None, dtype=F64):
    """x [sum L, d] -> y [M, d]: per sequence util_ragged.cls_concat_len_fwd on a batch of one without padding."""
    in0, _, _ = offsets(lens, 1)
    return torch.cat([R.cls_concat_len_fwd(x[in0[n]:in0[n + 1]][None], [L], cls, None if pos is None else pos[:L + 1], dtype)[0]
                      for n, L in enumerate(lens)], 0)


def concat_var_terms(x, lens, cls=None, pos=None):
    ab = lambda t: None if t is None else t.to(F64).abs()
    return concat_var_fwd(ab(x), lens, ab(cls), ab(pos))


def concat_var_bwd(dy, lens, mean_cls, dtype=F64):
    """dy [M, d] -> (dx [sum L, d], dtok [S_max, d]); dtok sums the sequences that have the token, in sequence order."""
    _, row0, _ = offsets(lens, 1)
    S_max = max(lens) + 1
    dxs, dtok = [], torch.zeros(S_max, dy.shape[1], dtype=dtype)
    for n, L in enumerate(lens):
        dx, tk = R.cls_concat_len_bwd(dy[row0[n]:row0[n + 1]][None], [L], mean_cls, dtype)
        dxs.append(dx[0])
        dtok[:L + 1] += tk
    return torch.cat(dxs, 0), dtok


def concat_var_bwd_terms(dy, lens, mean_cls):
    return concat_var_bwd(dy.to(F64).abs(), lens, mean_cls)


# ------------------------------------------------------------------------------------------- attention over offsets
def attn_var_reference(q, k, v, do, lens, H, dk, dv, table, index, keep, p_drop):
    """q, k [M, >= H*dk], v, do [M, >= H*dv] (the first H*d columns count), ``keep`` the flat ragged keep mask or None ->
    (P flat ragged, O [M, H*dv], dQ, dK, dV, dtable): util_mask.attn_reference_masked on every sequence alone, the table
    gradient summed over the sequences."""
    _, row0, prob0 = offsets(lens, H)
    P, outs, dtable = [], [[] for _ in range(4)], None
    for n, L in enumerate(lens):
        S, r = L + 1, slice(row0[n], row0[n + 1])
        kp = keep[prob0[n]:prob0[n + 1]].view(1, H, S, S) if keep is not None else None
        p, o, dq, dk_, dv_, dt = attn_reference_masked(q[r, :H * dk], k[r, :H * dk], v[r, :H * dv], None if do is None else do[r, :H * dv],
                                                        1, S, H, dk, dv, table, index, kp, p_drop, None)
        P.append(p.reshape(-1))
        for lst, t in zip(outs, (o, dq, dk_, dv_)):
            lst.append(t)
        if dt is not None:
            dtable = dt if dtable is None else dtable + dt
    cat = lambda lst: None if lst[0] is None else torch.cat(lst, 0)
    return torch.cat(P), cat(outs[0]), cat(outs[1]), cat(outs[2]), cat(outs[3]), dtable


# ------------------------------------------------------------------------------------------- the three CLS passes
def _padded(X2, lens):
    _, row0, _ = offsets(lens, 1)
    return R.pad_sequences([X2[row0[n]:row0[n + 1]] for n in range(len(lens))], max(lens) + 1, fill=0.0)[0]


def cls_dot_var(U, X2, lens, mode, probs=None, keep=None, p_drop=0.0, dtype=F64):
    """U [N, H, d], X2 [M, d] -> (out [N, H, S_max], probs): util_ragged.cls_dot_len with every sequence's own S_n keys."""
    return R.cls_dot_len(U, _padded(X2, lens), [L + 1 for L in lens], mode, probs, keep, p_drop, dtype)


def cls_wsum_var(W, X2, lens, dtype=F64):
    """Y[n, h] = sum_{j < S_n} W[n, h, j] X_n[j]."""
    _, row0, _ = offsets(lens, 1)
    return torch.stack([W[n, :, :L + 1].to(dtype) @ X2[row0[n]:row0[n + 1]].to(dtype) for n, L in enumerate(lens)])


def cls_outer_var(W1, U1, W2, U2, add0, lens, dtype=F64):
    """dX [M, d]: rows of sequence n = W1[n, :, :S_n]^T U1[n] + W2[n, :, :S_n]^T U2[n], ``add0[n]`` added to its row 0."""
    rows = []
    for n, L in enumerate(lens):
        r = W1[n, :, :L + 1].to(dtype).t() @ U1[n].to(dtype) + W2[n, :, :L + 1].to(dtype).t() @ U2[n].to(dtype)
        if add0 is not None:
            r = torch.cat([r[:1] + add0[n].to(dtype), r[1:]], 0)
        rows.append(r)
    return torch.cat(rows, 0)
