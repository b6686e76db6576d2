"""float64 reference of the top-k MIL loss (include/lstc_hip.h, LstcLossDesc.topk) in plain torch: ``util_rowops.loss_ref``
with the bag of a video replaced by the mean of the first k entries of its part means sorted (value descending, part index
ascending - a stable descending sort).  The reference project never computes top-k (its ``--topk`` is parsed and unused), so
there is no golden: this restatement is the yardstick, tests/test_topk_host.py checks it against ``torch.topk`` + autograd
and against ``loss_ref`` at k = 1, and tests/test_topk_gpu.py checks the kernel against it under ``util_rowops.tol``.

The hinge is restated here (``oracle.mil_loss`` takes the maximum itself); CE, BCE and the soft targets are the oracle's."""
import torch

from oracle import lstc_oracle as orc
from util_rowops import EPS32, F32, F64, tol          # noqa: F401  (re-exported: the tests take the one rule from here)


def part_means(score, bs, part_num, score_len):
    """pm [2 bs, part_num] of the flat score vector."""
    return score.reshape(2 * bs, part_num, score_len).mean(-1)


def topk_select(pm, k):
    """(values, part indices) [2 bs, k] of the selected set: the first k parts in the order (pm descending, index ascending)."""
    vals, idx = torch.sort(pm, dim=-1, descending=True, stable=True)
    return vals[:, :k], idx[:, :k]


def loss_graph(o, mode, bs, part_num, score_len, l1_skip, k, lambda_1, lambda_MIL, lambda_aux, lambda_normal=0.0,
               lambda_abnormal=0.0, abn_labels=None, label_len=1, targets=None):
    """(loss, mil, err, l1, aux) of the head output ``o`` [2 bs part_num score_len, c] as differentiable scalars in ``o``'s
    dtype: what ``loss_ref_topk`` differentiates, and what a test hangs behind an oracle forward pass."""
    c = 2 if mode == 1 else 1
    dtype = o.dtype
    score = o.reshape(-1, c)[:, c - 1]
    pm = part_means(score, bs, part_num, score_len)
    bag = topk_select(pm, k)[0].sum(-1) / k
    nor, abn = bag[:bs], bag[bs:]
    err = torch.relu(1.0 - abn[None, :] + nor[:, None]).sum() / float(bs) ** 2
    l1 = score[l1_skip:].mean()
    mil = err + lambda_1 * l1
    aux = torch.zeros((), dtype=dtype)
    if mode != 0 and (targets is not None or abn_labels is not None):
        if targets is not None:
            t = targets.to(dtype).reshape(2 * bs, part_num, 2)
        else:
            t = orc.soft_targets(abn_labels, bs, part_num, label_len).to(dtype)
        if mode == 1:
            aux = orc.ce_loss(o.reshape(-1, 2), t.reshape(-1, 2))
        else:
            # its own mean node, as in loss_ref: at k = 1 autograd then adds the same terms in the same order, bit for bit
            aux = orc.bce_loss(part_means(score, bs, part_num, score_len), t, lambda_normal, lambda_abnormal)
    return lambda_MIL * mil + lambda_aux * aux, mil, err, l1, aux


def loss_ref_topk(mode, out, bs, part_num, score_len, l1_skip, k, lambda_1, lambda_MIL, lambda_aux, lambda_normal=0.0,
                  lambda_abnormal=0.0, abn_labels=None, label_len=1, targets=None, dtype=F64):
    """``util_rowops.loss_ref`` with top-k bags.  Returns (scalars [loss, mil, err, l1, aux], dout), both ``dtype``
    (float64: the reference proper; float32: the f32 restatement of ``tol``)."""
    c = 2 if mode == 1 else 1
    o = out.detach().to(dtype).reshape(-1, c).requires_grad_(True)
    sc = loss_graph(o, mode, bs, part_num, score_len, l1_skip, k, lambda_1, lambda_MIL, lambda_aux, lambda_normal,
                    lambda_abnormal, abn_labels, label_len, targets)
    (dout,) = torch.autograd.grad(sc[0], o)
    return torch.stack([s.to(dtype) for s in sc]).detach(), dout.detach()


def loss_margins_topk(mode, out, bs, part_num, score_len, k):
    """(smallest |hinge argument 1 - abn_j + nor_i|, smallest gap between a video's k-th and (k+1)-th largest part mean), float64:
    how far the input is from the loss's two discontinuities (inf for the gap at k = part_num: every part is selected)."""
    c = 2 if mode == 1 else 1
    pm = part_means(out.to(F64).reshape(-1, c)[:, c - 1], bs, part_num, score_len)
    srt = torch.sort(pm, dim=-1, descending=True, stable=True)[0]
    bag = srt[:, :k].sum(-1) / k
    hinge = (1.0 - bag[bs:][None, :] + bag[:bs][:, None]).abs().min()
    gap = float((srt[:, k - 1] - srt[:, k]).min()) if k < part_num else float("inf")
    return float(hinge), gap


def loss_terms_topk(mode, out, bs, part_num, score_len, l1_skip, k, lambda_1, lambda_MIL, lambda_aux, lambda_normal=0.0,
                    lambda_abnormal=0.0, abn_labels=None, label_len=1, targets=None):
    """terms_abs of (scalars [5], dout) for ``tol``: ``util_rowops.loss_terms`` with top-k bags.  err: every active pair adds 1,
    -abn, nor (over bs**2), a bag counted as the mean of the |selected part means| (the terms summed into it); l1, aux and the
    auxiliary part of dout as in ``loss_terms``; the hinge part of dout is |d err / d out| of this reference."""
    c = 2 if mode == 1 else 1
    kw = dict(lambda_normal=lambda_normal, lambda_abnormal=lambda_abnormal, abn_labels=abn_labels, label_len=label_len, targets=targets)
    o = out.to(F64).reshape(-1, c)
    score = o[:, c - 1]
    n = score.numel()
    pm = part_means(score, bs, part_num, score_len)
    sel = topk_select(pm, k)[0]
    bag, bag_abs = sel.sum(-1) / k, sel.abs().sum(-1) / k
    act = (1.0 - bag[bs:][None, :] + bag[:bs][:, None]) > 0
    t_err = ((1.0 + bag_abs[bs:][None, :] + bag_abs[:bs][:, None]) * act).sum() / bs ** 2
    t_l1 = score[l1_skip:].abs().mean()
    _, g_err = loss_ref_topk(mode, out, bs, part_num, score_len, l1_skip, k, 0.0, 1.0, 0.0, **kw)      # d err / d out alone
    t_dout = lambda_MIL * g_err.abs()
    t_dout[l1_skip:, c - 1] += lambda_MIL * lambda_1 / (n - l1_skip)
    t_aux = torch.zeros((), dtype=F64)
    if mode != 0 and (targets is not None or abn_labels is not None):
        t = (targets.to(F64).reshape(2 * bs, part_num, 2) if targets is not None
             else orc.soft_targets(abn_labels, bs, part_num, label_len).to(F64))
        if mode == 1:
            t2 = t.reshape(-1, 2).abs()
            lse = torch.logsumexp(o, -1, keepdim=True)
            t_aux = (t2 * (o.abs() + lse.abs())).sum(-1).mean()
            t_dout += lambda_aux * (t2.sum(-1, keepdim=True) * torch.softmax(o, -1) + t2) / o.shape[0]
        else:
            a, b = 1 - pm + 1e-8, pm + 1e-8
            t_aux = (lambda_normal * t[..., 0].abs() * a.log().abs() + lambda_abnormal * t[..., 1].abs() * b.log().abs()).mean()
            gp = (lambda_normal * t[..., 0].abs() / a + lambda_abnormal * t[..., 1].abs() / b) / pm.numel() / score_len
            t_dout += lambda_aux * gp[..., None].expand(-1, -1, score_len).reshape(-1, 1)
    t_mil = t_err + abs(lambda_1) * t_l1
    return torch.stack([lambda_MIL * t_mil + lambda_aux * t_aux, t_mil, t_err, t_l1, t_aux]), t_dout
