"""float64 references of the row-wise, head, loss and optimizer kernels (csrc/rowops.hip, csrc/loss.hip) in plain torch,
and the one tolerance rule the tests of those kernels use.  No project kernel is called here: tests/test_rowops_ref_host.py
checks these functions against torch.autograd / torch.optim / the oracle before tests/test_rowops_f64_gpu.py checks the
kernels against them.

Every reference takes a ``dtype``: float64 is the reference proper, float32 is the "f32 restatement" of ``tol`` - the same
formulas evaluated with plain torch float32 ops on the same inputs."""
import torch

from oracle import lstc_oracle as orc

F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -24          # unit roundoff of float32


# ------------------------------------------------------------------------------------------- tolerance
def tol(ref64, f32_restatement, terms_abs):
    """The tolerance of ONE output tensor: ``8 * max(e32, floor)`` (a Python float), where

    * ``e32 = max |f32_restatement - ref64|``: what a plain torch float32 evaluation of the same formulas loses on this input;
    * ``floor = 4 * 2**-24 * B``, ``B`` the largest element of ``terms_abs``: per output element, the sum of the absolute values
      of the terms added into that element, computed in float64 (a tensor shaped like the output, or one number).

    A factor of 8 is three bits over a float32 evaluation of the same thing; the floor keeps an input on which torch's own
    summation order happens to be exact from demanding the same luck of the kernel."""
    ref64 = torch.as_tensor(ref64, dtype=F64)
    e32 = float((torch.as_tensor(f32_restatement).to(F64) - ref64).abs().max()) if ref64.numel() else 0.0
    B = float(torch.as_tensor(terms_abs, dtype=F64).abs().max())
    return 8.0 * max(e32, 4.0 * EPS32 * B)


# ------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, gamma, beta, eps, dtype=F64):
    """Biased variance, eps inside the sqrt, two-pass statistics.  Returns (y, mean, rstd)."""
    x, g, b = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    d = x.shape[-1]
    mean = x.sum(-1) / d
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1) / d + eps)
    return xc * rstd[:, None] * g + b, mean, rstd


def ln_fwd_terms(x, gamma, beta, eps):
    """terms_abs of (y, mean, rstd).  y = x*rs*g - mu*rs*g + b: x and mu are both ADDED into the element (for a row far from
    zero they cancel, and float32 keeps only ulp(|x|) of the difference).  rstd = (var + eps)**-0.5 moves by
    rstd**3 / 2 per unit of var, and var = mean((x - mu)**2) by 2 |x - mu| per unit of (x - mu): its terms are
    rstd**3 * mean(|x - mu| * (|x| + |mu|)), plus rstd itself for its own rounding."""
    _, mean, rstd = ln_fwd(x, gamma, beta, eps)
    x, g, b = x.to(F64), gamma.to(F64), beta.to(F64)
    a = x.abs() + mean.abs()[:, None]
    ty = a * rstd[:, None] * g.abs() + b.abs()
    tm = x.abs().mean(-1)
    tr = rstd ** 3 * ((x - mean[:, None]).abs() * a).mean(-1) + rstd
    return ty, tm, tr


def ln_bwd(dy, x, gamma, mean, rstd, dtype=F64):
    """dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)); dgamma = sum_rows dy xhat; dbeta = sum_rows dy.  ``mean`` / ``rstd``
    are given: the kernel's saved ones (promoted) when the backward is checked alone, ``ln_fwd``'s own otherwise."""
    dy, x, g, mean, rstd = (t.to(dtype) for t in (dy, x, gamma, mean, rstd))
    d = x.shape[-1]
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = dy * g
    m1 = gd.sum(-1, keepdim=True) / d
    m2 = (gd * xh).sum(-1, keepdim=True) / d
    dx = rstd[:, None] * (gd - m1 - xh * m2)
    return dx, (dy * xh).sum(0), dy.sum(0)


def ln_bwd_terms(dy, x, gamma, mean, rstd):
    """terms_abs of (dx, dgamma, dbeta).  With a = (|x| + |mu|) rstd, the sum of the two terms of xhat:
    dx: rstd (|g dy| + mean|g dy| + |xhat| mean|g dy xhat|) for the three terms as written, plus what the cancellation in xhat
    feeds back, rstd (a |m2| + |xhat| mean(|g dy| a)); dgamma: sum_rows |dy| a; dbeta: sum_rows |dy|."""
    dy, x, g, mean, rstd = (t.to(F64) for t in (dy, x, gamma, mean, rstd))
    rs = rstd[:, None]
    xh = (x - mean[:, None]) * rs
    a = (x.abs() + mean.abs()[:, None]) * rs
    gd = dy * g
    M1 = gd.abs().mean(-1, keepdim=True)
    M2 = (gd * xh).abs().mean(-1, keepdim=True)
    m2 = (gd * xh).mean(-1, keepdim=True)
    tdx = rs * (gd.abs() + M1 + xh.abs() * M2) + rs * (a * m2.abs() + xh.abs() * (gd.abs() * a).mean(-1, keepdim=True))
    return tdx, (dy.abs() * a).sum(0), dy.abs().sum(0)


# ------------------------------------------------------------------------------------------- column sums
def colsum(x, dtype=F64):
    return x.to(dtype).sum(0)


def colsum_terms(x):
    return x.to(F64).abs().sum(0)


# ------------------------------------------------------------------------------------------- CLS concat
def cls_concat_fwd(x, cls=None, pos=None, x_hi=None, n_lo=0, dtype=F64):
    """x [N or n_lo.., S-1, d] -> y [N, S, d]: token 0 = ``cls`` or the mean over the tokens, ``pos`` [S, d] added to every
    sequence.  With ``x_hi``: sequences [0, n_lo) come from ``x``, the rest from ``x_hi`` (the fused torch.cat)."""
    xs = x.to(dtype) if x_hi is None else torch.cat([x[:n_lo].to(dtype), x_hi.to(dtype)], 0)
    N, T, d = xs.shape
    c0 = cls.to(dtype).expand(N, d) if cls is not None else xs.sum(1) / T
    y = torch.cat([c0[:, None, :], xs], 1)
    return y + pos.to(dtype) if pos is not None else y


def cls_concat_terms(x, cls=None, pos=None, x_hi=None, n_lo=0):
    """terms_abs of y: the same sums over absolute values."""
    ab = lambda t: None if t is None else t.to(F64).abs()
    return cls_concat_fwd(ab(x), ab(cls), ab(pos), ab(x_hi), n_lo)


def cls_concat_bwd(dy, mean_cls, dtype=F64):
    """dx[n, t] = dy[n, t + 1] + (mean_cls ? dy[n, 0] / (S - 1) : 0)."""
    dy = dy.to(dtype)
    dx = dy[:, 1:, :]
    return dx + dy[:, :1, :] / (dy.shape[1] - 1) if mean_cls else dx.clone()


# ------------------------------------------------------------------------------------------- head output
def head_fwd(x, W, b, dtype=F64):
    """out = sigmoid(x W^T + b) for c = 1 (W [1, 32]), softmax for c = 2."""
    z = x.to(dtype) @ W.to(dtype).t() + b.to(dtype)
    return torch.sigmoid(z) if W.shape[0] == 1 else torch.softmax(z, -1)


def head_bwd(x, W, out, dout, dtype=F64):
    """(dx, dW, db) from d(out); ``out`` is the forward's result (sigmoid: dz = dout o (1 - o); softmax: dz = o (dout - <dout, o>))."""
    x, W, o, g = (t.to(dtype) for t in (x, W, out, dout))
    dz = g * o * (1 - o) if W.shape[0] == 1 else o * (g - (g * o).sum(-1, keepdim=True))
    return dz @ W, dz.t() @ x, dz.sum(0)


def head_terms(x, W, b, dout):
    """terms_abs of (out, dx, dW, db).  out: the activation's slope is at most 1, so the logit's terms sum |x_i W_i| + |b| bound
    it (plus 1 for the output's own rounding).  The backward through dz: |dz_c| and the effect on dz of an ulp of ``out`` are
    both bounded by G = sum_c |dout_c| per row (o, 1 - o <= 1), so dx: G sum_c |W_c|; dW: sum_rows G |x|; db: sum_rows G."""
    x, W, b, g = (t.to(F64) for t in (x, W, b, dout))
    to = x.abs() @ W.abs().t() + b.abs() + 1.0
    G = g.abs().sum(-1, keepdim=True)
    return to, G * W.abs().sum(0), (G * x.abs()).sum(0).expand(W.shape[0], -1), G.sum().expand(W.shape[0])


# ------------------------------------------------------------------------------------------- loss
def shard_rows(bs_global, rpv, rank_off, bs_local):
    """Global score-row indices of a rank's videos, in the rank's local order: its normal videos [rank_off, rank_off + bs_local),
    then its abnormal ones (global numbering: all normal videos first), ``rpv`` rows per video."""
    nor = torch.arange(rank_off * rpv, (rank_off + bs_local) * rpv)
    return torch.cat([nor, bs_global * rpv + nor])


def loss_ref(mode, out, bs, part_num, score_len, l1_skip, lambda_1, lambda_MIL, lambda_aux, lambda_normal=0.0,
             lambda_abnormal=0.0, abn_labels=None, label_len=1, targets=None, dtype=F64):
    """The GLOBAL loss of lstc_vad_loss (include/lstc_hip.h) from the oracle's own pieces, with autograd for d(loss)/d(out).

    mode 0: MIL only; 1: MIL on out[:, 1] + CE on the two-column ``out``; 2: MIL + weighted BCE on the part means.  ``out`` is
    [2 bs part_num score_len, c].  The soft targets are ``targets`` ([rows, 2], as given) or the oracle's ``soft_targets`` of
    ``abn_labels`` (which averages in float32, as the reference does); neither: no auxiliary term.  Added to the oracle: only the
    flat-slice rule of the sparsity term - l1 = mean of the flat score vector from element ``l1_skip`` on (the reference's
    ``y_pred[batch_size:]`` on whatever shape the caller had: bs for a flat vector, bs * part_num * score_len for [2bs, ...]).
    Returns (scalars [loss, mil, err, l1, aux], dout), both ``dtype``."""
    c = 2 if mode == 1 else 1
    o = out.detach().to(dtype).reshape(-1, c).requires_grad_(True)
    score = o[:, c - 1]
    _, err, _ = orc.mil_loss(score, bs, part_num, score_len, lambda_1)
    l1 = score[l1_skip:].mean()
    mil = err + lambda_1 * l1
    aux = torch.zeros((), dtype=dtype)
    if mode != 0 and (targets is not None or abn_labels is not None):
        if targets is not None:
            t = targets.to(dtype).reshape(2 * bs, part_num, 2)
        else:
            t = orc.soft_targets(abn_labels, bs, part_num, label_len).to(dtype)
        if mode == 1:
            aux = orc.ce_loss(o, t.reshape(-1, 2))
        else:
            aux = orc.bce_loss(score.reshape(2 * bs, part_num, score_len).mean(-1), t, lambda_normal, lambda_abnormal)
    loss = lambda_MIL * mil + lambda_aux * aux
    (dout,) = torch.autograd.grad(loss, o)
    return torch.stack([loss, mil, err, l1, aux]).detach(), dout.detach()


def loss_margins(mode, out, bs, part_num, score_len):
    """(smallest |hinge argument 1 - abn_j + nor_i|, smallest gap between a video's two largest part means), float64: how far
    the input is from the loss's two discontinuities (inf for the gap when part_num == 1)."""
    c = 2 if mode == 1 else 1
    pm = out.to(F64).reshape(-1, c)[:, c - 1].reshape(2 * bs, part_num, score_len).mean(-1)
    bag = pm.max(-1)[0]
    hinge = (1.0 - bag[bs:][None, :] + bag[:bs][:, None]).abs().min()
    top = pm.topk(2, -1)[0] if part_num > 1 else None
    return float(hinge), float((top[:, 0] - top[:, 1]).min()) if top is not None else float("inf")


def loss_terms(mode, out, bs, part_num, score_len, l1_skip, lambda_1, lambda_MIL, lambda_aux, lambda_normal=0.0,
               lambda_abnormal=0.0, abn_labels=None, label_len=1, targets=None):
    """terms_abs of (scalars [5], dout).  err: every active pair adds 1, -abn, nor (over bs**2); l1: mean |score|; aux: CE adds
    t_c p_c and t_c lse per row, BCE lambda t |log| per part; loss and mil: the same weights on those sums.  dout: |d err|, the
    constant lambda_1 / n and the two terms of the auxiliary gradient (CE: tsum softmax(p) and t; BCE: lambda_n t0 / a and
    lambda_a t1 / b), weighted as in the loss."""
    c = 2 if mode == 1 else 1
    kw = dict(lambda_normal=lambda_normal, lambda_abnormal=lambda_abnormal, abn_labels=abn_labels, label_len=label_len, targets=targets)
    o = out.to(F64).reshape(-1, c)
    score = o[:, c - 1]
    n = score.numel()
    bag = score.reshape(2 * bs, part_num, score_len).mean(-1).max(-1)[0]
    nor, abn = bag[:bs][:, None], bag[bs:][None, :]
    act = (1.0 - abn + nor) > 0
    t_err = ((1.0 + abn.abs() + nor.abs()) * act).sum() / bs ** 2
    t_l1 = score[l1_skip:].abs().mean()
    _, g_err = loss_ref(mode, out, bs, part_num, score_len, l1_skip, 0.0, 1.0, 0.0, **kw)      # d err / d out alone
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
            pm = score.reshape(2 * bs, part_num, score_len).mean(-1)
            a, b = 1 - pm + 1e-8, pm + 1e-8
            t_aux = (lambda_normal * t[..., 0].abs() * a.log().abs() + lambda_abnormal * t[..., 1].abs() * b.log().abs()).mean()
            gp = (lambda_normal * t[..., 0].abs() / a + lambda_abnormal * t[..., 1].abs() / b) / pm.numel() / score_len
            t_dout += lambda_aux * gp[..., None].expand(-1, -1, score_len).reshape(-1, 1)
    t_mil = t_err + abs(lambda_1) * t_l1
    return torch.stack([lambda_MIL * t_mil + lambda_aux * t_aux, t_mil, t_err, t_l1, t_aux]), t_dout


# ------------------------------------------------------------------------------------------- optimizer
def adagrad(w, grad, state, lr, weight_decay, eps, gscale, dtype=F64):
    """g = grad gscale + wd w; s += g**2; w -= lr g / (sqrt(s) + eps).  Returns (w, state) after the step."""
    w, grad, state = w.to(dtype), grad.to(dtype), state.to(dtype)
    g = grad * gscale + weight_decay * w
    s = state + g * g
    return w - lr * g / (s.sqrt() + eps), s


def adagrad_terms(w, grad, state, lr, weight_decay, eps, gscale):
    """terms_abs of (w, state): |w| + |update| and s + g**2 with g's own two terms taken by absolute value."""
    w, grad, state = w.to(F64), grad.to(F64), state.to(F64)
    ga = grad.abs() * abs(gscale) + weight_decay * w.abs()
    s = state + ga * ga
    return w.abs() + lr * ga / (s.sqrt() + eps), s


def sqnorm(xs, dtype=F64):
    """sum over the tensors of sum(x**2)."""
    return sum((x.to(dtype) ** 2).sum() for x in xs)


def clip_coef(total_sq, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient: min(1, max_norm / (sqrt(total_sq) + 1e-6))."""
    return min(1.0, float(max_norm) / (float(total_sq) ** 0.5 + 1e-6))
