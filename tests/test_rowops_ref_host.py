"""The float64 references of tests/util_rowops.py, checked before any kernel is checked against them: LayerNorm and the head
against torch.autograd, the loss wrapper against the oracle's own forward_loss pieces on golden cases, Adagrad against
torch.optim.Adagrad, and ``tol`` against its docstring on a hand-made example.  CPU only."""
import pytest
import torch

import util_rowops as R
from oracle import lstc_oracle as orc
from util import load_case

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("rows,d", [(1, 4), (5, 37), (7, 260)])
def test_layernorm_reference_equals_autograd(rows, d):
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x = (3.0 + torch.randn(rows, d, generator=g, dtype=F64)).requires_grad_(True)
    gamma = torch.randn(d, generator=g, dtype=F64).requires_grad_(True)
    beta = torch.randn(d, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(rows, d, generator=g, dtype=F64)
    y = torch.nn.functional.layer_norm(x, (d,), gamma, beta, 1e-6)
    y.backward(dy)
    yr, mean, rstd = R.ln_fwd(x.detach(), gamma.detach(), beta.detach(), 1e-6)
    dx, dg, db = R.ln_bwd(dy, x.detach(), gamma.detach(), mean, rstd)
    assert _rel(yr, y.detach()) < 1e-12
    assert _rel(mean, x.detach().mean(-1)) < 1e-12
    assert _rel(rstd, 1.0 / torch.sqrt(x.detach().var(-1, unbiased=False) + 1e-6)) < 1e-12
    assert _rel(dx, x.grad) < 1e-12
    assert _rel(dg, gamma.grad) < 1e-12 and _rel(db, beta.grad) < 1e-12
    # the float32 restatement is the same function: close, and not the float64 result rounded
    y32, _, _ = R.ln_fwd(x.detach(), gamma.detach(), beta.detach(), 1e-6, dtype=torch.float32)
    assert y32.dtype == torch.float32 and _rel(y32.double(), yr) < 1e-4


def test_layernorm_reference_constant_row():
    """Variance 0: rstd = 1 / sqrt(eps) and y = beta, finite."""
    x = torch.full((2, 8), 2.0, dtype=F64)
    gamma, beta = torch.arange(8, dtype=F64) + 1, torch.arange(8, dtype=F64) - 3
    y, mean, rstd = R.ln_fwd(x, gamma, beta, 1e-6)
    assert torch.equal(y, beta.expand(2, 8)) and torch.equal(mean, torch.full((2,), 2.0, dtype=F64))
    assert _rel(rstd, torch.full((2,), 1e3, dtype=F64)) < 1e-12


@pytest.mark.parametrize("c", [1, 2])
def test_head_reference_equals_autograd(c):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(9, 32, generator=g, dtype=F64).requires_grad_(True)
    W = torch.randn(c, 32, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(c, generator=g, dtype=F64).requires_grad_(True)
    dout = torch.randn(9, c, generator=g, dtype=F64)
    z = torch.nn.functional.linear(x, W, b)
    out = torch.sigmoid(z) if c == 1 else torch.softmax(z, -1)
    out.backward(dout)
    o = R.head_fwd(x.detach(), W.detach(), b.detach())
    dx, dW, db = R.head_bwd(x.detach(), W.detach(), o, dout)
    assert _rel(o, out.detach()) < 1e-12
    assert _rel(dx, x.grad) < 1e-12 and _rel(dW, W.grad) < 1e-12 and _rel(db, b.grad) < 1e-12


def test_cls_concat_reference_equals_autograd():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 6, 5, generator=g, dtype=F64).requires_grad_(True)
    pos, cls = torch.randn(7, 5, generator=g, dtype=F64), torch.randn(5, generator=g, dtype=F64)
    dy = torch.randn(3, 7, 5, generator=g, dtype=F64)
    y = R.cls_concat_fwd(x, pos=pos)
    assert torch.equal(y[:, 1:], x.detach() + pos[1:]) and _rel(y[:, 0].detach(), x.detach().mean(1) + pos[0]) < 1e-12
    y.backward(dy)
    assert _rel(R.cls_concat_bwd(dy, 1), x.grad) < 1e-12
    x.grad = None
    y2 = R.cls_concat_fwd(x, cls=cls)
    assert torch.equal(y2[:, 0].detach(), cls.expand(3, 5))
    y2.backward(dy)
    assert torch.equal(R.cls_concat_bwd(dy, 0), x.grad)
    lo, hi = x.detach()[:1], x.detach()[1:]
    assert torch.equal(R.cls_concat_fwd(lo, x_hi=hi, n_lo=1), R.cls_concat_fwd(x.detach()))


@pytest.mark.parametrize("name", ["ltn_sht", "stn_sht", "stn_mil_ce"])
def test_loss_wrapper_equals_oracle_pieces_on_golden_case(name):
    """The recorded head output of a golden step through ``loss_ref`` against forward_loss's own composition of mil_loss /
    soft_targets / ce_loss / bce_loss (oracle/lstc_oracle.py) on the same output, in float64, and against the five scalars the
    float32 oracle recorded with the fixture."""
    z, mode, _, skw = load_case(name)
    st = orc.StepCfg(mode=mode, **skw)
    bs, pn, L = st.batch_size, st.part_num, st.part_len
    outputs = torch.from_numpy(z["outputs"]).double()
    labs = torch.from_numpy(z["abnorm_labs"])
    if mode == "LTN":
        o = outputs.reshape(2 * bs * pn, 2).requires_grad_(True)
        t = orc.soft_targets(labs, bs, pn, L).reshape(2 * bs * pn, -1).double()
        aux = orc.ce_loss(o, t)
        mil, err, l1 = orc.mil_loss(o[:, 1], bs, pn, 1, st.lambda_1)
        loss = st.lambda_MIL * mil + st.lambda_CE * aux
        got = R.loss_ref(1, outputs, bs, pn, 1, bs, st.lambda_1, st.lambda_MIL, st.lambda_CE, abn_labels=labs, label_len=L)
    elif mode == "STN":
        o = outputs.reshape(2 * bs, pn * L, 1).requires_grad_(True)
        loss, err, l1 = orc.mil_loss(o, bs, pn, L, st.lambda_1)
        mil, aux = loss, torch.zeros((), dtype=F64)
        got = R.loss_ref(0, outputs, bs, pn, L, bs * pn * L, st.lambda_1, 1.0, 0.0)
    else:
        o = outputs.reshape(2 * bs * pn * L, 1).requires_grad_(True)
        t = orc.soft_targets(labs, bs, pn, L).double()
        mil, err, l1 = orc.mil_loss(o, bs, pn, L, st.lambda_1)
        aux = orc.bce_loss(o.reshape(2 * bs, pn, L).mean(-1), t, st.lambda_normal, st.lambda_abnormal)
        loss = st.lambda_BCE * aux + mil
        got = R.loss_ref(2, outputs, bs, pn, L, bs, st.lambda_1, 1.0, st.lambda_BCE, st.lambda_normal, st.lambda_abnormal,
                         abn_labels=labs, label_len=L)
    (dout,) = torch.autograd.grad(loss, o)
    want = torch.stack([loss, mil, err, l1, aux]).detach()
    assert _rel(got[0], want) < 1e-12, (got[0], want)
    assert _rel(got[1].reshape(-1), dout.reshape(-1)) < 1e-12
    assert float((got[0] - torch.from_numpy(z["scalars"]).double()).abs().max()) < 2e-6


def test_loss_sharding_and_margins():
    """shard_rows: the two ranks' rows partition the global rows; loss_margins on a hand-made input."""
    a, b = R.shard_rows(6, 4, 0, 2), R.shard_rows(6, 4, 2, 4)
    assert sorted(torch.cat([a, b]).tolist()) == list(range(48))
    assert a.tolist() == list(range(0, 8)) + list(range(24, 32))
    # bs 1, two parts of one score: bags 0.5 (normal) and 1.25 (abnormal): hinge argument 0.25; gaps 0.3 and 1.0
    out = torch.tensor([[0.5], [0.2], [0.25], [1.25]])
    h, gap = R.loss_margins(0, out, 1, 2, 1)
    assert abs(h - 0.25) < 1e-7 and abs(gap - 0.3) < 1e-7
    # an explicit target list equal to the soft targets gives the same loss
    labs = torch.tensor([[0.25, 1.0]])
    t = orc.soft_targets(labs, 1, 2, 1).reshape(-1, 2)
    s1, g1 = R.loss_ref(2, out * 0.5, 1, 2, 1, 1, 0.01, 1.0, 0.7, 0.2, 2.0, abn_labels=labs)
    s2, g2 = R.loss_ref(2, out * 0.5, 1, 2, 1, 1, 0.01, 1.0, 0.7, 0.2, 2.0, targets=t)
    assert torch.equal(s1, s2) and torch.equal(g1, g2)


def test_adagrad_reference_equals_torch_optim():
    g = torch.Generator().manual_seed(11)
    w0 = torch.randn(37, generator=g, dtype=F64)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.Adagrad([p], lr=1e-2, lr_decay=0, weight_decay=1e-3, initial_accumulator_value=0, eps=1e-10)
    w, s = w0.clone(), torch.zeros_like(w0)
    for _ in range(3):
        grad = torch.randn(37, generator=g, dtype=F64)
        p.grad = grad.clone()
        opt.step()
        w, s = R.adagrad(w, grad, s, 1e-2, 1e-3, 1e-10, 1.0)
        assert _rel(w, p.detach()) < 1e-12
        assert _rel(s, opt.state[p]["sum"]) < 1e-12
    # gscale multiplies the gradient before the weight decay is added
    w1, _ = R.adagrad(w0, grad, torch.zeros_like(w0), 1e-2, 1e-3, 1e-10, 0.37)
    w2, _ = R.adagrad(w0, grad * 0.37, torch.zeros_like(w0), 1e-2, 1e-3, 1e-10, 1.0)
    assert torch.equal(w1, w2)


def test_sqnorm_and_clip_reference_equal_torch():
    g = torch.Generator().manual_seed(12)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=F64)) for n in (1, 5, 300)]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g, dtype=F64)
    grads = [p.grad.clone() for p in ps]
    sq = R.sqnorm(grads)
    for max_norm in (1.0, 1e3):
        for p, g0 in zip(ps, grads):
            p.grad = g0.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(float(total) - float(sq) ** 0.5) < 1e-12 * float(total)
        coef = R.clip_coef(sq, max_norm)
        assert (coef < 1.0) == (max_norm == 1.0)
        for p, g0 in zip(ps, grads):
            assert _rel(g0 * coef, p.grad) < 1e-12


def test_tol_on_hand_made_example():
    """8 * max(e32, 4 * 2**-24 * B)."""
    ref = torch.tensor([1.0, 2.0, 3.0], dtype=F64)
    # e32 = 2**-10 dominates the floor 4 * 2**-24 * 5
    assert R.tol(ref, ref + torch.tensor([0.0, 2.0 ** -10, -(2.0 ** -12)], dtype=F64), torch.tensor([1.0, 5.0, 2.0])) == 8 * 2.0 ** -10
    # an exact restatement: the floor, from the LARGEST element of terms_abs
    assert R.tol(ref, ref.clone(), torch.tensor([1.0, 5.0, 2.0])) == 8 * 4 * 2.0 ** -24 * 5.0
    assert R.tol(ref, ref.float(), 16.0) == 8 * 4 * 2.0 ** -24 * 16.0
    # a float32 restatement is promoted, not the reference rounded: 0.1f - 0.1 = 1.49e-9
    r = torch.tensor([0.1], dtype=F64)
    assert R.tol(r, torch.tensor([0.1], dtype=torch.float32), 0.0) == 8 * abs(float(torch.tensor(0.1, dtype=torch.float32).double()) - 0.1)
