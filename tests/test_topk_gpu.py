"""The top-k MIL loss on the GPU (csrc/loss.hip, LstcLossDesc.topk; losses / engine: ``args.mil_topk``) against the float64
restatement of tests/util_topk.py, under the one tolerance rule ``util_rowops.tol``; k <= 1 against itself bit for bit; the tie
rule; the rank-sharded form; and the way up through ``training_loss``, ``engine.TrainStep`` and ``engine.GraphedStep``.

The shapes are the smallest that cross an edge of the kernel's top-k branch: one wavefront per video and one part per lane, so
part_num = 3 / 4 (a few lanes), 33 (past half a wave), 64 (every lane); 2 * bs = 260 local videos (65 trips of the four
wavefronts, and the second trip of the 256-thread loops behind them); k = 2, k = part_num, k = 7 of 64, k = 32 of 33."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

import util_rowops as R
import util_topk as T
from oracle import lstc_oracle as orc
from test_rowops_f64_gpu import LAMBDAS, Checks, _loss_inputs, _loss_variant
from util import load_case, max_abs_diff, oracle_cfgs, sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64


def _L():
    from lstc_vad_amd import _lib
    return _lib


def _loss_gpu(mode, out, bs_g, bs_l, rank_off, pn, Ls, l1_skip, phase, bag, topk, abn_labels=None, label_len=1, targets=None,
              lambdas=LAMBDAS):
    """One ``lstc_vad_loss`` launch on device copies of the CPU inputs; (scalars, dout) back on the CPU.  ``dout`` and the
    scalars start as NaN: an element the kernel does not write shows."""
    L = _L()
    d = L.LossDesc()
    d.mode, d.bs_global, d.bs_local, d.rank_off = mode, bs_g, bs_l, rank_off
    d.part_num, d.score_len, d.label_len, d.l1_skip = pn, Ls, label_len, l1_skip
    d.lambda_1, d.lambda_MIL, d.lambda_aux = lambdas["lambda_1"], lambdas["lambda_MIL"], lambdas["lambda_aux"]
    d.lambda_normal, d.lambda_abnormal = lambdas["lambda_normal"], lambdas["lambda_abnormal"]
    od = out.contiguous().to(DEV)
    ld = abn_labels.contiguous().to(DEV) if abn_labels is not None else None
    td = targets.contiguous().to(DEV) if targets is not None else None
    dout = torch.full_like(od, float("nan"))
    sc = torch.full((5,), float("nan"), device=DEV)
    d.out, d.abn_labels, d.targets, d.bag = L.dev_ptr(od), L.dev_ptr(ld), L.dev_ptr(td), L.dev_ptr(bag)
    d.dout, d.scalars, d.phase = L.dev_ptr(dout), L.dev_ptr(sc), phase
    if topk is not None:                    # None: the field is left as LossDesc() zero-initialises it
        d.topk = topk
    L.check(L.load().lstc_vad_loss(C.byref(d), L.stream_ptr()), "lstc_vad_loss")
    torch.cuda.synchronize()
    return sc.cpu(), dout.cpu()


# seeds chosen on the CPU so that, in float64, no hinge argument and no gap between a video's k-th and (k + 1)-th part mean lies
# within 1e-4 of zero (asserted in every test that uses one; the rule of test_rowops_f64_gpu.LOSS_SEEDS):
# (mode, bs, part_num, score_len, k) -> seed
TOPK_SEEDS = {(0, 3, 4, 2, 2): 1, (0, 3, 4, 2, 4): 1, (0, 130, 3, 2, 2): 1, (0, 130, 3, 2, 3): 2, (0, 2, 64, 2, 7): 1, (0, 2, 33, 2, 32): 1,
              (0, 4, 3, 2, 2): 1, (0, 3, 5, 2, 3): 1,
              (1, 3, 4, 1, 2): 1, (1, 3, 4, 1, 4): 1, (1, 130, 3, 1, 2): 2, (1, 130, 3, 1, 3): 1, (1, 2, 64, 1, 7): 1, (1, 2, 33, 1, 32): 1,
              (1, 4, 3, 1, 2): 1, (1, 3, 5, 1, 3): 1,
              (2, 3, 4, 2, 2): 1, (2, 3, 4, 2, 4): 1, (2, 130, 3, 2, 2): 1, (2, 130, 3, 2, 3): 1, (2, 2, 64, 2, 7): 1, (2, 2, 33, 2, 32): 1,
              (2, 4, 3, 2, 2): 1, (2, 3, 5, 2, 3): 1}
SHAPE_KS = [((3, 4), 2), ((3, 4), 4), ((130, 3), 2), ((130, 3), 3), ((2, 64), 7), ((2, 33), 32)]          # ((bs, part_num), k)


def _inputs(mode, bs, pn, Ls, k):
    out, labels, targets = _loss_inputs(mode, bs, pn, Ls, TOPK_SEEDS[(mode, bs, pn, Ls, k)])
    hinge, gap = T.loss_margins_topk(mode, out, bs, pn, Ls, k)
    print("loss margins: hinge %.3e gap between part means %d and %d: %.3e" % (hinge, k, k + 1, gap))
    assert hinge > 1e-4 and gap > 1e-4, ("input too close to a discontinuity of the loss: choose another seed", hinge, gap)
    return out, labels, targets


def _close_all(ck, prefix, sc, dout, ref, f32, terms):
    for i, name in enumerate(("loss", "mil", "err", "l1", "aux")):
        ck.close(prefix + name, sc[i:i + 1], ref[0][i:i + 1], f32[0][i:i + 1], terms[0][i:i + 1])
    if dout is not None:
        ck.close(prefix + "dout", dout, ref[1], f32[1], terms[1])


# ============================================================================================ a. parity with float64
PARITY_CASES = [(m, s, k, v, skip) for m in (0, 1, 2) for s, k in SHAPE_KS
                for v in (("no_aux",) if m == 0 else ("no_aux", "labels_L3")) for skip in ("skip_bs", "skip_normal_half")]


def _parity_id(case):
    m, (bs, pn), k, v, skip = case
    return "mode%d-bs%d_pn%d-k%d-%s-%s" % (m, bs, pn, k, v, skip)


@pytest.mark.parametrize("case", PARITY_CASES, ids=[_parity_id(c) for c in PARITY_CASES])
def test_topk_loss_single_rank_against_float64(case):
    """All five scalars and d(loss)/d(out) of one launch (phase 2) against the float64 top-k loss."""
    mode, (bs, pn), k, variant, skip = case
    Ls = 1 if mode == 1 else 2
    ck = Checks("topk", _parity_id(case))
    out, labels, targets = _inputs(mode, bs, pn, Ls, k)
    l1_skip = bs if skip == "skip_bs" else bs * pn * Ls
    aux = _loss_variant(variant, labels, targets)
    sc, dout = _loss_gpu(mode, out, bs, bs, 0, pn, Ls, l1_skip, 2, None, k, **aux)
    ref = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, **LAMBDAS, **aux)
    f32 = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, dtype=F32, **LAMBDAS, **aux)
    terms = T.loss_terms_topk(mode, out, bs, pn, Ls, l1_skip, k, **LAMBDAS, **aux)
    _close_all(ck, "", sc, dout, ref, f32, terms)
    # the selected set itself: the hinge part of dout is nonzero on exactly k parts of every video that has a gradient
    if variant == "no_aux" and skip == "skip_normal_half":
        c = 2 if mode == 1 else 1
        g = dout[:, c - 1].reshape(2 * bs, pn, Ls)[:bs]                          # normal half: no l1 term there under this skip
        want = ref[1][:, c - 1].reshape(2 * bs, pn, Ls)[:bs] != 0
        ck.true("selected parts of the normal videos", bool(((g != 0) == want).all()))
    ck.done()


# ============================================================================================ b. k = 0 and k = 1
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(3, 4), (130, 3), (2, 64), (2, 33)], ids=lambda s: "bs%d_pn%d" % s)
def test_topk_0_and_1_are_the_same_launch_bit_for_bit(mode, shape):
    """topk = 0 (what a descriptor of a caller built against the previous header holds), the field left untouched, and
    topk = 1 give the same bits, and they are the maximum's: the float64 reference at k = 1 is ``util_rowops.loss_ref``."""
    bs, pn = shape
    Ls = 1 if mode == 1 else 2
    out, labels, _ = _loss_inputs(mode, bs, pn, Ls, 3)
    aux = dict(abn_labels=labels[3], label_len=3) if mode else {}
    runs = [_loss_gpu(mode, out, bs, bs, 0, pn, Ls, bs, 2, None, tk, **aux) for tk in (None, 0, 1)]
    for sc, dout in runs[1:]:
        assert torch.equal(sc, runs[0][0]) and torch.equal(dout, runs[0][1])
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())
    bag0, bag1 = torch.zeros(2 * bs, device=DEV), torch.zeros(2 * bs, device=DEV)
    _loss_gpu(mode, out, bs, bs, 0, pn, Ls, bs, 0, bag0, 0, **aux)
    _loss_gpu(mode, out, bs, bs, 0, pn, Ls, bs, 0, bag1, 1, **aux)
    c = 2 if mode == 1 else 1
    assert torch.equal(bag0, bag1)
    pm32 = out[:, c - 1].reshape(2 * bs, pn, Ls)
    pm32 = (pm32[..., 0] + pm32[..., 1]) / 2 if Ls == 2 else pm32[..., 0] / 1
    assert torch.equal(bag1.cpu(), pm32.max(-1)[0])                               # the maximum of the float32 part means, undivided


# ============================================================================================ c. ties
def test_topk_ties_go_to_the_lower_part_index():
    """One abnormal video whose five parts all hold the same scores, lambda_1 = 0, no auxiliary term, k = 3: its dout is nonzero
    exactly on parts 0, 1, 2, with one value, gbag / (k * score_len).  Scores in [0, 1): every hinge pair is active."""
    bs, pn, Ls, k = 2, 5, 2, 3
    g = torch.Generator().manual_seed(0)
    out = torch.rand(2 * bs * pn * Ls, 1, generator=g)
    tied = bs + 1
    out.view(2 * bs, pn, Ls)[tied] = torch.tensor([0.3, 0.5])
    lam = dict(lambda_1=0.0, lambda_MIL=1.0, lambda_aux=0.0, lambda_normal=0.0, lambda_abnormal=0.0)
    sc, dout = _loss_gpu(0, out, bs, bs, 0, pn, Ls, bs, 2, None, k, lambdas=lam)
    d = dout.view(2 * bs, pn, Ls)
    assert bool((d[tied, :3] == d[tied, 0, 0]).all()) and float(d[tied, 0, 0]) != 0.0
    assert bool((d[tied, 3:] == 0).all())
    assert float(d[tied, 0, 0]) == float(torch.tensor(-bs / bs ** 2, dtype=F32) / (torch.tensor(float(k)) * torch.tensor(float(Ls))))
    # every other video: exactly k selected parts, and the launch agrees with the reference (which breaks ties the same way)
    assert ((d != 0).all(-1).sum(-1) == k).all() and ((d != 0).any(-1).sum(-1) == k).all()
    ref = T.loss_ref_topk(0, out, bs, pn, Ls, bs, k, **lam)
    assert torch.equal(dout != 0, ref[1] != 0)
    assert abs(float(sc[2]) - float(ref[0][2])) < 1e-6


# ============================================================================================ d. sharded
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_topk_sharded_loss_equals_global_loss(mode):
    """Two emulated ranks (the pattern of test_hip_parity.test_sharded_loss_equals_global_loss), bs 4, k = 2: the exchanged bag
    vector is bitwise the one-rank bag vector, the concatenated dout bitwise the one-rank dout, the summed scalars within tol."""
    bs, pn, k = 4, 3, 2
    Ls = 1 if mode == 1 else 2
    rpv, half = pn * Ls, bs // 2
    ck = Checks("topk", "mode%d sharded 2+2" % mode)
    out, labels, _ = _inputs(mode, bs, pn, Ls, k)
    aux = dict(abn_labels=labels[3], label_len=3) if mode else {}
    l1_skip = bs if mode else bs * rpv
    bag1 = torch.zeros(2 * bs, device=DEV)
    s_full, g_full = _loss_gpu(mode, out, bs, bs, 0, pn, Ls, l1_skip, 2, bag1, k, **aux)
    shard = lambda r: (out[R.shard_rows(bs, rpv, r * half, half)], dict(aux, abn_labels=labels[3][r * half:(r + 1) * half]) if mode else {})
    bag = torch.zeros(2 * bs, device=DEV)
    for r in range(2):
        o_r, aux_r = shard(r)
        _loss_gpu(mode, o_r, bs, half, r * half, pn, Ls, l1_skip, 0, bag, k, **aux_r)      # phase 0 fills this rank's slots
    assert torch.equal(bag, bag1)
    tot = torch.zeros(5, dtype=F64)
    dout = torch.full(out.shape, float("nan"))
    for r in range(2):
        o_r, aux_r = shard(r)
        s, g = _loss_gpu(mode, o_r, bs, half, r * half, pn, Ls, l1_skip, 1, bag, k, **aux_r)
        tot += s.to(F64)
        dout[R.shard_rows(bs, rpv, r * half, half)] = g
    assert torch.equal(dout, g_full)
    ref = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, **LAMBDAS, **aux)
    f32 = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, dtype=F32, **LAMBDAS, **aux)
    terms = T.loss_terms_topk(mode, out, bs, pn, Ls, l1_skip, k, **LAMBDAS, **aux)
    _close_all(ck, "sum of ranks ", tot, None, ref, f32, terms)
    _close_all(ck, "one rank ", s_full, g_full, ref, f32, terms)
    ck.done()


# ============================================================================================ e. through training_loss
@pytest.mark.parametrize("tmode,mode", [("LTN", 1), ("STN", 0), ("STN_MIL_CE", 2)])
def test_topk_through_training_loss_and_autograd(tmode, mode):
    """``losses.training_loss`` with ``args.mil_topk = 3``: the gradient autograd hands the head output is the kernel's dout
    (bit for bit, the launch with topk = 3 made by hand), and the scalars match the float64 reference."""
    from lstc_vad_amd.losses import get_MIL_loss, training_loss
    bs, pn, k = 3, 5, 3
    Ls = 1 if mode == 1 else 2
    L = 2                                                    # part_len: the label length, and score_len of the STN modes
    out, _, _ = _inputs(mode, bs, pn, Ls, k)
    labels = torch.rand(bs, pn * L, generator=torch.Generator().manual_seed(1))
    lam = dict(lambda_1=0.05, lambda_MIL=0.9 if mode == 1 else 1.0, lambda_aux=0.8 if mode else 0.0,
               lambda_normal=0.2 if mode == 2 else 0.0, lambda_abnormal=2.0 if mode == 2 else 0.0)
    args = Namespace(batch_size=bs, part_num=pn, part_len=L, lambda_1=lam["lambda_1"], lambda_MIL=lam["lambda_MIL"], lambda_CE=0.8,
                     lambda_BCE=0.8, lambda_normal=0.2, lambda_abnormal=2.0, temporal_only=False, mil_topk=k)
    l1_skip = bs * pn * Ls if mode == 0 else bs
    aux = dict(abn_labels=labels, label_len=L) if mode else {}
    head_out = out.to(DEV).requires_grad_(True)
    loss, sc = training_loss(args, tmode, head_out, labels.to(DEV))
    loss.backward()
    sc_k, dout_k = _loss_gpu(mode, out, bs, bs, 0, pn, Ls, l1_skip, 2, None, k, lambdas=lam, **aux)
    assert torch.equal(head_out.grad.cpu(), dout_k) and torch.equal(sc.cpu(), sc_k)
    ck = Checks("topk", "training_loss " + tmode)
    ref = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, **lam, **aux)
    f32 = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, dtype=F32, **lam, **aux)
    terms = T.loss_terms_topk(mode, out, bs, pn, Ls, l1_skip, k, **lam, **aux)
    _close_all(ck, "", sc.detach().cpu(), head_out.grad.cpu(), ref, f32, terms)
    ck.true("loss is scalars[0]", float(loss) == float(sc[0]))
    if mode == 0:                                            # the reference-named entry point reads the same attribute
        y = out.to(DEV).view(2 * bs, pn * Ls, 1).requires_grad_(True)
        l2, err2, l12 = get_MIL_loss(args, y)
        l2.backward()
        ck.true("get_MIL_loss", float(err2) == float(sc[2]) and float(l12) == float(sc[3]) and torch.equal(y.grad.view(-1, 1).cpu(), dout_k))
    ck.done()


# ============================================================================================ f. one training step
STEP_CASE = "ltn_ucf"          # the smallest reduced LTN case of tests/golden/cases.py: 16 sequences of 19 tokens, d_model 32, part_num 4
SCALAR_BAR = 2e-5              # tests/test_hip_parity.py:86, test_training_step_matches_reference_golden
GRAD_BAR = lambda g: 2e-4 * float(g.abs().max()) + 1e-7          # tests/test_hip_parity.py:94


def _models(mode, ekw, d_model, dropout=0.0, head_dropout=0.0):
    from lstc_vad_amd.models import Classifier, Encoder
    enc = Encoder(n_layers=3, MHA_attn_dropout=dropout, MHA_fc_dropout=dropout, FFN_dropout=dropout,
                  position_dropout=dropout, weight_init=False, **ekw)
    return enc, Classifier(d_model, head_dropout, weight_init=False)


def _args(skw, **extra):
    return Namespace(batch_size=skw["batch_size"], part_num=skw["part_num"], part_len=skw["part_len"], n_patch=skw["n_patch"],
                     lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8, lambda_BCE=1.0, lambda_normal=0.2, lambda_abnormal=2.0,
                     temporal_only=False, clip_grad=False, **extra)


def test_topk_training_step_matches_oracle_forward_plus_topk_loss():
    """One LTN step through ``engine.TrainStep`` with ``mil_topk = 2``, every dropout rate 0: the oracle's forward pass
    (``orc.forward_loss``) with the top-k loss of util_topk hung behind its head output, under autograd, gives the scalars and
    every parameter gradient within the bars test_hip_parity applies to this case at k = 1 - and the k = 1 loss of the same
    input lies further away than that bar, so the old kernel cannot pass."""
    from lstc_vad_amd.engine import TrainStep
    z, mode, ekw, skw = load_case(STEP_CASE)
    assert mode == "LTN"
    d, bs, pn, L, k = ekw["d_model"], skw["batch_size"], skw["part_num"], skw["part_len"], 2
    nf, af, al = (torch.from_numpy(z[n]) for n in ("norm_feats", "abnorm_feats", "abnorm_labs"))
    # reference: float32 on the CPU, as the golden fixtures of this case are
    ecfg, st = oracle_cfgs(mode, ekw, skw)
    enc_P = {n: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for n, v in sub(z, "enc_init.").items()}
    head_P = {n: v.clone().requires_grad_(True) for n, v in sub(z, "head_init.").items()}
    fw = orc.forward_loss(enc_P, head_P, ecfg, st, nf, af, al, training=True)
    ref_sc = T.loss_graph(fw["outputs"], 1, bs, pn, 1, bs, k, 0.01, 1.0, 0.8, abn_labels=al, label_len=L)
    ref_sc[0].backward()
    assert abs(float(ref_sc[0]) - float(fw["loss"])) > 10 * SCALAR_BAR, "k = 2 and k = 1 give the same loss on this input"
    k1 = T.loss_graph(fw["outputs"].detach(), 1, bs, pn, 1, bs, 1, 0.01, 1.0, 0.8, abn_labels=al, label_len=L)
    assert float(k1[0]) == pytest.approx(float(fw["loss"]), abs=1e-6)          # (the restatement at k = 1 is the oracle's loss)

    enc, head = _models(mode, ekw, d)
    enc.load_state_dict(sub(z, "enc_init."), strict=True)
    head.load_state_dict(sub(z, "head_init."), strict=True)
    enc, head = enc.to(DEV).train(), head.to(DEV).train()
    ts = TrainStep(_args(skw, mil_topk=k), mode, enc, head, 1e-4, 1e-2, 1e-3)
    loss, sc, outputs = ts.forward_loss(nf.to(DEV), af.to(DEV), al.to(DEV))
    ts.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    assert max_abs_diff(outputs.reshape(fw["outputs"].shape), fw["outputs"]) < 1e-4
    want = np.array([float(s) for s in ref_sc])
    got = sc.cpu().double().numpy()
    print("top-k step scalars: got %s want %s" % (got, want))
    assert np.max(np.abs(got - want)) < SCALAR_BAR
    assert abs(float(sc[0]) - float(fw["loss"])) > SCALAR_BAR                  # not the k = 1 loss
    n_checked = 0
    for name, p in list(enc.named_parameters()) + list(head.named_parameters()):
        ref_p = enc_P.get(name) if name in enc_P else head_P.get(name)
        if ref_p is None or ref_p.grad is None:
            assert p.grad is None, name                                        # unused LayerNorms stay grad-less
            continue
        assert max_abs_diff(p.grad, ref_p.grad) < GRAD_BAR(ref_p.grad), (name, max_abs_diff(p.grad, ref_p.grad))
        n_checked += 1
    assert n_checked > 20
    ts.optimizer.step()
    torch.cuda.synchronize()


# ============================================================================================ g. captured step
def test_topk_graphed_step_is_bitwise_the_eager_step():
    """``engine.GraphedStep`` with ``mil_topk = 2`` (built like test_hip_parity.test_graphed_step_is_bitwise_the_eager_step,
    dropout on): three replays against three eager steps from the same weights and seed counter - the five scalars of every
    step and every weight after the last one are bit-identical."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.engine import GraphedStep, TrainStep
    z, mode, ekw, skw = load_case(STEP_CASE)
    d = ekw["d_model"]
    args = _args(skw, mil_topk=2)
    g = torch.Generator().manual_seed(5)
    batches = []
    for i in range(3):
        nf = torch.from_numpy(z["norm_feats"]) * (1.0 + 0.1 * i) + 0.01 * torch.randn(z["norm_feats"].shape, generator=g).abs()
        af = torch.from_numpy(z["abnorm_feats"]) * (1.0 - 0.05 * i)
        batches.append((nf.to(DEV), af.to(DEV), torch.from_numpy(z["abnorm_labs"]).to(DEV)))
    res = {}
    for how in ("eager", "graph", "eager_k1"):
        enc, head = _models(mode, dict(ekw), d, dropout=0.2, head_dropout=0.3)
        enc.load_state_dict(sub(z, "enc_init."), strict=True)
        head.load_state_dict(sub(z, "head_init."), strict=True)
        enc, head = enc.to(DEV).train(), head.to(DEV).train()
        ts = TrainStep(args if how != "eager_k1" else _args(skw), mode, enc, head, 1e-3, 1e-2, 1e-3, fuse_qkv="off")
        Fn.reset_rng(11)
        stepper = GraphedStep(ts, *batches[0]) if how == "graph" else ts
        scs = [stepper.step(*batches[i]).clone() for i in range(3)]
        torch.cuda.synchronize()
        res[how] = (scs, {n: p.detach().clone() for n, p in list(enc.named_parameters()) + list(head.named_parameters())}, Fn._counter)
    assert res["eager"][2] == res["graph"][2]
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert torch.equal(a, b), (a, b)
    for n, w in res["eager"][1].items():
        assert torch.equal(w, res["graph"][1][n]), n
    assert not torch.equal(res["eager"][0][0], res["eager"][0][2])             # (the steps do differ from one another)
    assert not torch.equal(res["eager"][0][0], res["eager_k1"][0][0])          # (and k = 2 is not k = 1 here)
