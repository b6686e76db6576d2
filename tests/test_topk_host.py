"""CPU checks of the top-k MIL loss (LstcLossDesc.topk, --mil_topk): the float64 reference of tests/util_topk.py against
``torch.topk`` + autograd and against ``util_rowops.loss_ref`` at k = 1, its tie rule, the host-side refusals of
``lstc_vad_loss``, the descriptor layout, the command-line flag and the Python-side argument check.  No GPU is touched."""
import ctypes as C
import os
import subprocess
from argparse import Namespace

import pytest
import torch

import util_rowops as R
import util_topk as T
from oracle import lstc_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
LAMBDAS = dict(lambda_1=0.05, lambda_MIL=0.9, lambda_aux=0.8, lambda_normal=0.2, lambda_abnormal=2.0)


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _inputs(mode, bs, pn, Ls, seed):
    g = torch.Generator().manual_seed(seed)
    n = 2 * bs * pn * Ls
    out = (3.0 * torch.rand(n, 2 if mode == 1 else 1, generator=g) - 1.0) if mode != 2 else 0.05 + 0.9 * torch.rand(n, 1, generator=g)
    return out, torch.rand(bs, pn * 3, generator=g)


def _aux(mode, labels):
    return dict(abn_labels=labels, label_len=3) if mode else {}


# ------------------------------------------------------------------------------------------- 1. against torch.topk
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_reference_equals_torch_topk_with_autograd(mode, k):
    """On a tie-free input the selected set is ``torch.topk``'s: all five scalars and dout, float64, to rounding."""
    bs, pn, Ls = 4, 5, (1 if mode == 1 else 2)
    out, labels = _inputs(mode, bs, pn, Ls, 7 + mode)
    assert T.loss_margins_topk(mode, out, bs, pn, Ls, k)[1] > 1e-6            # tie-free
    l1_skip = bs
    sc, dout = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, k, **LAMBDAS, **_aux(mode, labels))
    c = 2 if mode == 1 else 1
    o = out.to(F64).requires_grad_(True)
    score = o[:, c - 1]
    pm = score.reshape(2 * bs, pn, Ls).mean(-1)
    bag = torch.topk(pm, k, -1).values.mean(-1)
    err = torch.relu(1.0 - bag[bs:][None, :] + bag[:bs][:, None]).sum() / bs ** 2
    l1 = score[l1_skip:].mean()
    mil = err + LAMBDAS["lambda_1"] * l1
    aux = torch.zeros((), dtype=F64)
    if mode:
        t = orc.soft_targets(labels, bs, pn, 3).to(F64)
        aux = orc.ce_loss(o, t.reshape(-1, 2)) if mode == 1 else orc.bce_loss(pm, t, LAMBDAS["lambda_normal"], LAMBDAS["lambda_abnormal"])
    loss = LAMBDAS["lambda_MIL"] * mil + LAMBDAS["lambda_aux"] * aux
    loss.backward()
    want = torch.stack([loss, mil, err, l1, aux]).detach()
    assert float((sc - want).abs().max()) < 1e-14, (sc, want)
    assert float((dout - o.grad).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------- 2. k = 1 is loss_ref
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_reference_at_k1_gives_exactly_the_numbers_of_loss_ref(mode, dtype):
    bs, pn, Ls = 5, 4, (1 if mode == 1 else 2)
    out, labels = _inputs(mode, bs, pn, Ls, 11 + mode)
    for l1_skip in (bs, bs * pn * Ls):
        a = R.loss_ref(mode, out, bs, pn, Ls, l1_skip, **LAMBDAS, **_aux(mode, labels), dtype=dtype)
        b = T.loss_ref_topk(mode, out, bs, pn, Ls, l1_skip, 1, **LAMBDAS, **_aux(mode, labels), dtype=dtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if dtype == F64:
            ta = R.loss_terms(mode, out, bs, pn, Ls, l1_skip, **LAMBDAS, **_aux(mode, labels))
            tb = T.loss_terms_topk(mode, out, bs, pn, Ls, l1_skip, 1, **LAMBDAS, **_aux(mode, labels))
            assert torch.equal(ta[0], tb[0]) and torch.equal(ta[1], tb[1])
            ma, mb = R.loss_margins(mode, out, bs, pn, Ls), T.loss_margins_topk(mode, out, bs, pn, Ls, 1)
            assert ma == mb


# ------------------------------------------------------------------------------------------- 3. the tie rule
def test_reference_ties_go_to_the_lower_part_index():
    """Parts 1, 2, 3 and 4 of one abnormal video hold the same scores and part 0 a smaller one: k = 3 selects parts 1, 2, 3 -
    of four equal means the three with the lowest indices - and each gets gbag / (k * score_len)."""
    bs, pn, Ls, k = 2, 5, 2, 3
    g = torch.Generator().manual_seed(0)
    out = torch.rand(2 * bs * pn * Ls, 1, generator=g)
    v = out.view(2 * bs, pn, Ls)
    v[bs, 0] = torch.tensor([0.1, 0.2])
    v[bs, 1:] = torch.tensor([0.3, 0.5])
    vals, idx = T.topk_select(T.part_means(out.to(F64)[:, 0], bs, pn, Ls), k)
    assert idx[bs].tolist() == [1, 2, 3]
    _, dout = T.loss_ref_topk(0, out, bs, pn, Ls, bs, k, 0.0, 1.0, 0.0)
    d = dout.view(2 * bs, pn, Ls)[bs]
    assert float(d[1, 0]) < 0 and bool((d[1:4] == d[1, 0]).all()) and bool((d[0] == 0).all()) and bool((d[4] == 0).all())
    assert abs(float(d[1, 0]) - (-bs / bs ** 2 / (k * Ls))) < 1e-15       # both normal videos are inside the margin: cnt = bs
    assert T.loss_margins_topk(0, out, bs, pn, Ls, k)[1] == 0.0


# ------------------------------------------------------------------------------------------- 4. host-side refusals
def test_lstc_vad_loss_refuses_bad_topk_before_any_launch(lib):
    from lstc_vad_amd._lib import LossDesc

    def desc(pn, topk):
        d = LossDesc()
        d.out = d.dout = d.scalars = 16                     # dummy pointers: every case below returns before a launch
        d.mode, d.phase, d.bs_global, d.bs_local, d.part_num, d.score_len = 0, 2, 2, 2, pn, 1
        d.topk = topk
        return d
    assert lib.lstc_vad_loss(C.byref(desc(4, -1)), None) == -2            # LSTC_E_SHAPE
    assert lib.lstc_vad_loss(C.byref(desc(4, 5)), None) == -5             # LSTC_E_RANGE: topk > part_num
    assert lib.lstc_vad_loss(C.byref(desc(65, 2)), None) == -5            # LSTC_E_RANGE: one part per lane of a wave64
    assert lib.lstc_vad_loss(C.byref(desc(1, 2)), None) == -5
    d = desc(4, -1)
    d.out = None
    assert lib.lstc_vad_loss(C.byref(d), None) == -1                      # a NULL `out` is still reported first
    d = desc(4, 5)
    d.dout = None
    assert lib.lstc_vad_loss(C.byref(d), None) == -1


# ------------------------------------------------------------------------------------------- 5. layout
def test_topk_is_the_last_field_in_the_old_tail_padding(lib, tmp_path):
    from lstc_vad_amd._lib import LossDesc
    names = [f for f, _ in LossDesc._fields_]
    assert names[-1] == "topk" and len(names) == 21
    # the 20 earlier fields where every caller built against the previous header has them
    before = {"mode": 0, "bs_global": 4, "bs_local": 8, "rank_off": 12, "part_num": 16, "score_len": 20, "label_len": 24,
              "l1_skip": 28, "lambda_1": 32, "lambda_MIL": 36, "lambda_aux": 40, "lambda_normal": 44, "lambda_abnormal": 48,
              "out": 56, "abn_labels": 64, "targets": 72, "bag": 80, "dout": 88, "scalars": 96, "phase": 104}
    assert names[:-1] == list(before)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(LstcLossDesc));']
    lines += [f'printf("{f} %zu\\n", offsetof(LstcLossDesc, {f}));' for f in names]
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {a: int(b) for a, b in (l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof"] == 112 == C.sizeof(LossDesc)
    assert got["topk"] == 108 == LossDesc.topk.offset
    for f, off in before.items():
        assert got[f] == off == getattr(LossDesc, f).offset, f
    assert LossDesc().topk == 0                                           # a zero-initialised descriptor: k = 1
    assert lib.lstc_version() == 112


# ------------------------------------------------------------------------------------------- 6. command line
def test_mil_topk_flag_parses_everywhere_and_topk_stays_unwired():
    from lstc_vad_amd import cli
    assert len(cli.SCRIPTS) == 7
    for script in cli.SCRIPTS:
        p = cli.build_parser(script)
        assert p.parse_args([]).mil_topk == 1, script
        assert p.parse_args(["--mil_topk", "3"]).mil_topk == 3, script
        assert cli.complete_args(script, Namespace(batch_size=2)).mil_topk == 1, script      # a caller-built namespace gets the default
        assert cli.complete_args(script, Namespace(mil_topk=4)).mil_topk == 4, script
        back = cli.complete_args(script, argv=cli.namespace_to_argv(script, p.parse_args(["--mil_topk", "3"])))
        assert back.mil_topk == 3, script                                                    # what a rank process is started with
    with_topk = [s for s in cli.SCRIPTS if s.startswith("spatio_")]
    assert len(with_topk) == 4
    for script in with_topk:                                  # the reference's --topk (default 7): parsed, unused, as upstream
        a = cli.build_parser(script).parse_args(["--topk", "5"])
        assert a.topk == 5 and a.mil_topk == 1, script
        assert cli.build_parser(script).parse_args([]).topk == 7
    help_text = cli.build_parser("spatio_transformer_shanghaitech").format_help()
    assert "--mil_topk" in help_text and "--topk" in help_text.split("--mil_topk", 1)[1]


# ------------------------------------------------------------------------------------------- 7. Python-side check
@pytest.mark.parametrize("pn,k", [(4, 0), (4, 5), (65, 2), (4, 2.0), (4, True)])
def test_losses_refuse_a_bad_mil_topk_before_the_device_matters(pn, k):
    """CPU tensors: without the check the first thing to fail would be the no-CPU-fallback RuntimeError of ``dev_ptr``."""
    from lstc_vad_amd.losses import get_MIL_loss, training_loss
    bs, L = 2, 2
    args = Namespace(batch_size=bs, part_num=pn, part_len=L, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8, lambda_BCE=1.0,
                     lambda_normal=0.2, lambda_abnormal=2.0, temporal_only=False, mil_topk=k)
    for mode, shape in (("LTN", (2 * bs * pn, 2)), ("STN", (2 * bs * pn * L, 1)), ("STN_MIL_CE", (2 * bs * pn * L, 1))):
        with pytest.raises(ValueError, match="mil_topk"):
            training_loss(args, mode, torch.rand(*shape), torch.rand(bs, pn * L))
    with pytest.raises(ValueError, match="mil_topk"):
        get_MIL_loss(args, torch.rand(2 * bs, pn * L, 1))
    # a valid value passes the check and reaches the HIP-only path
    args.mil_topk, args.part_num = 2, 4
    with pytest.raises(RuntimeError, match="HIP"):
        training_loss(args, "STN", torch.rand(2 * bs * 4 * L, 1), None)
    del args.mil_topk                                                     # absent: 1
    with pytest.raises(RuntimeError, match="HIP"):
        get_MIL_loss(args, torch.rand(2 * bs, 4 * L, 1))
