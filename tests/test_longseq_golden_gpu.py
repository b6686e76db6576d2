"""Long-sequence training steps (S = 145, 257: csrc/attention_long.hip) against the REAL reference's fixtures
(tests/golden/make_golden_longseq.py over tests/golden/longseq_cases.py), the dropout-on step replayed through the oracle, the
bf16-mode step, GraphedStep against the eager step, and the production-width case.  GPU tests read only the committed fixtures."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def load_long(name):
    """(z, mode, encoder kwargs, step kwargs) of a long-sequence fixture, in the form of util.load_case.  The fixtures keep one
    copy of the relative-position index (layer 0's initial one): every layer's buffer is that same index, restored here so the
    reference's state dicts load strictly."""
    from longseq_cases import LONG_CASES
    from util import GOLDEN
    zf = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    d = {k: zf[k] for k in zf.files}
    idx0 = "enc_init.layer_stack.0.slf_attn.relative_position_index"
    for pre in ("enc_init.", "enc_after2."):
        for li in range(3):
            d.setdefault(f"{pre}layer_stack.{li}.slf_attn.relative_position_index", d[idx0])

    class _Z(dict):
        files = property(lambda self: list(self.keys()))
    mode, ekw, skw = LONG_CASES[name]
    return _Z(d), mode, dict(ekw), dict(skw)


@pytest.fixture
def long_cases(monkeypatch):
    """tests/test_hip_parity.py's step-test bodies, reading the long-sequence fixtures."""
    import test_hip_parity as hp
    monkeypatch.setattr(hp, "load_case", load_long)
    return hp


def test_fixture_index_is_the_models_index():
    """The models build the reference's relative-position index (the UCF case's [256, 256] index read as its 144 x 144 corner)."""
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d
    for name in ("ltn_sht_long", "ltn_ucf_long", "ltn_long_dk32"):
        z, _, ekw, skw = load_long(name)
        idx = z["enc_init.layer_stack.0.slf_attn.relative_position_index"]
        assert np.array_equal(relative_position_index_3d(ekw["window_depth"], ekw["window_size"]).numpy(), idx), name
        assert idx.shape[0] >= skw["part_len"] * skw["n_patch"]
    assert load_long("ltn_ucf_long")[0]["enc_init.layer_stack.0.slf_attn.relative_position_index"].shape == (256, 256)


@pytest.mark.parametrize("cls_only", [False, True])
@pytest.mark.parametrize("name", ["ltn_sht_long", "ltn_ucf_long", "ltn_long_dk32"])
def test_long_training_step_matches_reference_golden(long_cases, name, cls_only):
    """Two steps against the reference: forward 1e-4, scalars 2e-5, every step-0 gradient within 2e-4 of its maximum, the
    encoder's weights after two Adagrad steps (the bars of test_hip_parity.test_training_step_matches_reference_golden)."""
    hp = long_cases
    from lstc_vad_amd.optim import Adagrad
    from util import max_abs_diff, sub
    z, mode, ekw, skw = load_long(name)
    d = ekw["d_model"]
    enc, head = hp._models(mode, ekw, d)
    enc.load_state_dict(sub(z, "enc_init."), strict=True)
    head.load_state_dict(sub(z, "head_init."), strict=True)
    enc, head = enc.to(DEV).train(), head.to(DEV).train()
    args = hp._args(mode, skw)
    nf, af, al = (torch.from_numpy(z[k]).to(DEV) for k in ("norm_feats", "abnorm_feats", "abnorm_labs"))
    opt = Adagrad([{"params": enc.parameters(), "lr": 1e-4}, {"params": head.parameters(), "lr": 1e-2}], weight_decay=1e-3)
    for step in range(2):
        enc_out, outputs, loss, sc = hp._step(enc, head, mode, args, nf, af, al, d, cls_only)
        opt.zero_grad()
        loss.backward()
        if step == 0:
            ref_enc = z["enc_out"][:, :1, :] if cls_only else z["enc_out"]
            assert max_abs_diff(enc_out, ref_enc) < 1e-4
            assert max_abs_diff(outputs.reshape(z["outputs"].shape), z["outputs"]) < 1e-4
            assert np.max(np.abs(sc.cpu().double().numpy() - z["scalars"])) < 2e-5
            ref_g, ref_h = sub(z, "enc_grad."), sub(z, "head_grad.")
            got = {k for k, p in enc.named_parameters() if p.grad is not None}
            assert got == set(ref_g), got ^ set(ref_g)
            n = 0
            for k, p in list(enc.named_parameters()) + list(head.named_parameters()):
                g = ref_g.get(k) if k in ref_g else ref_h.get(k)
                if g is None:
                    continue
                tol = 2e-4 * float(g.abs().max()) + 1e-7
                assert max_abs_diff(p.grad, g) < tol, (k, max_abs_diff(p.grad, g), tol)
                n += 1
            assert n >= 30
        else:
            assert np.max(np.abs(sc.cpu().double().numpy() - z["scalars_step2"])) < 1e-4
        opt.step()
    ref = sub(z, "enc_after2.")
    for k, v in enc.state_dict().items():
        if v.is_floating_point():
            diff = (v.cpu() - ref[k]).abs()
            assert float((diff > 5e-5).float().mean()) <= 1e-3 and float(diff.max()) <= 4e-4 + 1e-6, (k, float(diff.max()))


@pytest.mark.parametrize("cls_only", [False, True])
def test_long_dropout_run_replays_through_oracle(long_cases, cls_only):
    """Every dropout on at S = 145: the HIP run's masks (the long kernels' attention masks included) injected into the oracle
    reproduce scores, loss and every gradient."""
    long_cases.test_dropout_run_replays_through_oracle("ltn_sht_long", cls_only)


def test_long_bf16_compute_training_step_close_to_golden(long_cases):
    """A bf16-mode step at S = 145 (long kernels on bf16 products): loss within 2e-2, gradient directions (cosine > 0.9)."""
    long_cases.test_bf16_compute_training_step_close_to_golden("ltn_sht_long")


def test_long_graphed_step_is_bitwise_the_eager_step(long_cases):
    """GraphedStep replays with dropout on at S = 145 equal the eager steps bit for bit: the long kernels draw their masks
    from the device-side seed word like the short ones."""
    long_cases.test_graphed_step_is_bitwise_the_eager_step("ltn_sht_long", "fp32")


def test_bf16_mode_packed_products_at_s145():
    """bf16 mode with every product on the packed kernel (thresholds 0) and N*S a multiple of 256 - the shape where MHAFunction
    would ask the attention for a packed O: above S = 128 it asks for f32 rows (the long kernels write no pack), and forward and
    backward track the fp32 run."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.models import Encoder
    torch.manual_seed(0)
    enc = Encoder(n_layers=2, MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0, weight_init=True, n_head=2, d_k=128,
                  d_v=128, d_model=256, d_inner=512, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True, window_size=4,
                  window_depth=9).to(DEV).train()
    x = torch.randn(256, 144, 256, device=DEV)                     # 256 sequences x 145 tokens: N*S % 256 == 0
    res = {}
    for mode in ("fp32", "bf16"):
        Fn.set_compute_dtype(mode)
        if mode == "bf16":
            Fn.set_x3_threshold(0, 0, 0)
        try:
            if mode == "bf16":
                assert not Fn.attn_fwd_pack(256, 145, 2, 128) and Fn.attn_fwd_pack(256, 128, 2, 128)
            enc.zero_grad(set_to_none=True)
            y = enc(x)
            y.square().mean().backward()
            torch.cuda.synchronize()
        finally:
            Fn.set_compute_dtype("fp32")
            Fn.set_x3_threshold()
        res[mode] = (y.detach().clone(), {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None})
    a, b = res["bf16"][0].double().flatten(), res["fp32"][0].double().flatten()
    assert torch.isfinite(a).all() and float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.999
    for k, g in res["fp32"][1].items():
        h = res["bf16"][1][k]
        if g.numel() > 64 and float(g.norm()) > 0:
            assert torch.isfinite(h).all(), k
            assert float((h * g).sum() / (h.norm() * g.norm())) > 0.9, k


def test_long_full_width_step_matches_reference():
    """ltn_long_full: d_model 2048, H = 8 x 256, S = 145, 32 sequences.  Eval scores (full parts and both shorter tails) within
    1e-4, step-0 scores / scalars within 1e-4 / 2e-5, at least 99 % of the sampled gradient entries within 2e-4 of their tensor's
    maximum (every entry within the un-aligned bars of test_hip_parity); a remainder must disappear when the reference's decisions
    are imposed at its recorded ReLU-edge units."""
    import test_hip_parity as hp
    from cases import fill_params
    from longseq_cases import LONG_FULL_CASES
    from util import GOLDEN, cached_training_batch, max_abs_diff
    name = "ltn_long_full"
    mode, ekw, skw, seed = LONG_FULL_CASES[name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    assert int(z["seed"]) == seed
    d = ekw["d_model"]
    enc, head = hp._models(mode, dict(ekw), d)
    fill_params(enc, seed)
    fill_params(head, seed + 1)
    nf, _, af, al = cached_training_batch(skw["batch_size"], skw["part_num"], skw["part_len"], skw["n_patch"], d, seed=seed,
                                          with_pseudo=True, threshold=0.6)
    nf, af, al = (torch.from_numpy(t).to(DEV) for t in (nf, af, al))
    bs, pn, L, P = skw["batch_size"], skw["part_num"], skw["part_len"], skw["n_patch"]
    enc, head = enc.to(DEV).eval(), head.to(DEV).eval()
    with torch.no_grad():
        x = nf.float().view(bs * pn, L * P, d)[:8]
        for tag, xs in (("full", x), ("tail", x[:, :(L - 1) * P]), ("tail1", x[:, :P])):
            assert max_abs_diff(head(enc(xs)[:, 0, :]), z["eval_scores_" + tag]) < 1e-4, tag
    enc, head = enc.train(), head.train()
    args = hp._args(mode, skw)
    n_seq, S = 2 * bs * pn, 1 + P * L

    def step0(align):
        for p in list(enc.parameters()) + list(head.parameters()):
            p.grad = None
        edges = None
        if align:
            with hp._align_relu_edges(z, n_seq, S) as edges:
                enc_out, outputs, loss, sc = hp._step(enc, head, mode, args, nf, af, al, d, True)
        else:
            enc_out, outputs, loss, sc = hp._step(enc, head, mode, args, nf, af, al, d, True)
        loss.backward()
        _, _, (beyond, _), total = hp._compare_full_width_step0(z, enc, head, enc_out, outputs, sc, True, hp.UNALIGNED_GRAD_BAR,
                                                               hp.UNALIGNED_NORM_BAR, strict=2e-4)
        return 1.0 - beyond / max(total, 1), total, edges

    frac, total, _ = step0(False)
    assert total > 5000
    if frac < 0.99:
        frac_a, _, edges = step0(True)
        assert edges.changed >= 1 and frac_a >= 0.99, (frac, frac_a, edges.changed)
