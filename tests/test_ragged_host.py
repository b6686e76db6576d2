"""Padded (ragged) batches, CPU side: the new C entry points validate before any launch, the Python surface refuses what it
cannot take before anything touches a device, the padding helper of ``ltn_sequence_scores(ragged=True)`` keeps input order, and
the float64 references of tests/util_ragged.py agree with torch.autograd (tests/test_ragged_gpu.py then holds the kernels to them).
The arrangement of tests/test_cabi_host.py and tests/test_rowops_ref_host.py."""
import os

import pytest
import torch

import util_ragged as R

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_validate_before_any_launch(lib):
    """LSTC_E_NULL -1, LSTC_E_SHAPE -2, LSTC_E_ALIGN -3, LSTC_E_RANGE -5 (include/lstc_hip.h); no GPU is touched: every call here
    returns from the argument checks."""
    assert lib.lstc_version() == 112
    f, b = lib.lstc_cls_concat_len_fwd, lib.lstc_cls_concat_len_bwd
    # (x, lens, cls, pos, y, N, S, d, stream)
    assert f(None, 16, None, None, 16, 4, 49, 32, None) == -1
    assert f(16, None, None, None, 16, 4, 49, 32, None) == -1
    assert f(16, 16, None, None, None, 4, 49, 32, None) == -1
    assert f(16, 16, None, None, 16, 0, 49, 32, None) == -2
    assert f(16, 16, None, None, 16, -3, 49, 32, None) == -2
    assert f(16, 16, None, None, 16, 4, 1, 32, None) == -2          # S < 2: no token slot
    assert f(16, 16, None, None, 16, 4, 49, 0, None) == -2
    # (dy, lens, dx, dtok, N, S, d, mean_cls, stream)
    assert b(None, 16, 16, None, 4, 49, 32, 1, None) == -1
    assert b(16, None, 16, None, 4, 49, 32, 1, None) == -1
    assert b(16, 16, None, None, 4, 49, 32, 1, None) == -1          # neither dx nor dtok asked for
    assert b(16, 16, 16, 16, 0, 49, 32, 1, None) == -2
    assert b(16, 16, 16, None, 4, 1, 32, 1, None) == -2
    assert b(16, 16, None, 16, 4, 49, 0, 0, None) == -2
    # (U, X, klen, out, probs, N, S, H, d, mode, p, seed, stream): lstc_cls_dot's checks plus klen
    g = lib.lstc_cls_dot_len
    assert g(None, 16, 16, 16, 16, 4, 49, 2, 64, 1, 0.0, 0, None) == -1
    assert g(16, None, 16, 16, 16, 4, 49, 2, 64, 1, 0.0, 0, None) == -1
    assert g(16, 16, None, 16, 16, 4, 49, 2, 64, 1, 0.0, 0, None) == -1          # klen == NULL
    assert g(16, 16, 16, None, 16, 4, 49, 2, 64, 1, 0.0, 0, None) == -1
    assert g(16, 16, 16, 16, None, 4, 49, 2, 64, 1, 0.0, 0, None) == -1          # softmax mode needs probs
    assert g(16, 16, 16, 16, None, 4, 49, 2, 64, 2, 0.0, 0, None) == -1
    assert g(16, 16, 16, 16, 16, 0, 49, 2, 64, 1, 0.0, 0, None) == -2
    assert g(16, 16, 16, 16, 16, 4, 1, 2, 64, 1, 0.0, 0, None) == -2             # S < 2
    assert g(16, 16, 16, 16, 16, 4, 129, 2, 64, 1, 0.0, 0, None) == -5           # S > 128
    assert g(16, 16, 16, 16, 16, 4, 49, 17, 64, 1, 0.0, 0, None) == -5           # H > 16
    assert g(16, 16, 16, 16, 16, 4, 49, 2, 62, 1, 0.0, 0, None) == -3            # d % 4
    assert g(16, 24, 16, 16, 16, 4, 49, 2, 64, 1, 0.0, 0, None) == -3            # X not 16-B aligned
    assert g(16, 16, 16, 16, 16, 4, 49, 2, 64, 3, 0.0, 0, None) == -4            # unknown mode
    # the twin agrees wherever both apply
    t = lib.lstc_cls_dot
    for S, H, d in ((129, 2, 64), (49, 17, 64), (49, 2, 62)):
        assert t(16, 16, 16, 16, 4, S, H, d, 1, 0.0, 0, None) == g(16, 16, 16, 16, 16, 4, S, H, d, 1, 0.0, 0, None)


# ---------------------------------------------------------------------------------------------------- Python refusals
def _enc(**kw):
    from lstc_vad_amd.models import Encoder
    return Encoder(**R.encoder_kw(3, **kw))


@pytest.mark.parametrize("entry", ["forward", "forward_cls"])
def test_python_refusals_come_before_the_device_check(entry):
    """Every refusal on CPU tensors is a ValueError / NotImplementedError of its own, not the HIP-device RuntimeError: it is raised
    before anything could launch."""
    from lstc_vad_amd.functional import PackedAct
    enc = _enc()
    call = getattr(enc, entry)
    x = torch.zeros(3, 48, 32)
    for bad in ([0, 5, 48], [1, 5, 49], [-1, 2, 3], torch.tensor([1, 5, 49]), torch.tensor([0, 1, 2])):
        with pytest.raises(ValueError, match="length"):
            call(x, lengths=bad)
    for bad in ([1, 2], [1, 2, 3, 4], torch.tensor([1, 2]), torch.ones(3, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="entries"):
            call(x, lengths=bad)
    with pytest.raises(ValueError, match="integers"):
        call(x, lengths=[1.5, 2, 3])
    with pytest.raises(ValueError, match="integers"):
        call(x, lengths=torch.tensor([1.0, 2.0, 3.0]))
    bank = torch.zeros(10, 16, 32)
    with pytest.raises(ValueError, match="gather spec"):
        call((bank, torch.zeros(9, dtype=torch.int64), 3, 3), lengths=[1, 2, 3])
    with pytest.raises(NotImplementedError, match="PackedAct"):
        call(PackedAct(torch.zeros(8, dtype=torch.bfloat16), (3, 49, 32)), lengths=[1, 2, 3])
    if entry == "forward_cls":
        with pytest.raises(ValueError, match="enc_output_hi"):
            call(x, x, lengths=[1, 2, 3])
    # valid lengths on a CPU tensor get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP"):
        call(x, lengths=[1, 5, 48])
    with pytest.raises(RuntimeError, match="HIP"):
        call(x, lengths=torch.tensor([1, 5, 48], dtype=torch.int32))


def test_relative_pe_2d_takes_only_full_windows():
    from lstc_vad_amd.models import Encoder
    kw = R.encoder_kw(1, relative_pe=False, relative_pe_2D=True)
    enc = Encoder(**kw)
    x = torch.zeros(2, 16, 32)
    with pytest.raises(ValueError, match="relative_pe_2D"):
        enc(x, lengths=[16, 15])
    with pytest.raises(ValueError, match="relative_pe_2D"):
        enc.forward_cls(x, lengths=[3, 16])
    with pytest.raises(RuntimeError, match="HIP"):          # all full: passes the check, stops at the device
        enc(x, lengths=[16, 16])


def test_lengths_arg_and_key_padding_mask():
    from lstc_vad_amd.functional import lengths_arg
    from lstc_vad_amd.models.MultiHeadAttention import key_padding_mask
    lens, host = lengths_arg((3, 1, 4), 3, 5, "cpu")
    assert lens.dtype == torch.int32 and lens.tolist() == [3, 1, 4] and host == [3, 1, 4]
    lens, host = lengths_arg(torch.tensor([4, 4, 2], dtype=torch.int16), 3, 5, "cpu")
    assert lens.dtype == torch.int32 and host == [4, 4, 2]
    m = key_padding_mask(lens + 1, 5)
    assert m.shape == (3, 1, 1, 5) and m.dtype == torch.bool
    assert m[:, 0, 0].tolist() == [[True] * 5, [True] * 5, [True, True, True, False, False]]
    band = torch.ones(5, 5).tril(1).triu(-1)
    both = key_padding_mask(lens + 1, 5, band)
    assert both.shape == (3, 1, 5, 5) and torch.equal(both[2, 0], (band != 0) & m[2, 0, 0][None, :])
    # out-of-range key counts are clamped to [1, S], as the kernels clamp them
    assert key_padding_mask(torch.tensor([0, 9]), 5)[:, 0, 0].sum(-1).tolist() == [1, 5]


# ---------------------------------------------------------------------------------------------------- scoring helper
def test_ragged_batches_keep_input_order_and_lengths():
    from lstc_vad_amd.scoring import ragged_batches
    g = torch.Generator().manual_seed(5)
    lens = [16, 48, 32, 16, 1, 48, 16, 32, 32, 7, 48]
    seqs = [torch.randn(L, 8, generator=g) for L in lens]
    batches = ragged_batches(seqs, max_batch=4)
    assert [ids for ids, _, _ in batches] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    for ids, x, lengths in batches:
        assert x.shape == (len(ids), 48, 8) and lengths == [lens[i] for i in ids]
        for k, i in enumerate(ids):
            assert torch.equal(x[k, :lengths[k]], seqs[i]) and bool((x[k, lengths[k]:] == 0).all())
    (ids, x, lengths), = ragged_batches(seqs[:3])
    assert ids == [0, 1, 2] and x.shape == (3, 48, 8) and lengths == [16, 48, 32]


def test_scoring_and_pipeline_signatures_default_to_grouping_by_length():
    import inspect
    from lstc_vad_amd import pipeline, scoring
    for fn in (scoring.ltn_sequence_scores, scoring.ltn_part_scores, scoring.ltn_ucf_bin_scores, pipeline.generate_pseudo_labels,
               pipeline.evaluate_auc):
        assert inspect.signature(fn).parameters["ragged"].default is False, fn.__name__


# ---------------------------------------------------------------------------------------------------- float64 references
@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("with_pos", [False, True])
def test_concat_len_reference_against_autograd(learned, with_pos):
    g = torch.Generator().manual_seed(11)
    N, T, d = 4, 7, 6
    lens = [1, 3, 7, 6]
    x = torch.randn(N, T, d, generator=g, dtype=F64)
    for n, L in enumerate(lens):
        x[n, L:] = float("nan")                    # the reference never reads the padding
    x.requires_grad_(True)
    cls = torch.randn(d, generator=g, dtype=F64, requires_grad=True) if learned else None
    pos = torch.randn(T + 1, d, generator=g, dtype=F64, requires_grad=True) if with_pos else None
    dy = torch.randn(N, T + 1, d, generator=g, dtype=F64)
    y = R.cls_concat_len_fwd(x, lens, cls, pos)
    assert torch.isfinite(y).all()
    # the one rule: row n is the un-lengthed concat of x[n:n+1, :L_n], then zeros
    from util_rowops import cls_concat_fwd
    for n, L in enumerate(lens):
        alone = cls_concat_fwd(x[n:n + 1, :L].detach(), cls.detach() if learned else None, pos[:L + 1].detach() if with_pos else None)
        assert torch.equal(y[n, :L + 1].detach(), alone[0]) and bool((y[n, L + 1:] == 0).all())
    (y * dy).sum().backward()
    dx, dtok = R.cls_concat_len_bwd(dy, lens, mean_cls=not learned)
    for n, L in enumerate(lens):
        assert torch.allclose(x.grad[n, :L], dx[n, :L], rtol=0, atol=1e-14) and bool((dx[n, L:] == 0).all())
    if learned:
        assert torch.allclose(cls.grad, dtok[0], rtol=0, atol=1e-14)
    if with_pos:
        assert torch.allclose(pos.grad, dtok, rtol=0, atol=1e-14)


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
def test_cls_dot_len_reference_against_autograd(p_drop):
    g = torch.Generator().manual_seed(12)
    N, S, H, d = 3, 9, 2, 8
    klen = [1, 4, 9]
    U = torch.randn(N, H, d, generator=g, dtype=F64)
    X = torch.randn(N, S, d, generator=g, dtype=F64)
    G = torch.randn(N, H, d, generator=g, dtype=F64)                  # the backward's "U": d(out) = G . X
    keep = (torch.rand(N, H, S, generator=g) >= p_drop) if p_drop > 0 else None
    for n, kl in enumerate(klen):
        X[n, kl:] = float("nan")
    raw, _ = R.cls_dot_len(U, X, klen, 0)
    out, probs = R.cls_dot_len(U, X, klen, 1, keep=keep, p_drop=p_drop)
    ds, _ = R.cls_dot_len(G, X, klen, 2, probs=probs, keep=keep, p_drop=p_drop)
    for t in (raw, out, probs, ds):
        assert torch.isfinite(t).all()
    for n, kl in enumerate(klen):
        assert bool((raw[n, :, kl:] == 0).all() and (out[n, :, kl:] == 0).all() and (probs[n, :, kl:] == 0).all() and (ds[n, :, kl:] == 0).all())
        # the sequence alone, through autograd: logits -> softmax -> dropout -> <., G X>
        logit = (U[n] @ X[n, :kl].t()).requires_grad_(True)
        p = torch.softmax(logit, -1)
        pd = p * keep[n, :, :kl].to(F64) / (1 - p_drop) if p_drop > 0 else p
        (pd * (G[n] @ X[n, :kl].t())).sum().backward()
        assert torch.allclose(raw[n, :, :kl], logit.detach(), rtol=0, atol=1e-14)
        assert torch.allclose(probs[n, :, :kl], p.detach(), rtol=0, atol=1e-14) and torch.allclose(out[n, :, :kl], pd.detach(), rtol=0, atol=1e-14)
        assert torch.allclose(ds[n, :, :kl], logit.grad, rtol=0, atol=1e-13)
        assert abs(float(probs[n].sum()) - H) < 1e-12


@pytest.mark.parametrize("extra", [{}, {"CLS_learned": True}, {"position_encoding": True}])
def test_masked_oracle_restatement_is_the_oracle_without_a_mask(extra):
    """util_ragged.oracle_encoder_masked(mask=None) == oracle.encoder_forward, bit for bit; an all-ones mask changes nothing."""
    from lstc_vad_amd.models import Encoder
    from oracle import lstc_oracle as orc
    torch.manual_seed(3)
    kw = R.encoder_kw(3, **extra)
    P = {k: v.detach().clone() for k, v in Encoder(**kw).state_dict().items()}
    cfg = R.oracle_cfg(kw)
    x = torch.randn(2, 21, 32)
    ref = orc.encoder_forward(P, x, cfg)
    assert torch.equal(R.oracle_encoder_masked(P, x, cfg), ref)
    assert torch.equal(R.oracle_encoder_masked(P, x, cfg, torch.ones(22, 22)), ref)
    band = torch.ones(22, 22).tril(3).triu(-3)
    assert float((R.oracle_encoder_masked(P, x, cfg, band) - ref).abs().max()) > 1e-3
