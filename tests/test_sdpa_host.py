"""Rectangular attention, the part that needs no GPU: the host-side checks of ``lstc_sdpa_fwd`` / ``lstc_sdpa_bwd`` (made before
any launch), ``LstcSdpaDesc`` against the C compiler's layout, the rectangular form of ``functional.attn_mask_arg``, the public
class surface, the committed reference fixtures (tests/golden/sdpa_*.npz) on their own and their bit-for-bit regeneration
(skipped where the reference tree is absent)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
E_NULL, E_SHAPE, E_RANGE = -1, -2, -5
ENTRY = ("lstc_sdpa_fwd", "lstc_sdpa_bwd")
STRIDES = tuple(f"{o}_{s}" for o in "qkvo" for s in ("sn", "sh", "st"))


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _desc(N=2, H=2, Sq=49, Sk=17, dk=64, dv=32):
    """A head-major descriptor that passes every host check (the pointers are never dereferenced on the host; no call below
    launches)."""
    from lstc_vad_amd._lib import SdpaDesc
    d = SdpaDesc()
    d.N, d.H, d.Sq, d.Sk, d.dk, d.dv = N, H, Sq, Sk, dk, dv
    for o, l, w in (("q", Sq, dk), ("k", Sk, dk), ("v", Sk, dv), ("o", Sq, dv)):
        setattr(d, o + "_sn", H * l * w), setattr(d, o + "_sh", l * w), setattr(d, o + "_st", w)
    d.scale, d.dropout_p = 0.125, 0.2
    for f in ("Q", "K", "V", "O", "probs", "dO", "dQ", "dK", "dV"):
        setattr(d, f, 4096)
    return d


def _mask(ptr=4096, strides=(49 * 17, 0, 17, 1)):
    from lstc_vad_amd._lib import AttnMask
    return AttnMask(ptr, *strides)


def _first_failure(fn, d, m=None):
    return fn(C.byref(d), C.byref(m) if m is not None else None, None)


@pytest.mark.parametrize("entry", ENTRY)
def test_sdpa_entry_points_check_their_arguments_before_any_launch(lib, entry):
    fn = getattr(lib, entry)
    bwd = entry.endswith("bwd")
    assert fn(None, None, None) == E_NULL
    assert fn(None, C.byref(_mask()), None) == E_NULL
    required = ("Q", "K", "V", "probs") + (("dO", "dQ", "dK", "dV") if bwd else ("O",))
    for f in required:
        d = _desc()
        setattr(d, f, None)
        assert _first_failure(fn, d) == E_NULL, f
    assert _first_failure(fn, _desc(), _mask(ptr=None)) == E_NULL                  # a mask struct without bytes
    for f in ("N", "H", "Sq", "Sk", "dk", "dv"):
        for bad in (0, -3):
            d = _desc()
            setattr(d, f, bad)
            assert _first_failure(fn, d) == E_SHAPE, (f, bad)
    for f in STRIDES:
        d = _desc()
        setattr(d, f, -1)
        assert _first_failure(fn, d) == E_SHAPE, f
    if bwd:                                                                       # a broadcast Q, K or V cannot be written through
        for f in STRIDES[:9]:
            d = _desc()
            setattr(d, f, 0)
            assert _first_failure(fn, d) == E_SHAPE, f
    for i in range(4):
        st = [49 * 17, 0, 17, 1]
        st[i] = -1
        assert _first_failure(fn, _desc(), _mask(strides=st)) == E_SHAPE, i
    for kw in (dict(Sq=513), dict(Sk=513), dict(dk=528), dict(dv=528), dict(dk=24), dict(dv=40), dict(dk=8)):
        assert _first_failure(fn, _desc(**kw)) == E_RANGE, kw
        assert _first_failure(fn, _desc(**kw), _mask()) == E_RANGE, kw
    # the 32-bit dropout counter: N H Sq Sk <= 2^32 - 1
    assert _first_failure(fn, _desc(N=4096, H=4, Sq=512, Sk=512)) == E_RANGE       # 2^32
    assert _first_failure(fn, _desc(N=1 << 20, H=1 << 12, Sq=1, Sk=1)) == E_RANGE  # N H > 2^31 - 1
    # a NULL pointer is reported ahead of a bad size, a bad size ahead of a limit
    d = _desc(Sq=513)
    d.Q = None
    assert _first_failure(fn, d) == E_NULL
    d = _desc(Sq=513)
    d.k_st = -1
    assert _first_failure(fn, d) == E_SHAPE


def test_sdpa_desc_layout_matches_header(lib, tmp_path):
    """The ctypes mirror of LstcSdpaDesc against gcc's layout of include/lstc_hip.h, field by field; the existing structs keep
    their sizes."""
    from lstc_vad_amd._lib import AttnDesc, AttnMask, SdpaDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             'printf("LstcSdpaDesc %zu\\n", sizeof(LstcSdpaDesc));', 'printf("LstcAttnMask %zu\\n", sizeof(LstcAttnMask));',
             'printf("LstcAttnDesc %zu\\n", sizeof(LstcAttnDesc));', 'printf("version %d\\n", LSTC_VERSION);']
    for fname, _ in SdpaDesc._fields_:
        lines.append(f'printf("LstcSdpaDesc.{fname} %zu %zu\\n", offsetof(LstcSdpaDesc, {fname}), sizeof(((LstcSdpaDesc*)0)->{fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcSdpaDesc"][0]) == C.sizeof(SdpaDesc)
    assert int(got["LstcAttnMask"][0]) == C.sizeof(AttnMask) == 40
    assert int(got["LstcAttnDesc"][0]) == C.sizeof(AttnDesc)
    assert int(got["version"][0]) == 112 == lib.lstc_version()
    for fname, ctype in SdpaDesc._fields_:
        off, size = (int(x) for x in got[f"LstcSdpaDesc.{fname}"])
        assert off == getattr(SdpaDesc, fname).offset and size == C.sizeof(ctype), fname
    assert [f for f, _ in SdpaDesc._fields_] == ["N", "H", "Sq", "Sk", "dk", "dv", *STRIDES, "scale", "dropout_p", "dropout_seed",
                                                 "Q", "K", "V", "O", "probs", "dO", "dQ", "dK", "dV"]


N, H, SQ, SK = 3, 2, 5, 7
SHAPES = {                       # mask shape -> element strides over (n, h, i, j) of the normalised mask
    (SQ, SK): (0, 0, SK, 1),
    (1, 1, SQ, SK): (0, 0, SK, 1),
    (N, 1, 1, SK): (SK, 0, 0, 1),
    (N, 1, SQ, SK): (SQ * SK, 0, SK, 1),
    (N, H, SQ, SK): (H * SQ * SK, SQ * SK, SK, 1),
    (SQ, 1): (0, 0, 1, 0),
}


@pytest.mark.parametrize("dtype", [torch.bool, torch.float32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_attn_mask_arg_rectangular(shape, dtype):
    from lstc_vad_amd.functional import attn_mask_arg
    g = torch.Generator().manual_seed(sum(shape))
    kept = torch.rand(shape, generator=g) >= 0.4
    mask = kept if dtype == torch.bool else torch.where(kept, torch.rand(shape, generator=g) + 0.25, torch.zeros(shape))
    m, strides = attn_mask_arg(mask, N, H, SQ, Sk=SK)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (N, H, SQ, SK)
    assert strides == SHAPES[shape], (strides, SHAPES[shape])
    assert torch.equal(m, kept.expand(N, H, SQ, SK).to(torch.uint8))
    assert m.untyped_storage().nbytes() == kept.numel()                          # no [N, H, Sq, Sk] copy of a broadcast mask


@pytest.mark.parametrize("shape", [(SK, SQ), (SQ, SQ), (N, 1, 1, SQ), (N + 1, 1, 1, SK), (2, N, H, SQ, SK)])
def test_attn_mask_arg_rectangular_refuses_shapes_that_do_not_broadcast(shape):
    from lstc_vad_amd.functional import attn_mask_arg
    with pytest.raises(ValueError):
        attn_mask_arg(torch.ones(shape), N, H, SQ, Sk=SK)


def test_scaled_dot_product_attention_class_surface():
    """Import paths, the reference's constructor and attributes (:12-15), and the errors that need no device."""
    from models.MultiHeadAttention import ScaledDotProductAttention
    from lstc_vad_amd.models import ScaledDotProductAttention as Exported
    from lstc_vad_amd.models.MultiHeadAttention import ScaledDotProductAttention as Home
    import inspect
    assert ScaledDotProductAttention is Exported is Home
    mod = ScaledDotProductAttention(8.0)
    assert mod.temperature == 8.0 and isinstance(mod.dropout, torch.nn.Dropout) and mod.dropout.p == 0.1
    assert ScaledDotProductAttention(temperature=4.0, attn_dropout=0.3).dropout.p == 0.3
    assert not list(mod.parameters()) and not list(mod.buffers())
    sig = inspect.signature(mod.forward)
    assert list(sig.parameters) == ["q", "k", "v", "mask", "relative_pe", "window_size"]
    assert (sig.parameters["mask"].default, sig.parameters["relative_pe"].default, sig.parameters["window_size"].default) == (None, False, 4)
    q, k, v = torch.zeros(1, 2, 3, 16), torch.zeros(1, 2, 5, 16), torch.zeros(1, 2, 5, 32)
    with pytest.raises(RuntimeError, match="HIP"):                                # no CPU path
        mod(q, k, v)
    with pytest.raises(ValueError, match="len_k"):
        mod(q, k, torch.zeros(1, 2, 4, 32))
    with pytest.raises(ValueError, match="d_k"):
        mod(q, torch.zeros(1, 2, 5, 32), v)


def test_sdpa_fixtures_hold_what_the_cases_say():
    """The committed fixtures alone (runs everywhere): the listed shapes and mask kinds, every file under 1 MiB, the inputs and the
    mask what sdpa_cases builds, and in the REFERENCE's own ``attn`` masked keys of rows that keep a key exactly 0 and the fully
    masked row exactly 1 / len_k."""
    from sdpa_cases import H as HEADS, SDPA_CASES, build_inputs, build_mask
    assert {(c["Sq"], c["Sk"], c["dk"], c["dv"], c["kind"]) for c in SDPA_CASES.values()} == {
        (1, 49, 64, 64, "padding"), (49, 17, 64, 32, "rows"), (17, 145, 32, 64, "none"), (145, 49, 64, 64, "padding"),
        (200, 333, 16, 48, "rows")}
    assert SDPA_CASES["sdpa_145x49_pad"]["dtype"] == "bool" and SDPA_CASES["sdpa_200x333_rows"]["N"] == 1 and HEADS == 2
    for name, case in SDPA_CASES.items():
        path = os.path.join(GOLD, name + ".npz")
        assert os.path.getsize(path) < 1 << 20, name
        z = np.load(path, allow_pickle=False)
        Nc, Sq, Sk = case["N"], case["Sq"], case["Sk"]
        for key, want in zip(("q", "k", "v", "w"), build_inputs(case)):
            assert z[key].dtype == np.float32 and np.array_equal(z[key], want), (name, key)
            assert key == "w" or (np.abs(z[key]).max() <= 1.0 and np.abs(z[key]).max() > 0.9), (name, key)
        p = z["attn"]
        assert p.shape == (Nc, HEADS, Sq, Sk) and z["output"].shape == (Nc, HEADS, Sq, case["dv"])
        assert np.abs(p.sum(-1) - 1).max() < 1e-5
        mask = build_mask(case)
        if mask is None:
            assert "mask" not in z.files
        else:
            assert z["mask"].dtype == mask.dtype and np.array_equal(z["mask"], mask)
            kept = np.broadcast_to(mask != 0, (Nc, HEADS, Sq, Sk))
            alive = np.broadcast_to(kept.any(-1, keepdims=True), kept.shape)
            assert (~kept & alive).any() and np.all(p[~kept & alive] == 0.0), name
            if case["kind"] == "rows":
                n, r = case["dead_row"]
                assert not kept[n, :, r].any() and np.all(p[n, :, r] == np.float32(1.0 / Sk)), name
        for key in ("grad_q", "grad_k", "grad_v"):
            assert z[key].shape == z[key[-1]].shape and np.isfinite(z[key]).all() and np.abs(z[key]).max() > 0, (name, key)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (fixtures are generated in the build container)")
def test_make_golden_sdpa_reproduces_committed_fixtures(tmp_path):
    from sdpa_cases import SDPA_CASES
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_sdpa.py"), "--out", str(tmp_path)], env=env, cwd="/",
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in SDPA_CASES:
        a, b = np.load(os.path.join(tmp_path, name + ".npz"), allow_pickle=False), np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
