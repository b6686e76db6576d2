"""Attention masks, the part that needs no GPU: the host-side checks of the four ``*_masked`` C entry points (made before any
launch), ``LstcAttnMask`` against the C compiler's layout, ``functional.attn_mask_arg`` (shapes, dtypes, strides, no
materialised broadcast, errors), and the bit-for-bit regeneration of the committed reference fixtures
(tests/golden/mask_*.npz; skipped where the reference tree is absent)."""
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
E_NULL, E_SHAPE, E_UNSUPPORTED, E_RANGE = -1, -2, -4, -5
ENTRY = ("lstc_attn_fwd_masked", "lstc_attn_bwd_masked", "lstc_attn_cls_fwd_masked", "lstc_attn_cls_bwd_masked")


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _desc(S=49, dk=64, dv=64):
    """A descriptor that passes every host check (the pointers are never dereferenced on the host; no call below launches)."""
    from lstc_vad_amd._lib import AttnDesc
    d = AttnDesc()
    d.N, d.S, d.H, d.dk, d.dv = 2, S, 2, dk, dv
    d.ldq = d.ldk = 2 * dk
    d.ldv = d.ldo = 2 * dv
    d.scale = 0.125
    for f in ("Q", "K", "V", "O", "probs", "dO", "dQ", "dK", "dV"):
        setattr(d, f, 4096)
    return d


def _mask(ptr=4096, strides=(49 * 49, 0, 49, 1)):
    from lstc_vad_amd._lib import AttnMask
    return AttnMask(ptr, *strides)


@pytest.mark.parametrize("entry", ENTRY)
def test_masked_entry_points_check_their_arguments_before_any_launch(lib, entry):
    fn = getattr(lib, entry)
    d, m = _desc(), _mask()
    assert fn(C.byref(d), None, None) == E_NULL                                   # no mask struct
    assert fn(C.byref(d), C.byref(_mask(ptr=None)), None) == E_NULL               # no mask bytes
    assert fn(None, C.byref(m), None) == E_NULL
    for i in range(4):                                                            # a negative stride
        st = [49 * 49, 0, 49, 1]
        st[i] = -1
        assert fn(C.byref(d), C.byref(_mask(strides=st)), None) == E_SHAPE, i
    for field, value in (("O_pack", 4096), ("dQ_pack", 4096), ("dK_pack", 4096), ("dV_pack", 4096), ("in_pack_cols", 256),
                         ("dO_pack_cols", 128)):                                  # every packed form of the descriptor
        d = _desc()
        setattr(d, field, value)
        assert fn(C.byref(d), C.byref(m), None) == E_UNSUPPORTED, field
    assert fn(C.byref(_desc(S=513)), C.byref(m), None) == E_RANGE                 # as the unmasked calls
    for dk, dv in ((24, 64), (64, 40)):                                           # above S = 128: multiples of 16
        assert fn(C.byref(_desc(S=129, dk=dk, dv=dv)), C.byref(m), None) == E_RANGE, (dk, dv)
    d = _desc()
    d.Q = None                                                                    # the descriptor's own checks still apply
    assert fn(C.byref(d), C.byref(m), None) == E_NULL


def test_attn_mask_layout_matches_header(lib, tmp_path):
    """The ctypes mirror of LstcAttnMask against gcc's layout of include/lstc_hip.h; LstcAttnDesc keeps its size."""
    from lstc_vad_amd._lib import AttnDesc, AttnMask
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             'printf("LstcAttnMask %zu\\n", sizeof(LstcAttnMask));', 'printf("LstcAttnDesc %zu\\n", sizeof(LstcAttnDesc));']
    for fname, _ in AttnMask._fields_:
        lines.append(f'printf("LstcAttnMask.{fname} %zu\\n", offsetof(LstcAttnMask, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["LstcAttnMask"]) == C.sizeof(AttnMask) == 40
    assert int(got["LstcAttnDesc"]) == C.sizeof(AttnDesc)
    for fname, _ in AttnMask._fields_:
        assert int(got[f"LstcAttnMask.{fname}"]) == getattr(AttnMask, fname).offset, fname


N, H, S = 3, 2, 5
SHAPES = {                       # mask shape -> element strides over (n, h, i, j) of the normalised mask
    (S, S): (0, 0, S, 1),
    (1, 1, S, S): (0, 0, S, 1),
    (N, 1, 1, S): (S, 0, 0, 1),
    (N, 1, S, S): (S * S, 0, S, 1),
    (N, H, S, S): (H * S * S, S * S, S, 1),
}


@pytest.mark.parametrize("dtype", [torch.bool, torch.float32, torch.int64])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_attn_mask_arg_strides_and_values(shape, dtype):
    from lstc_vad_amd.functional import attn_mask_arg
    g = torch.Generator().manual_seed(sum(shape))
    kept = torch.rand(shape, generator=g) >= 0.4
    if dtype == torch.bool:
        mask = kept
    elif dtype == torch.float32:
        mask = torch.where(kept, torch.rand(shape, generator=g) + 0.25, torch.zeros(shape)) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    else:
        mask = torch.where(kept, torch.randint(1, 1000, shape, generator=g), torch.zeros(shape, dtype=torch.int64))
    m, strides = attn_mask_arg(mask, N, H, S)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (N, H, S, S)
    assert strides == SHAPES[shape], (strides, SHAPES[shape])
    assert torch.equal(m, kept.expand(N, H, S, S).to(torch.uint8))               # values in {0, 1}: non-zero = kept
    assert m.untyped_storage().nbytes() == kept.numel()                          # no [N, H, S, S] copy of a broadcast mask
    # what the kernels read: byte (n, h, i, j) through the strides
    flat = torch.as_strided(m, (m.untyped_storage().nbytes(),), (1,), 0)
    for n, h, i, j in ((0, 0, 0, 0), (N - 1, H - 1, S - 1, S - 1), (1, 1, 2, 3), (2, 0, 4, 1)):
        off = m.storage_offset() + n * strides[0] + h * strides[1] + i * strides[2] + j * strides[3]
        assert int(flat[off]) == int(kept.expand(N, H, S, S)[n, h, i, j])


def test_attn_mask_arg_single_sequence_and_head_axes():
    """N = 1 or H = 1: an axis of size 1 is reported as broadcast (stride 0), whatever the view's own stride."""
    from lstc_vad_amd.functional import attn_mask_arg
    m, st = attn_mask_arg(torch.ones(1, 1, 4, 4), 1, 1, 4)
    assert st == (0, 0, 4, 1) and tuple(m.shape) == (1, 1, 4, 4)


@pytest.mark.parametrize("shape", [(S + 1, S), (N + 1, 1, 1, S), (N, H + 1, S, S), (2, N, H, S, S), (N, 1, S, S - 1), (S - 1,)])
def test_attn_mask_arg_refuses_shapes_that_do_not_broadcast(shape):
    from lstc_vad_amd.functional import attn_mask_arg
    with pytest.raises(ValueError):
        attn_mask_arg(torch.ones(shape), N, H, S)


def test_attn_mask_arg_refuses_what_is_not_a_tensor():
    from lstc_vad_amd.functional import attn_mask_arg
    with pytest.raises(TypeError):
        attn_mask_arg([[1, 0], [1, 1]], 1, 1, 2)


def test_cross_attention_still_raises():
    from lstc_vad_amd.models import MultiHeadAttention
    mha = MultiHeadAttention(2, 32, 16, 16)
    x = torch.zeros(1, 5, 32)
    with pytest.raises(NotImplementedError, match="self-attention"):
        mha(x, x.clone(), x, mask=torch.ones(5, 5))


def test_mask_fixtures_hold_what_the_cases_say():
    """The committed fixtures alone (runs everywhere): the mask of each case is what mask_cases.build_mask builds, every case
    is under 1 MiB, masked keys of rows that keep a key have probability exactly 0 and the fully masked row is uniform - in the
    REFERENCE's own output (semantics points 2 and 3)."""
    from mask_cases import MASK_CASES, build_mask, seq_len
    kinds = {(c["kind"], c["dtype"] == "bool", seq_len(c) > 128) for c in MASK_CASES.values()}
    assert {(k, s) for k, _, s in kinds} == {("padding", False), ("padding", True), ("rows", False), ("rows", True)}
    assert {b for _, b, _ in kinds} == {True, False}
    for name, case in MASK_CASES.items():
        path = os.path.join(GOLD, name + ".npz")
        assert os.path.getsize(path) < 1 << 20, name
        z = np.load(path, allow_pickle=False)
        S = seq_len(case)
        mask = build_mask(case)
        assert z["mask"].dtype == mask.dtype and np.array_equal(z["mask"], mask)
        kept = np.broadcast_to(mask != 0, (case["N"], 2, S, S))
        alive = kept.any(-1, keepdims=True)
        for i in range(2):
            p = z[f"attn.{i}"]
            assert np.all(p[~kept & alive] == 0.0), (name, i)
            assert np.abs(p.sum(-1) - 1).max() < 1e-5
            if case["kind"] == "rows":
                n, r = case["dead_row"]
                assert not kept[n, :, r].any() and np.abs(p[n, :, r] - 1.0 / S).max() < 1e-7, (name, i)
        assert np.isfinite(z["out"]).all() and all(np.isfinite(z[k]).all() for k in z.files if k.startswith("grad"))


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (fixtures are generated in the build container)")
def test_make_golden_mask_reproduces_committed_fixtures(tmp_path):
    from mask_cases import MASK_CASES
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_mask.py"), "--out", str(tmp_path)], env=env, cwd="/",
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in MASK_CASES:
        a, b = np.load(os.path.join(tmp_path, name + ".npz"), allow_pickle=False), np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
