"""CPU-only checks of the long-sequence attention entry points (128 < S <= 512, csrc/attention_long.hip): host validation
returns the documented error codes before any launch."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _desc(S, dk, H=1, N=1):
    from lstc_vad_amd._lib import AttnDesc
    a = AttnDesc()
    a.Q = a.K = a.V = a.O = a.probs = a.dO = a.dQ = a.dK = a.dV = 4096
    a.N, a.S, a.H, a.dk, a.dv = N, S, H, dk, dk
    a.ldq = a.ldk = a.ldv = a.ldo = H * dk
    a.scale = dk ** -0.5
    return a


def test_long_sequence_limits(lib):
    for fn in (lib.lstc_attn_fwd, lib.lstc_attn_bwd, lib.lstc_attn_cls_fwd, lib.lstc_attn_cls_bwd):
        assert fn(C.byref(_desc(513, 16)), None) == -5                # S > 512
    assert lib.lstc_attn_fwd(C.byref(_desc(200, 8)), None) == -5      # d_k not a multiple of 16
    assert lib.lstc_attn_bwd(C.byref(_desc(200, 8)), None) == -5
    a = _desc(200, 16)
    a.probs_ld = 204
    assert lib.lstc_attn_fwd(C.byref(a), None) == -4                 # dense probs only (fill_params, before the long path)
    assert lib.lstc_attn_bwd(C.byref(a), None) == -4


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (fixtures are generated in the build container)")
def test_make_golden_longseq_reproduces_committed_fixtures(tmp_path):
    """tests/golden/make_golden_longseq.py (the reference's run over longseq_cases.py) regenerates the committed long-sequence
    fixtures bit for bit."""
    import subprocess
    import sys
    import numpy as np
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, gold)
    from longseq_cases import LONG_CASES, LONG_FULL_CASES
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(gold, "make_golden_longseq.py"), "--out", str(tmp_path)], env=env, cwd="/",
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in list(LONG_CASES) + list(LONG_FULL_CASES):
        a = np.load(os.path.join(tmp_path, name + ".npz"), allow_pickle=False)
        b = np.load(os.path.join(gold, name + ".npz"), allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), (name, set(a.files) ^ set(b.files))
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
        assert os.path.getsize(os.path.join(gold, name + ".npz")) < 1 << 20


def test_long_sequence_packed_forms_are_unsupported(lib):
    a = _desc(200, 16)
    a.O_pack = 4096
    assert lib.lstc_attn_fwd(C.byref(a), None) == -4
    a = _desc(200, 16)
    a.in_pack_cols, a.K_col0, a.V_col0 = 64, 16, 32
    a.O_pack = 4096
    assert lib.lstc_attn_fwd(C.byref(a), None) == -4
    a = _desc(200, 16)
    a.dQ_pack = a.dK_pack = a.dV_pack = 4096
    assert lib.lstc_attn_bwd(C.byref(a), None) == -4


def test_long_sequence_backward_needs_partial_tables(lib):
    a = _desc(200, 16)
    a.index_ld, a.table_rows, a.table, a.index, a.dtable = 199, 397, 4096, 4096, 4096
    assert lib.lstc_attn_bwd(C.byref(a), None) == -4                 # dtable_chunks == 0: atomics, not on this path
    a.dtable_chunks = 2                                               # N = 1 sequence cannot make two chunks
    assert lib.lstc_attn_bwd(C.byref(a), None) == -2
    a.table_rows = 100000                                             # per-wave LDS tables past 160 KB
    a.dtable_chunks = 1
    assert lib.lstc_attn_bwd(C.byref(a), None) == -5


def _row_injective(idx):
    s = idx.sort(dim=1).values
    return bool((s[:, 1:] != s[:, :-1]).all())


def test_model_indices_are_row_injective_on_every_read_corner():
    """Both attention backwards add the bias-table gradient by a plain LDS read-modify-write, one query per instruction
    (csrc/attention.hip attn_bwd_kernel, csrc/attention_long.hip pass Q): correct only if, within one row of the top-left
    (S-1) x (S-1) corner the kernels read, distinct keys map to distinct table rows (include/lstc_hip.h, `index`).  Every
    index the models build for S <= 512: the 3-D index for windows 3 and 4 and depths up to 32, the 2-D index for
    ws^2 + 1 <= 512.  A corner's rows are prefixes of the rows of the largest corner, so checking that one covers every S."""
    import torch
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_2d, relative_position_index_3d
    n_checked = 0
    for ws in (3, 4):
        for L in range(1, 33):
            idx = relative_position_index_3d(L, ws)
            m = min(idx.shape[0], 511)
            assert _row_injective(idx[:m, :m]), (ws, L)
            n_checked += 1
    for ws in range(1, 23):
        idx = relative_position_index_2d(ws)
        assert ws * ws + 1 <= 512 and _row_injective(idx), ws
        n_checked += 1
    assert n_checked == 86
    bad = torch.tensor([[0, 1, 0], [2, 1, 0], [0, 1, 2]])        # the check itself sees a repeated table row
    assert not _row_injective(bad) and _row_injective(bad[1:, :2])
