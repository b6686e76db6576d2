"""Cross-attention, the part that needs no GPU: the committed reference fixtures (tests/golden/mha_cross_*.npz) on their own and
their bit-for-bit regeneration (skipped where the reference tree is absent), every refusal of
``MultiHeadAttention.forward_cross`` (raised before any launch), the ``lstc_sdpa_few_query_max`` export, and the host side of the
``lstc_sdpa_*`` launcher under AddressSanitizer and UBSan as a stand-alone program (argument errors only: nothing is launched)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_mha_cross_fixtures_hold_what_the_cases_say():
    from mha_cross_cases import D_MODEL, H, MHA_CROSS_CASES, build_inputs, build_mask
    assert {(c["Sq"], c["Sk"], c["kind"], c["bias"], c["shared_kv"], c["layer_norm"]) for c in MHA_CROSS_CASES.values()} == {
        (1, 49, "padding", None, False, True), (5, 17, "none", None, True, True), (16, 145, "rows", None, False, True),
        (49, 17, "rows", None, False, False), (145, 200, "none", None, True, True), (49, 49, "none", "3d", True, True),
        (145, 145, "padding", "3d", False, True), (17, 17, "none", "2d", False, True)}
    assert (MHA_CROSS_CASES["mha_cross_5x17"]["dk"], MHA_CROSS_CASES["mha_cross_5x17"]["dv"]) == (32, 16) and (H, D_MODEL) == (2, 64)
    for name, case in MHA_CROSS_CASES.items():
        path = os.path.join(GOLD, name + ".npz")
        assert os.path.getsize(path) < 1 << 20, name
        z = np.load(path, allow_pickle=False)
        N, Sq, Sk = case["N"], case["Sq"], case["Sk"]
        for key, want in zip(("q", "k", "v", "w"), build_inputs(case)):
            assert z[key].dtype == np.float32 and np.array_equal(z[key], want), (name, key)
        assert z["q"].shape == (N, Sq, D_MODEL) and z["k"].shape == z["v"].shape == (N, Sk, D_MODEL)
        assert np.array_equal(z["k"], z["v"]) == case["shared_kv"], name
        p = z["attn"]
        assert p.shape == (N, H, Sq, Sk) and z["out"].shape == (N, Sq, D_MODEL)
        assert np.abs(p.sum(-1) - 1).max() < 1e-5
        mask = build_mask(case)
        if mask is None:
            assert "mask" not in z.files
        else:
            assert z["mask"].dtype == mask.dtype and np.array_equal(z["mask"], mask)
            kept = np.broadcast_to(mask != 0, (N, H, Sq, Sk))
            alive = np.broadcast_to(kept.any(-1, keepdims=True), kept.shape)
            assert (~kept & alive).any() and np.all(p[~kept & alive] == 0.0), name
            if case["kind"] == "rows":
                n, r = case["dead_row"]
                assert not kept[n, :, r].any() and np.all(p[n, :, r] == np.float32(1.0 / Sk)), name
        for key in ("grad_q", "grad_k") + (() if case["shared_kv"] else ("grad_v",)):
            assert z[key].shape == z[key[-1]].shape and np.isfinite(z[key]).all() and np.abs(z[key]).max() > 0, (name, key)
        assert not case["shared_kv"] or np.abs(z["grad_v"]).max() == 0
        widths = {"grad.w_qs.weight": (H * case["dk"], D_MODEL), "grad.w_ks.weight": (H * case["dk"], D_MODEL),
                  "grad.w_vs.weight": (H * case["dv"], D_MODEL), "grad.fc.weight": (D_MODEL, H * case["dv"]),
                  "grad.layer_norm.weight": (D_MODEL,), "grad.layer_norm.bias": (D_MODEL,)}
        for key, shape in widths.items():
            assert z[key].shape == shape and np.isfinite(z[key]).all(), (name, key)
            assert (np.abs(z[key]).max() > 0) == (case["layer_norm"] or "layer_norm" not in key), (name, key)
        assert ("grad.relative_position_bias_table" in z.files) == (case["bias"] is not None)
        if case["bias"] is not None:
            assert np.abs(z["grad.relative_position_bias_table"]).max() > 0


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (fixtures are generated in the build container)")
def test_make_golden_mha_cross_reproduces_committed_fixtures(tmp_path):
    from mha_cross_cases import MHA_CROSS_CASES
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_mha_cross.py"), "--out", str(tmp_path)], env=env, cwd="/",
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in MHA_CROSS_CASES:
        a, b = np.load(os.path.join(tmp_path, name + ".npz"), allow_pickle=False), np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)


def _mha(**kw):
    from lstc_vad_amd.models import MultiHeadAttention
    return MultiHeadAttention(2, 32, 16, 16, **kw)


def test_forward_cross_refusals_need_no_device():
    from lstc_vad_amd.functional import PackedAct
    z = lambda *s: torch.zeros(*s)
    mha = _mha()
    with pytest.raises(ValueError):
        mha.forward_cross(z(5, 32), z(1, 7, 32), z(1, 7, 32))                      # not 3-D
    with pytest.raises(ValueError):
        mha.forward_cross(z(1, 5, 32), z(1, 2, 7, 32), z(1, 7, 32))
    with pytest.raises(ValueError, match="d_model"):
        mha.forward_cross(z(1, 5, 32), z(1, 7, 16), z(1, 7, 32))
    with pytest.raises(ValueError, match="d_model"):
        mha.forward_cross(z(1, 5, 48), z(1, 7, 48), z(1, 7, 48))
    with pytest.raises(ValueError, match="len_k"):
        mha.forward_cross(z(1, 5, 32), z(1, 7, 32), z(1, 6, 32))
    for kw in (dict(relative_pe=True, window_size=4, window_depth=3), dict(relative_pe_2D=True, window_size=4)):
        with pytest.raises(ValueError, match="len_q == len_k"):
            _mha(**kw).forward_cross(z(1, 49, 32), z(1, 33, 32), z(1, 33, 32))
        with pytest.raises(ValueError, match="len_q == len_k"):                   # the reference's one accident is refused too
            _mha(**kw).forward_cross(z(1, 2, 32), z(1, 33, 32), z(1, 33, 32))
    with pytest.raises(RuntimeError, match="window_size"):
        _mha(relative_pe_2D=True, window_size=4).forward_cross(z(1, 10, 32), z(1, 10, 32), z(1, 10, 32))
    with pytest.raises(ValueError, match="relative position index"):
        _mha(relative_pe=True, window_size=4, window_depth=3).forward_cross(z(1, 50, 32), z(1, 50, 32), z(1, 50, 32))
    with pytest.raises(NotImplementedError, match="PackedAct"):
        mha.forward_cross(PackedAct(torch.zeros(8, dtype=torch.bfloat16), (1, 5, 32)), z(1, 7, 32), z(1, 7, 32))
    with pytest.raises(RuntimeError, match="not on a HIP device.*no CPU fallback"):
        mha.forward_cross(z(1, 5, 32), z(1, 7, 32), z(1, 7, 32))
    with pytest.raises(RuntimeError, match="not on a HIP device.*no CPU fallback"):
        _mha(relative_pe=True, window_size=4, window_depth=3).forward_cross(z(1, 49, 32), z(1, 49, 32), z(1, 49, 32))
    with pytest.raises(ValueError):                                                 # a mask that does not broadcast: checked with the shapes
        mha.forward_cross(z(1, 5, 32), z(1, 7, 32), z(1, 7, 32), mask=torch.ones(7, 5))


def test_forward_still_refuses_cross_attention():
    mha = _mha()
    x = torch.zeros(1, 5, 32)
    with pytest.raises(NotImplementedError, match="self-attention"):
        mha(x, x.clone(), x)


def test_few_query_max_is_declared_exported_and_the_version_stays(lib):
    from lstc_vad_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    assert re.search(r"\bint\s+lstc_sdpa_few_query_max\s*\(\s*void\s*\)\s*;", hdr)
    assert "lstc_sdpa_few_query_max" in _lib.EXPORTS
    assert 1 <= lib.lstc_sdpa_few_query_max() <= 16
    assert lib.lstc_version() == 112


SAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <stdint.h>
#include "lstc_hip.h"
/* what the launcher's translation unit expects from the rest of the library in a host-only build */
extern "C" const char FATBIN_SYMBOL[1024] = {0};
const uint64_t* lstc_seed_dev_current() { return nullptr; }
static LstcSdpaDesc good(void) {
    LstcSdpaDesc d; memset(&d, 0, sizeof d);
    d.N = 2; d.H = 2; d.Sq = 3; d.Sk = 17; d.dk = 64; d.dv = 32;
    d.q_sn = 2 * 3 * 64; d.q_sh = 3 * 64; d.q_st = 64; d.k_sn = 2 * 17 * 64; d.k_sh = 17 * 64; d.k_st = 64;
    d.v_sn = 2 * 17 * 32; d.v_sh = 17 * 32; d.v_st = 32; d.o_sn = 2 * 3 * 32; d.o_sh = 3 * 32; d.o_st = 32;
    d.scale = 0.125f; d.dropout_p = 0.2f;
    return d;
}
int main(void) {
    int bad = 0;
    LstcSdpaDesc d = good();                       /* a good descriptor on NULL device pointers: refused before any launch */
    LstcAttnMask m; memset(&m, 0, sizeof m);
    bad += lstc_sdpa_fwd(&d, NULL, NULL) != LSTC_E_NULL;
    bad += lstc_sdpa_bwd(&d, NULL, NULL) != LSTC_E_NULL;
    bad += lstc_sdpa_fwd(NULL, NULL, NULL) != LSTC_E_NULL;
    bad += lstc_sdpa_bwd(NULL, &m, NULL) != LSTC_E_NULL;
    static float buf[16];                          /* never dereferenced: every call below fails a host check */
    d.Q = d.K = d.V = buf; d.O = buf; d.probs = buf; d.dO = buf; d.dQ = d.dK = d.dV = buf;
    bad += lstc_sdpa_fwd(&d, &m, NULL) != LSTC_E_NULL;      /* a mask struct without bytes */
    bad += lstc_sdpa_bwd(&d, &m, NULL) != LSTC_E_NULL;
    LstcSdpaDesc e = d; e.Sq = 0;
    bad += lstc_sdpa_fwd(&e, NULL, NULL) != LSTC_E_SHAPE;
    e = d; e.k_st = -1;
    bad += lstc_sdpa_bwd(&e, NULL, NULL) != LSTC_E_SHAPE;
    e = d; e.v_sh = 0;
    bad += lstc_sdpa_bwd(&e, NULL, NULL) != LSTC_E_SHAPE;
    e = d; e.dropout_p = 1.5f;
    bad += lstc_sdpa_fwd(&e, NULL, NULL) != LSTC_E_SHAPE;
    e = d; e.dk = 24;
    bad += lstc_sdpa_fwd(&e, NULL, NULL) != LSTC_E_RANGE;
    e = d; e.Sk = 513;
    bad += lstc_sdpa_bwd(&e, NULL, NULL) != LSTC_E_RANGE;
    e = d; e.Sq = 1; e.N = 1 << 20; e.H = 1 << 12;
    bad += lstc_sdpa_fwd(&e, NULL, NULL) != LSTC_E_RANGE;
    int fq = lstc_sdpa_few_query_max();
    bad += !(fq >= 0 && fq <= 16);
    printf("few_query_max %d bad %d\n", fq, bad);
    return bad;
}
"""


def test_sdpa_launcher_host_side_is_clean_under_asan_and_ubsan(tmp_path):
    """The host half of csrc/attention_x.hip (the argument checks and the dispatch of both kernel families) compiled host-only
    with -fsanitize=address,undefined and linked with a small ``main`` that calls the entry points with bad descriptors and with
    a good one on NULL device pointers.  A stand-alone program: no GPU, nothing launched, nothing loaded into python."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc absent")
    # the sanitizer runtimes are linked statically into the program: it needs nothing from its environment
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libsan"]
    obj = tmp_path / "attention_x_host.o"
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-ffp-contract=off",
                    *[a for f in san for a in ("-Xarch_host", f)], "-I", os.path.join(ROOT, "include"), "-c",
                    os.path.join(ROOT, "lstc_vad_amd", "csrc", "attention_x.hip"), "-o", str(obj)], check=True, timeout=600)
    # a host-only object refers to its (absent) device image by a generated name: the program supplies an empty one
    syms = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    fatbin = re.search(r"\bU (__hip_fatbin_\w+)", syms).group(1)
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN.replace("FATBIN_SYMBOL", fatbin))
    exe = tmp_path / "sdpa_args"
    main_obj = tmp_path / "main.o"
    subprocess.run([hipcc, *san, "-x", "c++", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(main_obj)], check=True,
                   timeout=600)
    subprocess.run([hipcc, *san, str(main_obj), str(obj), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)      # the environment is left as it is
    assert r.returncode == 0 and "bad 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
