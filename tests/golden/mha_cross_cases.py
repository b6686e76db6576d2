"""Cross-attention parity cases, shared by make_golden_mha_cross.py (reference side) and tests/test_mha_cross_gpu.py /
tests/test_mha_cross_host.py.  The reference's ``MultiHeadAttention`` (models/MultiHeadAttention.py:93-132) runs as
``m(q, k, v, mask=..., return_attn=True)`` with both dropout rates 0, H = 2, d_model = 64, on three inputs whose lengths differ
(one query, a few queries, the general rectangular case, both lengths past 128) or agree (the relative biases need that).
Weights come from ``cases.fill_params`` and inputs from ``lstc_vad_amd.synthetic`` on both sides; the masks are
``sdpa_cases.build_mask``'s."""
import numpy as np

from sdpa_cases import build_mask  # noqa: F401  (re-exported: the case dicts carry its fields)

H, D_MODEL = 2, 64

MHA_CROSS_CASES = {
    # name: sequences, len_q, len_k, d_k, d_v, LayerNorm, one tensor as k and v, bias kind and window, mask kind / parameters / dtype
    "mha_cross_1x49_pad": dict(N=2, Sq=1, Sk=49, dk=32, dv=32, layer_norm=True, shared_kv=False, bias=None,
                               kind="padding", lengths=(49, 20), dtype="float32", seed=91),
    "mha_cross_5x17": dict(N=2, Sq=5, Sk=17, dk=32, dv=16, layer_norm=True, shared_kv=True, bias=None,
                           kind="none", dtype=None, seed=92),
    "mha_cross_16x145_rows": dict(N=2, Sq=16, Sk=145, dk=32, dv=32, layer_norm=True, shared_kv=False, bias=None,
                                  kind="rows", dead_row=(1, 9), dtype="bool", seed=93),
    "mha_cross_49x17_rows": dict(N=2, Sq=49, Sk=17, dk=32, dv=32, layer_norm=False, shared_kv=False, bias=None,
                                 kind="rows", dead_row=(1, 20), dtype="float32", seed=94),
    "mha_cross_145x200": dict(N=1, Sq=145, Sk=200, dk=32, dv=32, layer_norm=True, shared_kv=True, bias=None,
                              kind="none", dtype=None, seed=95),
    "mha_cross_49x49_bias": dict(N=2, Sq=49, Sk=49, dk=32, dv=32, layer_norm=True, shared_kv=True, bias="3d", window_size=4,
                                 window_depth=3, kind="none", dtype=None, seed=96),
    "mha_cross_145x145_bias_pad": dict(N=2, Sq=145, Sk=145, dk=32, dv=32, layer_norm=True, shared_kv=False, bias="3d", window_size=4,
                                       window_depth=9, kind="padding", lengths=(145, 100), dtype="bool", seed=97),
    "mha_cross_17x17_bias2d": dict(N=2, Sq=17, Sk=17, dk=32, dv=32, layer_norm=True, shared_kv=False, bias="2d", window_size=4,
                                   window_depth=3, kind="none", dtype=None, seed=98),
}


def module_kw(case):
    """Constructor arguments of ``MultiHeadAttention`` (the reference's and the build's take the same)."""
    kw = dict(n_head=H, d_model=D_MODEL, d_k=case["dk"], d_v=case["dv"], layerNorm=case["layer_norm"], attn_dropout=0.0,
              fc_dropout=0.0)
    if case["bias"] == "3d":
        kw.update(relative_pe=True, window_size=case["window_size"], window_depth=case["window_depth"])
    elif case["bias"] == "2d":
        kw.update(relative_pe_2D=True, window_size=case["window_size"])
    return kw


def build_inputs(case):
    """q [N, len_q, d_model], k, v [N, len_k, d_model] uniform in [-1, 1] (``v is k`` where the case shares them) and the fixed
    weights w of the objective sum(out * w), in [-1, 1] / out.size."""
    from lstc_vad_amd import synthetic as syn
    N, Sq, Sk, seed = (case[f] for f in ("N", "Sq", "Sk", "seed"))
    q = syn.small_uniform((N, Sq, D_MODEL), seed, 1, 1.0)
    k = syn.small_uniform((N, Sk, D_MODEL), seed, 2, 1.0)
    v = k if case["shared_kv"] else syn.small_uniform((N, Sk, D_MODEL), seed, 3, 1.0)
    w = (syn.small_uniform((N, Sq, D_MODEL), seed, 4, 1.0) / float(N * Sq * D_MODEL)).astype(np.float32)
    return q, k, v, w
