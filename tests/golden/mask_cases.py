"""Attention-mask parity cases, shared by make_golden_mask.py (reference side) and tests/test_attn_mask_gpu.py /
tests/test_attn_mask_host.py.  The reference ``Encoder`` runs with ``src_mask`` (models/MultiHeadAttention.py:105-106:
``attn.masked_fill(mask == 0, -1e9)`` before the relative bias and the softmax) at S = 49 (short kernels here) and S = 145
(key-tiled kernels), once with a key-padding mask of a different length per sequence and once with an [N, 1, S, S] mask that
holds one fully masked row; one ``bool`` and one float mask at each length.  Weights come from ``cases.fill_params`` and inputs
from ``lstc_vad_amd.synthetic`` on both sides (|bias table| <= 0.5, so -1e9f + bias is -1e9f)."""
import numpy as np

ENC_KW = dict(n_layers=2, d_model=32, n_head=2, d_k=16, d_v=16, d_inner=64, MHA_layerNorm=True, FFN_layerNorm=True,
              relative_pe=True, window_size=4)

MASK_CASES = {
    # name: window_depth (S = 16 * depth + 1), sequences, mask kind, its parameters, mask dtype, seed
    "mask_s49_pad": dict(window_depth=3, N=3, kind="padding", lengths=(49, 31, 17), dtype="bool", seed=71),
    "mask_s49_rows": dict(window_depth=3, N=3, kind="rows", dead_row=(1, 20), dtype="float32", seed=72),
    "mask_s145_pad": dict(window_depth=9, N=2, kind="padding", lengths=(145, 100), dtype="float32", seed=73),
    "mask_s145_rows": dict(window_depth=9, N=2, kind="rows", dead_row=(1, 77), dtype="bool", seed=74),
}


def seq_len(case):
    return 16 * case["window_depth"] + 1


def encoder_kw(case):
    return dict(ENC_KW, window_depth=case["window_depth"], MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0,
                weight_init=True)


def build_mask(case):
    """The case's mask as a numpy array of its dtype: [N, 1, 1, S] (padding: keys >= lengths[n] masked) or [N, 1, S, S] (rows:
    about 30 % of the positions masked by a fixed arithmetic pattern, query row ``dead_row = (n, i)`` masked entirely).  Kept
    entries of a float mask are 1.0 or 0.5: any non-zero value keeps."""
    N, S = case["N"], seq_len(case)
    if case["kind"] == "padding":
        keep = np.arange(S)[None, :] < np.asarray(case["lengths"])[:, None]
        keep = keep.reshape(N, 1, 1, S)
    else:
        n, i, j = np.meshgrid(np.arange(N), np.arange(S), np.arange(S), indexing="ij")
        keep = ((i * 37 + j * 101 + n * 53 + (i * j) % 7) % 10) >= 3
        dn, di = case["dead_row"]
        keep[dn, di, :] = False
        keep = keep.reshape(N, 1, S, S)
    if case["dtype"] == "bool":
        return keep
    j = np.arange(S).reshape(1, 1, 1, S)
    return np.where(keep, np.where(j % 2 == 0, 1.0, 0.5), 0.0).astype(case["dtype"])
