"""Rectangular-attention parity cases, shared by make_golden_sdpa.py (reference side) and tests/test_sdpa_gpu.py /
tests/test_sdpa_host.py.  The reference's ``ScaledDotProductAttention`` (models/MultiHeadAttention.py:9-23) runs in ``eval()`` on
q [N, H, len_q, d_k], k [N, H, len_k, d_k], v [N, H, len_k, d_v] with len_q != len_k: a single query, queries longer and shorter
than the keys, d_k != d_v, no mask, key-padding masks and dense [N, 1, len_q, len_k] masks that hold one fully masked row; bool
and float masks.  Inputs come from ``lstc_vad_amd.synthetic`` on both sides."""
import numpy as np

H = 2

SDPA_CASES = {
    # name: sequences, len_q, len_k, d_k, d_v, mask kind and its parameters, mask dtype, seed
    "sdpa_1x49_pad": dict(N=2, Sq=1, Sk=49, dk=64, dv=64, kind="padding", lengths=(49, 20), dtype="float32", seed=81),
    "sdpa_49x17_rows": dict(N=2, Sq=49, Sk=17, dk=64, dv=32, kind="rows", dead_row=(1, 20), dtype="float32", seed=82),
    "sdpa_17x145": dict(N=2, Sq=17, Sk=145, dk=32, dv=64, kind="none", dtype=None, seed=83),
    "sdpa_145x49_pad": dict(N=2, Sq=145, Sk=49, dk=64, dv=64, kind="padding", lengths=(33, 49), dtype="bool", seed=84),
    "sdpa_200x333_rows": dict(N=1, Sq=200, Sk=333, dk=16, dv=48, kind="rows", dead_row=(0, 131), dtype="bool", seed=85),
}


def build_mask(case):
    """The case's mask as a numpy array of its dtype, or None: [N, 1, 1, len_k] (padding: keys >= lengths[n] masked) or
    [N, 1, len_q, len_k] (rows: about 30 % of the positions masked by a fixed arithmetic pattern, query row ``dead_row = (n, i)``
    masked entirely).  Kept entries of a float mask are 1.0 or 0.5: any non-zero value keeps."""
    N, Sq, Sk = case["N"], case["Sq"], case["Sk"]
    if case["kind"] == "none":
        return None
    if case["kind"] == "padding":
        keep = np.arange(Sk)[None, :] < np.asarray(case["lengths"])[:, None]
        keep = keep.reshape(N, 1, 1, Sk)
    else:
        n, i, j = np.meshgrid(np.arange(N), np.arange(Sq), np.arange(Sk), indexing="ij")
        keep = ((i * 37 + j * 101 + n * 53 + (i * j) % 7) % 10) >= 3
        dn, di = case["dead_row"]
        keep[dn, di, :] = False
        keep = keep.reshape(N, 1, Sq, Sk)
    if case["dtype"] == "bool":
        return keep
    j = np.arange(Sk).reshape(1, 1, 1, Sk)
    return np.where(keep, np.where(j % 2 == 0, 1.0, 0.5), 0.0).astype(case["dtype"])


def build_inputs(case):
    """q, k, v uniform in [-1, 1] and the fixed weights w of the objective sum(output * w), in [-1, 1] / output.size."""
    from lstc_vad_amd import synthetic as syn
    N, Sq, Sk, dk, dv, seed = (case[f] for f in ("N", "Sq", "Sk", "dk", "dv", "seed"))
    q = syn.small_uniform((N, H, Sq, dk), seed, 1, 1.0)
    k = syn.small_uniform((N, H, Sk, dk), seed, 2, 1.0)
    v = syn.small_uniform((N, H, Sk, dv), seed, 3, 1.0)
    w = (syn.small_uniform((N, H, Sq, dv), seed, 4, 1.0) / float(N * H * Sq * dv)).astype(np.float32)
    return q, k, v, w
