"""Cost of an attention mask: the masked first-generation (S <= 128) and key-tiled (S > 128) kernels against the same kernels
unmasked, interleaved in one process with torch events (a sibling of tools/attn_time.py; H = 8, d_k = d_v = 256, dropout 0.2).

    python tools/attn_mask_time.py [> profiles/attn_mask_timing.txt]

Forms per shape: no mask (``variant = 1``: the first-generation kernels below S = 128 too), a key-padding mask
[N, 1, 1, S] (S bytes per sequence) and a dense [N, 1, S, S] byte mask (a quarter of the bytes of the P write), and a key-padding mask that keeps every key (the
masked code on unmasked data).  Best of three
interleaved rounds of 5 launches each; "no mask (again)" repeats the unmasked launches in every round and shows the box's spread."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import functional as Fn                                              # noqa: E402
from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d          # noqa: E402

dev = "cuda"
H, dk = 8, 256


def timed(fn, n=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, r


Fn._ATTN_VARIANT = 1
for N, S in ((2048, 49), (2048, 128), (256, 512)):
    L = -(-(S - 1) // 16)
    M = N * S
    g = torch.Generator(device=dev).manual_seed(S)
    q, k, v, do = (torch.randn(M, H * dk, device=dev, generator=g) for _ in range(4))
    idx = relative_position_index_3d(L, 4).to(dev)
    tab = torch.randn((2 * L - 1) * 49, H, device=dev, generator=g) * 0.1
    lengths = S - torch.arange(N) % max(1, S // 4)
    forms = {
        "no mask": None,
        "key padding [N,1,1,S]": Fn.attn_mask_arg((torch.arange(S)[None, :] < lengths[:, None]).view(N, 1, 1, S), N, H, S, device=dev),
        "dense [N,1,S,S]": Fn.attn_mask_arg(torch.rand(N, 1, S, S) >= 0.3, N, H, S, device=dev),
        "key padding, all kept": Fn.attn_mask_arg(torch.ones(N, 1, 1, S, dtype=torch.bool), N, H, S, device=dev),
        "no mask (again)": None,            # the same launches once more per round: the spread of this box
    }
    best = {name: [1e9, 1e9] for name in forms}
    for rnd in range(3):
        for name, m in forms.items():
            tf, (o, p) = timed(lambda: Fn.attn_fwd(q, k, v, N, S, H, dk, dk, tab, idx, 0.2, 7, mask=m))
            tb, _ = timed(lambda: Fn.attn_bwd(do, q, k, v, p, N, S, H, dk, dk, tab, idx, 0.2, 7, mask=m))
            best[name] = [min(best[name][0], tf), min(best[name][1], tb)]
            del o, p
    f0, b0 = best["no mask"]
    for name, (tf, tb) in best.items():
        print(f"ATTN-MASK N={N} S={S} H={H} d={dk} {name:24s} fwd {tf:8.3f} ms ({tf / f0:5.3f}x)  bwd {tb:8.3f} ms ({tb / b0:5.3f}x)", flush=True)
    del q, k, v, do
    torch.cuda.empty_cache()
