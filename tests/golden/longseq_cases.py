"""Long-sequence parity cases (S = 16 L + 1 > 128: the key-tiled attention core, csrc/attention_long.hip), shared by
make_golden_longseq.py (reference side) and tests/test_longseq_gpu.py.  Same shape of entries as cases.py / cases.FULL_CASES."""

LONG_CASES = {
    # ShanghaiTech with a 9-clip temporal window: S = 9 * 16 + 1 = 145, 3-D bias table [(2*9-1) * 49, 2]
    "ltn_sht_long": ("LTN", dict(d_model=32, n_head=2, d_k=16, d_v=16, d_inner=64, MHA_layerNorm=True, FFN_layerNorm=True,
                                 relative_pe=True, window_size=4, window_depth=9),
                     dict(batch_size=2, part_num=2, part_len=9, n_patch=16)),
    # UCF (9 patches) with a 16-clip window: S = 16 * 9 + 1 = 145; the index is built for window_depth * 4 * 4 = 256 tokens and
    # read as its top-left 144 x 144 block (models/MultiHeadAttention.py:107-111) - index row stride 256 != S - 1
    "ltn_ucf_long": ("LTN", dict(d_model=32, n_head=2, d_k=16, d_v=16, d_inner=64, MHA_layerNorm=True, FFN_layerNorm=True,
                                 relative_pe=True, window_size=4, window_depth=16),
                     dict(batch_size=2, part_num=2, part_len=16, n_patch=9)),
    # d_k = d_v = 32 at S = 16 * 16 + 1 = 257
    "ltn_long_dk32": ("LTN", dict(d_model=32, n_head=2, d_k=32, d_v=32, d_inner=48, MHA_layerNorm=True, FFN_layerNorm=True,
                                  relative_pe=True, window_size=4, window_depth=16),
                      dict(batch_size=1, part_num=2, part_len=16, n_patch=16)),
}

# production head width at S = 145: batch 1 x 16 parts -> 32 sequences, 4 640 tokens (samples, norms, eval scores kept)
LONG_FULL_CASES = {
    "ltn_long_full": ("LTN", dict(d_model=2048, n_head=8, d_k=256, d_v=256, d_inner=4096, MHA_layerNorm=True,
                                  FFN_layerNorm=True, relative_pe=True, window_size=4, window_depth=9),
                      dict(batch_size=1, part_num=16, part_len=9, n_patch=16), 41),
}
