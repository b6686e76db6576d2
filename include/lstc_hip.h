/*
 * lstc_hip.h — C ABI of liblstc_hip.so, the MI355X (gfx950) native kernels behind the
 * LSTC_VAD training hot path.
 *
 * The reference (shengyangsun/LSTC_VAD) has no FFI / plugin layer: its hot path is the
 * Python class surface models.Encoder / MultiHeadAttention / FFN / Regressor / Classifier
 * plus the loss functions and torch.optim.Adagrad inside the Train/ scripts, all of it implicit
 * ATen kernels.  Each entry point below replaces the ATen work of the reference lines it
 * cites (paths relative to the reference root).  lstc_vad_amd/_lib.py binds them with
 * ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.
 *  - Every buffer is owned by the caller (PyTorch allocates); the library never allocates
 *    or frees device memory and keeps no pointer after return.
 *  - Asynchronous on the given HIP stream (hipStream_t passed as void*); no internal sync.
 *  - Return 0 on success; <0 = argument/shape error detected on the host before launch
 *    (LSTC_E_*); >0 = hipError_t from the launch.  lstc_strerror() names either.
 *  - All matrices are row-major; "ld" = leading dimension in elements.
 */
#ifndef LSTC_HIP_H
#define LSTC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSTC_VERSION 112            /* 0.1.1 patch 2: see INTEGRATION.md, "ABI history" */

enum {
    LSTC_OK = 0,
    LSTC_E_NULL = -1,               /* required pointer is NULL */
    LSTC_E_SHAPE = -2,              /* non-positive / inconsistent dimension */
    LSTC_E_ALIGN = -3,              /* pointer / leading dimension breaks a documented alignment rule */
    LSTC_E_UNSUPPORTED = -4,        /* combination not implemented */
    LSTC_E_RANGE = -5               /* size exceeds a documented limit (e.g. sequence length, 32-bit indexing) */
};

enum { LSTC_F32 = 0, LSTC_BF16 = 1, LSTC_F32X3 = 2, LSTC_BF16P = 3 };

/* ----------------------------------------------------------------------------- GEMM
 * C[M,N] = epilogue( alpha * op(A)[M,K] * op(B)[K,N] )
 *   transA = 0: A stored [M,K] (K contiguous)      transA = 1: A stored [K,M] (M contiguous)
 *   transB = 0: B stored [K,N] (N contiguous)      transB = 1: B stored [N,K] (K contiguous)
 * Replaces every nn.Linear / torch.matmul-with-weights on the path:
 *   forward  X*W^T  (transA=0, transB=1): models/MultiHeadAttention.py:97-99,123; models/FFN.py:17;
 *                                         models/Regressor.py:19-20; models/Classifier.py:21-22
 *   backward dX = dY*W (0,0) and dW = dY^T*X (1,0): autograd of the above,
 *                                         Train/temporal_transformer_shanghaitech.py:138
 * Epilogue order (each stage optional, selected by `flags`):
 *   v = alpha*acc; v += bias[n]; v = relu(v); v = dropout(v); v += residual[m,n];
 *   v *= (relu_src[m,n] > 0); C = v   (or C += v with LSTC_EPI_ACCUM)
 * fusing  relu(W1 x + b1)            models/FFN.py:17
 *         dropout(W2 h + b2) + x     models/FFN.py:17-19
 *         dropout(fc(o)) + residual  models/MultiHeadAttention.py:123-124
 * Dropout keeps element i = m*N+n iff hash(seed, i) >= p*2^32 and scales kept values by
 * 1/(1-p); lstc_dropout_mask() / lstc_dropout_apply() regenerate the same mask.
 * dtype LSTC_F32: exact f32 MFMA (v_mfma_f32_32x32x2_f32) — bitwise an fmaf chain (acc = fmaf(a_k, b_k, acc) from 0, one rounding per
 *   term), NOT in ascending k: inside every 32-deep K tile the order is 0, 16, 1, 17, ... 7, 23, 8, 24, ... 15, 31 (the two lane
 *   halves of an issue hold k = j and k = 16 + j, the lower half is added first).  Every variant, tile size and the row split share
 *   that order, so they agree bit for bit (tests/test_gemm_f64_gpu.py compares each with that chain).
 * dtype LSTC_BF16: A, B, C stay f32 in memory; the operands are rounded to bf16 (RNE) while they are staged, f32 accumulate, C and
 *   the epilogue f32 (csrc/gemm_bf16c.hip).  There is no bf16 output: LSTC_EPI_OUT_F32 is accepted and changes nothing.
 * dtype LSTC_F32X3: f32-accurate product on the 16-bit matrix cores (3 f16 plane products per f32 product); A and B are PACKED operands produced by lstc_pack3
 *   (lda/ldb ignored).  (transA, transB) = (0, 1): packs of the [M,K] and [N,K] matrices (lstc_pack3 transposes k-major
 *   sources on the way).  (1, 0): packs of the k-major SOURCES [K,M] and [K,N] themselves - the weight-gradient product
 *   dY^T X reuses the packs the forward / input-gradient products made of X and dY; needs M, N, K multiples of 128.
 *   C, bias, residual, relu_src and the epilogue are f32 exactly as for LSTC_F32; no batch.
 * dtype LSTC_BF16P: the LSTC_BF16 arithmetic (operands rounded to bf16 RNE, f32 accumulate, f32 C / epilogue) on PACKED bf16
 *   operands produced by lstc_pack1 (lda/ldb ignored): 2 B per element through L2/LDS instead of 4, streamed by LDS-DMA into
 *   a 256x256x64-tile kernel (csrc/gemm_bf16p.hip).  (0, 1): packs of [M,K] and [N,K];  (1, 0): packs of the k-major SOURCES
 *   [K,M] and [K,N] (weight gradient dY^T X reusing the packs of dY and X; K must be a multiple of 128).  No batch.
 */
enum {
    LSTC_EPI_BIAS = 1, LSTC_EPI_RELU = 2, LSTC_EPI_DROPOUT = 4, LSTC_EPI_RESIDUAL = 8,
    LSTC_EPI_RELU_MASK = 16, LSTC_EPI_ACCUM = 32, LSTC_EPI_OUT_F32 = 64,
    /* LSTC_BF16P only, (0, 1) form, M and N multiples of 256, no K split (else LSTC_E_UNSUPPORTED):
     *   OUT_PACK:       C is an lstc_pack1 buffer (lstc_pack1_bytes(M, N)) that receives the result rounded to bf16 in the layout
     *                   of a packed [M, N] operand - the output of W1 (models/FFN.py:17) IS the A operand of W2 and of dW2, and
     *                   the gradient of that hidden IS the operand of dW1 / dX: no f32 copy, no lstc_pack1 pass (ldc ignored);
     *   RELU_MASK_PACK: relu_src is such a pack (the hidden's sign is read from its bf16 form; ld_relu ignored);
     *   RESIDUAL_PACK:  residual is such a pack of [M, N] (ldr ignored; with RESIDUAL and OUT_PACK, never with RELU_MASK): the
     *                   bf16 activation stream - dropout(fc(o)) + x (models/MultiHeadAttention.py:123-124), dropout(W2 h + b2) + x
     *                   (models/FFN.py:17-19) and the input gradients dX + dy read their residual as 2 bytes per element from
     *                   the pack the previous block's LayerNorm wrote and leave 2 bytes per element for the next one. */
    LSTC_EPI_OUT_PACK = 128, LSTC_EPI_RELU_MASK_PACK = 256, LSTC_EPI_RESIDUAL_PACK = 512
};

#define LSTC_VARIANT_NO_QTAIL (1 << 30)

typedef struct LstcGemmDesc {
    int32_t M, N, K;
    int32_t lda, ldb, ldc;
    int32_t transA, transB;
    int32_t dtype;                  /* LSTC_F32 | LSTC_BF16 */
    int32_t flags;                  /* LSTC_EPI_* */
    float   alpha;
    float   dropout_p;
    uint64_t dropout_seed;
    int32_t ldr;                    /* residual leading dimension */
    int32_t ld_relu;                /* relu_src leading dimension */
    int32_t split_k;                /* 0/1 = none; >1: K split over workgroups, partial sums added with f32 atomics
                                       into C, which the caller must have zeroed (only alpha epilogue allowed).
                                       LSTC_F32X3 with batch_stride_c != 0: split z writes its partial product to
                                       C + z*batch_stride_c instead (no atomics; the caller sums the partials) */
    int32_t variant;                /* 0 = library default tile (LSTC_F32: 128x128 tiles, one tile per workgroup, with the rows of a
                                       mostly empty last tile round on the 64x64 variant - bit-identical results; the default NEVER
                                       selects the persistent kernel); LSTC_F32 in the production library: 4 = the default loop
                                       without the row split, 8 = its fallback for unaligned operands (scalar epilogue: the
                                       reference of the bitwise tests), 11 = the 64x64 tail tile, 12 = the persistent walk of the
                                       default loop (bit-identical, measured slower); anything else -> LSTC_E_UNSUPPORTED.
                                       LSTC_F32X3: 0 = 3 = the 128x128 two-stage kernel (256x128 tiles for long weight gradients),
                                       2 = the 256x128-tile kernel; anything else -> LSTC_E_UNSUPPORTED.
                                       LSTC_BF16P: 0, or LSTC_VARIANT_NO_QTAIL = the product as ONE persistent launch of 256 x 256 tiles,
                                       without the quarter-tile kernel that otherwise takes the tiles behind the last whole round of
                                       workgroups (bit-identical results: the reference of the bitwise tests) */
    int32_t batch;                  /* 0/1 = single problem; >1: `batch` independent problems of identical shape, problem z
                                       uses A + z*batch_stride_a etc. (elements).  Per-head products of the last layer's
                                       CLS attention (q_h W_k,h etc.).  Only alpha / ACCUM epilogues. */
    int64_t batch_stride_a, batch_stride_b, batch_stride_c;
    const void* A;
    const void* B;
    void*       C;
    const float* bias;              /* [N] */
    const void*  residual;          /* [M,ldr], same dtype as C */
    const void*  relu_src;          /* [M,ld_relu], same dtype as C */
} LstcGemmDesc;

int lstc_gemm(const LstcGemmDesc* d, void* stream);

/* Number of K slices lstc_gemm actually launches for (dtype, K, split_k): ceil(kt / ceil(kt / split_k)) with kt = K tiles
 * of that dtype's kernel.  It can be SMALLER than split_k (e.g. 132 K tiles, split_k 16 -> 15 slices of 9 tiles), so a
 * caller that gives each slice its own partial output (batch_stride_c) must size and sum exactly this many. */
int32_t lstc_gemm_splits(int32_t dtype, int32_t K, int32_t split_k);

/* Operand packing for LSTC_F32X3.  The tensor is scaled by the power of two s that puts its largest magnitude in
 * [2^14, 2^15) and written as 128-row x 32-k tiles (row = an output row of A's side or an output column of B's side, K = the
 * contraction); each tile = two 8-KB f16 planes h = f16(x s), l = f16(x s - h), stored in the LDS image layout the GEMM
 * streams with global_load_lds (csrc/gemm_pk.hip); rows and K are zero-padded to the tile; a 256-B trailer carries the
 * tensor's absmax bits and 1/s (the GEMM epilogue multiplies by 1/(s_a s_b)).  Three launches: memset, absmax, pack.
 *   k_major = 0: src is [rows, K] with K contiguous (ld >= K)  - X of X*W^T, W of X*W^T, dY of dY*W
 *   k_major = 1: src is [K, rows] with rows contiguous (ld >= rows) - W of dY*W (and dY, X of dY^T*X when the
 *                (1, 0) form of lstc_gemm is not applicable)
 * dst needs lstc_pack3_bytes(rows, K) bytes, 16-B aligned.  The same nn.Linear products as lstc_gemm (see above). */
int64_t lstc_pack3_bytes(int64_t rows, int64_t K);
int lstc_pack3(const float* src, int64_t rows, int64_t K, int64_t ld, int32_t k_major, void* dst, void* stream);

/* Operand packing for LSTC_BF16P: the logical [rows, K] operand rounded to bf16 (RNE) and stored as 128-row x 32-k tiles,
 * each tile the 8-KB LDS image the GEMM reads (64-B rows, 16-B chunk index XOR (row >> 2) & 3); rows and K are zero-padded
 * to an EVEN number of tiles each way.  k_major as for lstc_pack3.  One launch.  dst needs lstc_pack1_bytes(rows, K) bytes,
 * 16-B aligned.  Same nn.Linear products as lstc_gemm (models/MultiHeadAttention.py:97-99,123; models/FFN.py:17). */
int64_t lstc_pack1_bytes(int64_t rows, int64_t K);
int lstc_pack1(const float* src, int64_t rows, int64_t K, int64_t ld, int32_t k_major, void* dst, void* stream);
/* Several operands in ONE launch - the weights of a model after an optimizer step (models/MultiHeadAttention.py:97-99,123 and
 * models/FFN.py:17,19 each need their nn.Linear weight in both layouts: ~35 launches of 10-20 us otherwise).  Each item as
 * lstc_pack1's arguments; results are bit for bit those of `count` lstc_pack1 calls. */
typedef struct LstcPackItem {
    const float* src; int64_t rows, K, ld; int32_t k_major; void* dst;
} LstcPackItem;
int lstc_pack1_multi(const LstcPackItem* items, int32_t count, void* stream);
/* out[k] (+)= sum over rows of the packed [rows, K] operand (bf16 values added in f32; two passes through `partial`
 * [n_partial, K]): the bias gradient db1 = column sums of the hidden's gradient (autograd of models/FFN.py:17) when that
 * gradient exists only as the packed output of a LSTC_EPI_OUT_PACK product. */
int lstc_colsum_pack1(const void* packed, int64_t rows, int32_t K, float* partial, int32_t n_partial, float* out,
                      int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------ attention
 * Fused core of models/MultiHeadAttention.py:103-122 for one layer, all sequences, heads:
 *   A = (Q/sqrt(d_k)) K^T ; A[:, :, 1:, 1:] += table[index[i-1, j-1], h] ; P = softmax(A, -1) ;
 *   Pd = dropout(P) ; O = Pd V, written head-merged ([N, S, H*dv]).
 * Q, K, V are the projection outputs as the GEMM leaves them: [N, S, H*dk] (token-major, heads
 * interleaved) — the reference's transpose(1,2)/contiguous copies (:101,:122) disappear.
 * `probs` [N, H, S, S] receives P (pre-dropout) for the backward pass / return_attn.
 * rel-bias: `table` [n_rows, H] float, `index` int64 [index_ld-wide rows]; entry used for
 * (i, j), 1 <= i,j < S is table[index[(i-1)*index_ld + (j-1)], h] — the top-left (S-1)x(S-1)
 * block, exactly the reference's `relative_position_index[:len_q-1, :len_q-1]` slice (:108).
 */
typedef struct LstcAttnDesc {
    int32_t N, S, H, dk, dv;        /* S <= 128: the short kernels below.  128 < S <= 512: the key-tiled kernels
                                       (csrc/attention_long.hip) - row (not packed) inputs and outputs only (packed forms ->
                                       LSTC_E_UNSUPPORTED), probs_ld 0 or S (as for every row-input call: LSTC_E_UNSUPPORTED
                                       otherwise), in the backward a table gradient only as dtable_chunks > 0 partial tables
                                       (else LSTC_E_UNSUPPORTED); `variant` is ignored there.  dk or dv not a multiple of 16,
                                       per-wave bias tables past the LDS budget, and S > 512: LSTC_E_RANGE.  LSTC_BF16 there
                                       is currently SLOWER than LSTC_F32 */
    int32_t ldq, ldk, ldv, ldo;     /* token strides in elements (normally H*dk / H*dv) */
    int32_t dtype;                  /* LSTC_F32: every product on the exact-f32 MFMA.  LSTC_BF16 (bf16 training mode): the operands of
                                       Q K^T, Pd V and of the four backward products are rounded to bf16 (RNE) in registers and
                                       contracted by v_mfma_f32_32x32x16_bf16 with f32 accumulation; Q, K, V, O, probs and the
                                       gradients stay f32 in memory, softmax / bias / dropout stay f32.  Taken by the staged
                                       kernels (S <= 96, dk and dv multiples of 32, 16-B aligned Q, K, V, dO and row strides that
                                       are multiples of 4; forward: variant 0 or 2, backward: any variant but 1, and per-wave
                                       bias tables that fit the LDS budget) and by the
                                       key-tiled kernels (128 < S <= 512: K and Q*scale rounded in the forward, every operand
                                       of the backward products likewise); every other case (S <= 128 outside the staged
                                       kernels) computes the exact-f32 products (the first-generation loops are latency-bound
                                       and got slower with bf16 products).  lstc_attn_cls_* : LSTC_F32 only */
    int32_t index_ld;               /* 0 = no relative bias */
    int32_t table_rows;             /* rows of `table` / `dtable` (backward: size of the per-workgroup LDS accumulator) */
    float   scale;                  /* 1/sqrt(d_k): multiplies Q (reference divides by temperature :49,:103) */
    float   dropout_p;
    uint64_t dropout_seed;
    const void* Q; const void* K; const void* V;
    void*  O;
    float* probs;                   /* [N,H,S,S] f32 */
    const float*   table;           /* [rows, H] or NULL */
    const int64_t* index;           /* or NULL.  Precondition of the backward (not checked): within each row i of the (S-1) x
                                       (S-1) block read, distinct columns j map to distinct table rows - both backwards add
                                       the table gradient by a plain LDS read-modify-write covering many keys of one query
                                       per instruction.  Every index the models build satisfies it (relative offsets of
                                       distinct positions differ; tests/test_longseq_host.py checks each); a non-injective
                                       row loses updates */
    /* backward only */
    const void* dO;                 /* [N,S,H*dv] */
    void* dQ; void* dK; void* dV;   /* [N,S,H*dk|dv], written (not accumulated) */
    float* dtable;                  /* dtable_chunks == 0: [rows,H] accumulated with atomics, caller zeroes; NULL = skip.
                                       dtable_chunks > 0: [chunks][rows][H] partial tables, one per chunk of
                                       ceil(N/chunks) sequences, written (no atomics; the caller sums them - a
                                       fixed-order, bit-reproducible gradient) */
    int32_t dtable_chunks;
    int32_t variant;                /* S <= 96, row operands, no mask.  0 = default kernels; 1 = first-generation kernels
                                       (operands straight from global in MFMA lane layout) - kept for A/B measurements and as the
                                       fallback for what the staged kernels do not take (d_k or d_v not a multiple of 32, a Q, K,
                                       V or dO base off a 16-B boundary, a row stride that is no multiple of 4, 96 < S <= 128):
                                       there every value runs them.  Backward: every value but 1 runs the staged kernel where it
                                       applies and its per-wave bias tables fit the LDS (else the first generation).  Forward,
                                       d_k and d_v multiples of 32, T = ceil(S / 32):
                                         LSTC_F32, d_v % 64 == 0 and O 16-B aligned: 0 = the lane-=-query f32 kernel at T = 1 and
                                           3, the first generation at T = 2; 2 = the staged (LDS-logit) kernel at T = 1 and 3,
                                           the first generation at T = 2; 3 = the lane-=-query kernel at every T;
                                         LSTC_F32, any other d_v or an O base off a 16-B boundary (the lane-=-query kernel
                                           writes O as 16-B groups): 0 and 2 = the staged kernel at T = 1 and 3, the first
                                           generation at T = 2; 3 = the first generation;
                                         LSTC_BF16: 0 and 2 = the staged kernel (bf16 products) at every T; 3 = as 1.
                                       Same results to rounding throughout (A/B measurements).
                                       Packed-input forward only (in_pack_cols > 0): 100 + n = n sequences per workgroup
                                       (1 <= n <= 16; the default picks n from N * H), a measurement hook - results do not
                                       depend on it */
    /* backward, bf16 mode: when all three are non-NULL, dQ / dK / dV are written ONLY as packed bf16 operands [N*S, H*dk|dv]
     * (lstc_pack1 layout, lstc_pack1_bytes(N*S, H*dk|dv) bytes each; dQ / dK / dV may be NULL) - they feed the packed weight- and
     * input-gradient products of the projections (autograd of models/MultiHeadAttention.py:97-99).  Needs the staged kernel
     * (S <= 96, d_k, d_v multiples of 32), N*S a multiple of 256, H*dk and H*dv multiples of 64; else LSTC_E_UNSUPPORTED. */
    void* dQ_pack; void* dK_pack; void* dV_pack;
    /* pack_cols > 0: the three pointers name ONE pack of a [N*S, pack_cols] matrix (the fused Q|K|V projection's gradient) whose
     * columns dQ_col0 / dK_col0 / dV_col0 .. + H*dk|dv receive dQ / dK / dV (multiples of 32, pack_cols a multiple of 64). */
    int32_t pack_cols, dQ_col0, dK_col0, dV_col0;
    /* forward, bf16 mode: when non-NULL, O is written ONLY as a packed bf16 operand [N*S, H*dv] (O may be NULL) - it feeds the
     * packed products of the output projection fc (models/MultiHeadAttention.py:122-123) and of its weight gradient.  N*S a
     * multiple of 256, H*dv a multiple of 64, d_v a multiple of 32; else LSTC_E_UNSUPPORTED. */
    void* O_pack;
    /* bf16 mode, PACKED INPUTS (third-generation kernels): in_pack_cols > 0 says that Q, K, V point at lstc_pack1 buffers of
     * a [N*S, in_pack_cols] matrix - normally all three at ONE pack, the fused Q|K|V projection written with LSTC_EPI_OUT_PACK
     * (models/MultiHeadAttention.py:97-99) - whose columns Q_col0 / K_col0 / V_col0 .. + H*dk|dv hold the projections (multiples
     * of 32; in_pack_cols a multiple of 64); ldq / ldk / ldv are ignored.  Backward: dO_pack_cols > 0 likewise makes dO a pack of
     * [N*S, dO_pack_cols], columns dO_col0 .. + H*dv (the packed input gradient of fc, :123).  Packed inputs come with packed
     * outputs only: the forward needs O_pack, the backward dQ_pack / dK_pack / dV_pack and both packed inputs.  dtype LSTC_BF16,
     * S <= 96, d_k a multiple of 32, d_v of 64, N*S of 256; else LSTC_E_UNSUPPORTED.  No f32 copy of Q, K, V, O, dO, dQ, dK or dV
     * exists in this form: the attention core moves 2 bytes per element each way. */
    int32_t in_pack_cols, Q_col0, K_col0, V_col0;
    int32_t dO_pack_cols, dO_col0;
    /* row pitch of `probs` in floats: 0 or S = dense [N,H,S,S].  The packed-input kernels need a multiple of 4 with
     * S <= probs_ld <= 32 * ceil(S / 32) (`probs` 16-B aligned; LSTC_E_SHAPE otherwise): they move the probabilities as 16-B
     * groups of a row's 32 * ceil(S / 32) key columns, the forward writes zeros into the padding columns [S, probs_ld) and the
     * backward expects them there.  A wider pitch would hold columns neither kernel touches, so it is refused. */
    int32_t probs_ld;
} LstcAttnDesc;

int lstc_attn_fwd(const LstcAttnDesc* d, void* stream);
/* autograd of the above (dV = Pd^T dO; dPd = dO V^T; dA = P*(dP - rowsum(dP*P)); dQ = dA K*scale;
 * dK = dA^T Q*scale; dtable[index] += dA[1:,1:] summed over sequences). */
int lstc_attn_bwd(const LstcAttnDesc* d, void* stream);

/* CLS-query attention for the LAST encoder layer: only enc_output[:, 0, :] is consumed downstream
 * (Train/temporal_transformer_shanghaitech.py:123; Train/spatio_transformer_shanghaitech.py:97), so its queries are
 * needed for token 0 only while keys/values still span all S tokens (row 0 carries no relative bias:
 * models/MultiHeadAttention.py:111 adds it to attn[:, :, 1:, 1:]).  Same descriptor; Q/dQ/O/dO hold ONE row per
 * sequence ([N, ldq] / [N, ldo]) and probs is [N, H, S].  S <= 512 (LSTC_E_RANGE above); S <= 128 runs the original
 * instantiation unchanged.  (lstc_cls_dot / _wsum / _outer and their packed forms below keep S <= 128.) */
int lstc_attn_cls_fwd(const LstcAttnDesc* d, void* stream);
int lstc_attn_cls_bwd(const LstcAttnDesc* d, void* stream);

/* Attention masks (reference models/MultiHeadAttention.py:105-106: attn.masked_fill(mask == 0, -1e9) before the relative bias
 * and the softmax).  One byte per (n, h, query i, key j), read as mask[n*sn + h*sh + i*sq + j*sk]; a stride of 0 broadcasts
 * that axis, so a key-padding mask [N, 1, 1, S] is (S, 0, 0, 1) and costs S bytes per sequence.  The caller owns the extent:
 * every offset up to (N-1)*sn + (H-1)*sh + (S-1)*sq + (S-1)*sk must lie inside the buffer.
 *   forward : where the byte is 0 the logit is -1e9f IN PLACE OF the scaled q.k; the bias is added afterwards in f32 (for
 *             |bias| < 32 the sum rounds back to -1e9f).  In a row that keeps a key every masked key has probability exactly
 *             0.0; a fully masked row is uniform, 1/S in every column - no -inf, no NaN.  probs hold the masked P before dropout;
 *             the dropout index of (n, h, i, j) is unchanged.
 *   backward: dV and rowsum(dP' * P) are as unmasked (the saved P carries the mask); the dA that feeds dQ and dK is zero at
 *             masked positions, the dA that feeds dtable is not (it differs from zero only in fully masked rows).
 * Same descriptor as the unmasked calls, row operands only: O_pack, dQ_pack / dK_pack / dV_pack, in_pack_cols > 0 and
 * dO_pack_cols > 0 return LSTC_E_UNSUPPORTED.  S <= 128 runs the masked instantiation of the first-generation kernels (any d_k,
 * d_v, alignment; exact-f32 products for LSTC_BF16 too; `variant` is not consulted), 128 < S <= 512 that of the key-tiled kernels
 * (d_k, d_v multiples of 16, else LSTC_E_RANGE; LSTC_BF16 = bf16 products), the CLS forms row 0 of the mask (sq is not read).
 * m or m->mask NULL: LSTC_E_NULL; a negative stride: LSTC_E_SHAPE - all checked before any launch.  Results are
 * bit-reproducible run to run (fixed summation order, one writer per element, no float atomics with dtable_chunks > 0). */
typedef struct LstcAttnMask {
    const uint8_t* mask;            /* 0 = masked, non-zero = kept */
    int64_t sn, sh, sq, sk;         /* element strides over (n, h, query i, key j); 0 = broadcast */
} LstcAttnMask;
int lstc_attn_fwd_masked(const LstcAttnDesc* d, const LstcAttnMask* m, void* stream);
int lstc_attn_bwd_masked(const LstcAttnDesc* d, const LstcAttnMask* m, void* stream);
int lstc_attn_cls_fwd_masked(const LstcAttnDesc* d, const LstcAttnMask* m, void* stream);   /* query row 0: sq is ignored */
int lstc_attn_cls_bwd_masked(const LstcAttnDesc* d, const LstcAttnMask* m, void* stream);

/* Attention over sequence offsets: an UNPADDED batch (same reference lines as lstc_attn_fwd, models/MultiHeadAttention.py:97-122,
 * applied to every sequence on its own length).  The tokens of all sequences lie back to back: Q, K, V, O (and dO, dQ, dK, dV) are
 * [M, ld] token-major as the projection GEMMs leave them, sequence n = rows row0[n] .. row0[n+1] - 1 (S_n tokens, CLS first).  The
 * probabilities are ragged: sequence n owns H * S_n * S_n floats [H, S_n, S_n] from probs + prob0[n].  A call covers the n_ids
 * sequences seq_ids[0 .. n_ids) (seq_ids NULL: sequences 0 .. n_ids - 1) in ONE launch whose LDS tile is sized by d->S, the
 * longest sequence of the call: callers bucket the sequences by ceil(S_n / 32) and call once per bucket.
 *   Structure and arithmetic are those of the first-generation kernels (csrc/attention.hip, attn_fwd_kernel / attn_bwd_kernel with
 *   VAR): exact-f32 products in every dtype, any d_k, d_v and alignment, no mask.  The relative bias of token pair (i, j), i, j >= 1,
 *   is table[index[(i-1)*index_ld + (j-1)], h]: a shorter sequence reads the top-left corner of the index alone.
 *   Dropout: the counter of element (n, h, i, j) is its offset prob0[n] + (h*S_n + i)*S_n + j in the ragged buffer, so
 *   lstc_dropout_mask() over that buffer with the same seed regenerates the mask.
 *   Backward: one workgroup per (chunk of the call's sequences, head); dtable is written as d->dtable_chunks partial tables
 *   [chunks, table_rows, H] (the caller sums them in a fixed order): dtable non-NULL needs dtable_chunks > 0, else
 *   LSTC_E_UNSUPPORTED.  There are no float atomics.
 * One writer per output element; its value depends neither on the bucketing nor on the other sequences of the batch.
 * Device offsets are trusted, except that S_n is clamped to [1, 32 * ceil(d->S / 32)] for the LDS tile.  d->N is not read.
 * Checked before any launch: d, s, row0, prob0, Q, K, V, probs, O (forward), dO / dQ / dK / dV (backward) NULL: LSTC_E_NULL;
 * any packed operand or output of the descriptor: LSTC_E_UNSUPPORTED; d->S > 128 or n_probs > 2^32 - 1 (the dropout counter is
 * 32 bits): LSTC_E_RANGE; n_ids <= 0, n_probs < 0 or a chunk count that does not match dtable_chunks: LSTC_E_SHAPE. */
typedef struct LstcSeqs {
    const int32_t* row0;            /* device int32 [N + 1]: first row of every sequence, row0[N] = M */
    const int64_t* prob0;           /* device int64 [N + 1]: first float of every sequence's probabilities, prob0[N] = n_probs */
    const int32_t* seq_ids;         /* device int32 [n_ids]: the sequences of this call; NULL = 0 .. n_ids - 1 */
    int32_t n_ids;
    int64_t n_probs;                /* floats in the ragged probabilities buffer */
} LstcSeqs;
int lstc_attn_var_fwd(const LstcAttnDesc* d, const LstcSeqs* s, void* stream);
int lstc_attn_var_bwd(const LstcAttnDesc* d, const LstcSeqs* s, void* stream);

/* The same over sequences of up to 512 tokens: 128 < d->S <= 512, d->S again the longest sequence of the call.  Everything the
 * comment above says about the offsets (row0, prob0, seq_ids), the ragged probabilities, the bias of a shorter sequence, the dropout
 * counter prob0[n] + (h*S_n + i)*S_n + j (lstc_dropout_mask() over the ragged buffer regenerates the mask), the partial bias tables
 * [dtable_chunks, table_rows, H] without float atomics and d->N holds here too.  One writer per output element; its value depends
 * neither on the bucketing nor on the other sequences of the batch.
 *   Structure and arithmetic are those of the key-tiled kernels (csrc/attention_long.hip, attn_long_fwd_kernel / attn_long_bwd_kernel
 *   with VAR): exact-f32 products in every dtype, no mask, with their preconditions: d_k and d_v multiples of 16, row operands and
 *   outputs, 32-bit offsets within a sequence (d->S * the largest row pitch < 2^31).  Forward: one wave per (sequence, head, 32-query
 *   block) with the block count of d->S; the waves behind a shorter sequence's end return at once.  Backward: one workgroup per
 *   (chunk of the call's sequences, head), every pass on the sequence's own S_n.  S_n is clamped to [1, 32 * ceil(d->S / 32)]; a
 *   sequence of any length in that range is computed correctly, and callers that want a sequence's bits to be a function of S_n
 *   alone send those of at most 128 tokens to lstc_attn_var_fwd / _bwd (functional.SeqLayout does).
 * Checked before any launch: d, s, row0, prob0, Q, K, V, probs, O (forward), dO / dQ / dK / dV (backward) NULL: LSTC_E_NULL; any
 * packed operand or output of the descriptor: LSTC_E_UNSUPPORTED; d->S <= 128, d->S > 512, d_k or d_v not a multiple of 16, or
 * n_probs > 2^32 - 1: LSTC_E_RANGE; n_ids <= 0, n_probs < 0 or a chunk count that does not match dtable_chunks: LSTC_E_SHAPE; dtable
 * non-NULL with dtable_chunks <= 0: LSTC_E_UNSUPPORTED.  lstc_attn_var_fwd / _bwd keep refusing d->S > 128. */
int lstc_attn_var_long_fwd(const LstcAttnDesc* d, const LstcSeqs* s, void* stream);
int lstc_attn_var_long_bwd(const LstcAttnDesc* d, const LstcSeqs* s, void* stream);

/* Rectangular attention (reference models/MultiHeadAttention.py:17-23, class ScaledDotProductAttention): the queries and the
 * keys have lengths of their own and there is no relative bias (csrc/attention_x.hip).
 *   A = (Q scale) K^T [N, H, Sq, Sk] ; A = mask byte == 0 ? -1e9f : A (m non-NULL) ; P = softmax(A, -1) ; Pd = dropout(P) ;
 *   O = Pd V.  `probs` receives P before dropout; the dropout decision of element (n, h, i, j) is the counter hash at the flat
 *   index ((n*H + h)*Sq + i)*Sk + j, so lstc_dropout_mask() over N*H*Sq*Sk elements with the same seed regenerates it.
 *   backward: dV = Pd^T dO ; dP' = dO V^T with the dropout replayed ; dA = P*(dP' - rowsum(dP'*P)) ; dQ = dA K scale ;
 *   dK = dA^T Q scale, all written (not accumulated).
 * Operands: Q [N, H, Sq, dk], K [N, H, Sk, dk], V [N, H, Sk, dv], O [N, H, Sq, dv], f32, each addressed as
 * base[n*sn + h*sh + t*st + feature] - the feature stride is 1.  Head-major [b, H, l, d] tensors ((H*l*d, l*d, d)) and the
 * transpose(1, 2) view of a token-major [b, l, H*d] projection ((l*H*d, d, H*d)) run without a copy.  dO uses O's strides;
 * dQ, dK, dV use those of Q, K, V.  Float4 loads are taken when the bases are 16-B aligned and the strides multiples of 4;
 * results do not depend on it.
 * Mask: LstcAttnMask as above, sq stepping over the query i < Sq and sk over the key j < Sk; m == NULL = no mask.  Masked keys
 *   of a row that keeps a key get probability exactly 0.0; a fully masked row is uniform, 1/Sk in every column - no -inf, no
 *   NaN; the dA that feeds dQ and dK is zero at masked positions; dV and the row sums are as unmasked (P carries the mask).
 * Limits: 1 <= Sq <= 512 and 1 <= Sk <= 512 independently; dk and dv multiples of 16 up to 512, dk != dv allowed - any other
 *   width returns LSTC_E_RANGE; N*H*Sq*Sk <= 2^32 - 1 (the dropout counter is 32 bits) and N*H <= 2^31 - 1, else LSTC_E_RANGE.
 * Every product runs on the exact-f32 MFMA in every compute mode; softmax and dropout are f32.
 * Checked before any launch: d, Q, K, V, probs, O (forward), dO / dQ / dK / dV (backward) or m->mask NULL: LSTC_E_NULL;
 *   a non-positive size, a negative stride, dropout_p outside [0, 1], in the backward a stride of 0 of Q, K or V over an axis
 *   longer than 1 (the gradient would have several writers per element): LSTC_E_SHAPE; then the limits.
 * Bit-reproducible run to run, forward and backward: one writer per element, fixed summation order, no float atomics. */
typedef struct LstcSdpaDesc {
    int32_t N, H, Sq, Sk, dk, dv;
    int64_t q_sn, q_sh, q_st;       /* element strides of Q (and dQ) over sequence, head, token */
    int64_t k_sn, k_sh, k_st;       /* of K (and dK) */
    int64_t v_sn, v_sh, v_st;       /* of V (and dV) */
    int64_t o_sn, o_sh, o_st;       /* of O (and dO) */
    float   scale;                  /* multiplies Q: 1 / temperature (:18) */
    float   dropout_p;
    uint64_t dropout_seed;
    const void* Q; const void* K; const void* V;
    void*  O;
    float* probs;                   /* dense [N, H, Sq, Sk] f32: written by the forward, read by the backward */
    /* backward only */
    const void* dO;
    void* dQ; void* dK; void* dV;
} LstcSdpaDesc;
int lstc_sdpa_fwd(const LstcSdpaDesc* d, const LstcAttnMask* mask_or_null, void* stream);
int lstc_sdpa_bwd(const LstcSdpaDesc* d, const LstcAttnMask* mask_or_null, void* stream);
/* Sq <= lstc_sdpa_few_query_max() (the compile-time constant SDPA_FEWQ_MAX of csrc/attention_x.hip, 1 .. 16; 0 = compiled out)
 * runs the few-query kernels behind the two calls above: one workgroup per (sequence, head), the [Sq][Sk] block in LDS, K and V
 * read once each.  Same contract, limits, return codes and bit-reproducibility; longer Sq runs the 32-row-tile kernels. */
int lstc_sdpa_few_query_max(void);

/* Re-associated CLS attention of the last layer: with one query per (sequence, head) the key / value projections are
 * never materialised — score[n,h,j] = u[n,h].x[n,j] with u = (q_h*scale) Wk_h, and o[n,h] = Wv_h (sum_j p[n,h,j] x[n,j]) —
 * which removes the layer's two [N*S,d]x[d,H*dk] projection GEMMs and their four backward GEMMs (same reference lines
 * as above: models/MultiHeadAttention.py:97-122 restricted to row 0).  U, Y: [N,H,d]; X, dX: [N,S,d]; W*, out, probs: [N,H,S].
 *   lstc_cls_dot   out[n,h,j] = sum_c U[n,h,c] X[n,j,c];  mode 0 raw | 1 softmax (+dropout), probs saved |
 *                  2 softmax/dropout backward: out = P*(dP - sum dP*P), dP = dot*keep
 *   lstc_cls_wsum  Y[n,h,c]  = sum_j W[n,h,j] X[n,j,c]
 *   lstc_cls_outer dX[n,j,c] = sum_h W1[n,h,j] U1[n,h,c] + W2[n,h,j] U2[n,h,c]
 * Requirements: d % 4 == 0, 16-B aligned pointers, S <= 128, H <= 16. */
int lstc_cls_dot(const float* U, const float* X, float* out, float* probs, int64_t N, int32_t S, int32_t H, int32_t d,
                 int32_t mode, float dropout_p, uint64_t seed, void* stream);
int lstc_cls_wsum(const float* W, const float* X, float* Y, int64_t N, int32_t S, int32_t H, int32_t d, void* stream);
int lstc_cls_outer(const float* W1, const float* U1, const float* W2, const float* U2, float* dX, int64_t N, int32_t S,
                   int32_t H, int32_t d, void* stream);

/* lstc_cls_dot for a padded batch: sequence n has klen[n] keys (device int32 [N]; the CLS token counts, so klen = real tokens + 1;
 * values are clamped to [1, S]).  Mode 1 runs the softmax over the keys j < klen[n]; in every mode out (and in mode 1 probs) is
 * exactly 0 for j >= klen[n], and the rows X[n, j >= klen[n]] are never read - they may hold anything, NaN included.  With zero
 * weights there lstc_cls_wsum / lstc_cls_outer need no length of their own as long as those rows are finite.  klen[n] == S for
 * every n gives lstc_cls_dot's result bit for bit.  Same requirements and return codes as lstc_cls_dot, S >= 2 (LSTC_E_SHAPE),
 * klen == NULL is LSTC_E_NULL. */
int lstc_cls_dot_len(const float* U, const float* X, const int32_t* klen, float* out, float* probs, int64_t N, int32_t S, int32_t H,
                     int32_t d, int32_t mode, float dropout_p, uint64_t seed, void* stream);

/* The three passes over an UNPADDED X (same reference lines: models/MultiHeadAttention.py:97-122 restricted to row 0): X and dX are
 * [M, d], sequence n = rows row0[n] .. row0[n+1] - 1 (device int32 [N + 1]; S_n is clamped to [1, S_max]).  U, Y stay [N, H, d] and
 * W*, out, probs [N, H, S_max], small N-row arrays: out (and probs) are exactly 0 for j >= S_n, mode 1 runs the softmax over the
 * sequence's own S_n keys, and only the first S_n entries of a W row are read.  lstc_cls_outer_var adds `add0` [N, d] (may be NULL)
 * to row 0 of every sequence - the CLS row's own terms - so every row of dX has one writer.  At equal lengths the results are those of
 * lstc_cls_dot / _wsum / _outer on the [N, S, d] view, bit for bit.  Requirements and return codes as lstc_cls_dot with S = S_max;
 * row0 == NULL is LSTC_E_NULL. */
int lstc_cls_dot_var(const float* U, const float* X, const int32_t* row0, float* out, float* probs, int64_t N, int32_t S_max, int32_t H,
                     int32_t d, int32_t mode, float dropout_p, uint64_t seed, void* stream);
int lstc_cls_wsum_var(const float* W, const float* X, const int32_t* row0, float* Y, int64_t N, int32_t S_max, int32_t H, int32_t d,
                      void* stream);
int lstc_cls_outer_var(const float* W1, const float* U1, const float* W2, const float* U2, const float* add0, const int32_t* row0,
                       float* dX, int64_t N, int32_t S_max, int32_t H, int32_t d, void* stream);

/* The three passes above over a PACKED X (round 5: the bf16 activation stream hands the last full layer's output to the CLS-only
 * layer as an lstc_pack1 operand of the [N*S, d] matrix and takes the gradient back as one; same reference lines).  Arithmetic is
 * f32 on the widened bf16 values; lstc_cls_outer_pack rounds dX once (RNE) after adding `add0` [N, d] (may be NULL) to row 0 of
 * every sequence - the CLS row's own terms dQ Wq + the residual gradient.  U, Y, W*, out, probs as above.
 * Requirements: (N*S) % 256 == 0, d = 512 / 1024 / 2048, H <= 8 (LSTC_E_UNSUPPORTED otherwise), S <= 128, 16-B aligned pointers. */
int lstc_cls_dot_pack(const float* U, const void* X_pack, float* out, float* probs, int64_t N, int32_t S, int32_t H, int32_t d,
                      int32_t mode, float dropout_p, uint64_t seed, void* stream);
int lstc_cls_wsum_pack(const float* W, const void* X_pack, float* Y, int64_t N, int32_t S, int32_t H, int32_t d, void* stream);
int lstc_cls_outer_pack(const float* W1, const float* U1, const float* W2, const float* U2, const float* add0, void* dX_pack,
                        int64_t N, int32_t S, int32_t H, int32_t d, void* stream);

/* ------------------------------------------------------------------- row-wise kernels */
/* y = LayerNorm(x) * gamma + beta over the last dim (eps inside the sqrt, biased variance) —
 * nn.LayerNorm(d_model, eps=1e-6): models/MultiHeadAttention.py:47,125-126; models/FFN.py:10,20-21;
 * models/Encoder.py:31,48-49.  Saves mean / rstd per row for the backward. */
int lstc_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                       float* mean, float* rstd, int64_t rows, int32_t d, float eps, void* stream);
/* dx, and per-workgroup partial dgamma/dbeta in `partial` [2, n_partial, d] (reduce with lstc_colsum).
 * d % 4 == 0, d <= 2048 and 16-B aligned dy, x, gamma, dx, partial: the register-resident kernel of csrc/rowops.hip (ln_bwd_pair,
 * two waves per row; workgroup w takes rows 2w and 2w + 1, then every 2 n_partial further) - the one kernel text behind
 * lstc_layernorm_bwd_drop and lstc_layernorm_bwd_drop_pack too, so the three give the same dx bit for bit, and at the same
 * n_partial the same dgamma / dbeta planes.  Any other d or alignment: a scalar kernel (2 d floats of LDS: LSTC_E_RANGE beyond
 * 64 KiB). */
int lstc_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                       float* dx, float* partial, int32_t n_partial, int64_t rows, int32_t d, void* stream);
/* bf16 mode: the same two kernels also emit the packed bf16 operand (lstc_pack1 layout, [rows, d]) of the GEMMs that read
 * their result, from the registers that hold the row - the separate lstc_pack1 pass (4 B read + 2 B written per element)
 * and, in the backward, the lstc_dropout_apply pass disappear.
 *   lstc_layernorm_fwd_pack:      `packed` = pack of y: the A operand of the next block's first product (the Q/K/V
 *                                 projections after models/FFN.py:20-21, W1 after models/MultiHeadAttention.py:125-126).
 *   lstc_layernorm_bwd_drop_pack: `packed` = pack of df = dropout-replay(dx) (keep iff the hash of the flat index row*d+col
 *                                 passes, scaled by 1/(1-p) - exactly lstc_dropout_apply(dx, p, seed)): the operand of the
 *                                 weight gradient and the input gradient of the Linear in front of the dropout
 *                                 (fc: MultiHeadAttention.py:123, w_2: FFN.py:17-18); `partial` is [3, n_partial, d], the
 *                                 third plane = column sums of df (that Linear's bias gradient).  dx stays f32 (residual).
 *                                 At every accepted width the kernel is lstc_layernorm_bwd's, with the replay compiled in.
 * Both need rows % 256 == 0, d % 64 == 0, d <= 2048 (the rows fill the pack's even tile grid exactly; LSTC_E_UNSUPPORTED
 * otherwise - the caller then packs with lstc_pack1) and `packed` of lstc_pack1_bytes(rows, d) bytes. */
int lstc_layernorm_fwd_pack(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int64_t rows, int32_t d, float eps, void* packed, void* stream);
/* The same fusion with an f32 result (fp32 / f32x3 modes): df = lstc_dropout_apply(dx, p, seed) written next to dx, `partial`
 * [3, n_partial, d] with the column sums of df as third plane.  d = 512, 1024 or 2048, the widths of the models and of its only
 * callers (LSTC_E_UNSUPPORTED otherwise, although the kernel behind it serves every d % 4 == 0 up to 2048). */
int lstc_layernorm_bwd_drop(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                            float* dx, float* df, float* partial, int32_t n_partial, int64_t rows, int32_t d, float dropout_p,
                            uint64_t dropout_seed, void* stream);
int lstc_layernorm_bwd_drop_pack(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                 float* dx, float* partial, int32_t n_partial, int64_t rows, int32_t d, float dropout_p,
                                 uint64_t dropout_seed, void* packed, void* stream);

/* bf16 ACTIVATION STREAM (round 5; the bf16 compute mode's default where the shapes allow).  Between the CLS concat and the last
 * full encoder layer no f32 activation exists: the residual sums dropout(f) + x (models/MultiHeadAttention.py:123-124,
 * models/FFN.py:17-19) leave the GEMM epilogues as lstc_pack1 operands (LSTC_EPI_OUT_PACK + LSTC_EPI_RESIDUAL_PACK), these two
 * kernels run nn.LayerNorm (models/MultiHeadAttention.py:125-126, models/FFN.py:20-21) and its backward ON the packs, and the
 * gradient of the residual stream travels as packs too - 2 bytes per element per pass instead of 4 (+2 for the pack).
 * Statistics, normalisation, dropout replay and the partial sums are f32 arithmetic; only what is stored is bf16 (RNE).
 *   lstc_layernorm_fwd_act: exactly one of x (f32 [rows, d]) / x_pack (pack of [rows, d]) is the input; y (f32) and / or y_pack
 *                           receive the result (f32: the stream's exit where the CLS-only layer cannot read a pack).
 *   lstc_layernorm_bwd_act: x_pack = the forward's input pack; the incoming gradient is dy (f32) or dy_pack; dx_pack (may be
 *                           NULL: nobody reads layer 0's) = gradient of the residual sum, df_pack = dropout-replay(dx) exactly
 *                           as lstc_layernorm_bwd_drop_pack, partial [3, n_partial, d] = dgamma, dbeta, column sums of df.
 *                           A kernel of its own (ln_bwd_act): it sums a row in another order than the f32-row kernel.
 * rows % 256 == 0 and d = 1024 or 2048 (LSTC_E_UNSUPPORTED otherwise); every pack lstc_pack1_bytes(rows, d) bytes, 16-B aligned. */
int lstc_layernorm_fwd_act(const float* x, const void* x_pack, const float* gamma, const float* beta, float* y, void* y_pack,
                           float* mean, float* rstd, int64_t rows, int32_t d, float eps, void* stream);
int lstc_layernorm_bwd_act(const float* dy, const void* dy_pack, const void* x_pack, const float* gamma, const float* mean,
                           const float* rstd, void* dx_pack, float* partial, int32_t n_partial, int64_t rows, int32_t d,
                           float dropout_p, uint64_t dropout_seed, void* df_pack, void* stream);

/* CLS = mean over tokens (or `cls_token` if not NULL), prepended; optional `pos` [S, d] added to every
 * sequence — models/Encoder.py:51-58.  x [N, S-1, d] -> y [N, S, d].  When `x_hi` is not NULL, sequences
 * [0, n_lo) are read from `x` and [n_lo, N) from `x_hi`: the reference's torch.cat([norm_feats, abnorm_feats])
 * (Train/temporal_transformer_shanghaitech.py:120) is fused into this pass instead of costing its own copy. */
int lstc_cls_concat_fwd(const float* x, const float* x_hi, int64_t n_lo, const float* cls_token, const float* pos,
                        float* y, int64_t N, int32_t S, int32_t d, void* stream);
/* The same with the packed bf16 form of y ([N*S, d], lstc_pack1 layout) written next to it: layer 0's A operand in bf16 mode
 * (N*S a multiple of 256, d a multiple of 64; else LSTC_E_UNSUPPORTED).  y may be NULL (round 5, the bf16 activation stream: the
 * pack is then the only output; d % 4 == 0 and 16-B aligned operands required). */
int lstc_cls_concat_fwd_pack(const float* x, const float* x_hi, int64_t n_lo, const float* cls_token, const float* pos,
                             float* y, int64_t N, int32_t S, int32_t d, void* packed, void* stream);

/* The same pass fed STRAIGHT from an HBM-resident feature bank [bank_clips, P, d] (round 5): token t of sequence n is patch t % P of
 * clip clip_idx[n * (S-1)/P + t / P], i.e. lstc_gather_rows (the batch formation `feat[chosen[...], :]`, utils/load_dataset.py:88 +
 * default collate) + the torch.cat + the CLS concat in ONE pass over the features - the gathered batch [B, T, P, d] is never
 * written.  y (f32 [N, S, d]) and / or packed (lstc_pack1 of [N*S, d]: N*S a multiple of 256, d of 64) receive the result.
 * (S-1) % P == 0, d % 4 == 0, 16-B aligned bases; idx entries must lie in [0, bank_clips). */
int lstc_cls_concat_gather_fwd(const float* bank, int64_t bank_clips, const int64_t* clip_idx, int32_t P, const float* cls_token,
                               const float* pos, float* y, int64_t N, int32_t S, int32_t d, void* packed, void* stream);

/* Gradient w.r.t. the Encoder input, needed only when something upstream is trainable (input_layerNorm,
 * models/Encoder.py:48-49): dx[n,t,:] = dy[n,t+1,:] + (mean_cls ? dy[n,0,:]/(S-1) : 0). */
int lstc_cls_concat_bwd(const float* dy, float* dx, int64_t N, int32_t S, int32_t d, int32_t mean_cls, void* stream);

/* The CLS concat of a PADDED batch: sequence n has lens[n] real tokens x[n, :lens[n]] (device int32 [N], the CLS token not
 * counted; values are clamped to [1, S-1]), the rest of its row of x is padding that is never read (it may hold NaN).
 *   forward:  y[n,0] = mean(x[n, :L_n]) (or `cls_token`), y[n,1+t] = x[n,t] for t < L_n, `pos` [S, d] added on rows 0..L_n, and the
 *             rows past L_n written as exact zeros: row n is what the un-lengthed call gives for x[n:n+1, :L_n], then zeros.
 *   backward: dx[n,t] = dy[n,t+1] + (mean_cls ? dy[n,0] / L_n : 0) for t < L_n, exact zeros beyond (dx may be NULL);
 *             dtok [S, d] (may be NULL) = sum over the sequences with t <= L_n of dy[n,t,:] - row 0 is the gradient of a learned
 *             CLS token, rows 0..S-1 that of the position table; the sequences are added in order (deterministic).
 * 16-B accesses when d % 4 == 0 and every operand is 16-B aligned, 4-B ones otherwise: the results are the same bits. */
int lstc_cls_concat_len_fwd(const float* x, const int32_t* lens, const float* cls_token, const float* pos, float* y, int64_t N,
                            int32_t S, int32_t d, void* stream);
int lstc_cls_concat_len_bwd(const float* dy, const int32_t* lens, float* dx, float* dtok, int64_t N, int32_t S, int32_t d,
                            int32_t mean_cls, void* stream);

/* The CLS concat (models/Encoder.py:51-58) unpadded in and unpadded out: x [M - N, d] holds the patch tokens of N sequences back to
 * back, y [M, d] the same with each sequence's CLS row in front.  row0 (device int32 [N + 1]) gives the rows of y: sequence n =
 * rows row0[n] .. row0[n+1] - 1 with L_n = S_n - 1 patch tokens, which are rows row0[n] - n .. of x.
 *   forward:  y[row0[n]] = mean of the sequence's own L_n rows (a sequential walk per column) or `cls_token`, the rows behind it the
 *             tokens; `pos` [>= S_max, d] (may be NULL) is added on rows 0..L_n of every sequence.
 *   backward: dx_n[t] = dy[row0[n]+1+t] + (mean_cls ? dy[row0[n]] / L_n : 0) (dx may be NULL); dtok [S_max, d] (may be NULL) = sum over
 *             the sequences that have token t of dy[row0[n]+t] - row 0 the gradient of a learned CLS token, rows 0..S_max-1 that of
 *             the position table; the sequences are added in order (deterministic).
 * 16-B accesses when d % 4 == 0 and every operand is 16-B aligned, 4-B ones otherwise: the results are the same bits, and a
 * sequence's bits do not depend on its neighbours.  The offsets are trusted. */
int lstc_cls_concat_var_fwd(const float* x, const int32_t* row0, const float* cls_token, const float* pos, float* y, int64_t N,
                            int32_t d, void* stream);
int lstc_cls_concat_var_bwd(const float* dy, const int32_t* row0, float* dx, float* dtok, int64_t N, int32_t S_max, int32_t d,
                            int32_t mean_cls, void* stream);

/* lstc_cls_concat_var_fwd fed from SPANS of an HBM-resident bank of rows [bank_rows, d]: y, row0, cls_token and pos as there, but the
 * L_n = row0[n+1] - row0[n] - 1 patch tokens of sequence n are rows src0[n] .. src0[n] + L_n - 1 of `bank` (src0: device int64 [N])
 * instead of rows of a packed input - the token matrix of an evaluation or label pass is never materialised.  Spans may overlap,
 * repeat and come in any order.  The same kernel text and the same sequential walk per column: for the same tokens y is bit-identical
 * to lstc_cls_concat_var_fwd, on the 16-B path (d % 4 == 0, aligned operands) and on the 4-B one, and a sequence's bits depend neither
 * on its neighbours nor on where it lies in the bank.  The offsets are trusted: every span must lie inside [0, bank_rows).  There is
 * no backward entry - a bank takes no gradient; a learned CLS token and the position table get theirs from lstc_cls_concat_var_bwd
 * with dx = NULL. */
int lstc_cls_concat_span_fwd(const float* bank, int64_t bank_rows, const int64_t* src0, const int32_t* row0, const float* cls_token,
                             const float* pos, float* y, int64_t N, int32_t d, void* stream);

/* out[c] = sum_r x[r, c] for x [rows, ld] (first `cols` columns); deterministic two-pass reduction.
 * `partial` is caller workspace of n_partial*cols floats.  Bias / LayerNorm / pos-enc gradients. */
int lstc_colsum(const float* x, int64_t rows, int32_t cols, int32_t ld, float* partial, int32_t n_partial,
                float* out, int32_t accumulate, void* stream);
/* `batch` column sums in the same two launches: plane b is x + b * batch_stride ([rows, ld]), its result out[b * cols ...];
 * `partial` holds batch * min(rows, n_partial) * cols floats.  Per plane the arithmetic (row -> partial row -> accumulator, order
 * of every addition) is lstc_colsum's two-pass form, so out[b] is bit-identical to lstc_colsum of plane b.  The LayerNorm
 * backward's three per-workgroup partial planes (dgamma, dbeta, dbias: autograd of nn.LayerNorm / nn.Linear.bias, models/FFN.py:
 * 19-21, models/MultiHeadAttention.py:123-126) are reduced by ONE call instead of three. */
int lstc_colsum_batched(const float* x, int32_t batch, int64_t rows, int32_t cols, int32_t ld, int64_t batch_stride,
                        float* partial, int32_t n_partial, float* out, void* stream);

/* y[i] = x[i] * keep(i)/(1-p) with the GEMM epilogue's mask (dropout backward / standalone dropout). */
int lstc_dropout_apply(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);
/* The same on an lstc_pack1 operand [rows, d] (rows % 256 == 0, d % 64 == 0): y_pack = dropout-replay(x_pack) with the mask of
 * the flat index row * d + col, bf16 in, bf16 out (one more RNE rounding).  The bf16 activation stream's backward of a block
 * WITHOUT LayerNorm (models/MultiHeadAttention.py:123-124 with layerNorm = False: the STN configs): the incoming gradient pack
 * is the gradient of dropout(f) + x, its dropped form the operand of fc's weight and input gradients. */
int lstc_dropout_apply_pack(const void* x_pack, void* y_pack, int64_t rows, int32_t d, float p, uint64_t seed, void* stream);
/* Second half of a K-split small product (round 5): C = epi(parts[0] + ... + parts[splits - 1]), parts[i] = the [M, N] partial result
 * of K chunk i at parts + i * part_stride (row-major, ld = N), added in chunk order; `flags` and the operands as LstcGemmDesc's
 * epilogue (bias, ReLU, dropout of the flat index row * N + col, residual, ReLU mask, accumulate - in that order; no pack flags).
 * The CLS-only last layer and the heads run [sequences, d] x [d, d] products whose few output tiles leave most of the chip idle
 * while one workgroup walks the whole K range (models/MultiHeadAttention.py:97-126 on row 0, models/FFN.py:17-19,
 * models/Classifier.py:8-14 for a rank's 256 sequences): the host side launches their K chunks as ONE batched lstc_gemm into
 * `parts` and finishes here.  `groups` > 1: that many independent [M, N] results in one call (the per-head products q_h W_k,h /
 * xbar_h W_v,h^T of the re-associated CLS attention) - group g's partials at parts + g * group_stride_parts, its result at
 * C + g * group_stride_c; only the plain sum (optionally LSTC_EPI_ACCUM).  groups = 1: the strides are ignored.
 * N, part_stride, ldc (ldr, ld_relu, group strides) multiples of 4; 16-B aligned pointers; groups * M * N < 2^32. */
int lstc_splitk_finish(const float* parts, int32_t splits, int64_t part_stride, int64_t M, int64_t N, const float* bias,
                       const float* residual, int64_t ldr, const float* relu_src, int64_t ld_relu, float* C, int64_t ldc, int32_t flags,
                       float dropout_p, uint64_t dropout_seed, int32_t groups, int64_t group_stride_parts, int64_t group_stride_c,
                       void* stream);
/* out[i, 0:K] = the bf16 values of row row0 + i * row_step of an lstc_pack1 operand [rows, K], widened to f32 (i < n; K % 8 == 0,
 * ldo % 4 == 0).  The CLS-only last layer reads its query rows (token 0 of every sequence: row0 = 0, row_step = S) out of the
 * activation stream's pack (models/MultiHeadAttention.py:97 restricted to row 0); tests read whole packs back with it. */
int lstc_unpack1_rows(const void* x_pack, int64_t rows, int32_t K, int64_t row0, int64_t row_step, int64_t n, float* out, int64_t ldo,
                      void* stream);
/* mask[i] = keep(i) ? 1 : 0 — exported so tests can replay a HIP dropout run through the oracle. */
int lstc_dropout_mask(uint8_t* mask, int64_t n, float p, uint64_t seed, void* stream);
/* Dropout seeds for a captured step (hipGraph).  Every entry that draws a dropout mask takes its 64-bit seed BY VALUE, so a
 * captured launch would replay one mask for ever.  While `dev_word` is non-NULL, every such launch of this process (from any host
 * thread - the autograd backward runs on its own) carries the pointer and uses  seed + *dev_word,  read ON THE DEVICE when the
 * kernel runs: the caller bumps the word between replays (by the number of seeds a step draws) and the replayed step sees the
 * masks the eager step with those seeds would have seen, bit for bit.  NULL (the default) restores plain by-value seeds.
 * Process-wide launch context, meant to bracket a stream capture; the word must outlive every graph that captured it.
 * Replaces nothing upstream: the reference draws its masks from torch's global generator (nn.Dropout, models/FFN.py:12). */
int lstc_dropout_seed_device(const uint64_t* dev_word);

/* Last head layer fused with its activation: out = sigmoid(x W^T + b) (c=1, models/Regressor.py:9) or
 * softmax(x W^T + b) (c=2, models/Classifier.py:10).  x [rows, 32]. */
int lstc_head_out_fwd(const float* x, const float* W, const float* b, float* out, int64_t rows, int32_t c,
                      void* stream);
/* dx [rows,32], dW [c,32], db [c] from d(out); dW/db are WRITTEN (round 4: no caller-side fill) by one workgroup that sums in a fixed order. */
int lstc_head_out_bwd(const float* x, const float* W, const float* out, const float* dout,
                      float* dx, float* dW, float* db, int64_t rows, int32_t c, void* stream);

/* ----------------------------------------------------------------------------- loss
 * MIL ranking loss + sparsity (+ CE on softmax outputs | + weighted BCE) and its gradient w.r.t. the
 * head output, one launch:
 *   mode 0 (STN):  Train/spatio_transformer_shanghaitech.py:21-32
 *   mode 1 (LTN):  Train/temporal_transformer_shanghaitech.py:21-36,125-134  (out [2bs*pn, 2]; score = out[:,1])
 *   mode 2 (STN + BCE): Train/spatio_transformer_MIL_CE.py:23-26,32-44,176-181
 * bag[v] = max_p mean_l score[v,p,l]; err = sum_ij relu(1 - abn_j + nor_i)/bs^2;
 * l1 = mean(score[l1_skip:]) (flat slice quirk: l1_skip = bs*pn*L for STN, bs for LTN / co-teach).
 * Soft targets are built in-kernel (Train/temporal_transformer_shanghaitech.py:103-112): normal parts
 * [1,0]; abnormal parts t1 = mean over label_len pseudo labels, t0 = 1-t1.
 * Data-parallel: the hinge couples all bs_global x bs_global pairs, so ranks exchange bag values
 * (2*bs_global floats, one sum-all-reduce) between phase 0 and phase 1; every other term is a local sum
 * divided by a global count.  scalars = rank-local contributions (their sum over ranks is the reference
 * value; on one GPU they are the reference values).
 *
 * Top-k bags (`topk`; the reference parses --topk and pools with torch.max, so this is the project's own extension):
 *   pm[v,p] = mean_l score[v,p,l], float32, summed over l in ascending order (the sum the maximum above is taken over).
 *   With k = topk (0 means 1) the selected set of video v is the first k parts in the order (pm descending, part index
 *   ascending): ties go to the lower index.  bag[v] = (float32 sum of the selected pm, in that order) / (float)k; for k = 1
 *   bag[v] is the selected pm itself, undivided - bit for bit the maximum above.  Hinge, l1, CE / BCE and the scalars are
 *   unchanged.  d err / d pm[v,p] = gbag[v] / k on the selected parts and 0 elsewhere, i.e. gbag[v] / (k * score_len) on their
 *   elements of dout.  Data parallel is unchanged: a rank contributes its own videos' bag values to the exchange, and a video's
 *   bag does not depend on how the batch is split.
 *   Limits for topk > 1: 1 <= topk <= part_num and part_num <= 64 (one part per lane of a wave64).  Checked before any launch:
 *   topk < 0 LSTC_E_SHAPE; topk > part_num LSTC_E_RANGE; topk > 1 with part_num > 64 LSTC_E_RANGE.
 *   NaN scores: k = 1 behaves as before (a NaN mean is never the maximum); for k > 1 the result is unspecified (a NaN mean
 *   ranks last), the launch completes and writes only dout / bag / scalars.
 */
typedef struct LstcLossDesc {
    int32_t mode;                   /* 0 STN, 1 LTN (MIL + CE), 2 STN co-teaching (MIL + BCE) */
    int32_t bs_global, bs_local, rank_off;  /* pairs per global batch / on this rank / first pair index of this rank */
    int32_t part_num;
    int32_t score_len;              /* scores per part in `out`: part_len for modes 0/2, 1 for mode 1 */
    int32_t label_len;              /* pseudo labels per part in `abn_labels` (= --part_len) */
    int32_t l1_skip;                /* leading entries of the GLOBAL flat score vector excluded from the l1 mean */
    float lambda_1, lambda_MIL, lambda_aux, lambda_normal, lambda_abnormal;
    const float* out;               /* head output of this rank: [2*bs_local*part_num*score_len, c], c = 2 (mode 1) or 1;
                                       normal videos first, abnormal second (the reference's cat order) */
    const float* abn_labels;        /* [bs_local, part_num*label_len] pseudo labels of this rank's abnormal videos;
                                       NULL = no CE/BCE term (--temporal_only / mode 0) */
    const float* targets;           /* optional explicit soft targets [parts_local, 2] (parts = rows for mode 1,
                                       [2*bs_local*part_num] for mode 2); overrides abn_labels — used by the
                                       reference-named get_CE_loss / get_BCE_loss wrappers */
    float* bag;                     /* [2*bs_global] bag values, normal half then abnormal half.  phase 0 writes this
                                       rank's entries (caller zeroes first, then sum-all-reduces); phase 1 reads all */
    float* dout;                    /* same shape as `out`: d(rank's loss contribution)/d(out) */
    float* scalars;                 /* [5] loss, mil, err, l1, aux — this rank's contributions */
    int32_t phase;                  /* 0 = bags only; 1 = loss + gradient from `bag`; 2 = both (single rank) */
    int32_t topk;                   /* parts pooled into a bag (see above); 0 (a zero-initialised descriptor) means 1.  Last
                                       field, in what was the struct's tail padding: offset 108, sizeof stays 112 */
} LstcLossDesc;

int lstc_vad_loss(const LstcLossDesc* d, void* stream);

/* ------------------------------------------------------------------------ optimizer
 * torch.optim.Adagrad step as configured at Train/temporal_transformer_shanghaitech.py:83-85,142
 * (lr_decay=0, eps=1e-10, initial accumulator 0): g = grad*gscale + wd*w; s += g*g; w -= lr*g/(sqrt(s)+eps).
 * `gscale` carries the clip_grad_norm_ coefficient (:139-141) or 1. */
int lstc_adagrad_step(float* w, const float* grad, float* state, int64_t n, float lr, float weight_decay,
                      float eps, float gscale, void* stream);

/* optimizer.step() (Train/temporal_transformer_shanghaitech.py:142; Train/spatio_transformer_shanghaitech.py:109): the same
 * update for EVERY parameter of the step in ONE launch (torch.optim.Adagrad loops over the ~45 tensors; here the items ride in
 * the kernel arguments, 48 per launch).  `items` is a HOST array; element
 * arithmetic and order are those of lstc_adagrad_step - bit-identical results. */
typedef struct LstcAdagradItem {
    float* w;
    const float* grad;
    float* state;
    int64_t n;
    float lr, weight_decay, eps, grad_scale;
} LstcAdagradItem;
int lstc_adagrad_multi(const LstcAdagradItem* items, int32_t count, void* stream);

/* lstc_adagrad_multi under a learning-rate schedule: the items, their checks, the 48-per-launch split and the element order are
 * lstc_adagrad_multi's; per workgroup  lr_t = (float)((double)lr * (double)*lr_scale)  (the widening lstc_adam_multi uses) and the
 * element runs with lr_t in place of lr.  `lr_scale` is ONE DEVICE float, read on the device by every launch of a split list, so a
 * captured launch follows whatever lstc_lr_schedule writes there.  *lr_scale == 1.0f gives lstc_adagrad_multi's results bit for
 * bit.  lr_scale == NULL: LSTC_E_NULL, like a NULL pointer of an item. */
int lstc_adagrad_multi_scaled(const LstcAdagradItem* items, int32_t count, const float* lr_scale, void* stream);

/* A learning-rate schedule evaluated on the device: ONE launch, one thread, does  t = *step;  *scale = f(t);  *step = t + 1
 * (a word at INT32_MAX is not incremented).  `step` and `scale` are DEVICE words; `scale` is the multiplier lstc_adam_multi and
 * lstc_adagrad_multi_scaled read.  t is the ZERO-based index of the optimizer step about to be taken (torch.optim.lr_scheduler's
 * last_epoch).  The schedule itself is passed by value and nothing that changes from step to step is, so a captured launch
 * replays as step t + 1, t + 2, ...
 *
 * f is evaluated in float64 from the f32 fields widened and rounded ONCE to f32.  With W = warmup_steps, T = total_steps,
 * ws = warmup_start, m = min_scale and D = T - W:
 *     t <  W, every kind:   f = ws + (1 - ws) * t / W
 *     t >= W, u = min(t - W, D):
 *         CONSTANT   f = 1
 *         LINEAR     f = 1 - (1 - m) * u / D
 *         COSINE     f = m + (1 - m) * 0.5 * (1 + cos(pi * u / D))
 *         STEP       f = max(m, gamma^floor((t - W) / step_size))          (the power by repeated squaring in float64)
 *         INV_SQRT   f = max(m, sqrt(W' / max(t, W')))  with  W' = max(W, 1)
 * Products and quotients associate left to right as written; there is no contraction.
 *
 * Refused before any launch: s, step or scale NULL (LSTC_E_NULL); an unknown kind, W < 0, LINEAR or COSINE with T <= W, STEP with
 * step_size < 1 (LSTC_E_SHAPE); ws or m outside [0, 1] or NaN, STEP with gamma outside (0, 1] or NaN (LSTC_E_RANGE). */
enum { LSTC_LR_CONSTANT = 0, LSTC_LR_LINEAR = 1, LSTC_LR_COSINE = 2, LSTC_LR_STEP = 3, LSTC_LR_INV_SQRT = 4 };
typedef struct LstcLrSchedule {
    int32_t kind;             /* LSTC_LR_* */
    int32_t warmup_steps;     /* W >= 0 */
    int32_t total_steps;      /* T; LINEAR / COSINE need T > W; ignored otherwise */
    int32_t step_size;        /* STEP: >= 1; ignored otherwise */
    float warmup_start;       /* ws in [0, 1]: the scale of step 0 when W > 0 */
    float min_scale;          /* m in [0, 1] */
    float gamma;              /* STEP: in (0, 1] */
} LstcLrSchedule;
int lstc_lr_schedule(const LstcLrSchedule* s, int32_t* step, float* scale, void* stream);

/* torch.optim.Adam (decoupled = 0: weight decay added to the gradient) and torch.optim.AdamW (decoupled = 1: the weight is
 * shrunk first), amsgrad = False, maximize = False, for EVERY parameter of the step in one launch - `items` is a HOST array that
 * rides in the kernel arguments, 48 per launch, like lstc_adagrad_multi's.  Nothing that changes from step to step is passed by
 * value, so a captured launch can be replayed: the step count t is the item's DEVICE word `step` (the call adds 1 to it with a
 * one-thread-per-item launch in front of the update, then every workgroup reads the new value), and the learning rate is
 * lr_t = lr * *lr_scale with `lr_scale` a DEVICE float (NULL = 1).  Each item owns its word.
 *
 * Per item, in float64 from the f32 fields widened, each rounded ONCE to f32:
 *     omb1 = 1 - beta1     omb2 = 1 - beta2     step = lr_t / (1 - beta1^t)     rsb2 = 1 / sqrt(1 - beta2^t)
 *     keep = 1 - lr_t * weight_decay            (lr_t = lr * *lr_scale and beta^t, by repeated squaring, in float64 too)
 * Per element, f32, one rounding per operation, in this order (no contraction):
 *     g = grad * grad_scale
 *     decoupled ?  w = w * keep  :  g = g + weight_decay * w
 *     m = m + omb1 * (g - m)
 *     v = beta2 * v + omb2 * (g * g)
 *     w = w - (step * m) / (sqrtf(v) * rsb2 + eps)
 * The result of an element does not depend on pointer alignment (float4 accesses when w, grad, m and v are all 16-byte aligned,
 * scalar ones otherwise) nor on how a list is split into calls.
 *
 * Refused before any launch: count < 0, items == NULL with count > 0, a NULL w / grad / m / v / step, n < 0, two items sharing one
 * step word (LSTC_E_SHAPE); beta1 or beta2 outside [0, 1), eps, lr or weight_decay negative or not finite (LSTC_E_RANGE).
 * An item with n == 0 updates nothing; its word is still incremented.  count == 0 does nothing. */
typedef struct LstcAdamItem {
    float* w;
    const float* grad;
    float* m;                 /* exp_avg */
    float* v;                 /* exp_avg_sq */
    int64_t n;
    int32_t* step;            /* DEVICE word of this item: the call adds 1 to it, then uses the new value as t */
    const float* lr_scale;    /* DEVICE float or NULL (= 1): lr_t = lr * *lr_scale, read on the device */
    float lr, beta1, beta2, eps, weight_decay, grad_scale;
    int32_t decoupled;        /* 0: Adam (wd added to the gradient), 1: AdamW (w *= 1 - lr_t * wd first) */
} LstcAdamItem;
int lstc_adam_multi(const LstcAdamItem* items, int32_t count, void* stream);

/* An exponential moving average of EVERY weight of the step in one launch (Polyak averaging; the update of
 * torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn, with TensorFlow's optional num_updates warm-up) - `items` is a
 * HOST array that rides in the kernel arguments, 48 per launch, like lstc_adam_multi's.  Nothing that changes from update to
 * update is passed by value, so a captured launch can be replayed: the update count t is the item's DEVICE word `count` (the
 * call adds 1 to it with a one-thread-per-item launch in front of the update, then every workgroup reads the new value).
 * Each item owns its word.
 *
 * Per item:  t == 1: the update is a bit copy, avg = w (AveragedModel at n_averaged == 0).
 *            t >  1: decay_t = warmup ? min(decay, (1 + u) / (10 + u)) : decay  with u = t - 1, and  a = 1 - decay_t,
 *                    in float64 from the f32 field widened, rounded ONCE to f32.
 * Per element, f32, one rounding per operation, in this order (no contraction):
 *     avg = avg + a * (w - avg)
 * (Adam's m update; torch.lerp(avg, w, a) for a < 0.5).  The result of an element does not depend on pointer alignment (float4
 * accesses when avg and w are both 16-byte aligned, scalar ones otherwise) nor on how a list is split into calls.
 *
 * Refused before any launch: count < 0, items == NULL with count > 0, a NULL avg / w / count, n < 0, two items sharing one
 * word, avg == w with n > 0 (LSTC_E_SHAPE); decay outside [0, 1) or not finite, warmup other than 0 or 1 (LSTC_E_RANGE).
 * An item with n == 0 updates nothing; its word is still incremented.  count == 0 does nothing. */
typedef struct LstcEmaItem {
    float* avg;               /* the average, updated in place */
    const float* w;           /* the weight, read only */
    int64_t n;
    int32_t* count;           /* DEVICE word of this item: the call adds 1 to it, then uses the new value as t */
    float decay;              /* in [0, 1) */
    int32_t warmup;           /* 0 / 1 */
} LstcEmaItem;
int lstc_ema_multi(const LstcEmaItem* items, int32_t count, void* stream);

/* a[i] <-> b[i], bit for bit, for every item in one launch (48 per launch; `items` is a HOST array that rides in the kernel
 * arguments); any alignment.  It puts averaged weights INTO the live parameter storage for an evaluation and takes them out
 * again, so views of that storage and raw pointers held elsewhere stay valid.
 * Refused before any launch (LSTC_E_SHAPE): count < 0, items == NULL with count > 0, a NULL a / b, n < 0, a == b with n > 0.
 * An item with n == 0 and count == 0 do nothing. */
typedef struct LstcSwapItem {
    float* a;
    float* b;
    int64_t n;
} LstcSwapItem;
int lstc_swap_multi(const LstcSwapItem* items, int32_t count, void* stream);
/* out[0] += sum(x^2) (f32 atomics over workgroup partials; caller zeroes) — for clip_grad_norm_. */
int lstc_sqnorm_accum(const float* x, int64_t n, float* out, void* stream);

/* torch.nn.utils.clip_grad_norm_(parameters, max_norm) (Train/temporal_transformer_shanghaitech.py:139-141) over a whole
 * parameter list without a host read-back, so a captured step (HIP graph) can contain it:
 *   lstc_sqnorm_multi      out[0] = sum over every tensor of sum(x^2), out[1] = its square root (the total norm the reference
 *                          logs): one launch over all tensors (48 per launch) writing one
 *                          partial per 8192-element slice into `scratch` (>= lstc_sqnorm_multi_scratch(items, count) floats),
 *                          then one workgroup adds the partials in index order - bit-reproducible, no float atomics;
 *   lstc_clip_scale_multi  x *= max_norm / (sqrt(sqnorm[0]) + 1e-6) for every tensor when that coefficient is < 1 (torch's
 *                          clamp to 1; a NaN norm multiplies every tensor by NaN, as torch does), the coefficient formed ON THE
 *                          DEVICE from the value lstc_sqnorm_multi left there.
 * `items` is a HOST array (it rides in the kernel arguments). */
typedef struct LstcVecItem {
    float* x;
    int64_t n;
} LstcVecItem;
int64_t lstc_sqnorm_multi_scratch(const LstcVecItem* items, int32_t count);
int lstc_sqnorm_multi(const LstcVecItem* items, int32_t count, float* scratch, int64_t scratch_floats, float* out, void* stream);
int lstc_clip_scale_multi(const LstcVecItem* items, int32_t count, const float* sqnorm, float max_norm, void* stream);

/* x *= alpha in place: applies the clip_grad_norm_ coefficient to a gradient tensor. */
int lstc_scale(float* x, int64_t n, float alpha, void* stream);

/* f32 -> bf16 (round to nearest even) and back, n elements: the optional half-width gradient all-reduce of the data-parallel
 * path (replaces nothing upstream - nn.DataParallel reduces fp32, Train/temporal_transformer_shanghaitech.py:76-78 - and is
 * off by default: lstc_vad_amd/dist.py, reduce_dtype). */
int lstc_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream);
int lstc_cast_bf16_f32(const void* x, float* y, int64_t n, void* stream);

/* ------------------------------------------------------------------------- data feed
 * dst[r, :] = src[idx[r], :] for r < n_rows, rows of `row_floats` contiguous floats (multiple of 4, 16-byte aligned
 * bases).  Forms the [B, part_num*part_len, n_patch, d] training batch out of an HBM-resident feature bank from the
 * clip indices the reference's sampler picks on the host (`feat[chosen[...], :]`, utils/load_dataset.py:88 +
 * default collate), so no feature bytes cross PCIe per step.  idx entries must lie in [0, src_rows). */
int lstc_gather_rows(const float* src, int64_t src_rows, const int64_t* idx, float* dst, int64_t n_rows,
                     int64_t row_floats, void* stream);

/* Means of runs of clips of a bank [bank_clips, P, d] -> out [n_seg, P, d] (the 32 bins of a UCF video, Test/evaluation_UCF.py:54-62,
 * one launch for every video of a pool): out[s, p, :] = (sum over c < count[s] of bank[first[s] + c, p, :]) / count[s], the sum in
 * order from the first clip.  first (device int64 [n_seg]) and count (device int32 [n_seg]) are clamped into the bank and count to
 * >= 1, so a count of 1 is a bit-exact copy (the reference's `feats[r[i]]` arm of an empty bin).  With l2_normalize != 0 each row of
 * d values is then divided by max(||row||_2, 1e-12) (F.normalize(p=2, dim=-1) on token rows); the squares are reduced in a fixed
 * order.  A segment's bits do not depend on what shares the launch.  16-B accesses when d % 4 == 0 and both bases are 16-B aligned,
 * 4-B ones otherwise (the means are the same bits; the norm's summation order differs between the two). */
int lstc_segment_mean(const float* bank, int64_t bank_clips, const int64_t* first, const int32_t* count, int64_t n_seg, int32_t P,
                      int32_t d, int32_t l2_normalize, float* out, void* stream);

/* dst[j][m, :] = src[j][map[m], :] for m < rows and j < n (1 <= n <= 3) matrices of `cols` floats per row, in ONE launch: the
 * ordinary [M, H d_k] Q, K and V of layer 0 out of the projections of the unique rows of a batch whose windows overlap
 * (DESIGN 3.2).  `src`, `dst`, `ld_src`, `ld_dst` are HOST arrays of n entries (device pointers; row strides in floats >= cols).
 * `map` is a device array of `rows` int32 row numbers into the sources; the kernel takes it as given and clamps nothing, so
 * every entry must name a row the sources hold.  Bases 16-byte aligned, cols and every row stride multiples of 4
 * (LSTC_E_ALIGN / LSTC_E_SHAPE), rows <= 2^31; n outside 1..3 LSTC_E_SHAPE; all refusals before the launch. */
int lstc_expand_rows(const float* const* src, const int64_t* ld_src, float* const* dst, const int64_t* ld_dst, int32_t n,
                     const int32_t* map, int64_t rows, int32_t cols, void* stream);

/* The mirror image of lstc_expand_rows: dst[j][u, :] = sum of src[j][order[k], :] over ptr[u] <= k < ptr[u + 1], for u < groups
 * and j < n (1 <= n <= 3) matrices of `cols` floats per row, in ONE launch - the sums of the rows of dQ, dK, dV that share an input
 * row, which layer 0's weight gradients contract with the distinct input rows.  A sum starts from its first row's
 * value and adds the others left to right in f32: a group of one is a bit-for-bit copy, and the result depends on the inputs alone
 * (no atomics).  Rows groups .. dst_rows - 1 of every destination, and the rows of empty groups, are written as zeros.  `src`,
 * `dst`, `ld_src`, `ld_dst` are HOST arrays of n entries (device pointers; row strides in floats >= cols); the sources hold
 * `src_rows` rows.  `order` (int32, src_rows entries: source rows sorted by group, ascending inside a group) and `ptr` (int32,
 * groups + 1 entries) are device arrays; the kernel clamps ptr into [0, src_rows] and order into the source, so a bad table cannot
 * fault.  Bases 16-byte aligned, cols and every row stride multiples of 4 (LSTC_E_ALIGN / LSTC_E_SHAPE); src_rows, groups >= 1,
 * groups <= dst_rows <= 2^31 - 1; n outside 1..3 LSTC_E_SHAPE; all refusals before the launch. */
int lstc_segment_sum_rows(const float* const* src, const int64_t* ld_src, float* const* dst, const int64_t* ld_dst, int32_t n,
                          const int32_t* order, const int32_t* ptr, int64_t src_rows, int64_t groups, int64_t dst_rows, int32_t cols,
                          void* stream);

/* --------------------------------------------------------------------------- metrics
 * Frame-level ROC-AUC of a pass without its host tail (replaces utils/eval_utils.py:21-24,139-143 - sklearn roc_curve + auc over
 * the frame scores - for passes whose frame scores only repeat row scores).  Row i has score scores[i] and covers pos[i] frames
 * labelled 1 and neg[i] frames labelled 0; the tie-aware trapezoid AUC of the expanded frames is the weighted pair count
 *     u2 = sum_i sum_j pos[i] neg[j] (2 [scores[i] > scores[j]] + [scores[i] == scores[j]]),   auc = u2 / (2 P N),
 * P = sum pos, N = sum neg.  The floats are compared with > and ==: +0.0 and -0.0 tie, denormals order as on the host.
 *   - a row with pos == neg == 0 does not exist: its score is never looked at, NaN included;
 *   - u2, pos (= P) and neg (= N) are exact integers, whatever the launch shape (integer partials, no atomics);
 *   - auc = (double)u2 / (2.0 * P * N), one IEEE division; NaN when P == 0 or N == 0;
 *   - flags & LSTC_AUC_NAN_SCORE: a row with non-zero weight has a NaN score; auc is NaN;
 *   - flags & LSTC_AUC_TOO_MANY_FRAMES: P + N > 2^26 (the bound keeps the per-thread 32-bit counts and 2 P N < 2^53 safe); auc
 *     is NaN and u2 is not meaningful.
 * All buffers are device memory owned by the caller; `workspace` holds at least lstc_auc_workspace_bytes(n) bytes at any
 * alignment (its content before and after the call is unspecified), `out` is 8-byte aligned (else LSTC_E_ALIGN).  Two launches on
 * `stream`, no allocation, no synchronisation: the call can be captured in a graph.  Checked before any launch: a NULL pointer
 * LSTC_E_NULL; n <= 0 LSTC_E_SHAPE; n > 2^24 LSTC_E_RANGE; workspace_bytes too small LSTC_E_SHAPE.
 * lstc_auc_workspace_bytes is positive and monotone in n (n is clamped into 1..2^24). */
typedef struct {
    uint64_t u2, pos, neg;
    double auc;
    uint32_t flags;
    uint32_t reserved;
} LstcAucOut;                           /* 40 bytes */
#define LSTC_AUC_NAN_SCORE 1u
#define LSTC_AUC_TOO_MANY_FRAMES 2u
int64_t lstc_auc_workspace_bytes(int64_t n);
int lstc_auc_weighted(const float* scores, const uint32_t* pos, const uint32_t* neg, int64_t n, void* workspace,
                      int64_t workspace_bytes, LstcAucOut* out, void* stream);

/* The detection report of the same rows (replaces utils/eval_utils.py:16-19, 26-95, 97-122, 145-148 - sklearn's
 * precision_recall_curve + auc and average_precision_score, the thresholded confusion family, the score statistics and the
 * per-class table - for passes whose frame scores only repeat row scores).  scores / pos / neg as above; gid[i] < n_groups is the
 * group (class) of row i, a row with gid[i] >= n_groups belongs to no group and is counted nowhere; gid == NULL puts every row in
 * group 0 and needs n_groups == 1.  A row with pos == neg == 0 does not exist: its score is never looked at, NaN included.
 * For every row i that covers a positive frame a pair kernel counts, over the rows j of i's group and in 32-bit integers,
 *     tp_ge = sum pos[j] [s_j >= s_i],  fp_ge = sum neg[j] [s_j >= s_i],  tp_eq, fp_eq: the same sums under s_j == s_i
 * (>= and == on the floats: +0.0 and -0.0 tie, a NaN compares false); they do not depend on the launch shape (slices of rows j
 * meet in integer atomics; no float atomic anywhere).  A finish kernel - one workgroup per group, fixed thread -> row assignment,
 * fixed reduction tree, so every double below has one summation order - writes out[g], with P = pos, N = neg of the group:
 *   - u2 = sum pos_i (2 (N - fp_ge) + fp_eq) and auc = (double)u2 / (2.0 * P * N): for an ungrouped call the u2 and the auc bits of
 *     lstc_auc_weighted; auc is NaN when P == 0 or N == 0;
 *   - ap = (sum pos_i prec_i) / P, prec_i = tp_ge / (tp_ge + fp_ge): sklearn's average_precision_score of the expanded frames;
 *   - pr_auc = (sum pos_i (prec_i + prev_i) / 2) / P, prev_i = (tp_ge - tp_eq) / ((tp_ge - tp_eq) + (fp_ge - fp_eq)), 1.0 when that
 *     denominator is 0 (sklearn's closing point: recall 0, precision 1): the trapezoid area under precision_recall_curve; ap and
 *     pr_auc are NaN when P == 0; every per-row division is an IEEE double division;
 *   - tp_at[t] = sum pos_i [s_i > thresholds[t]], fp_at[t] = sum neg_i [s_i > thresholds[t]] (strict, as cal_false_alarm), 0 for
 *     t >= n_thresholds: with P and N the whole confusion matrix at every threshold;
 *   - sum_s_pos = sum pos_i s_i, sum_s_neg = sum neg_i s_i, sum_sq_err = sum (pos_i (1 - s_i)^2 + neg_i s_i^2), in double (score
 *     gap, cal_pAUC, RMSE);
 *   - flags & LSTC_DET_NAN_SCORE: a row of the group with weight has a NaN score; flags & LSTC_DET_TOO_MANY_FRAMES: P + N > 2^26
 *     (the bound keeps the 32-bit counts safe).  With a flag every double is NaN; pos, neg, tp_at, fp_at and u2 stay the integers
 *     of the rows with a real score (pos and neg count the NaN rows too).
 * All buffers are device memory owned by the caller; `workspace` holds at least lstc_det_workspace_bytes(n, n_groups) =
 * 16 min(max(n, 1), 2^20) + 16 bytes at any alignment (content unspecified before and after), `out` holds n_groups records and is
 * 8-byte aligned.  At most one memset node and two launches on `stream`, no allocation, no synchronisation: capturable.
 * Checked before any launch: a NULL pointer (gid apart) LSTC_E_NULL; n <= 0, n_groups <= 0, n_thresholds outside 1..8, gid NULL
 * with n_groups != 1, workspace too small LSTC_E_SHAPE; n > 2^20 or n_groups > 64 LSTC_E_RANGE; `out` off an 8-byte boundary
 * LSTC_E_ALIGN.  The row limit is 2^20, not the AUC's 2^24: the work is quadratic with about twice the AUC kernel's instructions
 * per pair, 2^20 rows are about 28 of the largest lists scored here, and a call at 2^24 rows would occupy a shared GPU for minutes. */
typedef struct {
    uint64_t pos, neg, u2;
    uint64_t tp_at[8], fp_at[8];
    double auc, ap, pr_auc, sum_s_pos, sum_s_neg, sum_sq_err;
    uint32_t flags;
    uint32_t reserved;
} LstcDetOut;                           /* 208 bytes */
#define LSTC_DET_NAN_SCORE 1u
#define LSTC_DET_TOO_MANY_FRAMES 2u
int64_t lstc_det_workspace_bytes(int64_t n, int64_t n_groups);
int lstc_det_report(const float* scores, const uint32_t* pos, const uint32_t* neg, const uint32_t* gid, int64_t n, int64_t n_groups,
                    const float* thresholds, int32_t n_thresholds, void* workspace, int64_t workspace_bytes, LstcDetOut* out,
                    void* stream);

/* ------------------------------------------------------------------------------ misc */
int lstc_version(void);
const char* lstc_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* LSTC_HIP_H */
