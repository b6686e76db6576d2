// Key-tiled attention core for long sequences (128 < S <= 512), gfx950.
//
// The short-sequence kernels (csrc/attention.hip, csrc/attention_pk.hip) keep a whole S x S logit tile in LDS; at S = 512 that
// is 1 MB, so this path tiles the keys instead and never holds more than one 32 x 32 tile of a (query block, key block) pair in
// registers.  Same contract as the short path (include/lstc_hip.h, "attention"): scaled Q K^T, the relative bias gathered as
// table[index[(i-1)*index_ld + (j-1)], h] on rows and columns 1..S-1, softmax, P saved before dropout, the counter-based
// dropout mask of element (n, h, i, j), O = Pd V head-merged; the backward reads the saved P and regenerates only the mask.
//
// Fragment orientation.  A v_mfma_*_32x32 result X[a][b] has b on the lane (lane & 31) and a in the 16 registers (row
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), and a following MFMA that sums over a takes X as its A operand with no lane movement
// (csrc/attention.hip mma8: lane half h supplies the k values of its registers, the other operand reads the same rows).
//   forward:  X = K_blk Q_blk^T (keys in registers, one query per lane): the softmax row statistics are in-lane plus one
//             exchange between the lane halves, and O += X^T V needs no transpose.  The probabilities go out through a per-wave
//             32 x 33 LDS image so that every store instruction writes two whole 128-B row segments.
//   backward: X = dO_blk V_blk^T (queries in registers, one key per lane): P is read as 128-B row segments, dV += Pd^T dO and
//             dK += dA^T Q take X as it lies; dQ += dA K sums over the key (lane) index and goes through the LDS image once.
// Products on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32) for LSTC_F32, on v_mfma_f32_32x32x16_bf16 over RNE-rounded operands
// with f32 accumulation for LSTC_BF16.  Softmax, bias, dropout and every array in memory stay f32.
//
// Forward: one wave per (sequence, head, 32-query block), 4 independent waves per workgroup, no block barrier.  Sweep 1 runs
// the key blocks for the online row max and sum; sweep 2 recomputes the logits, writes normalised P and accumulates Pd V
// (d_v in groups of up to 256 columns; a further group repeats sweep 2).
// Backward: one workgroup per (chunk of sequences, head), as the short kernels.  Per sequence: (R) query blocks over the waves,
// rowsum(dP' * P) into LDS; (V) key blocks, dV = Pd^T dO; (K) key blocks, dK = dA^T Q scale; (Q) query blocks, dQ = dA K scale,
// and the bias-table gradient into one LDS table per wave.  Every sum has a fixed order (static wave -> block assignment, one
// writer per output element, no atomics), so the result is bit-reproducible run to run.
#include "attention_common.h"

namespace lstc_attn {
namespace {

constexpr int LNW = 4;                 // waves per workgroup
constexpr int LNT = 64 * LNW;
constexpr int TLD = 33;                // row pitch of the per-wave 32 x 32 transpose image (conflict-free both ways)
constexpr int LMAXS = 512;

// 32x32 accumulator += A[32 x 16] B[16 x 32] with lane half h supplying its eight k values of both operands (the idea of
// csrc/attention.hip's mma8): eight exact-f32 MFMAs, or one bf16 MFMA on the RNE-rounded values.
template <bool BF>
__device__ __forceinline__ floatx16 lmma8(const float* a, const float* b, floatx16 acc) {
    if constexpr (BF) {
        attn_h8 ah, bh;
#pragma unroll
        for (int s = 0; s < 8; ++s) { ah[s] = (__bf16)a[s]; bh[s] = (__bf16)b[s]; }
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
        return acc;
    }
}

// row of accumulator register r for lane half h2
__device__ __forceinline__ int frow(int r, int h2) { return (r & 3) + 8 * (r >> 2) + 4 * h2; }

__device__ __forceinline__ void lload16(const float* __restrict__ p, int k0, int kdim, bool vec, float (&f)[16]) {
    if (vec && k0 + 16 <= kdim) {
        const float4* q = reinterpret_cast<const float4*>(p + k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = q[i];
            f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = (k0 + e < kdim) ? p[k0 + e] : 0.f;
    }
}

// X[a][b] = sum_k A[a0 + a][k] * (B[b0 + b][k] * b_scale): b on the lane, a in the registers.  Rows past S - 1 are clamped
// (the caller discards what they produce).
template <bool BF>
__device__ __forceinline__ floatx16 tile_xt(const float* __restrict__ A, int lda, int a0, const float* __restrict__ B, int ldb,
                                            int b0, int S, int kdim, float b_scale, bool vec) {
    const int lane = threadIdx.x & 63, r = lane & 31, h2 = lane >> 5;
    const float* pa = A + (size_t)min(a0 + r, S - 1) * lda;
    const float* pb = B + (size_t)min(b0 + r, S - 1) * ldb;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 1
    for (int kb = 0; kb < kdim; kb += 32) {
        float a[16], b[16];
        lload16(pa, kb + 16 * h2, kdim, vec, a);
        lload16(pb, kb + 16 * h2, kdim, vec, b);
#pragma unroll
        for (int s = 0; s < 16; ++s) b[s] *= b_scale;
        acc = lmma8<BF>(a, b, acc);
        acc = lmma8<BF>(a + 8, b + 8, acc);
    }
    return acc;
}

// acc[dt] += X^T B[rows t0.., g0 + 32 dt ..]: X (16 registers per lane, rows t0 + frow(r)) is the A operand as it lies, the B
// operand is read as 128-B row segments of B (columns >= ncols and rows >= S read as zero / clamped: X is zero there).
template <bool BF, int DT>
__device__ __forceinline__ void acc_xtb(floatx16 (&acc)[DT], const float (&x)[16], const float* __restrict__ B, int ldb, int t0,
                                        int S, int g0, int ncols) {
    const int lane = threadIdx.x & 63, c = lane & 31, h2 = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = g0 + 32 * dt + c;
        if (g0 + 32 * dt >= ncols) break;                 // wave-uniform
        const bool cv = col < ncols;
        float b[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) b[r] = cv ? B[min(t0 + frow(r, h2), S - 1) * ldb + col] : 0.f;   // S * ld < 2^31 (long_check)
        acc[dt] = lmma8<BF>(x, b, acc[dt]);
        acc[dt] = lmma8<BF>(x + 8, b + 8, acc[dt]);
    }
}

template <int DT>
__device__ __forceinline__ void store_acc(const floatx16 (&acc)[DT], float* __restrict__ Out, int ldo, int t0, int S, int g0,
                                          int ncols, float scale) {
    const int lane = threadIdx.x & 63, c = lane & 31, h2 = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = g0 + 32 * dt + c;
        if (col >= ncols) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = t0 + frow(r, h2);
            if (row < S) Out[(size_t)row * ldo + col] = acc[dt][r] * scale;
        }
    }
}

template <int DT>
__device__ __forceinline__ void zero_acc(floatx16 (&acc)[DT]) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
}

// attn_long_fwd_kernel<BF, DT> / attn_long_bwd_kernel<BF, DT>: the kernel text is in attention_long.inc, included once under the kernels' own names
// (unmasked: exactly the text they always had) and once as the *_masked_kernel instantiations, which take the attention mask
// (attention_common.h MaskParams) as a second argument.
#define ATTN_MASKED 0
#define ATTN_MASK_PARAM
#define ATTN_LONG_FWD attn_long_fwd_kernel
#define ATTN_LONG_BWD attn_long_bwd_kernel
#include "attention_long.inc"
#undef ATTN_MASKED
#undef ATTN_MASK_PARAM
#undef ATTN_LONG_FWD
#undef ATTN_LONG_BWD
#define ATTN_MASKED 1
#define ATTN_MASK_PARAM , const MaskParams mk
#define ATTN_LONG_FWD attn_long_fwd_masked_kernel
#define ATTN_LONG_BWD attn_long_bwd_masked_kernel
#include "attention_long.inc"
#undef ATTN_MASKED
#undef ATTN_MASK_PARAM
#undef ATTN_LONG_FWD
#undef ATTN_LONG_BWD

template <typename Kern>
void long_set_lds(Kern k, size_t lds) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// 32-column output tiles per group: enough for max(d_k, d_v) up to 256 in one group
int long_dt(int dk, int dv) {
    const int t = ((dk > dv ? dk : dv) + 31) / 32;
    return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : 8;
}

// Preconditions shared by forward and backward (fill_params has run): row inputs and outputs, d_k and d_v multiples of 16,
// dense probs, S <= 512.  Packed forms are refused first (LSTC_E_UNSUPPORTED), the rest as a range error.
int long_check(const LstcAttnDesc* d, bool bwd) {
    if (d->in_pack_cols > 0 || d->O_pack || d->dO_pack_cols > 0 || d->dQ_pack || d->dK_pack || d->dV_pack) return LSTC_E_UNSUPPORTED;
    if (d->S > LMAXS || d->dk % 16 || d->dv % 16 || (d->probs_ld != 0 && d->probs_ld != d->S)) return LSTC_E_RANGE;
    if (!d->O && !bwd) return LSTC_E_NULL;
    const int64_t ldmax = d->ldq > d->ldk ? (d->ldq > d->ldv ? d->ldq : d->ldv) : (d->ldk > d->ldv ? d->ldk : d->ldv);
    if ((int64_t)d->S * (ldmax > d->ldo ? ldmax : d->ldo) >= 0x7fffffffLL) return LSTC_E_RANGE;     // 32-bit offsets within a sequence
    return 0;
}

}  // namespace

static int long_fwd_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams* mk, hipStream_t st) {
    int rc = long_check(d, false);
    if (rc) return rc;
    const int QT = (p.S + 31) / 32;
    const uint64_t waves = (uint64_t)p.N * p.H * QT;
    const dim3 grid((unsigned)((waves + LNW - 1) / LNW));
    const bool bf = d->dtype == LSTC_BF16;
#define LSTC_LFWD(BB, DD)                                                                              \
    do {                                                                                               \
        if (mk) hipLaunchKernelGGL((attn_long_fwd_masked_kernel<BB, DD>), grid, LNT, 0, st, p, *mk);   \
        else hipLaunchKernelGGL((attn_long_fwd_kernel<BB, DD>), grid, LNT, 0, st, p);                  \
    } while (0)
    switch (long_dt(p.dk, p.dv)) {
        case 1: if (bf) LSTC_LFWD(true, 1); else LSTC_LFWD(false, 1); break;
        case 2: if (bf) LSTC_LFWD(true, 2); else LSTC_LFWD(false, 2); break;
        case 4: if (bf) LSTC_LFWD(true, 4); else LSTC_LFWD(false, 4); break;
        default: if (bf) LSTC_LFWD(true, 8); else LSTC_LFWD(false, 8); break;
    }
#undef LSTC_LFWD
    return lstc_launch_status();
}

int attn_long_fwd_launch(const LstcAttnDesc* d, AttnParams& p, hipStream_t st) { return long_fwd_launch(d, p, nullptr, st); }
int attn_long_fwd_masked_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams& mk, hipStream_t st) {
    return long_fwd_launch(d, p, &mk, st);
}

static int long_bwd_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams* mk, hipStream_t st) {
    int rc = long_check(d, true);
    if (rc) return rc;
    const bool has_table = d->index_ld > 0 && d->dtable;
    if (has_table && d->table_rows <= 0) return LSTC_E_SHAPE;
    if (has_table && d->dtable_chunks <= 0) return LSTC_E_UNSUPPORTED;       // partial tables only: no float atomics
    p.table_rows = has_table ? d->table_rows : 0;
    p.table_partials = has_table ? 1 : 0;
    const size_t lds = ((size_t)LMAXS + (size_t)LNW * 32 * TLD + (size_t)LNW * p.table_rows) * sizeof(float);
    if (lds > 160 * 1024) return LSTC_E_RANGE;
    const int npw = has_table ? (p.N + d->dtable_chunks - 1) / d->dtable_chunks : 1;
    const int chunks = (p.N + npw - 1) / npw;
    if (has_table && chunks != d->dtable_chunks) return LSTC_E_SHAPE;
    p.n_per_wg = npw;
    const dim3 grid((unsigned)chunks, (unsigned)p.H);
    const bool bf = d->dtype == LSTC_BF16;
#define LSTC_LBWD(BB, DD)                                                                              \
    do {                                                                                               \
        static LstcDevOnce once;                                                                       \
        const int dev_ = once.begin();                                                                 \
        if (dev_ >= 0) {                                                                               \
            long_set_lds(attn_long_bwd_kernel<BB, DD>, 160 * 1024);                                    \
            long_set_lds(attn_long_bwd_masked_kernel<BB, DD>, 160 * 1024);                             \
            once.end(dev_);                                                                            \
        }                                                                                              \
        if (mk) hipLaunchKernelGGL((attn_long_bwd_masked_kernel<BB, DD>), grid, LNT, lds, st, p, *mk); \
        else hipLaunchKernelGGL((attn_long_bwd_kernel<BB, DD>), grid, LNT, lds, st, p);                \
    } while (0)
    switch (long_dt(p.dk, p.dv)) {
        case 1: if (bf) LSTC_LBWD(true, 1); else LSTC_LBWD(false, 1); break;
        case 2: if (bf) LSTC_LBWD(true, 2); else LSTC_LBWD(false, 2); break;
        case 4: if (bf) LSTC_LBWD(true, 4); else LSTC_LBWD(false, 4); break;
        default: if (bf) LSTC_LBWD(true, 8); else LSTC_LBWD(false, 8); break;
    }
#undef LSTC_LBWD
    return lstc_launch_status();
}

int attn_long_bwd_launch(const LstcAttnDesc* d, AttnParams& p, hipStream_t st) { return long_bwd_launch(d, p, nullptr, st); }
int attn_long_bwd_masked_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams& mk, hipStream_t st) {
    return long_bwd_launch(d, p, &mk, st);
}

}  // namespace lstc_attn
