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

// MASKED: the mask (attention_common.h MaskParams) as the second argument; the unmasked instantiation compiles to what the kernel
// was before masks existed (tools/isa_diff.py).
// VAR (lstc_attn_var_long_fwd / _bwd): the sequence, its length and its operand rows come from the offset tables of `sq` (the
// third argument, attention_common.h SeqParams; empty for the fixed-S kernels, which compile to what they were without it) -
// sequence n = rows row0[n] .. row0[n + 1] - 1, its probabilities [H, S_n, S_n] from prob0[n], which is also the dropout counter
// of its first element.  S_n is clamped to [1, 32 ceil(p.S / 32)]; the query and key block counts are the sequence's own.  The
// forward's jobs are (sequence, head, query block) with the block count of p.S, the longest sequence of the launch: a wave whose
// block lies behind its sequence's end returns at once (there is no block barrier to miss).
template <bool BF, int DT, bool MASKED, bool VAR = false>
__global__ void __launch_bounds__(LNT, DT == 8 ? 1 : 2) attn_long_fwd_kernel(const AttnParams p, const MaskArg<MASKED> mk, const SeqArg<VAR> sq) {
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ float trs[LNW][32 * TLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h2 = lane >> 5;
    int S = p.S;
    const int QTL = (S + 31) >> 5;                    // query blocks per (sequence, head) of the launch
    const uint32_t job = blockIdx.x * LNW + wave;
    if (job >= (uint32_t)(VAR ? seq_count(sq) : p.N) * (uint32_t)p.H * (uint32_t)QTL) return;      // no block barrier in this kernel
    const int qt = (int)(job % (uint32_t)QTL);
    const uint32_t nh = job / (uint32_t)QTL;
    const int h = (int)(nh % (uint32_t)p.H);
    int n = (int)(nh / (uint32_t)p.H);
    size_t r0;                                        // the sequence's first row
    if constexpr (VAR) {
        if (sq.ids) n = sq.ids[n];
        const int b = sq.row0[n];
        S = min(max(sq.row0[n + 1] - b, 1), 32 * QTL);
        if (32 * qt >= S) return;                     // a block behind the end of a shorter sequence
        r0 = (size_t)b;
    } else {
        r0 = (size_t)n * S;
    }
    const int QT = (S + 31) >> 5, KT = QT;
    const float* Qb = p.Q + r0 * p.ldq + (size_t)h * p.dk;
    const float* Kb = p.K + r0 * p.ldk + (size_t)h * p.dk;
    const float* Vb = p.V + r0 * p.ldv + (size_t)h * p.dv;
    float* Ob = p.O + r0 * p.ldo + (size_t)h * p.dv;
    float* tr = trs[wave];
    const int q = 32 * qt + c;                        // this lane's query
    const bool bias = p.index_ld > 0 && q >= 1 && q < S;
    const int64_t* irow = p.index + (size_t)(bias ? q - 1 : 0) * p.index_ld;
    const float* tabh = p.table + h;
    const uint8_t* mk_nh = nullptr;
    if constexpr (MASKED) mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;

    // logits of key block kt for this lane's query: register r = key 32 kt + frow(r); keys >= S -> -inf
    auto logits = [&](int kt, floatx16& x) {
        x = tile_xt<BF>(Kb, p.ldk, 32 * kt, Qb, p.ldq, 32 * qt, S, p.dk, p.scale, p.vec_qk);
        // Masked (both sweeps): the bytes of the tile are read in the lane order in which P is written (lane = key: one 32-byte run
        // per query row, two rows per load), turned through the wave's transpose image to the logits' orientation (lane = query) and
        // applied as a predicated select before the bias.  A fully masked row has the running max ATTN_MASK_FILL and comes out uniform;
        // a fully masked key block of a row that keeps a key adds exp(-1e9 - m) = 0 exactly; only the padding keys >= S are -inf.
        // sq == 0 (a key-padding mask): the byte depends on the key alone, which is the register index here - the 32 lanes of a half
        // read one and the same byte per load, and nothing goes through the image.
        if constexpr (MASKED) {
            if (mk.sq == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = 32 * kt + frow(r, h2);
                    x[r] = (j >= S || mk_nh[(int64_t)j * mk.sk]) ? x[r] : ATTN_MASK_FILL;
                }
            } else {
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int i = 32 * qt + 2 * rr + h2, j = 32 * kt + c;
                    tr[(2 * rr + h2) * TLD + c] = (i < S && j < S) ? (float)mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk] : 1.f;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 16; ++r) x[r] = tr[c * TLD + frow(r, h2)] != 0.f ? x[r] : ATTN_MASK_FILL;
                __builtin_amdgcn_wave_barrier();
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = 32 * kt + frow(r, h2);
            if (j >= S) x[r] = -INFINITY;
            else if (bias && j >= 1) x[r] += tabh[(size_t)irow[j - 1] * p.H];
        }
    };

    // sweep 1: online row max / sum (the two lane halves hold the two halves of each key block)
    float m = -INFINITY, l = 0.f;
#pragma unroll 1
    for (int kt = 0; kt < KT; ++kt) {
        floatx16 x;
        logits(kt, x);
        float tm = x[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tm = fmaxf(tm, x[r]);
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);
        float ts = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ts += expf(x[r] - mn);
        ts += __shfl_xor(ts, 32, 64);
        l = l * expf(m - mn) + ts;
        m = mn;
    }

    float* pr_base;
    uint32_t flat0;
    if constexpr (VAR) {
        const int64_t e0 = sq.prob0[n] + (int64_t)h * S * S;
        pr_base = p.probs + e0;
        flat0 = (uint32_t)e0;
    } else {
        pr_base = p.probs + ((size_t)n * p.H + h) * S * S;
        flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
    }
    // sweep 2 (once per group of up to 32 DT output columns): normalised P, its dropout, O += Pd V
#pragma unroll 1
    for (int g0 = 0; g0 < p.dv; g0 += 32 * DT) {
        floatx16 acc[DT];
        zero_acc<DT>(acc);
#pragma unroll 1
        for (int kt = 0; kt < KT; ++kt) {
            floatx16 x;
            logits(kt, x);
            float pd[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * kt + frow(r, h2);
                const float pv = j < S ? expf(x[r] - m) / l : 0.f;
                pd[r] = pv;
                if (g0 == 0) tr[c * TLD + frow(r, h2)] = pv;
                if (p.has_drop) pd[r] = drop_keep(flat0 + (uint32_t)(q * S + j), dkn) ? pv * dkn.scale : 0.f;
            }
            if (g0 == 0) {           // P rows out of the transpose image: two 128-B row segments per store
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int i = 32 * qt + 2 * rr + h2, j = 32 * kt + c;
                    const float v = tr[(2 * rr + h2) * TLD + c];
                    if (i < S && j < S) pr_base[(size_t)i * S + j] = v;
                }
                __builtin_amdgcn_wave_barrier();
            }
            acc_xtb<BF, DT>(acc, pd, Vb, p.ldv, 32 * kt, S, g0, p.dv);
        }
        store_acc<DT>(acc, Ob, p.ldo, 32 * qt, S, g0, p.dv, 1.f);
    }
}

// VAR: one workgroup per (chunk of the call's n_ids sequences, head) as the fixed form; the row sums in Dr, the barriers and the four
// passes run per sequence on its own S_n, and the bias-table gradient leaves as one partial table per chunk (as it always does here).
template <bool BF, int DT, bool MASKED, bool VAR = false>
__global__ void __launch_bounds__(LNT, 1) attn_long_bwd_kernel(const AttnParams p, const MaskArg<MASKED> mk, const SeqArg<VAR> sq) {
    const DropKey dkn = drop_key_now(p.dkey);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h2 = lane >> 5;
    float* Dr = sm;                                       // [LMAXS] rowsum(dP' * P) of the current sequence
    float* tr = sm + LMAXS + wave * 32 * TLD;             // this wave's transpose image
    float* tacc = sm + LMAXS + LNW * 32 * TLD;            // [LNW][table_rows] bias-table gradient, one copy per wave
    const int h = (int)blockIdx.y, SL = p.S, QTL = (SL + 31) >> 5;          // the launch's S and block count; VAR: each sequence's own below
    const bool has_bias = p.index_ld > 0 && p.dtable != nullptr;
    if (has_bias)
        for (int i = threadIdx.x; i < LNW * p.table_rows; i += LNT) tacc[i] = 0.f;
    float* const tw = tacc + wave * p.table_rows;
    const int n_begin = (int)blockIdx.x * p.n_per_wg;
    const int n_end = min(VAR ? seq_count(sq) : p.N, n_begin + p.n_per_wg);
#pragma unroll 1
    for (int it = n_begin; it < n_end; ++it) {
        const int n = seq_id(sq, it);
        const int S = VAR ? seq_len(sq, n, 32 * QTL) : SL;
        const int QT = VAR ? (S + 31) >> 5 : QTL, KT = QT;
        const size_t r0 = VAR ? seq_row0(sq, n) : (size_t)n * S;          // the sequence's first row
        const float* Qb = p.Q + r0 * p.ldq + (size_t)h * p.dk;
        const float* Kb = p.K + r0 * p.ldk + (size_t)h * p.dk;
        const float* Vb = p.V + r0 * p.ldv + (size_t)h * p.dv;
        const float* dOb = p.dO + r0 * p.ldo + (size_t)h * p.dv;
        const float* Pb;
        uint32_t flat0;
        if constexpr (VAR) {
            const int64_t e0 = sq.prob0[n] + (int64_t)h * S * S;
            Pb = p.probs + e0;
            flat0 = (uint32_t)e0;
        } else {
            Pb = p.probs + ((size_t)n * p.H + h) * S * S;
            flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
        }
        const uint8_t* mk_nh = nullptr;
        if constexpr (MASKED) mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
        // masked only.  bit r: the mask keeps (query of register r, this lane's key) - read with P's lane order, one 32-byte run per query row
        auto keep_bits = [&](int qt, int kt) -> uint32_t {
            if constexpr (MASKED) {
                const int j = 32 * kt + c;
                if (mk.sq == 0)       // a key-padding mask: one byte per lane serves all sixteen queries
                    return (j >= S || mk_nh[(int64_t)j * mk.sk]) ? 0xFFFFu : 0u;
                uint32_t km = 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = 32 * qt + frow(r, h2);
                    const bool k1 = (i < S && j < S) ? mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk] != 0 : true;
                    km |= (k1 ? 1u : 0u) << r;
                }
                return km;
            } else {
                return 0xFFFFu;
            }
        };

        // dP' tile of (query block qt, key block kt) with P and the keep factor: queries in the registers, one key per lane
        auto dp_tile = [&](int qt, int kt, float (&pv)[16], float (&dpk)[16]) {
            const floatx16 x = tile_xt<BF>(dOb, p.ldo, 32 * qt, Vb, p.ldv, 32 * kt, S, p.dv, 1.f, p.vec_v);
            const int j = 32 * kt + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * qt + frow(r, h2);
                pv[r] = dpk[r] = 0.f;
                if (i < S && j < S) {
                    pv[r] = Pb[(size_t)i * S + j];
                    const float keep = p.has_drop ? (drop_keep(flat0 + (uint32_t)(i * S + j), dkn) ? dkn.scale : 0.f) : 1.f;
                    dpk[r] = x[r] * keep;
                }
            }
        };
        // dA = P (dP' - rowsum) of the tile, same layout
        auto da_tile = [&](int qt, int kt, float (&da)[16]) {
            float pv[16], dpk[16];
            dp_tile(qt, kt, pv, dpk);
#pragma unroll
            for (int r = 0; r < 16; ++r) da[r] = pv[r] * (dpk[r] - Dr[min(32 * qt + frow(r, h2), LMAXS - 1)]);
        };

        __syncthreads();      // the previous sequence's readers of Dr are done
        // (R) rowsum over the keys: per-lane partials over all key blocks, then one reduction across the 32 lanes of each half
#pragma unroll 1
        for (int qt = wave; qt < QT; qt += LNW) {
            float part[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) part[r] = 0.f;
#pragma unroll 1
            for (int kt = 0; kt < KT; ++kt) {
                float pv[16], dpk[16];
                dp_tile(qt, kt, pv, dpk);
#pragma unroll
                for (int r = 0; r < 16; ++r) part[r] += dpk[r] * pv[r];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = part[r];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (c == 0) Dr[32 * qt + frow(r, h2)] = v;
            }
        }
        __syncthreads();

        // (V) dV = Pd^T dO and (K) dK = dA^T Q scale: key blocks over the waves, query blocks inner
#pragma unroll 1
        for (int kt = wave; kt < KT; kt += LNW) {
            const int j = 32 * kt + c;
#pragma unroll 1
            for (int g0 = 0; g0 < p.dv; g0 += 32 * DT) {
                floatx16 acc[DT];
                zero_acc<DT>(acc);
#pragma unroll 1
                for (int qt = 0; qt < QT; ++qt) {
                    float pd[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int i = 32 * qt + frow(r, h2);
                        float v = 0.f;
                        if (i < S && j < S) {
                            v = Pb[(size_t)i * S + j];
                            if (p.has_drop) v = drop_keep(flat0 + (uint32_t)(i * S + j), dkn) ? v * dkn.scale : 0.f;
                        }
                        pd[r] = v;
                    }
                    acc_xtb<BF, DT>(acc, pd, dOb, p.ldo, 32 * qt, S, g0, p.dv);
                }
                store_acc<DT>(acc, p.dV + r0 * p.ldv + (size_t)h * p.dv, p.ldv, 32 * kt, S, g0, p.dv, 1.f);
            }
#pragma unroll 1
            for (int g0 = 0; g0 < p.dk; g0 += 32 * DT) {
                floatx16 acc[DT];
                zero_acc<DT>(acc);
#pragma unroll 1
                for (int qt = 0; qt < QT; ++qt) {
                    float da[16];
                    da_tile(qt, kt, da);
                    if constexpr (MASKED) {     // no gradient reaches q.k at a masked position
                        const uint32_t km = keep_bits(qt, kt);
#pragma unroll
                        for (int r = 0; r < 16; ++r) da[r] = ((km >> r) & 1u) ? da[r] : 0.f;
                    }
                    acc_xtb<BF, DT>(acc, da, Qb, p.ldq, 32 * qt, S, g0, p.dk);
                }
                store_acc<DT>(acc, p.dK + r0 * p.ldk + (size_t)h * p.dk, p.ldk, 32 * kt, S, g0, p.dk, p.scale);
            }
        }

        // (Q) dQ = dA K scale: query blocks over the waves, key blocks inner; dA goes through the transpose image (keys onto the
        // registers).  The bias-table gradient is taken here, where every (i, j) is visited once: one lane half at a time, so the
        // 32 lanes of a store share the query i and their distinct keys j hit distinct table rows (relative offsets of distinct
        // positions differ) - plain read-modify-write, race-free, in a fixed order.
#pragma unroll 1
        for (int qt = wave; qt < QT; qt += LNW) {
#pragma unroll 1
            for (int g0 = 0; g0 < p.dk; g0 += 32 * DT) {
                floatx16 acc[DT];
                zero_acc<DT>(acc);
#pragma unroll 1
                for (int kt = 0; kt < KT; ++kt) {
                    float da[16];
                    da_tile(qt, kt, da);
                    const int j = 32 * kt + c;
                    if (has_bias && g0 == 0) {
#pragma unroll 1
                        for (int half = 0; half < 2; ++half) {
                            if (h2 == half && j >= 1 && j < S) {
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const int i = 32 * qt + frow(r, h2);
                                    if (i >= 1 && i < S) tw[p.index[(size_t)(i - 1) * p.index_ld + (j - 1)]] += da[r];
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                    if constexpr (MASKED) {     // the bias table above took dA as it is (the bias is added after the fill); dQ takes it zeroed at masked positions
                        const uint32_t km = keep_bits(qt, kt);
#pragma unroll
                        for (int r = 0; r < 16; ++r) da[r] = ((km >> r) & 1u) ? da[r] : 0.f;
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) tr[frow(r, h2) * TLD + c] = da[r];
                    __builtin_amdgcn_wave_barrier();
                    float dat[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) dat[r] = tr[c * TLD + frow(r, h2)];
                    __builtin_amdgcn_wave_barrier();
                    acc_xtb<BF, DT>(acc, dat, Kb, p.ldk, 32 * kt, S, g0, p.dk);
                }
                store_acc<DT>(acc, p.dQ + r0 * p.ldq + (size_t)h * p.dk, p.ldq, 32 * qt, S, g0, p.dk, p.scale);
            }
        }
    }
    if (has_bias) {
        __syncthreads();
        for (int i = threadIdx.x; i < p.table_rows; i += LNT) {
            float v = tacc[i];
#pragma unroll
            for (int w = 1; w < LNW; ++w) v += tacc[w * p.table_rows + i];
            p.dtable[((size_t)blockIdx.x * p.table_rows + i) * p.H + h] = v;
        }
    }
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

int attn_long_fwd_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams* mk, hipStream_t st) {
    int rc = long_check(d, false);
    if (rc) return rc;
    const int QT = (p.S + 31) / 32;
    const uint64_t waves = (uint64_t)p.N * p.H * QT;
    const dim3 grid((unsigned)((waves + LNW - 1) / LNW));
    const bool bf = d->dtype == LSTC_BF16;
    const int dt = long_dt(p.dk, p.dv);
    auto go = [&](auto masked, const auto& mask_arg) {          // static LDS only
        constexpr bool M = decltype(masked)::value;
        switch (dt) {
            case 1: if (bf) hipLaunchKernelGGL((attn_long_fwd_kernel<true, 1, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{});
                    else hipLaunchKernelGGL((attn_long_fwd_kernel<false, 1, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{}); break;
            case 2: if (bf) hipLaunchKernelGGL((attn_long_fwd_kernel<true, 2, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{});
                    else hipLaunchKernelGGL((attn_long_fwd_kernel<false, 2, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{}); break;
            case 4: if (bf) hipLaunchKernelGGL((attn_long_fwd_kernel<true, 4, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{});
                    else hipLaunchKernelGGL((attn_long_fwd_kernel<false, 4, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{}); break;
            default: if (bf) hipLaunchKernelGGL((attn_long_fwd_kernel<true, 8, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{});
                     else hipLaunchKernelGGL((attn_long_fwd_kernel<false, 8, M>), grid, LNT, 0, st, p, mask_arg, NoSeqs{}); break;
        }
    };
    if (mk) go(std::true_type{}, *mk); else go(std::false_type{}, NoMask{});
    return lstc_launch_status();
}

int attn_long_bwd_launch(const LstcAttnDesc* d, AttnParams& p, const MaskParams* mk, hipStream_t st) {
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
    const int dt = long_dt(p.dk, p.dv);
    auto go = [&](auto masked, const auto& mask_arg) {
        constexpr bool M = decltype(masked)::value;
        switch (dt) {
            case 1: if (bf) launch_big_lds<attn_long_bwd_kernel<true, 1, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{});
                    else launch_big_lds<attn_long_bwd_kernel<false, 1, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{}); break;
            case 2: if (bf) launch_big_lds<attn_long_bwd_kernel<true, 2, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{});
                    else launch_big_lds<attn_long_bwd_kernel<false, 2, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{}); break;
            case 4: if (bf) launch_big_lds<attn_long_bwd_kernel<true, 4, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{});
                    else launch_big_lds<attn_long_bwd_kernel<false, 4, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{}); break;
            default: if (bf) launch_big_lds<attn_long_bwd_kernel<true, 8, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{});
                     else launch_big_lds<attn_long_bwd_kernel<false, 8, M>>(grid, LNT, lds, st, p, mask_arg, NoSeqs{}); break;
        }
    };
    if (mk) go(std::true_type{}, *mk); else go(std::false_type{}, NoMask{});
    return lstc_launch_status();
}

// The key-tiled kernels over sequence offsets (lstc_attn_var_long_fwd / _bwd; fill_var has run): exact-f32 products only - the
// unpadded route runs exact f32 in every compute mode, and the bf16 products are slower above S = 128 anyway - and no mask.
// Forward: skipped-wave jobs, no device job table.  A launch group holds the sequences above 128 tokens only (functional.SeqLayout),
// so a job table could spare no more than the waves between a sequence's own block count and the group's, which return after two
// scalar loads; the table would cost a host pass and an upload per layout.
int attn_long_var_fwd_launch(const LstcAttnDesc* d, AttnParams& p, const SeqParams& sq, hipStream_t st) {
    int rc = long_check(d, false);
    if (rc) return rc;
    const int QT = (p.S + 31) / 32;
    const uint64_t waves = (uint64_t)sq.n_ids * p.H * QT;
    if (waves > 0xffffffffull) return LSTC_E_RANGE;          // 32-bit job numbers
    const dim3 grid((unsigned)((waves + LNW - 1) / LNW));
    switch (long_dt(p.dk, p.dv)) {
        case 1: hipLaunchKernelGGL((attn_long_fwd_kernel<false, 1, false, true>), grid, LNT, 0, st, p, NoMask{}, sq); break;
        case 2: hipLaunchKernelGGL((attn_long_fwd_kernel<false, 2, false, true>), grid, LNT, 0, st, p, NoMask{}, sq); break;
        case 4: hipLaunchKernelGGL((attn_long_fwd_kernel<false, 4, false, true>), grid, LNT, 0, st, p, NoMask{}, sq); break;
        default: hipLaunchKernelGGL((attn_long_fwd_kernel<false, 8, false, true>), grid, LNT, 0, st, p, NoMask{}, sq); break;
    }
    return lstc_launch_status();
}

int attn_long_var_bwd_launch(const LstcAttnDesc* d, AttnParams& p, const SeqParams& sq, hipStream_t st) {
    int rc = long_check(d, true);
    if (rc) return rc;
    const bool has_table = d->index_ld > 0 && d->dtable;
    if (has_table && d->table_rows <= 0) return LSTC_E_SHAPE;
    if (has_table && d->dtable_chunks <= 0) return LSTC_E_UNSUPPORTED;       // partial tables only: no float atomics
    p.table_rows = has_table ? d->table_rows : 0;
    p.table_partials = 1;
    const size_t lds = ((size_t)LMAXS + (size_t)LNW * 32 * TLD + (size_t)LNW * p.table_rows) * sizeof(float);
    if (lds > 160 * 1024) return LSTC_E_RANGE;
    const int npw = has_table ? (sq.n_ids + d->dtable_chunks - 1) / d->dtable_chunks : 1;
    const int chunks = (sq.n_ids + npw - 1) / npw;
    if (has_table && chunks != d->dtable_chunks) return LSTC_E_SHAPE;
    p.n_per_wg = npw;
    const dim3 grid((unsigned)chunks, (unsigned)p.H);
    switch (long_dt(p.dk, p.dv)) {
        case 1: launch_big_lds<attn_long_bwd_kernel<false, 1, false, true>>(grid, LNT, lds, st, p, NoMask{}, sq); break;
        case 2: launch_big_lds<attn_long_bwd_kernel<false, 2, false, true>>(grid, LNT, lds, st, p, NoMask{}, sq); break;
        case 4: launch_big_lds<attn_long_bwd_kernel<false, 4, false, true>>(grid, LNT, lds, st, p, NoMask{}, sq); break;
        default: launch_big_lds<attn_long_bwd_kernel<false, 8, false, true>>(grid, LNT, lds, st, p, NoMask{}, sq); break;
    }
    return lstc_launch_status();
}

}  // namespace lstc_attn
