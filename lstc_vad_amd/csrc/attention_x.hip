// Rectangular scaled-dot-product attention (len_q != len_k allowed), forward and backward, gfx950: lstc_sdpa_fwd / lstc_sdpa_bwd
// (include/lstc_hip.h, "rectangular attention"; reference models/MultiHeadAttention.py:17-23).
//
//   A = (Q scale) K^T [N, H, Sq, Sk]; A = mask byte == 0 ? -1e9f : A; P = softmax(A, -1), saved before dropout; Pd = dropout(P);
//   O = Pd V.  No relative bias.  1 <= Sq, Sk <= 512 independently; d_k, d_v multiples of 16 up to 512.
//
// Q, K, V and O are addressed through three element strides each (sequence, head, token; feature stride 1), so head-major
// [b, H, l, d] tensors and transpose(1, 2) views of token-major [b, l, H d] projections both run without a copy.
//
// Fragment orientation as in csrc/attention_long.hip: 32 x 32 tiles of v_mfma_f32_32x32x2_f32 whose result
// X[a][b] has b on the lane and a in the 16 registers (row frow(r, lane >> 5)), so a following product that sums over a takes X
// as its A operand with no lane movement.
//   forward:  X = K_blk Q_blk^T (keys in the registers, one query per lane): row max and sum are in-lane plus one exchange
//             between the lane halves, O += X^T V needs no transpose, P goes out as 128-B row segments through a 32 x 33 image.
//   backward: X = dO_blk V_blk^T (queries in the registers, one key per lane): dV += Pd^T dO and dK += dA^T Q take X as it
//             lies, dQ += dA K goes through the image once; rowsum(dP' * P) of the sequence sits in LDS.
// Key blocks run to ceil(Sk / 32), query blocks to ceil(Sq / 32); padding keys get -inf, padding queries are discarded.
//
// Forward: one wave per (sequence, head, 32-query block), 4 independent waves per workgroup, no block barrier; two sweeps over
// the key blocks (online max / sum, then normalised P and Pd V; d_v in groups of up to 256 columns).
// Backward: one workgroup per (sequence, head); (R) query blocks over the waves, rowsum into LDS; (V, K) key blocks over the
// waves; (Q) query blocks over the waves.  Static wave -> block assignment, one writer per output element, every sum in a fixed
// order, no atomics: two runs are bitwise equal.
// Every product is the exact-f32 MFMA; softmax and dropout are f32.  Static LDS only (forward 16.5 KB, backward 18.5 KB).
//
// Sq <= SDPA_FEWQ_MAX (<= 16) runs the few-query kernels at the end of this file instead: one workgroup per (sequence, head), the
// [Sq][Sk] block in LDS, K and V read once each, explicit fmaf chains (exact f32 as well).
#include "attention_common.h"

namespace lstc_attn {
namespace {

constexpr int XNW = 4;                 // waves per workgroup
constexpr int XNT = 64 * XNW;
constexpr int XLD = 33;                // row pitch of the per-wave 32 x 32 transpose image (conflict-free both ways)
constexpr int XMAXS = 512;
constexpr int XMAXD = 512;

struct XOperand {                      // one of Q, K, V, O: base pointer is per use (O / dO, Q / dQ ... share strides)
    int64_t sn, sh, st;                // element strides over sequence, head, token
};

struct SdpaParams {
    const float *Q, *K, *V;
    float* O;
    float* probs;
    const float* dO;
    float *dQ, *dK, *dV;
    XOperand q, k, v, o;
    int N, H, Sq, Sk, dk, dv;
    float scale;
    DropKey dkey;
    int has_drop;
    int vec_qk, vec_v;                 // float4 operand loads allowed for the d_k / d_v contractions
    int vec_dk, vec_dv;                // few-query backward: float4 stores of dK / dV rows allowed
};

__device__ __forceinline__ floatx16 xmma8(const float* a, const float* b, floatx16 acc) {
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}

// row of accumulator register r for lane half h2
__device__ __forceinline__ int xrow(int r, int h2) { return (r & 3) + 8 * (r >> 2) + 4 * h2; }

__device__ __forceinline__ void xload16(const float* __restrict__ p, int k0, int kdim, bool vec, float (&f)[16]) {
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

// X[a][b] = sum_k A[a0 + a][k] * (B[b0 + b][k] * b_scale): b on the lane, a in the registers.  Rows past na - 1 / nb - 1 are
// clamped (the caller discards what they produce).
__device__ __forceinline__ floatx16 x_tile(const float* __restrict__ A, int64_t lda, int a0, int na, const float* __restrict__ B,
                                           int64_t ldb, int b0, int nb, int kdim, float b_scale, bool vec) {
    const int lane = threadIdx.x & 63, r = lane & 31, h2 = lane >> 5;
    const float* pa = A + (int64_t)min(a0 + r, na - 1) * lda;
    const float* pb = B + (int64_t)min(b0 + r, nb - 1) * ldb;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 1
    for (int kb = 0; kb < kdim; kb += 32) {
        float a[16], b[16];
        xload16(pa, kb + 16 * h2, kdim, vec, a);
        xload16(pb, kb + 16 * h2, kdim, vec, b);
#pragma unroll
        for (int s = 0; s < 16; ++s) b[s] *= b_scale;
        acc = xmma8(a, b, acc);
        acc = xmma8(a + 8, b + 8, acc);
    }
    return acc;
}

// acc[dt] += X^T B[rows t0.., g0 + 32 dt ..]: X (16 registers per lane, rows t0 + xrow(r)) is the A operand as it lies, the B
// operand is read as 128-B row segments of B (columns >= ncols read as zero, rows >= nrows clamped: X is zero there).
template <int DT>
__device__ __forceinline__ void x_acc(floatx16 (&acc)[DT], const float (&x)[16], const float* __restrict__ B, int64_t ldb, int t0,
                                      int nrows, int g0, int ncols) {
    const int lane = threadIdx.x & 63, c = lane & 31, h2 = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = g0 + 32 * dt + c;
        if (g0 + 32 * dt >= ncols) break;                 // wave-uniform
        const bool cv = col < ncols;
        float b[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) b[r] = cv ? B[(int64_t)min(t0 + xrow(r, h2), nrows - 1) * ldb + col] : 0.f;
        acc[dt] = xmma8(x, b, acc[dt]);
        acc[dt] = xmma8(x + 8, b + 8, acc[dt]);
    }
}

template <int DT>
__device__ __forceinline__ void x_store(const floatx16 (&acc)[DT], float* __restrict__ Out, int64_t ldo, int t0, int nrows, int g0,
                                        int ncols, float scale) {
    const int lane = threadIdx.x & 63, c = lane & 31, h2 = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = g0 + 32 * dt + c;
        if (col >= ncols) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = t0 + xrow(r, h2);
            if (row < nrows) Out[(int64_t)row * ldo + col] = acc[dt][r] * scale;
        }
    }
}

template <int DT>
__device__ __forceinline__ void x_zero(floatx16 (&acc)[DT]) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
}

template <int DT, bool MASKED>
__global__ void __launch_bounds__(XNT, DT == 8 ? 1 : 2) sdpa_fwd_kernel(const SdpaParams p, const MaskArg<MASKED> mk) {
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ float trs[XNW][32 * XLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h2 = lane >> 5;
    const int Sq = p.Sq, Sk = p.Sk, QT = (Sq + 31) >> 5, KT = (Sk + 31) >> 5;
    const uint32_t job = blockIdx.x * XNW + wave;
    if (job >= (uint32_t)p.N * (uint32_t)p.H * (uint32_t)QT) return;      // no block barrier in this kernel
    const int qt = (int)(job % (uint32_t)QT);
    const uint32_t nh = job / (uint32_t)QT;
    const int h = (int)(nh % (uint32_t)p.H), n = (int)(nh / (uint32_t)p.H);
    const float* Qb = p.Q + n * p.q.sn + h * p.q.sh;
    const float* Kb = p.K + n * p.k.sn + h * p.k.sh;
    const float* Vb = p.V + n * p.v.sn + h * p.v.sh;
    float* Ob = p.O + n * p.o.sn + h * p.o.sh;
    float* tr = trs[wave];
    const int q = 32 * qt + c;                        // this lane's query
    const uint8_t* mk_nh = nullptr;
    if constexpr (MASKED) mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;

    // logits of key block kt for this lane's query: register r = key 32 kt + xrow(r); keys >= Sk -> -inf
    auto logits = [&](int kt, floatx16& x) {
        x = x_tile(Kb, p.k.st, 32 * kt, Sk, Qb, p.q.st, 32 * qt, Sq, p.dk, p.scale, p.vec_qk);
        // Masked (both sweeps): the bytes are read in P's lane order (lane = key: one 32-byte run per query row), turned through the
        // wave's image to the logits' orientation (lane = query) and applied as a select.  A fully masked row keeps the running
        // max ATTN_MASK_FILL and comes out uniform; a masked key of a row that keeps a key adds exp(-1e9 - m) = 0 exactly.
        // sq == 0 (key padding): the byte depends on the key alone, the register index here - nothing goes through the image.
        if constexpr (MASKED) {
            if (mk.sq == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = 32 * kt + xrow(r, h2);
                    x[r] = (j >= Sk || mk_nh[(int64_t)j * mk.sk]) ? x[r] : ATTN_MASK_FILL;
                }
            } else {
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int i = 32 * qt + 2 * rr + h2, j = 32 * kt + c;
                    tr[(2 * rr + h2) * XLD + c] = (i < Sq && j < Sk) ? (float)mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk] : 1.f;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 16; ++r) x[r] = tr[c * XLD + xrow(r, h2)] != 0.f ? x[r] : ATTN_MASK_FILL;
                __builtin_amdgcn_wave_barrier();
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (32 * kt + xrow(r, h2) >= Sk) x[r] = -INFINITY;
    };

    // sweep 1: online row max / sum (the two lane halves hold the two halves of each key block; key 32 kt is always < Sk)
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

    float* pr_base = p.probs + ((size_t)n * p.H + h) * (size_t)Sq * Sk;
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)Sq * (uint32_t)Sk;
    // sweep 2 (once per group of up to 32 DT output columns): normalised P, its dropout, O += Pd V
#pragma unroll 1
    for (int g0 = 0; g0 < p.dv; g0 += 32 * DT) {
        floatx16 acc[DT];
        x_zero<DT>(acc);
#pragma unroll 1
        for (int kt = 0; kt < KT; ++kt) {
            floatx16 x;
            logits(kt, x);
            float pd[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * kt + xrow(r, h2);
                const float pv = j < Sk ? expf(x[r] - m) / l : 0.f;
                pd[r] = pv;
                if (g0 == 0) tr[c * XLD + xrow(r, h2)] = pv;
                if (p.has_drop) pd[r] = drop_keep(flat0 + (uint32_t)q * (uint32_t)Sk + (uint32_t)j, dkn) ? pv * dkn.scale : 0.f;
            }
            if (g0 == 0) {           // P rows out of the transpose image: two 128-B row segments per store
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int i = 32 * qt + 2 * rr + h2, j = 32 * kt + c;
                    const float v = tr[(2 * rr + h2) * XLD + c];
                    if (i < Sq && j < Sk) pr_base[(size_t)i * Sk + j] = v;
                }
                __builtin_amdgcn_wave_barrier();
            }
            x_acc<DT>(acc, pd, Vb, p.v.st, 32 * kt, Sk, g0, p.dv);
        }
        x_store<DT>(acc, Ob, p.o.st, 32 * qt, Sq, g0, p.dv, 1.f);
    }
}

template <int DT, bool MASKED>
__global__ void __launch_bounds__(XNT, 1) sdpa_bwd_kernel(const SdpaParams p, const MaskArg<MASKED> mk) {
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ float Dr[XMAXS];                           // rowsum(dP' * P) of this (sequence, head)
    __shared__ float trs[XNW][32 * XLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h2 = lane >> 5;
    float* tr = trs[wave];
    const int Sq = p.Sq, Sk = p.Sk, QT = (Sq + 31) >> 5, KT = (Sk + 31) >> 5;
    const int h = (int)(blockIdx.x % (uint32_t)p.H), n = (int)(blockIdx.x / (uint32_t)p.H);
    const float* Qb = p.Q + n * p.q.sn + h * p.q.sh;
    const float* Kb = p.K + n * p.k.sn + h * p.k.sh;
    const float* Vb = p.V + n * p.v.sn + h * p.v.sh;
    const float* dOb = p.dO + n * p.o.sn + h * p.o.sh;
    const float* Pb = p.probs + ((size_t)n * p.H + h) * (size_t)Sq * Sk;
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)Sq * (uint32_t)Sk;
    const uint8_t* mk_nh = nullptr;
    if constexpr (MASKED) mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
    // masked only.  bit r: the mask keeps (query of register r, this lane's key)
    auto keep_bits = [&](int qt, int kt) -> uint32_t {
        if constexpr (MASKED) {
            const int j = 32 * kt + c;
            if (mk.sq == 0)       // key padding: one byte per lane serves all sixteen queries
                return (j >= Sk || mk_nh[(int64_t)j * mk.sk]) ? 0xFFFFu : 0u;
            uint32_t km = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * qt + xrow(r, h2);
                const bool k1 = (i < Sq && j < Sk) ? mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk] != 0 : true;
                km |= (k1 ? 1u : 0u) << r;
            }
            return km;
        } else {
            return 0xFFFFu;
        }
    };
    auto drop_scale = [&](int i, int j) -> float {
        return drop_keep(flat0 + (uint32_t)i * (uint32_t)Sk + (uint32_t)j, dkn) ? dkn.scale : 0.f;
    };

    // dP' tile of (query block qt, key block kt) with P and the keep factor: queries in the registers, one key per lane
    auto dp_tile = [&](int qt, int kt, float (&pv)[16], float (&dpk)[16]) {
        const floatx16 x = x_tile(dOb, p.o.st, 32 * qt, Sq, Vb, p.v.st, 32 * kt, Sk, p.dv, 1.f, p.vec_v);
        const int j = 32 * kt + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * qt + xrow(r, h2);
            pv[r] = dpk[r] = 0.f;
            if (i < Sq && j < Sk) {
                pv[r] = Pb[(size_t)i * Sk + j];
                dpk[r] = x[r] * (p.has_drop ? drop_scale(i, j) : 1.f);
            }
        }
    };
    // dA = P (dP' - rowsum) of the tile, zero at masked positions (no gradient reaches q.k there), same layout
    auto da_tile = [&](int qt, int kt, float (&da)[16]) {
        float pv[16], dpk[16];
        dp_tile(qt, kt, pv, dpk);
#pragma unroll
        for (int r = 0; r < 16; ++r) da[r] = pv[r] * (dpk[r] - Dr[min(32 * qt + xrow(r, h2), XMAXS - 1)]);
        if constexpr (MASKED) {
            const uint32_t km = keep_bits(qt, kt);
#pragma unroll
            for (int r = 0; r < 16; ++r) da[r] = ((km >> r) & 1u) ? da[r] : 0.f;
        }
    };

    // (R) rowsum over the keys: per-lane partials over all key blocks, then one reduction across the 32 lanes of each half
#pragma unroll 1
    for (int qt = wave; qt < QT; qt += XNW) {
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
            if (c == 0) Dr[32 * qt + xrow(r, h2)] = v;       // < 32 QT <= 512
        }
    }
    __syncthreads();

    // (V) dV = Pd^T dO and (K) dK = dA^T Q scale: key blocks over the waves, query blocks inner
#pragma unroll 1
    for (int kt = wave; kt < KT; kt += XNW) {
        const int j = 32 * kt + c;
#pragma unroll 1
        for (int g0 = 0; g0 < p.dv; g0 += 32 * DT) {
            floatx16 acc[DT];
            x_zero<DT>(acc);
#pragma unroll 1
            for (int qt = 0; qt < QT; ++qt) {
                float pd[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = 32 * qt + xrow(r, h2);
                    float v = 0.f;
                    if (i < Sq && j < Sk) {
                        v = Pb[(size_t)i * Sk + j];
                        if (p.has_drop) v *= drop_scale(i, j);
                    }
                    pd[r] = v;
                }
                x_acc<DT>(acc, pd, dOb, p.o.st, 32 * qt, Sq, g0, p.dv);
            }
            x_store<DT>(acc, p.dV + n * p.v.sn + h * p.v.sh, p.v.st, 32 * kt, Sk, g0, p.dv, 1.f);
        }
#pragma unroll 1
        for (int g0 = 0; g0 < p.dk; g0 += 32 * DT) {
            floatx16 acc[DT];
            x_zero<DT>(acc);
#pragma unroll 1
            for (int qt = 0; qt < QT; ++qt) {
                float da[16];
                da_tile(qt, kt, da);
                x_acc<DT>(acc, da, Qb, p.q.st, 32 * qt, Sq, g0, p.dk);
            }
            x_store<DT>(acc, p.dK + n * p.k.sn + h * p.k.sh, p.k.st, 32 * kt, Sk, g0, p.dk, p.scale);
        }
    }

    // (Q) dQ = dA K scale: query blocks over the waves, key blocks inner; dA goes through the image (keys onto the registers)
#pragma unroll 1
    for (int qt = wave; qt < QT; qt += XNW) {
#pragma unroll 1
        for (int g0 = 0; g0 < p.dk; g0 += 32 * DT) {
            floatx16 acc[DT];
            x_zero<DT>(acc);
#pragma unroll 1
            for (int kt = 0; kt < KT; ++kt) {
                float da[16];
                da_tile(qt, kt, da);
#pragma unroll
                for (int r = 0; r < 16; ++r) tr[xrow(r, h2) * XLD + c] = da[r];
                __builtin_amdgcn_wave_barrier();
                float dat[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) dat[r] = tr[c * XLD + xrow(r, h2)];
                __builtin_amdgcn_wave_barrier();
                x_acc<DT>(acc, dat, Kb, p.k.st, 32 * kt, Sk, g0, p.dk);
            }
            x_store<DT>(acc, p.dQ + n * p.q.sn + h * p.q.sh, p.q.st, 32 * qt, Sq, g0, p.dk, p.scale);
        }
    }
}

// 32-column output tiles per group: enough for max(d_k, d_v) up to 256 in one group
int sdpa_dt(int dk, int dv) {
    const int t = ((dk > dv ? dk : dv) + 31) / 32;
    return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : 8;
}

bool stride4(const XOperand& s) { return s.sn % 4 == 0 && s.sh % 4 == 0 && s.st % 4 == 0; }

// Every check of lstc_sdpa_fwd / lstc_sdpa_bwd, before any launch; fills p and mk (when m is given)
int sdpa_fill(const LstcSdpaDesc* d, const LstcAttnMask* m, bool bwd, SdpaParams& p, MaskParams& mk) {
    if (!d) return LSTC_E_NULL;
    if (!d->Q || !d->K || !d->V || !d->probs) return LSTC_E_NULL;
    if (bwd ? (!d->dO || !d->dQ || !d->dK || !d->dV) : !d->O) return LSTC_E_NULL;
    if (m && !m->mask) return LSTC_E_NULL;
    if (d->N <= 0 || d->H <= 0 || d->Sq <= 0 || d->Sk <= 0 || d->dk <= 0 || d->dv <= 0) return LSTC_E_SHAPE;
    const int64_t st[12] = {d->q_sn, d->q_sh, d->q_st, d->k_sn, d->k_sh, d->k_st, d->v_sn, d->v_sh, d->v_st, d->o_sn, d->o_sh, d->o_st};
    for (int i = 0; i < 12; ++i)
        if (st[i] < 0) return LSTC_E_SHAPE;
    if (m && (m->sn < 0 || m->sh < 0 || m->sq < 0 || m->sk < 0)) return LSTC_E_SHAPE;
    if (bwd) {      // dQ, dK, dV are written through the strides of Q, K, V: a broadcast axis would give one element several writers
        const int64_t len[3] = {d->N, d->H, 0};
        for (int i = 0; i < 9; ++i)
            if (st[i] == 0 && (i % 3 == 2 ? (i < 3 ? d->Sq : d->Sk) : len[i % 3]) > 1) return LSTC_E_SHAPE;
    }
    if (!(d->dropout_p >= 0.f && d->dropout_p <= 1.f)) return LSTC_E_SHAPE;
    if (d->Sq > XMAXS || d->Sk > XMAXS || d->dk > XMAXD || d->dv > XMAXD || d->dk % 16 || d->dv % 16) return LSTC_E_RANGE;
    if ((int64_t)d->N * d->H > 0x7fffffffLL) return LSTC_E_RANGE;
    if ((uint64_t)d->N * (uint64_t)d->H * (uint64_t)d->Sq * (uint64_t)d->Sk > 0xffffffffull) return LSTC_E_RANGE;   // 32-bit dropout counter
    p.Q = (const float*)d->Q; p.K = (const float*)d->K; p.V = (const float*)d->V;
    p.O = (float*)d->O; p.probs = d->probs;
    p.dO = (const float*)d->dO; p.dQ = (float*)d->dQ; p.dK = (float*)d->dK; p.dV = (float*)d->dV;
    p.q = {d->q_sn, d->q_sh, d->q_st}; p.k = {d->k_sn, d->k_sh, d->k_st};
    p.v = {d->v_sn, d->v_sh, d->v_st}; p.o = {d->o_sn, d->o_sh, d->o_st};
    p.N = d->N; p.H = d->H; p.Sq = d->Sq; p.Sk = d->Sk; p.dk = d->dk; p.dv = d->dv;
    p.scale = d->scale;
    p.has_drop = d->dropout_p > 0.f;
    p.dkey = make_drop_key(d->dropout_p, d->dropout_seed);
    // float4 loads: Q and K rows in the forward (over d_k), dO and V rows in the backward's dP' (over d_v)
    p.vec_qk = aligned16(d->Q) && aligned16(d->K) && stride4(p.q) && stride4(p.k);
    p.vec_v = aligned16(d->V) && (!bwd || aligned16(d->dO)) && stride4(p.v) && stride4(p.o);
    p.vec_dk = bwd && aligned16(d->dK) && stride4(p.k);
    p.vec_dv = bwd && aligned16(d->dV) && stride4(p.v);
    if (m) { mk.m = m->mask; mk.sn = m->sn; mk.sh = m->sh; mk.sq = m->sq; mk.sk = m->sk; }
    return 0;
}

template <template <int, bool> class Launch>
void sdpa_dispatch(int dt, const SdpaParams& p, const MaskParams* mk, dim3 grid, hipStream_t st) {
    auto go = [&](auto masked, const auto& mask_arg) {
        constexpr bool M = decltype(masked)::value;
        switch (dt) {
            case 1: Launch<1, M>::run(grid, st, p, mask_arg); break;
            case 2: Launch<2, M>::run(grid, st, p, mask_arg); break;
            case 4: Launch<4, M>::run(grid, st, p, mask_arg); break;
            default: Launch<8, M>::run(grid, st, p, mask_arg); break;
        }
    };
    if (mk) go(std::true_type{}, *mk); else go(std::false_type{}, NoMask{});
}

template <int DT, bool M>
struct FwdLaunch {
    static void run(dim3 grid, hipStream_t st, const SdpaParams& p, const MaskArg<M>& mk) {
        hipLaunchKernelGGL((sdpa_fwd_kernel<DT, M>), grid, XNT, 0, st, p, mk);
    }
};
template <int DT, bool M>
struct BwdLaunch {
    static void run(dim3 grid, hipStream_t st, const SdpaParams& p, const MaskArg<M>& mk) {
        hipLaunchKernelGGL((sdpa_bwd_kernel<DT, M>), grid, XNT, 0, st, p, mk);
    }
};

// ------------------------------------------------------------------------------------------------ few-query kernels
// 1 <= Sq <= SDPA_FEWQ_MAX (<= 16): a 32-row query tile would be mostly padding, so these run one workgroup of four waves per
// (sequence, head) with the whole [Sq][Sk] block of logits (forward) or of Pd / dP' / dA (backward) in LDS as f32, and read K
// and V from HBM once each.  QB = Sq rounded up to a power of two is the number of query rows held in registers, DB = 256 or 512
// the row pitch of the small LDS operand (Q scale in the forward, dO in the backward).  Three building blocks:
//   f_rowdot  X[i][j] = A_lds[i] . B[j]     keys over groups of four lanes (each lane every fourth float4 of the row), queries
//                                           in registers; the four partial sums are added by two lane exchanges
//   f_xt_rows out[j] = sum_i X[i][j] g[i]   keys over the waves, float4 columns over the lanes (g in registers): dV, dK
//   f_x_rows  out[i] = sum_j X[i][j] B[j]   keys j = wave (mod 4), float4 columns over the lanes; the four waves' partial rows
//                                           are added in wave order through LDS: O, dQ
// Every product is an explicit fmaf in a fixed order that depends on neither alignment nor on whether float4 accesses were
// taken; one writer per element, no atomics.  Static LDS: (max(QB DB, 1024 max(QB / 4, 1)) + 512 QB) * 4 bytes - the first term is the
// staged operand or the four waves' partial rows, whichever is larger: 6 KB at QB = 1, 8 KB at QB = 2, 48 KB at QB = 16, DB = 256,
// 64 KB at QB = 16, DB = 512.
#ifndef SDPA_FEWQ_MAX
#define SDPA_FEWQ_MAX 16               // largest Sq the few-query kernels take; 0 compiles the dispatch out
#endif
static_assert(SDPA_FEWQ_MAX >= 0 && SDPA_FEWQ_MAX <= 16, "the few-query kernels hold at most 16 query rows");
#if SDPA_FEWQ_MAX > 0

constexpr int FCOLS = 256;             // output columns per pass of f_xt_rows / f_x_rows: one float4 per lane

__device__ __forceinline__ float4 f_ld4(const float* __restrict__ p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void f_st4(float* __restrict__ p, const float4 v, bool vec) {
    if (vec) { *reinterpret_cast<float4*>(p) = v; return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
__device__ __forceinline__ void f_fma4(float4& acc, float s, const float4 v) {
    acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}

template <int QB, int DB>
constexpr int f_ar_floats() {
    constexpr int rb = QB >= 4 ? QB / 4 : 1;
    return QB * DB > XNW * rb * FCOLS ? QB * DB : XNW * rb * FCOLS;
}

// ar[i][c] = src[i][c] * s for i < nrows, c < kdim; zero rows up to QB
template <int QB, int DB>
__device__ __forceinline__ void f_stage(float* ar, const float* __restrict__ src, int64_t ld, int nrows, int kdim, float s) {
    for (int idx = threadIdx.x; idx < QB * DB; idx += XNT) {
        const int i = idx / DB, c = idx % DB;
        ar[idx] = (i < nrows && c < kdim) ? src[(int64_t)i * ld + c] * s : 0.f;
    }
}

template <int QB, int DB>
__device__ __forceinline__ void f_rowdot(const float* ar, const float* __restrict__ B, int64_t ldb, int nb, int kdim, bool vec,
                                         float (*X)[XMAXS]) {
    const int slice = threadIdx.x & 3;
#pragma unroll 1
    for (int j0 = 0; j0 < nb; j0 += XNT / 4) {
        const int j = j0 + (int)(threadIdx.x >> 2);
        const float* pb = B + (int64_t)min(j, nb - 1) * ldb;
        float acc[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) acc[i] = 0.f;
#pragma unroll 4
        for (int c = 4 * slice; c < kdim; c += 16) {
            const float4 b = f_ld4(pb + c, vec);
#pragma unroll
            for (int i = 0; i < QB; ++i) {
                const float4 a = *reinterpret_cast<const float4*>(ar + i * DB + c);
                acc[i] = fmaf(a.x, b.x, acc[i]); acc[i] = fmaf(a.y, b.y, acc[i]);
                acc[i] = fmaf(a.z, b.z, acc[i]); acc[i] = fmaf(a.w, b.w, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < QB; ++i) {
            float v = acc[i];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            if (slice == 0 && j < nb) X[i][j] = v;
        }
    }
}

// G(i, col, active) -> the float4 of row i at columns col .. col + 3 (zero for i >= Sq or an inactive lane)
template <int QB, typename G>
__device__ __forceinline__ void f_xt_rows(const float (*X)[XMAXS], G g_of, float* __restrict__ Out, int64_t ldo, int nk, int ncols,
                                          float s, bool vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int c0 = 0; c0 < ncols; c0 += FCOLS) {
        const int col = c0 + 4 * lane;
        const bool active = col < ncols;                  // widths are multiples of 16: col < ncols covers col + 3
        float4 g[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) g[i] = g_of(i, col, active);
#pragma unroll 2
        for (int j = wave; j < nk; j += XNW) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < QB; ++i) f_fma4(acc, X[i][j], g[i]);
            acc.x *= s; acc.y *= s; acc.z *= s; acc.w *= s;
            if (active) f_st4(Out + (int64_t)j * ldo + col, acc, vec);
        }
    }
}

template <int QB>
__device__ __forceinline__ void f_x_rows(const float (*X)[XMAXS], float* ar, const float* __restrict__ B, int64_t ldb, int nk,
                                         int ncols, bool vec, float* __restrict__ Out, int64_t ldo, int nrows, float s) {
    constexpr int RB = QB >= 4 ? QB / 4 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int c0 = 0; c0 < ncols; c0 += FCOLS) {
        const int col = c0 + 4 * lane;
        const bool active = col < ncols;
        float4 acc[QB];
#pragma unroll
        for (int i = 0; i < QB; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int j = wave; j < nk; j += XNW) {
            const float4 b = active ? f_ld4(B + (int64_t)j * ldb + col, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < QB; ++i) f_fma4(acc[i], X[i][j], b);
        }
#pragma unroll
        for (int pass = 0; pass < QB / RB; ++pass) {
            __syncthreads();                              // ar is free: its last readers are behind a barrier
#pragma unroll
            for (int r = 0; r < RB; ++r) *reinterpret_cast<float4*>(ar + (wave * RB + r) * FCOLS + 4 * lane) = acc[pass * RB + r];
            __syncthreads();
            for (int idx = threadIdx.x; idx < RB * FCOLS; idx += XNT) {
                const int r = idx / FCOLS, c = idx % FCOLS, i = pass * RB + r;
                const float v = ((ar[r * FCOLS + c] + ar[(RB + r) * FCOLS + c]) + ar[(2 * RB + r) * FCOLS + c]) + ar[(3 * RB + r) * FCOLS + c];
                if (i < nrows && c0 + c < ncols) Out[(int64_t)i * ldo + c0 + c] = v * s;
            }
        }
    }
}

template <int QB, int DB, bool MASKED>
__global__ void __launch_bounds__(XNT) sdpa_fewq_fwd_kernel(const SdpaParams p, const MaskArg<MASKED> mk) {
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ __attribute__((aligned(16))) float ar[f_ar_floats<QB, DB>()];   // Q scale, then the waves' partial O rows
    __shared__ float X[QB][XMAXS];                                             // logits, then Pd
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Sq = p.Sq, Sk = p.Sk;
    const int h = (int)(blockIdx.x % (uint32_t)p.H), n = (int)(blockIdx.x / (uint32_t)p.H);
    const float* Kb = p.K + n * p.k.sn + h * p.k.sh;
    const float* Vb = p.V + n * p.v.sn + h * p.v.sh;
    float* pr_base = p.probs + ((size_t)n * p.H + h) * (size_t)Sq * Sk;
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)Sq * (uint32_t)Sk;
    const uint8_t* mk_nh = nullptr;
    if constexpr (MASKED) mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;

    f_stage<QB, DB>(ar, p.Q + n * p.q.sn + h * p.q.sh, p.q.st, Sq, p.dk, p.scale);
    __syncthreads();
    f_rowdot<QB, DB>(ar, Kb, p.k.st, Sk, p.dk, p.vec_qk, X);
    __syncthreads();

    // softmax of row i by wave i mod 4: lane partial sums over j = lane + 64 t in t order, then the butterfly.  A fully masked
    // row has every logit ATTN_MASK_FILL and comes out uniform; a masked key of a row that keeps a key adds exp(-1e9 - m) = 0.
#pragma unroll 1
    for (int i = wave; i < QB; i += XNW) {
        if (i >= Sq) {                                    // padding rows take no part in O
            for (int j = lane; j < Sk; j += 64) X[i][j] = 0.f;
            continue;
        }
        float x[XMAXS / 64];
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < XMAXS / 64; ++t) {
            const int j = lane + 64 * t;
            float v = -INFINITY;
            if (j < Sk) {
                v = X[i][j];
                if constexpr (MASKED) v = mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk] ? v : ATTN_MASK_FILL;
            }
            x[t] = v;
            m = fmaxf(m, v);
        }
        m = wave_max(m);
        float l = 0.f;
#pragma unroll
        for (int t = 0; t < XMAXS / 64; ++t) {
            x[t] = lane + 64 * t < Sk ? expf(x[t] - m) : 0.f;
            l += x[t];
        }
        l = wave_sum(l);
#pragma unroll
        for (int t = 0; t < XMAXS / 64; ++t) {
            const int j = lane + 64 * t;
            if (j < Sk) {
                const float pv = x[t] / l;
                pr_base[(size_t)i * Sk + j] = pv;
                float pd = pv;
                if (p.has_drop) pd = drop_keep(flat0 + (uint32_t)i * (uint32_t)Sk + (uint32_t)j, dkn) ? pv * dkn.scale : 0.f;
                X[i][j] = pd;
            }
        }
    }
    __syncthreads();
    f_x_rows<QB>(X, ar, Vb, p.v.st, Sk, p.dv, p.vec_v, p.O + n * p.o.sn + h * p.o.sh, p.o.st, Sq, 1.f);
}

template <int QB, int DB, bool MASKED>
__global__ void __launch_bounds__(XNT) sdpa_fewq_bwd_kernel(const SdpaParams p, const MaskArg<MASKED> mk) {
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ __attribute__((aligned(16))) float ar[f_ar_floats<QB, DB>()];   // dO, then the waves' partial dQ rows
    __shared__ float X[QB][XMAXS];                                             // Pd, then dP', then dA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Sq = p.Sq, Sk = p.Sk;
    const int h = (int)(blockIdx.x % (uint32_t)p.H), n = (int)(blockIdx.x / (uint32_t)p.H);
    const float* Qb = p.Q + n * p.q.sn + h * p.q.sh;
    const float* Kb = p.K + n * p.k.sn + h * p.k.sh;
    const float* Vb = p.V + n * p.v.sn + h * p.v.sh;
    const float* Pb = p.probs + ((size_t)n * p.H + h) * (size_t)Sq * Sk;
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)Sq * (uint32_t)Sk;
    const uint8_t* mk_nh = nullptr;
    if constexpr (MASKED) mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
    auto keep_scale = [&](int i, int j) -> float {
        if (!p.has_drop) return 1.f;
        return drop_keep(flat0 + (uint32_t)i * (uint32_t)Sk + (uint32_t)j, dkn) ? dkn.scale : 0.f;
    };

    // X = Pd (zero rows past Sq); dO into LDS
    f_stage<QB, DB>(ar, p.dO + n * p.o.sn + h * p.o.sh, p.o.st, Sq, p.dv, 1.f);
#pragma unroll 1
    for (int i = wave; i < QB; i += XNW)
        for (int j = lane; j < Sk; j += 64) X[i][j] = i < Sq ? Pb[(size_t)i * Sk + j] * keep_scale(i, j) : 0.f;
    __syncthreads();
    // dV = Pd^T dO
    f_xt_rows<QB>(X, [&](int i, int col, bool active) {
        return active ? *reinterpret_cast<const float4*>(ar + i * DB + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }, p.dV + n * p.v.sn + h * p.v.sh, p.v.st, Sk, p.dv, 1.f, p.vec_dv);
    __syncthreads();
    // X = dP' = dO V^T
    f_rowdot<QB, DB>(ar, Vb, p.v.st, Sk, p.dv, p.vec_v, X);
    __syncthreads();
    // X = dA = P (dP' keep - rowsum(dP' keep P)), zero at masked positions and in the padding rows
#pragma unroll 1
    for (int i = wave; i < QB; i += XNW) {
        if (i >= Sq) {
            for (int j = lane; j < Sk; j += 64) X[i][j] = 0.f;
            continue;
        }
        float pv[XMAXS / 64], dpk[XMAXS / 64];
        float part = 0.f;
#pragma unroll
        for (int t = 0; t < XMAXS / 64; ++t) {
            const int j = lane + 64 * t;
            pv[t] = dpk[t] = 0.f;
            if (j < Sk) {
                pv[t] = Pb[(size_t)i * Sk + j];
                dpk[t] = X[i][j] * keep_scale(i, j);
            }
            part += dpk[t] * pv[t];
        }
        const float rs = wave_sum(part);
#pragma unroll
        for (int t = 0; t < XMAXS / 64; ++t) {
            const int j = lane + 64 * t;
            if (j < Sk) {
                float da = pv[t] * (dpk[t] - rs);
                if constexpr (MASKED) da = mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk] ? da : 0.f;
                X[i][j] = da;
            }
        }
    }
    __syncthreads();
    // dK = dA^T Q scale
    f_xt_rows<QB>(X, [&](int i, int col, bool active) {
        return (active && i < Sq) ? f_ld4(Qb + (int64_t)i * p.q.st + col, p.vec_qk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }, p.dK + n * p.k.sn + h * p.k.sh, p.k.st, Sk, p.dk, p.scale, p.vec_dk);
    // dQ = dA K scale
    f_x_rows<QB>(X, ar, Kb, p.k.st, Sk, p.dk, p.vec_qk, p.dQ + n * p.q.sn + h * p.q.sh, p.q.st, Sq, p.scale);
}

template <bool BWD, int QB, int DB, bool M>
void fewq_launch(const SdpaParams& p, const MaskArg<M>& mk, hipStream_t st) {
    const dim3 grid((unsigned)(p.N * p.H));
    if constexpr (BWD) hipLaunchKernelGGL((sdpa_fewq_bwd_kernel<QB, DB, M>), grid, XNT, 0, st, p, mk);
    else hipLaunchKernelGGL((sdpa_fewq_fwd_kernel<QB, DB, M>), grid, XNT, 0, st, p, mk);
}
template <bool BWD, int QB, bool M>
void fewq_width(const SdpaParams& p, const MaskArg<M>& mk, hipStream_t st) {
    if ((BWD ? p.dv : p.dk) <= 256) fewq_launch<BWD, QB, 256, M>(p, mk, st);
    else fewq_launch<BWD, QB, 512, M>(p, mk, st);
}
template <bool BWD, bool M>
void fewq_rows(const SdpaParams& p, const MaskArg<M>& mk, hipStream_t st) {
    if (p.Sq <= 1) fewq_width<BWD, 1, M>(p, mk, st);
    else if (p.Sq <= 2) fewq_width<BWD, 2, M>(p, mk, st);
    else if (p.Sq <= 4) fewq_width<BWD, 4, M>(p, mk, st);
    else if (p.Sq <= 8) fewq_width<BWD, 8, M>(p, mk, st);
    else fewq_width<BWD, 16, M>(p, mk, st);
}
// true: Sq <= SDPA_FEWQ_MAX and the few-query kernel was launched
template <bool BWD>
bool fewq_run(const SdpaParams& p, const MaskParams* mk, hipStream_t st) {
    if (p.Sq > SDPA_FEWQ_MAX) return false;
    if (mk) fewq_rows<BWD, true>(p, *mk, st); else fewq_rows<BWD, false>(p, NoMask{}, st);
    return true;
}
#else       // compiled out: neither the kernels nor their dispatch exist in this build
template <bool BWD>
bool fewq_run(const SdpaParams&, const MaskParams*, hipStream_t) { return false; }
#endif

}  // namespace
}  // namespace lstc_attn

extern "C" {

int lstc_sdpa_fwd(const LstcSdpaDesc* d, const LstcAttnMask* m, void* stream) {
    using namespace lstc_attn;
    SdpaParams p;
    MaskParams mk;
    const int rc = sdpa_fill(d, m, false, p, mk);
    if (rc) return rc;
    if (fewq_run<false>(p, m ? &mk : nullptr, (hipStream_t)stream)) return lstc_launch_status();
    const uint64_t waves = (uint64_t)p.N * p.H * ((p.Sq + 31) / 32);
    sdpa_dispatch<FwdLaunch>(sdpa_dt(p.dk, p.dv), p, m ? &mk : nullptr, dim3((unsigned)((waves + XNW - 1) / XNW)), (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_sdpa_bwd(const LstcSdpaDesc* d, const LstcAttnMask* m, void* stream) {
    using namespace lstc_attn;
    SdpaParams p;
    MaskParams mk;
    const int rc = sdpa_fill(d, m, true, p, mk);
    if (rc) return rc;
    if (fewq_run<true>(p, m ? &mk : nullptr, (hipStream_t)stream)) return lstc_launch_status();
    sdpa_dispatch<BwdLaunch>(sdpa_dt(p.dk, p.dv), p, m ? &mk : nullptr, dim3((unsigned)(p.N * p.H)), (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_sdpa_few_query_max(void) { return SDPA_FEWQ_MAX; }

}  // extern "C"
