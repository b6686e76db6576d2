// Key-tiled attention kernels (128 < S <= 512), forward and backward: the kernel text.
// Included twice by csrc/attention_long.hip: once with ATTN_MASKED 0 under the kernels' own names - the text the compiler sees is then exactly what
// it was before attention masks existed, so the unmasked kernels come out instruction for instruction as they were (checked by
// tools/attn_isa_diff.py) - and once with ATTN_MASKED 1 as attn_long_fwd_masked_kernel / attn_long_bwd_masked_kernel, which take the mask as a second kernel argument.
// No include guard on purpose.
template <bool BF, int DT>
__global__ void __launch_bounds__(LNT, DT == 8 ? 1 : 2) ATTN_LONG_FWD(const AttnParams p ATTN_MASK_PARAM) {
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ float trs[LNW][32 * TLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h2 = lane >> 5;
    const int S = p.S, QT = (S + 31) >> 5, KT = QT;
    const uint32_t job = blockIdx.x * LNW + wave;
    if (job >= (uint32_t)p.N * (uint32_t)p.H * (uint32_t)QT) return;      // no block barrier in this kernel
    const int qt = (int)(job % (uint32_t)QT);
    const uint32_t nh = job / (uint32_t)QT;
    const int h = (int)(nh % (uint32_t)p.H), n = (int)(nh / (uint32_t)p.H);
    const float* Qb = p.Q + (size_t)n * S * p.ldq + (size_t)h * p.dk;
    const float* Kb = p.K + (size_t)n * S * p.ldk + (size_t)h * p.dk;
    const float* Vb = p.V + (size_t)n * S * p.ldv + (size_t)h * p.dv;
    float* Ob = p.O + (size_t)n * S * p.ldo + (size_t)h * p.dv;
    float* tr = trs[wave];
    const int q = 32 * qt + c;                        // this lane's query
    const bool bias = p.index_ld > 0 && q >= 1 && q < S;
    const int64_t* irow = p.index + (size_t)(bias ? q - 1 : 0) * p.index_ld;
    const float* tabh = p.table + h;
#if ATTN_MASKED
    const uint8_t* const mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
#endif

    // logits of key block kt for this lane's query: register r = key 32 kt + frow(r); keys >= S -> -inf
    auto logits = [&](int kt, floatx16& x) {
        x = tile_xt<BF>(Kb, p.ldk, 32 * kt, Qb, p.ldq, 32 * qt, S, p.dk, p.scale, p.vec_qk);
#if ATTN_MASKED
        // Masked (both sweeps): the bytes of the tile are read in the lane order in which P is written (lane = key: one 32-byte run
        // per query row, two rows per load), turned through the wave's transpose image to the logits' orientation (lane = query) and
        // applied as a predicated select before the bias.  A fully masked row has the running max ATTN_MASK_FILL and comes out uniform;
        // a fully masked key block of a row that keeps a key adds exp(-1e9 - m) = 0 exactly; only the padding keys >= S are -inf.
        // sq == 0 (a key-padding mask): the byte depends on the key alone, which is the register index here - the 32 lanes of a half
        // read one and the same byte per load, and nothing goes through the image.
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
#endif
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

    float* pr_base = p.probs + ((size_t)n * p.H + h) * S * S;
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
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

template <bool BF, int DT>
__global__ void __launch_bounds__(LNT, 1) ATTN_LONG_BWD(const AttnParams p ATTN_MASK_PARAM) {
    const DropKey dkn = drop_key_now(p.dkey);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h2 = lane >> 5;
    float* Dr = sm;                                       // [LMAXS] rowsum(dP' * P) of the current sequence
    float* tr = sm + LMAXS + wave * 32 * TLD;             // this wave's transpose image
    float* tacc = sm + LMAXS + LNW * 32 * TLD;            // [LNW][table_rows] bias-table gradient, one copy per wave
    const int h = (int)blockIdx.y, S = p.S, QT = (S + 31) >> 5, KT = QT;
    const bool has_bias = p.index_ld > 0 && p.dtable != nullptr;
    if (has_bias)
        for (int i = threadIdx.x; i < LNW * p.table_rows; i += LNT) tacc[i] = 0.f;
    float* const tw = tacc + wave * p.table_rows;
    const int n_begin = (int)blockIdx.x * p.n_per_wg;
    const int n_end = min(p.N, n_begin + p.n_per_wg);
#pragma unroll 1
    for (int n = n_begin; n < n_end; ++n) {
        const float* Qb = p.Q + (size_t)n * S * p.ldq + (size_t)h * p.dk;
        const float* Kb = p.K + (size_t)n * S * p.ldk + (size_t)h * p.dk;
        const float* Vb = p.V + (size_t)n * S * p.ldv + (size_t)h * p.dv;
        const float* dOb = p.dO + (size_t)n * S * p.ldo + (size_t)h * p.dv;
        const float* Pb = p.probs + ((size_t)n * p.H + h) * S * S;
        const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
#if ATTN_MASKED
        const uint8_t* const mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
        // bit r: the mask keeps (query of register r, this lane's key) - read with P's lane order, one 32-byte run per query row
        auto keep_bits = [&](int qt, int kt) {
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
        };
#endif

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
                store_acc<DT>(acc, p.dV + (size_t)n * S * p.ldv + (size_t)h * p.dv, p.ldv, 32 * kt, S, g0, p.dv, 1.f);
            }
#pragma unroll 1
            for (int g0 = 0; g0 < p.dk; g0 += 32 * DT) {
                floatx16 acc[DT];
                zero_acc<DT>(acc);
#pragma unroll 1
                for (int qt = 0; qt < QT; ++qt) {
                    float da[16];
                    da_tile(qt, kt, da);
#if ATTN_MASKED     // no gradient reaches q.k at a masked position
                    {
                        const uint32_t km = keep_bits(qt, kt);
#pragma unroll
                        for (int r = 0; r < 16; ++r) da[r] = ((km >> r) & 1u) ? da[r] : 0.f;
                    }
#endif
                    acc_xtb<BF, DT>(acc, da, Qb, p.ldq, 32 * qt, S, g0, p.dk);
                }
                store_acc<DT>(acc, p.dK + (size_t)n * S * p.ldk + (size_t)h * p.dk, p.ldk, 32 * kt, S, g0, p.dk, p.scale);
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
#if ATTN_MASKED     // the bias table above took dA as it is (the bias is added after the fill); dQ takes it zeroed at masked positions
                    {
                        const uint32_t km = keep_bits(qt, kt);
#pragma unroll
                        for (int r = 0; r < 16; ++r) da[r] = ((km >> r) & 1u) ? da[r] : 0.f;
                    }
#endif
#pragma unroll
                    for (int r = 0; r < 16; ++r) tr[frow(r, h2) * TLD + c] = da[r];
                    __builtin_amdgcn_wave_barrier();
                    float dat[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) dat[r] = tr[c * TLD + frow(r, h2)];
                    __builtin_amdgcn_wave_barrier();
                    acc_xtb<BF, DT>(acc, dat, Kb, p.ldk, 32 * kt, S, g0, p.dk);
                }
                store_acc<DT>(acc, p.dQ + (size_t)n * S * p.ldq + (size_t)h * p.dk, p.ldq, 32 * qt, S, g0, p.dk, p.scale);
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
