// First-generation attention kernels (S <= 128), forward and backward: the kernel text.
// Included twice by csrc/attention.hip: once with ATTN_MASKED 0 under the kernels' own names - the text the compiler sees is then exactly what
// it was before attention masks existed, so the unmasked kernels come out instruction for instruction as they were (checked by
// tools/attn_isa_diff.py) - and once with ATTN_MASKED 1 as attn_fwd_masked_kernel / attn_bwd_masked_kernel, which take the mask as a second kernel argument.
// No include guard on purpose.
// Masked: where the mask byte of (n, h, i, j) is 0 the scaled logit is replaced by ATTN_MASK_FILL before the bias is added; in the
// backward the saved P carries the mask already, so dV and the row sums do not change.
template <int T>
__global__ void __launch_bounds__(NT, T <= 2 ? 4 : 2) ATTN1_FWD(const AttnParams p ATTN_MASK_PARAM) {
    const DropKey dkn = drop_key_now(p.dkey);
    constexpr bool BF = false;       // first generation: exact-f32 products only (bf16 products made these latency-bound loops slower)
    constexpr int SP = 32 * T, LD = SP + 1, NJ = (SP + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = ATTN_CHUNK, h = ATTN_HEAD, S = p.S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* Qb = p.Q + (size_t)n * S * p.ldq + (size_t)h * p.dk;
    const float* Kb = p.K + (size_t)n * S * p.ldk + (size_t)h * p.dk;
    const float* Vb = p.V + (size_t)n * S * p.ldv + (size_t)h * p.dv;
    float* Ob = p.O + (size_t)n * S * p.ldo + (size_t)h * p.dv;

#pragma unroll 1
    for (int t = wave; t < T * T; t += NT / 64) {
        const int ti = t / T, tj = t % T;
        if (32 * ti >= S || 32 * tj >= S) continue;   // fully padded tile: rows/cols are rewritten below
        const floatx16 acc = tile_abt<BF>(Qb, p.ldq, 32 * ti, Kb, p.ldk, 32 * tj, S, p.dk, p.scale, p.vec_qk);
        store_tile_lds<LD>(sm, ti, tj, acc);
    }
    __syncthreads();

    float* pr_base = p.probs + ((size_t)n * p.H + h) * S * S;
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
#if ATTN_MASKED
    const uint8_t* const mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
    // sq == 0 (a key-padding mask): every query row reads the same S bytes - once per (sequence, head), ahead of the row loop,
    // instead of one more exposed load per row of these latency-bound loops
    const bool mk_rows_alike = mk.sq == 0;
    uint8_t mk0[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) mk0[jj] = (mk_rows_alike && lane + 64 * jj < S) ? mk_nh[(int64_t)(lane + 64 * jj) * mk.sk] : (uint8_t)1;
#endif
#pragma unroll 1
    for (int i = wave; i < SP; i += NT / 64) {
        float* row = sm + i * LD;
        if (i >= S) {
            for (int j = lane; j < SP; j += 64) row[j] = 0.f;
            continue;
        }
        float v[NJ];
        float m = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = lane + 64 * jj;
            float x = -INFINITY;
            if (j < S) {
                x = row[j];
#if ATTN_MASKED     // a predicated select before the bias; the wave owns row i and its lanes walk j: one 64-byte run of mask bytes
                x = (mk_rows_alike ? mk0[jj] : mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk]) ? x : ATTN_MASK_FILL;
#endif
                if (p.index_ld > 0 && i >= 1 && j >= 1)
                    x += p.table[(size_t)p.index[(size_t)(i - 1) * p.index_ld + (j - 1)] * p.H + h];
            }
            v[jj] = x;
            m = fmaxf(m, x);
        }
        m = wave_max(m);
        float s = 0.f;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            v[jj] = (lane + 64 * jj < S) ? expf(v[jj] - m) : 0.f;
            s += v[jj];
        }
        s = wave_sum(s);
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = lane + 64 * jj;
            if (j < SP) {
                float pv = 0.f;
                if (j < S) {
                    pv = v[jj] / s;
                    pr_base[(size_t)i * S + j] = pv;
                    if (p.has_drop) pv = drop_keep(flat0 + (uint32_t)(i * S + j), dkn) ? pv * dkn.scale : 0.f;
                }
                row[j] = pv;
            }
        }
    }
    __syncthreads();
    lds_times_rows<T, false, BF>(sm, Vb, p.ldv, S, p.dv, 1.f, Ob, p.ldo, reinterpret_cast<__bf16*>(p.Op), (uint32_t)n * (uint32_t)S,
                             (uint32_t)((h * p.dv) >> 5), (uint32_t)p.kbo);
}

template <int T>
__global__ void __launch_bounds__(NT, T <= 3 ? 2 : 1) ATTN1_BWD(const AttnParams p ATTN_MASK_PARAM) {
    const DropKey dkn = drop_key_now(p.dkey);
    constexpr bool BF = false;       // first generation: exact-f32 products only (bf16 products made these latency-bound loops slower)
    constexpr int SP = 32 * T, LD = SP + 1, NJ = (SP + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Dm = sm;                 // dP~ then dA
    float* Pm = sm + SP * LD;       // dropped probabilities
    float* tacc = sm + 2 * SP * LD; // [NT/64][table_rows] bias-table gradient of this head, one copy per wave
    const int h = ATTN_HEAD, S = p.S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has_bias = p.index_ld > 0 && p.dtable != nullptr;
    if (has_bias)
        for (int i = threadIdx.x; i < (NT / 64) * p.table_rows; i += NT) tacc[i] = 0.f;
    // a wave owns its copy: within one row i the S - 1 columns map to distinct table rows (relative offsets of distinct
    // positions differ), and a wave walks its rows in order, so plain read-modify-write is race-free and the sum order fixed
    float* const tw = tacc + wave * p.table_rows;
    const int n_begin = ATTN_CHUNK * p.n_per_wg;
    const int n_end = min(p.N, n_begin + p.n_per_wg);
#pragma unroll 1
    for (int n = n_begin; n < n_end; ++n) {
        const float* Qb = p.Q + (size_t)n * S * p.ldq + (size_t)h * p.dk;
        const float* Kb = p.K + (size_t)n * S * p.ldk + (size_t)h * p.dk;
        const float* Vb = p.V + (size_t)n * S * p.ldv + (size_t)h * p.dv;
        const float* dOb = p.dO + (size_t)n * S * p.ldo + (size_t)h * p.dv;
        __syncthreads();   // previous sequence's LDS readers are done
#pragma unroll 1
        for (int t = wave; t < T * T; t += NT / 64) {
            const int ti = t / T, tj = t % T;
            if (32 * ti >= S || 32 * tj >= S) continue;
            const floatx16 acc = tile_abt<BF>(dOb, p.ldo, 32 * ti, Vb, p.ldv, 32 * tj, S, p.dv, 1.f, p.vec_v);
            store_tile_lds<LD>(Dm, ti, tj, acc);
        }
        __syncthreads();
        const float* pr_base = p.probs + ((size_t)n * p.H + h) * S * S;
        const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
#if ATTN_MASKED
        const uint8_t* const mk_nh = mk.m + (int64_t)n * mk.sn + (int64_t)h * mk.sh;
        const bool mk_rows_alike = mk.sq == 0;          // as in the forward: a key-padding mask is read once per (sequence, head)
        uint8_t mk0[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) mk0[jj] = (mk_rows_alike && lane + 64 * jj < S) ? mk_nh[(int64_t)(lane + 64 * jj) * mk.sk] : (uint8_t)1;
#endif
#pragma unroll 1
        for (int i = wave; i < SP; i += NT / 64) {
            float* drow = Dm + i * LD;
            float* prow = Pm + i * LD;
            if (i >= S) {
                for (int j = lane; j < SP; j += 64) drow[j] = prow[j] = 0.f;
                continue;
            }
            float pv[NJ], dp[NJ], keep[NJ];
#if ATTN_MASKED
            bool kept[NJ];
#endif
            float s = 0.f;
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = lane + 64 * jj;
                pv[jj] = dp[jj] = keep[jj] = 0.f;
#if ATTN_MASKED
                kept[jj] = j < S ? (mk_rows_alike ? mk0[jj] : mk_nh[(int64_t)i * mk.sq + (int64_t)j * mk.sk]) != 0 : true;
#endif
                if (j < S) {
                    pv[jj] = pr_base[(size_t)i * S + j];
                    keep[jj] = p.has_drop ? (drop_keep(flat0 + (uint32_t)(i * S + j), dkn) ? dkn.scale : 0.f) : 1.f;
                    dp[jj] = drow[j] * keep[jj];
                    s += dp[jj] * pv[jj];
                }
            }
            s = wave_sum(s);
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = lane + 64 * jj;
                if (j < SP) {
                    const float da = pv[jj] * (dp[jj] - s);      // zero for j >= S
#if ATTN_MASKED     // dQ = dA K and dK = dA^T Q read Dm: no gradient reaches q.k at a masked position; the bias table below still gets dA
                    drow[j] = kept[jj] ? da : 0.f;
#else
                    drow[j] = da;
#endif
                    prow[j] = pv[jj] * keep[jj];
                    if (has_bias && i >= 1 && j >= 1 && j < S)
                        tw[p.index[(size_t)(i - 1) * p.index_ld + (j - 1)]] += da;
                }
            }
        }
        __syncthreads();
        lds_times_rows<T, true, BF>(Pm, dOb, p.ldo, S, p.dv, 1.f, p.dV + (size_t)n * S * p.ldv + (size_t)h * p.dv, p.ldv);
        lds_times_rows<T, false, BF>(Dm, Kb, p.ldk, S, p.dk, p.scale, p.dQ + (size_t)n * S * p.ldq + (size_t)h * p.dk, p.ldq);
        lds_times_rows<T, true, BF>(Dm, Qb, p.ldq, S, p.dk, p.scale, p.dK + (size_t)n * S * p.ldk + (size_t)h * p.dk, p.ldk);
    }
    if (has_bias) {
        __syncthreads();
        for (int i = threadIdx.x; i < p.table_rows; i += NT) {
            float v = tacc[i];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) v += tacc[w * p.table_rows + i];
            if (p.table_partials) p.dtable[((size_t)ATTN_CHUNK * p.table_rows + i) * p.H + h] = v;
            else atomicAdd(&p.dtable[(size_t)i * p.H + h], v);
        }
    }
}
