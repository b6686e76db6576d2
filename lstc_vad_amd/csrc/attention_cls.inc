// CLS-query attention kernels, forward and backward: the kernel text.
// Included twice by csrc/attention.hip: once with ATTN_MASKED 0 under the kernels' own names - the text the compiler sees is then exactly what
// it was before attention masks existed, so the unmasked kernels come out instruction for instruction as they were (checked by
// tools/attn_isa_diff.py) - and once with ATTN_MASKED 1 as attn_cls_fwd_masked_kernel / attn_cls_bwd_masked_kernel, which take the mask as a second kernel argument.
// No include guard on purpose.
template <int MAXS>
__global__ void __launch_bounds__(NT) ATTN_CLS_FWD(const ClsParams p ATTN_MASK_PARAM) {
    constexpr int NJ = MAXS / 64;
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ float sc[NT / 64][MAXS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.x * (NT / 64) + wave;
    if (pair >= p.N * p.H) return;
    const int n = pair / p.H, h = pair % p.H, S = p.S;
    const float* q = p.Q + (size_t)n * p.ldq + (size_t)h * p.dk;
    const float* Kb = p.K + (size_t)n * S * p.ldk + (size_t)h * p.dk;
    const float* Vb = p.V + (size_t)n * S * p.ldv + (size_t)h * p.dv;
    float* s = sc[wave];
    for (int j = 0; j < S; ++j) {
        float a = 0.f;
        for (int c = lane; c < p.dk; c += 64) a += (q[c] * p.scale) * Kb[(size_t)j * p.ldk + c];
        a = wave_sum(a);
        if (lane == 0) s[j] = a;
    }
    __builtin_amdgcn_wave_barrier();
    float v[NJ], m = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = lane + 64 * jj;
        v[jj] = j < S ? s[j] : -INFINITY;
#if ATTN_MASKED     // row 0 of the mask; row 0 carries no bias
        if (j < S) v[jj] = mk.m[(int64_t)n * mk.sn + (int64_t)h * mk.sh + (int64_t)j * mk.sk] ? v[jj] : ATTN_MASK_FILL;
#endif
        m = fmaxf(m, v[jj]);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        v[jj] = (lane + 64 * jj < S) ? expf(v[jj] - m) : 0.f;
        sum += v[jj];
    }
    sum = wave_sum(sum);
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);       // row 0 of the full tensor
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = lane + 64 * jj;
        if (j < S) {
            float pv = v[jj] / sum;
            p.probs[((size_t)n * p.H + h) * S + j] = pv;
            if (p.has_drop) pv = drop_keep(flat0 + (uint32_t)j, dkn) ? pv * dkn.scale : 0.f;
            s[j] = pv;
        }
    }
    __builtin_amdgcn_wave_barrier();
    float* o = p.O + (size_t)n * p.ldo + (size_t)h * p.dv;
    for (int c = lane; c < p.dv; c += 64) {
        float a = 0.f;
        for (int j = 0; j < S; ++j) a += s[j] * Vb[(size_t)j * p.ldv + c];
        o[c] = a;
    }
}

template <int MAXS>
__global__ void __launch_bounds__(NT) ATTN_CLS_BWD(const ClsParams p ATTN_MASK_PARAM) {
    constexpr int NJ = MAXS / 64;
    const DropKey dkn = drop_key_now(p.dkey);
    __shared__ float sp[NT / 64][MAXS];      // dropped probabilities
    __shared__ float sd[NT / 64][MAXS];      // d(logit)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.x * (NT / 64) + wave;
    if (pair >= p.N * p.H) return;
    const int n = pair / p.H, h = pair % p.H, S = p.S;
    const float* q = p.Q + (size_t)n * p.ldq + (size_t)h * p.dk;
    const float* Kb = p.K + (size_t)n * S * p.ldk + (size_t)h * p.dk;
    const float* Vb = p.V + (size_t)n * S * p.ldv + (size_t)h * p.dv;
    const float* dO = p.dO + (size_t)n * p.ldo + (size_t)h * p.dv;
    float* dKb = p.dK + (size_t)n * S * p.ldk + (size_t)h * p.dk;
    float* dVb = p.dV + (size_t)n * S * p.ldv + (size_t)h * p.dv;
    float* pd = sp[wave];
    float* ds = sd[wave];
    // dP~_j = dO . V_j
    for (int j = 0; j < S; ++j) {
        float a = 0.f;
        for (int c = lane; c < p.dv; c += 64) a += dO[c] * Vb[(size_t)j * p.ldv + c];
        a = wave_sum(a);
        if (lane == 0) ds[j] = a;
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t flat0 = ((uint32_t)n * p.H + h) * (uint32_t)(S * S);
    float pv[NJ], dp[NJ], keep[NJ], rs = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = lane + 64 * jj;
        pv[jj] = dp[jj] = keep[jj] = 0.f;
        if (j < S) {
            pv[jj] = p.probs[((size_t)n * p.H + h) * S + j];
            keep[jj] = p.has_drop ? (drop_keep(flat0 + (uint32_t)j, dkn) ? dkn.scale : 0.f) : 1.f;
            dp[jj] = ds[j] * keep[jj];
            rs += dp[jj] * pv[jj];
        }
    }
    rs = wave_sum(rs);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int j = lane + 64 * jj;
        if (j < S) {
#if ATTN_MASKED     // d(logit) of a masked key is zero (no bias in row 0, so nothing else consumes it)
            ds[j] = mk.m[(int64_t)n * mk.sn + (int64_t)h * mk.sh + (int64_t)j * mk.sk] ? pv[jj] * (dp[jj] - rs) : 0.f;
#else
            ds[j] = pv[jj] * (dp[jj] - rs);
#endif
            pd[j] = pv[jj] * keep[jj];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // dV_j = Pd_j dO ; dK_j = scale dA_j q ; dq = scale sum_j dA_j K_j
    for (int c = lane; c < p.dv; c += 64) {
        const float g = dO[c];
        for (int j = 0; j < S; ++j) dVb[(size_t)j * p.ldv + c] = pd[j] * g;
    }
    float* dq = p.dQ + (size_t)n * p.ldq + (size_t)h * p.dk;
    for (int c = lane; c < p.dk; c += 64) {
        const float qs = q[c] * p.scale;
        float a = 0.f;
        for (int j = 0; j < S; ++j) {
            a += ds[j] * Kb[(size_t)j * p.ldk + c];
            dKb[(size_t)j * p.ldk + c] = ds[j] * qs;
        }
        dq[c] = a * p.scale;
    }
}
