// Frame-level ROC-AUC on the device (include/lstc_hip.h, "metrics"): the tie-aware trapezoid AUC of frames that repeat R row
// scores is a weighted Mann-Whitney count over the rows,
//     U2 = sum_i sum_j pos_i neg_j (2 [s_i > s_j] + [s_i == s_j]),   AUC = U2 / (2 P N),
// pure integer work: exact, independent of the launch shape, no sort, no atomics.  Two launches: auc_pairs_kernel (one 64-bit
// partial per workgroup) and auc_finish_kernel (one workgroup sums the partials and writes the record).
#include "lstc_common.h"

namespace {

constexpr int AUC_NT = 256;            // rows i of a workgroup, one per thread
constexpr int AUC_CHUNK = 1024;        // rows j staged through LDS at a time: 8 KiB of (score, neg) pairs
constexpr int AUC_MAX_SLICES = 64;     // grid.y: slices of rows j (whole chunks); the partials stay at 8 nb * 64 bytes
constexpr int64_t AUC_MAX_ROWS = 1ll << 24;
constexpr uint64_t AUC_MAX_FRAMES = 1ull << 26;

struct AucPlan {
    int64_t nb;      // workgroups along i
    int64_t ns;      // slices along j, none empty
    int64_t slice;   // rows j of a slice, a multiple of AUC_CHUNK
};

inline AucPlan auc_plan(int64_t n) {
    AucPlan p;
    p.nb = (n + AUC_NT - 1) / AUC_NT;
    const int64_t chunks = (n + AUC_CHUNK - 1) / AUC_CHUNK;
    const int64_t want = chunks < AUC_MAX_SLICES ? chunks : AUC_MAX_SLICES;
    p.slice = (chunks + want - 1) / want * AUC_CHUNK;
    p.ns = (n + p.slice - 1) / p.slice;
    return p;
}

// workspace (8-byte words behind the first 8-byte boundary): partial[ns][nb], pos_sum[nb], neg_sum[nb], nan_flag[nb]
inline int64_t auc_words(const AucPlan& p) { return p.nb * p.ns + 3 * p.nb; }

__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the AUC_NT threads (integers: any order gives the same bits); `red` holds AUC_NT / 64 words of LDS.
__device__ inline unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < AUC_NT / 64; ++w) t += red[w];
    return t;
}

// grid (nb, ns).  Thread t of block (bx, by) owns row i = 256 bx + t and walks the rows j of slice by: gt += neg_j where
// s_i > s_j, eq += neg_j where s_i == s_j (32 bits each: P + N <= 2^26 keeps 2 gt + eq below 2^28), then pos_i (2 gt + eq) in
// 64 bits.  The chunk's (score, neg) pairs lie interleaved in LDS and every lane reads the same 16 bytes per step (a broadcast).
// A NaN compares false both ways and a row without weight adds zeros, so neither needs a branch.  Slice 0 also sums the block's
// pos, neg and "weighted row with a NaN score" words.
__global__ __launch_bounds__(AUC_NT) void auc_pairs_kernel(const float* __restrict__ scores, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ neg, int n, int slice,
                                                            unsigned long long* __restrict__ partial,
                                                            unsigned long long* __restrict__ pos_sum,
                                                            unsigned long long* __restrict__ neg_sum,
                                                            unsigned long long* __restrict__ nan_flag) {
    __shared__ float4 sh[AUC_CHUNK / 2];
    __shared__ unsigned long long red[AUC_NT / 64];
    const int tid = threadIdx.x;
    const int i = (int)blockIdx.x * AUC_NT + tid;
    const bool live = i < n;
    const float si = live ? scores[i] : 0.f;
    const uint32_t pi = live ? pos[i] : 0u;
    if (blockIdx.y == 0) {
        const uint32_t ni = live ? neg[i] : 0u;
        const unsigned long long ps = block_sum_u64(pi, red), ns = block_sum_u64(ni, red);
        const unsigned long long bad = block_sum_u64(((pi | ni) != 0u && si != si) ? 1ull : 0ull, red);
        if (tid == 0) {
            pos_sum[blockIdx.x] = ps;
            neg_sum[blockIdx.x] = ns;
            nan_flag[blockIdx.x] = bad ? 1ull : 0ull;
        }
    }
    unsigned long long* const mine = partial + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (!__syncthreads_or(pi != 0u)) {            // block-uniform: no positive frame in these 256 rows (most of a list of normal videos)
        if (tid == 0) *mine = 0ull;
        return;
    }
    const int j0 = (int)blockIdx.y * slice;
    const int j1 = min(n, j0 + slice);
    uint32_t gt = 0u, eq = 0u;
    for (int c = j0; c < j1; c += AUC_CHUNK) {
        __syncthreads();                          // the previous chunk has been read
#pragma unroll
        for (int k = 0; k < AUC_CHUNK / AUC_NT; ++k) {
            const int q = tid + k * AUC_NT, j = c + q;
            float2 v = make_float2(0.f, 0.f);      // past the slice: weight 0
            if (j < j1) v = make_float2(scores[j], __uint_as_float(neg[j]));
            reinterpret_cast<float2*>(sh)[q] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < AUC_CHUNK / 2; ++q) {
            const float4 v = sh[q];
            gt += si > v.x ? __float_as_uint(v.y) : 0u;
            eq += si == v.x ? __float_as_uint(v.y) : 0u;
            gt += si > v.z ? __float_as_uint(v.w) : 0u;
            eq += si == v.z ? __float_as_uint(v.w) : 0u;
        }
    }
    const unsigned long long u = block_sum_u64((unsigned long long)pi * (2ull * gt + eq), red);
    if (tid == 0) *mine = u;
}

// One workgroup: U2 = sum of the partials, P, N, the flags, then the one division.
__global__ __launch_bounds__(AUC_NT) void auc_finish_kernel(const unsigned long long* __restrict__ partial, int64_t n_partial,
                                                             const unsigned long long* __restrict__ pos_sum,
                                                             const unsigned long long* __restrict__ neg_sum,
                                                             const unsigned long long* __restrict__ nan_flag, int64_t nb,
                                                             LstcAucOut* __restrict__ out) {
    __shared__ unsigned long long red[AUC_NT / 64];
    unsigned long long u = 0, p = 0, m = 0, bad = 0;
    for (int64_t k = threadIdx.x; k < n_partial; k += AUC_NT) u += partial[k];
    for (int64_t k = threadIdx.x; k < nb; k += AUC_NT) {
        p += pos_sum[k];
        m += neg_sum[k];
        bad += nan_flag[k];
    }
    u = block_sum_u64(u, red);
    p = block_sum_u64(p, red);
    m = block_sum_u64(m, red);
    bad = block_sum_u64(bad, red);
    if (threadIdx.x != 0) return;
    const uint32_t flags = (bad ? LSTC_AUC_NAN_SCORE : 0u) | (p + m > AUC_MAX_FRAMES ? LSTC_AUC_TOO_MANY_FRAMES : 0u);
    double auc = __longlong_as_double(0x7ff8000000000000ll);
    if (!flags && p != 0 && m != 0) auc = (double)u / (2.0 * (double)p * (double)m);      // 2 P N < 2^53: every operand is exact
    out->u2 = u;
    out->pos = p;
    out->neg = m;
    out->auc = auc;
    out->flags = flags;
    out->reserved = 0u;
}

}  // namespace

extern "C" {

int64_t lstc_auc_workspace_bytes(int64_t n) {
    const int64_t rows = n < 1 ? 1 : (n > AUC_MAX_ROWS ? AUC_MAX_ROWS : n);
    return 8 * auc_words(auc_plan(rows)) + 8;      // + 8: the words start at the first 8-byte boundary of any workspace
}

int lstc_auc_weighted(const float* scores, const uint32_t* pos, const uint32_t* neg, int64_t n, void* workspace,
                      int64_t workspace_bytes, LstcAucOut* out, void* stream) {
    if (!scores || !pos || !neg || !workspace || !out) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    if (n > AUC_MAX_ROWS) return LSTC_E_RANGE;
    if (workspace_bytes < lstc_auc_workspace_bytes(n)) return LSTC_E_SHAPE;
    if (((uintptr_t)out) & 7u) return LSTC_E_ALIGN;
    const AucPlan p = auc_plan(n);
    unsigned long long* const part = (unsigned long long*)((((uintptr_t)workspace) + 7u) & ~(uintptr_t)7u);
    unsigned long long* const ps = part + p.nb * p.ns;
    unsigned long long* const ns = ps + p.nb;
    unsigned long long* const bad = ns + p.nb;
    hipLaunchKernelGGL(auc_pairs_kernel, dim3((unsigned)p.nb, (unsigned)p.ns), AUC_NT, 0, (hipStream_t)stream, scores, pos, neg,
                       (int)n, (int)p.slice, part, ps, ns, bad);
    const int rc = lstc_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(auc_finish_kernel, dim3(1), AUC_NT, 0, (hipStream_t)stream, (const unsigned long long*)part, p.nb * p.ns,
                       (const unsigned long long*)ps, (const unsigned long long*)ns, (const unsigned long long*)bad, p.nb, out);
    return lstc_launch_status();
}

}  // extern "C"
