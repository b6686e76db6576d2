// Frame-level ROC-AUC on the device (include/lstc_hip.h, "metrics"): the tie-aware trapezoid AUC of frames that repeat R row
// scores is a weighted Mann-Whitney count over the rows,
//     U2 = sum_i sum_j pos_i neg_j (2 [s_i > s_j] + [s_i == s_j]),   AUC = U2 / (2 P N),
// pure integer work: exact, independent of the launch shape, no sort, no atomics.  Two launches: auc_pairs_kernel (one 64-bit
// partial per workgroup) and auc_finish_kernel (one workgroup sums the partials and writes the record).
#include "lstc_common.h"

#include <cstdlib>

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

// ------------------------------------------------------------------------------------------------ detection report
// lstc_det_report (include/lstc_hip.h): AUC, AP, trapezoid PR-AUC, the confusion counts at up to 8 thresholds and the score sums of
// the frames, overall or per group of rows, from the same (score, pos, neg) rows.  Every curve metric is a function of four per-row
// counts over the rows j of row i's own group,
//     tp_ge = sum pos_j [s_j >= s_i],  fp_ge = sum neg_j [s_j >= s_i],  tp_eq / fp_eq the same under s_j == s_i,
// which det_pairs_kernel forms for every row that covers a positive frame (integers; slices of rows j meet in integer atomics, so
// the counts are the same whatever the grid); det_finish_kernel, one workgroup per group with a fixed thread -> row assignment and
// a fixed reduction tree, turns them into the record.
constexpr int DET_NT = 256;             // rows i of a workgroup, one per thread
constexpr int DET_CHUNK = 256;          // rows j staged through LDS at a time: one 16-byte (score, pos, neg, gid) record per thread
constexpr int DET_MAX_SLICES = 64;      // grid.y
constexpr int DET_FILL = 2048;          // workgroups the plan aims at: 256 CUs x 8 resident workgroups of 256 threads
constexpr int64_t DET_MAX_ROWS = 1ll << 20;
constexpr int64_t DET_MAX_GROUPS = 64;
constexpr uint64_t DET_MAX_FRAMES = 1ull << 26;
static_assert(DET_NT == AUC_NT, "block_sum_u64 sums AUC_NT threads");

struct DetPlan {
    int64_t nb;      // workgroups along i
    int64_t ns;      // slices along j, none empty
    int64_t slice;   // rows j of a slice, a multiple of DET_CHUNK
};

// Few row blocks: split the rows j so that about DET_FILL workgroups run (19 x 19 at 4 640 rows, 49 x 25 at 12 461, 146 x 15 at
// 37 202); from 2048 row blocks on there is one slice.  `force` > 0 (tests: the counts must not depend on the plan) asks for that
// many slices instead.
inline DetPlan det_plan(int64_t n, int64_t force) {
    DetPlan p;
    p.nb = (n + DET_NT - 1) / DET_NT;
    const int64_t chunks = (n + DET_CHUNK - 1) / DET_CHUNK;
    int64_t want = force > 0 ? force : (DET_FILL + p.nb - 1) / p.nb;
    if (want > DET_MAX_SLICES) want = DET_MAX_SLICES;
    if (want > chunks) want = chunks;
    p.slice = (chunks + want - 1) / want * DET_CHUNK;
    p.ns = (n + p.slice - 1) / p.slice;
    return p;
}

// grid (nb, ns).  Thread t of block (bx, by) owns row i = 256 bx + t and walks the rows j of slice by.  A chunk's records lie in
// LDS and every lane reads the same 16 bytes per step (a broadcast); the next chunk's record is fetched into registers under the
// walk.  Two compares and four conditional adds per pair (GROUPED: one more compare, ANDed into both masks).  >= and == on the
// floats: +0.0 and -0.0 tie, a NaN on either side compares false.  A record past the slice has weight 0.  Only rows with
// pos_i > 0 store their counts - the finish kernel reads no others - and a workgroup without such a row leaves at once.
template <bool GROUPED>
__global__ __launch_bounds__(DET_NT) void det_pairs_kernel(const float* __restrict__ scores, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ neg, const uint32_t* __restrict__ gid, int n,
                                                            int slice, int atomic, uint32_t* __restrict__ counts) {
    __shared__ float4 sh[DET_CHUNK];
    const int tid = threadIdx.x;
    const int i = (int)blockIdx.x * DET_NT + tid;
    const bool live = i < n;
    const uint32_t pi = live ? pos[i] : 0u;
    if (!__syncthreads_or(pi != 0u)) return;      // block-uniform
    const float si = live ? scores[i] : 0.f;
    const uint32_t gi = (GROUPED && live) ? gid[i] : 0u;
    const int j0 = (int)blockIdx.y * slice;
    const int j1 = min(n, j0 + slice);
    auto record = [&](int j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < j1) {
            v.x = scores[j];
            v.y = __uint_as_float(pos[j]);
            v.z = __uint_as_float(neg[j]);
            if (GROUPED) v.w = __uint_as_float(gid[j]);
        }
        return v;
    };
    uint32_t tp_ge = 0u, fp_ge = 0u, tp_eq = 0u, fp_eq = 0u;
    float4 next = record(j0 + tid);
    for (int c = j0; c < j1; c += DET_CHUNK) {
        __syncthreads();                          // the previous chunk has been read
        sh[tid] = next;
        __syncthreads();
        if (c + DET_CHUNK < j1) next = record(c + DET_CHUNK + tid);
#pragma unroll 8
        for (int q = 0; q < DET_CHUNK; ++q) {
            const float4 v = sh[q];
            bool ge = v.x >= si, eq = v.x == si;
            if (GROUPED) {
                const bool same = __float_as_uint(v.w) == gi;
                ge = ge && same;
                eq = eq && same;
            }
            tp_ge += ge ? __float_as_uint(v.y) : 0u;
            fp_ge += ge ? __float_as_uint(v.z) : 0u;
            tp_eq += eq ? __float_as_uint(v.y) : 0u;
            fp_eq += eq ? __float_as_uint(v.z) : 0u;
        }
    }
    if (pi == 0u) return;                         // also every thread past n
    uint32_t* const mine = counts + 4 * (size_t)i;
    if (atomic) {                                 // several slices: the words were zeroed before the launch
        atomicAdd(mine + 0, tp_ge);
        atomicAdd(mine + 1, fp_ge);
        atomicAdd(mine + 2, tp_eq);
        atomicAdd(mine + 3, fp_eq);
    } else {
        *reinterpret_cast<uint4*>(mine) = make_uint4(tp_ge, fp_ge, tp_eq, fp_eq);
    }
}

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // both lanes of a pair add the same two values: one tree
    return v;
}

// The fixed tree of the f64 sums: the xor butterfly inside a wave, then the four waves in their order.
__device__ inline double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < DET_NT / 64; ++w) t += red[w];
    return t;
}

// grid (n_groups).  Workgroup g, thread t: rows t, t + 256, ... in that order, then the fixed tree - every f64 sum has one order
// whatever grid the pair kernel ran on.  NaN rows with weight raise the flag and stay out of every sum but pos / neg.
template <bool GROUPED>
__global__ __launch_bounds__(DET_NT) void det_finish_kernel(const float* __restrict__ scores, const uint32_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ neg, const uint32_t* __restrict__ gid, int n,
                                                             const float* __restrict__ thresholds, int n_thresholds,
                                                             const uint32_t* __restrict__ counts, LstcDetOut* __restrict__ out) {
    __shared__ unsigned long long red[DET_NT / 64];
    __shared__ double redf[DET_NT / 64];
    const uint32_t g = blockIdx.x;
    float th[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) th[k] = k < n_thresholds ? thresholds[k] : 0.f;
    unsigned long long P = 0, N = 0, Pv = 0, Nv = 0, A = 0, bad = 0, tp[8], fp[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tp[k] = fp[k] = 0;
    double ap = 0.0, pr = 0.0, sp = 0.0, sn = 0.0, se = 0.0;
    for (int i = threadIdx.x; i < n; i += DET_NT) {
        if (GROUPED && gid[i] != g) continue;
        const uint32_t pi = pos[i], ni = neg[i];
        if ((pi | ni) == 0u) continue;            // the row does not exist: its score is not read
        const float s = scores[i];
        P += pi;
        N += ni;
        if (s != s) {
            bad = 1;
            continue;
        }
        Pv += pi;
        Nv += ni;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool over = k < n_thresholds && s > th[k];
            tp[k] += over ? pi : 0u;
            fp[k] += over ? ni : 0u;
        }
        const double ds = (double)s, dp = (double)pi, dn = (double)ni, d1 = 1.0 - ds;
        sp += dp * ds;
        sn += dn * ds;
        se += dp * (d1 * d1) + dn * (ds * ds);
        if (pi != 0u) {
            const uint4 c = *reinterpret_cast<const uint4*>(counts + 4 * (size_t)i);      // tp_ge, fp_ge, tp_eq, fp_eq
            A += (unsigned long long)pi * (2ull * c.y - c.w);
            const double prec = (double)c.x / (double)(c.x + c.y);                        // tp_ge >= pos_i > 0
            const uint32_t tg = c.x - c.z, fg = c.y - c.w;
            const double prev = (tg + fg) != 0u ? (double)tg / (double)(tg + fg) : 1.0;   // the closing point (recall 0, precision 1)
            ap += dp * prec;
            pr += dp * ((prec + prev) * 0.5);
        }
    }
    P = block_sum_u64(P, red);
    N = block_sum_u64(N, red);
    Pv = block_sum_u64(Pv, red);
    Nv = block_sum_u64(Nv, red);
    A = block_sum_u64(A, red);
    bad = block_sum_u64(bad, red);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        tp[k] = block_sum_u64(tp[k], red);
        fp[k] = block_sum_u64(fp[k], red);
    }
    ap = block_sum_f64(ap, redf);
    pr = block_sum_f64(pr, redf);
    sp = block_sum_f64(sp, redf);
    sn = block_sum_f64(sn, redf);
    se = block_sum_f64(se, redf);
    if (threadIdx.x != 0) return;
    LstcDetOut* const o = out + g;
    const uint32_t flags = (bad ? LSTC_DET_NAN_SCORE : 0u) | (P + N > DET_MAX_FRAMES ? LSTC_DET_TOO_MANY_FRAMES : 0u);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned long long u2 = 2ull * Nv * Pv - A;      // sum pos_i (2 (N - fp_ge) + fp_eq) over the rows with a real score
    o->pos = P;
    o->neg = N;
    o->u2 = u2;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        o->tp_at[k] = tp[k];
        o->fp_at[k] = fp[k];
    }
    o->auc = (!flags && P != 0 && N != 0) ? (double)u2 / (2.0 * (double)P * (double)N) : nan;      // as lstc_auc_weighted
    o->ap = (!flags && P != 0) ? ap / (double)P : nan;
    o->pr_auc = (!flags && P != 0) ? pr / (double)P : nan;
    o->sum_s_pos = flags ? nan : sp;
    o->sum_s_neg = flags ? nan : sn;
    o->sum_sq_err = flags ? nan : se;
    o->flags = flags;
    o->reserved = 0u;
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

// workspace: the four 32-bit counts of every row behind the first 16-byte boundary - 16 n + 16 bytes, whatever the plan
int64_t lstc_det_workspace_bytes(int64_t n, int64_t n_groups) {
    (void)n_groups;
    const int64_t rows = n < 1 ? 1 : (n > DET_MAX_ROWS ? DET_MAX_ROWS : n);
    return 16 * rows + 16;
}

int lstc_det_report(const float* scores, const uint32_t* pos, const uint32_t* neg, const uint32_t* gid, int64_t n, int64_t n_groups,
                    const float* thresholds, int32_t n_thresholds, void* workspace, int64_t workspace_bytes, LstcDetOut* out,
                    void* stream) {
    if (!scores || !pos || !neg || !thresholds || !workspace || !out) return LSTC_E_NULL;
    if (n <= 0 || n_groups <= 0 || n_thresholds < 1 || n_thresholds > 8) return LSTC_E_SHAPE;
    if (!gid && n_groups != 1) return LSTC_E_SHAPE;
    if (n > DET_MAX_ROWS || n_groups > DET_MAX_GROUPS) return LSTC_E_RANGE;
    if (workspace_bytes < lstc_det_workspace_bytes(n, n_groups)) return LSTC_E_SHAPE;
    if (((uintptr_t)out) & 7u) return LSTC_E_ALIGN;
    // LSTC_DET_SLICES: the number of j slices, for the tests that compare two plans of one input; not a tuning knob
    const char* const forced = getenv("LSTC_DET_SLICES");
    const DetPlan p = det_plan(n, forced ? atoll(forced) : 0);
    uint32_t* const counts = (uint32_t*)((((uintptr_t)workspace) + 15u) & ~(uintptr_t)15u);
    const hipStream_t st = (hipStream_t)stream;
    const int atomic = p.ns > 1;
    if (atomic && hipMemsetAsync(counts, 0, 16 * (size_t)n, st) != hipSuccess) return lstc_launch_status();      // the memset's own error
    const dim3 grid((unsigned)p.nb, (unsigned)p.ns);
    if (gid)
        hipLaunchKernelGGL(det_pairs_kernel<true>, grid, DET_NT, 0, st, scores, pos, neg, gid, (int)n, (int)p.slice, atomic, counts);
    else
        hipLaunchKernelGGL(det_pairs_kernel<false>, grid, DET_NT, 0, st, scores, pos, neg, gid, (int)n, (int)p.slice, atomic, counts);
    const int rc = lstc_launch_status();
    if (rc) return rc;
    if (gid)
        hipLaunchKernelGGL(det_finish_kernel<true>, dim3((unsigned)n_groups), DET_NT, 0, st, scores, pos, neg, gid, (int)n, thresholds,
                           (int)n_thresholds, (const uint32_t*)counts, out);
    else
        hipLaunchKernelGGL(det_finish_kernel<false>, dim3(1), DET_NT, 0, st, scores, pos, neg, gid, (int)n, thresholds,
                           (int)n_thresholds, (const uint32_t*)counts, out);
    return lstc_launch_status();
}

}  // extern "C"
