// HBM-bound row-wise kernels of the training step (gfx950): LayerNorm fwd/bwd, CLS-mean + concat,
// column sums, dropout replay, the fused last head layer, Adagrad, squared-norm.
// All of them stream their operands once with 16-B-per-lane accesses where the layout allows
// (cdna_hip_programming Guideline 13) and reduce with wave shuffles.
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>
#include <vector>
#include "lstc_common.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------------------- LayerNorm
// One wave per row; the row lives in registers (NV float4 per lane, d <= 256*NV) so x is read once.
// Two-pass statistics (mean, then centred variance) like ATen's CPU kernel for parity.
typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));

template <int NV>
__global__ void __launch_bounds__(NT) ln_fwd_vec(const float* __restrict__ x, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float* __restrict__ y,
                                                  float* __restrict__ mean, float* __restrict__ rstd, int64_t rows,
                                                  int d, float eps, __bf16* __restrict__ packed, int KBp) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (NT / 64);
    const int nv4 = d >> 2;
    float4 g[NV], b[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv4) {
            g[i] = reinterpret_cast<const float4*>(gamma)[c];
            b[i] = reinterpret_cast<const float4*>(beta)[c];
        }
    }
    for (int64_t r = wave0; r < rows; r += nwaves) {
        const float4* xr = reinterpret_cast<const float4*>(x + r * d);
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < nv4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
        const float mu = wave_sum(s) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv4) {
                const float a0 = v[i].x - mu, a1 = v[i].y - mu, a2 = v[i].z - mu, a3 = v[i].w - mu;
                q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        }
        const float rs = 1.f / sqrtf(wave_sum(q) / (float)d + eps);
        float4* yr = reinterpret_cast<float4*>(y + r * d);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv4) {
                float4 o;
                o.x = (v[i].x - mu) * rs * g[i].x + b[i].x;
                o.y = (v[i].y - mu) * rs * g[i].y + b[i].y;
                o.z = (v[i].z - mu) * rs * g[i].z + b[i].z;
                o.w = (v[i].w - mu) * rs * g[i].w + b[i].w;
                yr[c] = o;
                if (packed) {       // the same row in the packed bf16 layout of the next GEMM's A operand: 8 B per lane,
                    bf16x4v h;      // 8 lanes = one tile row's 64 contiguous bytes
                    h[0] = (__bf16)o.x; h[1] = (__bf16)o.y; h[2] = (__bf16)o.z; h[3] = (__bf16)o.w;
                    *reinterpret_cast<bf16x4v*>(packed + p1_offset(r, 4 * c, KBp)) = h;
                }
            }
        }
        if (lane == 0) {
            mean[r] = mu;
            rstd[r] = rs;
        }
    }
}

// Any d (odd widths, > 2048): scalar, three passes over the row (re-reads hit L1/L2).
__global__ void __launch_bounds__(NT) ln_fwd_generic(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ y,
                                                      float* __restrict__ mean, float* __restrict__ rstd, int64_t rows,
                                                      int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (NT / 64);
    for (int64_t r = wave0; r < rows; r += nwaves) {
        const float* xr = x + r * d;
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += xr[c];
        const float mu = wave_sum(s) / (float)d;
        float q = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float a = xr[c] - mu;
            q += a * a;
        }
        const float rs = 1.f / sqrtf(wave_sum(q) / (float)d + eps);
        for (int c = lane; c < d; c += 64) y[r * d + c] = (xr[c] - mu) * rs * gamma[c] + beta[c];
        if (lane == 0) {
            mean[r] = mu;
            rstd[r] = rs;
        }
    }
}

// dx = rstd * (g*dy - mean_d(g*dy) - xhat * mean_d(g*dy*xhat)); per-workgroup partial dgamma = sum dy*xhat,
// dbeta = sum dy written to partial[0][blockIdx.x][:] / partial[1][blockIdx.x][:].
// Two waves per row, the row in registers (d % 4 == 0, d <= 512 * NVH): half h of the pair owns the float4 columns
// h * 64 * NVH + lane + 64 * i (i < NVH) below d / 4, so the second half is full at d = 512 * NVH and empty at d <= 256 * NVH.
// A wave holds half the row's registers: three accumulator rows (dgamma, dbeta, column sums of df) fit at 3 waves/SIMD.  The row
// statistics cross the wave pair through LDS (double-buffered by iteration parity: one barrier per row pair).
// MODE 0: dx and the two partials only.  1: + df = dropout-replay(dx) rounded to bf16 in the lstc_pack1 layout (what the two GEMMs
// behind the residual branch consume; dropout index = flat row * d + col, as lstc_dropout_apply) + a third partial, the column
// sums of df (the bias gradient of the Linear in front of the dropout).  2: + f32 df + third partial (f32 modes: `packed` is then
// a float [rows, d]).  The dropout replay needs no pass of its own in any mode.
template <int NVH, int MODE>
__global__ void __launch_bounds__(NT) ln_bwd_pair(const float* __restrict__ dy, const float* __restrict__ x,
                                                   const float* __restrict__ gamma, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, float* __restrict__ dx,
                                                   float* __restrict__ partial, int64_t rows, int d,
                                                   __bf16* __restrict__ packed, int KBp, DropKey key) {
    key = drop_key_now(key);
    constexpr bool PACK = MODE != 0;
    extern __shared__ __attribute__((aligned(16))) float sm[];   // [2][d] combine buffer, then [2][4][64][2] per-lane row sums
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, slot = wv >> 1, half = wv & 1;
    const int nv4 = d >> 2, c0 = half * 64 * NVH + lane;
    float* red = sm + 2 * d;
    float4 g[NVH], ag[NVH], ab[NVH], ad[PACK ? NVH : 1];
#pragma unroll
    for (int i = 0; i < NVH; ++i) {
        const int c = c0 + 64 * i;
        g[i] = c < nv4 ? reinterpret_cast<const float4*>(gamma)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        ag[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (PACK) ad[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int64_t stride = (int64_t)gridDim.x * 2;
    const int64_t iters = (rows + stride - 1) / stride;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t r = it * stride + (int64_t)blockIdx.x * 2 + slot;
        const bool live = r < rows;
        const int64_t rr = live ? r : 0;
        const float4* xr = reinterpret_cast<const float4*>(x + rr * d);
        const float4* dr = reinterpret_cast<const float4*>(dy + rr * d);
        const float mu = mean[rr], rs = rstd[rr];
        float4 xh[NVH], gd[NVH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NVH; ++i) {
            const int c = c0 + 64 * i;
            if (c < nv4 && live) {
                const float4 xv = xr[c], dv = dr[c];
                xh[i] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
                gd[i] = make_float4(dv.x * g[i].x, dv.y * g[i].y, dv.z * g[i].z, dv.w * g[i].w);
                s1 += (gd[i].x + gd[i].y) + (gd[i].z + gd[i].w);
                s2 += (gd[i].x * xh[i].x + gd[i].y * xh[i].y) + (gd[i].z * xh[i].z + gd[i].w * xh[i].w);
                ag[i].x += dv.x * xh[i].x; ag[i].y += dv.y * xh[i].y; ag[i].z += dv.z * xh[i].z; ag[i].w += dv.w * xh[i].w;
                ab[i].x += dv.x; ab[i].y += dv.y; ab[i].z += dv.z; ab[i].w += dv.w;
            } else {
                xh[i] = gd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        float2* rb = reinterpret_cast<float2*>(red) + (it & 1) * 256;
        rb[wv * 64 + lane] = make_float2(s1, s2);
        __syncthreads();
        // lane l of both waves adds the pair's per-lane halves in the same order (the first half's columns first), then the same
        // butterfly: the pair agrees bit for bit
        const float2 pa = rb[(slot * 2) * 64 + lane], pb = rb[(slot * 2 + 1) * 64 + lane];
        const float m1 = wave_sum(pa.x + pb.x) / (float)d, m2 = wave_sum(pa.y + pb.y) / (float)d;
        if (!live) continue;
        float4* o = reinterpret_cast<float4*>(dx + r * d);
#pragma unroll
        for (int i = 0; i < NVH; ++i) {
            const int c = c0 + 64 * i;
            if (c < nv4) {
                const float4 ov = make_float4(rs * (gd[i].x - m1 - xh[i].x * m2), rs * (gd[i].y - m1 - xh[i].y * m2),
                                              rs * (gd[i].z - m1 - xh[i].z * m2), rs * (gd[i].w - m1 - xh[i].w * m2));
                o[c] = ov;
                if (!PACK) continue;
                const uint32_t fi = (uint32_t)(r * d) + 4u * (uint32_t)c;
                float4 f;
                f.x = drop_keep(fi + 0, key) ? ov.x * key.scale : 0.f;
                f.y = drop_keep(fi + 1, key) ? ov.y * key.scale : 0.f;
                f.z = drop_keep(fi + 2, key) ? ov.z * key.scale : 0.f;
                f.w = drop_keep(fi + 3, key) ? ov.w * key.scale : 0.f;
                ad[i].x += f.x; ad[i].y += f.y; ad[i].z += f.z; ad[i].w += f.w;
                if constexpr (MODE == 2) {
                    reinterpret_cast<float4*>(reinterpret_cast<float*>(packed) + r * d)[c] = f;
                } else {
                    bf16x4v h;
                    h[0] = (__bf16)f.x; h[1] = (__bf16)f.y; h[2] = (__bf16)f.z; h[3] = (__bf16)f.w;
                    *reinterpret_cast<bf16x4v*>(packed + p1_offset(r, 4 * c, KBp)) = h;
                }
            }
        }
    }
    // combine the two row slots through LDS, one partial row per workgroup and kind
    float4* s4 = reinterpret_cast<float4*>(sm);
#pragma unroll
    for (int which = 0; which < (PACK ? 3 : 2); ++which) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NVH; ++i) {
            const int c = c0 + 64 * i;
            if (c < nv4) s4[slot * nv4 + c] = which == 0 ? ag[i] : which == 1 ? ab[i] : ad[PACK ? i : 0];
        }
        __syncthreads();
        for (int cc = threadIdx.x; cc < nv4; cc += NT) {
            const float4 t = s4[cc], u = s4[nv4 + cc];
            reinterpret_cast<float4*>(partial + ((size_t)which * gridDim.x + blockIdx.x) * d)[cc] =
                make_float4(t.x + u.x, t.y + u.y, t.z + u.z, t.w + u.w);
        }
    }
}

// ---- bf16 activation stream (round 5; --dtype bf16 with bf16 activations).  Between the CLS concat and the last full layer's
// LayerNorm no f32 activation exists: the residual sums leave the GEMM epilogues as lstc_pack1 operands (LSTC_EPI_OUT_PACK +
// LSTC_EPI_RESIDUAL_PACK), the LayerNorm reads that pack and writes the pack the next block consumes (A operand AND residual),
// and the gradient of the residual stream travels the same way.  A lane owns 16-B chunks (8 consecutive columns) of its row:
// chunk c8 of row r is one 16-B access at p1_offset(r, 8 c8, KBp); 4 lanes cover a tile row's 64 contiguous bytes.
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));

// One wave per row, NC = d / 512 chunks per lane.  XP: x is a pack (else f32 [rows, d]); YF / YP: write y as f32 / as a pack.
// (Measured and not kept: the next row's chunks prefetched before the current row is reduced - with gamma / beta in registers
// that is 174 VGPRs = 2 waves per SIMD; with gamma / beta in LDS 124 VGPRs = 4 waves, and 221 us instead of 173 us per 100352 x
// 2048 launch: the reduction waits on the LDS reads.  The plain form below is the fastest of the three.)
template <int NC, bool XP, bool YF, bool YP>
__global__ void __launch_bounds__(NT) ln_fwd_act(const float* __restrict__ x, const __bf16* __restrict__ xp,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ y, __bf16* __restrict__ yp, float* __restrict__ mean,
                                                  float* __restrict__ rstd, int64_t rows, int d, float eps, int KBp) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (NT / 64);
    float g[NC][8], b[NC][8];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c0 = 8 * (lane + 64 * i);
        const float4 g0 = *reinterpret_cast<const float4*>(gamma + c0), g1 = *reinterpret_cast<const float4*>(gamma + c0 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(beta + c0), b1 = *reinterpret_cast<const float4*>(beta + c0 + 4);
        g[i][0] = g0.x; g[i][1] = g0.y; g[i][2] = g0.z; g[i][3] = g0.w; g[i][4] = g1.x; g[i][5] = g1.y; g[i][6] = g1.z; g[i][7] = g1.w;
        b[i][0] = b0.x; b[i][1] = b0.y; b[i][2] = b0.z; b[i][3] = b0.w; b[i][4] = b1.x; b[i][5] = b1.y; b[i][6] = b1.z; b[i][7] = b1.w;
    }
    for (int64_t r = wave0; r < rows; r += nwaves) {
        float v[NC][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c0 = 8 * (lane + 64 * i);
            if constexpr (XP) {
                const bf16x8v h = *reinterpret_cast<const bf16x8v*>(xp + p1_offset(r, c0, KBp));
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = (float)h[j];
            } else {
                const float4 a0 = *reinterpret_cast<const float4*>(x + r * d + c0), a1 = *reinterpret_cast<const float4*>(x + r * d + c0 + 4);
                v[i][0] = a0.x; v[i][1] = a0.y; v[i][2] = a0.z; v[i][3] = a0.w; v[i][4] = a1.x; v[i][5] = a1.y; v[i][6] = a1.z; v[i][7] = a1.w;
            }
            s += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
        }
        const float mu = wave_sum(s) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float a = v[i][j] - mu; q += a * a; }
        const float rs = 1.f / sqrtf(wave_sum(q) / (float)d + eps);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c0 = 8 * (lane + 64 * i);
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mu) * rs * g[i][j] + b[i][j];
            if constexpr (YF) {
                *reinterpret_cast<float4*>(y + r * d + c0) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(y + r * d + c0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
            }
            if constexpr (YP) {
                bf16x8v h;
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = (__bf16)o[j];
                *reinterpret_cast<bf16x8v*>(yp + p1_offset(r, c0, KBp)) = h;
            }
        }
        if (lane == 0) {
            mean[r] = mu;
            rstd[r] = rs;
        }
    }
}

// Backward of z = LayerNorm(dropout(f) + x) on packs: two waves per row (NCH = d / 1024 chunks per lane each), the structure of
// ln_bwd_pair.  xp = pack of the pre-LayerNorm sum; the incoming gradient is a pack (DYP) or f32; DX: the gradient of the
// residual sum leaves as a pack (the residual operand of the block's input-gradient GEMM) - not at all when nobody reads it
// (layer 0).  dfp = pack of dropout-replay(dx); partial [3, gridDim.x, d] = dgamma, dbeta, column sums of df.
template <int NCH, bool DYP, bool DX>
__global__ void __launch_bounds__(NT) ln_bwd_act(const float* __restrict__ dy, const __bf16* __restrict__ dyp,
                                                  const __bf16* __restrict__ xp, const float* __restrict__ gamma,
                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  __bf16* __restrict__ dxp, float* __restrict__ partial, int64_t rows, int d,
                                                  __bf16* __restrict__ dfp, int KBp, DropKey key) {
    key = drop_key_now(key);
    extern __shared__ __attribute__((aligned(16))) float sm[];   // [2][d] combine buffer, then [2][4][64][2] per-lane row sums
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, slot = wv >> 1, half = wv & 1;
    const int hc = d >> 4;                                        // 16-B chunks per half row
    float* red = sm + 2 * d;
    float g[NCH][8], ag[NCH][8], ab[NCH][8], ad[NCH][8];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c0 = 8 * (half * hc + lane + 64 * i);
        const float4 g0 = *reinterpret_cast<const float4*>(gamma + c0), g1 = *reinterpret_cast<const float4*>(gamma + c0 + 4);
        g[i][0] = g0.x; g[i][1] = g0.y; g[i][2] = g0.z; g[i][3] = g0.w; g[i][4] = g1.x; g[i][5] = g1.y; g[i][6] = g1.z; g[i][7] = g1.w;
#pragma unroll
        for (int j = 0; j < 8; ++j) ag[i][j] = ab[i][j] = ad[i][j] = 0.f;
    }
    const int64_t stride = (int64_t)gridDim.x * 2;
    const int64_t iters = (rows + stride - 1) / stride;
    // operands of iteration it + 1 are requested before iteration it is reduced (raw bf16: 8 - 16 registers per tensor): twice the
    // bytes in flight per wave.  Rows beyond the end are clamped to row 0 (never used: ``live``).
    bf16x8v xc[NCH], xn[NCH], dc[DYP ? NCH : 1], dn[DYP ? NCH : 1];
    float4 fc[DYP ? 1 : 2 * NCH], fn[DYP ? 1 : 2 * NCH];
    auto fetch = [&](int64_t it, bf16x8v* xo, bf16x8v* dpo, float4* dfo) {
        const int64_t r = it * stride + (int64_t)blockIdx.x * 2 + slot;
        const int64_t rr = r < rows ? r : 0;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c0 = 8 * (half * hc + lane + 64 * i);
            const size_t off = p1_offset(rr, c0, KBp);
            xo[i] = *reinterpret_cast<const bf16x8v*>(xp + off);
            if constexpr (DYP) dpo[i] = *reinterpret_cast<const bf16x8v*>(dyp + off);
            else {
                dfo[2 * i] = *reinterpret_cast<const float4*>(dy + rr * d + c0);
                dfo[2 * i + 1] = *reinterpret_cast<const float4*>(dy + rr * d + c0 + 4);
            }
        }
    };
    if (iters > 0) fetch(0, xc, dc, fc);
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t r = it * stride + (int64_t)blockIdx.x * 2 + slot;
        const bool live = r < rows;
        const int64_t rr = live ? r : 0;
        if (it + 1 < iters) fetch(it + 1, xn, dn, fn);
        const float mu = mean[rr], rs = rstd[rr];
        float xh[NCH][8], gd[NCH][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (live) {
                float dv[8];
                if constexpr (DYP) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) dv[j] = (float)dc[i][j];
                } else {
                    const float4 a0 = fc[2 * i], a1 = fc[2 * i + 1];
                    dv[0] = a0.x; dv[1] = a0.y; dv[2] = a0.z; dv[3] = a0.w; dv[4] = a1.x; dv[5] = a1.y; dv[6] = a1.z; dv[7] = a1.w;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    xh[i][j] = ((float)xc[i][j] - mu) * rs;
                    gd[i][j] = dv[j] * g[i][j];
                    s1 += gd[i][j];
                    s2 += gd[i][j] * xh[i][j];
                    ag[i][j] += dv[j] * xh[i][j];
                    ab[i][j] += dv[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) xh[i][j] = gd[i][j] = 0.f;
            }
        }
        float2* rb = reinterpret_cast<float2*>(red) + (it & 1) * 256;
        rb[wv * 64 + lane] = make_float2(s1, s2);
        __syncthreads();
        const float2 pa = rb[(slot * 2) * 64 + lane], pb = rb[(slot * 2 + 1) * 64 + lane];
        const float m1 = wave_sum(pa.x + pb.x) / (float)d, m2 = wave_sum(pa.y + pb.y) / (float)d;
        if (live) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c0 = 8 * (half * hc + lane + 64 * i);
                const uint32_t fi = (uint32_t)(r * d) + (uint32_t)c0;
                bf16x8v ho, hf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float ov = rs * (gd[i][j] - m1 - xh[i][j] * m2);
                    const float f = drop_keep(fi + j, key) ? ov * key.scale : 0.f;
                    ad[i][j] += f;
                    ho[j] = (__bf16)ov;
                    hf[j] = (__bf16)f;
                }
                const size_t off = p1_offset(r, c0, KBp);
                if constexpr (DX) *reinterpret_cast<bf16x8v*>(dxp + off) = ho;
                *reinterpret_cast<bf16x8v*>(dfp + off) = hf;
            }
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            xc[i] = xn[i];
            if constexpr (DYP) dc[i] = dn[i];
            else { fc[2 * i] = fn[2 * i]; fc[2 * i + 1] = fn[2 * i + 1]; }
        }
    }
    // combine the two row slots through LDS, one partial row per workgroup and kind
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c0 = 8 * (half * hc + lane + 64 * i);
            float* dst = sm + slot * d + c0;
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[j] = which == 0 ? ag[i][j] : which == 1 ? ab[i][j] : ad[i][j];
        }
        __syncthreads();
        for (int cc = threadIdx.x; cc < (d >> 2); cc += NT) {
            const float4 t = reinterpret_cast<const float4*>(sm)[cc], u = reinterpret_cast<const float4*>(sm)[(d >> 2) + cc];
            reinterpret_cast<float4*>(partial + ((size_t)which * gridDim.x + blockIdx.x) * d)[cc] =
                make_float4(t.x + u.x, t.y + u.y, t.z + u.z, t.w + u.w);
        }
    }
}

__global__ void __launch_bounds__(NT) ln_bwd_generic(const float* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, float* __restrict__ dx,
                                                      float* __restrict__ partial, int64_t rows, int d) {
    // one workgroup = one partial row; each wave walks rows, threads accumulate columns in LDS-free fashion
    extern __shared__ __attribute__((aligned(16))) float sm[];   // [2][d] accumulated with LDS atomics
    for (int c = threadIdx.x; c < 2 * d; c += NT) sm[c] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (NT / 64);
    for (int64_t r = wave0; r < rows; r += nwaves) {
        const float mu = mean[r], rs = rstd[r];
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float xh = (x[r * d + c] - mu) * rs, gd = dy[r * d + c] * gamma[c];
            s1 += gd;
            s2 += gd * xh;
        }
        const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
        for (int c = lane; c < d; c += 64) {
            const float xh = (x[r * d + c] - mu) * rs, dv = dy[r * d + c];
            dx[r * d + c] = rs * (dv * gamma[c] - m1 - xh * m2);
            atomicAdd(&sm[c], dv * xh);
            atomicAdd(&sm[d + c], dv);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * d; c += NT) {
        const int which = c / d, cc = c % d;
        partial[((size_t)which * gridDim.x + blockIdx.x) * d + cc] = sm[c];
    }
}

// ------------------------------------------------------------------------------ column sums of a packed bf16 operand
// partial[rg][k] = sum over the rows of row-block group rg of the lstc_pack1 operand [rows, K] (bf16 -> f32 adds): the bias
// gradient of a Linear whose output gradient exists only in packed form (LSTC_EPI_OUT_PACK).  One workgroup per 32-k tile and
// row-block group; a thread owns one 16-B chunk (8 k) of rows r and r + 64 of every tile of its group.
__global__ void __launch_bounds__(NT) colsum_pack1_kernel(const __bf16* __restrict__ pk, int RB, int KBp, int K,
                                                           float* __restrict__ partial) {
    __shared__ float red[64][33];
    const int kb = blockIdx.x, rg = blockIdx.y, ngrp = gridDim.y;
    const int per = (RB + ngrp - 1) / ngrp, rb0 = rg * per, rb1 = min(RB, rb0 + per);
    const int r = threadIdx.x >> 2, c = threadIdx.x & 3;             // row (and row + 64), LOGICAL chunk
    typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int rb = rb0; rb < rb1; ++rb) {
        const bf16x8v* t = reinterpret_cast<const bf16x8v*>(pk + ((size_t)rb * KBp + kb) * 4096);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int rr = r + 64 * hh;
            const bf16x8v v = t[rr * 4 + (c ^ ((rr >> 2) & 3))];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[r][c * 8 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 32) {
        float s = 0.f;
        for (int i = 0; i < 64; ++i) s += red[i][threadIdx.x];
        const int k = kb * 32 + threadIdx.x;
        if (k < K) partial[(size_t)rg * K + k] = s;
    }
}

// ------------------------------------------------------------------------------ CLS concat
// y = [CLS row, the sequence's tokens]: CLS = `cls` or the mean of the tokens, `pos` added on every row written.  One kernel text each
// for the forward, the input gradient and the token-row gradient; the template arguments choose
//   V        the access pattern: 4-B (float) or 16-B (float4: d % 4 == 0, aligned operands); `dv` counts V's per row.  A column's
//            arithmetic is a sequential walk over the tokens in both, so the two give the same bits (at the headline batch in bf16
//            mode the 4-B loads and 2-B pack stores took 569 us, 2.0 GB moved: 3.6 TB/s);
//   LAY      where the sequences lie (concat_seq), its arguments in a ConcatArg<LAY> by value, so that an instantiation holds no
//            trace of the other layouts:
//     CONCAT_FIXED  x [N, S-1, d] -> y [N, S, d].  Sequences [0, n_lo) come from x and [n_lo, N) from x_hi when that is set: the
//                   reference's cat([normal, abnormal]) fused away.  `packed` (bf16 mode: layer 0's packed A operand, lstc_pack1 of
//                   [N*S, d]) is written next to y, or alone (y null: the bf16 activation stream).
//                   GATHER (round 5): `clip_idx` makes x a feature BANK [clips, P, d] and token t of sequence n the patch t % P of
//                   clip clip_idx[n * (S - 1) / P + t / P] - the batch formation (lstc_gather_rows: 805 MB written and read again at
//                   the headline shape) is fused into this pass.  The index of a token is wave-uniform (one sequence per
//                   workgroup): a scalar load, which the compiler issues only for a pointer it knows the stores to y cannot
//                   reach - a __restrict__ kernel parameter, not a member of the by-value struct (as a member the loads went
//                   through the vector path and the headline gather took 363 us instead of 337).
//     CONCAT_LEN    the same padded shapes, sequence n has lens[n] real tokens (clamped to [1, S-1]); the rest of its row of x is
//                   padding that is never read, and its rows of y / dx behind the tokens are written as exact zeros.
//     CONCAT_VAR    unpadded in and out: sequence n owns rows row0[n] .. row0[n + 1] - 1 of y [M, d] (CLS first) and, having one
//                   token fewer, rows row0[n] - n .. of x [M - N, d].  A sequence's bits depend neither on the path nor on its
//                   neighbours.
//                   GATHER (spans): x is a BANK of rows [bank_rows, d] and the tokens of sequence n are its rows clip_idx[n] ..
//                   clip_idx[n] + L_n - 1 (here the table holds one first ROW per sequence): spans may overlap, repeat and lie in
//                   any order, y keeps the unpadded layout.  Only where x0 comes from differs, so the bits are those of the packed
//                   input; the table is the same __restrict__ parameter, read with scalar loads.
enum ConcatLayout { CONCAT_FIXED, CONCAT_LEN, CONCAT_VAR };
struct ConcatFixed {
    const void* x_hi;
    int64_t n_lo;
    __bf16* packed;
    int KBp;
    int P;
};
struct ConcatLen { const int32_t* lens; };
struct ConcatVar { const int32_t* row0; };
template <int LAY>
using ConcatArg = std::conditional_t<LAY == CONCAT_FIXED, ConcatFixed, std::conditional_t<LAY == CONCAT_LEN, ConcatLen, ConcatVar>>;

__device__ inline int concat_len(const int32_t* __restrict__ lens, int64_t n, int S) { return min(max((int)lens[n], 1), S - 1); }

// Sequence n: its first row of y (the CLS row) and of x, its token count L, the divisor of its mean (L; an empty unpadded
// sequence divides by 1), and whether its rows behind the tokens, up to S - 1, are written as zeros.
struct ConcatSeq {
    int64_t y0, x0;
    int L, div;
    bool tail;
};
template <int LAY, bool GATHER = false>
__device__ inline ConcatSeq concat_seq(const ConcatArg<LAY>& a, int64_t n, int S, const int64_t* __restrict__ src0 = nullptr) {
    if constexpr (LAY == CONCAT_VAR) {
        const int64_t b = a.row0[n];
        const int L = (int)(a.row0[n + 1] - b) - 1;
        int64_t x0 = b - n;
        if constexpr (GATHER) x0 = src0[n];        // a span of bank rows
        return {b, x0, L, max(L, 1), false};
    } else {
        int L = S - 1;
        if constexpr (LAY == CONCAT_LEN) L = concat_len(a.lens, n, S);
        return {n * S, n * (int64_t)(S - 1), L, L, LAY == CONCAT_LEN};
    }
}

__device__ inline float vzero(float) { return 0.f; }
__device__ inline float4 vzero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ inline float vadd(float a, float b) { return a + b; }
__device__ inline float4 vadd(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float vdiv(float a, float r) { return a / r; }
__device__ inline float4 vdiv(const float4& a, float r) { return make_float4(a.x / r, a.y / r, a.z / r, a.w / r); }
// element c (in V's) of row `row` of the pack: a 2-B store, or the 8 B of four columns
__device__ inline void pack_put(__bf16* packed, int64_t row, int c, int KBp, float w) { packed[p1_offset(row, c, KBp)] = (__bf16)w; }
__device__ inline void pack_put(__bf16* packed, int64_t row, int c, int KBp, const float4& w) {
    bf16x4v h;
    h[0] = (__bf16)w.x; h[1] = (__bf16)w.y; h[2] = (__bf16)w.z; h[3] = (__bf16)w.w;
    *reinterpret_cast<bf16x4v*>(packed + p1_offset(row, 4 * c, KBp)) = h;
}

// grid (N, ceil(dv/NT)); a thread owns one V of columns (coalesced across the workgroup) and walks the tokens.
// y[0] = cls or mean(x[:L]); y[1+t] = x[t] for t < L; pos on rows 0..L.
template <typename V, int LAY, bool GATHER = false>
__global__ void __launch_bounds__(NT) cls_concat_fwd_kernel(const V* __restrict__ x, ConcatArg<LAY> a, const V* __restrict__ cls,
                                                             const V* __restrict__ pos, V* __restrict__ y, int S, int dv,
                                                             const int64_t* __restrict__ clip_idx) {
    const int64_t n = blockIdx.x;
    const int c = blockIdx.y * NT + threadIdx.x;
    if (c >= dv) return;
    const ConcatSeq q = concat_seq<LAY, GATHER>(a, n, S, clip_idx);
    const V* xr = x + q.x0 * dv + c;
    const int64_t* ci = nullptr;
    if constexpr (LAY == CONCAT_FIXED) {
        if (a.x_hi && n >= a.n_lo) xr = (const V*)a.x_hi + (n - a.n_lo) * (int64_t)(S - 1) * dv + c;
        if constexpr (GATHER) ci = clip_idx + n * (int64_t)((S - 1) / a.P);
    }
    V* yr = LAY != CONCAT_FIXED || y ? y + q.y0 * dv + c : nullptr;       // NULL: pack only
    auto put = [&](int t, const V& w) {        // row t of the sequence
        if constexpr (LAY == CONCAT_FIXED) {
            if (yr) yr[(int64_t)t * dv] = w;
            if (a.packed) pack_put(a.packed, q.y0 + t, c, a.KBp, w);
        } else {
            yr[(int64_t)t * dv] = w;
        }
    };
    V s = vzero(V{});
    // 8 loads in flight per thread: 4 -> 8 took the kernel 319 -> 286 us (f32 only), 480 -> 395 us (with the pack); 16: 303 / 387
#pragma unroll 8
    for (int t = 0; t < q.L; ++t) {
        V v;
        if constexpr (GATHER && LAY == CONCAT_FIXED) v = x[(ci[t / a.P] * a.P + t % a.P) * (int64_t)dv + c];
        else v = xr[(int64_t)t * dv];
        s = vadd(s, v);
        put(t + 1, pos ? vadd(v, pos[(int64_t)(t + 1) * dv + c]) : v);
    }
    if (q.tail)
        for (int t = q.L; t < S - 1; ++t) put(t + 1, vzero(V{}));
    V cv = cls ? cls[c] : vdiv(s, (float)q.div);
    if (pos) cv = vadd(cv, pos[c]);
    put(0, cv);
}

// dx[t] = dy[1+t] + (mean_cls ? dy[0] / L : 0) for t < L.  Same grid.
template <typename V, int LAY>
__global__ void __launch_bounds__(NT) cls_concat_bwd_kernel(const V* __restrict__ dy, ConcatArg<LAY> a, V* __restrict__ dx, int S, int dv,
                                                             int mean_cls) {
    const int64_t n = blockIdx.x;
    const int c = blockIdx.y * NT + threadIdx.x;
    if (c >= dv) return;
    const ConcatSeq q = concat_seq<LAY>(a, n, S);
    const V* dr = dy + q.y0 * dv + c;
    V* xr = dx + q.x0 * dv + c;
    const V g0 = mean_cls ? vdiv(dr[0], (float)q.div) : vzero(V{});
#pragma unroll 8
    for (int t = 0; t < q.L; ++t) xr[(int64_t)t * dv] = vadd(dr[(int64_t)(t + 1) * dv], g0);
    if (q.tail)
        for (int t = q.L; t < S - 1; ++t) xr[(int64_t)t * dv] = vzero(V{});
}

// dtok[t, :] = sum over the sequences that have row t (t <= L_n) of their dy[t, :]: the gradient of a learned CLS token (row 0) and
// of the position table.  grid (rows of dtok, ceil(dv/NT)); the sequences are walked in order, so the sum is deterministic.  (The
// fixed layout's sums are column sums of dy viewed [N, S * d]: lstc_colsum, another order.)
template <typename V, int LAY>
__global__ void __launch_bounds__(NT) cls_concat_dtok_kernel(const V* __restrict__ dy, ConcatArg<LAY> a, V* __restrict__ dtok, int64_t N,
                                                              int S, int dv) {
    const int t = blockIdx.x;
    const int c = blockIdx.y * NT + threadIdx.x;
    if (c >= dv) return;
    V s = vzero(V{});
    for (int64_t n = 0; n < N; ++n) {
        const ConcatSeq q = concat_seq<LAY>(a, n, S);
        if (t <= q.L) s = vadd(s, dy[(q.y0 + t) * dv + c]);
    }
    dtok[(int64_t)t * dv + c] = s;
}

// ---- CLS concat: every launch goes through concat_launch
// 16-B accesses are possible: d % 4 == 0 and every operand 16-B aligned (a null operand counts as aligned)
static bool concat_vec16(int32_t d, std::initializer_list<const void*> ops) {
    bool ok = d % 4 == 0;
    for (const void* p : ops) ok = ok && aligned16(p);
    return ok;
}

// Chooses the access type V (float4 where concat_vec16 allows, float otherwise), counts the V's of a row and sizes the grid
// (`rows` x column groups), then calls go(V{}, grid, dv), which launches that instantiation.
template <typename Go>
static void concat_launch(int32_t d, std::initializer_list<const void*> ops, int64_t rows, Go go) {
    const bool v4 = concat_vec16(d, ops);
    const int dv = v4 ? d / 4 : d;
    const dim3 grid((unsigned)rows, (unsigned)((dv + NT - 1) / NT));
    if (v4) go(float4{}, grid, dv);
    else go(float{}, grid, dv);
}

template <int LAY, bool GATHER = false>
static void concat_fwd(const float* x, const ConcatArg<LAY>& a, const float* cls, const float* pos, float* y, int64_t N, int32_t S,
                       int32_t d, hipStream_t st, const int64_t* clip_idx = nullptr) {
    const void* x_hi = nullptr;
    if constexpr (LAY == CONCAT_FIXED) x_hi = a.x_hi;
    concat_launch(d, {x, x_hi, y, cls, pos}, N, [&](auto v, dim3 grid, int dv) {
        using V = decltype(v);
        // the fixed layout's gather exists on the 16-B path (its entry point refuses the rest); the spans on both
        if constexpr (!GATHER || LAY == CONCAT_VAR || std::is_same_v<V, float4>)
            hipLaunchKernelGGL((cls_concat_fwd_kernel<V, LAY, GATHER>), grid, NT, 0, st, (const V*)x, a, (const V*)cls, (const V*)pos,
                               (V*)y, S, dv, clip_idx);
    });
}

// dx (N sequences) and / or dtok (`tok_rows` rows; the len and var layouts only), each may be null
template <int LAY>
static void concat_bwd(const float* dy, const ConcatArg<LAY>& a, float* dx, float* dtok, int64_t N, int32_t tok_rows, int32_t S, int32_t d,
                       int32_t mean_cls, hipStream_t st) {
    if (dx)
        concat_launch(d, {dy, dx, dtok}, N, [&](auto v, dim3 grid, int dv) {
            using V = decltype(v);
            hipLaunchKernelGGL((cls_concat_bwd_kernel<V, LAY>), grid, NT, 0, st, (const V*)dy, a, (V*)dx, S, dv, mean_cls);
        });
    if constexpr (LAY != CONCAT_FIXED)
        if (dtok)
            concat_launch(d, {dy, dx, dtok}, tok_rows, [&](auto v, dim3 grid, int dv) {
                using V = decltype(v);
                hipLaunchKernelGGL((cls_concat_dtok_kernel<V, LAY>), grid, NT, 0, st, (const V*)dy, a, (V*)dtok, N, S, dv);
            });
}

// ---------------------------------------------------------------------------------- colsum
// pass 1: grid (ceil(cols/NT), n_partial): workgroup y sums rows y, y+n_partial, ... of NT columns.
// (blockIdx.z = plane of a batched call, lstc_colsum_batched: planes are `xstride` / n_partial * cols floats apart)
__global__ void __launch_bounds__(NT) colsum_pass1(const float* __restrict__ x, int64_t rows, int cols, int ld,
                                                    float* __restrict__ partial, int64_t xstride = 0) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= cols) return;
    x += (size_t)blockIdx.z * xstride;
    partial += (size_t)blockIdx.z * gridDim.y * cols;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const int64_t step = gridDim.y;
    int64_t r = blockIdx.y;
    for (; r + 3 * step < rows; r += 4 * step) {
        s0 += x[r * ld + c];
        s1 += x[(r + step) * ld + c];
        s2 += x[(r + 2 * step) * ld + c];
        s3 += x[(r + 3 * step) * ld + c];
    }
    for (; r < rows; r += step) s0 += x[r * ld + c];
    partial[(size_t)blockIdx.y * cols + c] = (s0 + s1) + (s2 + s3);
}
// pass 2: 64 threads per column group of 64 columns x 4 partial-row lanes; each thread sums every 4th partial row with
// 4 independent accumulators (the loop is latency-bound, not bandwidth-bound), then the 4 lanes combine through LDS.
__global__ void __launch_bounds__(NT) colsum_pass2(const float* __restrict__ partial, int n_partial, int cols,
                                                    float* __restrict__ out, int accumulate) {
    __shared__ float red[NT];
    partial += (size_t)blockIdx.y * n_partial * cols;          // blockIdx.y = plane of a batched call (0 otherwise)
    out += (size_t)blockIdx.y * cols;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int lane_p = threadIdx.x >> 6;                 // 0..3
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < cols) {
        int p = lane_p;
        for (; p + 12 < n_partial; p += 16) {
            s0 += partial[(size_t)p * cols + c];
            s1 += partial[(size_t)(p + 4) * cols + c];
            s2 += partial[(size_t)(p + 8) * cols + c];
            s3 += partial[(size_t)(p + 12) * cols + c];
        }
        for (; p < n_partial; p += 4) s0 += partial[(size_t)p * cols + c];
    }
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (lane_p == 0 && c < cols) {
        const float s = (red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
        out[c] = accumulate ? out[c] + s : s;
    }
}

// A few rows (the partial products of a split-K weight gradient: 2-8 rows of out*in columns): ONE pass, float4 columns, the
// summation order of pass 1 + pass 2 on the same input (row p goes to accumulator p & 3 in increasing p, then (a0 + a1) +
// (a2 + a3)), so the result is bit-identical to the two-pass form - which copied the rows once before adding them.
__global__ void __launch_bounds__(NT) colsum_few(const float* __restrict__ x, int rows, int cols, int ld, float* __restrict__ out,
                                                  int accumulate) {
    const int c4 = (blockIdx.x * NT + threadIdx.x) * 4;
    if (c4 >= cols) return;
    float4 a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r0 = 0; r0 < rows; r0 += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (r0 + j < rows) {
                const float4 v = *reinterpret_cast<const float4*>(x + (size_t)(r0 + j) * ld + c4);
                a[j].x += v.x; a[j].y += v.y; a[j].z += v.z; a[j].w += v.w;
            }
    }
    float4 s;
    s.x = (a[0].x + a[1].x) + (a[2].x + a[3].x);
    s.y = (a[0].y + a[1].y) + (a[2].y + a[3].y);
    s.z = (a[0].z + a[1].z) + (a[2].z + a[3].z);
    s.w = (a[0].w + a[1].w) + (a[2].w + a[3].w);
    float4* o = reinterpret_cast<float4*>(out + c4);
    if (accumulate) { const float4 q = *o; s.x = q.x + s.x; s.y = q.y + s.y; s.z = q.z + s.z; s.w = q.w + s.w; }
    *o = s;
}

// C = epi(parts[0] + parts[1] + ... + parts[s - 1]) with the epilogue of lstc_gemm (csrc/gemm_f32.hip: bias, ReLU, dropout of the flat
// index row * N + col, residual, ReLU mask, accumulate - in that order); the K chunks of a small product arrive as separate partial
// results and are added in chunk order (no atomics).  One thread per four columns.
// `groups` > 1 (per-head products): group g's partials start at parts + g * group_stride_parts, its [M, N] result at C + g * group_stride_c.
__global__ void __launch_bounds__(NT) splitk_finish_kernel(const float* __restrict__ parts, int s, int64_t part_stride, int M, int N,
                                                            const float* __restrict__ bias, const float* __restrict__ res, int64_t ldr,
                                                            const float* __restrict__ relu_src, int64_t ld_relu, float* __restrict__ C,
                                                            int64_t ldc, int flags, DropKey dk, int groups, int64_t group_stride_parts,
                                                            int64_t group_stride_c) {
    dk = drop_key_now(dk);
    const int n4 = N >> 2;
    const int64_t per_group = (int64_t)M * n4, total = per_group * groups;
    for (int64_t q0 = (int64_t)blockIdx.x * NT + threadIdx.x; q0 < total; q0 += (int64_t)gridDim.x * NT) {
        const int grp = (int)(q0 / per_group);
        const int64_t q = q0 - (int64_t)grp * per_group;
        const int row = (int)(q / n4), col = 4 * (int)(q - (int64_t)row * n4);
        const float* pp = parts + (int64_t)grp * group_stride_parts + (int64_t)row * N + col;
        float4 v = *reinterpret_cast<const float4*>(pp);
        for (int i = 1; i < s; ++i) {
            const float4 x = *reinterpret_cast<const float4*>(pp + i * part_stride);
            v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
        }
        if (flags & LSTC_EPI_BIAS) {
            const float4 b = *reinterpret_cast<const float4*>(bias + col);
            v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        }
        // the chain behind the head: lstc_common.h (this kernel's head adds its bias under the flag, there is no alpha)
        float4* cp = reinterpret_cast<float4*>(C + (int64_t)grp * group_stride_c + (int64_t)row * ldc + col);
        v = epi_chain4(v, flags, (uint32_t)row * (uint32_t)N + (uint32_t)col, dk,
                       [&] { return *reinterpret_cast<const float4*>(res + (int64_t)row * ldr + col); },
                       [&] { return *reinterpret_cast<const float4*>(relu_src + (int64_t)row * ld_relu + col); }, [&] { return *cp; });
        *cp = v;
    }
}

// out[i, :] = widen(pack row row0 + i * step): n rows of an lstc_pack1 operand back as f32 (one thread per 16-B chunk)
__global__ void __launch_bounds__(NT) unpack1_rows_kernel(const __bf16* __restrict__ pk, int KBp, int64_t row0, int64_t step, int64_t n,
                                                           int K, float* __restrict__ out, int64_t ldo) {
    const int cpr = K >> 3;
    const int64_t total = n * cpr;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < total; q += (int64_t)gridDim.x * NT) {
        const int64_t i = q / cpr;
        const int c = (int)(q - i * cpr);
        const bf16x8v h = *reinterpret_cast<const bf16x8v*>(pk + p1_offset(row0 + i * step, 8 * c, KBp));
        float4* o = reinterpret_cast<float4*>(out + i * ldo + 8 * c);
        o[0] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        o[1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
    }
}

// --------------------------------------------------------------------------------- dropout
__global__ void __launch_bounds__(NT) dropout_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            int64_t n, DropKey k) {
    k = drop_key_now(k);
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride)
        y[i] = drop_keep((uint32_t)i, k) ? x[i] * k.scale : 0.f;
}
// The same on an lstc_pack1 operand [rows, d] (bf16 activation stream: the backward of a block WITHOUT LayerNorm, whose incoming
// gradient pack is the gradient of dropout(f) + x as it stands).  A thread owns one 16-B chunk in STORAGE order (fully coalesced);
// the element's flat index row * d + col - the mask's counter - follows from the chunk's place in its 128-row x 32-k tile.
__global__ void __launch_bounds__(NT) dropout_apply_pack_kernel(const __bf16* __restrict__ x, __bf16* __restrict__ y, int64_t chunks,
                                                                 int KBp, int d, DropKey k) {
    k = drop_key_now(k);
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < chunks; q += stride) {
        const int64_t tile = q >> 9;
        const int rr = (int)(q & 511) >> 2, pc = (int)(q & 3), ch = pc ^ ((rr >> 2) & 3);
        const int64_t row = (tile / KBp) * 128 + rr;
        const int col0 = (int)(tile % KBp) * 32 + ch * 8;
        const uint32_t fi = (uint32_t)(row * d) + (uint32_t)col0;
        const bf16x8v v = reinterpret_cast<const bf16x8v*>(x)[q];
        bf16x8v o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = drop_keep(fi + j, k) ? (__bf16)((float)v[j] * k.scale) : (__bf16)0.f;
        reinterpret_cast<bf16x8v*>(y)[q] = o;
    }
}
__global__ void __launch_bounds__(NT) dropout_mask_kernel(uint8_t* __restrict__ m, int64_t n, DropKey k) {
    k = drop_key_now(k);
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) m[i] = drop_keep((uint32_t)i, k) ? 1 : 0;
}

// ------------------------------------------------------------------------------ head output
// x [rows,32] -> c logits -> sigmoid (c=1) or softmax (c=2); thread per row.
__global__ void __launch_bounds__(NT) head_out_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                           const float* __restrict__ b, float* __restrict__ out,
                                                           int64_t rows, int c) {
    __shared__ float w[2 * 32 + 2];
    if (threadIdx.x < c * 32) w[threadIdx.x] = W[threadIdx.x];
    if (threadIdx.x < c) w[64 + threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= rows) return;
    const float4* xr = reinterpret_cast<const float4*>(x + r * 32);
    float z0 = 0.f, z1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 v = xr[i];
        z0 += v.x * w[4 * i] + v.y * w[4 * i + 1] + v.z * w[4 * i + 2] + v.w * w[4 * i + 3];
        if (c == 2) z1 += v.x * w[32 + 4 * i] + v.y * w[32 + 4 * i + 1] + v.z * w[32 + 4 * i + 2] + v.w * w[32 + 4 * i + 3];
    }
    z0 += w[64];
    if (c == 1) {
        out[r] = 1.f / (1.f + expf(-z0));
    } else {
        z1 += w[65];
        const float m = fmaxf(z0, z1);
        const float e0 = expf(z0 - m), e1 = expf(z1 - m);
        const float inv = 1.f / (e0 + e1);
        out[2 * r] = e0 * inv;
        out[2 * r + 1] = e1 * inv;
    }
}

// ONE workgroup walks all rows (a few thousand at most: one row per sequence): every thread keeps its own partial sums of
// dW / db in registers, then wave shuffles and a wave-ordered LDS sum - a fixed summation order, no atomics.
__global__ void __launch_bounds__(NT) head_out_bwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                           const float* __restrict__ out, const float* __restrict__ dout,
                                                           float* __restrict__ dx, float* __restrict__ dW,
                                                           float* __restrict__ db, int64_t rows, int c) {
    __shared__ float w[64];
    __shared__ float accw[NT / 64][2 * 32 + 2];
    if (threadIdx.x < c * 32) w[threadIdx.x] = W[threadIdx.x];
    __syncthreads();
    float a0[32], a1[32], b0 = 0.f, b1 = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) a0[i] = a1[i] = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += NT) {
        float dz0, dz1 = 0.f;
        if (c == 1) {
            const float o = out[r];
            dz0 = dout[r] * o * (1.f - o);
        } else {
            const float o0 = out[2 * r], o1 = out[2 * r + 1], g0 = dout[2 * r], g1 = dout[2 * r + 1];
            const float dot = g0 * o0 + g1 * o1;
            dz0 = o0 * (g0 - dot);
            dz1 = o1 * (g1 - dot);
        }
        const float4* xr = reinterpret_cast<const float4*>(x + r * 32);
        float4* dr = reinterpret_cast<float4*>(dx + r * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 v = xr[i];
            float4 d4;
            d4.x = dz0 * w[4 * i] + (c == 2 ? dz1 * w[32 + 4 * i] : 0.f);
            d4.y = dz0 * w[4 * i + 1] + (c == 2 ? dz1 * w[32 + 4 * i + 1] : 0.f);
            d4.z = dz0 * w[4 * i + 2] + (c == 2 ? dz1 * w[32 + 4 * i + 2] : 0.f);
            d4.w = dz0 * w[4 * i + 3] + (c == 2 ? dz1 * w[32 + 4 * i + 3] : 0.f);
            dr[i] = d4;
            a0[4 * i] += dz0 * v.x; a0[4 * i + 1] += dz0 * v.y; a0[4 * i + 2] += dz0 * v.z; a0[4 * i + 3] += dz0 * v.w;
            a1[4 * i] += dz1 * v.x; a1[4 * i + 1] += dz1 * v.y; a1[4 * i + 2] += dz1 * v.z; a1[4 * i + 3] += dz1 * v.w;
        }
        b0 += dz0; b1 += dz1;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float s0 = wave_sum(a0[i]), s1 = wave_sum(a1[i]);
        if (lane == 0) { accw[wave][i] = s0; accw[wave][32 + i] = s1; }
    }
    {
        const float s0 = wave_sum(b0), s1 = wave_sum(b1);
        if (lane == 0) { accw[wave][64] = s0; accw[wave][65] = s1; }
    }
    __syncthreads();
    if (threadIdx.x < 66) {
        float v = accw[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < NT / 64; ++q) v += accw[q][threadIdx.x];
        if (threadIdx.x < c * 32) dW[threadIdx.x] = v;             // written, not added to: one workgroup holds the whole sum
        else if (threadIdx.x >= 64 && threadIdx.x - 64 < c) db[threadIdx.x - 64] = v;
    }
}

// --------------------------------------------------------------------------------- Adagrad
__global__ void __launch_bounds__(NT) adagrad_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                      float* __restrict__ s, int64_t n, float lr, float wd, float eps,
                                                      float gscale) {
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t n4 = n >> 2;
    const bool vec = aligned16(w) && aligned16(g) && aligned16(s);
    int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (vec) {
        for (; i < n4; i += stride) {
            float4 wv = reinterpret_cast<float4*>(w)[i], sv = reinterpret_cast<float4*>(s)[i];
            const float4 gv = reinterpret_cast<const float4*>(g)[i];
            float gg;
            gg = gv.x * gscale + wd * wv.x; sv.x += gg * gg; wv.x -= lr * gg / (sqrtf(sv.x) + eps);
            gg = gv.y * gscale + wd * wv.y; sv.y += gg * gg; wv.y -= lr * gg / (sqrtf(sv.y) + eps);
            gg = gv.z * gscale + wd * wv.z; sv.z += gg * gg; wv.z -= lr * gg / (sqrtf(sv.z) + eps);
            gg = gv.w * gscale + wd * wv.w; sv.w += gg * gg; wv.w -= lr * gg / (sqrtf(sv.w) + eps);
            reinterpret_cast<float4*>(w)[i] = wv;
            reinterpret_cast<float4*>(s)[i] = sv;
        }
        i = n4 * 4 + (int64_t)blockIdx.x * NT + threadIdx.x;
    }
    for (; i < n; i += stride) {
        const float gg = g[i] * gscale + wd * w[i];
        const float sv = s[i] + gg * gg;
        s[i] = sv;
        w[i] -= lr * gg / (sqrtf(sv) + eps);
    }
}

// All parameters of an optimizer step in ONE launch: up to ADA_MAX tensors ride in the kernel arguments (no device-side table,
// no host-to-device copy); a workgroup finds its tensor by scanning the prefix of workgroup counts and then runs the optimizer's
// element update on its ADA_PER_WG slice.  The scan, the slicing and the float4 / scalar loops are stated ONCE
// (multi_tensor_update) for every optimizer; an optimizer is an Op: its per-workgroup scalars and ``elem``, the update of one
// element.  Adagrad's elem is adagrad_kernel's arithmetic in adagrad_kernel's order: results are bit-identical.
constexpr int ADA_MAX = 48;
constexpr int ADA_PER_WG = NT * 4 * 8;        // elements per workgroup: 8 float4 per thread
template <int NS> struct MultiBatch {         // NS state tensors beside the weight and the gradient
    float* w[ADA_MAX];
    const float* g[ADA_MAX];
    float* s[NS][ADA_MAX];
    long long n[ADA_MAX];
    int first_wg[ADA_MAX + 1];
    int count;
};
template <> struct MultiBatch<0> {            // no state: the Op updates `w` from `g` alone
    float* w[ADA_MAX];
    const float* g[ADA_MAX];
    long long n[ADA_MAX];
    int first_wg[ADA_MAX + 1];
    int count;
};
struct AdaBatch : MultiBatch<1> {
    float lr[ADA_MAX], wd[ADA_MAX], eps[ADA_MAX], gscale[ADA_MAX];
};
struct AdagradOp {
    static constexpr int NS = 1;
    static constexpr bool HAS_G = true;
    float lr, wd, eps, gscale;
    __device__ AdagradOp(const AdaBatch& b, int t) : lr(b.lr[t]), wd(b.wd[t]), eps(b.eps[t]), gscale(b.gscale[t]) {}
    __device__ __forceinline__ void elem(float& w, float g, float& s, float&) const {
        const float gg = g * gscale + wd * w;
        s += gg * gg;
        w -= lr * gg / (sqrtf(s) + eps);
    }
};
// lstc_adagrad_multi_scaled: Adagrad under a learning-rate schedule.  Per workgroup lr_t = (float)((double)lr * (double)*lr_scale),
// Adam's widening, from ONE device float that every launch of a split list reads; the element is AdagradOp's with lr_t for lr,
// so *lr_scale == 1.0f gives lstc_adagrad_multi's bits.
struct AdaScaledBatch : AdaBatch {
    const float* lr_scale;
};
static_assert(sizeof(AdaScaledBatch) <= 4096, "the items must fit the kernel-argument segment");
struct AdagradScaledOp : AdagradOp {
    __device__ AdagradScaledOp(const AdaScaledBatch& b, int t) : AdagradOp(b, t) {
        const float* __restrict__ scale = b.lr_scale;                        // uniform address: one scalar load per workgroup
        lr = (float)((double)lr * (double)*scale);
    }
};

// Adam / AdamW (lstc_adam_multi, include/lstc_hip.h).  What changes from step to step is read on the device: t from the item's
// step word (adam_tick_kernel has added 1 to it, earlier in stream order), the learning-rate multiplier from *lr_scale.  The
// per-item scalars are formed in float64 from the f32 fields widened and rounded ONCE to f32, per workgroup:
//   omb1 = 1 - b1,  omb2 = 1 - b2,  step = lr_t / (1 - b1^t),  rsb2 = 1 / sqrt(1 - b2^t),  keep = 1 - lr_t wd,  lr_t = lr *lr_scale
// (b^t by repeated squaring in float64).  The element arithmetic is f32, one rounding per operation, in this order:
//   g = grad * gscale;   decoupled ? w = w * keep : g = g + wd * w;
//   m = m + omb1 * (g - m);   v = b2 * v + omb2 * (g * g);   w = w - (step * m) / (sqrtf(v) * rsb2 + eps)
struct AdamBatch : MultiBatch<2> {
    int* step[ADA_MAX];
    const float* lr_scale[ADA_MAX];
    float lr[ADA_MAX], b1[ADA_MAX], b2[ADA_MAX], eps[ADA_MAX], wd[ADA_MAX], gscale[ADA_MAX];
    unsigned long long decoupled;             // bit i: item i is AdamW
};
static_assert(sizeof(AdamBatch) <= 4096, "the items must fit the kernel-argument segment");
__device__ __forceinline__ double pow_f64(double b, unsigned e) {
    double r = 1.0;
    for (; e; e >>= 1, b *= b)
        if (e & 1u) r *= b;
    return r;
}
struct AdamOp {
    static constexpr int NS = 2;
    static constexpr bool HAS_G = true;
    float omb1, b2, omb2, step, rsb2, eps, wd, gscale, keep;
    bool decoupled;
    __device__ AdamOp(const AdamBatch& b, int i) {
        const int* __restrict__ word = b.step[i];
        const float* __restrict__ scale = b.lr_scale[i];
        const unsigned t = (unsigned)*word;                                  // uniform address: one scalar load per workgroup
        const double lr_t = (double)b.lr[i] * (double)(scale ? *scale : 1.0f);
        const double d1 = (double)b.b1[i], d2 = (double)b.b2[i];
        omb1 = (float)(1.0 - d1);
        omb2 = (float)(1.0 - d2);
        step = (float)(lr_t / (1.0 - pow_f64(d1, t)));
        rsb2 = (float)(1.0 / sqrt(1.0 - pow_f64(d2, t)));
        keep = (float)(1.0 - lr_t * (double)b.wd[i]);
        b2 = b.b2[i]; eps = b.eps[i]; wd = b.wd[i]; gscale = b.gscale[i];
        decoupled = (b.decoupled >> i) & 1ull;
    }
    __device__ __forceinline__ void elem(float& w, float g, float& m, float& v) const {
        float gg = g * gscale;
        if (decoupled) w = w * keep;
        else gg = gg + wd * w;
        m = m + omb1 * (gg - m);
        v = b2 * v + omb2 * (gg * gg);
        w = w - step * m / (sqrtf(v) * rsb2 + eps);
    }
};

// The exponential moving average of a weight (lstc_ema_multi, include/lstc_hip.h): `w` of the shared loops is the average, `g` the
// weight it follows, there is no state tensor.  t is the item's count word (ema_tick_kernel has added 1 to it, earlier in stream
// order).  t == 1 copies the weight's bits; after that a = (float)(1 - decay_t) is formed in float64 per workgroup, with
// decay_t = warmup ? min(decay, (1 + u) / (10 + u)) : decay and u = t - 1, and the element is  avg = avg + a * (w - avg)  in f32.
struct EmaBatch : MultiBatch<0> {
    int* step[ADA_MAX];
    float decay[ADA_MAX];
    unsigned long long warmup;                // bit i: item i ramps its decay up
};
static_assert(sizeof(EmaBatch) <= 4096, "the items must fit the kernel-argument segment");
struct EmaOp {
    static constexpr int NS = 0;
    static constexpr bool HAS_G = true;
    float a;
    bool first;
    __device__ EmaOp(const EmaBatch& b, int i) {
        const int* __restrict__ word = b.step[i];
        const unsigned t = (unsigned)*word;                                  // uniform address: one scalar load per workgroup
        double d = (double)b.decay[i];
        if ((b.warmup >> i) & 1ull) {
            const double u = (double)(t - 1u);
            d = fmin(d, (1.0 + u) / (10.0 + u));
        }
        a = (float)(1.0 - d);
        first = t == 1u;
    }
    __device__ __forceinline__ void elem(float& avg, float w, float&, float&) const { avg = first ? w : avg + a * (w - avg); }
};

// lstc_swap_multi: `w` and the one state tensor trade their bits; no gradient operand.
struct SwapBatch : MultiBatch<1> {};
struct SwapOp {
    static constexpr int NS = 1;
    static constexpr bool HAS_G = false;
    __device__ SwapOp(const SwapBatch&, int) {}
    __device__ __forceinline__ void elem(float& a, float, float& b, float&) const {
        const float x = a;
        a = b;
        b = x;
    }
};

template <int K, int NS> __device__ __forceinline__ float* state_ptr(const MultiBatch<NS>& b, int t) {
    if constexpr (K >= 0 && K < NS) return b.s[K][t];
    else return nullptr;
}
// element i of an operand the Op has, else a stand-in that is never used
template <bool Have, class T> __device__ __forceinline__ T operand(const T* p, int64_t i, const T& absent) {
    if constexpr (Have) return p[i];
    else return absent;
}
template <class Op, class Batch> __device__ __forceinline__ void multi_tensor_update(const Batch& b) {
    constexpr bool one = Op::NS > 0, two = Op::NS > 1, grad = Op::HAS_G;
    int t = 0;
    while (t + 1 < b.count && (int)blockIdx.x >= b.first_wg[t + 1]) ++t;          // wave-uniform scan (scalar loads of the arguments)
    float* __restrict__ w = b.w[t];
    const float* __restrict__ g = b.g[t];
    float* __restrict__ s = state_ptr<0>(b, t);           // nullptr and never touched when Op::NS == 0
    float* __restrict__ s2 = state_ptr<Op::NS - 1>(b, t); // the second state tensor (Op::NS == 2), else `s` again and unused
    const int64_t n = b.n[t];
    const Op op(b, t);
    const int64_t e0 = (int64_t)((int)blockIdx.x - b.first_wg[t]) * ADA_PER_WG;
    const int64_t e1 = min(n, e0 + ADA_PER_WG);
    const bool vec = aligned16(w) && aligned16(g) && aligned16(s) && aligned16(s2);          // an absent operand is nullptr: aligned
    if (vec) {
        const int64_t v1 = e1 == n ? (n >> 2) : (e1 >> 2);
        for (int64_t i = (e0 >> 2) + threadIdx.x; i < v1; i += NT) {
            float4 wv = reinterpret_cast<float4*>(w)[i], sv;
            if constexpr (one) sv = reinterpret_cast<float4*>(s)[i];
            else sv = wv;
            float4 tv = sv;
            if constexpr (two) tv = reinterpret_cast<float4*>(s2)[i];
            const float4 gv = operand<grad>(reinterpret_cast<const float4*>(g), i, wv);
            op.elem(wv.x, gv.x, sv.x, tv.x);
            op.elem(wv.y, gv.y, sv.y, tv.y);
            op.elem(wv.z, gv.z, sv.z, tv.z);
            op.elem(wv.w, gv.w, sv.w, tv.w);
            reinterpret_cast<float4*>(w)[i] = wv;
            if constexpr (one) reinterpret_cast<float4*>(s)[i] = sv;
            if constexpr (two) reinterpret_cast<float4*>(s2)[i] = tv;
        }
        if (e1 != n) return;
    }
    // fully scalar when a pointer is unaligned; else the tensor's last 0-3 elements (its last workgroup only)
    for (int64_t i = (vec ? (n >> 2) * 4 : e0) + threadIdx.x; i < e1; i += NT) {
        float wv = w[i], sv = operand<one>(s, i, wv), tv = sv;
        if constexpr (two) tv = s2[i];
        op.elem(wv, operand<grad>(g, i, wv), sv, tv);
        if constexpr (one) s[i] = sv;
        if constexpr (two) s2[i] = tv;
        w[i] = wv;
    }
}
__global__ void __launch_bounds__(NT) adagrad_multi_kernel(const AdaBatch b) { multi_tensor_update<AdagradOp>(b); }
__global__ void __launch_bounds__(NT) adam_multi_kernel(const AdamBatch b) { multi_tensor_update<AdamOp>(b); }
__global__ void __launch_bounds__(NT) ema_multi_kernel(const EmaBatch b) { multi_tensor_update<EmaOp>(b); }
__global__ void __launch_bounds__(NT) swap_multi_kernel(const SwapBatch b) { multi_tensor_update<SwapOp>(b); }
// t = ++*step of every item of the launch, n == 0 items included; one thread per item, in front of adam_multi_kernel
__global__ void __launch_bounds__(64) adam_tick_kernel(const AdamBatch b) {
    if ((int)threadIdx.x < b.count) *b.step[threadIdx.x] += 1;
}
__global__ void __launch_bounds__(64) ema_tick_kernel(const EmaBatch b) {          // the same, in front of ema_multi_kernel
    if ((int)threadIdx.x < b.count) *b.step[threadIdx.x] += 1;
}
__global__ void __launch_bounds__(NT) adagrad_multi_scaled_kernel(const AdaScaledBatch b) { multi_tensor_update<AdagradScaledOp>(b); }

// lstc_lr_schedule (include/lstc_hip.h states the arithmetic): the learning-rate multiplier of optimizer step t, zero-based, in
// float64 from the f32 fields widened, rounded ONCE to f32.  One thread: t = *step, *scale = f(t), *step = t + 1 (INT32_MAX stays).
// The schedule rides by value; what changes from step to step is the device word, so a captured launch replays as t + 1, t + 2, ...
__device__ __forceinline__ double lr_schedule_f64(const LstcLrSchedule& s, int t) {
    const double W = (double)s.warmup_steps, ws = (double)s.warmup_start, m = (double)s.min_scale;
    if (t < s.warmup_steps) return ws + (1.0 - ws) * (double)t / W;
    const double D = (double)s.total_steps - W;                              // in float64: exact, and no int overflow for a T the kind ignores
    const double u = fmin((double)(t - s.warmup_steps), D);                  // LINEAR / COSINE only: D > 0 there
    switch (s.kind) {
    case LSTC_LR_LINEAR: return 1.0 - (1.0 - m) * u / D;
    case LSTC_LR_COSINE: return m + (1.0 - m) * 0.5 * (1.0 + cos(3.141592653589793 * u / D));
    case LSTC_LR_STEP: return fmax(m, pow_f64((double)s.gamma, (unsigned)((t - s.warmup_steps) / s.step_size)));
    case LSTC_LR_INV_SQRT: {
        const double Wp = fmax(W, 1.0);
        return fmax(m, sqrt(Wp / fmax((double)t, Wp)));
    }
    default: return 1.0;          // LSTC_LR_CONSTANT
    }
}
__global__ void __launch_bounds__(64) lr_schedule_kernel(const LstcLrSchedule s, int* __restrict__ step, float* __restrict__ scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int t = *step;
    *scale = (float)lr_schedule_f64(s, t);
    if (t != 0x7fffffff) *step = t + 1;
}

// The launcher of multi_tensor_update, for every optimizer: 48 items per launch, item i of a launch owning workgroups
// first_wg[i] .. first_wg[i + 1] - 1 (none when n == 0).  `fill` copies one item's fields into slot i, `launch` issues the kernels.
template <class Batch, class Item, class Fill, class Launch>
static int multi_tensor_launch(const Item* items, int32_t count, void* stream, Fill fill, Launch launch) {
    for (int32_t base = 0; base < count; base += ADA_MAX) {
        Batch b;
        b.count = count - base < ADA_MAX ? count - base : ADA_MAX;
        int wg = 0;
        for (int i = 0; i < b.count; ++i) {
            const Item& it = items[base + i];
            fill(b, i, it);
            b.n[i] = it.n;
            b.first_wg[i] = wg;
            const int64_t nwg = (it.n + ADA_PER_WG - 1) / ADA_PER_WG;
            if (nwg > 0x7fffffff - wg) return LSTC_E_RANGE;
            wg += (int)nwg;
        }
        for (int i = b.count; i <= ADA_MAX; ++i) b.first_wg[i] = wg;
        launch(b, wg, (hipStream_t)stream);
        const int rc = lstc_launch_status();
        if (rc) return rc;
    }
    return 0;
}

__global__ void __launch_bounds__(NT) sqnorm_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
    __shared__ float red[NT / 64];
    const int64_t stride = (int64_t)gridDim.x * NT;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) s += x[i] * x[i];
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) atomicAdd(out, s);
}

// clip_grad_norm_ over a parameter LIST in two launches and without a host read-back (the reference: one norm kernel per tensor, a
// stack, a norm of norms and a python comparison, Train/temporal_transformer_shanghaitech.py:139-141).  Items ride in the kernel
// arguments like adagrad_multi_kernel's; workgroup w owns one ADA_PER_WG-element slice of one tensor and writes ONE partial
// (fixed slice -> workgroup map, fixed tree inside the workgroup), a single workgroup then adds the partials in index order:
// the norm is run-to-run bit-identical (no float atomics).
struct VecBatch {
    float* x[ADA_MAX];
    long long n[ADA_MAX];
    int first_wg[ADA_MAX + 1];
    int count;
};
__global__ void __launch_bounds__(NT) sqnorm_multi_kernel(const VecBatch b, float* __restrict__ partials) {
    __shared__ float red[NT / 64];
    int t = 0;
    while (t + 1 < b.count && (int)blockIdx.x >= b.first_wg[t + 1]) ++t;
    const float* __restrict__ x = b.x[t];
    const int64_t n = b.n[t];
    const int64_t e0 = (int64_t)((int)blockIdx.x - b.first_wg[t]) * ADA_PER_WG;
    const int64_t e1 = min(n, e0 + ADA_PER_WG);
    float s = 0.f;
    if (aligned16(x)) {          // e0 is a multiple of 4: float4 over the whole quads, then the tensor's last 0-3 elements
        const int64_t v1 = e1 >> 2;
        for (int64_t i = (e0 >> 2) + threadIdx.x; i < v1; i += NT) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            s += v.x * v.x; s += v.y * v.y; s += v.z * v.z; s += v.w * v.w;
        }
        for (int64_t i = (v1 << 2) + threadIdx.x; i < e1; i += NT) s += x[i] * x[i];
    } else {
        for (int64_t i = e0 + threadIdx.x; i < e1; i += NT) s += x[i] * x[i];
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
__global__ void __launch_bounds__(NT) sum_partials_kernel(const float* __restrict__ partials, int64_t n, float* __restrict__ out) {
    __shared__ float red[NT / 64];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += NT) s += partials[i];
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) { out[0] = s; out[1] = sqrtf(s); }
}
// x *= min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) for every tensor of the list, the coefficient formed on the device
// (torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1); coefficient 1 leaves the data untouched.
// A NaN total norm gives a NaN coefficient, and torch.clamp keeps NaN: every gradient is multiplied by it there - so here too
// (round 5; rounds 1-4 returned early and kept a diverged step's NaN local).
__global__ void __launch_bounds__(NT) clip_scale_multi_kernel(const VecBatch b, const float* __restrict__ sqnorm, float max_norm) {
    const float coef = max_norm / (sqrtf(sqnorm[0]) + 1e-6f);
    if (coef >= 1.0f) return;                 // NaN falls through: the gradients become NaN, as in torch
    int t = 0;
    while (t + 1 < b.count && (int)blockIdx.x >= b.first_wg[t + 1]) ++t;
    float* __restrict__ x = b.x[t];
    const int64_t n = b.n[t];
    const int64_t e0 = (int64_t)((int)blockIdx.x - b.first_wg[t]) * ADA_PER_WG;
    const int64_t e1 = min(n, e0 + ADA_PER_WG);
    if (aligned16(x)) {
        const int64_t v1 = e1 >> 2;
        for (int64_t i = (e0 >> 2) + threadIdx.x; i < v1; i += NT) {
            float4 v = reinterpret_cast<float4*>(x)[i];
            v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
            reinterpret_cast<float4*>(x)[i] = v;
        }
        for (int64_t i = (v1 << 2) + threadIdx.x; i < e1; i += NT) x[i] *= coef;
    } else {
        for (int64_t i = e0 + threadIdx.x; i < e1; i += NT) x[i] *= coef;
    }
}

__global__ void __launch_bounds__(NT) scale_kernel(float* __restrict__ x, int64_t n, float alpha) {
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) x[i] *= alpha;
}

// f32 <-> bf16 (RNE) streams for a half-width gradient all-reduce (lstc_vad_amd/dist.py, reduce_dtype="bf16")
__global__ void __launch_bounds__(NT) cast_f32_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ y, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) y[i] = (__bf16)x[i];
}
__global__ void __launch_bounds__(NT) cast_bf16_f32_kernel(const __bf16* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) y[i] = (float)x[i];
}

// dst row r <- src row idx[r].  grid.x = row, grid.y = chunk of the row; float4 streaming copy (HBM-bound, 2 x bytes).
__global__ void __launch_bounds__(NT) gather_rows_kernel(const float4* __restrict__ src, int64_t src_rows,
                                                         const int64_t* __restrict__ idx, float4* __restrict__ dst,
                                                         int64_t row_vec) {
    const int64_t r = blockIdx.x;
    int64_t s = idx[r];
    s = s < 0 ? 0 : (s >= src_rows ? src_rows - 1 : s);          // never fault on a bad index
    const float4* __restrict__ in = src + s * row_vec;
    float4* __restrict__ out = dst + r * row_vec;
    for (int64_t i = (int64_t)blockIdx.y * NT + threadIdx.x; i < row_vec; i += (int64_t)gridDim.y * NT)
        out[i] = in[i];
}

// dst_j[m, :] = src_j[map[m], :] for j < n matrices of `cols4` float4 per row (row strides in float4): Q, K and V of the token rows
// [M, .] out of the projections of the UNIQUE rows (layer 0 of a batch whose windows overlap), one launch for the three.  One wave
// per row, the row index wave-uniform; HBM-bound (the unique rows are read once from HBM, their repeats from L2).  The map is taken
// as given: its entries must lie inside the source matrices.
struct ExpandArgs {
    const float4* src[3];
    float4* dst[3];
    int64_t ld_src[3], ld_dst[3];
};
__global__ void __launch_bounds__(NT) expand_rows_kernel(ExpandArgs a, int n, const int32_t* __restrict__ map, int64_t rows,
                                                         int cols4) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (m >= rows) return;
    const int64_t s = map[m];
    for (int j = 0; j < n; ++j) {
        const float4* __restrict__ in = a.src[j] + s * a.ld_src[j];
        float4* __restrict__ out = a.dst[j] + m * a.ld_dst[j];
#pragma unroll 8
        for (int c = lane; c < cols4; c += 64) out[c] = in[c];
    }
}

// The mirror image of expand_rows: dst_j[u, :] = sum of src_j[m, :] over the tokens m of group u = order[ptr[u] .. ptr[u + 1]), added
// left to right in f32 from the first one's value (a group of one is a bit-for-bit copy, nothing depends on what shares the launch:
// no atomics); rows groups .. dst_rows - 1 and empty groups are written as zeros.  The row sums of dQ, dK, dV that the layer-0 weight
// gradients contract with the distinct input rows.  grid = (destination row, matrix): the group bounds and the token rows are
// wave-uniform (scalar loads), clamped into the source - a bad table cannot fault.  A thread owns the float4 columns c and c + NT of
// its slice and walks the group in order, four tokens x two columns = 8 loads in flight; groups are mostly 1-3 tokens long, so it is
// the resident workgroups (8 per CU) that cover an HBM miss.  HBM-bound: (tokens + destination rows) x cols x 4 bytes.
__device__ inline int64_t clamp_row(int64_t m, int64_t rows) { return m < 0 ? 0 : (m >= rows ? rows - 1 : m); }
__global__ void __launch_bounds__(NT) segment_sum_rows_kernel(ExpandArgs a, const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ ptr, int64_t src_rows, int64_t groups,
                                                              int cols4) {
    const int64_t u = blockIdx.x;
    const int j = blockIdx.y;
    const float4* __restrict__ src = a.src[j];
    const int64_t ld = a.ld_src[j];
    float4* __restrict__ out = a.dst[j] + u * a.ld_dst[j];
    int64_t beg = 0, end = 0;
    if (u < groups) {
        beg = ptr[u];
        end = ptr[u + 1];
        beg = beg < 0 ? 0 : (beg > src_rows ? src_rows : beg);
        end = end < beg ? beg : (end > src_rows ? src_rows : end);
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = threadIdx.x; c < cols4; c += 2 * NT) {
        const bool two = c + NT < cols4;
        float4 s0 = zero, s1 = zero;
        if (beg < end) {
            const int64_t m = clamp_row(order[beg], src_rows);
            s0 = src[m * ld + c];
            if (two) s1 = src[m * ld + c + NT];
        }
#pragma unroll 4
        for (int64_t k = beg + 1; k < end; ++k) {
            const int64_t m = clamp_row(order[k], src_rows);
            s0 = vadd(s0, src[m * ld + c]);
            if (two) s1 = vadd(s1, src[m * ld + c + NT]);
        }
        out[c] = s0;
        if (two) out[c + NT] = s1;
    }
}

// ---------------------------------------------------------------------------------- segment mean
// out[s, p, :] = mean over the count[s] clips from first[s] of bank[., p, :] (the UCF bins), optionally divided by
// max(||row||_2, 1e-12) (F.normalize on token rows).  One workgroup per (segment, patch); a thread owns the V's c, c + NT, .. of the
// row and walks the clips in order from the first (a count of 1 copies the row bit for bit), 8 loads in flight as in the CLS concat:
// 32 KiB per workgroup on the 16-B path, which a CU's resident workgroups multiply past what hides an HBM miss.  The squares are
// summed per thread in column order, then by block_sum's fixed tree: nothing depends on what shares the launch.  With l2 a thread
// reads back the means it wrote itself and scales them.  HBM-bound: (count + 1) rows moved per row written.  first / count are
// wave-uniform __restrict__ parameters (scalar loads) and are clamped into the bank: a bad table cannot fault.
__device__ inline float vsq(float a) { return a * a; }
__device__ inline float vsq(const float4& a) { return a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w; }
template <typename V>
__global__ void __launch_bounds__(NT) segment_mean_kernel(const V* __restrict__ bank, int64_t bank_clips, const int64_t* __restrict__ first,
                                                           const int32_t* __restrict__ count, int P, int dv, int l2,
                                                           V* __restrict__ out) {
    __shared__ float red[NT / 64];
    const int64_t seg = blockIdx.x / P;
    const int p = blockIdx.x % P;
    int64_t f = first[seg];
    f = f < 0 ? 0 : (f >= bank_clips ? bank_clips - 1 : f);
    int64_t cnt = count[seg];
    cnt = cnt < 1 ? 1 : (cnt > bank_clips - f ? bank_clips - f : cnt);
    const int64_t step = (int64_t)P * dv;
    const V* xr = bank + (f * P + p) * dv;
    V* o = out + (int64_t)blockIdx.x * dv;
    const float div = (float)cnt;
    float sq = 0.f;
    for (int c = threadIdx.x; c < dv; c += NT) {
        V s = xr[c];
#pragma unroll 8
        for (int64_t k = 1; k < cnt; ++k) s = vadd(s, xr[k * step + c]);
        s = vdiv(s, div);
        o[c] = s;
        sq += vsq(s);
    }
    if (!l2) return;                                    // uniform over the launch
    const float nrm = fmaxf(sqrtf(block_sum<NT>(sq, red)), 1e-12f);
    for (int c = threadIdx.x; c < dv; c += NT) o[c] = vdiv(o[c], nrm);
}

inline int grid_for(int64_t work_items, int per_block, int cap = 2048) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

}  // namespace

extern "C" {

static int ln_fwd_launch(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                         int64_t rows, int32_t d, float eps, void* packed, int KBp, void* stream) {
    if (!x || !gamma || !beta || !y || !mean || !rstd) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0) return LSTC_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_for(rows, NT / 64, 4096);
    const bool vec = d % 4 == 0 && d <= 2048 && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta);
    if (vec) {
        if (d <= 256) hipLaunchKernelGGL(ln_fwd_vec<1>, grid, NT, 0, st, x, gamma, beta, y, mean, rstd, rows, d, eps, (__bf16*)packed, KBp);
        else if (d <= 512) hipLaunchKernelGGL(ln_fwd_vec<2>, grid, NT, 0, st, x, gamma, beta, y, mean, rstd, rows, d, eps, (__bf16*)packed, KBp);
        else if (d <= 1024) hipLaunchKernelGGL(ln_fwd_vec<4>, grid, NT, 0, st, x, gamma, beta, y, mean, rstd, rows, d, eps, (__bf16*)packed, KBp);
        else hipLaunchKernelGGL(ln_fwd_vec<8>, grid, NT, 0, st, x, gamma, beta, y, mean, rstd, rows, d, eps, (__bf16*)packed, KBp);
    } else {
        if (packed) return LSTC_E_UNSUPPORTED;
        hipLaunchKernelGGL(ln_fwd_generic, grid, NT, 0, st, x, gamma, beta, y, mean, rstd, rows, d, eps);
    }
    return lstc_launch_status();
}

// The row-wise producers write whole 128-row x 32-k tiles only when the matrix fills the even-by-even tile grid of
// lstc_pack1 exactly (the GEMM streams tile pairs and would add the garbage of an unwritten tile into real outputs).
static bool pack_fused_ok(int64_t rows, int32_t d) { return rows % 256 == 0 && d % 64 == 0 && d <= 2048; }

int lstc_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                       int64_t rows, int32_t d, float eps, void* stream) {
    return ln_fwd_launch(x, gamma, beta, y, mean, rstd, rows, d, eps, nullptr, 0, stream);
}

int lstc_layernorm_fwd_pack(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                            int64_t rows, int32_t d, float eps, void* packed, void* stream) {
    if (!packed) return LSTC_E_NULL;
    if (rows > 0 && d > 0 && !pack_fused_ok(rows, d)) return LSTC_E_UNSUPPORTED;
    if (!aligned16(packed)) return LSTC_E_ALIGN;
    return ln_fwd_launch(x, gamma, beta, y, mean, rstd, rows, d, eps, packed, d / 32, stream);
}

// ln_bwd_pair for d % 4 == 0, d <= 2048 and 16-B-aligned operands (the callers check): NVH float4 per lane of each half row.
// `out`: MODE 1's pack, MODE 2's f32 df, unused in MODE 0.
static int ln_bwd_pair_launch(int mode, const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                              float* dx, float* partial, int32_t n_partial, int64_t rows, int32_t d, void* out, int KBp,
                              DropKey key, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(2 * d + 1024) * sizeof(float);
#define LN_BWD_PAIR(NVH, MODE) hipLaunchKernelGGL((ln_bwd_pair<NVH, MODE>), n_partial, NT, lds, st, dy, x, gamma, mean, rstd, dx, partial, rows, d, (__bf16*)out, KBp, key)
#define LN_BWD_PAIR_D(MODE) do { if (d <= 512) LN_BWD_PAIR(1, MODE); else if (d <= 1024) LN_BWD_PAIR(2, MODE); else LN_BWD_PAIR(4, MODE); } while (0)
    if (mode == 0) LN_BWD_PAIR_D(0);
    else if (mode == 1) LN_BWD_PAIR_D(1);
    else LN_BWD_PAIR_D(2);
#undef LN_BWD_PAIR_D
#undef LN_BWD_PAIR
    return lstc_launch_status();
}

int lstc_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                       float* dx, float* partial, int32_t n_partial, int64_t rows, int32_t d, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !partial) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0 || n_partial <= 0) return LSTC_E_SHAPE;
    if (d % 4 == 0 && d <= 2048 && aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(gamma) && aligned16(partial))
        return ln_bwd_pair_launch(0, dy, x, gamma, mean, rstd, dx, partial, n_partial, rows, d, nullptr, 0, make_drop_key(0.f, 0),
                                  stream);
    if ((size_t)2 * d * sizeof(float) > 64 * 1024) return LSTC_E_RANGE;
    hipLaunchKernelGGL(ln_bwd_generic, n_partial, NT, (size_t)2 * d * sizeof(float), (hipStream_t)stream, dy, x, gamma, mean, rstd,
                       dx, partial, rows, d);
    return lstc_launch_status();
}

int lstc_layernorm_bwd_drop_pack(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                 float* dx, float* partial, int32_t n_partial, int64_t rows, int32_t d, float dropout_p,
                                 uint64_t dropout_seed, void* packed, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !partial || !packed) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0 || n_partial <= 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return LSTC_E_SHAPE;
    if (!pack_fused_ok(rows, d)) return LSTC_E_UNSUPPORTED;
    if ((uint64_t)rows * (uint64_t)d > 0xffffffffull) return LSTC_E_RANGE;      // 32-bit dropout counter
    if (!(aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(gamma) && aligned16(partial) && aligned16(packed)))
        return LSTC_E_ALIGN;
    return ln_bwd_pair_launch(1, dy, x, gamma, mean, rstd, dx, partial, n_partial, rows, d, packed, d / 32,
                              make_drop_key(dropout_p, dropout_seed), stream);
}

int lstc_layernorm_bwd_drop(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                            float* dx, float* df, float* partial, int32_t n_partial, int64_t rows, int32_t d, float dropout_p,
                            uint64_t dropout_seed, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !df || !partial) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0 || n_partial <= 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return LSTC_E_SHAPE;
    if (d != 512 && d != 1024 && d != 2048) return LSTC_E_UNSUPPORTED;          // the model widths: the only callers
    if ((uint64_t)rows * (uint64_t)d > 0xffffffffull) return LSTC_E_RANGE;      // 32-bit dropout counter
    if (!(aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(df) && aligned16(gamma) && aligned16(partial))) return LSTC_E_ALIGN;
    return ln_bwd_pair_launch(2, dy, x, gamma, mean, rstd, dx, partial, n_partial, rows, d, df, 0,
                              make_drop_key(dropout_p, dropout_seed), stream);
}

// bf16 activation stream: the model widths only (d = 1024 / 2048), rows filling the pack's tile grid
static bool act_shape_ok(int64_t rows, int32_t d) { return rows % 256 == 0 && (d == 1024 || d == 2048); }

int lstc_layernorm_fwd_act(const float* x, const void* x_pack, const float* gamma, const float* beta, float* y, void* y_pack,
                           float* mean, float* rstd, int64_t rows, int32_t d, float eps, void* stream) {
    if ((!x) == (!x_pack) || !gamma || !beta || (!y && !y_pack) || !mean || !rstd) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0) return LSTC_E_SHAPE;
    if (!act_shape_ok(rows, d)) return LSTC_E_UNSUPPORTED;
    if (!(aligned16(x) && aligned16(x_pack) && aligned16(y) && aligned16(y_pack) && aligned16(gamma) && aligned16(beta))) return LSTC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid_for(rows, NT / 64, 4096);
    const int KBp = d / 32;
    const __bf16* xp = (const __bf16*)x_pack;
    __bf16* yp = (__bf16*)y_pack;
#define LN_FWD_ACT(NC, XP, YF, YP) hipLaunchKernelGGL((ln_fwd_act<NC, XP, YF, YP>), grid, NT, 0, st, x, xp, gamma, beta, y, yp, mean, rstd, rows, d, eps, KBp)
#define LN_FWD_ACT_D(XP, YF, YP) do { if (d == 1024) LN_FWD_ACT(2, XP, YF, YP); else LN_FWD_ACT(4, XP, YF, YP); } while (0)
    if (x_pack) {
        if (y && y_pack) LN_FWD_ACT_D(true, true, true);
        else if (y) LN_FWD_ACT_D(true, true, false);
        else LN_FWD_ACT_D(true, false, true);
    } else {
        if (y && y_pack) LN_FWD_ACT_D(false, true, true);
        else if (y) LN_FWD_ACT_D(false, true, false);
        else LN_FWD_ACT_D(false, false, true);
    }
#undef LN_FWD_ACT_D
#undef LN_FWD_ACT
    return lstc_launch_status();
}

int lstc_layernorm_bwd_act(const float* dy, const void* dy_pack, const void* x_pack, const float* gamma, const float* mean,
                           const float* rstd, void* dx_pack, float* partial, int32_t n_partial, int64_t rows, int32_t d,
                           float dropout_p, uint64_t dropout_seed, void* df_pack, void* stream) {
    if ((!dy) == (!dy_pack) || !x_pack || !gamma || !mean || !rstd || !partial || !df_pack) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0 || n_partial <= 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return LSTC_E_SHAPE;
    if (!act_shape_ok(rows, d)) return LSTC_E_UNSUPPORTED;
    if ((uint64_t)rows * (uint64_t)d > 0xffffffffull) return LSTC_E_RANGE;      // 32-bit dropout counter
    if (!(aligned16(dy) && aligned16(dy_pack) && aligned16(x_pack) && aligned16(dx_pack) && aligned16(gamma) && aligned16(partial) &&
          aligned16(df_pack))) return LSTC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const DropKey key = make_drop_key(dropout_p, dropout_seed);
    const int KBp = d / 32;
    const size_t lds2 = (size_t)(2 * d + 1024) * sizeof(float);
    const __bf16 *dyp = (const __bf16*)dy_pack, *xp = (const __bf16*)x_pack;
    __bf16 *dxp = (__bf16*)dx_pack, *dfp = (__bf16*)df_pack;
#define LN_BWD_ACT(NCH, DYP, DX) hipLaunchKernelGGL((ln_bwd_act<NCH, DYP, DX>), n_partial, NT, lds2, st, dy, dyp, xp, gamma, mean, rstd, dxp, partial, rows, d, dfp, KBp, key)
#define LN_BWD_ACT_D(DYP, DX) do { if (d == 1024) LN_BWD_ACT(1, DYP, DX); else LN_BWD_ACT(2, DYP, DX); } while (0)
    if (dy_pack) { if (dx_pack) LN_BWD_ACT_D(true, true); else LN_BWD_ACT_D(true, false); }
    else { if (dx_pack) LN_BWD_ACT_D(false, true); else LN_BWD_ACT_D(false, false); }
#undef LN_BWD_ACT_D
#undef LN_BWD_ACT
    return lstc_launch_status();
}

int lstc_cls_concat_fwd(const float* x, const float* x_hi, int64_t n_lo, const float* cls_token, const float* pos,
                        float* y, int64_t N, int32_t S, int32_t d, void* stream) {
    if (!x || !y) return LSTC_E_NULL;
    if (N <= 0 || S < 2 || d <= 0 || (x_hi && (n_lo < 0 || n_lo > N))) return LSTC_E_SHAPE;
    concat_fwd<CONCAT_FIXED>(x, ConcatFixed{x_hi, n_lo, nullptr, 0, 1}, cls_token, pos, y, N, S, d, (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_cls_concat_fwd_pack(const float* x, const float* x_hi, int64_t n_lo, const float* cls_token, const float* pos,
                             float* y, int64_t N, int32_t S, int32_t d, void* packed, void* stream) {
    if (!x || !packed) return LSTC_E_NULL;
    if (N <= 0 || S < 2 || d <= 0 || (x_hi && (n_lo < 0 || n_lo > N))) return LSTC_E_SHAPE;
    if ((N * S) % 256 != 0 || d % 64 != 0) return LSTC_E_UNSUPPORTED;      // the rows fill the pack's even tile grid exactly
    if (!aligned16(packed)) return LSTC_E_ALIGN;
    // y == NULL (pack only: the bf16 activation stream) exists on the 16-B path
    if (!y && !concat_vec16(d, {x, x_hi, cls_token, pos})) return LSTC_E_ALIGN;
    concat_fwd<CONCAT_FIXED>(x, ConcatFixed{x_hi, n_lo, (__bf16*)packed, d / 32, 1}, cls_token, pos, y, N, S, d,
                             (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_cls_concat_gather_fwd(const float* bank, int64_t bank_clips, const int64_t* clip_idx, int32_t P, const float* cls_token,
                               const float* pos, float* y, int64_t N, int32_t S, int32_t d, void* packed, void* stream) {
    if (!bank || !clip_idx || (!y && !packed)) return LSTC_E_NULL;
    if (N <= 0 || S < 2 || d <= 0 || P <= 0 || bank_clips <= 0 || (S - 1) % P != 0) return LSTC_E_SHAPE;
    if (packed && ((N * S) % 256 != 0 || d % 64 != 0)) return LSTC_E_UNSUPPORTED;      // the rows fill the pack's even tile grid exactly
    if (!concat_vec16(d, {bank, y, packed, cls_token, pos})) return LSTC_E_ALIGN;
    concat_fwd<CONCAT_FIXED, true>(bank, ConcatFixed{nullptr, 0, (__bf16*)packed, d / 32, P}, cls_token, pos, y, N, S, d,
                                   (hipStream_t)stream, clip_idx);
    return lstc_launch_status();
}

int lstc_cls_concat_bwd(const float* dy, float* dx, int64_t N, int32_t S, int32_t d, int32_t mean_cls, void* stream) {
    if (!dy || !dx) return LSTC_E_NULL;
    if (N <= 0 || S < 2 || d <= 0) return LSTC_E_SHAPE;
    concat_bwd<CONCAT_FIXED>(dy, ConcatFixed{}, dx, nullptr, N, 0, S, d, mean_cls, (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_cls_concat_len_fwd(const float* x, const int32_t* lens, const float* cls_token, const float* pos, float* y, int64_t N,
                            int32_t S, int32_t d, void* stream) {
    if (!x || !lens || !y) return LSTC_E_NULL;
    if (N <= 0 || S < 2 || d <= 0) return LSTC_E_SHAPE;
    concat_fwd<CONCAT_LEN>(x, ConcatLen{lens}, cls_token, pos, y, N, S, d, (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_cls_concat_len_bwd(const float* dy, const int32_t* lens, float* dx, float* dtok, int64_t N, int32_t S, int32_t d,
                            int32_t mean_cls, void* stream) {
    if (!dy || !lens || (!dx && !dtok)) return LSTC_E_NULL;
    if (N <= 0 || S < 2 || d <= 0) return LSTC_E_SHAPE;
    concat_bwd<CONCAT_LEN>(dy, ConcatLen{lens}, dx, dtok, N, S, S, d, mean_cls, (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_cls_concat_var_fwd(const float* x, const int32_t* row0, const float* cls_token, const float* pos, float* y, int64_t N,
                            int32_t d, void* stream) {
    if (!x || !row0 || !y) return LSTC_E_NULL;
    if (N <= 0 || d <= 0) return LSTC_E_SHAPE;
    concat_fwd<CONCAT_VAR>(x, ConcatVar{row0}, cls_token, pos, y, N, 0, d, (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_cls_concat_span_fwd(const float* bank, int64_t bank_rows, const int64_t* src0, const int32_t* row0, const float* cls_token,
                             const float* pos, float* y, int64_t N, int32_t d, void* stream) {
    if (!bank || !src0 || !row0 || !y) return LSTC_E_NULL;
    if (N <= 0 || d <= 0 || bank_rows <= 0) return LSTC_E_SHAPE;
    concat_fwd<CONCAT_VAR, true>(bank, ConcatVar{row0}, cls_token, pos, y, N, 0, d, (hipStream_t)stream, src0);
    return lstc_launch_status();
}

int lstc_cls_concat_var_bwd(const float* dy, const int32_t* row0, float* dx, float* dtok, int64_t N, int32_t S_max, int32_t d,
                            int32_t mean_cls, void* stream) {
    if (!dy || !row0 || (!dx && !dtok)) return LSTC_E_NULL;
    if (N <= 0 || d <= 0 || (dtok && S_max < 1)) return LSTC_E_SHAPE;
    concat_bwd<CONCAT_VAR>(dy, ConcatVar{row0}, dx, dtok, N, S_max, 0, d, mean_cls, (hipStream_t)stream);
    return lstc_launch_status();
}

int lstc_colsum(const float* x, int64_t rows, int32_t cols, int32_t ld, float* partial, int32_t n_partial, float* out,
                int32_t accumulate, void* stream) {
    if (!x || !partial || !out) return LSTC_E_NULL;
    if (rows <= 0 || cols <= 0 || ld < cols || n_partial <= 0) return LSTC_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int np = (int)(rows < n_partial ? rows : n_partial);
    if (rows <= 12 && rows <= n_partial && cols % 4 == 0 && ld % 4 == 0 && aligned16(x) && aligned16(out)) {
        hipLaunchKernelGGL(colsum_few, dim3((cols / 4 + NT - 1) / NT), NT, 0, st, x, (int)rows, cols, ld, out, accumulate);
        return lstc_launch_status();
    }
    hipLaunchKernelGGL(colsum_pass1, dim3((cols + NT - 1) / NT, np), NT, 0, st, x, rows, cols, ld, partial);
    hipLaunchKernelGGL(colsum_pass2, dim3((cols + 63) / 64), NT, 0, st, partial, np, cols, out, accumulate);
    return lstc_launch_status();
}

int lstc_colsum_batched(const float* x, int32_t batch, int64_t rows, int32_t cols, int32_t ld, int64_t batch_stride,
                        float* partial, int32_t n_partial, float* out, void* stream) {
    if (!x || !partial || !out) return LSTC_E_NULL;
    if (batch <= 0 || batch > 65535 || rows <= 0 || cols <= 0 || ld < cols || n_partial <= 0 || batch_stride < 0) return LSTC_E_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int np = (int)(rows < n_partial ? rows : n_partial);
    hipLaunchKernelGGL(colsum_pass1, dim3((cols + NT - 1) / NT, np, batch), NT, 0, st, x, rows, cols, ld, partial, batch_stride);
    hipLaunchKernelGGL(colsum_pass2, dim3((cols + 63) / 64, batch), NT, 0, st, partial, np, cols, out, 0);
    return lstc_launch_status();
}

int lstc_colsum_pack1(const void* packed, int64_t rows, int32_t K, float* partial, int32_t n_partial, float* out,
                      int32_t accumulate, void* stream) {
    if (!packed || !partial || !out) return LSTC_E_NULL;
    if (rows <= 0 || K <= 0 || n_partial <= 0) return LSTC_E_SHAPE;
    if (!aligned16(packed)) return LSTC_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rb = (rows + 127) / 128;
    const int RB = (int)(rb + (rb & 1)), KB = (K + 31) / 32, KBp = KB + (KB & 1);        // padded rows are zeros
    const int np = (int)(RB < n_partial ? RB : n_partial);
    hipLaunchKernelGGL(colsum_pack1_kernel, dim3(KB, np), NT, 0, st, (const __bf16*)packed, RB, KBp, K, partial);
    hipLaunchKernelGGL(colsum_pass2, dim3((K + 63) / 64), NT, 0, st, partial, np, K, out, accumulate);
    return lstc_launch_status();
}

int lstc_dropout_apply(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream) {
    if (!x || !y) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    if ((uint64_t)n > 0xffffffffull) return LSTC_E_RANGE;
    hipLaunchKernelGGL(dropout_apply_kernel, grid_for(n, NT * 4), NT, 0, (hipStream_t)stream, x, y, n, make_drop_key(p, seed));
    return lstc_launch_status();
}

int lstc_dropout_apply_pack(const void* x_pack, void* y_pack, int64_t rows, int32_t d, float p, uint64_t seed, void* stream) {
    if (!x_pack || !y_pack) return LSTC_E_NULL;
    if (rows <= 0 || d <= 0 || !(p >= 0.f && p < 1.f)) return LSTC_E_SHAPE;
    if (rows % 256 != 0 || d % 64 != 0) return LSTC_E_UNSUPPORTED;            // the matrix fills the pack's even tile grid exactly
    if ((uint64_t)rows * (uint64_t)d > 0xffffffffull) return LSTC_E_RANGE;    // 32-bit dropout counter
    if (!aligned16(x_pack) || !aligned16(y_pack)) return LSTC_E_ALIGN;
    const int64_t chunks = rows * (int64_t)d / 8;
    hipLaunchKernelGGL(dropout_apply_pack_kernel, grid_for(chunks, NT * 2), NT, 0, (hipStream_t)stream, (const __bf16*)x_pack,
                       (__bf16*)y_pack, chunks, d / 32, d, make_drop_key(p, seed));
    return lstc_launch_status();
}

int lstc_splitk_finish(const float* parts, int32_t splits, int64_t part_stride, int64_t M, int64_t N, const float* bias,
                       const float* residual, int64_t ldr, const float* relu_src, int64_t ld_relu, float* C, int64_t ldc, int32_t flags,
                       float dropout_p, uint64_t dropout_seed, int32_t groups, int64_t group_stride_parts, int64_t group_stride_c,
                       void* stream) {
    if (!parts || !C) return LSTC_E_NULL;
    if (((flags & LSTC_EPI_BIAS) && !bias) || ((flags & LSTC_EPI_RESIDUAL) && !residual) || ((flags & LSTC_EPI_RELU_MASK) && !relu_src))
        return LSTC_E_NULL;
    if (splits <= 0 || M <= 0 || N <= 0 || part_stride < M * N || ldc < N || ((flags & LSTC_EPI_RESIDUAL) && ldr < N) ||
        ((flags & LSTC_EPI_RELU_MASK) && ld_relu < N) || !(dropout_p >= 0.f && dropout_p < 1.f)) return LSTC_E_SHAPE;
    if (flags & ~(LSTC_EPI_BIAS | LSTC_EPI_RELU | LSTC_EPI_DROPOUT | LSTC_EPI_RESIDUAL | LSTC_EPI_RELU_MASK | LSTC_EPI_ACCUM))
        return LSTC_E_UNSUPPORTED;
    if (groups < 1 || (groups > 1 && (group_stride_parts < (int64_t)splits * part_stride || group_stride_c <= 0))) return LSTC_E_SHAPE;
    if (groups > 1 && (flags & ~LSTC_EPI_ACCUM)) return LSTC_E_UNSUPPORTED;          // per-head groups: plain sums only
    if (M > 0x7fffffffLL || N > 0x7fffffffLL || (uint64_t)M * (uint64_t)N * (uint64_t)groups > 0xffffffffull) return LSTC_E_RANGE;
    if (group_stride_parts % 4 || group_stride_c % 4) return LSTC_E_ALIGN;
    if (N % 4 || part_stride % 4 || ldc % 4 || ((flags & LSTC_EPI_RESIDUAL) && ldr % 4) || ((flags & LSTC_EPI_RELU_MASK) && ld_relu % 4) ||
        !aligned16(parts) || !aligned16(C) || !aligned16(bias) || !aligned16(residual) || !aligned16(relu_src)) return LSTC_E_ALIGN;
    const DropKey dk = make_drop_key((flags & LSTC_EPI_DROPOUT) ? dropout_p : 0.f, dropout_seed);
    hipLaunchKernelGGL(splitk_finish_kernel, grid_for(M * (N / 4) * groups, NT), NT, 0, (hipStream_t)stream, parts, (int)splits, part_stride,
                       (int)M, (int)N, bias, residual, ldr, relu_src, ld_relu, C, ldc, (int)flags, dk, (int)groups, group_stride_parts,
                       group_stride_c);
    return lstc_launch_status();
}

int lstc_unpack1_rows(const void* x_pack, int64_t rows, int32_t K, int64_t row0, int64_t row_step, int64_t n, float* out, int64_t ldo,
                      void* stream) {
    if (!x_pack || !out) return LSTC_E_NULL;
    if (rows <= 0 || K <= 0 || n <= 0 || row0 < 0 || row_step <= 0 || row0 + (n - 1) * row_step >= rows || ldo < K) return LSTC_E_SHAPE;
    if (K % 8 != 0 || ldo % 4 != 0 || !aligned16(x_pack) || !aligned16(out)) return LSTC_E_ALIGN;
    const int kb = (K + 31) / 32, KBp = kb + (kb & 1);               // 32-k tiles per row block (even: csrc/gemm_bf16p.hip p1_kbp)
    hipLaunchKernelGGL(unpack1_rows_kernel, grid_for(n * (K / 8), NT), NT, 0, (hipStream_t)stream, (const __bf16*)x_pack, KBp, row0,
                       row_step, n, K, out, ldo);
    return lstc_launch_status();
}

int lstc_dropout_mask(uint8_t* mask, int64_t n, float p, uint64_t seed, void* stream) {
    if (!mask) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    if ((uint64_t)n > 0xffffffffull) return LSTC_E_RANGE;
    hipLaunchKernelGGL(dropout_mask_kernel, grid_for(n, NT * 4), NT, 0, (hipStream_t)stream, mask, n, make_drop_key(p, seed));
    return lstc_launch_status();
}

int lstc_head_out_fwd(const float* x, const float* W, const float* b, float* out, int64_t rows, int32_t c, void* stream) {
    if (!x || !W || !b || !out) return LSTC_E_NULL;
    if (rows <= 0 || (c != 1 && c != 2)) return LSTC_E_SHAPE;
    if (!aligned16(x)) return LSTC_E_ALIGN;
    hipLaunchKernelGGL(head_out_fwd_kernel, (unsigned)((rows + NT - 1) / NT), NT, 0, (hipStream_t)stream, x, W, b, out, rows, c);
    return lstc_launch_status();
}

int lstc_head_out_bwd(const float* x, const float* W, const float* out, const float* dout, float* dx, float* dW,
                      float* db, int64_t rows, int32_t c, void* stream) {
    if (!x || !W || !out || !dout || !dx || !dW || !db) return LSTC_E_NULL;
    if (rows <= 0 || (c != 1 && c != 2)) return LSTC_E_SHAPE;
    if (!aligned16(x) || !aligned16(dx)) return LSTC_E_ALIGN;
    hipLaunchKernelGGL(head_out_bwd_kernel, 1u, NT, 0, (hipStream_t)stream, x, W, out, dout, dx, dW, db, rows, c);
    return lstc_launch_status();
}

int lstc_adagrad_step(float* w, const float* grad, float* state, int64_t n, float lr, float weight_decay, float eps,
                      float gscale, void* stream) {
    if (!w || !grad || !state) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    hipLaunchKernelGGL(adagrad_kernel, grid_for(n, NT * 4), NT, 0, (hipStream_t)stream, w, grad, state, n, lr,
                       weight_decay, eps, gscale);
    return lstc_launch_status();
}

int lstc_adagrad_multi(const LstcAdagradItem* items, int32_t count, void* stream) {
    if (!items) return LSTC_E_NULL;
    if (count <= 0) return LSTC_E_SHAPE;
    for (int32_t i = 0; i < count; ++i) {
        if (!items[i].w || !items[i].grad || !items[i].state) return LSTC_E_NULL;
        if (items[i].n <= 0) return LSTC_E_SHAPE;
    }
    return multi_tensor_launch<AdaBatch>(items, count, stream, [](AdaBatch& b, int i, const LstcAdagradItem& it) {
        b.w[i] = it.w; b.g[i] = it.grad; b.s[0][i] = it.state;
        b.lr[i] = it.lr; b.wd[i] = it.weight_decay; b.eps[i] = it.eps; b.gscale[i] = it.grad_scale;
    }, [](const AdaBatch& b, int wg, hipStream_t st) {
        hipLaunchKernelGGL(adagrad_multi_kernel, dim3((unsigned)wg), NT, 0, st, b);
    });
}

int lstc_adagrad_multi_scaled(const LstcAdagradItem* items, int32_t count, const float* lr_scale, void* stream) {
    if (!items || !lr_scale) return LSTC_E_NULL;
    if (count <= 0) return LSTC_E_SHAPE;
    for (int32_t i = 0; i < count; ++i) {
        if (!items[i].w || !items[i].grad || !items[i].state) return LSTC_E_NULL;
        if (items[i].n <= 0) return LSTC_E_SHAPE;
    }
    return multi_tensor_launch<AdaScaledBatch>(items, count, stream, [lr_scale](AdaScaledBatch& b, int i, const LstcAdagradItem& it) {
        b.w[i] = it.w; b.g[i] = it.grad; b.s[0][i] = it.state;
        b.lr[i] = it.lr; b.wd[i] = it.weight_decay; b.eps[i] = it.eps; b.gscale[i] = it.grad_scale;
        b.lr_scale = lr_scale;
    }, [](const AdaScaledBatch& b, int wg, hipStream_t st) {
        hipLaunchKernelGGL(adagrad_multi_scaled_kernel, dim3((unsigned)wg), NT, 0, st, b);
    });
}

int lstc_lr_schedule(const LstcLrSchedule* s, int32_t* step, float* scale, void* stream) {
    if (!s || !step || !scale) return LSTC_E_NULL;
    const bool decays = s->kind == LSTC_LR_LINEAR || s->kind == LSTC_LR_COSINE;
    if (s->kind < LSTC_LR_CONSTANT || s->kind > LSTC_LR_INV_SQRT || s->warmup_steps < 0 || (decays && s->total_steps <= s->warmup_steps) ||
        (s->kind == LSTC_LR_STEP && s->step_size < 1))
        return LSTC_E_SHAPE;
    const auto unit = [](float x) { return x >= 0.f && x <= 1.f; };          // NaN fails
    if (!unit(s->warmup_start) || !unit(s->min_scale) || (s->kind == LSTC_LR_STEP && !(s->gamma > 0.f && s->gamma <= 1.f)))
        return LSTC_E_RANGE;
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), 64, 0, (hipStream_t)stream, *s, step, scale);
    return lstc_launch_status();
}

int lstc_adam_multi(const LstcAdamItem* items, int32_t count, void* stream) {
    if (count < 0 || (!items && count > 0)) return LSTC_E_SHAPE;
    std::vector<const int32_t*> words((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        const LstcAdamItem& it = items[i];
        if (!it.w || !it.grad || !it.m || !it.v || !it.step || it.n < 0) return LSTC_E_SHAPE;
        const auto bad = [](float x) { return !(x >= 0.f) || std::isinf(x); };          // negative, NaN or infinite
        if (bad(it.beta1) || it.beta1 >= 1.f || bad(it.beta2) || it.beta2 >= 1.f || bad(it.eps) || bad(it.lr) || bad(it.weight_decay))
            return LSTC_E_RANGE;
        words[(size_t)i] = it.step;
    }
    std::sort(words.begin(), words.end());
    if (std::adjacent_find(words.begin(), words.end()) != words.end()) return LSTC_E_SHAPE;          // every item owns its word
    return multi_tensor_launch<AdamBatch>(items, count, stream, [](AdamBatch& b, int i, const LstcAdamItem& it) {
        if (i == 0) b.decoupled = 0;
        b.w[i] = it.w; b.g[i] = it.grad; b.s[0][i] = it.m; b.s[1][i] = it.v;
        b.step[i] = it.step; b.lr_scale[i] = it.lr_scale;
        b.lr[i] = it.lr; b.b1[i] = it.beta1; b.b2[i] = it.beta2; b.eps[i] = it.eps; b.wd[i] = it.weight_decay; b.gscale[i] = it.grad_scale;
        if (it.decoupled) b.decoupled |= 1ull << i;
    }, [](const AdamBatch& b, int wg, hipStream_t st) {
        hipLaunchKernelGGL(adam_tick_kernel, dim3(1), 64, 0, st, b);
        if (wg > 0) hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)wg), NT, 0, st, b);          // wg == 0: only empty items
    });
}

int lstc_ema_multi(const LstcEmaItem* items, int32_t count, void* stream) {
    if (count < 0 || (!items && count > 0)) return LSTC_E_SHAPE;
    std::vector<const int32_t*> words((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        const LstcEmaItem& it = items[i];
        if (!it.avg || !it.w || !it.count || it.n < 0 || (it.avg == it.w && it.n > 0)) return LSTC_E_SHAPE;
        if (!(it.decay >= 0.f) || !(it.decay < 1.f) || (it.warmup != 0 && it.warmup != 1)) return LSTC_E_RANGE;          // NaN fails both
        words[(size_t)i] = it.count;
    }
    std::sort(words.begin(), words.end());
    if (std::adjacent_find(words.begin(), words.end()) != words.end()) return LSTC_E_SHAPE;          // every item owns its word
    return multi_tensor_launch<EmaBatch>(items, count, stream, [](EmaBatch& b, int i, const LstcEmaItem& it) {
        if (i == 0) b.warmup = 0;
        b.w[i] = it.avg; b.g[i] = it.w; b.step[i] = it.count; b.decay[i] = it.decay;
        if (it.warmup) b.warmup |= 1ull << i;
    }, [](const EmaBatch& b, int wg, hipStream_t st) {
        hipLaunchKernelGGL(ema_tick_kernel, dim3(1), 64, 0, st, b);
        if (wg > 0) hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)wg), NT, 0, st, b);          // wg == 0: only empty items
    });
}

int lstc_swap_multi(const LstcSwapItem* items, int32_t count, void* stream) {
    if (count < 0 || (!items && count > 0)) return LSTC_E_SHAPE;
    for (int32_t i = 0; i < count; ++i)
        if (!items[i].a || !items[i].b || items[i].n < 0 || (items[i].a == items[i].b && items[i].n > 0)) return LSTC_E_SHAPE;
    return multi_tensor_launch<SwapBatch>(items, count, stream, [](SwapBatch& b, int i, const LstcSwapItem& it) {
        b.w[i] = it.a; b.g[i] = nullptr; b.s[0][i] = it.b;
    }, [](const SwapBatch& b, int wg, hipStream_t st) {
        if (wg > 0) hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)wg), NT, 0, st, b);
    });
}

static int vec_batch(const LstcVecItem* items, int32_t base, int32_t count, VecBatch& b) {
    b.count = count - base < ADA_MAX ? count - base : ADA_MAX;
    int wg = 0;
    for (int i = 0; i < b.count; ++i) {
        b.x[i] = items[base + i].x; b.n[i] = items[base + i].n;
        b.first_wg[i] = wg;
        const int64_t nwg = (items[base + i].n + ADA_PER_WG - 1) / ADA_PER_WG;
        if (nwg > 0x7fffffff - wg) return -1;
        wg += (int)nwg;
    }
    for (int i = b.count; i <= ADA_MAX; ++i) b.first_wg[i] = wg;
    return wg;
}

int64_t lstc_sqnorm_multi_scratch(const LstcVecItem* items, int32_t count) {
    if (!items || count <= 0) return 0;
    int64_t wg = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (items[i].n <= 0) return 0;
        wg += (items[i].n + ADA_PER_WG - 1) / ADA_PER_WG;
    }
    return wg;
}

int lstc_sqnorm_multi(const LstcVecItem* items, int32_t count, float* scratch, int64_t scratch_floats, float* out, void* stream) {
    if (!items || !scratch || !out) return LSTC_E_NULL;
    if (count <= 0) return LSTC_E_SHAPE;
    for (int32_t i = 0; i < count; ++i) {
        if (!items[i].x) return LSTC_E_NULL;
        if (items[i].n <= 0) return LSTC_E_SHAPE;
    }
    const int64_t need = lstc_sqnorm_multi_scratch(items, count);
    if (scratch_floats < need) return LSTC_E_SHAPE;
    int64_t off = 0;
    for (int32_t base = 0; base < count; base += ADA_MAX) {
        VecBatch b;
        const int wg = vec_batch(items, base, count, b);
        if (wg < 0) return LSTC_E_RANGE;
        hipLaunchKernelGGL(sqnorm_multi_kernel, dim3((unsigned)wg), NT, 0, (hipStream_t)stream, b, scratch + off);
        const int rc = lstc_launch_status();
        if (rc) return rc;
        off += wg;
    }
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), NT, 0, (hipStream_t)stream, scratch, need, out);
    return lstc_launch_status();
}

int lstc_clip_scale_multi(const LstcVecItem* items, int32_t count, const float* sqnorm, float max_norm, void* stream) {
    if (!items || !sqnorm) return LSTC_E_NULL;
    if (count <= 0 || !(max_norm > 0.f)) return LSTC_E_SHAPE;
    for (int32_t i = 0; i < count; ++i) {
        if (!items[i].x) return LSTC_E_NULL;
        if (items[i].n <= 0) return LSTC_E_SHAPE;
    }
    for (int32_t base = 0; base < count; base += ADA_MAX) {
        VecBatch b;
        const int wg = vec_batch(items, base, count, b);
        if (wg < 0) return LSTC_E_RANGE;
        hipLaunchKernelGGL(clip_scale_multi_kernel, dim3((unsigned)wg), NT, 0, (hipStream_t)stream, b, sqnorm, max_norm);
        const int rc = lstc_launch_status();
        if (rc) return rc;
    }
    return 0;
}

int lstc_scale(float* x, int64_t n, float alpha, void* stream) {
    if (!x) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    hipLaunchKernelGGL(scale_kernel, grid_for(n, NT * 4), NT, 0, (hipStream_t)stream, x, n, alpha);
    return lstc_launch_status();
}

int lstc_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream) {
    if (!x || !y) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    hipLaunchKernelGGL(cast_f32_bf16_kernel, grid_for(n, NT * 4), NT, 0, (hipStream_t)stream, x, (__bf16*)y, n);
    return lstc_launch_status();
}

int lstc_cast_bf16_f32(const void* x, float* y, int64_t n, void* stream) {
    if (!x || !y) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    hipLaunchKernelGGL(cast_bf16_f32_kernel, grid_for(n, NT * 4), NT, 0, (hipStream_t)stream, (const __bf16*)x, y, n);
    return lstc_launch_status();
}

int lstc_gather_rows(const float* src, int64_t src_rows, const int64_t* idx, float* dst, int64_t n_rows,
                     int64_t row_floats, void* stream) {
    if (!src || !idx || !dst) return LSTC_E_NULL;
    if (src_rows <= 0 || n_rows <= 0 || row_floats <= 0 || (row_floats & 3) || n_rows > 0x7fffffffLL) return LSTC_E_SHAPE;
    if (!aligned16(src) || !aligned16(dst)) return LSTC_E_ALIGN;
    const int64_t row_vec = row_floats / 4;
    int chunks = (int)((row_vec + NT * 4 - 1) / (NT * 4));        // ~4 float4 per thread
    if (chunks < 1) chunks = 1;
    if (chunks > 64) chunks = 64;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n_rows, (unsigned)chunks), NT, 0, (hipStream_t)stream,
                       (const float4*)src, src_rows, idx, (float4*)dst, row_vec);
    return lstc_launch_status();
}

int lstc_segment_mean(const float* bank, int64_t bank_clips, const int64_t* first, const int32_t* count, int64_t n_seg, int32_t P,
                      int32_t d, int32_t l2_normalize, float* out, void* stream) {
    if (!bank || !first || !count || !out) return LSTC_E_NULL;
    if (bank_clips <= 0 || n_seg <= 0 || P <= 0 || d <= 0 || n_seg * P > 0x7fffffffLL) return LSTC_E_SHAPE;
    const bool v4 = d % 4 == 0 && aligned16(bank) && aligned16(out);
    const dim3 grid((unsigned)(n_seg * P));
    if (v4)
        hipLaunchKernelGGL(segment_mean_kernel<float4>, grid, NT, 0, (hipStream_t)stream, (const float4*)bank, bank_clips, first, count,
                           (int)P, (int)(d / 4), (int)l2_normalize, (float4*)out);
    else
        hipLaunchKernelGGL(segment_mean_kernel<float>, grid, NT, 0, (hipStream_t)stream, bank, bank_clips, first, count, (int)P, (int)d,
                           (int)l2_normalize, out);
    return lstc_launch_status();
}

int lstc_expand_rows(const float* const* src, const int64_t* ld_src, float* const* dst, const int64_t* ld_dst, int32_t n,
                     const int32_t* map, int64_t rows, int32_t cols, void* stream) {
    if (!src || !ld_src || !dst || !ld_dst || !map) return LSTC_E_NULL;
    if (n < 1 || n > 3 || rows <= 0 || rows > 0x80000000LL || cols <= 0 || (cols & 3)) return LSTC_E_SHAPE;
    ExpandArgs a = {};
    for (int j = 0; j < n; ++j) {
        if (!src[j] || !dst[j]) return LSTC_E_NULL;
        if (ld_src[j] < cols || ld_dst[j] < cols) return LSTC_E_SHAPE;
        if (!aligned16(src[j]) || !aligned16(dst[j]) || (ld_src[j] & 3) || (ld_dst[j] & 3)) return LSTC_E_ALIGN;
        a.src[j] = (const float4*)src[j];
        a.dst[j] = (float4*)dst[j];
        a.ld_src[j] = ld_src[j] / 4;
        a.ld_dst[j] = ld_dst[j] / 4;
    }
    const int64_t wg = (rows + NT / 64 - 1) / (NT / 64);
    hipLaunchKernelGGL(expand_rows_kernel, dim3((unsigned)wg), NT, 0, (hipStream_t)stream, a, (int)n, map, rows, (int)(cols / 4));
    return lstc_launch_status();
}

int lstc_segment_sum_rows(const float* const* src, const int64_t* ld_src, float* const* dst, const int64_t* ld_dst, int32_t n,
                          const int32_t* order, const int32_t* ptr, int64_t src_rows, int64_t groups, int64_t dst_rows, int32_t cols,
                          void* stream) {
    if (!src || !ld_src || !dst || !ld_dst || !order || !ptr) return LSTC_E_NULL;
    if (n < 1 || n > 3 || src_rows <= 0 || src_rows > 0x7fffffffLL || groups <= 0 || dst_rows < groups || dst_rows > 0x7fffffffLL ||
        cols <= 0 || (cols & 3))
        return LSTC_E_SHAPE;
    ExpandArgs a = {};
    for (int j = 0; j < n; ++j) {
        if (!src[j] || !dst[j]) return LSTC_E_NULL;
        if (ld_src[j] < cols || ld_dst[j] < cols) return LSTC_E_SHAPE;
        if (!aligned16(src[j]) || !aligned16(dst[j]) || (ld_src[j] & 3) || (ld_dst[j] & 3)) return LSTC_E_ALIGN;
        a.src[j] = (const float4*)src[j];
        a.dst[j] = (float4*)dst[j];
        a.ld_src[j] = ld_src[j] / 4;
        a.ld_dst[j] = ld_dst[j] / 4;
    }
    hipLaunchKernelGGL(segment_sum_rows_kernel, dim3((unsigned)dst_rows, (unsigned)n), NT, 0, (hipStream_t)stream, a, order, ptr,
                       src_rows, groups, (int)(cols / 4));
    return lstc_launch_status();
}

int lstc_sqnorm_accum(const float* x, int64_t n, float* out, void* stream) {
    if (!x || !out) return LSTC_E_NULL;
    if (n <= 0) return LSTC_E_SHAPE;
    hipLaunchKernelGGL(sqnorm_kernel, grid_for(n, NT * 8, 1024), NT, 0, (hipStream_t)stream, x, n, out);
    return lstc_launch_status();
}

}  // extern "C"
