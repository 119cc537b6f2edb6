// The wave-per-row vocabulary of the row kernels (device side; included by the .hip files only): one 64-lane wave per
// row, four rows per 256-thread workgroup, d % 4 == 0 and d <= 1024, so a lane holds the row as up to four f32x4_t
// pieces (vector column c = lane + 64 * i).  LayerNorm statistics are two-pass (mean, then squared deviations) in a fixed
// summation order.  Also the one definition of the GELU forms and of the 16-bit pack / unpack of 4- and 8-wide pieces.
// Everything here is stateless and inlined: a kernel built from these helpers is the straight-line code it was when the
// loops were written out in it.
#pragma once
#include "common.hpp"

#define ROWS_PER_BLOCK 4   // 256 threads = 4 waves = 4 rows
#define LN_EPS 1e-5f

// ---- row shape
__device__ __forceinline__ int row_lane() { return threadIdx.x & 63; }
// the row of this wave (R = int64_t where rows * d may pass 2^31)
template <class R = int>
__device__ __forceinline__ R wave_row() { return (R)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6); }
// The grid-stride form of the shape: f(row) for the rows wave_row(), + gridDim.x * ROWS_PER_BLOCK, ... below `rows` (the whole
// wave calls f; a `return` in f goes on to the wave's next row).  Its grid is wave_stride_grid(rows) (host_plan.hpp), whose cap
// keeps the first row and the step far inside 32 bits.
template <class R, class F>
__device__ __forceinline__ void for_wave_rows(R rows, F&& f) {
    for (R i = (R)(blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)); i < rows; i += (R)(gridDim.x * ROWS_PER_BLOCK)) f(i);
}

// f(i, c) for the pieces i = 0..3 of this lane that exist in a row of nv vector columns
template <class F>
__device__ __forceinline__ void for_pieces(int lane, int nv, F&& f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) f(i, c);
    }
}

// ---- statistics
__device__ __forceinline__ float piece_sum(const f32x4_t v) { return (v[0] + v[1]) + (v[2] + v[3]); }
// s: this lane's piece_sum()s added in piece order
__device__ __forceinline__ float row_mean(float s, int d) { return wave_sum(s) / (float)d; }
// 1 / sqrt(var + LN_EPS).  EXACT: the IEEE square root and division of the split mode (its bits are under the 1e-4
// contract); else v_rsq_f32.  The squared deviations are a separate multiply and add per element (t = 0..3, pieces in order),
// never an fma: that is the arithmetic every one of these kernels has always run, and with contraction left to the
// compiler it depends on whether a piece's guard is branched over or if-converted.
template <bool EXACT = false>
__device__ __forceinline__ float row_rstd(const f32x4_t (&v)[4], float mean, int lane, int nv, int d) {
    float q = 0.f;
    for_pieces(lane, nv, [&](int i, int) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma clang fp contract(off)
            const float dl = v[i][t] - mean;
            q += dl * dl;
        }
    });
    const float var = wave_sum(q) / (float)d + LN_EPS;
    return EXACT ? 1.0f / sqrtf(var) : rsqrtf(var);
}

// ---- affine: (v - mean) * rstd * g[c] + b[c] on vector column c; the last multiply and add are ONE fma, written out: that is what
// these kernels have always run (v_pk_fma_f32), and as an fmaf it no longer rests on the compiler's contraction
__device__ __forceinline__ f32x4_t ln_affine(const f32x4_t v, float mean, float rstd, const float* __restrict__ g,
                                             const float* __restrict__ b, int c) {
    const f32x4_t gg = ((const f32x4_t*)g)[c];
    const f32x4_t bb = ((const f32x4_t*)b)[c];
    f32x4_t o;
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = fmaf((v[t] - mean) * rstd, gg[t], bb[t]);
    return o;
}

// ---- backward: v = the forward's LN input pieces, g = dy * gamma;  store(c, rstd * (g - mean(g) - xhat * mean(g * xhat))).
// The last expression is left to the compiler's contraction (an explicit fmaf(-xhat, c2, g - c1) is NOT what it chooses): its bits are
// held to the previous build's only by scripts/lib_ab.py, which is to be rerun when this function or the compiler changes.
template <class Store>
__device__ __forceinline__ void ln_bwd_tail(f32x4_t (&v)[4], const f32x4_t (&g)[4], float mean, float rstd, int lane, int nv,
                                            int d, Store&& store) {
    float sg = 0.f, sgx = 0.f;
    for_pieces(lane, nv, [&](int i, int) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            v[i][t] = (v[i][t] - mean) * rstd;
            sg += g[i][t];
            sgx = fmaf(g[i][t], v[i][t], sgx);
        }
    });
    const float c1 = wave_sum(sg) / (float)d, c2 = wave_sum(sgx) / (float)d;
    for_pieces(lane, nv, [&](int i, int c) {
        f32x4_t o;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = rstd * (g[i][t] - c1 - v[i][t] * c2);
        store(c, o);
    });
}

// ---- GELU
// exact: 0.5 x (1 + erf(x / sqrt 2))
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
// QuickGELU x * sigmoid(1.702 x), fast form: sigmoid = 1 / (1 + 2^(-1.702 log2(e) x)) on v_exp_f32 + v_rcp_f32 (1 ulp each; the
// result is rounded to 16 bits anyway) instead of an IEEE division.  x -> -inf: 2^(+inf) = inf, rcp(inf) = 0, x * 0 = -0.
__device__ __forceinline__ float quick_gelu_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.4554670f * x));
}
__device__ __forceinline__ float quick_gelu(float x) { return x * quick_gelu_sigmoid(x); }
// d quick_gelu / dx = s + 1.702 x s (1 - s).  The product runs on x clamped to +-1e38: beyond it s is exactly 0 or 1 and the
// second term is 0, but 1.702 x itself overflows from |x| = 2e38 on and inf * 0 made the gradient NaN at the ends of the bf16
// range.  Inside the clamp the expression and its bits are what they were.
__device__ __forceinline__ float quick_gelu_grad(float x) {
    const float s = quick_gelu_sigmoid(x);
    const float xc = fminf(fmaxf(x, -1e38f), 1e38f);
    return s + 1.702f * xc * s * (1.0f - s);
}
// the expf / division form of the fp32-grade modes (as the fp32 CPU path)
__device__ __forceinline__ float quick_gelu_exact(float x) { return x / (1.0f + expf(-1.702f * x)); }

// ---- 16-bit pieces <-> fp32 (bf16, or IEEE fp16 with F16)
template <bool F16 = false>
__device__ __forceinline__ f32x4_t unpack4(const u32x2_t w) {
    return f32x4_t{Op16<F16>::lo(w[0]), Op16<F16>::hi(w[0]), Op16<F16>::lo(w[1]), Op16<F16>::hi(w[1])};
}
template <bool F16 = false>
__device__ __forceinline__ u32x2_t pack4(const f32x4_t f) {
    return u32x2_t{Op16<F16>::pack2(f[0], f[1]), Op16<F16>::pack2(f[2], f[3])};
}
template <bool F16 = false>
__device__ __forceinline__ void unpack8(const u32x4_t v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = Op16<F16>::lo(v[i]);
        f[2 * i + 1] = Op16<F16>::hi(v[i]);
    }
}
template <bool F16 = false>
__device__ __forceinline__ u32x4_t pack8(const float* f) {
    return u32x4_t{Op16<F16>::pack2(f[0], f[1]), Op16<F16>::pack2(f[2], f[3]), Op16<F16>::pack2(f[4], f[5]),
                   Op16<F16>::pack2(f[6], f[7])};
}
