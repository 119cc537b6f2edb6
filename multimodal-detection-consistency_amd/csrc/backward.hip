// Input-gradient (dX only) row kernels of the vision tower: what a PGD / Hubness attack needs from
// `encode_image_tensor(x, requires_grad=True)` (reference: src/attacks/pgd_attack.py:456-486,
// src/attacks/hubness_attack.py:269-424).  No weight gradients.
// HBM-bound, one 64-lane wave per row, 16-byte accesses, shuffle reductions -- the layout of elementwise.hip.
// The row shape, the LayerNorm statistics and backward tail, QuickGELU and the bf16 unpack / pack come from rows.hpp.
#include "common.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "rows.hpp"

// ---------------------------------------------------------------------------
// LayerNorm backward with the residual path folded in:
//   x_eff = x (+ delta)            the forward's LN input (fp32 residual stream + the delta it folded: bf16, or fp32 when D32)
//   g     = dy * gamma             dy: gradient w.r.t. the LN output (bf16, or fp32 when DY32)
//   dx    = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ dres)
// dres / dx are fp32 [*, d] rows of the residual-stream gradient (may alias: in place); dx16 (optional) receives
// the bf16 copy that the next GEMM reads.  Row addressing (elements; pinned by tests/test_gpu_tower_ops.py): x AND delta
// row r at r * x_row_stride -- delta shares x's layout, as in the forward --; dy dense [rows, d]; dres, dx and dx16 row r at
// r * out_row_stride (ln_post scatters into the class rows of a zeroed [B * T, d] buffer: what lies between the rows is not written).
// ---------------------------------------------------------------------------
template <bool DY32, bool D32 = false>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, int64_t x_row_stride,
                                                            const void* __restrict__ delta,
                                                            const void* __restrict__ dy, const float* __restrict__ gamma,
                                                            const float* dres, float* dx, uint16_t* __restrict__ dx16,
                                                            int rows, int d, int64_t out_row_stride) {
    const int lane = row_lane();
    const int row = wave_row();
    if (row >= rows) return;
    const f32x4_t* xr = (const f32x4_t*)(x + (int64_t)row * x_row_stride);
    const u32x2_t* dr = delta && !D32 ? (const u32x2_t*)((const uint16_t*)delta + (int64_t)row * x_row_stride) : nullptr;
    const f32x4_t* dr32 = delta && D32 ? (const f32x4_t*)((const float*)delta + (int64_t)row * x_row_stride) : nullptr;
    const int nv = d >> 2;
    f32x4_t v[4] = {}, g[4] = {};
    float s = 0.f;
    for_pieces(lane, nv, [&](int i, int c) {
        v[i] = xr[c];
        if (dr) v[i] += unpack4(dr[c]);
        if (D32 && dr32) v[i] += dr32[c];
        s += piece_sum(v[i]);
        const f32x4_t gm = ((const f32x4_t*)gamma)[c];
        if (DY32) g[i] = ((const f32x4_t*)((const float*)dy + (int64_t)row * d))[c] * gm;
        else g[i] = unpack4(((const u32x2_t*)((const uint16_t*)dy + (int64_t)row * d))[c]) * gm;
    });
    const float mean = row_mean(s, d);
    const float rstd = row_rstd(v, mean, lane, nv, d);
    const f32x4_t* rr = dres ? (const f32x4_t*)(dres + (int64_t)row * out_row_stride) : nullptr;
    f32x4_t* ox = (f32x4_t*)(dx + (int64_t)row * out_row_stride);
    u32x2_t* o16 = dx16 ? (u32x2_t*)(dx16 + (int64_t)row * out_row_stride) : nullptr;
    ln_bwd_tail(v, g, mean, rstd, lane, nv, d, [&](int c, f32x4_t o) {
        if (rr) o += rr[c];
        ox[c] = o;
        if (o16) o16[c] = pack4(o);
    });
}

hipError_t launch_layernorm_bwd(const float* x, int64_t x_row_stride, const uint16_t* delta, const void* dy, int dy_fp32,
                                const float* gamma, const float* dres, float* dx, uint16_t* dx16, int rows, int d,
                                int64_t out_row_stride, hipStream_t stream) {
    if (d % 4 != 0 || d > 1024 || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return dispatch<true, false>(dy_fp32 != 0, [&](auto f32) {
        return launch<layernorm_bwd_kernel<f32.value>>(row_grid(rows), dim3(256), 0, stream, x, x_row_stride, (const void*)delta, dy, gamma,
                                                       dres, dx, dx16, rows, d, out_row_stride);
    });
}

// the split-bf16 gradient's form: fp32 delta, fp32 dy, fp32 dx only
hipError_t launch_layernorm_bwd_f32(const float* x, int64_t x_row_stride, const float* delta, const float* dy, const float* gamma,
                                    const float* dres, float* dx, int rows, int d, int64_t out_row_stride, hipStream_t stream) {
    if (d % 4 != 0 || d > 1024 || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return launch<layernorm_bwd_kernel<true, true>>(row_grid(rows), dim3(256), 0, stream, x, x_row_stride, (const void*)delta, (const void*)dy,
                                                    gamma, dres, dx, (uint16_t*)nullptr, rows, d, out_row_stride);
}

// ---------------------------------------------------------------------------
// ln_pre backward: the forward's input row is (t == 0 ? cls : patch_out[b, t-1]) + pos[t] (assemble_lnpre_kernel);
// dy = fp32 gradient w.r.t. the residual stream after ln_pre; out = bf16 (fp32 with OUT32) gradient w.r.t. patch_out rows
// [B * (T-1), d] (the class row's gradient goes to a parameter and is dropped).
// ---------------------------------------------------------------------------
template <bool OUT32>
__global__ __launch_bounds__(256) void lnpre_bwd_kernel(const float* __restrict__ patch_out, const float* __restrict__ pos,
                                                        const float* __restrict__ gamma, const float* __restrict__ dy,
                                                        void* __restrict__ dpatch, int B, int T, int d) {
    const int lane = row_lane();
    const int64_t prow = wave_row<int64_t>();     // row of patch_out
    if (prow >= (int64_t)B * (T - 1)) return;
    const int64_t b = prow / (T - 1);
    const int t = (int)(prow - b * (T - 1)) + 1;
    const f32x4_t* src = (const f32x4_t*)(patch_out + prow * d);
    const f32x4_t* pr = (const f32x4_t*)(pos + (int64_t)t * d);
    const f32x4_t* gy = (const f32x4_t*)(dy + (b * T + t) * d);
    const int nv = d >> 2;
    f32x4_t v[4] = {}, g[4] = {};
    float s = 0.f;
    for_pieces(lane, nv, [&](int i, int c) {
        v[i] = src[c] + pr[c];
        s += piece_sum(v[i]);
        g[i] = gy[c] * ((const f32x4_t*)gamma)[c];
    });
    const float mean = row_mean(s, d);
    const float rstd = row_rstd(v, mean, lane, nv, d);
    u32x2_t* o = (u32x2_t*)((uint16_t*)dpatch + prow * d);
    f32x4_t* o32 = (f32x4_t*)((float*)dpatch + prow * d);
    ln_bwd_tail(v, g, mean, rstd, lane, nv, d, [&](int c, f32x4_t r) {
        if (OUT32) o32[c] = r;
        else o[c] = pack4(r);
    });
}

hipError_t launch_lnpre_bwd(const float* patch_out, const float* pos, const float* gamma, const float* dy,
                            uint16_t* dpatch, int B, int T, int d, hipStream_t stream) {
    if (d % 4 != 0 || d > 1024) return hipErrorInvalidValue;
    const int64_t rows = (int64_t)B * (T - 1);
    if (rows == 0) return hipSuccess;
    return launch<lnpre_bwd_kernel<false>>(row_grid(rows), dim3(256), 0, stream, patch_out, pos,
                                           gamma, dy, (void*)dpatch, B, T, d);
}

hipError_t launch_lnpre_bwd_f32(const float* patch_out, const float* pos, const float* gamma, const float* dy, float* dpatch, int B,
                                int T, int d, hipStream_t stream) {
    if (d % 4 != 0 || d > 1024) return hipErrorInvalidValue;
    const int64_t rows = (int64_t)B * (T - 1);
    if (rows == 0) return hipSuccess;
    return launch<lnpre_bwd_kernel<true>>(row_grid(rows), dim3(256), 0, stream, patch_out, pos, gamma, dy, (void*)dpatch, B, T, d);
}

// ---------------------------------------------------------------------------
// quick-GELU backward, in place on dm:  du = dm * (s + 1.702 u s (1 - s)),  s = sigmoid(1.702 u)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gelu_bwd_kernel(uint16_t* __restrict__ dm, const uint16_t* __restrict__ u, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        float g[8], x[8];
        unpack8(((const u32x4_t*)dm)[i], g);
        unpack8(((const u32x4_t*)u)[i], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] *= quick_gelu_grad(x[e]);
        ((u32x4_t*)dm)[i] = pack8(g);
    }
}

hipError_t launch_gelu_bwd(uint16_t* dm, const uint16_t* u, int64_t n, hipStream_t stream) {
    if (n % 8 != 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    return launch<gelu_bwd_kernel>(stride_grid(n / 8, 16384), dim3(256), 0, stream, dm, u, n / 8);
}

// the same on fp32 dm and fp32 u (split-bf16 gradient), the expf / division sigmoid of the fp32-grade modes:
//   s = 1 / (1 + exp(-1.702 u)): u -> -inf: exp = inf, s = 0; the second term runs on u clamped as quick_gelu_grad's
__global__ __launch_bounds__(256) void gelu_bwd_f32_kernel(float* __restrict__ dm, const float* __restrict__ u, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4_t g = ((const f32x4_t*)dm)[i];
        const f32x4_t x = __builtin_nontemporal_load((const f32x4_t*)u + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s = 1.0f / (1.0f + expf(-1.702f * x[e]));
            const float xc = fminf(fmaxf(x[e], -1e38f), 1e38f);
            g[e] *= s + 1.702f * xc * s * (1.0f - s);
        }
        ((f32x4_t*)dm)[i] = g;
    }
}

hipError_t launch_gelu_bwd_f32(float* dm, const float* u, int64_t n, hipStream_t stream) {
    if (n % 4 != 0 || n < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    return launch<gelu_bwd_f32_kernel>(stride_grid(n / 4, 16384), dim3(256), 0, stream, dm, u, n / 4);
}

// quick-GELU forward on a bf16 buffer (the grad-mode forward stores the pre-activation and applies this)
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const uint16_t* __restrict__ u, uint16_t* __restrict__ out, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        float x[8];
        unpack8(((const u32x4_t*)u)[i], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = quick_gelu(x[e]);
        ((u32x4_t*)out)[i] = pack8(x);
    }
}

hipError_t launch_gelu_fwd(const uint16_t* u, uint16_t* out, int64_t n, hipStream_t stream) {
    if (n % 8 != 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    return launch<gelu_fwd_kernel>(stride_grid(n / 8, 16384), dim3(256), 0, stream, u, out, n / 8);
}

// ---------------------------------------------------------------------------
// y = x / |x| backward (rows of the projected embedding):  dx = (dy - y (y . dy)) / |x|;  out bf16 (GEMM operand), or fp32
// with OUT32.  normalize == 0: plain cast / copy.
// ---------------------------------------------------------------------------
template <bool OUT32>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         void* __restrict__ dx, int rows, int d, int normalize) {
    const int lane = row_lane();
    const int row = wave_row();
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * d;
    const float* gr = dy + (int64_t)row * d;
    uint16_t* o = (uint16_t*)dx + (int64_t)row * d;
    float* o32 = (float*)dx + (int64_t)row * d;
    auto put = [&](int c, float v) {
        if (OUT32) o32[c] = v;
        else o[c] = f32_to_bf16_bits(v);
    };
    if (!normalize) {
        for (int c = lane; c < d; c += 64) put(c, gr[c]);
        return;
    }
    float ss = 0.f, sd = 0.f;
    for (int c = lane; c < d; c += 64) { ss = fmaf(xr[c], xr[c], ss); sd = fmaf(xr[c], gr[c], sd); }
    ss = wave_sum(ss); sd = wave_sum(sd);
    const float inv = 1.0f / sqrtf(ss);
    const float k = sd * inv * inv;                     // (y . dy) / |x| = (x . dy) / |x|^2
    for (int c = lane; c < d; c += 64) put(c, (gr[c] - xr[c] * k) * inv);
}

hipError_t launch_l2norm_bwd(const float* x, const float* dy, uint16_t* dx16, int rows, int d, int normalize, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    return launch<l2norm_bwd_kernel<false>>(row_grid(rows), dim3(256), 0, stream, x, dy, (void*)dx16, rows, d,
                                            normalize);
}

hipError_t launch_l2norm_bwd_f32(const float* x, const float* dy, float* dx, int rows, int d, int normalize, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    return launch<l2norm_bwd_kernel<true>>(row_grid(rows), dim3(256), 0, stream, x, dy, (void*)dx, rows, d, normalize);
}

// ---------------------------------------------------------------------------
// col2im of the stride = patch conv: dcols fp32 [B*P, Kp] (column order (c, ky, kx)) -> dpix fp32 [B,3,S,S].
// Patches do not overlap: every pixel reads exactly one element.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void col2im_kernel(const float* __restrict__ dcols, float* __restrict__ dpix, int B, int S,
                                                     int patch, int Kp) {
    const int gside = S / patch, P = gside * gside;
    const int64_t total = (int64_t)B * 3 * S * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % S);
        const int yy = (int)((i / S) % S);
        const int c = (int)((i / ((int64_t)S * S)) % 3);
        const int64_t b = i / ((int64_t)3 * S * S);
        const int py = yy / patch, ky = yy - py * patch, px = xx / patch, kx = xx - px * patch;
        dpix[i] = dcols[(b * P + py * gside + px) * Kp + (c * patch + ky) * patch + kx];
    }
}

hipError_t launch_col2im(const float* dcols, float* dpix, int B, int S, int patch, int Kp, hipStream_t stream) {
    const int64_t total = (int64_t)B * 3 * S * S;
    if (total == 0) return hipSuccess;
    return launch<col2im_kernel>(stride_grid(total, 16384), dim3(256), 0, stream, dcols, dpix, B, S, patch, Kp);
}

// ---------------------------------------------------------------------------
// bf16 [R, C] -> [C, R] (weights for the dX GEMMs: A operand = W^T, K-contiguous along the forward's out features)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int R, int C) {
    __shared__ uint16_t tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) tile[j][tx] = in[(int64_t)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) out[(int64_t)(c0 + j) * R + r0 + tx] = tile[tx][j];
}

hipError_t launch_transpose_bf16(const uint16_t* in, uint16_t* out, int R, int C, hipStream_t stream) {
    if (R <= 0 || C <= 0) return hipSuccess;
    return launch<transpose_bf16_kernel>(dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, stream, in, out, R, C);
}

// ---------------------------------------------------------------------------
// One PGD step on a batch (src/attacks/pgd_attack.py:500-521): momentum on the per-sample L1-normalised gradient,
// sign step, projection to the eps ball around the clean image, clamp.  One workgroup per image.
//   mom = mu * mom + grad / |grad|_1      (use_momentum; else the raw gradient)
//   adv = clamp(clean + clamp(adv + dir * alpha * sign(mom) - clean, -eps, eps), lo, hi)      dir = +1 untargeted, -1 targeted
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void pgd_step_kernel(float* __restrict__ adv, const float* __restrict__ clean,
                                                        const float* __restrict__ grad, float* __restrict__ mom, int64_t n,
                                                        float eps, float alpha, float mu, float lo, float hi, float dir) {
    __shared__ float red[16];
    const int64_t base = (int64_t)blockIdx.x * n;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float inv = 1.0f;
    if (mom) {
        float s = 0.f;
        for (int64_t i = t; i < n; i += 1024) s += fabsf(grad[base + i]);
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += red[w];
        inv = 1.0f / tot;
    }
    for (int64_t i = t; i < n; i += 1024) {
        float g = grad[base + i];
        if (mom) { g = mu * mom[base + i] + g * inv; mom[base + i] = g; }
        const float sgn = (g > 0.f) ? 1.f : ((g < 0.f) ? -1.f : 0.f);      // torch.sign
        const float c = clean[base + i];
        float a = adv[base + i] + dir * alpha * sgn;
        float dl = a - c;
        dl = fminf(fmaxf(dl, -eps), eps);
        adv[base + i] = fminf(fmaxf(c + dl, lo), hi);
    }
}

// ---------------------------------------------------------------------------
// L2-constrained step (src/attacks/hubness_attack.py:378-386), one workgroup per image:
//   adv += dir * step * grad / (|grad|_2 + 1e-8);   d = adv - clean;   d *= min(|d|_2, eps) / (|d|_2 + 1e-8)
//   adv = clamp(clean + d, lo, hi)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void l2_step_kernel(float* __restrict__ adv, const float* __restrict__ clean,
                                                       const float* __restrict__ grad, int64_t n, float eps, float step,
                                                       float lo, float hi, float dir) {
    __shared__ float red[16];
    const int64_t base = (int64_t)blockIdx.x * n;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += red[w];
        return tot;
    };
    float s = 0.f;
    for (int64_t i = t; i < n; i += 1024) { const float g = grad[base + i]; s += g * g; }
    const float gscale = dir * step / (sqrtf(block_sum(s)) + 1e-8f);
    float q = 0.f;
    for (int64_t i = t; i < n; i += 1024) {
        const float a = adv[base + i] + gscale * grad[base + i];
        adv[base + i] = a;                       // each element is read back by the thread that wrote it
        const float d = a - clean[base + i];
        q += d * d;
    }
    const float dn = sqrtf(block_sum(q));
    const float dscale = fminf(dn, eps) / (dn + 1e-8f);
    for (int64_t i = t; i < n; i += 1024) {
        const float c = clean[base + i];
        adv[base + i] = fminf(fmaxf(c + (adv[base + i] - c) * dscale, lo), hi);
    }
}

hipError_t launch_l2_step(float* adv, const float* clean, const float* grad, int B, int64_t n, float eps, float step, float lo,
                          float hi, int descent, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    return launch<l2_step_kernel>(dim3(B), dim3(1024), 0, stream, adv, clean, grad, n, eps, step, lo, hi, descent ? -1.0f : 1.0f);
}

hipError_t launch_pgd_step(float* adv, const float* clean, const float* grad, float* mom, int B, int64_t n, float eps,
                           float alpha, float mu, float lo, float hi, int targeted, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    return launch<pgd_step_kernel>(dim3(B), dim3(1024), 0, stream, adv, clean, grad, mom, n, eps, alpha, mu, lo, hi,
                                   targeted ? -1.0f : 1.0f);
}
