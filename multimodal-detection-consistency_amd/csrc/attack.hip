// FSTA / SMA attack kernels (src/attacks/fsta_attack.py:156-297, src/attacks/sma_attack.py:207-373,577-735): both loops are
// one loop with different constants, so one feature-loss gradient kernel and one step kernel serve both.
//
//   feature grad  `attack_feature_grad_kernel`, one 256-thread workgroup per batch row i.  With n = |f_i|, fh = f / n,
//           vh = v / |v| and S = sum_j fh_j the loss is
//               L = a_tgt mean_i cos(f_i, g_i) + a_txt mean_i cos(f_i, t_i) + w_out mse(f, g) + w_div (|S|^2 - B) / (B (B - 1))
//           and its gradient for row i
//               a (vh_i - c_i fh_i) / (n_i B)                                  per cosine term, c_i = fh_i . vh_i
//               -a (f_i - v_i) / (|f_i - v_i| B), 0 at distance 0                per term under the Euclidean metric
//               2 w_out (f_i - g_i) / (B D)
//               2 w_div ((S - fh_i) - (fh_i . S - 1) fh_i) / (n_i B (B - 1))    0 when B = 1
//           The rows couple only through S.  Every workgroup sums it itself, rows in j order (the [B, B] cosine matrix is
//           never formed): the inverse norms of 256 rows at a time go to LDS, a wave per row; then thread t adds fh_j[c] for
//           its columns c = t, t + 256, ...  S[c] waits in grad[i, c] -- written and read back by the same thread -- until
//           fh_i . S is known.  A term whose weight is 0 is skipped, not multiplied by 0: a NaN row reaches the other rows
//           through S only, and only when w_div != 0.  Fixed summation order, no atomics: the outputs are a pure function of
//           the inputs.
//   step    inf: `attack_step_inf_kernel`, elementwise over all B n elements on a capped grid-stride grid, 16 bytes per access
//           when B n is a multiple of 4 and the pointers are aligned.  l2: `attack_step_l2_kernel`, one 1024-thread workgroup
//           per image (the projection needs |adv - clean|_2 of the image).
//               g = grad + p (adv - clean);  clip > 0: g = clamp(g, -clip, clip);  m = mu m + g
//               inf: a = adv - lr sign(m);  adv = clamp(clean + clamp(a - clean, -eps, eps), lo, hi)
//               l2 : a = adv - lr m;  d = a - clean;  d *= min(1, eps / (|d|_2 + 1e-8));  adv = clamp(clean + d, lo, hi)
//           p == 0 and clip <= 0 skip their operation (not "+ 0 x"): the bits are those of a kernel without the term.  Products
//           and sums of the momentum chain are rounded one by one (no fma): up to the image's L2 norm, an element is what the
//           same chain of fp32 operations gives anywhere else.
#include "common.hpp"
#include "kernels.hpp"
#include "launch.hpp"

#define ATTACK_INV_CHUNK 256        // rows whose inverse norms one LDS pass holds
#define ATTACK_STEP_MAX_BLOCKS 2048 // grid cap of the elementwise step: 8 workgroups of 256 threads per compute unit

// sum over the workgroup's 256 threads of NV values each, every thread gets every total; red: [4][NV] floats of LDS
template <int NV>
__device__ __forceinline__ void block_sum4(float (&v)[NV], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();                                  // the previous use of red is over
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = (red[k] + red[NV + k]) + (red[2 * NV + k] + red[3 * NV + k]);
}

__global__ __launch_bounds__(256) void attack_feature_grad_kernel(const float* __restrict__ f, const float* __restrict__ t,
                                                                  const float* __restrict__ g, int B, int D, float a_tgt,
                                                                  float a_txt, int euclid, float w_out, float w_div,
                                                                  float* __restrict__ grad, float* __restrict__ loss_rows) {
    __shared__ float red[4 * 7];
    __shared__ float inv[ATTACK_INV_CHUNK];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* fi = f + (int64_t)i * D;
    const float* ti = t + (int64_t)i * D;
    const float* gi = g + (int64_t)i * D;
    float* out = grad + (int64_t)i * D;

    // ---- the row's own sums: |f|^2, |t|^2, |g|^2, f.t, f.g, |f - t|^2, |f - g|^2
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < D; c += 256) {
        const float x = fi[c], y = ti[c], z = gi[c];
        s[0] += x * x; s[1] += y * y; s[2] += z * z; s[3] += x * y; s[4] += x * z;
        s[5] += (x - y) * (x - y); s[6] += (x - z) * (x - z);
    }
    block_sum4<7>(s, red);
    const float inv_n = 1.0f / sqrtf(s[0]), inv_t = 1.0f / sqrtf(s[1]), inv_g = 1.0f / sqrtf(s[2]);
    const float cos_t = s[3] * inv_n * inv_t, cos_g = s[4] * inv_n * inv_g;
    const float dist_t = sqrtf(s[5]), dist_g = sqrtf(s[6]);

    // ---- S = sum_j f_j / |f_j| in j order, into out[]; q = fh_i . S
    float q1 = 0.f;                                   // sum_{j != i} cos_ij = fh_i . S - 1
    if (B > 1) {
        for (int c = tid; c < D; c += 256) out[c] = 0.f;
        for (int j0 = 0; j0 < B; j0 += ATTACK_INV_CHUNK) {
            const int nj = min(ATTACK_INV_CHUNK, B - j0);
            __syncthreads();                          // the previous chunk's inv[] has been read
            for (int j = wave; j < nj; j += 4) {
                const float* fj = f + (int64_t)(j0 + j) * D;
                float ss = 0.f;
                for (int c = lane; c < D; c += 64) ss += fj[c] * fj[c];
                ss = wave_sum(ss);
                if (lane == 0) inv[j] = 1.0f / sqrtf(ss);
            }
            __syncthreads();
            for (int c = tid; c < D; c += 256) {
                float acc = out[c];
                for (int j = 0; j < nj; ++j) acc += f[(int64_t)(j0 + j) * D + c] * inv[j];
                out[c] = acc;
            }
        }
        float q[1] = {0.f};
        for (int c = tid; c < D; c += 256) q[0] += (fi[c] * inv_n) * out[c];
        block_sum4<1>(q, red);
        q1 = q[0] - 1.0f;
    }

    // ---- the gradient row
    const float invB = 1.0f / (float)B;
    const float k_out = 2.0f * w_out / ((float)B * (float)D);
    const float k_div = (B > 1) ? 2.0f * w_div * inv_n / ((float)B * (float)(B - 1)) : 0.f;
    const bool div_on = B > 1 && w_div != 0.f;
    // Euclidean: d|f - v| / df = (f - v) / |f - v|, 0 at distance 0 (torch's norm backward); the loss term is -a mean |f - v|
    const float e_g = (dist_g > 0.f) ? -a_tgt * invB / dist_g : 0.f;
    const float e_t = (dist_t > 0.f) ? -a_txt * invB / dist_t : 0.f;
    const float k_g = a_tgt * invB * inv_n, k_t = a_txt * invB * inv_n;
    for (int c = tid; c < D; c += 256) {
        const float x = fi[c], fh = x * inv_n;
        float r = 0.f;
        if (euclid) {
            if (a_tgt != 0.f) r += e_g * (x - gi[c]);
            if (a_txt != 0.f) r += e_t * (x - ti[c]);
        } else {
            if (a_tgt != 0.f) r += k_g * (gi[c] * inv_g - cos_g * fh);
            if (a_txt != 0.f) r += k_t * (ti[c] * inv_t - cos_t * fh);
        }
        if (w_out != 0.f) r += k_out * (x - gi[c]);
        if (div_on) r += k_div * ((out[c] - fh) - q1 * fh);
        out[c] = r;
    }
    if (tid == 0) {
        float* lr = loss_rows + (int64_t)i * 4;
        lr[0] = euclid ? dist_g : cos_g;
        lr[1] = euclid ? dist_t : cos_t;
        lr[2] = s[6] / (float)D;
        lr[3] = q1;
    }
}

hipError_t launch_attack_feature_grad(const float* f, const float* t, const float* g, int B, int D, float a_tgt, float a_txt,
                                      int euclid, float w_out, float w_div, float* grad, float* loss_rows, hipStream_t stream) {
    if (B <= 0 || D <= 0) return hipSuccess;
    return launch<attack_feature_grad_kernel>(dim3(B), dim3(256), 0, stream, f, t, g, B, D, a_tgt, a_txt, euclid, w_out, w_div,
                                              grad, loss_rows);
}

// ---- step --------------------------------------------------------------------------------------------------------------
// the clipped, momentum-accumulated gradient of one element; m is updated in place
__device__ __forceinline__ float attack_momentum(float gr, float a, float c, float& m, float mu, float clip, float p) {
    if (p != 0.f) gr = __fadd_rn(gr, __fmul_rn(p, a - c));        // _rn: never contracted into an fma, so every element is the
    if (clip > 0.f) gr = fminf(fmaxf(gr, -clip), clip);          // fp32 chain of separately rounded operations
    m = __fadd_rn(__fmul_rn(mu, m), gr);
    return m;
}

__device__ __forceinline__ float attack_inf_element(float gr, float a, float c, float& m, float eps, float lr, float mu,
                                                    float clip, float p, float lo, float hi) {
    const float mm = attack_momentum(gr, a, c, m, mu, clip, p);
    const float sgn = (mm > 0.f) ? 1.f : ((mm < 0.f) ? -1.f : 0.f);      // torch.sign
    float dl = (a - lr * sgn) - c;                                     // lr * sgn is exact: one rounding, fused or not
    dl = fminf(fmaxf(dl, -eps), eps);
    return fminf(fmaxf(c + dl, lo), hi);
}

template <int VEC>
__global__ __launch_bounds__(256) void attack_step_inf_kernel(float* __restrict__ adv, const float* __restrict__ clean,
                                                              const float* __restrict__ grad, float* __restrict__ mom,
                                                              int64_t total, float eps, float lr, float mu, float clip, float p,
                                                              float lo, float hi) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    if constexpr (VEC == 4) {
        const int64_t nv = total / 4;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
            float4 a = ((const float4*)adv)[i], m = ((const float4*)mom)[i];
            const float4 c = ((const float4*)clean)[i], gr = ((const float4*)grad)[i];
            a.x = attack_inf_element(gr.x, a.x, c.x, m.x, eps, lr, mu, clip, p, lo, hi);
            a.y = attack_inf_element(gr.y, a.y, c.y, m.y, eps, lr, mu, clip, p, lo, hi);
            a.z = attack_inf_element(gr.z, a.z, c.z, m.z, eps, lr, mu, clip, p, lo, hi);
            a.w = attack_inf_element(gr.w, a.w, c.w, m.w, eps, lr, mu, clip, p, lo, hi);
            ((float4*)mom)[i] = m;
            ((float4*)adv)[i] = a;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
            float m = mom[i];
            adv[i] = attack_inf_element(grad[i], adv[i], clean[i], m, eps, lr, mu, clip, p, lo, hi);
            mom[i] = m;
        }
    }
}

__global__ __launch_bounds__(1024) void attack_step_l2_kernel(float* __restrict__ adv, const float* __restrict__ clean,
                                                              const float* __restrict__ grad, float* __restrict__ mom, int64_t n,
                                                              float eps, float lr, float mu, float clip, float p, float lo,
                                                              float hi) {
    __shared__ float red[16];
    const int64_t base = (int64_t)blockIdx.x * n;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float q = 0.f;
    for (int64_t i = t; i < n; i += 1024) {
        const float c = clean[base + i];
        float a = adv[base + i], m = mom[base + i];
        const float mm = attack_momentum(grad[base + i], a, c, m, mu, clip, p);
        mom[base + i] = mm;
        a = __fsub_rn(a, __fmul_rn(lr, mm));
        adv[base + i] = a;                       // each element is read back by the thread that wrote it
        const float d = a - c;
        q += d * d;
    }
    q = wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += red[w];
    const float scale = fminf(1.0f, eps / (sqrtf(tot) + 1e-8f));
    for (int64_t i = t; i < n; i += 1024) {
        const float c = clean[base + i];
        adv[base + i] = fminf(fmaxf(c + (adv[base + i] - c) * scale, lo), hi);
    }
}

hipError_t launch_attack_step(float* adv, const float* clean, const float* grad, float* mom, int B, int64_t n, float eps, float lr,
                              float mu, float clip, float p, float lo, float hi, int l2, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    if (l2) return launch<attack_step_l2_kernel>(dim3(B), dim3(1024), 0, stream, adv, clean, grad, mom, n, eps, lr, mu, clip, p, lo, hi);
    const int64_t total = (int64_t)B * n;
    const bool vec = total % 4 == 0 && (((uintptr_t)adv | (uintptr_t)clean | (uintptr_t)grad | (uintptr_t)mom) & 15) == 0;
    if (vec)
        return launch<attack_step_inf_kernel<4>>(stride_grid(total / 4, ATTACK_STEP_MAX_BLOCKS), dim3(256), 0, stream, adv, clean,
                                                 grad, mom, total, eps, lr, mu, clip, p, lo, hi);
    return launch<attack_step_inf_kernel<1>>(stride_grid(total, ATTACK_STEP_MAX_BLOCKS), dim3(256), 0, stream, adv, clean, grad, mom,
                                             total, eps, lr, mu, clip, p, lo, hi);
}
