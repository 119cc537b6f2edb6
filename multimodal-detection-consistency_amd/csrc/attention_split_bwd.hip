// Attention backward of the split-bf16 input gradient (TVC_OPT_GRAD_PRECISION = 2; include/tvc.h): fp32 qkv (kept by
// the forward) and fp32 dO -> fp32 dQ | dK | dV.  The two passes of attention_bwd.hip (lane = query: dQ and the softmax
// statistics; lane = key: dK, dV over all query tiles) with every operand carried as hi | lo bf16 and every product
// formed from three MFMAs, small terms first, as split.hip's forward:
//   S = K Q^T,  dP = V dO^T,  dQ^T = K^T dS^T           (pass A)
//   S = Q K^T,  dP = dO V^T,  dV^T += dO^T P,  dK^T += Q^T dS      (pass B)
// The softmax, delta = rowsum(P * dP) (= rowsum(dO * O)) and dS = P (dP - delta) / 8 are fp32; P and dS are split into
// hi | lo when they become MFMA operands.  Non-causal, dense sequences of T <= 288 tokens, head dim 64.
//
// LDS: FOUR images per pass (hi and lo of two tensors), all with ATT_KROW's 128-byte swizzled rows -- 512 bytes per
// token, 147 456 B at 288 tokens (+ 4 608 B of statistics in pass B): one workgroup per CU.  The padded 160-byte rows
// that attention_bwd.hip reads transposed would need 184 KB.  So the transposed reads (ds_read_b64_tr_b16) address
// the swizzled image themselves: a lane's 8 bytes lie inside one 16-byte chunk, whose position the row's swizzle gives.
#include "attn_frag.hpp"
#include "kernels.hpp"
#include "launch.hpp"

namespace {

// Byte offset of this lane's transposed 8-byte read in an ATT_KROW image: row 16 t + 4 g + (r16 >> 2), head dims
// 16 md + 4 (r16 & 3) .. + 3 (tr_lane_off's element, through swz_chunk)
__device__ __forceinline__ int tr_swz_off(int t, int md, int g, int r16) {
    const int row = t * 16 + 4 * g + (r16 >> 2);
    const int c = md * 2 + ((r16 & 3) >> 1);
    return row * ATT_KROW + swz_chunk(c, row) + ((r16 & 1) << 3);
}

// hi | lo A fragments [16 dh x 32 rows] of the tile pair (t0, t1) of a swizzled image pair
__device__ __forceinline__ void tr_pair(const char* img_h, const char* img_l, int t0, int t1, int md, int g, int r16, bf16x8_t& ah,
                                        bf16x8_t& al) {
    const int o0 = tr_swz_off(t0, md, g, r16), o1 = tr_swz_off(t1, md, g, r16);
    const bf16x4_t h0 = tr16_read(img_h + o0), h1 = tr16_read(img_h + o1), l0 = tr16_read(img_l + o0), l1 = tr16_read(img_l + o1);
    ah = join8<false>(h0, h1);
    al = join8<false>(l0, l1);
}

// one 16 x 16 tile of A B^T over the 64 head dims: A = rows 16 t + r16 of a swizzled image pair, B = a lane's row as
// four fragments (dh 8 g .. + 7 and 32 + 8 g .. + 7, hi and lo); small terms first
__device__ __forceinline__ f32x4_t rows_dot(const char* img_h, const char* img_l, int t, int r16, int sw0, int sw1, const bf16x8_t b0h,
                                            const bf16x8_t b0l, const bf16x8_t b1h, const bf16x8_t b1l, f32x4_t c) {
    const int ro = (t * 16 + r16) * ATT_KROW;
    const bf16x8_t a0h = *(const bf16x8_t*)(img_h + ro + sw0), a1h = *(const bf16x8_t*)(img_h + ro + sw1);
    const bf16x8_t a0l = *(const bf16x8_t*)(img_l + ro + sw0), a1l = *(const bf16x8_t*)(img_l + ro + sw1);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0h, b0l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1h, b1l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0l, b0h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1l, b1h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0h, b0h, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1h, b1h, c, 0, 0, 0);
}

// a lane's row (64 fp32 at p, this lane's dh 8 g .. and 32 + 8 g ..) as hi | lo B fragments
__device__ __forceinline__ void row_frags(const float* p, bf16x8_t& b0h, bf16x8_t& b0l, bf16x8_t& b1h, bf16x8_t& b1l) {
    u32x4_t h0, l0, h1, l1;
    split8(*(const f32x4_t*)p, *(const f32x4_t*)(p + 4), h0, l0);
    split8(*(const f32x4_t*)(p + 32), *(const f32x4_t*)(p + 36), h1, l1);
    b0h = __builtin_bit_cast(bf16x8_t, h0); b0l = __builtin_bit_cast(bf16x8_t, l0);
    b1h = __builtin_bit_cast(bf16x8_t, h1); b1l = __builtin_bit_cast(bf16x8_t, l1);
}

// the accumulators of two tiles -> hi | lo B fragments (pack8's k-slot order)
__device__ __forceinline__ void split_pack(const f32x4_t p0, const f32x4_t p1, bf16x8_t& bh, bf16x8_t& bl) {
    f32x4_t h0, l0, h1, l1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float hh, ll;
        split2(p0[e], hh, ll); h0[e] = hh; l0[e] = ll;
        split2(p1[e], hh, ll); h1[e] = hh; l1[e] = ll;
    }
    bh = pack8<false>(h0, h1);
    bl = pack8<false>(l0, l1);
}

// rows [0, n_rows) of two fp32 tensors (64 columns each from a / b, row pitches ld_a / ld_b) -> two swizzled image pairs;
// rows >= T are zero
__device__ __forceinline__ void fill_split_images(char* ah, char* al, const float* __restrict__ a, int64_t ld_a, char* bh, char* bl,
                                                  const float* __restrict__ b, int64_t ld_b, int n_rows, int T, int tid) {
    for (int idx = tid; idx < n_rows * 8; idx += 256) {
        const int r = idx >> 3, c = idx & 7;
        const int rc = r < T ? r : T - 1;
        const float* pa = a + rc * ld_a + c * 8;
        const float* pb = b + rc * ld_b + c * 8;
        u32x4_t xh, xl, yh, yl;
        split8(*(const f32x4_t*)pa, *(const f32x4_t*)(pa + 4), xh, xl);
        split8(*(const f32x4_t*)pb, *(const f32x4_t*)(pb + 4), yh, yl);
        const u32x4_t z = u32x4_t{0u, 0u, 0u, 0u};
        const bool ok = r < T;
        const int o = r * ATT_KROW + swz_chunk(c, r);
        *(u32x4_t*)(ah + o) = ok ? xh : z;
        *(u32x4_t*)(al + o) = ok ? xl : z;
        *(u32x4_t*)(bh + o) = ok ? yh : z;
        *(u32x4_t*)(bl + o) = ok ? yl : z;
    }
}

// ---------------------------------------------------------------------------
// pass A: dQ and the softmax statistics.  stats fp32 [rows, heads, 4] = {max * c, 1 / sum, delta, 0}
// ---------------------------------------------------------------------------
template <int MAXT>
__global__ __launch_bounds__(256) void attention_split_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dao,
                                                                     float* __restrict__ dqkv, float* __restrict__ stats, int T,
                                                                     int heads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int width = heads * ATT_DH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = xcd_contiguous(blockIdx.x, gridDim.x);
    const int seq = item / heads, h = item - seq * heads;
    const int64_t row0 = (int64_t)seq * T, ld = 3 * (int64_t)width;
    const int NT = (T + 15) >> 4, KT = NT * 16;
    char* ldsKh = smem;
    char* ldsKl = ldsKh + KT * ATT_KROW;
    char* ldsVh = ldsKl + KT * ATT_KROW;
    char* ldsVl = ldsVh + KT * ATT_KROW;
    const int g = lane >> 4, r16 = lane & 15;
    const int sw0 = swz_chunk(0 + g, lane), sw1 = swz_chunk(4 + g, lane);
    const float* base = qkv + row0 * ld + h * ATT_DH;
    fill_split_images(ldsKh, ldsKl, base + width, ld, ldsVh, ldsVl, base + 2 * width, ld, KT, T, tid);
    __syncthreads();

    const float scale_log2 = ATT_SCALE_LOG2;
    f32x4_t pen_tail;
#pragma unroll
    for (int r = 0; r < 4; ++r) pen_tail[r] = key_penalty((NT - 1) * 16 + 4 * g + r, T);
    for (int qb = wave; qb < NT; qb += 4) {
        const int qr = qb * 16 + r16;
        const int qrow = qr < T ? qr : T - 1;
        bf16x8_t q0h, q0l, q1h, q1l, d0h, d0l, d1h, d1l;
        row_frags(base + qrow * ld + 8 * g, q0h, q0l, q1h, q1l);
        row_frags(dao + (row0 + qrow) * (int64_t)width + h * ATT_DH + 8 * g, d0h, d0l, d1h, d1l);

        f32x4_t s[MAXT], dp[MAXT];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            dp[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (t < NT) {
                const f32x4_t c0 = (t == NT - 1) ? pen_tail : f32x4_t{0.f, 0.f, 0.f, 0.f};
                s[t] = rows_dot(ldsKh, ldsKl, t, r16, sw0, sw1, q0h, q0l, q1h, q1l, c0);
                dp[t] = rows_dot(ldsVh, ldsVl, t, r16, sw0, sw1, d0h, d0l, d1h, d1l, f32x4_t{0.f, 0.f, 0.f, 0.f});
                mx = fmaxf(mx, fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])));
            }
        }
        mx = group_max4(mx);
        const float mxs = mx * scale_log2;
        float lsum = 0.f, dl = 0.f;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < NT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = exp2f(fmaf(s[t][r], scale_log2, -mxs));
                    s[t][r] = p;
                    lsum += p;
                    dl = fmaf(p, dp[t][r], dl);
                }
            }
        }
        lsum = group_sum4(lsum);
        dl = group_sum4(dl);
        const float inv = 1.0f / lsum;
        const float delta = dl * inv;
        const float k8 = 0.125f * inv;
        // dS^T = P (dP - delta) / 8 as hi | lo, then dQ^T = K^T dS^T
        f32x4_t o[4];
#pragma unroll
        for (int md = 0; md < 4; ++md) o[md] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < (MAXT + 1) / 2; ++u) {
            const int t0 = 2 * u, t1 = 2 * u + 1;
            if (t0 < NT) {
                const bool pair = t1 < MAXT && t1 < NT;
                f32x4_t e0, e1 = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) e0[r] = s[t0][r] * k8 * (dp[t0][r] - delta);
                if (pair) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e1[r] = s[t1 < MAXT ? t1 : 0][r] * k8 * (dp[t1 < MAXT ? t1 : 0][r] - delta);
                }
                bf16x8_t sh, sl;
                split_pack(e0, e1, sh, sl);
                const int tt1 = pair ? t1 : t0;      // a tile without a partner multiplies its own rows by zeros
#pragma unroll
                for (int md = 0; md < 4; ++md) {
                    bf16x8_t ah, al;
                    tr_pair(ldsKh, ldsKl, t0, tt1, md, g, r16, ah, al);
                    o[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, sl, o[md], 0, 0, 0);
                    o[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, sh, o[md], 0, 0, 0);
                    o[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, sh, o[md], 0, 0, 0);
                }
            }
        }
        if (qr < T) {
            float* op = dqkv + (row0 + qr) * ld + h * ATT_DH + 4 * g;
#pragma unroll
            for (int md = 0; md < 4; ++md) *(f32x4_t*)(op + md * 16) = o[md];
            if (g == 0) *(f32x4_t*)(stats + ((row0 + qr) * heads + h) * 4) = f32x4_t{mxs, inv, delta, 0.f};
        }
    }
}

// ---------------------------------------------------------------------------
// pass B: dK, dV (lane = key; loops over all query tiles, two at a time)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_split_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dao,
                                                                      float* __restrict__ dqkv, const float* __restrict__ stats, int T,
                                                                      int heads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int width = heads * ATT_DH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = xcd_contiguous(blockIdx.x, gridDim.x);
    const int seq = item / heads, h = item - seq * heads;
    const int64_t row0 = (int64_t)seq * T, ld = 3 * (int64_t)width;
    const int NT = (T + 15) >> 4, NP = (NT + 1) >> 1, QR = NP * 32;
    char* ldsQh = smem;
    char* ldsQl = ldsQh + QR * ATT_KROW;
    char* ldsOh = ldsQl + QR * ATT_KROW;
    char* ldsOl = ldsOh + QR * ATT_KROW;
    float* ldsS = (float*)(ldsOl + QR * ATT_KROW);         // [QR][4] statistics per query
    const int g = lane >> 4, r16 = lane & 15;
    const int sw0 = swz_chunk(0 + g, lane), sw1 = swz_chunk(4 + g, lane);
    const float* base = qkv + row0 * ld + h * ATT_DH;
    fill_split_images(ldsQh, ldsQl, base, ld, ldsOh, ldsOl, dao + row0 * (int64_t)width + h * ATT_DH, width, QR, T, tid);
    for (int q = tid; q < QR; q += 256) {
        const f32x4_t st = *(const f32x4_t*)(stats + ((row0 + (q < T ? q : T - 1)) * heads + h) * 4);
        *(f32x4_t*)(ldsS + q * 4) = (q < T) ? st : f32x4_t{0.f, 0.f, 0.f, 0.f};         // inv = 0: padded queries give P = 0
    }
    __syncthreads();

    const float scale_log2 = ATT_SCALE_LOG2;
    for (int kb = wave; kb < NT; kb += 4) {
        const int kc = kb * 16 + r16;                    // this lane's key
        const bool kvalid = kc < T;
        const float* kp = base + (kvalid ? kc : T - 1) * ld + width + 8 * g;
        bf16x8_t k0h, k0l, k1h, k1l, v0h, v0l, v1h, v1l;
        row_frags(kp, k0h, k0l, k1h, k1l);
        row_frags(kp + width, v0h, v0l, v1h, v1l);
        f32x4_t dk[4], dv[4];
#pragma unroll
        for (int md = 0; md < 4; ++md) { dk[md] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dv[md] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
        for (int u = 0; u < NP; ++u) {
            f32x4_t pv[2], dsv[2];
#pragma unroll
            for (int w2 = 0; w2 < 2; ++w2) {
                const int tq = 2 * u + w2;               // query tile; rows beyond T are zero images with inv = 0
                const f32x4_t sc = rows_dot(ldsQh, ldsQl, tq, r16, sw0, sw1, k0h, k0l, k1h, k1l, f32x4_t{0.f, 0.f, 0.f, 0.f});
                const f32x4_t dp = rows_dot(ldsOh, ldsOl, tq, r16, sw0, sw1, v0h, v0l, v1h, v1l, f32x4_t{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x4_t st = *(const f32x4_t*)(ldsS + (tq * 16 + 4 * g + r) * 4);      // {m2, inv, delta}
                    float p = exp2f(fmaf(sc[r], scale_log2, -st[0])) * st[1];
                    p = kvalid ? p : 0.f;
                    pv[w2][r] = p;
                    dsv[w2][r] = p * 0.125f * (dp[r] - st[2]);
                }
            }
            bf16x8_t ph, pl, sh, sl;
            split_pack(pv[0], pv[1], ph, pl);
            split_pack(dsv[0], dsv[1], sh, sl);
#pragma unroll
            for (int md = 0; md < 4; ++md) {
                bf16x8_t ah, al;
                tr_pair(ldsOh, ldsOl, 2 * u, 2 * u + 1, md, g, r16, ah, al);
                dv[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pl, dv[md], 0, 0, 0);
                dv[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, ph, dv[md], 0, 0, 0);
                dv[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, ph, dv[md], 0, 0, 0);
                tr_pair(ldsQh, ldsQl, 2 * u, 2 * u + 1, md, g, r16, ah, al);
                dk[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, sl, dk[md], 0, 0, 0);
                dk[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, sh, dk[md], 0, 0, 0);
                dk[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, sh, dk[md], 0, 0, 0);
            }
        }
        if (kvalid) {
            float* ok = dqkv + (row0 + kc) * ld + width + h * ATT_DH + 4 * g;
#pragma unroll
            for (int md = 0; md < 4; ++md) {
                *(f32x4_t*)(ok + md * 16) = dk[md];
                *(f32x4_t*)(ok + width + md * 16) = dv[md];
            }
        }
    }
}

}  // namespace

// qkv fp32 [n_seq * T, 3 * width], dao fp32 [n_seq * T, width] -> dqkv fp32 [n_seq * T, 3 * width];
// stats_ws fp32 [n_seq * T, heads, 4] scratch
hipError_t launch_attention_split_bwd(const float* qkv, const float* dao, float* dqkv, float* stats_ws, int n_seq, int T, int heads,
                                      hipStream_t stream) {
    if (n_seq <= 0) return hipSuccess;
    if (T < 1 || T > 288 || heads < 1) return hipErrorInvalidValue;
    const int NT = (T + 15) / 16, NP = (NT + 1) / 2;
    const size_t lds_a = (size_t)NT * 16 * 4 * ATT_KROW;
    const size_t lds_b = (size_t)NP * 32 * (4 * ATT_KROW + 16);
    constexpr size_t MAX_LDS = 160 * 1024;
    const dim3 grid(n_seq * heads), block(256);
    const hipError_t st = NT > 4 ? launch<attention_split_bwd_dq_kernel<18>, MAX_LDS>(grid, block, lds_a, stream, qkv, dao, dqkv, stats_ws, T, heads)
                                 : launch<attention_split_bwd_dq_kernel<4>, MAX_LDS>(grid, block, lds_a, stream, qkv, dao, dqkv, stats_ws, T, heads);
    if (st != hipSuccess) return st;
    return launch<attention_split_bwd_dkv_kernel, MAX_LDS>(grid, block, lds_b, stream, qkv, dao, dqkv, stats_ws, T, heads);
}
