// Row kernels and attention of the split-bf16 tower mode (TVC_OPT_TOWER_PRECISION = 2; include/tvc.h): every fp32
// activation x travels to the matrix cores as TWO bf16 planes, hi = bf16(x) and lo = bf16(x - hi) (x = hi + lo to
// ~2^-17 relative), and every product a * b is formed as a_hi b_hi + a_hi b_lo + a_lo b_hi on v_mfma_f32_16x16x32_bf16
// with fp32 accumulation (the a_lo b_lo term is ~2^-18 of the result and is dropped): fp32-grade results at a third of
// the bf16 matrix rate instead of the 1/16 of the exact-f32 instruction (precise.hip).
//
// Plane layout of a GEMM operand: [rows, 2 * K] bf16, hi plane in columns 0 .. K-1, lo plane in K .. 2K-1 -- the
// GEMM's "planes" mechanism (gemm_core.hpp) addresses them as column offsets, so the tower GEMMs run on the same
// ring kernel as the bf16 mode with planes = 3.  split2 / split8 are common.hpp's; the row shape, the LayerNorm statistics and the GELU forms come from rows.hpp.
#include "attn_frag.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "rows.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm of the fp32 residual stream (+ up to two fp32 deltas: the previous store-only projections, folded in here
// as the bf16 tower's layernorm_kernel folds its bf16 ones) -> hi | lo planes [rows, 2d] and / or fp32 rows.
// One wave per row, d % 4 == 0, d <= 1024.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_split_kernel(float* __restrict__ x, int64_t x_row_stride, const int32_t* __restrict__ row_idx,
                                                       const float* __restrict__ d1, const float* __restrict__ d2, int write_x,
                                                       const float* __restrict__ g, const float* __restrict__ b,
                                                       uint16_t* __restrict__ planes, float* __restrict__ y32, int rows, int d) {
    const int lane = row_lane();
    const int row = wave_row();
    if (row >= rows) return;
    const int64_t src = row_idx ? (int64_t)row_idx[row] : (int64_t)row;
    f32x4_t* xr = (f32x4_t*)(x + src * x_row_stride);
    const f32x4_t* p1 = d1 ? (const f32x4_t*)(d1 + src * x_row_stride) : nullptr;
    const f32x4_t* p2 = d2 ? (const f32x4_t*)(d2 + src * x_row_stride) : nullptr;
    const int nv = d >> 2;
    f32x4_t v[4] = {};
    float s = 0.f;
    for_pieces(lane, nv, [&](int i, int c) {
        v[i] = xr[c];
        if (p1) v[i] += p1[c];
        if (p2) v[i] += p2[c];
        if (write_x && (p1 || p2)) xr[c] = v[i];
        s += piece_sum(v[i]);
    });
    const float mean = row_mean(s, d);
    const float rstd = row_rstd<true>(v, mean, lane, nv, d);      // IEEE sqrt and division: this mode's bits are under contract
    for_pieces(lane, nv, [&](int i, int c) {
        const f32x4_t o = ln_affine(v[i], mean, rstd, g, b, c);
        if (y32) ((f32x4_t*)(y32 + (int64_t)row * d))[c] = o;
        if (planes) {
            float h[4], l[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) split2(o[t], h[t], l[t]);
            uint16_t* pr = planes + (int64_t)row * 2 * d + c * 4;
            *(u32x2_t*)pr = u32x2_t{pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3])};
            *(u32x2_t*)(pr + d) = u32x2_t{pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3])};
        }
    });
}

// fp32 rows [rows, ld_in] (first K columns used) -> planes [rows, 2 * Kp], zero padded from K to Kp; gelu 1 applies
// QuickGELU x * sigmoid(1.702 x) first (exact expf and division, as the fp32 CPU path), gelu 2 the erf GELU.
// K % 4 == 0, Kp % 4 == 0.
__global__ __launch_bounds__(256) void rows_split_kernel(const float* __restrict__ x, int64_t ld_in, uint16_t* __restrict__ out,
                                                         int64_t rows, int K, int Kp, int gelu) {
    const int nv = Kp >> 2;
    const int64_t total = rows * nv;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / nv;
        const int c = (int)(t - r * nv);
        f32x4_t v = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (c * 4 < K) v = __builtin_nontemporal_load((const f32x4_t*)(x + r * ld_in) + c);
        float h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float u = v[e];
            if (gelu == 1) u = quick_gelu_exact(u);
            else if (gelu == 2) u = gelu_erf(u);
            split2(u, h[e], l[e]);
        }
        uint16_t* o = out + r * (int64_t)(2 * Kp) + c * 4;
        *(u32x2_t*)o = u32x2_t{pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3])};
        *(u32x2_t*)(o + Kp) = u32x2_t{pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3])};
    }
}

// fp32 W [I, ld] (first K columns used) -> planes of W^T: out [*, 2 * Ip] bf16, row k = (hi | lo) of W[0 .. I-1][k] (the A
// operand of the split-bf16 gradient's dX GEMMs).  Writes rows k < K, columns i < I of each plane only: the caller zeroes the
// padding (rows up to the GEMM's row tile, columns I .. Ip).  32 x 32 tiles through LDS, 256 threads.
__global__ __launch_bounds__(256) void rows_split_t_kernel(const float* __restrict__ w, int64_t ld, uint16_t* __restrict__ out, int I,
                                                           int K, int Ip) {
    __shared__ float tile[32][33];
    const int k0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    for (int j = ty; j < 32; j += 8)
        if (i0 + j < I && k0 + tx < K) tile[j][tx] = w[(int64_t)(i0 + j) * ld + k0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        if (k0 + j < K && i0 + tx < I) {
            float hi, lo;
            split2(tile[tx][j], hi, lo);
            uint16_t* o = out + (int64_t)(k0 + j) * (2 * Ip) + i0 + tx;
            o[0] = f32_to_bf16_bits(hi);
            o[Ip] = f32_to_bf16_bits(lo);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Attention on split operands: qkv fp32 [rows, 3 * width] (q | k | v) -> out planes [rows, 2 * width].
// Structure of attention.hip's kernel (one workgroup of 4 waves per (sequence, head); K and V of the head in LDS,
// "swapped" products S^T = K Q^T and O^T = V^T P^T so that softmax statistics are per-lane scalars; exact single-pass
// softmax), with K, V, Q and the probabilities each held as hi | lo bf16 and three MFMAs per product:
//   S = K_hi Q_lo + K_lo Q_hi + K_hi Q_hi,   O = V_hi P_lo + V_lo P_hi + V_hi P_hi   (small terms first)
// The probabilities are exp2 of fp32 scores, their row sum is taken in fp32 over the un-rounded values.
// Ragged / prefix-sharing sequences as attention.hip (SeqView; the lane maps and fragments are attn_frag.hpp's).
// LDS: 2 x KT x 128 B + 2 x KT x 160 B (T = 257: 156 672 B, one workgroup per CU).
// ---------------------------------------------------------------------------------------------------------------

template <int MAXT, bool CAUSAL>
__global__ __launch_bounds__(256) void attention_split_kernel(const float* __restrict__ qkv, uint16_t* __restrict__ out,
                                                              const int32_t* __restrict__ starts, int T_fixed, int heads,
                                                              int n_items, int kt_alloc, const int32_t* __restrict__ pfx, int n_seq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int width = heads * ATT_DH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = xcd_contiguous(blockIdx.x, gridDim.x);
    if (item >= n_items) return;
    const int seq = item / heads, h = item - seq * heads;
    // SeqView's decode, in its own text: through the constructor the <2> and <6> forms' registers are allocated differently (EXPERIMENTS.md)
    int64_t row0, prow0 = 0;
    int T, P = 0;
    if (starts) {
        const int s0 = __builtin_amdgcn_readfirstlane(starts[seq]);
        const int s1 = __builtin_amdgcn_readfirstlane(starts[seq + 1]);
        row0 = s0; T = s1 - s0;
        if (CAUSAL && pfx) {
            P = __builtin_amdgcn_readfirstlane(pfx[seq]);
            prow0 = __builtin_amdgcn_readfirstlane(pfx[n_seq + seq]);
            T += P;
        }
    } else { row0 = (int64_t)seq * T_fixed; T = T_fixed; }
    auto key_row = [&](int t) -> int64_t { return t < P ? prow0 + t : row0 + (t - P); };
    if (T > MAXT * 16) T = MAXT * 16;
    const int NT = (T + 15) >> 4, KT = NT * 16;
    char* ldsKh = smem;
    char* ldsKl = ldsKh + kt_alloc * ATT_KROW;
    char* ldsVh = ldsKl + kt_alloc * ATT_KROW;
    char* ldsVl = ldsVh + kt_alloc * ATT_VROW;
    const int64_t ld = 3 * (int64_t)width;
    const int g = lane >> 4, r16 = lane & 15;
    const int sw0 = swz_chunk(0 + g, lane), sw1 = swz_chunk(4 + g, lane);
    const int tr_off = tr_lane_off<ATT_VROW>(g, r16);
    const float scale_log2 = ATT_SCALE_LOG2;
    const int own = T - P;
    const int NQ = (own + 15) >> 4;

    // ---- fill: 8 fp32 (two 16-byte loads) -> one hi piece + one lo piece; zero rows beyond T
    for (int idx = tid; idx < KT * 8; idx += 256) {
        const int key = idx >> 3, c = idx & 7;
        const float* src = qkv + key_row(key < T ? key : T - 1) * ld + h * ATT_DH + c * 8;
        const f32x4_t k0 = *(const f32x4_t*)(src + width), k1 = *(const f32x4_t*)(src + width + 4);
        const f32x4_t v0 = *(const f32x4_t*)(src + 2 * width), v1 = *(const f32x4_t*)(src + 2 * width + 4);
        u32x4_t kh, kl, vh, vl;
        split8(k0, k1, kh, kl);
        split8(v0, v1, vh, vl);
        const u32x4_t z = u32x4_t{0u, 0u, 0u, 0u};
        const bool ok = key < T;
        const int ko = key * ATT_KROW + swz_chunk(c, key), vo = key * ATT_VROW + (c << 4);
        *(u32x4_t*)(ldsKh + ko) = ok ? kh : z;
        *(u32x4_t*)(ldsKl + ko) = ok ? kl : z;
        *(u32x4_t*)(ldsVh + vo) = ok ? vh : z;
        *(u32x4_t*)(ldsVl + vo) = ok ? vl : z;
    }
    __syncthreads();

    f32x4_t pen_tail;
#pragma unroll
    for (int r = 0; r < 4; ++r) pen_tail[r] = key_penalty((NT - 1) * 16 + 4 * g + r, T);

    for (int qb = wave; qb < NQ; qb += 4) {
        const int qr = qb * 16 + r16;
        const int qrow = qr < own ? qr : own - 1;
        const float* qp = qkv + (row0 + qrow) * ld + h * ATT_DH + 8 * g;
        u32x4_t q0h, q0l, q1h, q1l;
        split8(*(const f32x4_t*)qp, *(const f32x4_t*)(qp + 4), q0h, q0l);
        split8(*(const f32x4_t*)(qp + 32), *(const f32x4_t*)(qp + 36), q1h, q1l);
        const bf16x8_t bq0h = __builtin_bit_cast(bf16x8_t, q0h), bq0l = __builtin_bit_cast(bf16x8_t, q0l);
        const bf16x8_t bq1h = __builtin_bit_cast(bf16x8_t, q1h), bq1l = __builtin_bit_cast(bf16x8_t, q1l);
        const int qmin = P + qb * 16, qmax = qmin + 15, qpos = P + qr;
        const int nt_q = SeqView<CAUSAL>::nt_q(qmax, NT);

        f32x4_t s[MAXT];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (t < nt_q) {
                f32x4_t c0 = (t == NT - 1) ? pen_tail : f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (CAUSAL && t * 16 + 15 > qmin) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (SeqView<CAUSAL>::hidden(t * 16 + 4 * g + r, qpos)) c0[r] = -INFINITY;
                }
                const int ro = (t * 16 + r16) * ATT_KROW;
                const bf16x8_t a0h = *(const bf16x8_t*)(ldsKh + ro + sw0), a1h = *(const bf16x8_t*)(ldsKh + ro + sw1);
                const bf16x8_t a0l = *(const bf16x8_t*)(ldsKl + ro + sw0), a1l = *(const bf16x8_t*)(ldsKl + ro + sw1);
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0h, bq0l, c0, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1h, bq1l, c0, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0l, bq0h, c0, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1l, bq1h, c0, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0h, bq0h, c0, 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1h, bq1h, c0, 0, 0, 0);
                mx = fmaxf(mx, fmaxf(fmaxf(s[t][0], s[t][1]), fmaxf(s[t][2], s[t][3])));
            }
        }
        mx = group_max4(mx);
        const float mxs = mx * scale_log2;
        float lsum = 0.f;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt_q) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[t][r] = exp2f(fmaf(s[t][r], scale_log2, -mxs));
                    lsum += s[t][r];
                }
            }
        }
        lsum = group_sum4(lsum);

        f32x4_t o[4];
#pragma unroll
        for (int md = 0; md < 4; ++md) o[md] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < (MAXT + 1) / 2; ++u) {
            const int t0 = 2 * u, t1 = 2 * u + 1;
            if (t0 < nt_q) {
                // k-slots j < 4: keys 16 t0 + 4g + j; j >= 4: keys 16 t1 + 4g + (j - 4).  An unpaired last tile multiplies
                // its own V rows by zero probabilities (no zero partner rows in LDS).
                const bool pair = t1 < nt_q;
                const f32x4_t p0 = s[t0];
                const f32x4_t p1 = (t1 < MAXT && pair) ? s[t1 < MAXT ? t1 : 0] : f32x4_t{0.f, 0.f, 0.f, 0.f};
                f32x4_t ph0, pl0, ph1, pl1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float hh, ll;
                    split2(p0[e], hh, ll); ph0[e] = hh; pl0[e] = ll;
                    split2(p1[e], hh, ll); ph1[e] = hh; pl1[e] = ll;
                }
                const bf16x8_t pbh = pack8<false>(ph0, ph1), pbl = pack8<false>(pl0, pl1);
                const int tt1 = pair ? t1 : t0;
#pragma unroll
                for (int md = 0; md < 4; ++md) {
                    const int o0 = tr_off + md * 32 + t0 * 16 * ATT_VROW, o1 = tr_off + md * 32 + tt1 * 16 * ATT_VROW;
                    const bf16x4_t h0 = tr16_read(ldsVh + o0), h1 = tr16_read(ldsVh + o1), l0 = tr16_read(ldsVl + o0), l1 = tr16_read(ldsVl + o1);
                    const bf16x8_t ah = join8<false>(h0, h1), al = join8<false>(l0, l1);
                    o[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pbl, o[md], 0, 0, 0);
                    o[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, pbh, o[md], 0, 0, 0);
                    o[md] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pbh, o[md], 0, 0, 0);
                }
            }
        }
        const float inv = 1.0f / lsum;
        if (qr < own) {
            uint16_t* op = out + (row0 + qr) * (int64_t)(2 * width) + h * ATT_DH + 4 * g;
#pragma unroll
            for (int md = 0; md < 4; ++md) {
                float hh[4], ll[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split2(o[md][e] * inv, hh[e], ll[e]);
                *(u32x2_t*)(op + md * 16) = u32x2_t{pack_bf16x2(hh[0], hh[1]), pack_bf16x2(hh[2], hh[3])};
                *(u32x2_t*)(op + md * 16 + width) = u32x2_t{pack_bf16x2(ll[0], ll[1]), pack_bf16x2(ll[2], ll[3])};
            }
        }
    }
}

template <int MAXT, bool CAUSAL>
hipError_t launch_split_one(const float* qkv, uint16_t* out, const int32_t* starts, int n_seq, int T, int heads,
                            hipStream_t stream, const int32_t* pfx) {
    const int kt = (T + 15) / 16 * 16;
    const size_t lds = (size_t)kt * (2 * ATT_KROW + 2 * ATT_VROW);
    const int n_items = n_seq * heads;
    return launch<attention_split_kernel<MAXT, CAUSAL>, 160 * 1024>(dim3(n_items), dim3(256), lds, stream, qkv, out, starts, T, heads,
                                                                    n_items, kt, pfx, n_seq);
}

}  // namespace

hipError_t launch_ln_split(float* x, int64_t x_row_stride, const int32_t* row_idx, const float* d1, const float* d2, int write_x,
                           const float* g, const float* b, uint16_t* planes, float* y32, int rows, int d, hipStream_t stream) {
    if (d % 4 != 0 || d > 1024 || rows < 0 || (!planes && !y32)) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return launch<ln_split_kernel>(row_grid(rows), dim3(256), 0, stream, x, x_row_stride, row_idx, d1, d2, write_x, g, b, planes,
                                   y32, rows, d);
}

hipError_t launch_rows_split(const float* x, int64_t ld_in, uint16_t* out, int64_t rows, int K, int Kp, int gelu, hipStream_t stream) {
    if (K % 4 != 0 || Kp % 4 != 0 || Kp < K || rows < 0) return hipErrorInvalidValue;
    if (rows == 0) return hipSuccess;
    return launch<rows_split_kernel>(stride_grid(rows * (Kp >> 2), 32768), dim3(256), 0, stream, x, ld_in, out, rows, K, Kp, gelu);
}

hipError_t launch_rows_split_t(const float* w, int64_t ld, uint16_t* out, int I, int K, int Ip, hipStream_t stream) {
    if (I < 1 || K < 1 || Ip < I || ld < K || (I + 31) / 32 > 65535) return hipErrorInvalidValue;
    return launch<rows_split_t_kernel>(dim3((K + 31) / 32, (I + 31) / 32), dim3(256), 0, stream, w, ld, out, I, K, Ip);
}

// starts == nullptr: n_seq sequences of seq_len rows; else packed rows (+ pfx: shared prefixes), seq_len = the maximum
hipError_t launch_attention_split(const float* qkv, uint16_t* out, const int32_t* starts, int n_seq, int seq_len, int heads,
                                  int causal, hipStream_t stream, const int32_t* pfx) {
    if (n_seq <= 0) return hipSuccess;
    // K / V of a head as hi | lo images: 576 bytes per key row, 160 KB of LDS -> 272 keys (17 tiles: the 257 tokens of ViT-L/14)
    if (seq_len < 1 || seq_len > 272 || heads < 1 || (pfx && (!starts || !causal))) return hipErrorInvalidValue;
    const int NT = (seq_len + 15) / 16;
    if (causal) {
        if (NT <= 2) return launch_split_one<2, true>(qkv, out, starts, n_seq, seq_len, heads, stream, pfx);
        if (NT <= 6) return launch_split_one<6, true>(qkv, out, starts, n_seq, seq_len, heads, stream, pfx);
        return launch_split_one<18, true>(qkv, out, starts, n_seq, seq_len, heads, stream, pfx);
    }
    if (NT <= 2) return launch_split_one<2, false>(qkv, out, starts, n_seq, seq_len, heads, stream, nullptr);
    if (NT <= 6) return launch_split_one<6, false>(qkv, out, starts, n_seq, seq_len, heads, stream, nullptr);
    return launch_split_one<18, false>(qkv, out, starts, n_seq, seq_len, heads, stream, nullptr);
}
