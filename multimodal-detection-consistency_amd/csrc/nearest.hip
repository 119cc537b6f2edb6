// The closest pair of a registered bank slot (similarity eviction, src/ref_bank.py:395-427: the most similar pair of stored
// vectors, which the reference finds with a double loop over i < j), as two kernels.
//
//   rows    `later_nearest_kernel`: partner[i] = the arg-max over the LATER rows j > i of cos(x_i, x_j), sim[i] = that cosine.
//           radius_tile_kernel's upper-triangle self-GEMM (gemm_core.hpp's main loop on slot_self_operands: a bf16 slot
//           multiplies one plane, an fp32 slot all four hi / lo products) oriented as kmeans_assign_kernel: the workgroup's own
//           256 rows i sit on the LANE dimension, the candidate partners j on the MFMA row dimension, so the running (best, j) of
//           a row is four register pairs per lane and no score ever leaves the accumulators.  The workgroup of row tile ti walks
//           the partner tiles tj = ti .. last only -- the reference's loop order and half the work; in the diagonal tile an
//           element counts only if j > i.  score = acc * rinv[j], rinv = 1 / |x| from an fp32 vector padded to whole tiles: 0 for a
//           zero row (the reference's _cosine_similarity returns 0.0 there), NaN for a row of non-finite norm and in the
//           padding -- NaN never wins cand_better.  The winner is multiplied by rinv[i] once at the end: a positive row scale
//           does not change the arg-max over j.  The four lane groups of a wave and the two wave rows that share a row i are
//           reduced once, after the last tile.  A row with no admissible partner (the last row, a row of non-finite norm, a row
//           all of whose later rows are non-finite) writes partner = -1, sim = -inf.
//   pair    `closest_pair_kernel`: one workgroup reduces (sim[i], i, partner[i]) under (sim desc, i asc) with select.hpp's
//           block_best.  Every row already holds its LOWEST best j, so the result is the first maximal pair in lexicographic
//           (i, j) order: the pair the reference's strict `similarity > max_similarity` keeps.
// Plain vector stores, no atomics, no floating-point reduction across workgroups: the outputs are a pure function of the slot.
#include "gemm_core.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "select.hpp"

#define NN_LDS_BYTES (GEMM_LDS_BYTES + 256 * 8)           // as KM_LDS_BYTES (kmeans.hip)

// in place: rinv[r] holds |x_r|^2 on entry (launch_kmeans_rownorm), r < R
__global__ __launch_bounds__(256) void nearest_rinv_kernel(float* __restrict__ rinv, int R, int rpad) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rpad) return;
    float v = __builtin_nanf("");
    if (r < R) {
        const float n2 = rinv[r];
        if (__builtin_isfinite(n2)) v = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
    }
    rinv[r] = v;
}

__global__ __launch_bounds__(GEMM_THREADS) void later_nearest_kernel(GemmOperands g, const float* __restrict__ rinv,
                                                                     int32_t* __restrict__ partner, float* __restrict__ sim, int R,
                                                                     int tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red_v = (float*)(smem + GEMM_LDS_BYTES);        // the bests of wave row 1, per own row of the tile
    int* red_i = (int*)(red_v + 256);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 2;
    // Row tile ti walks tiles - ti partner tiles, and workgroups start in the order of blockIdx.x: ti = blockIdx.x starts the
    // heaviest workgroups first, so the short ones fill the tail of the launch.
    const int ti = blockIdx.x;
    const int i0 = ti * GEMM_BN;
    int own[4];
    float bv[4];
    int bi[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { own[n] = gemm_acc_col(i0, wave, lane, n); bv[n] = -INFINITY; bi[n] = CAND_NONE; }
    for (int tj = ti; tj < tiles; ++tj) {
        gemm_acc_t acc;
        gemm_zero_acc(acc);
        // partners on the MFMA row dimension (A), own rows on the lane dimension (B)
        gemm_mainloop(acc, g, tj * GEMM_BM, i0, smem);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int c0 = gemm_acc_row(tj * GEMM_BM, wave, lane, m);
            const f32x4_t rj = *(const f32x4_t*)(rinv + c0);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = acc[m][n][r] * rj[r];
                    // j > i: only the diagonal tile has elements that fail it
                    if (c0 + r > own[n] && cand_better(s, c0 + r, bv[n], bi[n])) { bv[n] = s; bi[n] = c0 + r; }
                }
            }
        }
    }
    // the 4 lane groups of a wave, then the 2 wave rows, share an own row
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv[n], o, 64);
            const int oi = __shfl_xor(bi[n], o, 64);
            if (cand_better(ov, oi, bv[n], bi[n])) { bv[n] = ov; bi[n] = oi; }
        }
        const int il = gemm_acc_col(0, wave, lane, n);
        if (wm == 1 && (lane >> 4) == 0) { red_v[il] = bv[n]; red_i[il] = bi[n]; }
    }
    __syncthreads();
    if (wm == 0 && (lane >> 4) == 0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int il = gemm_acc_col(0, wave, lane, n);
            const int row = own[n];
            if (row >= R) continue;
            float v = bv[n];
            int j = bi[n];
            if (cand_better(red_v[il], red_i[il], v, j)) { v = red_v[il]; j = red_i[il]; }
            const float ri = rinv[row];
            // a row of non-finite norm has no partner, whatever its products came to
            const bool none = j == CAND_NONE || ri != ri;
            partner[row] = none ? -1 : j;
            sim[row] = none ? -INFINITY : v * ri;
        }
    }
}

__global__ __launch_bounds__(1024) void closest_pair_kernel(const int32_t* __restrict__ partner, const float* __restrict__ sim, int R,
                                                            int32_t* __restrict__ pair, float* __restrict__ pair_sim) {
    __shared__ BestSlots<1024, 1> red;
    Best<1> b;
    b.pay[0] = -1;
    for (int i = threadIdx.x; i < R; i += 1024) {
        const int j = partner[i];
        if (j < 0) continue;
        Best<1> o;
        o.v = sim[i]; o.id = i; o.pay[0] = j;
        best_take(b, o);
    }
    const Best<1> f = block_best<1024, 1>(b, red, 0);
    if (threadIdx.x == 0) {
        const bool none = f.id == CAND_NONE;
        pair[0] = none ? -1 : f.id;
        pair[1] = none ? -1 : f.pay[0];
        *pair_sim = none ? -INFINITY : f.v;
    }
}

hipError_t launch_closest_pair(const ClosestPairLaunch& L, hipStream_t stream) {
    const BankRows& B = L.bank;
    const NearestPlan& P = L.plan;
    if (!P.ok || B.R < 1 || B.R > NEAREST_MAX_ROWS || P.tiles != (B.R + GEMM_BM - 1) / GEMM_BM || P.rpad != (int64_t)P.tiles * GEMM_BM ||
        B.D < 64 || B.D % 64 != 0 || B.planes < 1 || B.planes > 2 || !L.rinv || !L.partner || !L.sim || !L.pair || !L.pair_sim)
        return hipErrorInvalidValue;
    const int R = (int)B.R;
    hipError_t st = launch_kmeans_rownorm(B, L.rinv, stream);
    if (st != hipSuccess) return st;
    st = launch<nearest_rinv_kernel>(dim3((unsigned)(P.rpad / 256)), dim3(256), 0, stream, L.rinv, R, (int)P.rpad);
    if (st != hipSuccess) return st;
    st = launch<later_nearest_kernel, NN_LDS_BYTES>(dim3((unsigned)P.tiles), dim3(GEMM_THREADS), NN_LDS_BYTES, stream,
                                                    slot_self_operands(B), (const float*)L.rinv, L.partner, L.sim, R, P.tiles);
    if (st != hipSuccess) return st;
    return launch<closest_pair_kernel>(dim3(1), dim3(1024), 0, stream, (const int32_t*)L.partner, (const float*)L.sim, R, L.pair,
                                       L.pair_sim);
}
