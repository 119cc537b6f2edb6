// What the GEMM-tile passes over a bank slot share beyond the main loop (gemm_core.hpp): the running arg-max of a lane's four
// columns over the tiles a workgroup walks (kmeans.hip, nearest.hip), and the padded per-row fp32 vector such a pass reads
// 16 bytes at a time (dbscan.hip, nearest.hip).  Included by the .hip files only.
#pragma once
#include "gemm_core.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "select.hpp"

// the main loop's LDS, then the bests of wave row 1 per column of the tile: 256 values, 256 ids
#define SLOT_BEST_LDS_BYTES (GEMM_LDS_BYTES + 256 * 8)

// The best (score, candidate) of each of the lane's four columns (gemm_acc_col: n = 0 .. 3), candidates on the MFMA row
// dimension.  The order is cand_better (score desc, id asc): a NaN score never wins, and a column nothing was taken for ends
// as (-inf, CAND_NONE).
struct SlotBest {
    float v[4];
    int id[4];

    __device__ __forceinline__ SlotBest() {
#pragma unroll
        for (int n = 0; n < 4; ++n) { v[n] = -INFINITY; id[n] = CAND_NONE; }
    }

    // One tile whose first candidate row is t0.  vec is the candidates' fp32 vector, readable in whole 16-byte pieces up to the
    // end of the tile; score(acc value, vec element, candidate, n, &s) sets the element's score s and returns whether the
    // element is admitted.
    template <class Score>
    __device__ __forceinline__ void take(const gemm_acc_t& acc, const float* __restrict__ vec, int t0, int wave, int lane, Score score) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int c0 = gemm_acc_row(t0, wave, lane, m);
            const f32x4_t x = *(const f32x4_t*)(vec + c0);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s;
                    if (score(acc[m][n][r], x[r], c0 + r, n, s) && cand_better(s, c0 + r, v[n], id[n])) { v[n] = s; id[n] = c0 + r; }
                }
            }
        }
    }

    // After the last tile, once per workgroup and by every thread: the 4 lane groups of a wave, then the 2 wave rows, share a
    // column.  Wave row 1 hands its bests over behind the main loop's LDS; wave row 0, lane group 0 then calls
    // store(tile-local column, score, id) for each of its four columns.
    template <class Store>
    __device__ __forceinline__ void finish(char* smem, int wave, int lane, Store store) {
        float* red_v = (float*)(smem + GEMM_LDS_BYTES);
        int* red_i = (int*)(red_v + 256);
        const int wm = wave >> 2;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ov = __shfl_xor(v[n], o, 64);
                const int oi = __shfl_xor(id[n], o, 64);
                if (cand_better(ov, oi, v[n], id[n])) { v[n] = ov; id[n] = oi; }
            }
            const int cl = gemm_acc_col(0, wave, lane, n);
            if (wm == 1 && (lane >> 4) == 0) { red_v[cl] = v[n]; red_i[cl] = id[n]; }
        }
        __syncthreads();
        if (wm == 0 && (lane >> 4) == 0) {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int cl = gemm_acc_col(0, wave, lane, n);
                float bv = v[n];
                int bi = id[n];
                if (cand_better(red_v[cl], red_i[cl], bv, bi)) { bv = red_v[cl]; bi = red_i[cl]; }
                store(cl, bv, bi);
            }
        }
    }
};

// in place: v[r] holds |x_r|^2 on entry, r < R
template <class F>
__global__ __launch_bounds__(256) void slot_row_vector_kernel(float* __restrict__ v, int R, int pad, F f) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= pad) return;
    float out = __builtin_nanf("");
    if (r < R) {
        const float n2 = v[r];
        if (__builtin_isfinite(n2)) out = f(n2);
    }
    v[r] = out;
}

// v[r] = f(|x_r|^2) of the slot's stored rows, r < R; NaN for a row whose norm is not finite and for the padding R <= r < pad
template <class F>
hipError_t launch_slot_row_vector(const BankRows& bank, float* v, int64_t pad, F f, hipStream_t stream) {
    const hipError_t st = launch_kmeans_rownorm(bank, v, stream);
    if (st != hipSuccess) return st;
    return launch<slot_row_vector_kernel<F>>(dim3((unsigned)((pad + 255) / 256)), dim3(256), 0, stream, v, (int)bank.R, (int)pad, f);
}
