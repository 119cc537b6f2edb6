// The closest pair of a registered bank slot (similarity eviction, src/ref_bank.py:395-427: the most similar pair of stored
// vectors, which the reference finds with a double loop over i < j), as two kernels.
//
//   rows    `later_nearest_kernel`: partner[i] = the arg-max over the LATER rows j > i of cos(x_i, x_j), sim[i] = that cosine.
//           An upper-triangle self-GEMM (gemm_core.hpp's main loop on slot_self_operands: a bf16 slot multiplies one plane, an
//           fp32 slot all four hi / lo products): the workgroup's own 256 rows i sit on the LANE dimension, the candidate
//           partners j on the MFMA row dimension, and slot_tile.hpp's SlotBest keeps each row's running (best, j).  The
//           workgroup of row tile ti walks the partner tiles tj = ti .. last only -- the reference's loop order and half the
//           work; in the diagonal tile an element counts only if j > i.  score = acc * rinv[j], rinv = 1 / |x| from an fp32
//           vector padded to whole tiles: 0 for a zero row (the reference's _cosine_similarity returns 0.0 there), NaN for a row
//           of non-finite norm and in the padding.  The winner is multiplied by rinv[i] once at the end: a positive row scale
//           does not change the arg-max over j.  A row with no admissible partner (the last row, a row of non-finite norm, a row
//           all of whose later rows are non-finite) writes partner = -1, sim = -inf.
//   pair    `closest_pair_kernel`: one workgroup reduces (sim[i], i, partner[i]) under (sim desc, i asc) with select.hpp's
//           block_best.  Every row already holds its LOWEST best j, so the result is the first maximal pair in lexicographic
//           (i, j) order: the pair the reference's strict `similarity > max_similarity` keeps.
// Plain vector stores, no atomics, no floating-point reduction across workgroups: the outputs are a pure function of the slot.
#include "slot_tile.hpp"

// rinv from |x|^2 (launch_slot_row_vector)
struct NearestRinv {
    __device__ __forceinline__ float operator()(float n2) const { return n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f; }
};

__global__ __launch_bounds__(GEMM_THREADS) void later_nearest_kernel(GemmOperands g, const float* __restrict__ rinv,
                                                                     int32_t* __restrict__ partner, float* __restrict__ sim, int R,
                                                                     int tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // Row tile ti walks tiles - ti partner tiles, and workgroups start in the order of blockIdx.x: ti = blockIdx.x starts the
    // heaviest workgroups first, so the short ones fill the tail of the launch.
    const int ti = blockIdx.x;
    const int i0 = ti * GEMM_BN;
    int own[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) own[n] = gemm_acc_col(i0, wave, lane, n);
    SlotBest best;
    for (int tj = ti; tj < tiles; ++tj) {
        gemm_acc_t acc;
        gemm_zero_acc(acc);
        // partners on the MFMA row dimension (A), own rows on the lane dimension (B)
        gemm_mainloop(acc, g, tj * GEMM_BM, i0, smem);
        // j > i: only the diagonal tile has elements that fail it
        best.take(acc, rinv, tj * GEMM_BM, wave, lane, [&](float a, float rj, int j, int n, float& s) {
            s = a * rj;
            return j > own[n];
        });
    }
    best.finish(smem, wave, lane, [&](int il, float v, int j) {
        const int row = i0 + il;
        if (row >= R) return;
        const float ri = rinv[row];
        // a row of non-finite norm has no partner, whatever its products came to
        const bool none = j == CAND_NONE || ri != ri;
        partner[row] = none ? -1 : j;
        sim[row] = none ? -INFINITY : v * ri;
    });
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
    if (!P.ok || !slot_tile_ok(B, NEAREST_MAX_ROWS) || P.tiles != (B.R + GEMM_BM - 1) / GEMM_BM || P.rpad != (int64_t)P.tiles * GEMM_BM ||
        !L.rinv || !L.partner || !L.sim || !L.pair || !L.pair_sim)
        return hipErrorInvalidValue;
    const int R = (int)B.R;
    hipError_t st = launch_slot_row_vector(B, L.rinv, P.rpad, NearestRinv{}, stream);
    if (st != hipSuccess) return st;
    st = launch<later_nearest_kernel, SLOT_BEST_LDS_BYTES>(dim3((unsigned)P.tiles), dim3(GEMM_THREADS), SLOT_BEST_LDS_BYTES, stream,
                                                           slot_self_operands(B), (const float*)L.rinv, L.partner, L.sim, R, P.tiles);
    if (st != hipSuccess) return st;
    return launch<closest_pair_kernel>(dim3(1), dim3(1024), 0, stream, (const int32_t*)L.partner, (const float*)L.sim, R, L.pair,
                                       L.pair_sim);
}
