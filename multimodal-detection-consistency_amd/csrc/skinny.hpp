// ---------------------------------------------------------------------------------------------------------------
// The skinny stream, shared by bank_filter_skinny_kernel and bank_sample_skinny_kernel (bank.hip, M <= 64) and by
// ivf_scan_kernel (ivf.hip, <= 64 (query, probe) pairs of one list): bank rows go ONCE from memory into MFMA operand
// registers and are multiplied with 16 * NQT query columns held in LDS.
//   * each of a workgroup's 8 waves walks its own 16-row groups (grp = wave, wave + 8, ...): all D / 64 x 2 sixteen-byte
//     pieces of a group are requested before the previous group is multiplied (two register sets: ~50 KB of loads in
//     flight per wave, 400 KB per CU -- latency is covered by bytes, not by occupancy);
//   * a lane (row r16 = lane & 15, k-group g = lane >> 4) loads the 32 contiguous bytes [g * 32, g * 32 + 32) of every
//     128-byte line of its row: the two MFMAs of a 64-deep block take k = 64 kb + 16 g + {0..7} and {8..15} -- any
//     k permutation is a valid inner product as long as the query fragments use the same one (they do: the LDS image of
//     the queries is read with the same offsets);
//   * queries: QP planes (hi, or hi | lo) of 16 * NQT rows, [D * QP] bf16 per row in LDS, row pitch D * 2 * QP + 16 bytes
//     (16 lanes of a ds_read_b128 group hit 16 distinct 16-byte bank groups: conflict-free); rows >= M are zeros.
// The kernels supply the row address of a group, what is done with its accumulators, and their own copy of the queries to
// LDS (a rolled loop in the filter kernel, six pieces deep in the latency-bound sample kernel: EXPERIMENTS.md).
// ---------------------------------------------------------------------------------------------------------------
#pragma once
#include "common.hpp"

// the lane's 2 * KB pieces of one row; src = the row + g * 16 elements.  NT: non-temporal (a row that is read once)
template <int KB, bool NT>
__device__ __forceinline__ void skinny_load_group(const uint16_t* src, u32x4_t (&a)[2 * KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        if (NT) {
            a[2 * kb] = __builtin_nontemporal_load((const u32x4_t*)(src + kb * 64));
            a[2 * kb + 1] = __builtin_nontemporal_load((const u32x4_t*)(src + kb * 64 + 8));
        } else {
            a[2 * kb] = *(const u32x4_t*)(src + kb * 64);
            a[2 * kb + 1] = *(const u32x4_t*)(src + kb * 64 + 8);
        }
    }
}
// acc[n] += the group's 16 rows x the queries n * 16 .. n * 16 + 15, the products of the first QP planes of an LDS image of
// row pitch QPITCH bytes; qbase = the LDS image + r16 * QPITCH + g * 32.  FENCE: a scheduling barrier per 64-deep block
template <int KB, int NQT, int QP, int QPITCH, bool FENCE>
__device__ __forceinline__ void skinny_mfma_acc(const u32x4_t (&a)[2 * KB], const char* qbase, f32x4_t (&acc)[NQT]) {
    constexpr int D = KB * 64;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const bf16x8_t af = __builtin_bit_cast(bf16x8_t, a[2 * kb + hf]);
#pragma unroll
            for (int n = 0; n < NQT; ++n) {
                const char* qp = qbase + n * 16 * QPITCH + kb * 128 + hf * 16;
#pragma unroll
                for (int p = 0; p < QP; ++p)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, *(const bf16x8_t*)(qp + p * 2 * D), acc[n], 0, 0, 0);
            }
        }
        if (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
}
// as skinny_mfma_acc, but every 64-deep block is summed in an accumulator of its own that starts at zero and is then added to
// acc[n] by the vector ALU.  The matrix pipe does not round its running sum to nearest: over one accumulator chain of 4 D / 32
// MFMAs, rows whose products are mostly of one sign (a query near its bank row, |q||x| in the hundreds) ended 1.2e-6 |q||x|
// off fp64; a chain of 2 QP MFMAs per block and KB rounded additions stays a few 1e-7 off.  For kernels whose accumulators
// ARE the result (ivf_scan_kernel); the filter kernels of bank.hip re-score what they list.
template <int KB, int NQT, int QP, int QPITCH>
__device__ __forceinline__ void skinny_mfma_blocks(const u32x4_t (&a)[2 * KB], const char* qbase, f32x4_t (&acc)[NQT]) {
    constexpr int D = KB * 64;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        const bf16x8_t af0 = __builtin_bit_cast(bf16x8_t, a[2 * kb]), af1 = __builtin_bit_cast(bf16x8_t, a[2 * kb + 1]);
#pragma unroll
        for (int n = 0; n < NQT; ++n) {                       // one block accumulator alive at a time
            const char* qp = qbase + n * 16 * QPITCH + kb * 128;
            f32x4_t t = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < QP; ++p) {
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af0, *(const bf16x8_t*)(qp + p * 2 * D), t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af1, *(const bf16x8_t*)(qp + 16 + p * 2 * D), t, 0, 0, 0);
            }
            acc[n] += t;
            asm volatile("" : "+v"(acc[n]));                    // the sum exists before the next block starts
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// acc[n] = the group's 16 rows x the queries n * 16 .. n * 16 + 15, the products of the QP planes summed into one accumulator;
// the LDS image holds exactly the QP planes (row pitch D * 2 * QP + 16 bytes)
template <int KB, int NQT, int QP, bool FENCE>
__device__ __forceinline__ void skinny_mfma(const u32x4_t (&a)[2 * KB], const char* qbase, f32x4_t (&acc)[NQT]) {
#pragma unroll
    for (int n = 0; n < NQT; ++n) acc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    skinny_mfma_acc<KB, NQT, QP, KB * 64 * 2 * QP + 16, FENCE>(a, qbase, acc);
}
// the walk of a wave over its groups from `grp` on, whose pieces are already requested into a0: group i + 8 is in flight
// while group i is multiplied
template <int N, class Load, class Compute>
__device__ __forceinline__ void skinny_walk(int grp, int n_groups, u32x4_t (&a0)[N], u32x4_t (&a1)[N], Load&& load, Compute&& compute) {
    while (grp < n_groups) {
        if (grp + 8 < n_groups) load(grp + 8, a1);
        compute(grp, a0);
        grp += 8;
        if (grp >= n_groups) break;
        if (grp + 8 < n_groups) load(grp + 8, a0);
        compute(grp, a1);
        grp += 8;
    }
}
