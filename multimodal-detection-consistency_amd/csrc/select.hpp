// Device code only: "k rounds of block arg-max by (value desc, id asc)" and the block-wide exclusive scan, written once for
// bank_select_kernel and row_topk_kernel (bank.hip), the two selects of ivf.hip, kmeans_offsets_kernel (kmeans.hip),
// dbscan_roots_kernel (dbscan.hip) and, with 64-bit sums, pair_scan_kernel (pairs.hip).
// A round: every thread scans the elements it owns into a Best (WHAT it admits stays with the kernel: they differ), block_best()
// gives every thread the block's best after ONE barrier, thread 0 writes it out and the thread that owns the winning element
// strikes it -- the only thread that ever reads it again, so nothing has to order the two.
#pragma once
#include "common.hpp"

#define CAND_NONE 0x7fffffff      // the id of "no candidate": above every id in cand_better's order

// the best candidate so far: (v, id) in cand_better's order plus NP ints that travel with it (a pool slot, a position)
template <int NP>
struct Best {
    float v = -INFINITY;
    int id = CAND_NONE;
    int pay[NP];
};
// The take rule is cand_better alone: against the empty (-inf, CAND_NONE) a candidate with v > -inf wins, one with v == -inf
// wins by its id and a NaN never does; an empty `o` beats nothing.
template <int NP>
__device__ __forceinline__ void best_take(Best<NP>& b, const Best<NP>& o) {
    if (cand_better(o.v, o.id, b.v, b.id)) b = o;
}
// all-lane best over groups of W lanes, xor distances W / 2 ... 1.  With distinct ids the order is total and the winner does
// not depend on this shape; among equal (v, id) pairs (a list probed twice) it decides whose payload is struck first.
template <int W, int NP>
__device__ __forceinline__ void best_lanes(Best<NP>& b) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        Best<NP> x;
        x.v = __shfl_xor(b.v, o, 64); x.id = __shfl_xor(b.id, o, 64);
#pragma unroll
        for (int p = 0; p < NP; ++p) x.pay[p] = __shfl_xor(b.pay[p], o, 64);
        best_take(b, x);
    }
}
// block_best's LDS for workgroups of T threads: one entry per wave, twice (the rounds' parity)
template <int T, int NP>
struct BestSlots {
    float v[2][T / 64];
    int id[2][T / 64], pay[NP][2][T / 64];
};
// the block's best of every thread's `b`, in all threads: the waves' bests go to the slots of the round's parity, every wave
// reduces the T / 64 entries again.  One barrier: round r + 2 reuses round r's slots, and by then every thread has passed the
// barrier of round r + 1.
template <int T, int NP>
__device__ __forceinline__ Best<NP> block_best(Best<NP> b, BestSlots<T, NP>& red, int round) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, par = round & 1, w = lane & (T / 64 - 1);
    best_lanes<64>(b);
    if (lane == 0) {
        red.v[par][wave] = b.v; red.id[par][wave] = b.id;
#pragma unroll
        for (int p = 0; p < NP; ++p) red.pay[p][par][wave] = b.pay[p];
    }
    __syncthreads();
    Best<NP> f;
    f.v = red.v[par][w]; f.id = red.id[par][w];
#pragma unroll
    for (int p = 0; p < NP; ++p) f.pay[p] = red.pay[p][par][w];
    best_lanes<T / 64>(f);
    return f;
}

// -> the exclusive prefix of `mine` over the workgroup's T threads, `total` = the sum over all of them: a wave scan, the waves'
// totals through wsum (T / 64 values of LDS), one barrier.  V = int, or long long where the total can pass 2^31
template <int T, class V>
__device__ __forceinline__ V block_exclusive_scan(V mine, V* wsum, V& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const V incl = wave_inclusive_scan(mine, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    V base = incl - mine;
    total = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        const V v = wsum[w];
        if (w < wave) base += v;
        total += v;
    }
    return base;
}
