// What the data validator (src/evaluation/data_validator.py:353-543) asks of a radius graph: WHICH pairs i < j are in it, in the
// order of the reference's nested loops, and their cosine at fp32 grade.  Exact integer work on any bitmask adj [R, words]
// (dbscan.hip's layout; no bank slot) plus one row kernel over a bank slot.
//
//   count   `pair_count_kernel`: one wave per row i, the lanes stride over the words from i / 32 on; the word of the diagonal
//           loses its bits j <= i, the last words their padding bits j >= R, so the lower triangle, the diagonal and the padding
//           never count.  With a group vector a bit also needs group[i] >= 0, group[j] >= 0 and group[i] != group[j]: each
//           lane filters its word bit by bit before the popcount.  `pair_scan_kernel`: one workgroup scans the R <= 131 072
//           counts in place into exclusive offsets, in 64-bit sums (a full graph holds 8.6e9 pairs); offsets[R] is the total.
//   fill    `pair_fill_kernel`: one wave per row again, chunks of 64 words, a running base that starts at offsets[i] and a wave
//           prefix sum over the lanes' popcounts; a lane writes the pairs (i, j) of its word in ascending j.  The list is
//           lexicographic in (i, j), a pure function of (adj, group): no atomics.  A slot outside [0, P) is never written.
//   cosine  `pair_cosine_kernel`: PAIR_COS_LANES = 16 lanes per pair whatever D is; lane s owns the elements [128 c + 8 s,
//           128 c + 8 s + 8) of every 128-wide chunk c and adds x.y, |x|^2 and |y|^2 with one fp32 FMA chain each, elements
//           in ascending order; the 16 partial sums meet in lanes_sum's xor butterfly (distances 8, 4, 2, 1), which leaves the
//           same bits in every lane.  Products and fp32 additions commute, so swapping the two rows of a pair changes no bit:
//           sim(i, j) == sim(j, i), and nothing depends on the launch.  sim = dot / sqrt(|x|^2 |y|^2), both correctly rounded.
#include "kernels.hpp"
#include "launch.hpp"
#include "select.hpp"

// the bits j of word w of row i with i < j < R
__device__ __forceinline__ uint32_t pair_upper_word(const uint32_t* __restrict__ row, int w, int i, int R) {
    const int n = R - w * 32;                            // live bits of the word
    if (n <= 0) return 0u;
    uint32_t x = row[w];
    if (w == (i >> 5)) x &= 0xfffffffeu << (i & 31);     // bits 0 .. i & 31 of the diagonal's word: the lower triangle and i itself
    if (n < 32) x &= (1u << n) - 1u;
    return x;
}

// of the bits of x (word w, all < R), those whose row is in a group and in another group than gi
__device__ __forceinline__ uint32_t pair_group_filter(uint32_t x, int w, int gi, const int32_t* __restrict__ group) {
    uint32_t keep = 0u;
    for_each_set_bit(x, [&](int b) {
        const int gj = group[w * 32 + b];
        if (gj >= 0 && gj != gi) keep |= 1u << b;
    });
    return keep;
}

__global__ __launch_bounds__(256) void pair_count_kernel(const uint32_t* __restrict__ adj, int R, int words,
                                                         const int32_t* __restrict__ group, int64_t* __restrict__ offsets) {
    const int lane = row_lane();
    for_wave_rows(R, [&](int i) {
        const uint32_t* row = adj + (int64_t)i * words;
        const int gi = group ? group[i] : 0;
        int s = 0;
        if (gi >= 0) {
            for (int w = (i >> 5) + lane; w < words; w += 64) {
                uint32_t x = pair_upper_word(row, w, i, R);
                if (group) x = pair_group_filter(x, w, gi, group);
                s += __popc(x);
            }
        }
        s = wave_sum(s);
        if (lane == 0) offsets[i] = s;
    });
}

// one workgroup: thread t owns the rows [t * per, (t + 1) * per); counts -> exclusive offsets in place, offsets[R] = the total
__global__ __launch_bounds__(PAIRS_SCAN_THREADS) void pair_scan_kernel(int64_t* __restrict__ offsets, int R, int per) {
    __shared__ long long wsum[PAIRS_SCAN_THREADS / 64];
    const int t = threadIdx.x;
    const int j0 = (int64_t)t * per < R ? t * per : R, j1 = j0 + per < R ? j0 + per : R;
    long long mine = 0;
    for (int j = j0; j < j1; ++j) mine += offsets[j];
    long long total;
    long long base = block_exclusive_scan<PAIRS_SCAN_THREADS>(mine, wsum, total);
    for (int j = j0; j < j1; ++j) {
        const long long c = offsets[j];
        offsets[j] = base;
        base += c;
    }
    if (t == 0) offsets[R] = total;
}

__global__ __launch_bounds__(256) void pair_fill_kernel(const uint32_t* __restrict__ adj, int R, int words,
                                                        const int32_t* __restrict__ group, const int64_t* __restrict__ offsets,
                                                        int32_t* __restrict__ pairs, int64_t P) {
    const int lane = row_lane();
    for_wave_rows(R, [&](int i) {
        const uint32_t* row = adj + (int64_t)i * words;
        const int gi = group ? group[i] : 0;
        if (gi < 0) return;
        int64_t base = offsets[i];
        for (int w0 = i >> 5; w0 < words; w0 += 64) {
            const int w = w0 + lane;
            uint32_t x = 0u;
            if (w < words) {
                x = pair_upper_word(row, w, i, R);
                if (group) x = pair_group_filter(x, w, gi, group);
            }
            const int c = __popc(x);
            const int incl = wave_inclusive_scan(c, lane);
            int64_t slot = base + (incl - c);
            for_each_set_bit(x, [&](int b) {
                if ((uint64_t)slot < (uint64_t)P) {
                    pairs[2 * slot] = i;
                    pairs[2 * slot + 1] = w * 32 + b;
                }
                ++slot;
            });
            base += __shfl(incl, 63, 64);
        }
    });
}

__global__ __launch_bounds__(256) void pair_cosine_kernel(BankRows bank, const int32_t* __restrict__ pairs, int64_t P,
                                                          float* __restrict__ sim) {
    constexpr int PER = 256 / PAIR_COS_LANES;            // pairs per workgroup and trip
    const int sub = threadIdx.x & (PAIR_COS_LANES - 1);
    for (int64_t p0 = (int64_t)blockIdx.x * PER; p0 < P; p0 += (int64_t)gridDim.x * PER) {
        const int64_t p = p0 + threadIdx.x / PAIR_COS_LANES;
        const bool live = p < P;
        int i = -1, j = -1;
        if (live) { i = pairs[2 * p]; j = pairs[2 * p + 1]; }
        const bool in = i >= 0 && j >= 0 && (int64_t)i < bank.R && (int64_t)j < bank.R;
        float dot = 0.f, nx = 0.f, ny = 0.f;
        if (in) {
            const uint16_t* xr = bank.p + (int64_t)i * bank.ld;
            const uint16_t* yr = bank.p + (int64_t)j * bank.ld;
            for (int c = sub * 8; c < bank.D; c += PAIR_COS_LANES * 8) {
                float x[8], y[8];
                bank_row8(xr + c, bank.D, bank.planes, x);
                bank_row8(yr + c, bank.D, bank.planes, y);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    dot = fmaf(x[e], y[e], dot);
                    nx = fmaf(x[e], x[e], nx);
                    ny = fmaf(y[e], y[e], ny);
                }
            }
        }
        dot = lanes_sum<PAIR_COS_LANES>(dot);
        nx = lanes_sum<PAIR_COS_LANES>(nx);
        ny = lanes_sum<PAIR_COS_LANES>(ny);
        if (live && sub == 0) {
            float s = __builtin_nanf("");
            if (in) {
                if (nx == 0.f || ny == 0.f) s = (nx != nx || ny != ny) ? __builtin_nanf("") : 0.f;    // a zero row: 0 unless the other is NaN
                else s = dot / sqrtf(nx * ny);
            }
            sim[p] = s;
        }
    }
}

static bool pair_args_ok(const uint32_t* adj, int R, const void* offsets) { return adj && offsets && pairs_plan(R).ok; }

hipError_t launch_graph_pair_count(const uint32_t* adj, int R, const int32_t* group, int64_t* offsets, hipStream_t stream) {
    if (!pair_args_ok(adj, R, offsets)) return hipErrorInvalidValue;
    const PairsPlan pl = pairs_plan(R);
    hipError_t st = launch<pair_count_kernel>(dim3(pl.row_grid), dim3(256), 0, stream, adj, R, pl.words, group, offsets);
    if (st != hipSuccess) return st;
    return launch<pair_scan_kernel>(dim3(1), dim3(PAIRS_SCAN_THREADS), 0, stream, offsets, R, pl.scan_per);
}

hipError_t launch_graph_pair_fill(const uint32_t* adj, int R, const int32_t* group, const int64_t* offsets, int32_t* pairs, int64_t P,
                                  hipStream_t stream) {
    if (!pair_args_ok(adj, R, offsets) || P < 0 || (P > 0 && !pairs)) return hipErrorInvalidValue;
    if (P == 0) return hipSuccess;
    const PairsPlan pl = pairs_plan(R);
    return launch<pair_fill_kernel>(dim3(pl.row_grid), dim3(256), 0, stream, adj, R, pl.words, group, offsets, pairs, P);
}

hipError_t launch_pair_cosine(const BankRows& bank, const int32_t* pairs, int64_t P, float* sim, hipStream_t stream) {
    if (!bank.p || bank.R < 1 || bank.D < 8 || bank.D % 8 != 0 || bank.planes < 1 || bank.planes > 2 || P < 0 ||
        (P > 0 && (!pairs || !sim)))
        return hipErrorInvalidValue;
    if (P == 0) return hipSuccess;
    return launch<pair_cosine_kernel>(dim3(pair_cosine_grid(P)), dim3(256), 0, stream, bank, pairs, P, sim);
}
