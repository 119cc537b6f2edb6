// K-means over a registered bank slot (src/ref_bank.py:259-339; the training half of an IVF index): one Lloyd iteration is
// an ASSIGN pass (nearest centre of every bank row) and an UPDATE pass (the mean of every cluster's rows).
//
//   assign  `kmeans_assign_kernel`: a workgroup owns 256 bank rows and walks the centre tiles.  Per 256 x 256 tile it runs
//           the GEMM main loop with the CENTRES on the MFMA row dimension and the BANK ROWS on the lane dimension, and
//           keeps each row's running (best score, centre) in slot_tile.hpp's SlotBest: no score leaves the accumulators.
//           score = x.c - |c|^2 / 2 (arg-max = Euclidean nearest), the half norms come from an fp32 [K] vector padded to
//           whole tiles with NaN: a padded centre can never win.  A row whose scores are all NaN gets label -1.
//           Products as in the bank search (slot_operands, gemm_core.hpp): centres are split into (hi | lo) bf16 planes; a bf16
//           bank multiplies both (exact products), an fp32 bank's planes take hi.hi + hi.lo + lo.hi.
//   update  a counting sort -- per-block label histogram (integer atomics into the block's own counter row), a column
//           scan over the blocks, an exclusive scan over the clusters, a STABLE scatter (rank inside a 256-row chunk by
//           comparison, chunks in order) -- gives the member lists in ascending row order; one workgroup per cluster then
//           sums its members in a fixed order in fp32.  No floating-point atomics: the centres are a pure function of
//           (bank, labels).  The sort is a launch of its own (launch_label_sort): ivf.hip groups (query, probe) pairs by list
//           with it, and takes the half norms of its centroids from kmeans_halfnorm_kernel.
// The slot's rows arrive as a BankRows (kernels.hpp); the row kernels decode them with bank_row8 (common.hpp); the offsets'
// block-wide scan is select.hpp's.
#include "slot_tile.hpp"

// ---- assign ------------------------------------------------------------------------------------------------------
// halfnorm[k] = |c_k|^2 / 2 from the fp32 centres, k < K; NaN for the padding up to Kpad (a multiple of 256)
__global__ __launch_bounds__(256) void kmeans_halfnorm_kernel(const float* __restrict__ c, int D, int K, int Kpad,
                                                              float* __restrict__ halfnorm) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= Kpad) return;
    float s = __builtin_nanf("");
    if (k < K) {
        const float* row = c + (int64_t)k * D;
        s = 0.f;
        for (int i = lane * 4; i < D; i += 256) {
            const f32x4_t v = *(const f32x4_t*)(row + i);
            s = fmaf(v[0], v[0], fmaf(v[1], v[1], fmaf(v[2], v[2], fmaf(v[3], v[3], s))));
        }
        s = 0.5f * wave_sum(s);
    }
    if (lane == 0) halfnorm[k] = s;
}

// out[r] = |x_r|^2 of the stored row (hi + lo of an fp32 bank), one wave per row
__global__ __launch_bounds__(256) void kmeans_rownorm_kernel(BankRows bank, float* __restrict__ out) {
    const int lane = row_lane();
    for_wave_rows(bank.R, [&](int64_t r) {
        const uint16_t* br = bank.p + r * bank.ld;
        float s = 0.f;
        for (int c = lane * 8; c < bank.D; c += 512) {
            float x[8];
            bank_row8(br + c, bank.D, bank.planes, x);
#pragma unroll
            for (int e = 0; e < 4; ++e) s = fmaf(x[2 * e], x[2 * e], fmaf(x[2 * e + 1], x[2 * e + 1], s));
        }
        s = wave_sum(s);
        if (lane == 0) out[r] = s;
    });
}

struct KmeansAssignArgs {
    const float* halfnorm;     // [n_ctiles * 256], NaN beyond K
    int32_t* labels;           // [R]
    float* score;              // [R] or null
    float* dist2;              // [R] or null; holds |x|^2 on entry
    int R;
};

__global__ __launch_bounds__(GEMM_THREADS) void kmeans_assign_kernel(GemmOperands g, KmeansAssignArgs e, int n_ctiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int j0 = blockIdx.x * GEMM_BN;
    SlotBest best;
    for (int ct = 0; ct < n_ctiles; ++ct) {
        gemm_acc_t acc;
        gemm_zero_acc(acc);
        gemm_mainloop(acc, g, ct * GEMM_BM, j0, smem);
        best.take(acc, e.halfnorm, ct * GEMM_BM, wave, lane, [](float a, float hn, int, int, float& s) {
            s = a - hn;
            return true;
        });
    }
    best.finish(smem, wave, lane, [&](int jl, float v, int i) {
        const int row = j0 + jl;
        if (row >= e.R) return;
        const bool none = i == CAND_NONE;
        e.labels[row] = none ? -1 : i;
        if (e.score) e.score[row] = v;
        if (e.dist2) e.dist2[row] = none ? 0.f : fmaxf(0.f, e.dist2[row] - 2.f * v);
    });
}

hipError_t launch_kmeans_halfnorm(const float* centroids, int D, int K, int Kpad, float* halfnorm, hipStream_t stream) {
    return launch<kmeans_halfnorm_kernel>(dim3((Kpad + 3) / 4), dim3(256), 0, stream, centroids, D, K, Kpad, halfnorm);
}

hipError_t launch_kmeans_rownorm(const BankRows& bank, float* out, hipStream_t stream) {
    if (bank.R < 1 || bank.D < 8 || bank.D % 8 != 0 || bank.planes < 1 || bank.planes > 2) return hipErrorInvalidValue;
    return launch<kmeans_rownorm_kernel>(dim3(wave_stride_grid(bank.R)), dim3(256), 0, stream, bank, out);
}

hipError_t launch_kmeans_assign(const KmeansAssignLaunch& L, hipStream_t stream) {
    const BankRows& B = L.bank;
    if (!slot_tile_ok(B, 0x7fffffffLL) || L.K < 1) return hipErrorInvalidValue;
    const int n_ctiles = (L.K + GEMM_BM - 1) / GEMM_BM;
    const int Kpad = n_ctiles * GEMM_BM;
    hipError_t st = launch_kmeans_halfnorm(L.centroids, B.D, L.K, Kpad, L.halfnorm, stream);
    if (st != hipSuccess) return st;
    if (L.dist2) {
        st = launch_kmeans_rownorm(B, L.dist2, stream);
        if (st != hipSuccess) return st;
    }
    // centres on the MFMA row dimension (A), bank rows on the lane dimension (B)
    const GemmOperands g = slot_operands(L.cplanes, L.K, B);
    KmeansAssignArgs e;
    e.halfnorm = L.halfnorm; e.labels = L.labels; e.score = L.score; e.dist2 = L.dist2; e.R = (int)B.R;
    const int64_t n_btiles = (B.R + GEMM_BN - 1) / GEMM_BN;
    return launch<kmeans_assign_kernel, SLOT_BEST_LDS_BYTES>(dim3((unsigned)n_btiles), dim3(GEMM_THREADS), SLOT_BEST_LDS_BYTES, stream, g, e, n_ctiles);
}

// ---- update ------------------------------------------------------------------------------------------------------
// Block b of the counting sort owns the rows [b * rpb, (b + 1) * rpb) and row b of the [nblocks, K] counter matrix.
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ labels, int64_t R, int K, int rpb,
                                                          int32_t* __restrict__ blk_cnt) {
    const int64_t beg = (int64_t)blockIdx.x * rpb;
    const int64_t end = beg + rpb < R ? beg + rpb : R;
    int32_t* cnt = blk_cnt + (int64_t)blockIdx.x * K;
    for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)K) atomicAdd(&cnt[l], 1);       // integer: the counts do not depend on the order
    }
}
// per cluster: the counters of the blocks become exclusive prefixes over the blocks; counts[j] = the total
__global__ __launch_bounds__(256) void kmeans_colscan_kernel(int32_t* __restrict__ blk_cnt, int nblocks, int K,
                                                             int32_t* __restrict__ counts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    int run = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int t = blk_cnt[(int64_t)b * K + j];
        blk_cnt[(int64_t)b * K + j] = run;
        run += t;
    }
    counts[j] = run;
}
// offsets[0 .. K] = exclusive scan of counts; one workgroup, thread t owns the clusters [t * per, (t + 1) * per)
__global__ __launch_bounds__(1024) void kmeans_offsets_kernel(const int32_t* __restrict__ counts, int K, int per,
                                                              int32_t* __restrict__ offsets) {
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    const int j0 = t * per, j1 = (j0 + per < K) ? j0 + per : K;
    int mine = 0;
    for (int j = j0; j < j1; ++j) mine += counts[j];
    int total;
    int base = block_exclusive_scan<1024>(mine, wsum, total);
    for (int j = j0; j < j1; ++j) { offsets[j] = base; base += counts[j]; }
    if (t == 0) offsets[K] = total;
}
// stable scatter: a block walks its rows in chunks of 256; inside a chunk a row's rank among the rows of its label is
// counted by comparison, between chunks the block's running position per label is its entry of the counter matrix
__global__ __launch_bounds__(256) void kmeans_scatter_kernel(const int32_t* __restrict__ labels, int64_t R, int K, int rpb,
                                                             int32_t* blk_cnt, const int32_t* __restrict__ offsets,
                                                             int32_t* __restrict__ order) {
    __shared__ int lab[256];
    const int t = threadIdx.x;
    const int64_t beg = (int64_t)blockIdx.x * rpb;
    const int64_t end = beg + rpb < R ? beg + rpb : R;
    int32_t* cnt = blk_cnt + (int64_t)blockIdx.x * K;
    for (int64_t base = beg; base < end; base += 256) {
        const int64_t i = base + t;
        int l = i < end ? labels[i] : -1;
        if ((unsigned)l >= (unsigned)K) l = -1;
        lab[t] = l;
        __syncthreads();
        int rank = 0, total = 0;
        if (l >= 0) {
            for (int u = 0; u < 256; ++u) {
                const int same = lab[u] == l;
                rank += same & (u < t);
                total += same;
            }
            const int64_t pos = (int64_t)offsets[l] + cnt[l] + rank;
            if (pos < R) order[pos] = (int32_t)i;      // always true for the labels the histogram saw
        }
        __syncthreads();
        if (l >= 0 && rank == total - 1) cnt[l] += total;
        __syncthreads();
    }
}
// one workgroup per cluster: thread (g, p) sums the 8 columns of piece p over the members g, g + G, ... in list order, the G
// partial sums are added in the order of g; an empty cluster copies its input row
__global__ __launch_bounds__(256) void kmeans_centroid_kernel(BankRows bank, const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ offsets, const float* __restrict__ cin,
                                                              float* __restrict__ cout) {
    __shared__ float red[256 * 8];
    const int k = blockIdx.x, t = threadIdx.x, D = bank.D;
    const int beg = offsets[k], n = offsets[k + 1] - beg;
    if (n <= 0) {
        for (int c = t; c < D; c += 256) cout[(int64_t)k * D + c] = cin[(int64_t)k * D + c];
        return;
    }
    const int pieces = D / 8;
    const int P = pieces < 256 ? pieces : 256;
    const int G = 256 / P;
    const int g = t / P, p = t - g * P;
    for (int p0 = 0; p0 < pieces; p0 += P) {
        const bool live = g < G && p0 + p < pieces;
        const int c = (p0 + p) * 8;
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = 0.f;
        if (live) {
#pragma unroll 4
            for (int i = g; i < n; i += G) {
                float x[8];
                bank_row8(bank.p + (int64_t)order[beg + i] * bank.ld + c, D, bank.planes, x);
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] += x[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) red[(g * P + p) * 8 + e] = s[e];
        }
        __syncthreads();
        if (live && g == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = s[e];
                for (int gg = 1; gg < G; ++gg) v += red[(gg * P + p) * 8 + e];
                cout[(int64_t)k * D + c + e] = v / (float)n;
            }
        }
        __syncthreads();
    }
}

// the stable counting sort alone: the indices 0 .. R - 1 grouped by label (ascending inside a label) -> order, offsets, counts.
// The k-means update sorts bank rows by cluster; the IVF scan (ivf.hip) sorts (query, probe) pairs by the list they read.
hipError_t launch_label_sort(const LabelSortLaunch& L, hipStream_t stream) {
    if (L.R < 1 || L.R > 0x7fffffffLL || L.K < 1 || L.nblocks < 1 || L.rows_per_block < 1 ||
        (int64_t)L.nblocks * L.rows_per_block < L.R)
        return hipErrorInvalidValue;
    hipError_t st = hipMemsetAsync(L.blk_cnt, 0, (size_t)L.nblocks * L.K * 4, stream);
    if (st != hipSuccess) return st;
    st = launch<kmeans_hist_kernel>(dim3(L.nblocks), dim3(256), 0, stream, L.labels, L.R, L.K, L.rows_per_block, L.blk_cnt);
    if (st != hipSuccess) return st;
    st = launch<kmeans_colscan_kernel>(dim3((L.K + 255) / 256), dim3(256), 0, stream, L.blk_cnt, L.nblocks, L.K, L.counts);
    if (st != hipSuccess) return st;
    st = launch<kmeans_offsets_kernel>(dim3(1), dim3(1024), 0, stream, (const int32_t*)L.counts, L.K, (L.K + 1023) / 1024, L.offsets);
    if (st != hipSuccess) return st;
    return launch<kmeans_scatter_kernel>(dim3(L.nblocks), dim3(256), 0, stream, L.labels, L.R, L.K, L.rows_per_block, L.blk_cnt,
                                         (const int32_t*)L.offsets, L.order);
}

hipError_t launch_kmeans_update(const KmeansUpdateLaunch& L, hipStream_t stream) {
    const BankRows& B = L.bank;
    if (!slot_tile_ok(B, 0x7fffffffLL) || L.K < 1 || L.nblocks < 1 || L.rows_per_block < 1 || (int64_t)L.nblocks * L.rows_per_block < B.R)
        return hipErrorInvalidValue;
    LabelSortLaunch S;
    S.labels = L.labels; S.R = B.R; S.K = L.K; S.nblocks = L.nblocks; S.rows_per_block = L.rows_per_block;
    S.blk_cnt = L.blk_cnt; S.counts = L.counts; S.offsets = L.offsets; S.order = L.order;
    hipError_t st = launch_label_sort(S, stream);
    if (st != hipSuccess) return st;
    return launch<kmeans_centroid_kernel>(dim3(L.K), dim3(256), 0, stream, B, (const int32_t*)L.order, (const int32_t*)L.offsets,
                                          L.centroids_in, L.centroids_out);
}
