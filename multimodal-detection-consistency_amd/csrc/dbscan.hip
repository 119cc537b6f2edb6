// DBSCAN over a registered bank slot (src/ref_bank.py:302-315), as two independent halves.
//
//   graph   `radius_tile_kernel`: the eps-graph A[i, j] = (|x_i - x_j|^2 <= eps^2) of the slot's rows as a bitmask uint32
//           [R, words] -- a self-GEMM on gemm_core.hpp's main loop (slot_self_operands: A = B = the slot's rows, 256 x 256
//           tiles), the scores never leave the accumulators.  The test is  x_i.x_j >= h_i + h_j  with h = |x|^2 / 2 - eps^2 / 4 (fp32
//           addition commutes: the right side is the same number for (i, j) and (j, i)); h is NaN for a row whose norm is not
//           finite and in the padding up to whole tiles, so such a row or column compares false everywhere.  A bf16 slot
//           multiplies one plane (both operands are the stored values), an fp32 slot all four hi / lo products: a radius graph
//           is asked about near-duplicate rows, where the lo.lo term is ~1e-6 |x|^2 of a squared distance near zero.
//           In gemm_acc_t's layout the 16 lanes `lane & 15` hold 16 consecutive columns of one row: a __ballot per (m, n, r)
//           is 4 rows x 16 columns, four of them one 64-bit word for each of the 4 rows, stored by lanes 0 .. 3.
//           Only the tiles on and above the diagonal compute (the rest of adj is zeroed first); `radius_symmetrise_kernel`
//           then ORs adj with its bit transpose, one pair of 32 x 32 bit blocks per half wave, so adj is symmetric bit for
//           bit although the two orientations of a pair inside a diagonal tile add their products in a different order.
//           `radius_degree_kernel`: degree = the popcount of the final row.
//   labels  exact integer work on ANY such bitmask (no bank slot): comp[i] = i for core rows (degree >= min_samples), R
//           otherwise; a sweep lowers comp[i] and comp[comp[i]] to the minimum label among the core neighbours (integer
//           atomicMin; hooking the old root as FastSV does), a pointer jump follows it.  Labels only ever fall and stay
//           indices of the same component, so the fixed point -- every core row holds its component's lowest core index --
//           does not depend on the order; the number of sweeps does.  The finish numbers the roots by an exclusive scan,
//           hands core rows their root's id and border rows the lowest id among their core neighbours.
// Caller-supplied graphs are read defensively: a set bit beyond R or a label outside [0, R) is skipped, never dereferenced.
#include "slot_tile.hpp"

// ---- graph -------------------------------------------------------------------------------------------------------
// h from |x|^2 (launch_slot_row_vector)
struct RadiusHalf {
    float quarter_eps2;
    __device__ __forceinline__ float operator()(float n2) const { return 0.5f * n2 - quarter_eps2; }
};

__global__ __launch_bounds__(GEMM_THREADS) void radius_tile_kernel(GemmOperands g, const float* __restrict__ half,
                                                                   uint32_t* __restrict__ adj, int R, int words) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;                                  // the symmetrise pass fills the lower triangle
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i0 = ti * GEMM_BM, j0 = tj * GEMM_BN;
    const bool diag = ti == tj;
    gemm_acc_t acc;
    gemm_zero_acc(acc);
    gemm_mainloop(acc, g, i0, j0, smem);
    const int jw = gemm_acc_col(j0, wave, 0, 0) >> 5;     // the wave's 64 columns: words jw, jw + 1 of a row
    float hj[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) hj[n] = half[gemm_acc_col(j0, wave, lane, n)];
    const int shift = (lane & 3) * 16;                    // lanes 0 .. 3 assemble the words of the lane groups 0 .. 3
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int ib = gemm_acc_row(i0, wave, 0, m);      // the first of the block's 16 rows
        const f32x4_t hi = *(const f32x4_t*)(half + gemm_acc_row(i0, wave, lane, m));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = gemm_acc_row(i0, wave, lane, m) + r;
            uint64_t word = 0;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                bool in = acc[m][n][r] >= hi[r] + hj[n];
                // the diagonal bit of a finite row is set, not computed
                if (diag) in = in || (i == gemm_acc_col(j0, wave, lane, n) && hi[r] == hi[r]);
                const uint64_t b = __ballot(in);
                word |= ((b >> shift) & 0xffffull) << (n * 16);
            }
            const int row = ib + (lane & 3) * 4 + r;
            if (lane < 4 && jw < words && row < R) *(uint64_t*)(adj + (int64_t)row * words + jw) = word;
        }
    }
}

// x[t] of the 32 lanes of a half wave = the rows of a 32 x 32 bit block -> the rows of its transpose
__device__ __forceinline__ uint32_t bit_transpose32(uint32_t x, int lane) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const uint64_t col = __ballot((x >> k) & 1u);
        if ((lane & 31) == k) out = (uint32_t)(col >> (lane & 32));
    }
    return out;
}

// adj |= adj^T in place.  The half wave (a, b), b >= a, owns block (a, b) and block (b, a) and nobody else touches them.
__global__ __launch_bounds__(256) void radius_symmetrise_kernel(uint32_t* __restrict__ adj, int R, int words) {
    const int lane = threadIdx.x & 63;
    const int t = lane & 31;
    const int a = blockIdx.y;
    const int b = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = b >= a && b < words;
    const int ra = a * 32 + t, rb = b * 32 + t;
    const bool la = live && ra < R, lb = live && rb < R;
    uint32_t x = 0, y = 0;
    if (la) x = adj[(int64_t)ra * words + b];
    if (lb) y = adj[(int64_t)rb * words + a];
    const uint32_t xt = bit_transpose32(x, lane);
    const uint32_t yt = bit_transpose32(y, lane);
    if (la) adj[(int64_t)ra * words + b] = x | yt;
    if (lb && b != a) adj[(int64_t)rb * words + a] = y | xt;
}

__global__ __launch_bounds__(256) void radius_degree_kernel(const uint32_t* __restrict__ adj, int R, int words,
                                                            int32_t* __restrict__ degree) {
    const int lane = row_lane();
    for_wave_rows(R, [&](int i) {
        const uint32_t* row = adj + (int64_t)i * words;
        int s = 0;
        for (int w = lane; w < words; w += 64) s += __popc(row[w]);
        s = wave_sum(s);
        if (lane == 0) degree[i] = s;
    });
}

hipError_t launch_radius_graph(const RadiusGraphLaunch& L, hipStream_t stream) {
    const BankRows& B = L.bank;
    const RadiusPlan& P = L.plan;
    if (!P.ok || !slot_tile_ok(B, RADIUS_MAX_ROWS) || P.words != (B.R + 63) / 64 * 2 || P.hpad < B.R || !(L.eps > 0.f) || !L.half ||
        !L.adj || !L.degree)
        return hipErrorInvalidValue;
    const int R = (int)B.R, words = (int)P.words;
    hipError_t st = launch_slot_row_vector(B, L.half, P.hpad, RadiusHalf{0.25f * L.eps * L.eps}, stream);
    if (st != hipSuccess) return st;
    st = hipMemsetAsync(L.adj, 0, (size_t)P.adj_bytes, stream);
    if (st != hipSuccess) return st;
    st = launch<radius_tile_kernel, GEMM_LDS_BYTES>(dim3(P.tiles, P.tiles), dim3(GEMM_THREADS), GEMM_LDS_BYTES, stream,
                                                    slot_self_operands(B), (const float*)L.half, L.adj, R, words);
    if (st != hipSuccess) return st;
    st = launch<radius_symmetrise_kernel>(dim3(P.sym_grid_x, P.blocks32), dim3(256), 0, stream, L.adj, R, words);
    if (st != hipSuccess) return st;
    return launch<radius_degree_kernel>(dim3(wave_stride_grid(R)), dim3(256), 0, stream, (const uint32_t*)L.adj, R, words, L.degree);
}

// ---- labels ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dbscan_init_kernel(const int32_t* __restrict__ degree, int R, int min_samples,
                                                          int32_t* __restrict__ comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < R) comp[i] = degree[i] >= min_samples ? i : R;
}

// the minimum of f(j) over the core neighbours j of row i (one wave; every lane gets the result); `none` when there is none
template <class F>
__device__ __forceinline__ int core_neighbour_min(const uint32_t* __restrict__ row, const int32_t* __restrict__ degree, int R,
                                                  int words, int min_samples, int none, F f) {
    int m = none;
    for (int w = row_lane(); w < words; w += 64) {
        for_each_set_bit(row[w], [&](int b) {
            const int j = w * 32 + b;
            if (j < R && degree[j] >= min_samples) {
                const int v = f(j);
                m = v < m ? v : m;
            }
        });
    }
    return wave_min(m);
}

__global__ __launch_bounds__(256) void dbscan_sweep_kernel(const uint32_t* __restrict__ adj, const int32_t* __restrict__ degree,
                                                           int R, int words, int min_samples, int32_t* comp, int32_t* changed) {
    const int lane = row_lane();
    for_wave_rows(R, [&](int i) {
        if (degree[i] < min_samples) return;
        const int mine = comp[i];
        const int m = core_neighbour_min(adj + (int64_t)i * words, degree, R, words, min_samples, R, [&](int j) {
            const int c = comp[j];
            return (unsigned)c < (unsigned)R ? c : R;
        });
        if (lane == 0 && m < mine) {
            atomicMin(&comp[i], m);
            if ((unsigned)mine < (unsigned)R) atomicMin(&comp[mine], m);      // hook the old root as well
            atomicOr(changed, 1);
        }
    });
}

// comp[i] = the end of the chain i -> comp[i] -> ... (strictly falling, so it ends); other threads lower entries meanwhile,
// always to labels of the same component
__global__ __launch_bounds__(256) void dbscan_jump_kernel(const int32_t* __restrict__ degree, int R, int min_samples, int32_t* comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R || degree[i] < min_samples) return;
    const int first = comp[i];
    int c = first;
    while ((unsigned)c < (unsigned)R) {
        const int n = comp[c];
        if (n >= c || n < 0) break;
        c = n;
    }
    if (c < first) atomicMin(&comp[i], c);
}

// one workgroup: thread t owns the rows [t * per, (t + 1) * per); a root (a core row with comp[i] == i) gets its rank
__global__ __launch_bounds__(1024) void dbscan_roots_kernel(const int32_t* __restrict__ degree, const int32_t* __restrict__ comp, int R,
                                                            int min_samples, int per, int32_t* __restrict__ labels,
                                                            int32_t* __restrict__ n_clusters) {
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    const int j0 = t * per < R ? t * per : R, j1 = j0 + per < R ? j0 + per : R;
    int mine = 0;
    for (int j = j0; j < j1; ++j) mine += degree[j] >= min_samples && comp[j] == j;
    int total;
    int base = block_exclusive_scan<1024>(mine, wsum, total);
    for (int j = j0; j < j1; ++j)
        if (degree[j] >= min_samples && comp[j] == j) labels[j] = base++;
    if (t == 0) *n_clusters = total;
}

// one wave per row.  Only the roots' entries of labels are read here and no root's entry is written: nothing races.
__global__ __launch_bounds__(256) void dbscan_labels_kernel(const uint32_t* __restrict__ adj, const int32_t* __restrict__ degree,
                                                            const int32_t* __restrict__ comp, int R, int words, int min_samples,
                                                            int32_t* labels, uint8_t* __restrict__ core) {
    const int lane = row_lane();
    const int none = 0x7fffffff;
    for_wave_rows(R, [&](int i) {
        if (degree[i] >= min_samples) {
            const int r = comp[i];
            if (lane == 0) {
                core[i] = 1;
                if (r != i) labels[i] = (unsigned)r < (unsigned)R ? labels[r] : -1;
            }
            return;
        }
        const int m = core_neighbour_min(adj + (int64_t)i * words, degree, R, words, min_samples, none, [&](int j) {
            const int r = comp[j];
            return (unsigned)r < (unsigned)R ? labels[r] : none;
        });
        if (lane == 0) {
            core[i] = 0;
            labels[i] = m == none ? -1 : m;
        }
    });
}

static bool dbscan_args_ok(int R, int min_samples) { return R >= 1 && R <= RADIUS_MAX_ROWS && min_samples >= 1; }

hipError_t launch_dbscan_sweep(const uint32_t* adj, const int32_t* degree, int R, int min_samples, int32_t* comp, int32_t* changed,
                               int init, hipStream_t stream) {
    if (!dbscan_args_ok(R, min_samples) || !adj || !degree || !comp || !changed) return hipErrorInvalidValue;
    const int words = (int)radius_plan(R).words;
    hipError_t st;
    if (init) {
        st = launch<dbscan_init_kernel>(dim3((R + 255) / 256), dim3(256), 0, stream, degree, R, min_samples, comp);
        if (st != hipSuccess) return st;
    }
    st = launch<dbscan_sweep_kernel>(dim3(wave_stride_grid(R)), dim3(256), 0, stream, adj, degree, R, words, min_samples, comp, changed);
    if (st != hipSuccess) return st;
    return launch<dbscan_jump_kernel>(dim3((R + 255) / 256), dim3(256), 0, stream, degree, R, min_samples, comp);
}

hipError_t launch_dbscan_finish(const uint32_t* adj, const int32_t* degree, int R, int min_samples, const int32_t* comp,
                                int32_t* labels, uint8_t* core, int32_t* n_clusters, hipStream_t stream) {
    if (!dbscan_args_ok(R, min_samples) || !adj || !degree || !comp || !labels || !core || !n_clusters) return hipErrorInvalidValue;
    const int words = (int)radius_plan(R).words;
    hipError_t st = launch<dbscan_roots_kernel>(dim3(1), dim3(1024), 0, stream, degree, comp, R, min_samples, (R + 1023) / 1024, labels,
                                                n_clusters);
    if (st != hipSuccess) return st;
    return launch<dbscan_labels_kernel>(dim3(wave_stride_grid(R)), dim3(256), 0, stream, adj, degree, comp, R, words, min_samples, labels,
                                        core);
}
