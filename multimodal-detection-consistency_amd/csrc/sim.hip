// Similarity metrics (src/utils/metrics.py:89-106,166-276 SimilarityMetrics / SimilarityCalculator, src/retrieval.py:158-193
// ConsistencyCalculator): cosine, Euclidean and Manhattan distance, Pearson and Spearman correlation of PAIRS of rows, one
// launch for a batch of pairs, and the top-k overlap of two retrievals.
//
// Row form (sim_rows_kernel): one workgroup per pair of rows of n = D <= SIM_MAX_D elements, fp32 or int32 (SIM_KEY_I32: index
// lists; an int32 converts to fp64 exactly and is ordered as an integer).  A thread keeps its elements tid, tid + T, ... of both
// rows in registers from the first pass on.
//   sums      fp64 over the elements in thread order, then a fixed tree (sim_block_reduce): bits depend on n alone
//   Pearson   two passes: the fp64 means, then the sums of cx cy, cx cx, cy cy of the centred values
//   Spearman  exact integers.  The row's order-preserving 32-bit keys (-0.0 as 0.0) are sorted, without payload, by a bitonic
//             network in LDS padded to a power of two with the largest key; a real key may equal the padding (INT32_MAX), so the
//             padding is kept out by searching the first n sorted keys only, where the n real keys are.  Each thread finds
//             lo = #(keys < own) and hi = #(keys <= own) of its own elements by fixed-step lower and upper bound: the doubled
//             1-based average rank is lo + hi + 1, the centred doubled rank c = lo + hi - n, |c| <= n - 1, and the three
//             sums of products are int64.  y reuses x's LDS.
// Long form (one pair of n <= SIM_MAX_N elements): the caller sorts the values; sim_flat_rank_kernel finds every element's c by
// the same two searches in the sorted array (no scan, no dependency between workgroups); the sums run as partial kernel +
// one-workgroup finish kernel, twice (means, then centred sums), over the caller's workspace (host_plan.hpp: sim_flat_plan).
// Grid and chunks are functions of n alone and every hand-off between workgroups crosses a kernel boundary.
// Both forms close with sim_close.  No atomics, no inline assembly; contraction is off, so the formulas are literal.
#include "common.hpp"
#include "kernels.hpp"
#include "launch.hpp"

#pragma clang fp contract(off)

#define SIM_NSUM 7      // sums of x, y, x y, x x, y y, (x - y)^2, |x - y|
#define SIM_QNAN __longlong_as_double(0x7ff8000000000000LL)

struct SimAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct SimMin { __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); } };
struct SimMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };

// v[k] over the workgroup's NW waves, for every k: the wave's xor butterfly (distances 32 ... 1), then the waves' values in
// wave order; every thread ends with the same bits.  sc: NW * K words of LDS, free again once every thread has returned.
template <int NW, int K, class T, class Op>
__device__ __forceinline__ void sim_block_reduce(T (&v)[K], T* sc, int lane, int wave, Op op) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = op(v[k], __shfl_xor(v[k], o, 64));
    }
    if (NW == 1) return;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sc[k * NW + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T s = sc[k * NW];
#pragma unroll
        for (int w = 1; w < NW; ++w) s = op(s, sc[k * NW + w]);
        v[k] = s;
    }
}

struct SimScratch {
    double d[SIM_NSUM * 4];
    long long i[4 * 4];
};

// what a thread accumulates over its elements in the first pass
struct SimPass1 {
    double s[SIM_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double lo[2] = {INFINITY, INFINITY};        // min of x, of y (fmin: a NaN element is passed over)
    double hi[2] = {-INFINITY, -INFINITY};
    long long nan = 0;
    __device__ __forceinline__ void take(double x, double y) {
        const double d = x - y;
        s[0] += x; s[1] += y; s[2] += x * y; s[3] += x * x; s[4] += y * y; s[5] += d * d; s[6] += fabs(d);
        lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y);
        hi[0] = fmax(hi[0], x); hi[1] = fmax(hi[1], y);
        nan += (x != x) + (y != y);
    }
};

template <int NW>
__device__ __forceinline__ void sim_reduce_pass1(SimPass1& p, SimScratch& sc, int lane, int wave) {
    sim_block_reduce<NW>(p.s, sc.d, lane, wave, SimAdd());
    sim_block_reduce<NW>(p.lo, sc.d, lane, wave, SimMin());
    sim_block_reduce<NW>(p.hi, sc.d, lane, wave, SimMax());
}

__device__ __forceinline__ double sim_canon(double v) { return v != v ? SIM_QNAN : v; }

// The closing formulas, shared by the two forms.  s: the first pass's sums; lo / hi: the rows' extremes; c: the centred sums
// of cx cy, cx cx, cy cy; ic: the same over the centred doubled ranks; nan: the NaN elements of the pair.  A NaN result is
// written as the one quiet NaN 0x7ff8000000000000.
__device__ __forceinline__ void sim_close(int64_t n, const double* s, const double* lo, const double* hi, const double* c,
                                          const long long* ic, long long nan, double* out, int64_t* ints) {
    double cosv = s[2] / sqrt(s[3] * s[4]);
    if (nan == 0 && (s[3] == 0.0 || s[4] == 0.0)) cosv = 0.0;
    double r = SIM_QNAN;
    if (n >= 2 && lo[0] != hi[0] && lo[1] != hi[1]) {
        r = c[0] / sqrt(c[1] * c[2]);
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                    // keeps a NaN
    }
    double rho = SIM_QNAN;
    if (n >= 2 && nan == 0 && ic[1] != 0 && ic[2] != 0) rho = (double)ic[0] / sqrt((double)ic[1] * (double)ic[2]);
    out[0] = sim_canon(cosv);
    out[1] = sim_canon(sqrt(s[5]));
    out[2] = sim_canon(s[6]);
    out[3] = sim_canon(r);
    out[4] = sim_canon(rho);
    out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
    const bool void_ranks = nan != 0;
    ints[0] = void_ranks ? 0 : ic[0];
    ints[1] = void_ranks ? 0 : ic[1];
    ints[2] = void_ranks ? 0 : ic[2];
    ints[3] = nan;
}

// ---- row form
template <bool I32>
__device__ __forceinline__ double sim_value(uint32_t w) { return I32 ? (double)(int32_t)w : (double)__uint_as_float(w); }
// order-preserving key: ascending keys = ascending values; -0.0 gets 0.0's key
template <bool I32>
__device__ __forceinline__ uint32_t sim_key(uint32_t w) {
    if (I32) return w ^ 0x80000000u;
    if (w == 0x80000000u) w = 0u;
    return (w & 0x80000000u) ? ~w : (w | 0x80000000u);
}

// how many of the first n entries of the ascending array keys are < key (UPPER: <= key); P = a power of two >= n
template <bool UPPER>
__device__ __forceinline__ int sim_count_keys(const uint32_t* keys, int n, int P, uint32_t key) {
    int pos = 0;
    for (int s = P; s > 0; s >>= 1) {
        const int q = pos + s;
        if (q <= n) {
            const uint32_t v = keys[q - 1];
            if (UPPER ? v <= key : v < key) pos = q;
        }
    }
    return pos;
}

// sorts keys[0, P) ascending: P a power of two, T threads, one barrier per stage (and one in front: the fill)
template <int T>
__device__ __forceinline__ void sim_bitonic_sort(uint32_t* keys, int P, int tid) {
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = keys[i], b = keys[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    }
}

// the centred doubled ranks of the thread's elements of one row (words w[E]) into c[E]; leaves keys readable until the next fill
template <int T, int E, bool I32>
__device__ __forceinline__ void sim_row_ranks(const uint32_t (&w)[E], int n, int P, uint32_t* keys, int tid, int (&c)[E]) {
    __syncthreads();                                                    // the previous row's searches are done
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid + e * T;
        if (i < P) keys[i] = i < n ? sim_key<I32>(w[e]) : 0xffffffffu;
    }
    sim_bitonic_sort<T>(keys, P, tid);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        c[e] = 0;
        if (tid + e * T < n) {
            const uint32_t key = sim_key<I32>(w[e]);
            c[e] = sim_count_keys<false>(keys, n, P, key) + sim_count_keys<true>(keys, n, P, key) - n;
        }
    }
}

template <int T, bool I32>
__global__ __launch_bounds__(T) void sim_rows_kernel(SimRowsLaunch a) {
    constexpr int NW = T / 64, E = T == 64 ? 4 : SIM_MAX_D / 256;      // T * E elements at most: 256, or SIM_MAX_D
    __shared__ uint32_t keys[T * E];
    __shared__ SimScratch sc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.D;
    const int64_t row = blockIdx.x;
    const uint32_t* xr = (const uint32_t*)a.x + row * a.ldx;
    const uint32_t* yr = (const uint32_t*)a.y + row * a.ldy;
    uint32_t xw[E], yw[E];
    SimPass1 p;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = tid + e * T;
        xw[e] = 0u; yw[e] = 0u;
        if (i < n) {
            xw[e] = xr[i]; yw[e] = yr[i];
            p.take(sim_value<I32>(xw[e]), sim_value<I32>(yw[e]));
        }
    }
    sim_reduce_pass1<NW>(p, sc, lane, wave);
    const double mx = p.s[0] / (double)n, my = p.s[1] / (double)n;
    double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (tid + e * T < n) {
            const double cx = sim_value<I32>(xw[e]) - mx, cy = sim_value<I32>(yw[e]) - my;
            c[0] += cx * cy; c[1] += cx * cx; c[2] += cy * cy;
        }
    }
    sim_block_reduce<NW>(c, sc.d, lane, wave, SimAdd());

    int P = 1;
    while (P < n) P <<= 1;
    int rx[E], ry[E];
    sim_row_ranks<T, E, I32>(xw, n, P, keys, tid, rx);
    sim_row_ranks<T, E, I32>(yw, n, P, keys, tid, ry);
    long long ic[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < E; ++e) {
        ic[0] += (long long)rx[e] * ry[e]; ic[1] += (long long)rx[e] * rx[e]; ic[2] += (long long)ry[e] * ry[e];
    }
    long long nan[1] = {p.nan};
    sim_block_reduce<NW>(ic, sc.i, lane, wave, SimAdd());
    sim_block_reduce<NW>(nan, sc.i, lane, wave, SimAdd());
    if (tid == 0) sim_close(n, p.s, p.lo, p.hi, c, ic, nan[0], a.out + row * SIM_COLS, a.ints + row * SIM_INTS);
}

hipError_t launch_sim_rows(const SimRowsLaunch& L, hipStream_t stream) {
    if (L.B < 0 || L.B > 0x7fffffffLL || L.D < 1 || L.D > SIM_MAX_D || L.ldx < L.D || L.ldy < L.D) return hipErrorInvalidValue;
    if (L.key != SIM_KEY_F32 && L.key != SIM_KEY_I32) return hipErrorInvalidValue;
    if (L.B == 0) return hipSuccess;
    if (!L.x || !L.y || !L.out || !L.ints) return hipErrorInvalidValue;
    const dim3 grid((unsigned)L.B);
    const bool i32 = L.key == SIM_KEY_I32;
    if (sim_row_threads(L.D) == 64)
        return i32 ? launch<sim_rows_kernel<64, true>>(grid, dim3(64), 0, stream, L) : launch<sim_rows_kernel<64, false>>(grid, dim3(64), 0, stream, L);
    return i32 ? launch<sim_rows_kernel<256, true>>(grid, dim3(256), 0, stream, L) : launch<sim_rows_kernel<256, false>>(grid, dim3(256), 0, stream, L);
}

// ---- long form
// how many of the n ascending values (NaN last) are < v (UPPER: <= v); a NaN v counts nothing
template <bool UPPER>
__device__ __forceinline__ int sim_count_values(const float* sorted, int n, int P, float v) {
    int pos = 0;
    for (int s = P; s > 0; s >>= 1) {
        const int q = pos + s;
        if (q <= n) {
            const float u = sorted[q - 1];
            if (UPPER ? u <= v : u < v) pos = q;
        }
    }
    return pos;
}

__global__ __launch_bounds__(SIM_FLAT_THREADS) void sim_flat_rank_kernel(const float* v, const float* sorted, int n, int P,
                                                                           int32_t* crank, int64_t* nan_count) {
    const int i = blockIdx.x * SIM_FLAT_THREADS + threadIdx.x;
    if (i < n) {
        const float x = v[i];
        crank[i] = sim_count_values<false>(sorted, n, P, x) + sim_count_values<true>(sorted, n, P, x) - n;
    }
    if (i == 0 && nan_count) nan_count[0] = n - sim_count_values<true>(sorted, n, P, INFINITY);      // the NaNs sort last
}

__device__ __forceinline__ double* sim_ws_p1(void* ws, int b) { return (double*)ws + SIM_WS_HEAD + (size_t)b * SIM_WS_P1; }
__device__ __forceinline__ double* sim_ws_p2(void* ws, int grid, int b) {
    return (double*)ws + SIM_WS_HEAD + (size_t)grid * SIM_WS_P1 + (size_t)b * SIM_WS_P2;
}

// the 16 words of a pass-1 record (a partial, or the totals): 7 sums, min x, min y, max x, max y, 3 rank sums, NaNs, 0
__device__ __forceinline__ void sim_store_p1(double* rec, const SimPass1& p, const long long* ic) {
#pragma unroll
    for (int k = 0; k < SIM_NSUM; ++k) rec[k] = p.s[k];
    rec[7] = p.lo[0]; rec[8] = p.lo[1]; rec[9] = p.hi[0]; rec[10] = p.hi[1];
    long long* ri = (long long*)rec;
    ri[11] = ic[0]; ri[12] = ic[1]; ri[13] = ic[2]; ri[14] = p.nan; ri[15] = 0;
}

__global__ __launch_bounds__(SIM_FLAT_THREADS) void sim_flat_part1_kernel(SimFlatLaunch a) {
    constexpr int T = SIM_FLAT_THREADS, NW = T / 64;
    __shared__ SimScratch sc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * SIM_FLAT_CHUNK;
    SimPass1 p;
    long long ic[4] = {0, 0, 0, 0};
#pragma unroll 4
    for (int e = 0; e < SIM_FLAT_CHUNK / T; ++e) {
        const int64_t i = base + tid + e * T;
        if (i < a.n) {
            p.take((double)a.x[i], (double)a.y[i]);
            const long long cx = a.cx[i], cy = a.cy[i];
            ic[0] += cx * cy; ic[1] += cx * cx; ic[2] += cy * cy;
        }
    }
    ic[3] = p.nan;
    sim_reduce_pass1<NW>(p, sc, lane, wave);
    sim_block_reduce<NW>(ic, sc.i, lane, wave, SimAdd());
    p.nan = ic[3];
    if (tid == 0) sim_store_p1(sim_ws_p1(a.ws, blockIdx.x), p, ic);
}

__global__ __launch_bounds__(SIM_FLAT_THREADS) void sim_flat_finish1_kernel(SimFlatLaunch a, int grid) {
    constexpr int T = SIM_FLAT_THREADS, NW = T / 64;
    __shared__ SimScratch sc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SimPass1 p;
    long long ic[4] = {0, 0, 0, 0};
    for (int b = tid; b < grid; b += T) {
        const double* rec = sim_ws_p1(a.ws, b);
        const long long* ri = (const long long*)rec;
#pragma unroll
        for (int k = 0; k < SIM_NSUM; ++k) p.s[k] += rec[k];
        p.lo[0] = fmin(p.lo[0], rec[7]); p.lo[1] = fmin(p.lo[1], rec[8]);
        p.hi[0] = fmax(p.hi[0], rec[9]); p.hi[1] = fmax(p.hi[1], rec[10]);
#pragma unroll
        for (int k = 0; k < 4; ++k) ic[k] += ri[11 + k];
    }
    sim_reduce_pass1<NW>(p, sc, lane, wave);
    sim_block_reduce<NW>(ic, sc.i, lane, wave, SimAdd());
    p.nan = ic[3];
    if (tid == 0) sim_store_p1((double*)a.ws, p, ic);
}

__global__ __launch_bounds__(SIM_FLAT_THREADS) void sim_flat_part2_kernel(SimFlatLaunch a, int grid) {
    constexpr int T = SIM_FLAT_THREADS, NW = T / 64;
    __shared__ SimScratch sc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* head = (const double*)a.ws;
    const double mx = head[0] / (double)a.n, my = head[1] / (double)a.n;
    const int64_t base = (int64_t)blockIdx.x * SIM_FLAT_CHUNK;
    double c[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int e = 0; e < SIM_FLAT_CHUNK / T; ++e) {
        const int64_t i = base + tid + e * T;
        if (i < a.n) {
            const double cx = (double)a.x[i] - mx, cy = (double)a.y[i] - my;
            c[0] += cx * cy; c[1] += cx * cx; c[2] += cy * cy;
        }
    }
    sim_block_reduce<NW>(c, sc.d, lane, wave, SimAdd());
    if (tid == 0) {
        double* rec = sim_ws_p2(a.ws, grid, blockIdx.x);
        rec[0] = c[0]; rec[1] = c[1]; rec[2] = c[2]; rec[3] = 0.0;
    }
}

__global__ __launch_bounds__(SIM_FLAT_THREADS) void sim_flat_finish2_kernel(SimFlatLaunch a, int grid) {
    constexpr int T = SIM_FLAT_THREADS, NW = T / 64;
    __shared__ SimScratch sc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double c[3] = {0.0, 0.0, 0.0};
    for (int b = tid; b < grid; b += T) {
        const double* rec = sim_ws_p2(a.ws, grid, b);
        c[0] += rec[0]; c[1] += rec[1]; c[2] += rec[2];
    }
    sim_block_reduce<NW>(c, sc.d, lane, wave, SimAdd());
    if (tid != 0) return;
    const double* head = (const double*)a.ws;
    const long long* hi64 = (const long long*)a.ws;
    const double lo[2] = {head[7], head[8]}, hi[2] = {head[9], head[10]};
    const long long ic[3] = {hi64[11], hi64[12], hi64[13]};
    sim_close(a.n, head, lo, hi, c, ic, hi64[14], a.out, a.ints);
}

hipError_t launch_sim_flat_rank(const float* v, const float* sorted_v, int64_t n, int32_t* crank, int64_t* nan_count, hipStream_t stream) {
    const SimFlatPlan plan = sim_flat_plan(n);
    if (!plan.ok || !v || !sorted_v || !crank) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + SIM_FLAT_THREADS - 1) / SIM_FLAT_THREADS));
    return launch<sim_flat_rank_kernel>(grid, dim3(SIM_FLAT_THREADS), 0, stream, v, sorted_v, (int)n, plan.pow2, crank, nan_count);
}

hipError_t launch_sim_flat(const SimFlatLaunch& L, hipStream_t stream) {
    const SimFlatPlan plan = sim_flat_plan(L.n);
    if (!plan.ok || !L.x || !L.y || !L.cx || !L.cy || !L.out || !L.ints || !L.ws || ((uintptr_t)L.ws & 7)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)plan.grid), one(1), block(SIM_FLAT_THREADS);
    hipError_t st;
    if ((st = launch<sim_flat_part1_kernel>(grid, block, 0, stream, L)) != hipSuccess) return st;
    if ((st = launch<sim_flat_finish1_kernel>(one, block, 0, stream, L, plan.grid)) != hipSuccess) return st;
    if ((st = launch<sim_flat_part2_kernel>(grid, block, 0, stream, L, plan.grid)) != hipSuccess) return st;
    return launch<sim_flat_finish2_kernel>(one, block, 0, stream, L, plan.grid);
}

// ---- top-k overlap: one wave per query
// A lane owns the elements lane, lane + 64, ... of a[q, :ka] (E of them at most).  It walks a[q, :ka] once to mark those of
// its elements that repeat an earlier one, and b[q, :kb] once to mark those that occur there; the count is the wave's sum of
// first occurrences that b holds.
template <int E>
__global__ __launch_bounds__(256) void topk_overlap_kernel(const int32_t* a, const int32_t* b, int64_t M, int La, int Lb, int k,
                                                           int32_t* count) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (q >= M) return;
    const int ka = k < La ? k : La, kb = k < Lb ? k : Lb;
    const int32_t* ar = a + q * La;
    const int32_t* br = b + q * Lb;
    int32_t own[E];
    uint32_t valid = 0u, dup = 0u, in = 0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        own[e] = 0;
        if (i < ka) { own[e] = ar[i]; valid |= 1u << e; }
    }
    for (int t = 0; t < ka; ++t) {
        const int32_t v = ar[t];
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (own[e] == v && t < lane + 64 * e) dup |= 1u << e;
    }
    for (int t = 0; t < kb; ++t) {
        const int32_t v = br[t];
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (own[e] == v) in |= 1u << e;
    }
    const int c = wave_sum(__popc(in & ~dup & valid));
    if (lane == 0) count[q] = c;
}

hipError_t launch_topk_overlap(const int32_t* a, const int32_t* b, int64_t M, int La, int Lb, int k, int32_t* count, hipStream_t stream) {
    if (M < 0 || M > 0x7fffffffLL || La < 0 || Lb < 0 || k < 1 || k > TOPK_OVERLAP_MAX_K) return hipErrorInvalidValue;
    if (M == 0) return hipSuccess;
    if (!a || !b || !count) return hipErrorInvalidValue;
    const int e = (k + 63) / 64;
    const int E = e <= 1 ? 1 : e <= 2 ? 2 : e <= 4 ? 4 : 16;
    return dispatch<1, 2, 4, 16>(E, [&](auto ec) {
        return launch<topk_overlap_kernel<decltype(ec)::value>>(row_grid(M), dim3(256), 0, stream, a, b, M, La, Lb, k, count);
    });
}
