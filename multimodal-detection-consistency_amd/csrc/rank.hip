// Retrieval evaluation over a registered bank slot (src/utils/metrics.py:379-573: Recall@K / mAP / MRR / NDCG): the rank of
// every RELEVANT bank row of every query, however deep it sits, without a [Q, N] matrix and without a sort of a row.
//
// Relevance comes from labels: (i, j) is relevant iff qlabel[i] == glabel[j] >= 0; a relevant row of a query is a TARGET.
// The order is cand_better (score desc, row asc).  The 0-based position of a target t of query i is
//     pos(t) = (targets of i ahead of t) + (irrelevant rows of i ahead of t),
// and every metric is a pure function of the positions.
//
//   tile    `rank_tile_kernel<COUNT>`: a workgroup owns 256 bank rows on the lane dimension and walks the query tiles on the MFMA
//           row dimension (gemm_core.hpp: gemm_mainloop, the gemm_acc_t layout); no score leaves the accumulators except a target's.
//     EMIT    every relevant element writes (score, row) to slot tgt_off[i] + gpos[j] of the query's target list; gpos[j] is
//             row j's place inside its label group in ascending row order, so every slot is written exactly once: no atomics.
//     COUNT   takes the lists back in rank order.  An irrelevant element is dropped by one compare against the score of the
//             query's LAST target (tlow, +inf for a query without targets and for the padding rows); the others binary-search
//             the list for the first target b they are ahead of and add 1 to hist[tgt_off[i] + b] -- an integer atomic, so the
//             counts do not depend on the scheduling.  Relevant elements never count: the mutual order of a query's targets
//             is the list's, so its positions are distinct whatever the rounding.  A NaN score fails every compare.
//   metrics `rank_metrics_kernel`: one wave per query; pos[c] = c + sum_{b <= c} hist[b] by a wave scan in chunks of 64, then
//           AP, RR and per k (hits, DCG, IDCG) in fp64.  Nothing is reduced over the queries on the device.
// Products as slot_operands (gemm_core.hpp) orders them: queries split into (hi | lo) bf16 planes, 2 products on a bf16 slot, 3
// on an fp32 slot.  LDS holds the main loop's 128 KiB and nothing else: the counters are global, which is why the slow path of
// COUNT must be (and, behind the tlow compare, is) rare.
#include "gemm_core.hpp"
#include "kernels.hpp"
#include "launch.hpp"

typedef __attribute__((ext_vector_type(4))) int32_t i32x4_t;

// qlab[i] = qlabel[i], -1 for the padding M <= i < Mpad; with tgt_off also tlow[i] = the score of query i's last target in
// rank order, +inf for a query without targets and for the padding
__global__ __launch_bounds__(256) void rank_prep_kernel(const int32_t* __restrict__ qlabel, int M, int Mpad,
                                                        const int64_t* __restrict__ tgt_off, const float* __restrict__ tgt_sim,
                                                        int32_t* __restrict__ qlab, float* __restrict__ tlow) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Mpad) return;
    qlab[i] = i < M ? qlabel[i] : -1;
    if (tlow) {
        float t = INFINITY;
        if (i < M && tgt_off[i + 1] > tgt_off[i]) t = tgt_sim[tgt_off[i + 1] - 1];
        tlow[i] = t;
    }
}

struct RankTileArgs {
    const int32_t* qlab;       // [n_qtiles * 256], -1 beyond M
    const int32_t* glabel;     // [R]
    const int32_t* gpos;       // [R]            (EMIT)
    const float* tlow;         // [n_qtiles * 256] (COUNT)
    const int64_t* tgt_off;    // [M + 1]
    float* tgt_sim;            // [T]: written by EMIT, read in rank order by COUNT
    int32_t* tgt_row;          // [T]
    int32_t* hist;             // [T]            (COUNT)
    int M, R;
};

// COUNT's slow path: the first target of query i that the irrelevant element (s, j) is ahead of takes one count
__device__ __forceinline__ void rank_count_one(const RankTileArgs& e, int i, float s, int j) {
    const int64_t beg = e.tgt_off[i];
    int lo = 0, hi = (int)(e.tgt_off[i + 1] - beg);          // the answer is in [lo, hi]; hi = P means none
    const int P = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cand_better(s, j, e.tgt_sim[beg + mid], e.tgt_row[beg + mid])) hi = mid; else lo = mid + 1;
    }
    if (lo < P) atomicAdd(&e.hist[beg + lo], 1);             // integer: the counts do not depend on the order
}

template <bool COUNT>
__global__ __launch_bounds__(GEMM_THREADS) void rank_tile_kernel(GemmOperands g, RankTileArgs e, int n_qtiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int j0 = blockIdx.x * GEMM_BN;
    // the lane's four bank rows: label, place in the label group, in range
    int gl[4], gp[4];
    bool jin[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int j = gemm_acc_col(j0, wave, lane, n);
        jin[n] = j < e.R;
        gl[n] = jin[n] ? e.glabel[j] : -1;
        gp[n] = (!COUNT && jin[n]) ? e.gpos[j] : 0;
    }
    for (int qt = 0; qt < n_qtiles; ++qt) {
        gemm_acc_t acc;
        gemm_zero_acc(acc);
        gemm_mainloop(acc, g, qt * GEMM_BM, j0, smem);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i0 = gemm_acc_row(qt * GEMM_BM, wave, lane, m);
            const i32x4_t ql = *(const i32x4_t*)(e.qlab + i0);
            f32x4_t tl = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (COUNT) tl = *(const f32x4_t*)(e.tlow + i0);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                // the elements of this block that have work to do, as a mask over r
                unsigned todo = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool rel = ql[r] == gl[n] && ql[r] >= 0;           // a padding row has ql = -1, a padding column gl = -1
                    const bool hit = COUNT ? (!rel && jin[n] && acc[m][n][r] >= tl[r]) : rel;
                    todo |= (unsigned)hit << r;
                }
                const int j = gemm_acc_col(j0, wave, lane, n);
                while (todo) {
                    const int r = __builtin_ctz(todo);
                    todo &= todo - 1;
                    const float s = r == 0 ? acc[m][n][0] : r == 1 ? acc[m][n][1] : r == 2 ? acc[m][n][2] : acc[m][n][3];
                    const int i = i0 + r;
                    if (i >= e.M) continue;              // COUNT only: an overflowed score may equal the padding's +inf
                    if (COUNT) {
                        rank_count_one(e, i, s, j);
                    } else {
                        const int64_t slot = e.tgt_off[i] + gp[n];
                        if (gp[n] < 0 || slot >= e.tgt_off[i + 1]) continue;     // a gpos that is not the group's: never out of the list
                        e.tgt_sim[slot] = s;
                        e.tgt_row[slot] = j;
                    }
                }
            }
        }
    }
}

struct RankMetricsArgs {
    const int64_t* tgt_off;    // [M + 1]
    const int32_t* hist;       // [T]
    int32_t* pos;              // [T]
    double* ap;                // [M]
    double* rr;                // [M]
    int32_t* hits;             // [M, n_k]
    double* dcg;               // [M, n_k]
    double* idcg;              // [M, n_k]
    int M, n_k;
    int k[RANK_MAX_K];
};

__global__ __launch_bounds__(256) void rank_metrics_kernel(RankMetricsArgs a) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.M) return;
    const int64_t beg = a.tgt_off[q];
    const int64_t P = a.tgt_off[q + 1] - beg;
    double ap = 0.0, dcg[RANK_MAX_K];
    int hits[RANK_MAX_K];
#pragma unroll
    for (int t = 0; t < RANK_MAX_K; ++t) { dcg[t] = 0.0; hits[t] = 0; }
    int carry = 0, first = 0;                                // irrelevant rows ahead of the chunk; pos of target 0
    for (int64_t c0 = 0; c0 < P; c0 += 64) {
        const int64_t c = c0 + lane;
        const int v = wave_inclusive_scan(c < P ? a.hist[beg + c] : 0, lane);
        if (c < P) {
            const int64_t p = c + carry + v;
            a.pos[beg + c] = (int32_t)p;
            ap += (double)(c + 1) / (double)(p + 1);
            const double gain = 1.0 / log2((double)(p + 2));
#pragma unroll
            for (int t = 0; t < RANK_MAX_K; ++t)
                if (t < a.n_k && p < a.k[t]) { hits[t] += 1; dcg[t] += gain; }
        }
        if (c0 == 0) first = __shfl(v, 0, 64);
        carry += __shfl(v, 63, 64);
    }
    ap = wave_sum(ap);
    if (lane == 0) {
        a.ap[q] = P > 0 ? ap / (double)P : 0.0;
        a.rr[q] = P > 0 ? 1.0 / (double)(first + 1) : 0.0;
    }
#pragma unroll
    for (int t = 0; t < RANK_MAX_K; ++t) {
        if (t >= a.n_k) break;
        const int64_t n_ideal = P < a.k[t] ? P : a.k[t];
        double ideal = 0.0;
        for (int64_t c = lane; c < n_ideal; c += 64) ideal += 1.0 / log2((double)(c + 2));
        ideal = wave_sum(ideal);
        const double d = wave_sum(dcg[t]);
        const int hsum = wave_sum(hits[t]);
        if (lane == 0) {
            a.hits[(int64_t)q * a.n_k + t] = hsum;
            a.dcg[(int64_t)q * a.n_k + t] = d;
            a.idcg[(int64_t)q * a.n_k + t] = ideal;
        }
    }
}

template <bool COUNT>
static hipError_t launch_rank_tile(const RankTileLaunch& L, hipStream_t stream) {
    const BankRows& B = L.bank;
    if (!slot_tile_ok(B, 0x7fffffffLL) || L.M < 1) return hipErrorInvalidValue;
    const int n_qtiles = (L.M + GEMM_BM - 1) / GEMM_BM;
    const int Mpad = n_qtiles * GEMM_BM;
    hipError_t st = launch<rank_prep_kernel>(dim3((Mpad + 255) / 256), dim3(256), 0, stream, L.qlabel, L.M, Mpad,
                                             COUNT ? L.tgt_off : (const int64_t*)nullptr, (const float*)L.tgt_sim, L.qlab,
                                             COUNT ? L.tlow : (float*)nullptr);
    if (st != hipSuccess) return st;
    // queries on the MFMA row dimension (A), bank rows on the lane dimension (B)
    const GemmOperands g = slot_operands(L.qplanes, L.M, B);
    RankTileArgs e;
    e.qlab = L.qlab; e.glabel = L.glabel; e.gpos = L.gpos; e.tlow = L.tlow; e.tgt_off = L.tgt_off;
    e.tgt_sim = L.tgt_sim; e.tgt_row = L.tgt_row; e.hist = L.hist; e.M = L.M; e.R = (int)B.R;
    const int64_t n_btiles = (B.R + GEMM_BN - 1) / GEMM_BN;
    return launch<rank_tile_kernel<COUNT>, GEMM_LDS_BYTES>(dim3((unsigned)n_btiles), dim3(GEMM_THREADS), GEMM_LDS_BYTES, stream, g, e,
                                                           n_qtiles);
}

hipError_t launch_rank_targets(const RankTileLaunch& L, hipStream_t stream) { return launch_rank_tile<false>(L, stream); }
hipError_t launch_rank_count(const RankTileLaunch& L, hipStream_t stream) { return launch_rank_tile<true>(L, stream); }

hipError_t launch_rank_metrics(const RankMetricsLaunch& L, hipStream_t stream) {
    if (L.M < 1 || L.n_k < 0 || L.n_k > RANK_MAX_K) return hipErrorInvalidValue;
    RankMetricsArgs a;
    a.tgt_off = L.tgt_off; a.hist = L.hist; a.pos = L.pos; a.ap = L.ap; a.rr = L.rr; a.hits = L.hits; a.dcg = L.dcg; a.idcg = L.idcg;
    a.M = L.M; a.n_k = L.n_k;
    for (int t = 0; t < RANK_MAX_K; ++t) a.k[t] = t < L.n_k ? L.k[t] : 0;
    return launch<rank_metrics_kernel>(dim3((L.M + 3) / 4), dim3(256), 0, stream, a);
}
