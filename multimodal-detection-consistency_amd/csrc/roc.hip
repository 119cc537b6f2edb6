// Detection evaluation (src/utils/metrics.py:286-376,816-874: roc_curve / roc_auc_score / Youden threshold / FPR at a TPR /
// precision_recall_curve / bootstrap_metric): the ROC sweep of N scores under B integer weightings, one workgroup per weighting.
//
// The N fp32 scores are sorted ONCE by the caller (descending, stable): scores[pos], labels[pos] and order[pos] (the original index
// of sorted position pos).  A ROW weights the N samples by integer multiplicities w >= 0; a bootstrap resample only changes w.
//   counts  the row's multiplicities over the ORIGINAL indices, uint32, from one of three sources: the caller's weights (plain
//           stores), the caller's draws, or Philox4x32-10 draws made here (integer atomic adds: no arrival order in the result).
//           Two storages, one code: LDS up to ROC_LDS_ROWS samples (RocCounts<true>), else a row of a global workspace
//           (RocCounts<false>: the adds land in L2, so every read is an agent-scope load that does not stop at this CU's L1).
//           The sweep gathers w = counts[order[pos]]: the sources never see the sort.
//   totals  P = sum of w over the positives, N = sum over the negatives; P == 0 or N == 0 is an invalid row (zeros, valid = 0).
//   sweep   chunks of ROC_THREADS sorted positions: a wave scan of (TP << 32 | FP) with the waves' totals through LDS and a carry
//           across chunks; a position is a POINT when it ends a tie group (scores[pos + 1] != scores[pos]; -0.0 == 0.0) whose
//           weight is > 0, i.e. whose cumulative weight exceeds the one at the last group end before it.  Points are compacted
//           into LDS in order.  sklearn keeps a point iff it is the first, the last, or the second difference of FP or of TP is
//           non-zero there: the verdict needs the successor, so a point is evaluated once its successor is known -- the last
//           point of a chunk waits, carried (with its predecessor) in registers, for the next chunk or for the end of the row.
//   eval    per point, exact: auc2 += dFP * (TP + TP_prev) (int64), ap += (dTP / P) * (TP / (TP + FP)) (fp64), and for a kept
//           point J = TP / P - FP / N and |TP / P - target|: two correctly rounded divisions and one subtraction, contraction off.
//           Arg-max of J / arg-min of the distance start from the curve's origin (point index -1: J = 0, distance = target) and
//           ties go to the lower point index: numpy's first arg-extreme over (origin, kept points).
// No float atomics, no inline assembly.  fp64 sums (ap) are per thread in point order, then a fixed tree: identical between runs.
#include "common.hpp"
#include "kernels.hpp"
#include "launch.hpp"

// ---- Philox4x32-10 (Salmon et al., SC'11): counter (c0 .. c3), key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- the row's multiplicities over the original indices: one interface, two storages
template <bool LDS>
struct RocCounts {
    uint32_t* p;
    __device__ __forceinline__ void set(int i, uint32_t v) const { p[i] = v; }
    __device__ __forceinline__ void add(int i) const { atomicAdd(&p[i], 1u); }
    __device__ __forceinline__ uint32_t get(int i) const {
        if (LDS) return p[i];
        return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The workgroup's barrier between two phases over the counts.  The global form's stores and adds are first released at agent
// scope (and waited for): the next phase's adds and agent-scope loads meet them in L2, whichever wave issues them.
template <bool LDS>
__device__ __forceinline__ void roc_publish() {
    if (!LDS) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
}

struct RocPoint { int tp, fp, pos; };

// the best (value, point index) of an arg-extreme with what is reported of it; MAXI: larger wins, else smaller; ties: lower g
struct RocBest { double v; int g, tp, fp, pos; };
template <bool MAXI>
__device__ __forceinline__ void roc_take(RocBest& b, const RocBest& o) {
    const bool better = MAXI ? (o.v > b.v) : (o.v < b.v);
    if (better || (o.v == b.v && o.g < b.g)) b = o;
}
template <bool MAXI>
__device__ __forceinline__ void roc_best_lanes(RocBest& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RocBest x;
        x.v = __shfl_xor(b.v, o, 64); x.g = __shfl_xor(b.g, o, 64); x.tp = __shfl_xor(b.tp, o, 64);
        x.fp = __shfl_xor(b.fp, o, 64); x.pos = __shfl_xor(b.pos, o, 64);
        roc_take<MAXI>(b, x);
    }
}

// what a thread accumulates over the points it evaluates
struct RocAcc {
    long long auc2 = 0;
    double ap = 0.0;
    int kept = 0;
    RocBest yo, tg;
};

struct RocScratch {
    int pt_tp[ROC_THREADS], pt_fp[ROC_THREADS], pt_pos[ROC_THREADS];    // the chunk's points, compacted
    long long wsum[ROC_THREADS / 64];   // the waves' (TP << 32 | FP) totals of the chunk
    int wend[ROC_THREADS / 64];         // cumulative weight, from the wave's start, at the wave's last group end; -1: none
    int wpts[ROC_THREADS / 64];         // the waves' point counts
    int tot[2][ROC_THREADS / 64];       // totals pass: positives' weight, all weight
    // the final reduction
    long long r_auc2[ROC_THREADS / 64];
    double r_ap[ROC_THREADS / 64];
    int r_kept[ROC_THREADS / 64];
    RocBest r_yo[ROC_THREADS / 64], r_tg[ROC_THREADS / 64];
};

// One point with its neighbours; has_pred = it is not the row's first point, has_succ = not its last.
__device__ __forceinline__ void roc_eval(const RocLaunch& a, int g, bool has_pred, const RocPoint& pred, const RocPoint& cur,
                                         bool has_succ, const RocPoint& succ, int P, int Nn, RocAcc& acc) {
#pragma clang fp contract(off)
    const int ptp = has_pred ? pred.tp : 0, pfp = has_pred ? pred.fp : 0;
    acc.auc2 += (long long)(cur.fp - pfp) * (long long)(cur.tp + ptp);
    acc.ap += ((double)(cur.tp - ptp) / (double)P) * ((double)cur.tp / (double)(cur.tp + cur.fp));
    const bool kept = !has_pred || !has_succ || (succ.fp - cur.fp) != (cur.fp - pred.fp) || (succ.tp - cur.tp) != (cur.tp - pred.tp);
    if (a.mode == ROC_MODE_CURVE) {
        a.pt_tp[g] = cur.tp; a.pt_fp[g] = cur.fp; a.pt_pos[g] = cur.pos; a.pt_kept[g] = kept ? 1 : 0;
    }
    if (!kept) return;
    acc.kept += 1;
    const double tpr = (double)cur.tp / (double)P, fpr = (double)cur.fp / (double)Nn;
    RocBest o;
    o.g = g; o.tp = cur.tp; o.fp = cur.fp; o.pos = cur.pos;
    o.v = tpr - fpr;
    roc_take<true>(acc.yo, o);
    o.v = fabs(tpr - a.target);
    roc_take<false>(acc.tg, o);
}

template <bool LDS>
__global__ __launch_bounds__(ROC_THREADS) void roc_kernel(RocLaunch a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t roc_counts_lds[];
    __shared__ RocScratch sc;
    constexpr int T = ROC_THREADS, NW = ROC_THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N;
    const int64_t row = a.row0 + blockIdx.x;
    const RocCounts<LDS> cnt{LDS ? roc_counts_lds : a.ws + (size_t)blockIdx.x * (size_t)roc_ws_stride(N)};

    // ---- counts
    if (a.source == ROC_SRC_WEIGHTS) {
        const int32_t* w = a.src ? a.src + row * N : nullptr;
        for (int i = tid; i < N; i += T) {
            const int32_t v = w ? w[i] : 1;
            cnt.set(i, v > 0 ? (uint32_t)v : 0u);
        }
    } else {
        for (int i = tid; i < N; i += T) cnt.set(i, 0u);
        roc_publish<LDS>();
        if (a.source == ROC_SRC_INDICES) {
            const int32_t* d = a.src + row * N;
            for (int i = tid; i < N; i += T) {
                const int32_t j = d[i];
                if ((uint32_t)j < (uint32_t)N) cnt.add(j);          // a draw outside [0, N) is dropped, never written
            }
        } else {
            const uint32_t b = (uint32_t)(a.first + row), k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
            const int n4 = (N + 3) >> 2;
            for (int c = tid; c < n4; c += T) {
                uint32_t x[4];
                philox4x32_10((uint32_t)c, b, 0u, 0u, k0, k1, x);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * c + j < N) cnt.add((int)(((uint64_t)x[j] * (uint64_t)(uint32_t)N) >> 32));     // < N
            }
        }
    }
    roc_publish<LDS>();

    // ---- totals (and the read-back of the multiplicities over the sorted positions)
    uint32_t sp = 0, sw = 0;
    for (int pos = tid; pos < N; pos += T) {
        const int o = a.order[pos];
        const uint32_t w = (uint32_t)o < (uint32_t)N ? cnt.get(o) : 0u;
        if (a.mode == ROC_MODE_WEIGHTS) a.w_out[row * N + pos] = (int32_t)w;
        sp += a.labels[pos] ? w : 0u;
        sw += w;
    }
    if (a.mode == ROC_MODE_WEIGHTS) return;
    sp = (uint32_t)wave_sum((int)sp);
    sw = (uint32_t)wave_sum((int)sw);
    if (lane == 0) { sc.tot[0][wave] = (int)sp; sc.tot[1][wave] = (int)sw; }
    __syncthreads();
    int P = 0, W = 0;
#pragma unroll
    for (int w2 = 0; w2 < NW; ++w2) { P += sc.tot[0][w2]; W += sc.tot[1][w2]; }
    const int Nn = W - P;
    const bool sweep = a.mode == ROC_MODE_SWEEP;
    if (P <= 0 || Nn <= 0) {                                           // an invalid row: zeros, not an error
        if (tid == 0) {
            if (sweep) {
                a.n_pos[row] = 0; a.n_neg[row] = 0; a.valid[row] = 0; a.n_points[row] = 0; a.n_kept[row] = 0;
                a.auc2[row] = 0; a.auc[row] = 0.0; a.ap[row] = 0.0; a.youden_j[row] = 0.0;
                a.youden_pos[row] = 0; a.youden_tp[row] = 0; a.youden_fp[row] = 0;
                a.target_pos[row] = 0; a.target_tp[row] = 0; a.target_fp[row] = 0;
                for (int t = 0; t < a.n_thr; ++t) { a.thr_tp[row * a.n_thr + t] = 0; a.thr_fp[row * a.n_thr + t] = 0; }
            } else {
                a.pt_count[0] = 0; a.pt_count[1] = 0;
            }
        }
        return;
    }

    // ---- sweep
    RocAcc acc;
    acc.yo = RocBest{0.0, -1, 0, 0, -1};                               // the origin: J = 0
    acc.tg = RocBest{fabs(0.0 - a.target), -1, 0, 0, -1};              // the origin: |0 - target|
    if (tid != 0) { acc.yo.g = 0x7fffffff; acc.yo.v = -INFINITY; acc.tg.g = 0x7fffffff; acc.tg.v = INFINITY; }   // one owner
    long long carry = 0;                // (TP << 32 | FP) before the chunk
    int prev_end = 0;                   // cumulative weight at the last group end before the chunk
    int g0 = 0;                         // points before the chunk
    RocPoint cA{0, 0, -1}, cB{0, 0, -1};// points g0 - 2 and g0 - 1
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int c0 = 0; c0 < N; c0 += T) {
        const int pos = c0 + tid;
        const bool in = pos < N;
        uint32_t w = 0;
        int lab = 0;
        float s = 0.f, sn = 0.f;
        bool end = false;
        if (in) {
            const int o = a.order[pos];
            w = (uint32_t)o < (uint32_t)N ? cnt.get(o) : 0u;
            lab = a.labels[pos];
            s = a.scores[pos];
            sn = pos + 1 < N ? a.scores[pos + 1] : 0.f;
            end = pos == N - 1 || sn != s;
        }
        const long long incl = wave_inclusive_scan(lab ? ((long long)w << 32) : (long long)w, lane);
        const int lw = (int)(incl >> 32) + (int)(incl & 0xffffffffLL);            // weight from the wave's start
        const uint64_t emask = __ballot(end);
        const int hl = emask ? 63 - __clzll((long long)emask) : 0;
        const int lw_last = __shfl(lw, hl, 64);
        if (lane == 63) sc.wsum[wave] = incl;
        if (lane == 0) sc.wend[wave] = emask ? lw_last : -1;
        __syncthreads();
        long long run = carry, base = 0;
        int pe = prev_end, my_pe = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
            if (w2 == wave) { base = run; my_pe = pe; }
            const int e = sc.wend[w2];
            if (e >= 0) pe = (int)(run >> 32) + (int)(run & 0xffffffffLL) + e;
            run += sc.wsum[w2];
        }
        const uint64_t lower = emask & below;
        const int pl = lower ? 63 - __clzll((long long)lower) : 0;
        const int lw_prev = __shfl(lw, pl, 64);
        const int base_w = (int)(base >> 32) + (int)(base & 0xffffffffLL);
        const int before = lower ? base_w + lw_prev : my_pe;          // cumulative weight at the last group end before pos
        const long long cum = base + incl;
        const int ctp = (int)(cum >> 32), cfp = (int)(cum & 0xffffffffLL);
        const bool pt = end && ctp + cfp > before;
        if (sweep && in) {
            for (int t = 0; t < a.n_thr; ++t)
                if (s >= a.thr[t] && (pos == N - 1 || !(sn >= a.thr[t]))) { a.thr_tp[row * a.n_thr + t] = ctp; a.thr_fp[row * a.n_thr + t] = cfp; }
        }
        const uint64_t pmask = __ballot(pt);
        if (lane == 0) sc.wpts[wave] = __popcll(pmask);
        __syncthreads();
        int k = 0, pbase = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
            if (w2 == wave) pbase = k;
            k += sc.wpts[w2];
        }
        if (pt) {
            const int e = pbase + __popcll(pmask & below);
            sc.pt_tp[e] = ctp; sc.pt_fp[e] = cfp; sc.pt_pos[e] = pos;
        }
        __syncthreads();
        // thread tid takes the point j = tid - 1 of (carried last, the chunk's points); the chunk's last point waits
        const int j = tid - 1;
        if (j < 0 ? (g0 >= 1 && k >= 1) : j <= k - 2) {
            const RocPoint cur = j < 0 ? cB : RocPoint{sc.pt_tp[j], sc.pt_fp[j], sc.pt_pos[j]};
            const RocPoint pred = j < 0 ? cA : j == 0 ? cB : RocPoint{sc.pt_tp[j - 1], sc.pt_fp[j - 1], sc.pt_pos[j - 1]};
            const RocPoint succ{sc.pt_tp[j + 1], sc.pt_fp[j + 1], sc.pt_pos[j + 1]};
            roc_eval(a, g0 + j, g0 + j > 0, pred, cur, true, succ, P, Nn, acc);
        }
        if (k >= 2) {
            cA = RocPoint{sc.pt_tp[k - 2], sc.pt_fp[k - 2], sc.pt_pos[k - 2]};
            cB = RocPoint{sc.pt_tp[k - 1], sc.pt_fp[k - 1], sc.pt_pos[k - 1]};
        } else if (k == 1) {
            cA = cB;
            cB = RocPoint{sc.pt_tp[0], sc.pt_fp[0], sc.pt_pos[0]};
        }
        g0 += k;
        carry = run;
        prev_end = pe;
    }
    // the row's last point (a valid row has weight, so it has one): kept by rule
    if (tid == 0 && g0 >= 1) roc_eval(a, g0 - 1, g0 > 1, cA, cB, false, cB, P, Nn, acc);

    // ---- the row's results: integer sums, a fixed tree for ap, the two arg-extremes
    acc.auc2 = wave_sum(acc.auc2);
    acc.ap = wave_sum(acc.ap);
    acc.kept = wave_sum(acc.kept);
    roc_best_lanes<true>(acc.yo);
    roc_best_lanes<false>(acc.tg);
    if (lane == 0) {
        sc.r_auc2[wave] = acc.auc2; sc.r_ap[wave] = acc.ap; sc.r_kept[wave] = acc.kept; sc.r_yo[wave] = acc.yo; sc.r_tg[wave] = acc.tg;
    }
    __syncthreads();
    if (tid != 0) return;
    long long auc2 = 0;
    double ap = 0.0;
    int kept = 0;
    RocBest yo = sc.r_yo[0], tg = sc.r_tg[0];
    for (int w2 = 0; w2 < NW; ++w2) {
        auc2 += sc.r_auc2[w2]; ap += sc.r_ap[w2]; kept += sc.r_kept[w2];
        if (w2 > 0) { roc_take<true>(yo, sc.r_yo[w2]); roc_take<false>(tg, sc.r_tg[w2]); }
    }
    if (!sweep) {
        a.pt_count[0] = g0; a.pt_count[1] = kept;
        return;
    }
    a.n_pos[row] = P; a.n_neg[row] = Nn; a.valid[row] = 1; a.n_points[row] = g0; a.n_kept[row] = kept;
    a.auc2[row] = auc2;
    a.auc[row] = (double)auc2 / (2.0 * (double)P * (double)Nn);
    a.ap[row] = ap;
    a.youden_j[row] = yo.v; a.youden_pos[row] = yo.pos; a.youden_tp[row] = yo.tp; a.youden_fp[row] = yo.fp;
    a.target_pos[row] = tg.pos; a.target_tp[row] = tg.tp; a.target_fp[row] = tg.fp;
    // a threshold above every score has no position that ends `score >= thr` (the sweep wrote nothing): it counts nothing
    for (int t = 0; t < a.n_thr; ++t)
        if (!(a.scores[0] >= a.thr[t])) { a.thr_tp[row * a.n_thr + t] = 0; a.thr_fp[row * a.n_thr + t] = 0; }
}

hipError_t launch_roc(const RocLaunch& L, hipStream_t stream) {
    if (L.N < 1 || L.N > ROC_MAX_N || L.B < 1 || L.B > 0x7fffffffLL || L.n_thr < 0 || L.n_thr > ROC_MAX_THR || !L.scores || !L.labels ||
        !L.order || !(L.target >= 0.0 && L.target <= 1.0))
        return hipErrorInvalidValue;
    if (L.source != ROC_SRC_WEIGHTS && L.source != ROC_SRC_INDICES && L.source != ROC_SRC_PHILOX) return hipErrorInvalidValue;
    if (L.source == ROC_SRC_INDICES && !L.src) return hipErrorInvalidValue;
    if (L.mode == ROC_MODE_WEIGHTS ? !L.w_out : L.mode == ROC_MODE_CURVE ? (L.B != 1 || !L.pt_tp || !L.pt_fp || !L.pt_pos || !L.pt_kept || !L.pt_count)
                                                                         : L.mode != ROC_MODE_SWEEP)
        return hipErrorInvalidValue;
    if (L.ws) return launch<roc_kernel<false>>(dim3((unsigned)L.B), dim3(ROC_THREADS), 0, stream, L);
    constexpr size_t MAX_LDS = (size_t)ROC_LDS_ROWS * 4;
    if (L.N > ROC_LDS_ROWS || L.lds_bytes < (size_t)L.N * 4) return hipErrorInvalidValue;
    return launch<roc_kernel<true>, MAX_LDS>(dim3((unsigned)L.B), dim3(ROC_THREADS), L.lds_bytes, stream, L);
}
