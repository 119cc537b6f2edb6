// IVF search over a bank slot whose rows are stored in list order (the search half of faiss.IndexIVFFlat, src/retrieval.py:
// 101-103; kmeans.hip is the training half).  An index = centroids fp32 [nlist, D], the rows in list order, list_offsets
// int32 [nlist + 1] and row_ids int32 [R] (the original index of every stored row).
//
//   probe   the nprobe best lists of a query by q.c - |c|^2 / 2 (kmeans_assign's score and order, so a row sits in the list
//           this rule ranks first for it): the plane GEMM writes [chunk, nlist] scores, `ivf_probe_select_kernel` (one
//           workgroup per query) subtracts the half norms and takes nprobe rounds of block arg-max by cand_better
//           (select.hpp, no payload).  NaN scores never win; ranks without a list are -1 / -inf.
//   invert  the flattened probes [chunk * nprobe] are labels over the lists: kmeans.hip's stable counting sort gives, per
//           list, the (query, probe) pairs that read it.
//   scan    `ivf_scan_kernel`, list-major: a work item = (list, chunk of <= 512 rows).  The item walks its rows with the skinny
//           stream (skinny.hpp) once per group of <= 64 pairs (32 at D = 768: both query planes of the group are one LDS image),
//           the group's query rows gathered by pair.  bf16 slot: bank x (query hi | lo), exact products; fp32 slot: the
//           hi plane of a 16-row group x (query hi | lo), then its lo plane x (query hi | lo) through the second register
//           set into the same accumulators -- all FOUR products: the flat search's hi.hi + lo.hi + hi.lo drops lo.lo,
//           which is |lo|^2 ~ 1e-6 |x|^2 when the query IS a bank row (self-retrieval; the flat path re-scores its
//           candidates in fp32 instead, the scan has no second pass).  The accumulators are the result, so every
//           64-deep block has a short MFMA chain of its own, added by the vector ALU (skinny_mfma_blocks).  Every lane stores its 4 rows x one query as one 16-byte store into
//           scores[pair * pitch + row in list]: no atomics, no candidate lists, every value written exactly once.
//   select  `ivf_select_kernel`, one workgroup per query over its nprobe segments (lengths from list_offsets): k rounds of
//           block arg-max by (similarity desc, original row id asc) (select.hpp; the winner's stored position and segment
//           travel with it); the segments are copied to LDS first when they fit.
//           NaN and -inf similarities are never returned; short results are padded with -1 / -inf.
// A probed list longer than the declared max_list_rows is read up to max_list_rows rows and raises bit 2 of the overflow word.
#include "kernels.hpp"
#include "launch.hpp"
#include "select.hpp"
#include "skinny.hpp"

#define IVF_T 1024

// ---- probe -------------------------------------------------------------------------------------------------------
// sims [*, nlist]: the plane GEMM's q.c of one chunk of queries; lists / score [*, nprobe] of the same queries
__global__ __launch_bounds__(IVF_T) void ivf_probe_select_kernel(float* __restrict__ sims, const float* __restrict__ halfnorm,
                                                                 int nlist, int nprobe, int32_t* __restrict__ lists,
                                                                 float* __restrict__ score) {
    __shared__ BestSlots<IVF_T, 0> red;
    const int q = blockIdx.x, t = threadIdx.x;
    float* row = sims + (int64_t)q * nlist;
    // thread t owns the entries t, t + IVF_T, ...: it alone reads and strikes them, so no barrier orders the two
    for (int i = t; i < nlist; i += IVF_T) row[i] = row[i] - halfnorm[i];
    for (int r = 0; r < nprobe; ++r) {
        Best<0> b;
        for (int i = t; i < nlist; i += IVF_T) {
            const float v = row[i];
            if (v > -INFINITY) best_take(b, Best<0>{v, i});      // false for NaN and for a struck entry
        }
        const Best<0> f = block_best(b, red, r);
        const bool none = f.id == CAND_NONE;
        if (t == 0) {
            lists[(int64_t)q * nprobe + r] = none ? -1 : f.id;
            if (score) score[(int64_t)q * nprobe + r] = none ? -INFINITY : f.v;
        }
        if (!none && (f.id & (IVF_T - 1)) == t) row[f.id] = -INFINITY;      // taken
    }
}

hipError_t launch_ivf_probe(const IvfProbeLaunch& L, hipStream_t stream) {
    if (L.M < 1 || L.nlist < 1 || L.nprobe < 1 || L.D < 64 || L.D % 64 != 0 || L.chunk < 1) return hipErrorInvalidValue;
    hipError_t st = launch_kmeans_halfnorm(L.centroids, L.D, L.nlist, L.nlist, L.halfnorm, stream);
    if (st != hipSuccess) return st;
    for (int m0 = 0; m0 < L.M; m0 += L.chunk) {
        const int m = L.M - m0 < L.chunk ? L.M - m0 : L.chunk;
        // centroids on the rows of A as an fp32 bank's planes: chi.qhi + chi.qlo + clo.qhi
        const GemmLaunch G = gemm_launch_planes(L.cplanes, 2 * (int64_t)L.D, L.nlist, 2, L.qplanes + (int64_t)m0 * 2 * L.D, m, L.D,
                                                L.sims, L.nlist);
        st = launch_gemm_bf16(G, stream);
        if (st != hipSuccess) return st;
        st = launch<ivf_probe_select_kernel>(dim3(m), dim3(IVF_T), 0, stream, L.sims, (const float*)L.halfnorm, L.nlist, L.nprobe,
                                             L.lists + (int64_t)m0 * L.nprobe, L.score ? L.score + (int64_t)m0 * L.nprobe : nullptr);
        if (st != hipSuccess) return st;
    }
    return hipSuccess;
}

// ---- scan --------------------------------------------------------------------------------------------------------
// the rows a probe of list l reads: stored positions [beg, beg + len), len = min(the list's length, max_list_rows); a list that
// does not lie inside the slot's R rows (offsets that are not this slot's) is cut to the rows that do.  over: it was longer
__device__ __forceinline__ int ivf_list_rows(const int32_t* __restrict__ list_offsets, int l, int max_list_rows, int64_t R, int& beg,
                                             bool& over) {
    beg = list_offsets[l];
    int64_t len = (int64_t)list_offsets[l + 1] - beg;
    if (beg < 0 || beg >= R) len = 0;
    if (len > R - beg) len = R - beg;
    over = len > max_list_rows;
    if (over) len = max_list_rows;
    return len > 0 ? (int)len : 0;
}
// grid (nlist, row chunks).  BP = the slot's planes (1: bf16 rows, 2: the hi | lo planes of fp32 rows); the LDS image holds
// both query planes of 16 * NQT pairs at row pitch 4 D + 16 bytes.  pair_order / pair_offsets: the chunk's pairs grouped by
// list; pair p belongs to query p / nprobe of the chunk and owns scores[p * pitch, (p + 1) * pitch).
template <int KB, int NQT, int BP>
__global__ __launch_bounds__(512) void ivf_scan_kernel(const uint16_t* __restrict__ bank, int64_t ldb,
                                                        const uint16_t* __restrict__ qplanes,
                                                        const int32_t* __restrict__ list_offsets, int64_t R,
                                                        const int32_t* __restrict__ pair_offsets,
                                                        const int32_t* __restrict__ pair_order, int nprobe, int max_list_rows,
                                                        int64_t pitch, float* __restrict__ scores, int32_t* __restrict__ overflow) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = KB * 64, QPITCH = 4 * D + 16, G = NQT * 16;
    const int l = blockIdx.x;
    const int p0 = pair_offsets[l], np = pair_offsets[l + 1] - p0;
    if (np <= 0) return;                                      // nobody probes this list
    int beg32;
    bool over;
    const int len = ivf_list_rows(list_offsets, l, max_list_rows, R, beg32, over);
    if (over && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(overflow, 4);     // never truncated silently
    const int64_t beg = beg32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const char* qbase = smem + r16 * QPITCH + g * 32;
    for (int64_t c = blockIdx.y; c * IVF_CHUNK_ROWS < len; c += gridDim.y) {
        const int r_lo = (int)(c * IVF_CHUNK_ROWS);
        const int r_hi = len - r_lo < IVF_CHUNK_ROWS ? len : r_lo + IVF_CHUNK_ROWS;
        const int n_groups = (r_hi - r_lo + 15) >> 4;
        // the rows of group grp, plane `plane`; rows past the chunk's end are clamped (their products land in the pitch's
        // padding or in rows the select pass never reads)
        auto load_group = [&](int grp, int plane, u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) {
            int r = r_lo + grp * 16 + r16;
            if (r >= r_hi) r = r_hi - 1;
            skinny_load_group<KB, false>(bank + (beg + r) * ldb + plane * D + g * 16, a);
        };
        for (int pg = 0; pg < np; pg += G) {
            u32x4_t a0[2 * KB], a1[2 * KB];
            if (wave < n_groups) load_group(wave, 0, a0);
            __syncthreads();                                  // the previous image has been read
            // ---- the group's query planes, gathered by pair (pairs past the list's last: zeros)
            for (int idx = tid; idx < G * (D / 4); idx += 512) {
                const int j = idx / (D / 4), piece = idx - j * (D / 4);
                u32x4_t v = u32x4_t{0u, 0u, 0u, 0u};
                if (pg + j < np) {
                    const int q = pair_order[p0 + pg + j] / nprobe;
                    v = *(const u32x4_t*)(qplanes + (int64_t)q * 2 * D + piece * 8);
                }
                *(u32x4_t*)(smem + j * QPITCH + piece * 16) = v;
            }
            int64_t out_base[NQT];                            // < 0: the lane's column holds no pair
#pragma unroll
            for (int n = 0; n < NQT; ++n) {
                const int j = pg + n * 16 + r16;
                out_base[n] = j < np ? (int64_t)pair_order[p0 + j] * pitch + r_lo + 4 * g : -1;
            }
            __syncthreads();
            auto store_group = [&](int grp, const f32x4_t (&acc)[NQT]) __attribute__((always_inline)) {
#pragma unroll
                for (int n = 0; n < NQT; ++n)
                    if (out_base[n] >= 0) *(f32x4_t*)(scores + out_base[n] + grp * 16) = acc[n];
            };
            if constexpr (BP == 1) {
                auto load = [&](int grp, u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) { load_group(grp, 0, a); };
                auto compute = [&](int grp, const u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) {
                    f32x4_t acc[NQT];
#pragma unroll
                    for (int n = 0; n < NQT; ++n) acc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                    skinny_mfma_blocks<KB, NQT, 2, QPITCH>(a, qbase, acc);
                    store_group(grp, acc);
                };
                skinny_walk(wave, n_groups, a0, a1, load, compute);
            } else {
                for (int grp = wave; grp < n_groups; grp += 8) {
                    load_group(grp, 1, a1);
                    f32x4_t acc[NQT];
#pragma unroll
                    for (int n = 0; n < NQT; ++n) acc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                    skinny_mfma_blocks<KB, NQT, 2, QPITCH>(a0, qbase, acc);          // hi x (query hi | lo)
                    if (grp + 8 < n_groups) load_group(grp + 8, 0, a0);
                    skinny_mfma_blocks<KB, NQT, 2, QPITCH>(a1, qbase, acc);          // lo x (query hi | lo)
                    store_group(grp, acc);
                }
            }
        }
        __syncthreads();
    }
}

// ---- select ------------------------------------------------------------------------------------------------------
// one workgroup per query of the chunk; segment j = the first min(length of list probes[q, j], max_list_rows) floats of pair
// q * nprobe + j.  Element i of a segment is owned by thread i & (IVF_T - 1): only that thread copies, reads and strikes it.
__global__ __launch_bounds__(IVF_T) void ivf_select_kernel(float* __restrict__ scores, int64_t pitch, const int32_t* __restrict__ probes,
                                                           int nprobe, const int32_t* __restrict__ list_offsets, int nlist,
                                                           int64_t R, int max_list_rows, const int32_t* __restrict__ row_ids, int64_t idx_offset,
                                                           int k, int use_lds, int32_t* __restrict__ topk_idx,
                                                           float* __restrict__ topk_sim, int32_t* __restrict__ topk_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* vals = (float*)smem;
    __shared__ BestSlots<IVF_T, 2> red;      // payload: the stored position and the segment
    __shared__ int seg_beg[128], seg_len[128], seg_base[128];
    const int q = blockIdx.x, t = threadIdx.x;
    if (t < nprobe) {
        const int l = probes[(int64_t)q * nprobe + t];
        int beg = 0, len = 0;
        bool over;
        if ((unsigned)l < (unsigned)nlist) len = ivf_list_rows(list_offsets, l, max_list_rows, R, beg, over);
        seg_beg[t] = beg; seg_len[t] = len;
    }
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int j = 0; j < nprobe; ++j) { seg_base[j] = run; run += seg_len[j]; }
    }
    __syncthreads();
    float* const mine = scores + (int64_t)q * nprobe * pitch;
    if (use_lds) {
        for (int j = 0; j < nprobe; ++j) {
            const int len = seg_len[j];
            const float* src = mine + (int64_t)j * pitch;
            float* dst = vals + seg_base[j];
            for (int i = t; i < len; i += IVF_T) dst[i] = src[i];
        }
    }
    for (int r = 0; r < k; ++r) {
        Best<2> b;
        b.pay[0] = 0; b.pay[1] = 0;
        for (int j = 0; j < nprobe; ++j) {
            const int len = seg_len[j];
            if (len == 0) continue;
            const int beg = seg_beg[j];
            const float* src = use_lds ? vals + seg_base[j] : mine + (int64_t)j * pitch;
            for (int i = t; i < len; i += IVF_T) {
                const float v = src[i];
                // NaN, -inf and struck entries fail the first test; the original id is read only where it can decide
                if (v > -INFINITY && v >= b.v) best_take(b, Best<2>{v, row_ids ? row_ids[beg + i] : beg + i, {beg + i, j}});
            }
        }
        const Best<2> f = block_best(b, red, r);
        if (f.id == CAND_NONE) {                               // the probed lists hold fewer than k rows: pad the rest
            for (int rr = r + t; rr < k; rr += IVF_T) {
                topk_idx[(int64_t)q * k + rr] = -1;
                topk_sim[(int64_t)q * k + rr] = -INFINITY;
                if (topk_pos) topk_pos[(int64_t)q * k + rr] = -1;
            }
            break;
        }
        if (t == 0) {
            topk_idx[(int64_t)q * k + r] = (int32_t)(f.id + idx_offset);
            topk_sim[(int64_t)q * k + r] = f.v;
            if (topk_pos) topk_pos[(int64_t)q * k + r] = f.pay[0];
        }
        const int seg = f.pay[1], i = f.pay[0] - seg_beg[seg];
        if ((i & (IVF_T - 1)) == t) {
            if (use_lds) vals[seg_base[seg] + i] = -INFINITY;
            else mine[(int64_t)seg * pitch + i] = -INFINITY;
        }
    }
}

template <int KB, int BP>
static hipError_t launch_ivf_scan_kb(const IvfScanLaunch& L, const uint16_t* qplanes, int nqt, hipStream_t stream) {
    constexpr int QPITCH = KB * 256 + 16;
    constexpr int NQT_MAX = 4 * 16 * QPITCH <= IVF_LDS_BYTES ? 4 : 2;
    const dim3 grid(L.plan.grid_lists, L.plan.grid_chunks);
    auto go = [&](auto n) {
        constexpr size_t lds = (size_t)n.value * 16 * QPITCH;
        return launch<ivf_scan_kernel<KB, n.value, BP>, lds>(grid, dim3(512), lds, stream, L.bank.p, L.bank.ld, qplanes, L.list_offsets, L.bank.R,
                                                             (const int32_t*)L.pair_offsets, (const int32_t*)L.pair_order, L.nprobe,
                                                             L.max_list_rows, L.plan.pitch, L.scores, L.overflow);
    };
    if constexpr (NQT_MAX == 4) return dispatch<1, 2, 4>(nqt, go);
    else return dispatch<1, 2>(nqt, go);
}

hipError_t launch_ivf_scan(const IvfScanLaunch& L, hipStream_t stream) {
    const IvfScanPlan& P = L.plan;
    const BankRows& B = L.bank;
    if (!P.ok || L.M < 1 || L.k < 1 || L.k > 128 || B.planes < 1 || B.planes > 2 || B.ld % 8 != 0 || B.R < 1)
        return hipErrorInvalidValue;
    hipError_t st = hipMemsetAsync(L.overflow, 0, sizeof(int32_t), stream);
    if (st != hipSuccess) return st;
    for (int m0 = 0; m0 < L.M; m0 += P.chunk) {
        const int m = L.M - m0 < P.chunk ? L.M - m0 : P.chunk;
        const int32_t* probes = L.probes + (int64_t)m0 * L.nprobe;
        // ---- invert: the chunk's (query, probe) pairs grouped by list
        LabelSortLaunch S;
        S.labels = probes; S.R = (int64_t)m * L.nprobe; S.K = L.nlist;
        kmeans_update_plan(S.R, L.nlist, &S.nblocks, &S.rows_per_block);
        S.blk_cnt = L.blk_cnt; S.counts = L.pair_counts; S.offsets = L.pair_offsets; S.order = L.pair_order;
        st = launch_label_sort(S, stream);
        if (st != hipSuccess) return st;
        // ---- scan
        const uint16_t* qplanes = L.qplanes + (int64_t)m0 * 2 * B.D;
        st = dispatch<128, 512, 768>(B.D, [&](auto d) {
            return dispatch<1, 2>(B.planes, [&](auto bp) {
                return launch_ivf_scan_kb<d.value / 64, bp.value>(L, qplanes, P.nqt, stream);
            });
        });
        if (st != hipSuccess) return st;
        // ---- select
        st = launch<ivf_select_kernel, (size_t)IVF_SELECT_LDS_FLOATS * 4>(
            dim3(m), dim3(IVF_T), P.select_lds, stream, L.scores, P.pitch, probes, L.nprobe, L.list_offsets, L.nlist, B.R, L.max_list_rows,
            L.row_ids, L.idx_offset, L.k, P.select_lds ? 1 : 0, L.topk_idx + (int64_t)m0 * L.k, L.topk_sim + (int64_t)m0 * L.k,
            L.topk_pos ? L.topk_pos + (int64_t)m0 * L.k : nullptr);
        if (st != hipSuccess) return st;
    }
    return hipSuccess;
}
