// K5: exact top-k inner-product search of query rows against the reference
// bank, fused with per-row moments.  The [M, R] similarity matrix is never
// written: it lives only in MFMA accumulators.
//
//   pass 0  a strided SAMPLE of the bank (n_sample rows) is multiplied with the
//           query planes by the dense GEMM (fp32 store) and `kth_bound` turns
//           each query's sample row into tau[q] = a LOWER bound of its final
//           k-th best similarity (the k-th largest of 256 disjoint group
//           maxima: k distinct sample elements are >= it).
//   pass 1  `bank_search_kernel`: persistent workgroups own (query tile, bank
//           chunk); per 256x256 tile they run the GEMM main loop (bank rows on
//           the MFMA row dimension, queries on the lane dimension, so every
//           lane filters against its OWN query's tau), accumulate sum / sumsq /
//           max / count in registers and append the few survivors (v > tau) to
//           a per-(chunk, query) list: slot from an LDS counter, no global
//           atomics.
//   pass 2  `bank_select_kernel`: one workgroup (1 024 threads) per query gathers its lists
//           (~0.3-2k entries) into LDS, re-scores them exactly in the fast form and extracts the k
//           best, ordered by (similarity desc, index asc); reduces the moments over chunks.
//
//   small query batches (M <= 64, the reference's own call pattern): pass 1 is `bank_filter_skinny_kernel` (the bank
//           streamed once from HBM into MFMA operand registers) and, over a bf16 bank, pass 0 is
//           `bank_sample_skinny_kernel` + `kth_groups_kernel` (the sample's 256 group maxima straight from the matrix
//           pipe: no [M, n_sample] similarities).
//
//   fast form (no moments requested): pass 1 multiplies ONE product (bank hi x query hi) and
//           filters against tau - margin[q], margin = a Cauchy-Schwarz bound of the dropped
//           products (max bank-row norms x the query's plane norms), so every row whose exact
//           similarity exceeds tau is still listed; pass 2 re-scores the listed rows in fp32
//           (bank hi + lo against the fp32 query) before selecting.  Same result set, half /
//           a third of the MFMA work.
//
// Precision: queries are split into bf16 (hi, lo) planes, so with a bf16 bank
// the products are exact and the result is the fp32-accumulated cosine of the
// stored values (|err| ~ 1e-6); an fp32 bank is split the same way and uses the
// three products hi.hi + lo.hi + hi.lo.
//
// Written once, ahead of the kernels that use them:
//   cand_better / Best<NP> / block_best / block_exclusive_scan
//                                     the (v desc, idx asc) order (common.hpp), the rounds of block arg-max in it (select,
//                                     row_topk) and the block-wide scan (select): select.hpp, shared with kmeans.hip and ivf.hip
//   BankRows                          the stored rows of a slot, as every launch over one takes them (kernels.hpp)
//   Moments / combine / mom_lanes<>   the (sum, sumsq, max, count) 4-tuple and its reductions (search, select, merge)
//   cand_append / cand_count_out      the listing rule of all four filter kernels: slot, cap, overflow flag
//   bank_item / bank_lane_setup       item order and lane set-up of bank_search_kernel<FILTER> and bank_filter_ring_kernel
//   bank_tile_epilogue<FULL, FILTER>  a 256 x 256 tile of similarities -> lists (+ moments)
//   skinny_load_group / skinny_mfma / skinny_walk
//                                     the stream of bank_filter_skinny_kernel and bank_sample_skinny_kernel (skinny.hpp)
#include "gemm_core.hpp"
#include "gemm_ring4.hpp"
#include "skinny.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "select.hpp"
#include <cstdlib>

#define BANK_POOL 6144
#define BANK_MAX_RESCORE_D 2048   // fp32 query row staged in LDS by the re-scoring select
#define BANK_LDS_BYTES (GEMM_LDS_BYTES + 256 * 4 + 2 * 256 * 4 * 4)

struct Cand {
    float v;
    int32_t idx;
};
// (cand_better, the (v desc, idx asc) ordering: common.hpp -- kmeans.hip orders its centres by it too; the rounds of block
// arg-max in that order: select.hpp)

// A query's moments over a set of bank rows, [sum, sum of squares, max, count >= count_thr] as stored in mom_part / moments.
// Every reduction over lanes, waves, chunks and shards is a chain of combine() calls in a fixed order.
struct Moments {
    float sum = 0.f, sq = 0.f, mx = -INFINITY, cnt = 0.f;
};
__device__ __forceinline__ Moments combine(const Moments a, const Moments b) {
    Moments r;
    r.sum = a.sum + b.sum; r.sq = a.sq + b.sq; r.mx = fmaxf(a.mx, b.mx); r.cnt = a.cnt + b.cnt;
    return r;
}
__device__ __forceinline__ Moments mom_load(const float* p) {
    Moments r;
    r.sum = p[0]; r.sq = p[1]; r.mx = p[2]; r.cnt = p[3];
    return r;
}
__device__ __forceinline__ void mom_store(float* p, const Moments m) { p[0] = m.sum; p[1] = m.sq; p[2] = m.mx; p[3] = m.cnt; }
// combine() with the lanes at the xor distances Os, taken in that order, all lanes; written field by field (the sums, then
// the maximum: the order wave_sum / wave_max calls gave) -- distance by distance through combine() is the same arithmetic,
// but hipcc then allocates bank_search_kernel<false>'s tile loop differently (EXPERIMENTS.md)
template <int... Os>
__device__ __forceinline__ Moments mom_lanes(Moments m) {
    ((m.sum += __shfl_xor(m.sum, Os, 64)), ...);
    ((m.sq += __shfl_xor(m.sq, Os, 64)), ...);
    ((m.cnt += __shfl_xor(m.cnt, Os, 64)), ...);
    ((m.mx = fmaxf(m.mx, __shfl_xor(m.mx, Os, 64))), ...);
    return m;
}

// (bank_plan: host_plan.hpp)

// tau[q] = (k-th largest of 256 group maxima of the query's sample similarities) minus a safety margin
// FILTER form: tau is lowered by the bound of what the one-product pass leaves out,
//   |b.q - bhi.qhi| <= |bhi||qlo| + |blo||qhi| + |blo||qlo|   (bank_bounds = max |bhi|, max |blo|)
// Shared tail of the two tau kernels: thread t < 256 brings group t's maximum `m`; needs blockDim.x >= 256.
__device__ __forceinline__ void kth_finish(float m, int q, int k, float* __restrict__ tau, const uint16_t* __restrict__ qplanes,
                                           int D, const float* __restrict__ bank_bounds, float* gm, float (*nrm)[4]) {
    const int t = threadIdx.x;
    float margin = 0.f;
    if (qplanes) {
        float h2 = 0.f, l2 = 0.f;
        if (t < 256) {
            const uint16_t* qr = qplanes + (int64_t)q * 2 * D;
            for (int c = t; c < D; c += 256) {
                const float h = bf16_bits_to_f32(qr[c]), l = bf16_bits_to_f32(qr[D + c]);
                h2 = fmaf(h, h, h2); l2 = fmaf(l, l, l2);
            }
            h2 = wave_sum(h2); l2 = wave_sum(l2);
            if ((t & 63) == 0) { nrm[0][t >> 6] = h2; nrm[1][t >> 6] = l2; }
        }
        __syncthreads();
        const float qh = sqrtf(nrm[0][0] + nrm[0][1] + nrm[0][2] + nrm[0][3]);
        const float ql = sqrtf(nrm[1][0] + nrm[1][1] + nrm[1][2] + nrm[1][3]);
        const float bh = bank_bounds[0], bl = bank_bounds[1];
        margin = (bh * ql + bl * qh + bl * ql) * 1.001f + 4e-6f * (1.f + bh * qh);
    }
    if (t < 256) gm[t] = m;
    __syncthreads();
    if (t >= 256) return;
    int rank = 0;
    for (int u = 0; u < 256; ++u) {
        const float o = gm[u];
        rank += (o > m) || (o == m && u < t);
    }
    const int keff = k > BANK_KEFF ? k : BANK_KEFF;
    if (rank == keff - 1) {
        float v = m;
        if (v > -INFINITY) v = v - 1e-6f - 1e-6f * fabsf(v) - margin;
        // a NaN / inf margin (NaN or inf bank rows reach bank_bounds) must list every finite row:
        // the lists overflow, tvc_bank_status reports it and the brute-force path takes over
        if (!(v == v)) v = -INFINITY;
        tau[q] = v;
    }
}

// s0 [M, n_sample] (the dense sample GEMM's output) -> tau.  1 024 threads scan the row with 16-byte loads, four in flight
// per thread (one workgroup of 256 threads with scalar loads took 44-51 us per launch whatever M was: 245 dependent
// round trips); thread t's elements belong to group t & 255 -- any partition into 256 disjoint groups gives a valid bound.
__global__ __launch_bounds__(1024) void kth_bound_kernel(const float* __restrict__ s0, int n_sample,
                                                         int k, float* __restrict__ tau,
                                                         const uint16_t* __restrict__ qplanes, int D,
                                                         const float* __restrict__ bank_bounds) {
    __shared__ float gm[256];
    __shared__ float part[3][256];
    __shared__ float nrm[2][4];
    const int q = blockIdx.x, t = threadIdx.x;
    const float* row = s0 + (int64_t)q * n_sample;
    float m = -INFINITY;
    if ((n_sample & 3) == 0) {
        const f32x4_t* row4 = (const f32x4_t*)row;
        const int n4 = n_sample >> 2;
        int i = t;
        for (; i + 3 * 1024 < n4; i += 4 * 1024) {
            const f32x4_t a = row4[i], b = row4[i + 1024], c = row4[i + 2048], d = row4[i + 3072];
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3]))));
            m = fmaxf(m, fmaxf(fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3])), fmaxf(fmaxf(d[0], d[1]), fmaxf(d[2], d[3]))));
        }
        for (; i < n4; i += 1024) {
            const f32x4_t a = row4[i];
            m = fmaxf(m, fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])));
        }
    } else {
        for (int i = t; i < n_sample; i += 1024) m = fmaxf(m, row[i]);
    }
    if (t >= 256) part[(t >> 8) - 1][t & 255] = m;
    __syncthreads();
    if (t < 256) m = fmaxf(fmaxf(m, part[0][t]), fmaxf(part[1][t], part[2][t]));
    kth_finish(m, q, k, tau, qplanes, D, bank_bounds, gm, nrm);
}

// gmax [M, 256] (bank_sample_skinny_kernel's group maxima) -> tau; also clears the search's overflow flag
__global__ __launch_bounds__(256) void kth_groups_kernel(const float* __restrict__ gmax, int k, float* __restrict__ tau,
                                                         const uint16_t* __restrict__ qplanes, int D,
                                                         const float* __restrict__ bank_bounds, int32_t* __restrict__ overflow) {
    __shared__ float gm[256];
    __shared__ float nrm[2][4];
    const int q = blockIdx.x;
    if (q == 0 && threadIdx.x == 0) *overflow = 0;
    kth_finish(gmax[(int64_t)q * 256 + threadIdx.x], q, k, tau, qplanes, D, bank_bounds, gm, nrm);
}

// max over rows of |hi plane| and |lo plane| (squared, as ordered uint bit patterns)
__global__ __launch_bounds__(256) void bank_bounds_kernel(BankRows bank, uint32_t* __restrict__ out_sq) {
    const int lane = threadIdx.x & 63, D = bank.D;
    float mh = 0.f, ml = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < bank.R; r += (int64_t)gridDim.x * 4) {
        const uint16_t* br = bank.p + r * bank.ld;
        float h2 = 0.f, l2 = 0.f;
        for (int c = lane * 8; c < D; c += 512) {
            const u32x4_t h = *(const u32x4_t*)(br + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = Op16<false>::lo(h[e]), b = Op16<false>::hi(h[e]);
                h2 = fmaf(a, a, fmaf(b, b, h2));
            }
            if (bank.planes > 1) {
                const u32x4_t l = *(const u32x4_t*)(br + D + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = Op16<false>::lo(l[e]), b = Op16<false>::hi(l[e]);
                    l2 = fmaf(a, a, fmaf(b, b, l2));
                }
            }
        }
        mh = fmaxf(mh, wave_sum(h2)); ml = fmaxf(ml, wave_sum(l2));
    }
    if (lane == 0) {
        // NaN/inf rows: the uint order puts them on top, the margin becomes inf/NaN, tau = -inf and the
        // filter lists every finite row (-> overflow flag -> brute-force path); never a wrong result
        atomicMax(out_sq, __float_as_uint(mh));
        atomicMax(out_sq + 1, __float_as_uint(ml));
    }
}
__global__ void bank_bounds_finish_kernel(float* b) {
    b[0] = sqrtf(b[0]) * 1.0001f; b[1] = sqrtf(b[1]) * 1.0001f;
}

hipError_t launch_bank_bounds(const BankRows& bank, float* bounds, hipStream_t stream) {
    hipError_t st = hipMemsetAsync(bounds, 0, 8, stream);
    if (st != hipSuccess || bank.R == 0) return st;
    int64_t grid = (bank.R + 3) / 4;
    if (grid > 4096) grid = 4096;
    st = launch<bank_bounds_kernel>(dim3((int)grid), dim3(256), 0, stream, bank, (uint32_t*)bounds);
    if (st != hipSuccess) return st;
    return launch<bank_bounds_finish_kernel>(dim3(1), dim3(1), 0, stream, bounds);
}

struct BankEpilogue {
    const float* tau;      // [M]
    Cand* cand;            // [S, M, cap]
    int32_t* cand_cnt;     // [S, M]
    float* mom_part;       // [S, M, 4]
    int32_t* overflow;
    int64_t R;
    int64_t idx_offset;
    int M;
    float count_thr;
};

// ---- the listing rule of the four filter kernels: one definition each of the append and of the count write-out
// Bank row `row` survived query q0 + ql's filter with value v: append it to the list of (chunk, q0 + ql); ql = the query's
// counter in lds_cnt.  A rare path (a few survivors per lane per bank chunk): the pin keeps its address arithmetic inside
// the caller's branch, not hoisted into registers that stay live across the main loop.  Padded query lanes (q0 + ql >= M)
// carry tau = +inf and never get here; the guard keeps a stray append out of the lists of (chunk + 1, q - M).  Slots past
// the cap are counted, not stored (cand_count_out reports them).
__device__ __forceinline__ void cand_append(const BankEpilogue& e, int* lds_cnt, int chunk, int q0, int ql, float v, int64_t row) {
    asm volatile("" : "+v"(ql));
    if (q0 + ql < e.M) {
        const int slot = atomicAdd(&lds_cnt[ql], 1);
        if (slot < BANK_CAP) {
            Cand c;
            c.v = v;
            c.idx = (int32_t)(row + e.idx_offset);
            e.cand[((int64_t)chunk * e.M + (q0 + ql)) * BANK_CAP + slot] = c;
        }
    }
}
// the list length of (chunk, q < M) from its counter c (read after a barrier); a counter past the cap sets the overflow flag
__device__ __forceinline__ void cand_count_out(const BankEpilogue& e, int chunk, int q, int c) {
    if (c > BANK_CAP) { c = BANK_CAP; atomicOr(e.overflow, 1); }
    e.cand_cnt[(int64_t)chunk * e.M + q] = c;
}

// Order of the (query tile, bank chunk) items inside an XCD (consecutive `lin` = concurrently resident workgroups): blocks
// of 4 query tiles x 8 chunks, so the 32 workgroups of a block keep 4 query tiles (1.6 MB of planes) in the XCD's L2 AND
// read every bank tile four times from L2 for one HBM read (query-tile-slowest order streamed the whole bank once per
// query tile: 30 GB per launch at cfg 2).  Ragged counts fall back to query tile slowest.
__device__ __forceinline__ void bank_item(int nQt, int S, int& qt, int& chunk) {
    const int lin = xcd_contiguous(blockIdx.x, nQt * S);
    if ((nQt & 3) == 0 && (S & 7) == 0) {
        const int blk = lin >> 5, r = lin & 31;
        const int ncg = S >> 3;
        const int qg = blk / ncg, cg = blk - qg * ncg;
        qt = qg * 4 + (r & 3);
        chunk = cg * 8 + (r >> 2);
    } else {
        qt = lin / S; chunk = lin - qt * S;
    }
}

// What a lane of the 256-query-tile kernels knows before its first tile: its item, its place in the 2 x 4 wave grid and
// the item's bank tiles [bt0, bt1) ...
struct BankLane {
    int chunk, j0, lane, wm, wn, bt0, bt1;
};
// ... and the taus of its four queries (+inf for padded query rows: never listed); clears the item's list counters and ends
// with a barrier.  (tau is an array of the kernel's own and the tile epilogue takes the BankLane by value: with tau inside
// the struct, or the struct by reference, hipcc allocates the same kernels differently -- EXPERIMENTS.md.)
__device__ __forceinline__ BankLane bank_lane_setup(const BankEpilogue& e, int nQt, int S, int tiles_per_chunk, int n_bank_tiles,
                                                    int* lds_cnt, float (&tau)[4]) {
    BankLane L;
    int qt;
    bank_item(nQt, S, qt, L.chunk);
    L.j0 = qt * GEMM_BN;
    L.lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    L.wm = wave >> 2; L.wn = wave & 3;
    if (threadIdx.x < 256) lds_cnt[threadIdx.x] = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int q = L.j0 + L.wn * 64 + n * 16 + (L.lane & 15);
        tau[n] = (q < e.M) ? e.tau[q] : INFINITY;
    }
    __syncthreads();
    L.bt0 = L.chunk * tiles_per_chunk;
    L.bt1 = L.bt0 + tiles_per_chunk;
    if (L.bt1 > n_bank_tiles) L.bt1 = n_bank_tiles;
    return L;
}

// One 256 x 256 tile of similarities: survivors to the lists; !FILTER: also into the lane's moments mom[4] (FILTER: unused, may be null)
template <bool FULL, bool FILTER>
__device__ __forceinline__ void bank_tile_epilogue(const gemm_acc_t& acc, const BankEpilogue& e, int64_t tile_row0, const BankLane L,
                                                   const float (&tau)[4], Moments* mom, int* lds_cnt) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int ql = L.wn * 64 + n * 16 + (L.lane & 15);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int64_t row = tile_row0 + L.wm * 128 + m * 16 + (L.lane >> 4) * 4;
            f32x4_t v = acc[m][n];
            if (!FULL) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (row + r >= e.R) v[r] = -INFINITY;
            }
            const float m4 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            if (!FILTER) {
                if (FULL) {
                    mom[n].sum += (v[0] + v[1]) + (v[2] + v[3]);
                    mom[n].sq = fmaf(v[0], v[0], fmaf(v[1], v[1], fmaf(v[2], v[2], fmaf(v[3], v[3], mom[n].sq))));
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row + r < e.R) { mom[n].sum += v[r]; mom[n].sq = fmaf(v[r], v[r], mom[n].sq); }
                }
                mom[n].mx = fmaxf(mom[n].mx, m4);
                if (m4 >= e.count_thr) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) mom[n].cnt += (v[r] >= e.count_thr) ? 1.f : 0.f;
                }
            }
            // NaN similarities (zero-norm query row, NaN bank row) are never listed: every comparison
            // with a NaN is false, and fmaxf drops NaN operands; tau itself is never NaN (kth_bound_kernel)
            if (m4 > tau[n]) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (v[r] > tau[n] && (FULL || row + r < e.R)) cand_append(e, lds_cnt, L.chunk, L.j0, ql, v[r], row + r);
            }
        }
    }
}
template <bool FILTER>
__global__ __launch_bounds__(GEMM_THREADS) void bank_search_kernel(GemmOperands g, BankEpilogue e,
                                                                   int nQt, int S, int tiles_per_chunk,
                                                                   int n_bank_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* lds_cnt = (int*)(smem + GEMM_LDS_BYTES);
    float* lds_mom = (float*)(smem + GEMM_LDS_BYTES + 256 * 4);
    float tau[4];
    const BankLane L = bank_lane_setup(e, nQt, S, tiles_per_chunk, n_bank_tiles, lds_cnt, tau);
    Moments mom_regs[4];
    Moments* const mom = FILTER ? nullptr : mom_regs;      // the filter form carries no moments
    for (int bt = L.bt0; bt < L.bt1; ++bt) {
        gemm_acc_t acc;
        gemm_zero_acc(acc);
        const int64_t tile_row0 = (int64_t)bt * GEMM_BM;
        gemm_mainloop(acc, g, (int)tile_row0, L.j0, smem);
        if (tile_row0 + GEMM_BM <= e.R)
            bank_tile_epilogue<true, FILTER>(acc, e, tile_row0, L, tau, mom, lds_cnt);
        else
            bank_tile_epilogue<false, FILTER>(acc, e, tile_row0, L, tau, mom, lds_cnt);
    }

    if (!FILTER) {
        // moments: the 4 lane groups of a wave and the 2 wm-waves share a query
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const Moments m = mom_lanes<16, 32>(mom[n]);
            if ((L.lane >> 4) == 0) mom_store(lds_mom + ((L.wm * 256) + L.wn * 64 + n * 16 + (L.lane & 15)) * 4, m);
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        const int q = L.j0 + threadIdx.x;
        if (q < e.M) {
            if (!FILTER)
                mom_store(e.mom_part + ((int64_t)L.chunk * e.M + q) * 4,
                          combine(mom_load(lds_mom + threadIdx.x * 4), mom_load(lds_mom + (256 + threadIdx.x) * 4)));
            cand_count_out(e, L.chunk, q, lds_cnt[threadIdx.x]);
        }
    }
}

// The filter pass on GEMM form 4 (gemm_ring4.hpp): the workgroup's bank tiles are ONE stream through the LDS-DMA ring --
// counted waits, barrier-staggered ping-pong of the two wave groups, the next tile's K-tiles loading while this tile is
// filtered -- instead of gemm_mainloop's drain-and-barrier per K-tile.  Both operands of this product come out of the L2
// (a query tile is resident, a bank tile is read by four workgroups for one HBM read), where the CU's request path
// delivers 2-3 x what it does for first-touch rows, so the loop is bound by the matrix pipe.  Same products, summed in
// the same order: the listed candidates are identical.  Preconditions (launch_bank_search): the query planes are
// readable up to the next multiple of 256 rows, row pitches are multiples of 128 bytes; the stream takes the FULL bank
// tiles, a ragged last tile goes through gemm_mainloop as before.
__global__ __launch_bounds__(GEMM_THREADS) void bank_filter_ring_kernel(GemmOperands g, BankEpilogue e, int nQt, int S,
                                                                        int tiles_per_chunk, int n_bank_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* lds_cnt = (int*)(smem + GEMM_LDS_BYTES);
    float tau[4];
    const BankLane L = bank_lane_setup(e, nQt, S, tiles_per_chunk, n_bank_tiles, lds_cnt, tau);
    const int n_full = (int)(e.R / GEMM_BM);
    const int bt_ring_end = L.bt1 < n_full ? L.bt1 : n_full;
    ring4_stream(
        g, smem, bt_ring_end - L.bt0,
        [&](int n, int& i0, int& jj0) __attribute__((always_inline)) { i0 = (L.bt0 + n) * GEMM_BM; jj0 = L.j0; },
        [&](int n, const gemm_acc_t& acc) __attribute__((always_inline)) {
            bank_tile_epilogue<true, true>(acc, e, (int64_t)(L.bt0 + n) * GEMM_BM, L, tau, nullptr, lds_cnt);
        });
    for (int bt = (bt_ring_end > L.bt0 ? bt_ring_end : L.bt0); bt < L.bt1; ++bt) {      // the ragged last bank tile
        gemm_acc_t acc;
        gemm_zero_acc(acc);
        const int64_t tile_row0 = (int64_t)bt * GEMM_BM;
        gemm_mainloop(acc, g, (int)tile_row0, L.j0, smem);
        bank_tile_epilogue<false, true>(acc, e, tile_row0, L, tau, nullptr, lds_cnt);
    }
    __syncthreads();
    if (threadIdx.x < 256 && L.j0 + threadIdx.x < e.M) cand_count_out(e, L.chunk, L.j0 + threadIdx.x, lds_cnt[threadIdx.x]);
}


// (the skinny stream of bank_filter_skinny_kernel and bank_sample_skinny_kernel below -- skinny_load_group / skinny_mfma /
// skinny_walk: skinny.hpp; ivf.hip streams a list's rows with it too)
// ---------------------------------------------------------------------------------------------------------------
// The filter pass for SMALL query batches (M <= 64: the reference searches ONE query at a time, src/retrieval.py:636-680;
// BASELINE configs[0] has 48 rows) -- the HBM-bound regime of SURVEY.md 8(d).  The 256-query tile of the kernels above
// multiplies 256 query columns whatever M is (R x 256 x D x 2 FLOP: 0.28 ms at R = 1 M even at the matrix peak) and
// re-reads the bank through the L2 5 x; here the bank is streamed ONCE, straight from HBM (non-temporal loads), against
// the queries' hi planes: a workgroup (8 waves, one per CU) owns a contiguous chunk of bank rows.
//   * epilogue: as bank_tile_epilogue<FILTER> -- every lane compares its 4 rows x NQT queries with its queries' tau and
//     appends survivors to the per-(chunk, query) lists (cand_append).  The products are summed
//     in another k order than in the ring kernel (fp32: ~1e-7), which the margin of kth_bound_kernel covers; the select
//     pass re-scores the listed rows exactly, so the top-k set and values are the same.
// ---------------------------------------------------------------------------------------------------------------
template <int KB, int NQT>
__global__ __launch_bounds__(512) void bank_filter_skinny_kernel(const uint16_t* __restrict__ bank, int64_t ldb,
                                                                  const uint16_t* __restrict__ qplanes, BankEpilogue e,
                                                                  int rows_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = KB * 64;
    constexpr int QPITCH = D * 2 + 16;
    int* lds_cnt = (int*)(smem + NQT * 16 * QPITCH);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = blockIdx.x;
    const int r16 = lane & 15, g = lane >> 4;
    // ---- queries' hi planes -> LDS (rows >= M: zeros, tau = +inf below)
    for (int idx = tid; idx < NQT * 16 * (D / 8); idx += 512) {
        const int q = idx / (D / 8), c = idx - q * (D / 8);
        u32x4_t v = u32x4_t{0u, 0u, 0u, 0u};
        if (q < e.M) v = *(const u32x4_t*)(qplanes + (int64_t)q * 2 * D + c * 8);
        *(u32x4_t*)(smem + q * QPITCH + c * 16) = v;
    }
    if (tid < NQT * 16) lds_cnt[tid] = 0;
    float tau[NQT];
#pragma unroll
    for (int n = 0; n < NQT; ++n) {
        const int q = n * 16 + r16;
        tau[n] = (q < e.M) ? e.tau[q] : INFINITY;
    }
    __syncthreads();

    const int64_t row_lo = (int64_t)chunk * rows_per_chunk;
    int64_t row_hi = row_lo + rows_per_chunk;
    if (row_hi > e.R) row_hi = e.R;
    const int n_groups = row_hi > row_lo ? (int)((row_hi - row_lo + 15) >> 4) : 0;
    const char* qbase = smem + r16 * QPITCH + g * 32;

    auto load_group = [&](int grp, u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) {
        int64_t row = row_lo + (int64_t)grp * 16 + r16;
        if (row >= e.R) row = e.R - 1;                        // clamped: masked in the epilogue
        skinny_load_group<KB, true>(bank + row * ldb + g * 16, a);
    };
    auto compute_group = [&](int grp, const u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) {
        f32x4_t acc[NQT];
        skinny_mfma<KB, NQT, 1, false>(a, qbase, acc);
        const int64_t row0 = row_lo + (int64_t)grp * 16 + 4 * g;
#pragma unroll
        for (int n = 0; n < NQT; ++n) {
            const f32x4_t v = acc[n];
            const float m4 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            if (m4 > tau[n]) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (v[r] > tau[n] && row0 + r < row_hi) cand_append(e, lds_cnt, chunk, 0, n * 16 + r16, v[r], row0 + r);
            }
        }
    };
    u32x4_t a0[2 * KB], a1[2 * KB];
    if (wave < n_groups) load_group(wave, a0);
    skinny_walk(wave, n_groups, a0, a1, load_group, compute_group);
    __syncthreads();
    if (tid < NQT * 16 && tid < e.M) cand_count_out(e, chunk, tid, lds_cnt[tid]);
}

template <int KB>
static hipError_t launch_skinny_kb(const uint16_t* bank, int64_t ldb, const uint16_t* qplanes, const BankEpilogue& e, int S,
                                   int rows_per_chunk, hipStream_t stream) {
    const int nqt = (e.M + 15) / 16;
    const size_t lds = (size_t)nqt * 16 * (KB * 128 + 16) + 64 * 4 + 64;
    // every NQT is registered with the LDS of NQT = 4
    constexpr size_t max_lds = 4 * 16 * (KB * 128 + 16) + 64 * 4 + 64;
    return dispatch<1, 2, 3, 4>(nqt, [&](auto n) {
        return launch<bank_filter_skinny_kernel<KB, n.value>, max_lds>(dim3(S), dim3(512), lds, stream, bank, ldb, qplanes, e,
                                                                       rows_per_chunk);
    });
}

// D in {128, 512, 768} (two register sets of D / 64 x 2 sixteen-byte pieces: D = 1024 would spill) and M <= 64; false = shape
// not covered (the caller takes the 256-query-tile kernels)
static bool skinny_covers(int D, int M) { return M >= 1 && M <= 64 && (D == 128 || D == 512 || D == 768); }
static hipError_t launch_bank_filter_skinny(const uint16_t* bank, int64_t ldb, int D, const uint16_t* qplanes, const BankEpilogue& e,
                                            int S, int rows_per_chunk, hipStream_t stream) {
    return dispatch<128, 512, 768>(D, [&](auto d) {
        return launch_skinny_kb<d.value / 64>(bank, ldb, qplanes, e, S, rows_per_chunk, stream);
    });
}

// ---------------------------------------------------------------------------------------------------------------
// Pass 0 for small query batches over a bf16 bank (M <= 64): the sample's 256 group maxima straight from the matrix
// pipe -- no [M, n_sample] similarities, no scan of them.  (The dense sample GEMM ran one 256 x 256 tile per workgroup
// for M query columns, 49 us, and kth_bound_kernel another 46 us: a third of a 1 M-row search's time that is not the
// bank stream.)  Workgroup (G, qb): sample rows [G * per, (G + 1) * per) -- bank rows i * sample_stride -- against
// the 16 * NQT queries of block qb, whose [hi | lo] planes sit in LDS (pitch 4 D + 16 bytes, conflict-free as in the
// filter kernel); both products of a bf16 bank, b.qhi + b.qlo, go into one accumulator (exact bf16 x bf16 products,
// fp32 sums: the value the dense sample GEMM computed, in another k order -- inside kth_finish's slack).
// Lane (r16, g) owns query n * 16 + r16 and the group's rows 4 g .. 4 g + 3: a running maximum per lane, reduced over
// g by two shuffles and over the eight waves through LDS.  Rows past the group's end are clamped for the load and
// masked to -inf (a duplicated row in two groups would break "k distinct sample rows are >= tau").
// ---------------------------------------------------------------------------------------------------------------
template <int KB, int NQT>
__global__ __launch_bounds__(512) void bank_sample_skinny_kernel(const uint16_t* __restrict__ bank, int64_t ldb,
                                                                  const uint16_t* __restrict__ qplanes, int M, int n_sample,
                                                                  int sample_stride, int per, float* __restrict__ gmax) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = KB * 64;
    constexpr int QPITCH = 4 * D + 16;
    float* red = (float*)(smem + NQT * 16 * QPITCH);          // [8][NQT * 16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = blockIdx.x, q0 = blockIdx.y * NQT * 16;
    const int r16 = lane & 15, g = lane >> 4;
    const int i_lo = G * per;
    int i_hi = i_lo + per;
    if (i_hi > n_sample) i_hi = n_sample;
    const int n_groups = i_hi > i_lo ? (i_hi - i_lo + 15) >> 4 : 0;
    const char* qbase = smem + r16 * QPITCH + g * 32;
    float mx[NQT];
#pragma unroll
    for (int n = 0; n < NQT; ++n) mx[n] = -INFINITY;

    auto load_group = [&](int grp, u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) {
        int i = i_lo + grp * 16 + r16;
        if (i >= i_hi) i = i_hi - 1;
        skinny_load_group<KB, false>(bank + (int64_t)i * sample_stride * ldb + g * 16, a);
    };
    auto compute_group = [&](int grp, const u32x4_t (&a)[2 * KB]) __attribute__((always_inline)) {
        f32x4_t acc[NQT];
        // the fence keeps hipcc from hoisting every fragment read of the group (154 spills)
        skinny_mfma<KB, NQT, 2, true>(a, qbase, acc);
        const int i0 = i_lo + grp * 16 + 4 * g;
#pragma unroll
        for (int n = 0; n < NQT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i0 + r < i_hi) mx[n] = fmaxf(mx[n], acc[n][r]);
    };
    // a wave has two or three groups (n_sample / 256 rows per workgroup), both requested up front -- and the first before
    // the queries' planes are copied to LDS (NQT * 16 * D / 4 sixteen-byte pieces, 3 per thread and query at D = 768,
    // unrolled so that a thread's pieces are in flight together): the launch is latency-bound, the two latencies overlap
    u32x4_t a0[2 * KB], a1[2 * KB];
    if (wave < n_groups) load_group(wave, a0);
    {
        constexpr int PIECES = NQT * 16 * (D / 4);
        constexpr int ROUNDS = (PIECES + 511) / 512;
#pragma unroll 6
        for (int u = 0; u < ROUNDS; ++u) {
            const int idx = tid + u * 512;
            const int q = idx / (D / 4), c = idx - q * (D / 4);
            u32x4_t v = u32x4_t{0u, 0u, 0u, 0u};
            if (idx < PIECES && q0 + q < M) v = *(const u32x4_t*)(qplanes + (int64_t)(q0 + q) * 2 * D + c * 8);
            if (idx < PIECES) *(u32x4_t*)(smem + q * QPITCH + c * 16) = v;
        }
    }
    __syncthreads();
    skinny_walk(wave, n_groups, a0, a1, load_group, compute_group);
#pragma unroll
    for (int n = 0; n < NQT; ++n) {
        float v = mx[n];
        v = fmaxf(v, __shfl_xor(v, 16, 64));
        v = fmaxf(v, __shfl_xor(v, 32, 64));
        if (g == 0) red[wave * (NQT * 16) + n * 16 + r16] = v;
    }
    __syncthreads();
    if (tid < NQT * 16 && q0 + tid < M) {
        float v = red[tid];
#pragma unroll
        for (int w = 1; w < 8; ++w) v = fmaxf(v, red[w * (NQT * 16) + tid]);
        gmax[(int64_t)(q0 + tid) * 256 + G] = v;
    }
}

// 16 * NQT queries per workgroup, NQT <= 3: both planes of 48 queries are 146 KB of LDS at D = 768 (64 queries: two blocks of 32)
template <int KB>
static hipError_t launch_sample_skinny_kb(const uint16_t* bank, int64_t ldb, const uint16_t* qplanes, int M, int n_sample,
                                          int sample_stride, float* gmax, hipStream_t stream) {
    const int nqt = M <= 16 ? 1 : (M > 32 && M <= 48) ? 3 : 2;
    const int per = (n_sample + 255) / 256;
    const dim3 grid(256, (M + nqt * 16 - 1) / (nqt * 16));
    const size_t lds = (size_t)nqt * 16 * (KB * 256 + 16) + 8 * nqt * 16 * 4;
    return dispatch<1, 2, 3>(nqt, [&](auto n) {
        constexpr size_t max_lds = n.value * 16 * (KB * 256 + 16) + 8 * n.value * 16 * 4;
        return launch<bank_sample_skinny_kernel<KB, n.value>, max_lds>(grid, dim3(512), lds, stream, bank, ldb, qplanes, M, n_sample,
                                                                       sample_stride, per, gmax);
    });
}
static hipError_t launch_bank_sample_skinny(const uint16_t* bank, int64_t ldb, int D, const uint16_t* qplanes, int M, int n_sample,
                                            int sample_stride, float* gmax, hipStream_t stream) {
    return dispatch<128, 512, 768>(D, [&](auto d) {
        return launch_sample_skinny_kb<d.value / 64>(bank, ldb, qplanes, M, n_sample, sample_stride, gmax, stream);
    });
}

// One workgroup of SEL_T threads per query.  Round 4: 1 024 threads (16 waves x 4 rows in flight in the re-scoring: the
// ~250-350 listed rows of a query took 16-22 round trips of ~2 us with 4 waves, a fifth of a small search), and the list
// gather reads a thread's chunk counts in one batch of independent loads instead of one dependent load per chunk.
#define SEL_T 1024
#define SEL_W (SEL_T / 64)
#define SEL_CPT 8          // chunks per thread kept in registers (S <= SEL_T * SEL_CPT; more: the counts are read twice)
__global__ __launch_bounds__(SEL_T) void bank_select_kernel(const Cand* __restrict__ cand,
                                                            const int32_t* __restrict__ cand_cnt,
                                                            const float* __restrict__ mom_part, int S, int M,
                                                            int k, int32_t* __restrict__ topk_idx,
                                                            float* __restrict__ topk_sim,
                                                            float* __restrict__ moments,
                                                            int32_t* __restrict__ overflow, BankRows rs,      // re-scoring: the bank (rs.p null: none)
                                                            const float* __restrict__ rs_rows,
                                                            int64_t idx_offset) {
    __shared__ Cand pool[BANK_POOL];
    __shared__ __attribute__((aligned(16))) float qs[BANK_MAX_RESCORE_D];
    __shared__ int wsum[SEL_W];
    __shared__ BestSlots<SEL_T, 1> red;      // payload: the pool slot
    __shared__ float mom_red[SEL_W][4];
    const int q = blockIdx.x, t = threadIdx.x, D = rs.D;
    const int lane = t & 63, wave = t >> 6;

    // chunks handled by this thread: c = t, t + SEL_T, ...
    const bool few = S <= SEL_T * SEL_CPT;
    int cnt[SEL_CPT];
    int mine = 0;
    if (few) {
#pragma unroll
        for (int u = 0; u < SEL_CPT; ++u) {
            const int c = t + u * SEL_T;
            cnt[u] = c < S ? cand_cnt[(int64_t)c * M + q] : 0;
        }
#pragma unroll
        for (int u = 0; u < SEL_CPT; ++u) mine += cnt[u];
    } else {
        for (int c = t; c < S; c += SEL_T) mine += cand_cnt[(int64_t)c * M + q];
    }
    int total_all;
    int off = block_exclusive_scan<SEL_T>(mine, wsum, total_all);
    if (few) {
#pragma unroll
        for (int u = 0; u < SEL_CPT; ++u) {
            const int n = cnt[u];
            if (n > 0) {
                const Cand* src = cand + ((int64_t)(t + u * SEL_T) * M + q) * BANK_CAP;
                for (int i = 0; i < n; ++i) {
                    if (off < BANK_POOL) pool[off] = src[i];
                    ++off;
                }
            }
        }
    } else {
        for (int c = t; c < S; c += SEL_T) {
            const int n = cand_cnt[(int64_t)c * M + q];
            const Cand* src = cand + ((int64_t)c * M + q) * BANK_CAP;
            for (int i = 0; i < n; ++i) {
                if (off < BANK_POOL) pool[off] = src[i];
                ++off;
            }
        }
    }
    if (t == 0 && total_all > BANK_POOL) atomicOr(overflow, 2);
    const int total = total_all < BANK_POOL ? total_all : BANK_POOL;
    if (rs.p) {
        for (int c = t; c < D; c += SEL_T) qs[c] = rs_rows[(int64_t)q * D + c];
    }
    __syncthreads();

    if (rs.p) {
        // exact fp32 re-scoring of the listed rows: one wave per row, four rows in flight per wave
        for (int i0 = wave; i0 < total; i0 += 4 * SEL_W) {
            float part[4];
            const uint16_t* br[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int i = i0 + u * SEL_W;
                i = i < total ? i : total - 1;
                br[u] = rs.p + ((int64_t)pool[i].idx - idx_offset) * rs.ld;
                part[u] = 0.f;
            }
            for (int c = lane * 8; c < D; c += 512) {
                // (not bank_row8: its zero lo plane costs this loop registers -- EXPERIMENTS.md)
                u32x4_t h[4], l[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    h[u] = *(const u32x4_t*)(br[u] + c);
                    if (rs.planes > 1) l[u] = *(const u32x4_t*)(br[u] + D + c);
                }
                const f32x4_t q0 = *(const f32x4_t*)(qs + c), q1 = *(const f32x4_t*)(qs + c + 4);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int e2 = 0; e2 < 4; ++e2) {
                        float a = Op16<false>::lo(h[u][e2]), b = Op16<false>::hi(h[u][e2]);
                        if (rs.planes > 1) {
                            a += Op16<false>::lo(l[u][e2]);
                            b += Op16<false>::hi(l[u][e2]);
                        }
                        const float qa = e2 < 2 ? q0[e2 * 2] : q1[e2 * 2 - 4];
                        const float qb = e2 < 2 ? q0[e2 * 2 + 1] : q1[e2 * 2 - 3];
                        part[u] = fmaf(a, qa, fmaf(b, qb, part[u]));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float v = wave_sum(part[u]);
                const int i = i0 + u * SEL_W;
                if (lane == 0 && i < total) pool[i].v = v;
            }
        }
        __syncthreads();
    }

    // k rounds of arg-max (select.hpp); a pool entry is admitted while its idx >= 0: a similarity of -inf can win, a NaN never.
    // The winner's pool slot, not its id (any int32), says whether there was one; the slot's owner (slot % SEL_T) strikes it
    for (int r = 0; r < k; ++r) {
        Best<1> b;
        b.pay[0] = -1;
        for (int i = t; i < total; i += SEL_T) {
            const Cand c = pool[i];
            if (c.idx >= 0) best_take(b, Best<1>{c.v, c.idx, {i}});
        }
        const Best<1> f = block_best(b, red, r);
        const int fp = f.pay[0];
        if (t == 0) {
            topk_idx[(int64_t)q * k + r] = fp >= 0 ? f.id : -1;
            topk_sim[(int64_t)q * k + r] = fp >= 0 ? f.v : -INFINITY;
        }
        if (fp >= 0 && (fp & (SEL_T - 1)) == t) pool[fp].idx = -1;     // taken
    }

    if (moments) {
        Moments m;
        for (int ch = t; ch < S; ch += SEL_T) m = combine(m, mom_load(mom_part + ((int64_t)ch * M + q) * 4));
        m = mom_lanes<32, 16, 8, 4, 2, 1>(m);
        if (lane == 0) mom_store(mom_red[wave], m);
        __syncthreads();
        if (t == 0) {
            Moments o;
            for (int w = 0; w < SEL_W; ++w) o = combine(o, mom_load(mom_red[w]));
            mom_store(moments + (int64_t)q * 4, o);
        }
    }
}

// ---------------------------------------------------------------------------
// Dense fallback for degenerate banks (candidate lists overflowed): the similarities of a
// block of query rows are materialised ([m, R] fp32, m <= 64) by the dense GEMM and every row
// is reduced by k rounds of block arg-max.  Slow (R reads per round) but unconditional.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void row_topk_kernel(float* __restrict__ sims, int64_t R, int k,
                                                        float count_thr, int64_t idx_offset,
                                                        int32_t* __restrict__ topk_idx,
                                                        float* __restrict__ topk_sim,
                                                        float* __restrict__ moments) {
    __shared__ BestSlots<1024, 0> red;
    __shared__ float rs[16], rq[16], rc[16];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float* row = sims + (int64_t)q * R;
    if (moments) {
        // three sums, not a Moments: the maximum is the first arg-max round's
        float s = 0.f, s2 = 0.f, c = 0.f;
        for (int64_t i = t; i < R; i += 1024) { const float v = row[i]; s += v; s2 = fmaf(v, v, s2); c += (v >= count_thr) ? 1.f : 0.f; }
        s = wave_sum(s); s2 = wave_sum(s2); c = wave_sum(c);
        if (lane == 0) { rs[wave] = s; rq[wave] = s2; rc[wave] = c; }
        __syncthreads();
        if (t == 0) {
            float a = 0.f, b = 0.f, d = 0.f;
            for (int w = 0; w < 16; ++w) { a += rs[w]; b += rq[w]; d += rc[w]; }
            moments[(int64_t)q * 4 + 0] = a; moments[(int64_t)q * 4 + 1] = b; moments[(int64_t)q * 4 + 3] = d;
        }
    }
    // k rounds of arg-max (select.hpp); thread i & 1023 owns element i; a round without a candidate writes -1 / -inf
    for (int r = 0; r < k; ++r) {
        Best<0> b;
        for (int64_t i = t; i < R; i += 1024) {
            const float v = row[i];
            // NaN similarities (NaN bank rows / zero-norm queries), -inf and struck entries are never returned
            if (v > -INFINITY) best_take(b, Best<0>{v, (int)i});
        }
        const Best<0> f = block_best(b, red, r);
        const bool none = f.id == CAND_NONE;
        if (t == 0) {
            topk_idx[(int64_t)q * k + r] = none ? -1 : (int32_t)(f.id + idx_offset);
            topk_sim[(int64_t)q * k + r] = f.v;                  // -inf when none
            if (r == 0 && moments) moments[(int64_t)q * 4 + 2] = f.v;
        }
        if (!none && (f.id & 1023) == t) row[f.id] = -INFINITY;      // taken
    }
}

hipError_t launch_bank_search_dense(const BankSearchLaunch& L, float* sims_ws, int block_rows, hipStream_t stream) {
    const int D = L.bank.D;
    for (int m0 = 0; m0 < L.M; m0 += block_rows) {
        const int m = (L.M - m0 < block_rows) ? L.M - m0 : block_rows;
        const GemmLaunch G = gemm_launch_planes(L.bank.p, L.bank.ld, (int)L.bank.R, L.bank.planes, L.qplanes + (int64_t)m0 * 2 * D, m, D,
                                                sims_ws, L.bank.R);
        hipError_t st = launch_gemm_bf16(G, stream);
        if (st != hipSuccess) return st;
        st = launch<row_topk_kernel>(dim3(m), dim3(1024), 0, stream, sims_ws, L.bank.R, L.k, L.count_thr, L.idx_offset,
                                     L.topk_idx + (int64_t)m0 * L.k, L.topk_sim + (int64_t)m0 * L.k,
                                     L.moments ? L.moments + (int64_t)m0 * 4 : nullptr);
        if (st != hipSuccess) return st;
    }
    return hipSuccess;
}

// an on / off switch of the A/B runs: on unless the variable is set to 0 (callers read it once per process)
static bool env_flag(const char* name) {
    const char* v = getenv(name);
    return !v || atoi(v) != 0;
}

hipError_t launch_bank_search(const BankSearchLaunch& L, hipStream_t stream) {
    const BankRows& B = L.bank;
    const int D = B.D;
    // products: (bank plane, query plane) pairs accumulated into one tile
    //   bf16 bank : b.qhi + b.qlo
    //   fp32 bank : bhi.qhi + bhi.qlo + blo.qhi
    // fast form: one-product filter + exact re-scoring (needs no per-row moments)
    const bool filter = (L.moments == nullptr) && L.bank_bounds && L.rows && D <= BANK_MAX_RESCORE_D && L.allow_filter;

    // small query batches: the bank streamed once from HBM against <= 64 query columns (TVC_BANK_SKINNY=0: off, for A/B runs)
    static const bool skinny_on = env_flag("TVC_BANK_SKINNY");
    const bool skinny = filter && skinny_on && skinny_covers(D, L.M) && B.ld % 8 == 0;
    // ... and, over a bf16 bank, the sample's group maxima by the same route (TVC_BANK_SKINNY_SAMPLE=0: the dense sample GEMM)
    static const bool skinny_sample_on = env_flag("TVC_BANK_SKINNY_SAMPLE");

    // ---- pass 0: sample GEMM + tau ----------------------------------------
    hipError_t st;
    if (skinny && skinny_sample_on && B.planes == 1) {
        // s0 holds >= M * n_sample floats, n_sample >= 256 or the whole bank: the first [M, 256] of it take the group maxima
        st = launch_bank_sample_skinny(B.p, B.ld, D, L.qplanes, L.M, L.n_sample, L.sample_stride, L.gmax, stream);
        if (st != hipSuccess) return st;
        st = launch<kth_groups_kernel>(dim3(L.M), dim3(256), 0, stream, L.gmax, L.k, L.tau, L.qplanes, D, L.bank_bounds, L.overflow);
        if (st != hipSuccess) return st;
    } else {
        const GemmLaunch G = gemm_launch_planes(B.p, B.ld * (int64_t)L.sample_stride, L.n_sample, B.planes, L.qplanes, L.M, D,
                                                L.s0, L.n_sample);
        st = launch_gemm_bf16(G, stream);
        if (st != hipSuccess) return st;
        st = launch<kth_bound_kernel>(dim3(L.M), dim3(1024), 0, stream, L.s0, L.n_sample, L.k, L.tau, filter ? L.qplanes : nullptr, D,
                                      L.bank_bounds);
        if (st != hipSuccess) return st;
        st = hipMemsetAsync(L.overflow, 0, sizeof(int32_t), stream);
        if (st != hipSuccess) return st;
    }

    // ---- pass 1: fused GEMM + filter ---------------------------------------
    GemmOperands g = gemm_operands(gemm_launch_planes(B.p, B.ld, (int)B.R, B.planes, L.qplanes, L.M, D, nullptr, 0));
    if (filter) g.planes = 1;       // the first product alone: bank hi x query hi
    BankEpilogue e;
    e.tau = L.tau; e.cand = (Cand*)L.cand; e.cand_cnt = L.cand_cnt; e.mom_part = L.mom_part;
    e.overflow = L.overflow; e.R = B.R; e.idx_offset = L.idx_offset; e.M = L.M; e.count_thr = L.count_thr;
    const int nQt = (L.M + GEMM_BN - 1) / GEMM_BN;
    const int nbt = (int)((B.R + GEMM_BM - 1) / GEMM_BM);
    const int tpc = (nbt + L.S - 1) / L.S;
    // the filter pass streams its bank tiles through GEMM form 4 where that form's preconditions hold (TVC_BANK_RING=0:
    // the one-tile-at-a-time loop, for A/B runs); the ragged last bank tile is handled inside the kernel
    static const bool ring_on = env_flag("TVC_BANK_RING");
    const bool ring = filter && ring_on && L.q_rows_padded && (g.lda % 64 == 0) && (g.ldb % 64 == 0) && B.R >= GEMM_BM;
    const dim3 grid(nQt * L.S), block(GEMM_THREADS);
    if (skinny)
        st = launch_bank_filter_skinny(B.p, B.ld, D, L.qplanes, e, L.S, tpc * GEMM_BM, stream);
    else if (ring)
        st = launch<bank_filter_ring_kernel, BANK_LDS_BYTES>(grid, block, BANK_LDS_BYTES, stream, g, e, nQt, L.S, tpc, nbt);
    else
        st = dispatch<false, true>(filter, [&](auto f) {
            return launch<bank_search_kernel<f.value>, BANK_LDS_BYTES>(grid, block, BANK_LDS_BYTES, stream, g, e, nQt, L.S, tpc, nbt);
        });
    if (st != hipSuccess) return st;

    // ---- pass 2: select -----------------------------------------------------
    BankRows rs = B;
    if (!filter) rs.p = nullptr;
    return launch<bank_select_kernel>(dim3(L.M), dim3(SEL_T), 0, stream, (const Cand*)L.cand, L.cand_cnt, L.mom_part, L.S, L.M, L.k,
                                      L.topk_idx, L.topk_sim, L.moments, L.overflow, rs, L.rows, L.idx_offset);
}

// ---------------------------------------------------------------------------
// merge of W per-shard partial top-k lists (bank sharded over GPUs)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_merge_kernel(const int32_t* __restrict__ idx_parts,
                                                         const float* __restrict__ sim_parts,
                                                         const float* __restrict__ feat_parts,
                                                         const float* __restrict__ mom_parts, int W,
                                                         int M, int k, int kf, int D,
                                                         int32_t* __restrict__ idx_out,
                                                         float* __restrict__ sim_out,
                                                         float* __restrict__ feat_out,
                                                         float* __restrict__ mom_out) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ int src_of_rank[32];
    const int q = blockIdx.x, t = threadIdx.x;
    const int n = W * k;   // <= 256
    float v = -INFINITY;
    int id = -1;
    if (t < n) {
        const int w = t / k, j = t - w * k;
        id = idx_parts[((int64_t)w * M + q) * k + j];
        v = (id >= 0) ? sim_parts[((int64_t)w * M + q) * k + j] : -INFINITY;
    }
    sv[t] = v; si[t] = id;
    if (t < 32) src_of_rank[t] = -1;
    __syncthreads();
    if (t < n) {
        int rank = 0;
        for (int u = 0; u < n; ++u) {
            if (u == t) continue;
            const float ov = sv[u]; const int oi = si[u];
            // entries with idx < 0 sort last; among valid: (v desc, idx asc); stable by position
            bool before;
            if (oi < 0) before = false;
            else if (id < 0) before = true;
            else before = (ov > v) || (ov == v && (oi < id || (oi == id && u < t)));
            rank += before ? 1 : 0;
        }
        if (id < 0) {
            // padded entries: count how many padded entries precede (keep ranks unique)
            int valid = 0, pad_before = 0;
            for (int u = 0; u < n; ++u) { valid += (si[u] >= 0); pad_before += (si[u] < 0 && u < t); }
            rank = valid + pad_before;
        }
        if (rank < k) {
            idx_out[(int64_t)q * k + rank] = id;
            sim_out[(int64_t)q * k + rank] = v;
            if (rank < kf) src_of_rank[rank] = t;
        }
    }
    __syncthreads();
    if (feat_out && feat_parts) {
        for (int r = 0; r < kf; ++r) {
            const int s = src_of_rank[r];
            float* o = feat_out + ((int64_t)q * kf + r) * D;
            if (s < 0 || si[s] < 0) {
                for (int c = t; c < D; c += 256) o[c] = 0.f;
            } else {
                const int w = s / k, j = s - w * k;
                // a global rank < kf implies a shard-local rank < kf
                const float* f = feat_parts + (((int64_t)w * M + q) * kf + (j < kf ? j : kf - 1)) * D;
                for (int c = t; c < D; c += 256) o[c] = f[c];
            }
        }
    }
    if (mom_out && mom_parts && t == 0) {
        Moments m;
        for (int w = 0; w < W; ++w) m = combine(m, mom_load(mom_parts + ((int64_t)w * M + q) * 4));
        mom_store(mom_out + (int64_t)q * 4, m);
    }
}

hipError_t launch_topk_merge(const int32_t* idx_parts, const float* sim_parts, const float* feat_parts,
                             const float* mom_parts, int W, int M, int k, int kf, int D,
                             int32_t* idx_out, float* sim_out, float* feat_out, float* mom_out,
                             hipStream_t stream) {
    if (M == 0) return hipSuccess;
    if (W < 1 || k < 1 || k > 128 || W * k > 256 || kf < 0 || kf > k || kf > 32) return hipErrorInvalidValue;
    return launch<topk_merge_kernel>(dim3(M), dim3(256), 0, stream, idx_parts, sim_parts, feat_parts, mom_parts, W, M, k, kf, D,
                                     idx_out, sim_out, feat_out, mom_out);
}
