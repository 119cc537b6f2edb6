// The "swapped" MFMA idiom of the attention kernels, defined once (device only).
//
// Both products keep the reduction-free index (the query; the key in the dK / dV pass) on the lane:
//   S^T[key, q] = K . Q^T     A = 16 rows of the K image (ds_read_b128), B = a Q fragment, lane (g, r16) = (lane >> 4, lane & 15)
//                             holds S^T[16 t + 4 g + r, q = r16] in accumulator element r
//   O^T[dh, q]  = V^T . P^T   A = V^T by ds_read_b64_tr_b16 of the row-major V image, B = P^T packed from the S^T accumulators
//                             of two key tiles with no lane movement (k-slots j < 4: tile t0's keys 4 g + j, j >= 4: tile t1's)
// so a row's softmax statistics are per-lane scalars, completed over the four 16-lane groups, and a lane's output is four
// consecutive head dims per 16-wide tile.  Users: attention.hip, attention_bwd.hip (both passes), split.hip's attention and
// sd_attention.hip.  What is tuned per kernel -- loop shapes, fences, wait placement, prefetch depth -- stays in the kernels.
#pragma once
#include "common.hpp"

#define ATT_DH 64        // head dim of the tower kernels
#define ATT_KROW 128     // image read along rows only: 64 x 16 bit per row, 16-byte chunks XOR-swizzled (swz_chunk)
#define ATT_VROW 160     // image read transposed (and along rows): + 32 B pad, conflict-free for both read kinds
#define ATT_SCALE_LOG2 (0.125f * 1.4426950408889634f)      // dh^-0.5 * log2(e)

// IEEE-754-2019 maximum (NaN-propagating): hipcc emits v_maximum3_f32 with no canonicalising copy of the MFMA outputs
__device__ __forceinline__ float mx3(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// A fragment of ones: one more "V^T tile" that leaves sum_k P[k, q] in every accumulator row
template <bool F16>
__device__ __forceinline__ typename Op16<F16>::x8 ones8() {
    constexpr uint32_t one2 = Op16<F16>::ONE2;
    return __builtin_bit_cast(typename Op16<F16>::x8, u32x4_t{one2, one2, one2, one2});
}
// Transposed read: lane i of a 16-lane group supplies row 4 g + (i >> 2), columns 4 (i & 3) .. + 3 of a [16 rows][16 dh] block
template <int PITCH>
__device__ __forceinline__ int tr_lane_off(int g, int r16) { return (4 * g + (r16 >> 2)) * PITCH + ((r16 & 3) << 3); }
// Byte offset of 16-byte chunk c in row `row` (or any value equal to it mod 16: the lane index for the row 16 t + r16) of an
// ATT_KROW image: conflict-free ds_read_b128 of (row = r16, chunk = 4 s + g).
// A macro: behind a function call hipcc no longer sees that a fill loop's rows, 16 apart, share the offset (EXPERIMENTS.md).
#define swz_chunk(c, row) (((c) ^ (((row) >> 1) & 7)) << 4)
// Where a lane stores its first swap_pack16 piece (the second: + 32 elements); dh0 = the row's head dim 0
__device__ __forceinline__ uint16_t* swap_store_ptr(uint16_t* dh0, int g) { return dh0 + (g & 1) * 16 + (g >> 1) * 8; }
// Two transposed 8-byte LDS reads -> one A fragment of 8: k-slots j < 4 from p0 (tile t0), j >= 4 from p1 (tile t1); p = image
// + tr_lane_off + 32 md + 16 t pitch.  The instruction moves 16-bit words whatever they encode, so both formats read through
// the bf16-typed builtin.
// tr16_read + join8 are its two halves: split.hip issues the four reads of its two planes before it joins them.
__device__ __forceinline__ bf16x4_t tr16_read(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)p);
}
template <bool F16>
__device__ __forceinline__ typename Op16<F16>::x8 join8(const bf16x4_t v0, const bf16x4_t v1) {
    bf16x8_t a;
    a[0] = v0[0]; a[1] = v0[1]; a[2] = v0[2]; a[3] = v0[3];
    a[4] = v1[0]; a[5] = v1[1]; a[6] = v1[2]; a[7] = v1[3];
    return __builtin_bit_cast(typename Op16<F16>::x8, a);
}
template <bool F16>
__device__ __forceinline__ typename Op16<F16>::x8 tr16_frag(const char* p0, const char* p1) { return join8<F16>(tr16_read(p0), tr16_read(p1)); }
// The accumulators of two key tiles -> one B fragment of 8 (the k-slot order of tr16_frag)
template <bool F16>
__device__ __forceinline__ typename Op16<F16>::x8 pack8(const f32x4_t p0, const f32x4_t p1) {
    u32x4_t pk;
    pk[0] = Op16<F16>::pack2(p0[0], p0[1]);
    pk[1] = Op16<F16>::pack2(p0[2], p0[3]);
    pk[2] = Op16<F16>::pack2(p1[0], p1[1]);
    pk[3] = Op16<F16>::pack2(p1[2], p1[3]);
    return __builtin_bit_cast(typename Op16<F16>::x8, pk);
}
// Two neighbouring output tiles md, md + 1 (already scaled) -> one 16-byte store piece.  A lane's 4 features per 16-wide tile
// are 8 B; swapping 16-lane rows between the two tiles (v_permlane16_swap, as the GEMM's bf16 epilogue does) leaves every lane
// with 8 consecutive features from swap_store_ptr on: 64 contiguous bytes per row and instruction.  The partner lanes carry the
// same column, so the swap sits outside the caller's store mask.
template <bool F16>
__device__ __forceinline__ u32x4_t swap_pack16(const f32x4_t v0, const f32x4_t v1) {
    const auto r0 = __builtin_amdgcn_permlane16_swap(Op16<F16>::pack2(v0[0], v0[1]), Op16<F16>::pack2(v1[0], v1[1]), false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(Op16<F16>::pack2(v0[2], v0[3]), Op16<F16>::pack2(v1[2], v1[3]), false, false);
    return u32x4_t{r0[0], r1[0], r0[1], r1[1]};
}
// ---- a column's statistic over the four 16-lane groups
__device__ __forceinline__ float group_max4(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64)); }
__device__ __forceinline__ float group_sum4(float v) { v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64); }
// Masking costs nothing after the MFMA: the accumulator is INITIALISED with 0 or -inf (-inf + q.k = -inf).  The initialiser of
// key `key` (16 t + 4 g + r in accumulator element r) of T keys in all: only the last tile holds keys >= T.
__device__ __forceinline__ float key_penalty(int key, int T) { return key >= T ? -INFINITY : 0.f; }
// ---- one sequence of the tower kernels, wave-uniform (SGPRs: the per-tile guards stay scalar branches).
// starts == nullptr: sequence `seq` owns rows [seq * T_fixed, + T_fixed); otherwise rows [starts[seq], starts[seq + 1]).
// CAUSAL with pfx (int32 [2 * n_seq]): the keys are P = pfx[seq] shared-prefix rows from packed row pfx[n_seq + seq] on, then
// the own rows; the queries are the own rows only (positions P .. T - 1).  The pointers come by reference: tested by value, a
// kernel argument's null check takes another form than the kernel's own and is made twice.
template <bool CAUSAL>
struct SeqView {
    int64_t row0;          // first of the sequence's own rows
    int64_t prow0 = 0;
    int T;                 // keys: prefix + own rows, at most max_T (the host guarantees it; never index past the LDS region)
    int P = 0;
    __device__ __forceinline__ SeqView(const int32_t* __restrict__ const& starts, const int32_t* __restrict__ const& pfx, int T_fixed,
                                       int seq, int n_seq, int max_T) {
        if (starts) {
            const int s0 = __builtin_amdgcn_readfirstlane(starts[seq]);
            const int s1 = __builtin_amdgcn_readfirstlane(starts[seq + 1]);
            row0 = s0; T = s1 - s0;
            if (CAUSAL && pfx) {
                P = __builtin_amdgcn_readfirstlane(pfx[seq]);
                prow0 = __builtin_amdgcn_readfirstlane(pfx[n_seq + seq]);
                T += P;
            }
        } else { row0 = (int64_t)seq * T_fixed; T = T_fixed; }
        if (T > max_T) T = max_T;
    }
    // packed row of key / position t
    __device__ __forceinline__ int64_t key_row(int t) const { return t < P ? prow0 + t : row0 + (t - P); }
    // key tiles (of NT) a query block sees whose last query stands at position qmax
    __device__ static __forceinline__ int nt_q(int qmax, int NT) {
        const int nt_c = (qmax >> 4) + 1;
        return CAUSAL ? (nt_c < NT ? nt_c : NT) : NT;
    }
    // the query at position qpos does not see `key`: its accumulator initialiser is -inf
    __device__ static __forceinline__ bool hidden(int key, int qpos) { return CAUSAL && key > qpos; }
};
// Fill two images with `T` rows of 64 16-bit values each, taken from qkv-like rows (zero beyond T): image a [rows_a][ATT_VROW],
// image b [rows_b][ATT_VROW] or (SWZ_B) [rows_b][ATT_KROW, swizzled].  ALL loads of both images are issued before the first LDS
// write and none sits behind a condition (row index clamped, zeros selected at the write), so a workgroup pays one memory
// latency for its operands: a load, a wait and an LDS write per 16-byte piece and loop trip paid eighteen in series.
template <int MAXROWS, bool SWZ_B = false, int NTHR = 256>
__device__ __forceinline__ void fill_two_images(char* lds_a, const uint16_t* __restrict__ src_a, int64_t ld_a, int col_a, int rows_a,
                                                char* lds_b, const uint16_t* __restrict__ src_b, int64_t ld_b, int col_b, int rows_b,
                                                int64_t row0, int T, int tid) {
    constexpr int NIT = (MAXROWS * 8 + NTHR - 1) / NTHR;
    u32x4_t va[NIT], vb[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int idx = tid + i * NTHR, r = idx >> 3, c = idx & 7;
        const int rc = r < T ? r : T - 1;
        va[i] = __builtin_nontemporal_load((const u32x4_t*)(src_a + (row0 + rc) * ld_a + col_a + c * 8));
        vb[i] = __builtin_nontemporal_load((const u32x4_t*)(src_b + (row0 + rc) * ld_b + col_b + c * 8));
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int idx = tid + i * NTHR, r = idx >> 3, c = idx & 7;
        const u32x4_t z = u32x4_t{0u, 0u, 0u, 0u};
        if (r < rows_a) *(u32x4_t*)(lds_a + r * ATT_VROW + (c << 4)) = r < T ? va[i] : z;
        if (r < rows_b) {
            if (SWZ_B) *(u32x4_t*)(lds_b + r * ATT_KROW + swz_chunk(c, r)) = r < T ? vb[i] : z;
            else *(u32x4_t*)(lds_b + r * ATT_VROW + (c << 4)) = r < T ? vb[i] : z;
        }
    }
}
