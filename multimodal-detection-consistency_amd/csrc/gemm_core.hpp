// bf16 MFMA GEMM core for gfx950:  acc[i, j] = sum_k A[i, k] * B[j, k]
//
//   A  bf16 [I, lda]   "row operand": weights (out-features) or bank rows
//   B  bf16 [J, ldb]   "column operand": tokens or query rows
//
// Both operands are K-contiguous (the nn.Linear weight layout and the natural
// layout of activations / bank rows), so both are staged with the same 16-byte
// global_load_lds pieces.  Workgroup tile 256 (I) x 256 (J) x 64 (K), 8 waves
// as 2 (I) x 4 (J); each wave owns 128 x 64 = 8 x 4 MFMA 16x16x32 tiles
// (128 fp32 accumulators per lane).  MFMA rows = I so that a lane holds 4
// consecutive out-features of one token: the epilogue stores 8-byte (bf16) or
// 16-byte (fp32) pieces of the token-major output.
//
// LDS: 2 buffers x (A tile 32 KiB + B tile 32 KiB) = 128 KiB, tiles are
// [256 rows][64 k] bf16 with 128-byte rows.  global_load_lds writes a wave's
// 64 x 16 B linearly (8 rows), so the XOR swizzle that makes the ds_read_b128
// fragment reads conflict-free is applied to the per-lane SOURCE address and
// to the read address (16-byte chunk c of row r lives at chunk c ^ ((r>>1)&7)).
//
// K may consist of several "planes" (split-bf16 operands for fp32-grade
// cosines): plane p reads A columns a_plane_off[p] + k and B columns
// b_plane_off[p] + k, all accumulated into the same tile.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

#define GEMM_BM 256          // I rows per workgroup
#define GEMM_BN 256          // J rows per workgroup
#define GEMM_BK 64
#define GEMM_THREADS 512
#define GEMM_MAX_PLANES 9
#define GEMM_TILE_BYTES (256 * 64 * 2)            // 32 KiB
#define GEMM_LDS_BYTES (4 * GEMM_TILE_BYTES)      // 128 KiB

struct GemmOperands {
    const uint16_t* A;
    const uint16_t* B;
    int64_t lda, ldb;          // elements
    int I, J;                  // valid rows of A / B (loads clamp to the last row)
    int ksteps_per_plane;      // K / 64
    int planes;                // 1..GEMM_MAX_PLANES (2-3: split-bf16 operands; 9: the taps of a 3x3 convolution)
    int a_plane_off[GEMM_MAX_PLANES];
    int b_plane_off[GEMM_MAX_PLANES];
};

// the operand half of a host-side launch (kernels.hpp) as the kernels take it
inline GemmOperands gemm_operands(const GemmLaunch& L) {
    GemmOperands g;
    g.A = L.A; g.B = L.B; g.lda = L.lda; g.ldb = L.ldb; g.I = L.I; g.J = L.J;
    g.ksteps_per_plane = L.K / GEMM_BK;
    g.planes = L.planes;
    for (int p = 0; p < GEMM_MAX_PLANES; ++p) { g.a_plane_off[p] = L.a_plane_off[p]; g.b_plane_off[p] = L.b_plane_off[p]; }
    return g;
}

// The operands of a pass over a bank slot.  The plane order is part of the contract: it is the order in which a tile's fp32
// products are added, so reordering two planes changes result bits (and nothing else).
// slot_operands: X rows of (hi | lo) planes at pitch 2 * D on A (the MFMA row dimension), the slot's rows on B (the lane
// dimension).  bf16 slot: xhi.b + xlo.b; fp32 slot: xhi.bhi + xhi.blo + xlo.bhi (the lo.lo term is below fp32).
inline GemmOperands slot_operands(const uint16_t* xplanes, int X, const BankRows& bank) {
    GemmOperands g;
    g.A = xplanes; g.lda = 2 * (int64_t)bank.D; g.I = X;
    g.B = bank.p; g.ldb = bank.ld; g.J = (int)bank.R;
    g.ksteps_per_plane = bank.D / GEMM_BK;
    for (int p = 0; p < GEMM_MAX_PLANES; ++p) { g.a_plane_off[p] = 0; g.b_plane_off[p] = 0; }
    if (bank.planes == 2) {
        g.planes = 3;
        g.b_plane_off[1] = bank.D;
        g.a_plane_off[2] = bank.D;
    } else {
        g.planes = 2;
        g.a_plane_off[1] = bank.D;
    }
    return g;
}
// slot_self_operands: the slot's rows on both sides.  bf16 slot: b.b; fp32 slot: hi.hi + hi.lo + lo.hi + lo.lo
inline GemmOperands slot_self_operands(const BankRows& bank) {
    GemmOperands g;
    g.A = bank.p; g.lda = bank.ld; g.I = (int)bank.R;
    g.B = bank.p; g.ldb = bank.ld; g.J = (int)bank.R;
    g.ksteps_per_plane = bank.D / GEMM_BK;
    for (int p = 0; p < GEMM_MAX_PLANES; ++p) { g.a_plane_off[p] = 0; g.b_plane_off[p] = 0; }
    g.planes = 1;
    if (bank.planes == 2) {
        g.planes = 4;
        g.b_plane_off[1] = bank.D;
        g.a_plane_off[2] = bank.D;
        g.a_plane_off[3] = bank.D; g.b_plane_off[3] = bank.D;
    }
    return g;
}

// The accumulators of a workgroup tile: wave w = (w >> 2, w & 3) of the 2 x 4 waves owns 128 x 64 of it as 8 x 4 MFMA blocks
// (m, n); in a block the 16 lanes `lane & 15` hold 16 consecutive columns and `lane >> 4` picks a group of four rows, whose
// row r is element r of acc[m][n].  In a tile whose first row / column is i0 / j0 (0: tile-local), gemm_acc_row is the row of
// element r = 0 and gemm_acc_col the lane's column.
typedef f32x4_t gemm_acc_t[8][4];
__device__ __forceinline__ int gemm_acc_row(int i0, int wave, int lane, int m) { return i0 + (wave >> 2) * 128 + m * 16 + (lane >> 4) * 4; }
__device__ __forceinline__ int gemm_acc_col(int j0, int wave, int lane, int n) { return j0 + (wave & 3) * 64 + n * 16 + (lane & 15); }

// Stage one [256][64] bf16 tile: wave w copies rows w*32 .. w*32+31 with four
// 1-KiB LDS-DMA pieces (8 rows each).
__device__ __forceinline__ void gemm_stage_tile(const uint16_t* __restrict__ base, int64_t ld,
                                                int row0, int nrows, int koff,
                                                char* lds_tile, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wave * 32 + i * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        int gr = row0 + r;
        gr = gr < nrows ? gr : nrows - 1;
        const uint16_t* src = base + (int64_t)gr * ld + koff + c * 8;
        glds16(src, lds_tile + (wave * 32 + i * 8) * 128);
    }
}

// acc must be zero-initialised by the caller (or carry a running sum).
// [step_begin, step_end): range of 64-deep K steps (over all planes) to multiply; the default is
// the whole K (split-K partial tiles pass a sub-range).  F16: the operands are IEEE fp16 (common.hpp: Op16).
template <bool F16 = false>
__device__ __forceinline__ void gemm_mainloop(gemm_acc_t& acc, const GemmOperands& g,
                                              int i0, int j0, char* smem, int step_begin = 0, int step_end = -1) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int nk = (step_end < 0 ? g.planes * g.ksteps_per_plane : step_end) - step_begin;

    // lane-constant swizzled chunk offsets for k-sub-steps 0 and 1
    const int sw0 = ((0 + (lane >> 4)) ^ ((lane >> 1) & 7)) * 16;
    const int sw1 = ((4 + (lane >> 4)) ^ ((lane >> 1) & 7)) * 16;
    const int a_row_off = (wm * 128 + (lane & 15)) * 128;
    const int b_row_off = (wn * 64 + (lane & 15)) * 128;

    int p = step_begin / g.ksteps_per_plane, kk = step_begin - p * g.ksteps_per_plane;   // plane / k-step-in-plane of the NEXT tile to stage
    auto stage_next = [&](int buf) {
        const int aoff = g.a_plane_off[p] + kk * GEMM_BK;
        const int boff = g.b_plane_off[p] + kk * GEMM_BK;
        char* t = smem + buf * (2 * GEMM_TILE_BYTES);
        gemm_stage_tile(g.A, g.lda, i0, g.I, aoff, t, wave, lane);
        gemm_stage_tile(g.B, g.ldb, j0, g.J, boff, t + GEMM_TILE_BYTES, wave, lane);
        if (++kk == g.ksteps_per_plane) { kk = 0; ++p; }
    };

    stage_next(0);
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt has landed and every wave is done reading the other buffer.
        // The LDS-DMA pieces are only ordered by the issuing wave's vmcnt: wait
        // explicitly (hipcc does not always emit it before the barrier).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage_next((kt + 1) & 1);
        const char* ta = smem + (kt & 1) * (2 * GEMM_TILE_BYTES);
        const char* tb = ta + GEMM_TILE_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int sw = s ? sw1 : sw0;
            typedef typename Op16<F16>::x8 x8;
            x8 a[8], b[4];
#pragma unroll
            for (int m = 0; m < 8; ++m)
                a[m] = *(const x8*)(ta + a_row_off + m * 2048 + sw);
#pragma unroll
            for (int n = 0; n < 4; ++n)
                b[n] = *(const x8*)(tb + b_row_off + n * 2048 + sw);
#pragma unroll
            for (int m = 0; m < 8; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[m][n] = Op16<F16>::mfma(a[m], b[n], acc[m][n]);
        }
    }
    // all waves must be done with the last buffer before a caller restages
    __syncthreads();
}

__device__ __forceinline__ void gemm_zero_acc(gemm_acc_t& acc) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}
