// Shared device helpers for the TVC HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

#define TVC_WAVE 64

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t h) {
    return __uint_as_float(((uint32_t)h) << 16);
}
// round-to-nearest-even through the compiler's cast (v_cvt_pk_bf16_f32; keeps NaN a NaN)
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    bf16x2_t v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
}

// ---- the hi | lo split of the split-bf16 kernels: x = hi + lo to ~2^-17 relative, hi = bf16(x), lo = bf16(x - hi)
__device__ __forceinline__ void split2(float x, float& hi, float& lo) {
    hi = bf16_bits_to_f32(f32_to_bf16_bits(x));
    lo = x - hi;                                 // exact in fp32; rounded to bf16 when packed
}
// 8 consecutive fp32 -> one 16-byte hi piece + one 16-byte lo piece
__device__ __forceinline__ void split8(const f32x4_t a, const f32x4_t b, u32x4_t& hi, u32x4_t& lo) {
    float h[8], l[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { split2(a[e], h[e], l[e]); split2(b[e], h[4 + e], l[4 + e]); }
#pragma unroll
    for (int e = 0; e < 4; ++e) { hi[e] = pack_bf16x2(h[2 * e], h[2 * e + 1]); lo[e] = pack_bf16x2(l[2 * e], l[2 * e + 1]); }
}

// IEEE fp16 (TVC_OPT_TOWER_PRECISION = 3).  The casts round to nearest even (v_cvt_pk_f16_f32) and overflow to +-inf;
// the round-toward-zero packer (which also saturates at 65504) is deliberately not used.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;

__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) {
    _Float16 v = (_Float16)f;
    return __builtin_bit_cast(uint16_t, v);
}
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
    f16x2_t v;
    v[0] = (_Float16)lo;
    v[1] = (_Float16)hi;
    return __builtin_bit_cast(uint32_t, v);
}
// the two 16-bit values of a packed pair as fp32 (lo = element 0)
__device__ __forceinline__ float f16x2_lo(uint32_t w) { return (float)__builtin_bit_cast(f16x2_t, w)[0]; }
__device__ __forceinline__ float f16x2_hi(uint32_t w) { return (float)__builtin_bit_cast(f16x2_t, w)[1]; }

// The 16-bit operand format of the tower kernels, a compile-time parameter: bf16 (F16 = false) or IEEE fp16 (F16 = true).
// Same bytes per element, same LDS images and fragment layouts; only the MFMA and the conversions differ.
template <bool F16> struct Op16;
template <> struct Op16<false> {
    typedef bf16x8_t x8;
    static constexpr uint32_t ONE2 = 0x3f803f80u;           // two 1.0 values
    __device__ static __forceinline__ f32x4_t mfma(x8 a, x8 b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    __device__ static __forceinline__ uint32_t pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
    __device__ static __forceinline__ uint16_t from_f32(float f) { return f32_to_bf16_bits(f); }
    __device__ static __forceinline__ float lo(uint32_t w) { return __uint_as_float(w << 16); }
    __device__ static __forceinline__ float hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
};
template <> struct Op16<true> {
    typedef f16x8_t x8;
    static constexpr uint32_t ONE2 = 0x3c003c00u;
    __device__ static __forceinline__ f32x4_t mfma(x8 a, x8 b, f32x4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    __device__ static __forceinline__ uint32_t pack2(float lo, float hi) { return pack_f16x2(lo, hi); }
    __device__ static __forceinline__ uint16_t from_f32(float f) { return f32_to_f16_bits(f); }
    __device__ static __forceinline__ float lo(uint32_t w) { return f16x2_lo(w); }
    __device__ static __forceinline__ float hi(uint32_t w) { return f16x2_hi(w); }
};

// All-lane sum over groups of W lanes (float, int, double): an xor butterfly, distances W / 2 ... 1.  The distances are the
// order of the floating-point additions, so they are part of every result's bits; every lane of a group ends with the same bits.
template <int W, class T>
__device__ __forceinline__ T lanes_sum(T v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// wave-level all-lane sum / max / min over 64 lanes (distances 32 ... 1)
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return lanes_sum<64>(v); }
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
// the inclusive prefix sum of v over the wave's lanes 0 .. lane (int, long long); lane 63 holds the wave's total
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// f(b) for every set bit b of x, in ascending order
template <class F>
__device__ __forceinline__ void for_each_set_bit(uint32_t x, F&& f) {
    while (x) {
        const int b = __ffs(x) - 1;
        x &= x - 1;
        f(b);
    }
}

// (v desc, idx asc): the order of the bank search's candidates and of k-means' centres; false whenever v is NaN
__device__ __forceinline__ bool cand_better(float v, int idx, float ov, int oidx) {
    return (v > ov) || (v == ov && idx < oidx);
}

// Eight elements of a stored bank row as fp32: 16 bytes of the hi plane at br, plus the lo plane's at br + D (planes > 1: the
// hi | lo split of an fp32 bank); a one-plane slot adds a zero lo.  x + 0.0f differs from x only for x = -0.0f, and the users
// square x (kmeans_rownorm_kernel) or add it to a sum that starts at +0.0f and so is never -0.0f (kmeans_centroid_kernel): the
// bits of skipping the add.  (bank_select_kernel's re-scoring skips it, in its own loop: EXPERIMENTS.md has the registers.)
__device__ __forceinline__ void bank_row8(const uint16_t* br, int D, int planes, float (&x)[8]) {
    const u32x4_t h = *(const u32x4_t*)br;
    u32x4_t l = u32x4_t{0u, 0u, 0u, 0u};
    if (planes > 1) l = *(const u32x4_t*)(br + D);
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = Op16<false>::lo(h[e]) + Op16<false>::lo(l[e]); x[2 * e + 1] = Op16<false>::hi(h[e]) + Op16<false>::hi(l[e]); }
}

// 16-byte async global->LDS copy (global_load_lds_dwordx4).  `lds_wave_base`
// must be wave-uniform: the hardware writes lane L at lds_wave_base + 16*L.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)gsrc,
        (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Same copy issued from inline asm: scalar 64-bit base + per-lane 32-bit byte offset,
// LDS destination byte address in M0 (saved / restored: M0 is compiler-reserved).
// hipcc does not count this load in its own vmcnt bookkeeping, so (unlike the builtin)
// it never drains the queue before a ds_read that "may alias" a pending LDS-DMA:
// ALL ordering of these loads is by the caller's explicit s_waitcnt vmcnt(N) + barrier.
// Compiler-counted waits for its own younger loads stay correct (they are only stricter).
__device__ __forceinline__ void glds16_asm(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}

// Four pieces of one ring stage in ONE asm statement: a single M0 save / restore, and the
// second destination of each operand is the first + `second` bytes.
__device__ __forceinline__ void glds16x4_asm(const void* abase, uint32_t va0, uint32_t va1, uint32_t a_lds,
                                             const void* bbase, uint32_t vb0, uint32_t vb1, uint32_t b_lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\t"
                 "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %6, %4\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %7, %4\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(va0), "v"(va1), "s"(abase), "s"(bbase), "s"(a_lds), "v"(vb0), "v"(vb1), "s"(b_lds)
                 : "memory", "scc");
}

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)p);
}

// Bijective XCD-contiguous remap of a 1-D grid (8 XCDs, round-robin dispatch):
// workgroups that land on one XCD get a contiguous range of `lin`, so tiles
// sharing an operand panel share that XCD's L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
    const int xcd = bid & 7;
    const int q = nwg >> 3, r = nwg & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}
