// The one place a kernel is started, and the grids of the common kernel shapes (included by the .hip files only;
// kernels.hpp and handle.hpp stay free of it).  The third shape's grid, wave_stride_grid of a wave-per-row grid-stride
// kernel, is host_plan.hpp's: the host-only builds plan with it too.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <type_traits>
#include "host_plan.hpp" // wave_stride_grid
#include "rows.hpp"      // ROWS_PER_BLOCK

static_assert(ROWS_PER_BLOCK == 4, "wave_stride_grid (host_plan.hpp) gives four rows to a workgroup");

// Starts Kernel and returns hipGetLastError().  MaxLds > 0: the kernel takes more than 64 KiB of dynamic LDS, so its first
// launch registers MaxLds bytes with the runtime (once per kernel, thread-safe: the Python lock is per engine, two engines
// may first-launch from two threads); a failed registration or lds > MaxLds is returned without launching.
template <auto Kernel, size_t MaxLds = 0, class... Args>
hipError_t launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if constexpr (MaxLds > 0) {
        static std::once_flag once;
        static hipError_t attr = hipSuccess;
        std::call_once(once, [] {
            attr = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MaxLds);
        });
        if (attr != hipSuccess) return attr;
        if (lds > MaxLds) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}

// Runtime value -> template argument: calls f(std::integral_constant<.., V>{}) for the V of Vs that equals v and returns its
// result; hipErrorInvalidValue when v is none of them.  Only the listed values are instantiated (a left fold: in list order).
template <auto... Vs, class T, class F>
hipError_t dispatch(T v, F&& f) {
    hipError_t st = hipErrorInvalidValue;
    (void)(... || (v == Vs && ((st = f(std::integral_constant<decltype(Vs), Vs>{})), true)));
    return st;
}

// Grid of a wave-per-row kernel: ROWS_PER_BLOCK rows per 256-thread workgroup.
inline dim3 row_grid(int64_t rows) { return dim3((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)); }
// Grid of a grid-stride kernel over `total` items on 256 threads, at most `cap` workgroups (each kernel keeps its own cap).
inline dim3 stride_grid(int64_t total, int64_t cap) {
    const int64_t g = (total + 255) / 256;
    return dim3((unsigned)(g < cap ? g : cap));
}
