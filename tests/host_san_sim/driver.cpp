// Host-only sanitizer driver of the similarity-metric entry points (tests/test_similarity_host.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly
// sized host blocks).  A stand-alone program: walks every refusal of tvc_sim_rows, tvc_sim_flat_rank, tvc_sim_flat and
// tvc_topk_overlap, the legal empty calls (B == 0, M == 0), the workspace sizing at n = 1, 4096, 4097 and 2^20 with a workspace
// one byte short and a misaligned one, accepted calls with exactly sized buffers, and a leak-free tvc_destroy (the calls keep
// nothing in the handle).
#include "driver_common.hpp"
#include "host_plan.hpp"

#include <vector>

int main() {
    // the plan the product and this build share
    const int64_t ns[] = {1, 4096, 4097, (int64_t)1 << 20};
    const int grids[] = {1, 1, 2, 256};
    for (int i = 0; i < 4; ++i) {
        const SimFlatPlan p = sim_flat_plan(ns[i]);
        CHECK(p.ok && p.grid == grids[i] && p.pow2 >= ns[i] && (p.pow2 & (p.pow2 - 1)) == 0 && (ns[i] == 1 || p.pow2 / 2 < ns[i]));
        CHECK(p.ws_bytes == 8 * (16 + 20 * (int64_t)grids[i]));
        CHECK(tvc_sim_flat_workspace(ns[i]) == (uint64_t)p.ws_bytes);
    }
    CHECK(!sim_flat_plan(0).ok && !sim_flat_plan(-3).ok && !sim_flat_plan(((int64_t)1 << 20) + 1).ok);
    CHECK(tvc_sim_flat_workspace(0) == 0 && tvc_sim_flat_workspace(-1) == 0 && tvc_sim_flat_workspace(((int64_t)1 << 20) + 1) == 0);
    CHECK(sim_row_threads(1) == 64 && sim_row_threads(256) == 64 && sim_row_threads(257) == 256 && sim_row_threads(TVC_SIM_MAX_D) == 256);
    // n (n - 1)^2 at the cap stays inside int64
    CHECK((long double)TVC_SIM_MAX_N * (TVC_SIM_MAX_N - 1) * (TVC_SIM_MAX_N - 1) < 9.2e18L);

    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the calls need none
    const uint64_t ws0 = tvc_workspace_bytes(h);
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };

    // ---- tvc_sim_rows
    const int B = 3, D = 65, ld = 70;
    float* x = (float*)buf((size_t)(B - 1) * ld + D, 4);                    // the last row ends at its D-th element
    float* y = (float*)buf((size_t)B * D, 4);
    double* out = (double*)buf((size_t)B * TVC_SIM_COLS, 8);
    int64_t* ints = (int64_t*)buf((size_t)B * TVC_SIM_INTS, 8);
    CHECK(tvc_sim_rows(nullptr, x, y, B, D, ld, D, TVC_SIM_KEY_F32, out, ints, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_sim_rows(h, x, y, -1, D, ld, D, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, 0, ld, D, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, TVC_SIM_MAX_D + 1, TVC_SIM_MAX_D + 1, TVC_SIM_MAX_D + 1, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, D, D - 1, D, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, D, ld, D - 1, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, D, ld, D, 2, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, D, ld, D, -1, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, nullptr, y, B, D, ld, D, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, nullptr, B, D, ld, D, TVC_SIM_KEY_F32, out, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, D, ld, D, TVC_SIM_KEY_F32, nullptr, ints, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    REFUSED(tvc_sim_rows(h, x, y, B, D, ld, D, TVC_SIM_KEY_F32, out, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_rows");
    OK(tvc_sim_rows(h, x, y, B, D, ld, D, TVC_SIM_KEY_F32, out, ints, nullptr));
    OK(tvc_sim_rows(h, x, y, B, D, ld, D, TVC_SIM_KEY_I32, out, ints, nullptr));
    OK(tvc_sim_rows(h, x, y, 1, 1, 1, 1, TVC_SIM_KEY_F32, out, ints, nullptr));
    OK(tvc_sim_rows(h, nullptr, nullptr, 0, D, D, D, TVC_SIM_KEY_F32, nullptr, nullptr, nullptr));      // B == 0: legal, no buffers
    REFUSED(tvc_sim_rows(h, nullptr, nullptr, 0, 0, D, D, TVC_SIM_KEY_F32, nullptr, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_rows");   // but not a bad D

    // ---- the long form
    for (int i = 0; i < 4; ++i) {
        const int64_t n = ns[i];
        const uint64_t need = tvc_sim_flat_workspace(n);
        float* v = (float*)dev((size_t)n * 4);
        float* s = (float*)dev((size_t)n * 4);
        int32_t* cx = (int32_t*)dev((size_t)n * 4);
        int32_t* cy = (int32_t*)dev((size_t)n * 4);
        int64_t* nan = (int64_t*)dev(8);
        char* ws = (char*)dev(need + 8);
        OK(tvc_sim_flat_rank(h, v, s, n, cx, nan, nullptr));
        OK(tvc_sim_flat_rank(h, s, v, n, cy, nullptr, nullptr));                                  // the NaN count is optional
        OK(tvc_sim_flat(h, v, s, cx, cy, n, out, ints, ws, need, nullptr));
        REFUSED(tvc_sim_flat(h, v, s, cx, cy, n, out, ints, ws, need - 1, nullptr), TVC_E_INVALID, "tvc_sim_flat");      // too small a workspace
        REFUSED(tvc_sim_flat(h, v, s, cx, cy, n, out, ints, ws + 4, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");      // misaligned
        REFUSED(tvc_sim_flat(h, v, s, cx, cy, n, out, ints, nullptr, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, s, cx, cy, n, out, ints, ws, 0, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        (void)hipFree(v); (void)hipFree(s); (void)hipFree(cx); (void)hipFree(cy); (void)hipFree(nan); (void)hipFree(ws);
    }
    {
        float* v = (float*)buf(8, 4);
        int32_t* c = (int32_t*)buf(8, 4);
        char* ws = (char*)buf(tvc_sim_flat_workspace(8), 1);
        const uint64_t need = tvc_sim_flat_workspace(8);
        CHECK(tvc_sim_flat_rank(nullptr, v, v, 8, c, nullptr, nullptr) == TVC_E_INVALID);
        CHECK(tvc_sim_flat(nullptr, v, v, c, c, 8, out, ints, ws, need, nullptr) == TVC_E_INVALID);
        REFUSED(tvc_sim_flat_rank(h, v, v, 0, c, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_flat_rank");
        REFUSED(tvc_sim_flat_rank(h, v, v, -8, c, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_flat_rank");
        REFUSED(tvc_sim_flat_rank(h, v, v, (int64_t)TVC_SIM_MAX_N + 1, c, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_flat_rank");
        REFUSED(tvc_sim_flat_rank(h, nullptr, v, 8, c, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_flat_rank");
        REFUSED(tvc_sim_flat_rank(h, v, nullptr, 8, c, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_flat_rank");
        REFUSED(tvc_sim_flat_rank(h, v, v, 8, nullptr, nullptr, nullptr), TVC_E_INVALID, "tvc_sim_flat_rank");
        REFUSED(tvc_sim_flat(h, v, v, c, c, 0, out, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, v, c, c, (int64_t)TVC_SIM_MAX_N + 1, out, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, nullptr, v, c, c, 8, out, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, nullptr, c, c, 8, out, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, v, nullptr, c, 8, out, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, v, c, nullptr, 8, out, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, v, c, c, 8, nullptr, ints, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
        REFUSED(tvc_sim_flat(h, v, v, c, c, 8, out, nullptr, ws, need, nullptr), TVC_E_INVALID, "tvc_sim_flat");
    }

    // ---- tvc_topk_overlap
    const int M = 5, La = 7, Lb = 3;
    int32_t* a = (int32_t*)buf((size_t)M * La, 4);
    int32_t* b = (int32_t*)buf((size_t)M * Lb, 4);
    int32_t* count = (int32_t*)buf(M, 4);
    CHECK(tvc_topk_overlap(nullptr, a, b, M, La, Lb, 4, count, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_topk_overlap(h, a, b, -1, La, Lb, 4, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, a, b, M, -1, Lb, 4, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, a, b, M, La, -1, 4, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, a, b, M, La, Lb, 0, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, a, b, M, La, Lb, TVC_TOPK_OVERLAP_MAX_K + 1, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, nullptr, b, M, La, Lb, 4, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, a, nullptr, M, La, Lb, 4, count, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    REFUSED(tvc_topk_overlap(h, a, b, M, La, Lb, 4, nullptr, nullptr), TVC_E_INVALID, "tvc_topk_overlap");
    for (int k : {1, 3, 4, 64, 65, 1000, TVC_TOPK_OVERLAP_MAX_K}) OK(tvc_topk_overlap(h, a, b, M, La, Lb, k, count, nullptr));
    OK(tvc_topk_overlap(h, nullptr, nullptr, 0, La, Lb, 4, nullptr, nullptr));                     // M == 0: legal, no buffers

    CHECK(tvc_workspace_bytes(h) == ws0);                                   // no call keeps anything in the handle
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every device block was released
    printf("HOST_SAN_SIM_OK\n");
    return 0;
}
