// Host-only sanitizer driver of the closest-pair entry point (tests/test_nearest_host.py), built by tests/host_san_build.py
// under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly sized
// host blocks).  A stand-alone program: walks every refusal of tvc_closest_pair (no handle, no bank, a bank of no rows, NULL
// outputs, more rows than the plan takes; D % 64 != 0 cannot get past tvc_bank_set, the entry point's own check stays as a
// guard), checks that a refusal allocates nothing, runs accepted calls on an fp32 and a bf16 slot, at R = 1 and around the tile
// boundary, the profiling bracket, and a leak-free tvc_destroy.
#include "driver_common.hpp"
#include "host_plan.hpp"

#include <vector>

int main() {
    // the plan the product and this build share
    const int64_t Rs[] = {1, 2, 255, 256, 257, 1000, 10000, 100000, NEAREST_MAX_ROWS};
    for (int64_t R : Rs) {
        const NearestPlan p = nearest_plan(R);
        CHECK(p.ok && (int64_t)p.tiles * 256 >= R && (int64_t)(p.tiles - 1) * 256 < R && p.rpad == (int64_t)p.tiles * 256);
        CHECK(p.rpad <= 0x7fffffffLL && p.tile_pairs == 0.5 * p.tiles * (p.tiles + 1.0));
    }
    CHECK(!nearest_plan(0).ok && !nearest_plan(-5).ok && !nearest_plan(NEAREST_MAX_ROWS + 1).ok);

    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the call needs none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int R = 1000, D = 128;
    float* rows32 = (float*)buf((size_t)R * D, 4);
    uint16_t* rows16 = (uint16_t*)buf((size_t)R * D, 2);
    int32_t* partner = (int32_t*)buf(R, 4);
    float* sim = (float*)buf(R, 4);
    int32_t* pair = (int32_t*)buf(2, 4);
    float* pair_sim = (float*)buf(1, 4);

    // ---- no handle, no bank, a bank of no rows
    CHECK(tvc_closest_pair(nullptr, partner, sim, pair, pair_sim, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
    OK(tvc_bank_set(h, rows32, 0, D, TVC_DTYPE_F32, nullptr));
    REFUSED(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
    OK(tvc_bank_set(h, rows16, 0, D, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
    OK(tvc_bank_set(h, nullptr, 0, D, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
    const uint64_t ws0 = tvc_workspace_bytes(h);
    for (int dtype = 0; dtype < 2; ++dtype) {
        OK(tvc_bank_select(h, dtype));
        OK(tvc_bank_set(h, dtype == 0 ? (const void*)rows32 : (const void*)rows16, R, D, dtype == 0 ? TVC_DTYPE_F32 : TVC_DTYPE_BF16, nullptr));
        REFUSED(tvc_closest_pair(h, nullptr, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
        REFUSED(tvc_closest_pair(h, partner, nullptr, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
        REFUSED(tvc_closest_pair(h, partner, sim, nullptr, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
        REFUSED(tvc_closest_pair(h, partner, sim, pair, nullptr, nullptr), TVC_E_INVALID, "tvc_closest_pair");
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) == ws0);                                 // a refusal allocates nothing
        OK(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr));
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) >= ws0 + (uint64_t)nearest_plan(R).rpad * 4);
    }
    // R = 1 is valid; the sizes around the tile boundary, with exactly sized outputs
    for (int r : {1, 2, 255, 256, 257}) {
        int32_t* p = (int32_t*)dev((size_t)r * 4);
        float* s = (float*)dev((size_t)r * 4);
        OK(tvc_bank_set(h, rows16, r, D, TVC_DTYPE_BF16, nullptr));
        OK(tvc_closest_pair(h, p, s, pair, pair_sim, nullptr));
        (void)hipFree(p); (void)hipFree(s);
    }
    // more rows than the plan takes (a bf16 slot is used in place: only its first rows exist here, nothing reads them)
    OK(tvc_bank_set(h, rows16, NEAREST_MAX_ROWS + 1, 64, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");
    OK(tvc_bank_set(h, nullptr, 0, 64, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr), TVC_E_INVALID, "tvc_closest_pair");       // a released slot refuses again

    // the profiling bracket counts the pass as bank work
    OK(tvc_bank_select(h, 0));
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t launches[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h)); OK(tvc_closest_pair(h, partner, sim, pair, pair_sim, nullptr)); OK(tvc_profile_end(h, ms, work, launches, big));
    CHECK(launches[TVC_PROF_BANK] == 1);
    // 4 tiles a side, 10 on and above the diagonal, four products of an fp32 slot
    CHECK(work[TVC_PROF_BANK] == 2.0 * 10 * 256 * 256 * D * 4);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_NEAREST_OK\n");
    return 0;
}
