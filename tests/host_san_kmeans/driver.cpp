// Host-only sanitizer driver of the k-means entry points (tests/test_kmeans_host.py), built by tests/host_san_build.py
// under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device" blocks are exactly sized host blocks).  Walks every refusal of
// tvc_kmeans_assign / tvc_kmeans_update (no bank, R = 0, K out of range, NULL buffers), a valid call on an fp32 and on a
// bf16 slot, workspace growth from a small to a larger K, and a leak-free tvc_destroy.
#include "driver_common.hpp"

#include <vector>

int main() {
    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the bank calls need none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int R = 1000, D = 128, Kmax = 600;
    float* rows32 = (float*)buf((size_t)R * D, 4);
    uint16_t* rows16 = (uint16_t*)buf((size_t)R * D, 2);
    float* cin = (float*)buf((size_t)Kmax * D, 4); float* cout = (float*)buf((size_t)Kmax * D, 4);
    int32_t* labels = (int32_t*)buf(R, 4); float* score = (float*)buf(R, 4); float* dist2 = (float*)buf(R, 4);
    int32_t* counts = (int32_t*)buf(Kmax, 4); int32_t* offsets = (int32_t*)buf(Kmax + 1, 4); int32_t* order = (int32_t*)buf(R, 4);

    CHECK(tvc_kmeans_assign(nullptr, cin, 4, labels, score, dist2, nullptr) == TVC_E_INVALID);
    CHECK(tvc_kmeans_update(nullptr, labels, cin, 4, cout, counts, offsets, order, nullptr) == TVC_E_INVALID);
    // ---- no bank in the slot, then a bank of no rows: TVC_E_STATE, with a message
    CHECK(tvc_kmeans_assign(h, cin, 4, labels, score, dist2, nullptr) == TVC_E_STATE && strlen(tvc_last_error(h)) > 0);
    CHECK(tvc_kmeans_update(h, labels, cin, 4, cout, counts, offsets, order, nullptr) == TVC_E_STATE);
    OK(tvc_bank_set(h, rows32, 0, D, TVC_DTYPE_F32, nullptr));
    CHECK(tvc_kmeans_assign(h, cin, 4, labels, score, dist2, nullptr) == TVC_E_STATE);
    CHECK(tvc_kmeans_update(h, labels, cin, 4, cout, counts, offsets, order, nullptr) == TVC_E_STATE);
    OK(tvc_bank_set(h, nullptr, 0, D, TVC_DTYPE_BF16, nullptr));
    CHECK(tvc_kmeans_assign(h, cin, 1, labels, score, dist2, nullptr) == TVC_E_STATE);
    const uint64_t ws0 = tvc_workspace_bytes(h);                             // a refusal allocates nothing

    for (int dtype = 0; dtype < 2; ++dtype) {
        // ---- an fp32 slot (planes owned by the handle), then a bf16 slot (used in place) under another slot number
        OK(tvc_bank_select(h, dtype));
        OK(tvc_bank_set(h, dtype == 0 ? (const void*)rows32 : (const void*)rows16, R, D, dtype == 0 ? TVC_DTYPE_F32 : TVC_DTYPE_BF16, nullptr));
        // K out of range
        CHECK(tvc_kmeans_assign(h, cin, 0, labels, score, dist2, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_assign(h, cin, -3, labels, score, dist2, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_assign(h, cin, R + 1, labels, score, dist2, nullptr) == TVC_E_INVALID && strlen(tvc_last_error(h)) > 0);
        CHECK(tvc_kmeans_assign(h, cin, 65537, labels, score, dist2, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, labels, cin, 0, cout, counts, offsets, order, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, labels, cin, R + 1, cout, counts, offsets, order, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, labels, cin, 65537, cout, counts, offsets, order, nullptr) == TVC_E_INVALID);
        // NULL required buffers
        CHECK(tvc_kmeans_assign(h, nullptr, 4, labels, score, dist2, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_assign(h, cin, 4, nullptr, score, dist2, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, nullptr, cin, 4, cout, counts, offsets, order, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, labels, nullptr, 4, cout, counts, offsets, order, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, labels, cin, 4, nullptr, counts, offsets, order, nullptr) == TVC_E_INVALID);
        CHECK(tvc_kmeans_update(h, labels, cin, 4, cout, nullptr, offsets, order, nullptr) == TVC_E_INVALID);
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) == ws0);
        // ---- valid calls: optional outputs present and absent; then a larger K grows the workspaces
        OK(tvc_kmeans_assign(h, cin, 4, labels, score, dist2, nullptr));
        OK(tvc_kmeans_assign(h, cin, 4, labels, nullptr, nullptr, nullptr));
        OK(tvc_kmeans_update(h, labels, cin, 4, cout, counts, offsets, order, nullptr));
        OK(tvc_kmeans_update(h, labels, cin, 4, cout, counts, nullptr, nullptr, nullptr));
        const uint64_t small = tvc_workspace_bytes(h);
        OK(tvc_kmeans_assign(h, cin, Kmax, labels, score, dist2, nullptr));
        OK(tvc_kmeans_update(h, labels, cin, Kmax, cout, counts, nullptr, nullptr, nullptr));
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) > small);
        OK(tvc_kmeans_assign(h, cin, 1, labels, score, dist2, nullptr));     // back to a small K: the blocks stay
        OK(tvc_kmeans_assign(h, cin, R, labels, nullptr, dist2, nullptr));   // K = R
        OK(tvc_kmeans_update(h, labels, cin, R <= Kmax ? R : Kmax, cout, counts, offsets, order, nullptr));
    }
    // the fp32 slot still answers after the bf16 slot was used; a released slot refuses again
    OK(tvc_bank_select(h, 0));
    OK(tvc_kmeans_assign(h, cin, 8, labels, score, dist2, nullptr));
    OK(tvc_bank_set(h, nullptr, 0, 64, TVC_DTYPE_BF16, nullptr));
    CHECK(tvc_kmeans_assign(h, cin, 8, labels, score, dist2, nullptr) == TVC_E_STATE);
    // the profiling bracket counts the assign as bank work
    OK(tvc_bank_select(h, 1));
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t launches[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h)); OK(tvc_kmeans_assign(h, cin, 8, labels, score, dist2, nullptr)); OK(tvc_profile_end(h, ms, work, launches, big));
    CHECK(launches[TVC_PROF_BANK] == 1);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_KMEANS_OK\n");
    return 0;
}
