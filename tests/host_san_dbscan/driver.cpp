// Host-only sanitizer driver of the radius-graph / DBSCAN entry points (tests/test_dbscan_host.py), built by
// tests/host_san_build.py under ASan / UBSan against tests/host_san's HIP stand-in (kernels are no-ops, "device"
// blocks are exactly sized host blocks).  Walks every refusal of tvc_radius_graph (no handle, no bank, R = 0, a bad eps, too
// many rows, NULL or misaligned buffers) and of tvc_dbscan_sweep / tvc_dbscan_finish (R and min_samples out of range, NULL
// buffers), checks that a refusal allocates nothing, runs accepted calls of each entry on an fp32 and a bf16 slot and at the
// sizes around the word and tile boundaries, the profiling bracket, and a leak-free tvc_destroy.
#include "driver_common.hpp"
#include "host_plan.hpp"

#include <cmath>
#include <vector>

int main() {
    // the plan the product and this build share
    const int64_t Rs[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 65536, 131071, 131072};
    for (int64_t R : Rs) {
        const RadiusPlan p = radius_plan(R);
        CHECK(p.ok && p.words % 2 == 0 && p.words * 32 >= R && p.words * 32 < R + 64 && p.tiles * 256 >= R && (p.tiles - 1) * 256 < R);
        CHECK(p.hpad == (int64_t)p.tiles * 256 && p.blocks32 == p.words && p.sym_grid_x * 8 >= p.blocks32 && p.adj_bytes == R * p.words * 4);
        CHECK(p.sym_grid_x >= 1 && p.blocks32 <= 65535 && p.adj_bytes <= ((int64_t)2 << 30));
    }
    CHECK(!radius_plan(0).ok && !radius_plan(-5).ok && !radius_plan(131073).ok);

    tvc_handle* h = nullptr;
    CHECK(tvc_create(nullptr, nullptr, nullptr, &h) == TVC_OK && h);       // a handle without towers: the calls need none
    std::vector<void*> keep;
    auto buf = [&](size_t elems, size_t es) { void* p = dev(elems * es); keep.push_back(p); return p; };
    const int R = 1000, D = 128;
    const int W = (int)radius_plan(R).words;
    float* rows32 = (float*)buf((size_t)R * D, 4);
    uint16_t* rows16 = (uint16_t*)buf((size_t)R * D, 2);
    uint32_t* adj = (uint32_t*)buf((size_t)R * W, 4);
    int32_t* degree = (int32_t*)buf(R, 4);
    int32_t* comp = (int32_t*)buf(R, 4);
    int32_t* changed = (int32_t*)buf(1, 4);
    int32_t* labels = (int32_t*)buf(R, 4);
    uint8_t* core = (uint8_t*)buf(R, 1);
    int32_t* ncl = (int32_t*)buf(1, 4);
    const char* RG = "tvc_radius_graph";
    const char* SW = "tvc_dbscan_sweep";
    const char* FI = "tvc_dbscan_finish";

    // ---- tvc_radius_graph: no handle, no bank, a bank of no rows
    CHECK(tvc_radius_graph(nullptr, 0.5f, adj, degree, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_radius_graph(h, 0.5f, adj, degree, nullptr), TVC_E_STATE, RG);
    OK(tvc_bank_set(h, rows32, 0, D, TVC_DTYPE_F32, nullptr));
    REFUSED(tvc_radius_graph(h, 0.5f, adj, degree, nullptr), TVC_E_STATE, RG);
    OK(tvc_bank_set(h, nullptr, 0, D, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_radius_graph(h, 0.5f, adj, degree, nullptr), TVC_E_STATE, RG);
    const uint64_t ws0 = tvc_workspace_bytes(h);
    for (int dtype = 0; dtype < 2; ++dtype) {
        OK(tvc_bank_select(h, dtype));
        OK(tvc_bank_set(h, dtype == 0 ? (const void*)rows32 : (const void*)rows16, R, D, dtype == 0 ? TVC_DTYPE_F32 : TVC_DTYPE_BF16, nullptr));
        REFUSED(tvc_radius_graph(h, 0.f, adj, degree, nullptr), TVC_E_INVALID, RG);
        REFUSED(tvc_radius_graph(h, -0.5f, adj, degree, nullptr), TVC_E_INVALID, RG);
        REFUSED(tvc_radius_graph(h, NAN, adj, degree, nullptr), TVC_E_INVALID, RG);
        REFUSED(tvc_radius_graph(h, INFINITY, adj, degree, nullptr), TVC_E_INVALID, RG);
        REFUSED(tvc_radius_graph(h, 0.5f, nullptr, degree, nullptr), TVC_E_INVALID, RG);
        REFUSED(tvc_radius_graph(h, 0.5f, adj, nullptr, nullptr), TVC_E_INVALID, RG);
        REFUSED(tvc_radius_graph(h, 0.5f, adj + 1, degree, nullptr), TVC_E_INVALID, RG);      // 4-byte aligned only
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) == ws0);                                 // a refusal allocates nothing
        OK(tvc_radius_graph(h, 0.5f, adj, degree, nullptr));
        OK(tvc_radius_graph(h, 1e-3f, adj, degree, nullptr));
        if (dtype == 0) CHECK(tvc_workspace_bytes(h) > ws0);
    }
    // the sizes around the word and tile boundaries (the workspaces shrink and grow with the padded half-norm vector)
    for (int r : {1, 2, 63, 64, 65, 255, 256, 257}) {
        uint32_t* a = (uint32_t*)dev((size_t)r * radius_plan(r).words * 4);
        int32_t* d = (int32_t*)dev((size_t)r * 4);
        OK(tvc_bank_set(h, rows16, r, D, TVC_DTYPE_BF16, nullptr));
        OK(tvc_radius_graph(h, 0.5f, a, d, nullptr));
        (void)hipFree(a); (void)hipFree(d);
    }
    // more rows than TVC_RADIUS_MAX_ROWS (a bf16 slot is used in place: only its first rows exist here, nothing reads them)
    OK(tvc_bank_set(h, rows16, (int64_t)TVC_RADIUS_MAX_ROWS + 1, 64, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_radius_graph(h, 0.5f, adj, degree, nullptr), TVC_E_INVALID, RG);
    OK(tvc_bank_set(h, nullptr, 0, 64, TVC_DTYPE_BF16, nullptr));
    REFUSED(tvc_radius_graph(h, 0.5f, adj, degree, nullptr), TVC_E_STATE, RG);      // a released slot refuses again

    // ---- tvc_dbscan_sweep / tvc_dbscan_finish: they read no bank slot
    const uint64_t ws1 = tvc_workspace_bytes(h);
    CHECK(tvc_dbscan_sweep(nullptr, adj, degree, R, 5, comp, changed, 1, nullptr) == TVC_E_INVALID);
    CHECK(tvc_dbscan_finish(nullptr, adj, degree, R, 5, comp, labels, core, ncl, nullptr) == TVC_E_INVALID);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, 0, 5, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, -1, 5, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, TVC_RADIUS_MAX_ROWS + 1, 5, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, R, 0, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, R, -2, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, nullptr, degree, R, 5, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, nullptr, R, 5, comp, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, R, 5, nullptr, changed, 1, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_sweep(h, adj, degree, R, 5, comp, nullptr, 0, nullptr), TVC_E_INVALID, SW);
    REFUSED(tvc_dbscan_finish(h, adj, degree, 0, 5, comp, labels, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, degree, TVC_RADIUS_MAX_ROWS + 1, 5, comp, labels, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, degree, R, 0, comp, labels, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, nullptr, degree, R, 5, comp, labels, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, nullptr, R, 5, comp, labels, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, degree, R, 5, nullptr, labels, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, degree, R, 5, comp, nullptr, core, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, degree, R, 5, comp, labels, nullptr, ncl, nullptr), TVC_E_INVALID, FI);
    REFUSED(tvc_dbscan_finish(h, adj, degree, R, 5, comp, labels, core, nullptr, nullptr), TVC_E_INVALID, FI);
    OK(tvc_dbscan_sweep(h, adj, degree, R, 5, comp, changed, 1, nullptr));
    OK(tvc_dbscan_sweep(h, adj, degree, R, 5, comp, changed, 0, nullptr));
    OK(tvc_dbscan_sweep(h, adj, degree, 1, 1, comp, changed, 1, nullptr));
    OK(tvc_dbscan_finish(h, adj, degree, R, 5, comp, labels, core, ncl, nullptr));
    OK(tvc_dbscan_finish(h, adj, degree, 1, 1, comp, labels, core, ncl, nullptr));
    CHECK(tvc_workspace_bytes(h) == ws1);                           // neither component call owns a workspace

    // the profiling bracket counts the graph as bank work
    OK(tvc_bank_select(h, 0));
    double ms[TVC_PROF_NCAT], work[TVC_PROF_NCAT], big[3]; int64_t launches[TVC_PROF_NCAT];
    OK(tvc_profile_begin(h)); OK(tvc_radius_graph(h, 0.5f, adj, degree, nullptr)); OK(tvc_profile_end(h, ms, work, launches, big));
    CHECK(launches[TVC_PROF_BANK] == 1);
    // 4 tiles a side, 10 on and above the diagonal, four products of an fp32 slot
    CHECK(work[TVC_PROF_BANK] == 2.0 * 10 * 256 * 256 * D * 4);
    tvc_destroy(h);
    for (void* p : keep) (void)hipFree(p);
    CHECK(hip_stub_blocks().empty());                               // every handle-owned device block was released
    printf("HOST_SAN_DBSCAN_OK\n");
    return 0;
}
